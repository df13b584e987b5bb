// pgx_batch_locate.hip -- pgx_batch_locate (pgx_mem_locate_kernels.hip): the occurrences of the last run's MEMs, on the device, and its two results.
#include <string>

#include "pgx_batch_internal.hpp"

// values one pass of the intermediate buffer may hold: PGX_LOCATE_BUDGET_MB (fractions allowed), default a quarter of free device memory
static uint64_t locate_budget_values() {
    uint64_t bytes = 0;
    if (const char *e = std::getenv("PGX_LOCATE_BUDGET_MB")) {
        const double mb = std::strtod(e, nullptr);
        if (mb > 0) bytes = (uint64_t)(mb * 1048576.0);
    }
    if (!bytes) {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); mem_free = 1ull << 30; }
        bytes = mem_free / 4;
    }
    return std::max<uint64_t>(bytes / 8, 1);
}

// PGX_LOCATE_SETS=0 (read per call): PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE by the segmented sort even where the sequence sets would serve it
static bool locate_sets_enabled() {
    const char *e = std::getenv("PGX_LOCATE_SETS");
    return !(e && e[0] == '0' && e[1] == 0);
}

extern "C" pgx_status pgx_batch_locate(pgx_batch *b, uint32_t flags, uint64_t max_occ, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_locate");
    if ((flags & PGX_LOCATE_SEQ_SETS) && (flags & (PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE))) // (a contradiction in the call itself: said with or without a device)
        throw Error(PGX_ERR_ARG, "pgx_batch_locate: PGX_LOCATE_SEQ_SETS goes with PGX_LOCATE_CHAINS alone");
    checked_device_count();
    if (!b) throw Error(PGX_ERR_ARG, "pgx_batch_locate: null batch");
    if (flags & ~(PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE | PGX_LOCATE_CHAINS | PGX_LOCATE_SEQ_SETS)) throw Error(PGX_ERR_ARG, "pgx_batch_locate: unknown flag");
    if (!b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_locate: batch has not been run");
    LocWork &w = b->lw;
    w.valid = false;
    locate_check_supported(b->h, "pgx_batch_locate");
    use_device(b->device);
    pgx_device_image *d = locate_image(b->h, b->device);
    hipStream_t s = batch_stream(b, stream);
    const uint64_t n = b->n_mems, bwt_n = d->loc.n;
    const bool sets_form = (flags & PGX_LOCATE_SEQ_SETS) != 0;
    const bool seq_ids = sets_form || (flags & PGX_LOCATE_SEQ_IDS) != 0, uniq = (flags & PGX_LOCATE_UNIQUE) != 0;
    // sequence sets: the result itself (PGX_LOCATE_SEQ_SETS), or what the sorted unique sequence ids are expanded from (routed) in place of the sort
    const uint64_t n_seq = b->h->meta.n_sequences();
    const uint64_t W = (n_seq + 63) / 64;
    const bool sets_fit = W >= 1 && W <= PGX_ML_SET_WORDS_MAX;
    if (sets_form && !sets_fit)
        throw Error(PGX_ERR_UNSUPPORTED, "pgx_batch_locate: PGX_LOCATE_SEQ_SETS serves at most " + std::to_string(64 * PGX_ML_SET_WORDS_MAX) + " sequences, the index has " +
                                             std::to_string(n_seq));
    const bool routed = !sets_form && seq_ids && uniq && sets_fit && locate_sets_enabled();
    const bool build_sets = sets_form || routed, sort_uniq = uniq && !routed;
    // the resident suffix array: the LCE image in text coordinates and its sequence starts (built from this very locate image's chains)
    const bool resident = !(flags & PGX_LOCATE_CHAINS) && d->lce_state == 1 && d->img.lce_sa && d->lce_seq_start.p && d->lce_n_seq && d->img.n == bwt_n;
    w.timer.begin(b->timed, s);
    // 1. plan: counts (cap, range checks), ranges, not-located total; value offsets
    //    ctr: [0] wave list [1] workgroup list [2] scratch total [3] unique values of a pass [4] not located [5] values [6..7] cut
    w.cnt.ensure((n ? n : 1) * 8); w.qs.ensure((n ? n : 1) * 8); w.qe.ensure((n ? n : 1) * 8); w.voff.ensure((n + 1) * 8); w.ctr.ensure(64);
    unsigned long long *ctr = w.ctr.as<unsigned long long>();
    HIPCHECK(hipMemsetAsync(w.ctr.p, 0, 64, s));
    if (n) {
        hipLaunchKernelGGL(pgx_ml_plan_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const pgx_mem *)b->mems.as<pgx_mem>(), n, bwt_n, max_occ,
                           w.cnt.as<uint64_t>(), w.qs.as<uint64_t>(), w.qe.as<uint64_t>(), ctr + 4);
        HIPCHECK(hipGetLastError());
    }
    scan_excl(1, w.cnt.p, n, 0, w.voff.as<uint64_t>(), w.scan_tmp, s, reinterpret_cast<uint64_t *>(ctr + 5));
    uint64_t tot[2];
    read_scalars(tot, ctr + 4, 16, s);
    const uint64_t n_not = tot[0], V = tot[1];
    const uint64_t *voff = w.voff.as<uint64_t>();
    // 2. passes over consecutive MEMs whose values fit the budget (one pass unless the batch exceeds it)
    const uint64_t budget = locate_budget_values();
    if (sets_form) { // the result: n x W words, cleared once; loc_offsets[m] = m * W
        w.vals.ensure((n ? n * W : 1) * 8); w.uoff.ensure((n + 1) * 8);
        if (n) HIPCHECK(hipMemsetAsync(w.vals.p, 0, n * W * 8, s));
        hipLaunchKernelGGL(pgx_ml_stride_kernel, dim3(grid_for(n + 1, 256)), dim3(256), 0, s, w.uoff.as<uint64_t>(), n + 1, W);
        HIPCHECK(hipGetLastError());
    } else if (!uniq) w.vals.ensure((V ? V : 1) * 8); // (the values are written in place: no intermediate buffer)
    else { w.ucount.ensure((n ? n : 1) * 8); w.uoff.ensure((n + 1) * 8); }
    // the values of a pass need a buffer unless they are written in place or go straight from the resident suffix array into the sets
    const bool value_buffer = sort_uniq || (build_sets && !resident);
    const uint64_t set_mems = std::max<uint64_t>(budget / (W ? W : 1), 1); // MEMs whose sets fit the budget (routed: the set array is intermediate too)
    uint64_t U = 0; // unique values of the passes so far
    for (uint64_t m0 = 0, o0 = 0; m0 < n;) {
        uint64_t m1 = n, o1 = V;
        const bool by_values = !(build_sets && resident) && V - o0 > budget;
        const uint64_t m_lim = routed && n - m0 > set_mems ? m0 + set_mems : n;
        if (by_values || m_lim < n) {
            hipLaunchKernelGGL(pgx_ml_cut_kernel, dim3(1), dim3(64), 0, s, voff, m_lim, m0, by_values ? budget : V, reinterpret_cast<uint64_t *>(ctr + 6));
            HIPCHECK(hipGetLastError());
            uint64_t c[2];
            read_scalars(c, ctr + 6, 16, s);
            m1 = c[0]; o1 = c[1];
        }
        const uint64_t np = m1 - m0, nv = o1 - o0;
        if (value_buffer) w.gbuf.ensure((nv ? nv : 1) * 8);
        uint64_t *dst = value_buffer ? w.gbuf.as<uint64_t>() : w.vals.as<uint64_t>() + o0; // value o of the batch goes to dst[o - o0]
        unsigned long long *sets = nullptr; // the pass's sets: MEM m at sets[(m - m0) * W ..)
        if (sets_form) sets = w.vals.as<unsigned long long>() + m0 * W;
        else if (routed) {
            w.sets.ensure(np * W * 8);
            sets = w.sets.as<unsigned long long>();
            HIPCHECK(hipMemsetAsync(sets, 0, np * W * 8, s));
        }
        if (nv && resident && build_sets) {
            hipLaunchKernelGGL(pgx_ml_sets_kernel, dim3(grid_for(nv, PGX_ML_SPAN)), dim3(256), 0, s, (const pgx_mem *)b->mems.as<pgx_mem>(), voff, m0, m1, o0, nv,
                               (const uint32_t *)d->img.lce_sa, bwt_n, (const uint64_t *)d->lce_seq_start.as<uint64_t>(), d->lce_n_seq, (uint32_t)W, sets);
            HIPCHECK(hipGetLastError());
        } else if (nv && resident) {
            hipLaunchKernelGGL(pgx_ml_gather_kernel, dim3(grid_for(nv, PGX_ML_SPAN)), dim3(256), 0, s, (const pgx_mem *)b->mems.as<pgx_mem>(), voff, m0, m1, o0, nv,
                               (const uint32_t *)d->img.lce_sa, bwt_n, (const uint64_t *)d->lce_seq_start.as<uint64_t>(), d->lce_n_seq, d->loc.max_length,
                               seq_ids ? 1 : 0, dst);
            HIPCHECK(hipGetLastError());
        } else if (nv) { // the sample chains of pgx_locate_batch, from the device ranges
            w.run0.ensure(np * 8); w.npieces.ensure(np * 8); w.poff.ensure((np + 1) * 8);
            const uint64_t *qs = w.qs.as<uint64_t>() + m0, *qe = w.qe.as<uint64_t>() + m0;
            hipLaunchKernelGGL(pgx_locate_plan_kernel, dim3(grid_for(np, 256)), dim3(256), 0, s, d->loc, qs, qe, np, w.run0.as<uint64_t>(), w.npieces.as<uint64_t>());
            HIPCHECK(hipGetLastError());
            scan_excl(1, w.npieces.p, np, 0, w.poff.as<uint64_t>(), w.scan_tmp, s);
            const uint64_t n_pieces = read_u64(w.poff.as<uint64_t>() + np, s);
            if (n_pieces) {
                hipLaunchKernelGGL(pgx_locate_walk_kernel, dim3(grid_for(n_pieces, 256)), dim3(256), 0, s, d->loc, qs, qe, np, (const uint64_t *)w.run0.as<uint64_t>(),
                                   (const uint64_t *)w.poff.as<uint64_t>(), n_pieces, voff + m0, o0, seq_ids ? 1 : 0, dst);
                HIPCHECK(hipGetLastError());
                if (build_sets) { // the pass's sequence ids -> bits
                    hipLaunchKernelGGL(pgx_ml_sets_ids_kernel, dim3(grid_for(nv, PGX_ML_SPAN)), dim3(256), 0, s, voff, m0, m1, o0, nv, (const uint64_t *)dst, (uint32_t)W,
                                       sets);
                    HIPCHECK(hipGetLastError());
                }
            }
        }
        if (routed) { // the sets as ascending ids behind the passes before: sorted and unique by construction
            uint32_t Wp = 1;
            while (Wp < W) Wp <<= 1;
            uint64_t *ucount = w.ucount.as<uint64_t>() + m0;
            w.uloc.ensure((np + 1) * 8);
            hipLaunchKernelGGL(pgx_ml_set_count_kernel, dim3(grid_for(np * Wp, 256)), dim3(256), 0, s, (const unsigned long long *)sets, np, (uint32_t)W, Wp, ucount);
            HIPCHECK(hipGetLastError());
            scan_excl(1, ucount, np, 0, w.uloc.as<uint64_t>(), w.scan_tmp, s, reinterpret_cast<uint64_t *>(ctr + 3));
            const uint64_t Up = read_u64(reinterpret_cast<const uint64_t *>(ctr + 3), s);
            w.vals.ensure_keep((U + Up ? U + Up : 1) * 8, U * 8); // (the stream is idle here: the read-back above synchronised it)
            if (Up) {
                hipLaunchKernelGGL(pgx_ml_set_expand_kernel, dim3(grid_for(np, 4)), dim3(256), 0, s, (const unsigned long long *)sets, np, (uint32_t)W,
                                   (const uint64_t *)w.uloc.as<uint64_t>(), w.vals.as<uint64_t>() + U);
                HIPCHECK(hipGetLastError());
            }
            U += Up;
        }
        if (sort_uniq) { // segmented sort-unique with the tag stage's kernels, size-class lists built on the device, then compaction behind the passes before
            w.seg.ensure((np + 1) * 8); w.lists.ensure(2 * np * 8); w.need.ensure(np * 8); w.soff.ensure((np + 1) * 8); w.uloc.ensure((np + 1) * 8);
            uint64_t *seg = w.seg.as<uint64_t>(), *wave_list = w.lists.as<uint64_t>(), *wg_list = wave_list + np, *ucount = w.ucount.as<uint64_t>() + m0;
            const uint64_t *cnt = w.cnt.as<uint64_t>() + m0;
            HIPCHECK(hipMemsetAsync(w.ctr.p, 0, 32, s));
            hipLaunchKernelGGL(pgx_ml_classify_kernel, dim3(grid_for(np + 1, 256)), dim3(256), 0, s, cnt, voff + m0, np, seg, wave_list, wg_list,
                               w.need.as<uint64_t>(), ucount, ctr);
            HIPCHECK(hipGetLastError());
            scan_excl(1, w.need.p, np, 0, w.soff.as<uint64_t>(), w.scan_tmp, s, reinterpret_cast<uint64_t *>(ctr + 2));
            uint64_t c[3];
            read_scalars(c, ctr, 24, s);
            const uint64_t n_wave = c[0], n_wg = c[1], S = c[2];
            if (n_wave)
                hipLaunchKernelGGL(pgx_tag_sort_unique_kernel<PgxTagDense>, dim3(grid_for(n_wave, 4)), dim3(256), 0, s, PgxTagDense{wave_list, cnt, seg}, n_wave,
                                   (const uint64_t *)nullptr, (const uint64_t *)nullptr, w.gbuf.as<uint64_t>(), ucount);
            if (n_wg) {
                w.scratch.ensure((S ? S : 1) * 8);
                HIPCHECK(hipFuncSetAttribute((const void *)pgx_tag_sort_large_kernel<PgxTagDense>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(PGX_SORT_WG_LDS_CAP * 8)));
                hipLaunchKernelGGL(pgx_tag_sort_large_kernel<PgxTagDense>, dim3(grid_for(n_wg, 1)), dim3(1024), (size_t)PGX_SORT_WG_LDS_CAP * 8, s, PgxTagDense{wg_list, cnt, seg},
                                   n_wg, (const uint64_t *)nullptr, (const uint64_t *)nullptr, w.gbuf.as<uint64_t>(), w.scratch.as<uint64_t>(),
                                   (const uint64_t *)w.soff.as<uint64_t>(), ucount);
            }
            HIPCHECK(hipGetLastError());
            scan_excl(1, ucount, np, 0, w.uloc.as<uint64_t>(), w.scan_tmp, s, reinterpret_cast<uint64_t *>(ctr + 3));
            const uint64_t Up = read_u64(reinterpret_cast<const uint64_t *>(ctr + 3), s);
            w.vals.ensure_keep((U + Up ? U + Up : 1) * 8, U * 8); // (the stream is idle here: the read-back above synchronised it)
            if (Up) {
                hipLaunchKernelGGL(pgx_tag_compact_kernel<PgxTagDense>, dim3(grid_for(np, 16)), dim3(256), 0, s, PgxTagDense{nullptr, nullptr, seg}, np,
                                   (const uint64_t *)nullptr, (const uint64_t *)nullptr, (const uint64_t *)ucount, (const uint64_t *)w.gbuf.as<uint64_t>(),
                                   (const uint64_t *)w.uloc.as<uint64_t>(), w.vals.as<uint64_t>() + U, ~0ull);
                HIPCHECK(hipGetLastError());
            }
            U += Up;
        }
        m0 = m1; o0 = o1;
    }
    if (uniq) scan_excl(1, w.ucount.p, n, 0, w.uoff.as<uint64_t>(), w.scan_tmp, s);
    w.vals.ensure(8);
    w.ms = w.timer.end(s);
    if (!b->timed) HIPCHECK(hipStreamSynchronize(s)); // (a timed call has waited in end())
    w.d_off = uniq || sets_form ? w.uoff.as<uint64_t>() : voff;
    w.n_mems = n;
    w.n_values = sets_form ? n * W : uniq ? U : V;
    w.n_not_located = n_not;
    w.flags = flags & (PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE | PGX_LOCATE_SEQ_SETS);
    w.set_words = build_sets ? (uint32_t)W : 0;
    w.resident = resident;
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void locations_header(const pgx_batch *b, pgx_locations *out) {
    const LocWork &w = b->lw;
    std::memset(out, 0, sizeof *out);
    out->n_mems = w.n_mems;
    out->n_values = w.n_values;
    out->n_not_located = w.n_not_located;
    out->flags = w.flags;
    out->resident = w.resident ? 1u : 0u;
    out->ms_locate = w.ms;
    out->set_words = w.set_words;
}

extern "C" pgx_status pgx_batch_device_locations(pgx_batch *b, pgx_locations *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->lw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_locations: batch has no locate result");
    locations_header(b, out);
    out->loc_offsets = b->lw.d_off;
    out->values = b->lw.vals.as<uint64_t>();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_locations(pgx_batch *b, pgx_locations *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->lw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_locations: batch has no locate result");
    use_device(b->device);
    LocWork &w = b->lw;
    w.h_off.ensure((w.n_mems + 1) * 8);
    w.h_vals.ensure((w.n_values ? w.n_values : 1) * 8);
    HIPCHECK(hipMemcpyAsync(w.h_off.p, w.d_off, (w.n_mems + 1) * 8, hipMemcpyDeviceToHost, b->own));
    if (w.n_values) HIPCHECK(hipMemcpyAsync(w.h_vals.p, w.vals.p, w.n_values * 8, hipMemcpyDeviceToHost, b->own));
    HIPCHECK(hipStreamSynchronize(b->own)); // (the locate itself completed inside pgx_batch_locate, on whatever stream it used)
    locations_header(b, out);
    out->loc_offsets = w.h_off.as<uint64_t>();
    out->values = w.h_vals.as<uint64_t>();
    return PGX_OK;
    PGX_GUARD_END
}

