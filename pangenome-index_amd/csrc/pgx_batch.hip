// pgx_batch.hip -- the pgx_batch object (create, free, the uploads), pgx_batch_run with its stages and kernel tables, and the plain results.
// The other result forms are in pgx_batch_forms.hip, pgx_batch_locate in pgx_batch_locate.hip, the read stages (hits, place, verify, align, walk)
// in pgx_read_stages.hip; pgx_batch_internal.hpp is what they share.
//
// Pipeline of pgx_batch_run (one HIP stream, results stay on the device):
//   scan(cap)      -> slot offsets (worst-case MEMs per read: min(len, len - min_len + 1)); the slot buffer
//                     is bounded, larger batches run in chunks of consecutive reads
//   find_mems      -> MEM slots + per-read counts                      [dominant kernel, persistent grid]
//   scan(count)    -> CSR offsets ; compact slots -> dense MEM array in read order
//   tag_locate     -> per MEM run_nums + first item + size-class lists ; scans -> segment offsets
//   tag_small      -> <= 16 runs: gather + sort + unique in registers
//   tag_gather / tag_sort_unique / tag_sort_large -> listed bigger queries (identical large ones once)
//   scan ; tag_compact -> positions CSR
// The only host synchronisations are the scalar read-backs that size the next buffer.
#include <memory>
#include <string>
#include <thread>

#include "pgx_batch_internal.hpp"

// ------------------------------------------------------------------------------------------
static void batch_release(pgx_batch *b) {
    if (!b) return;
    if (hipSetDevice(b->device) == hipSuccess) {
        release_all({&b->reads, &b->offsets, &b->slot_off, &b->slots, &b->mem_count, &b->mem_off, &b->mems, &b->scan_tmp,
                     &b->counters, &b->heavy_list, &b->heavy_scratch, &b->read_flags, &b->side_list, &b->side_count, &b->packed, &b->ovf_base,
                     &b->up_side_ids, &b->up_side_off, &b->up_side_bytes, &b->fx_text, &b->fx_tiles, &b->fx_tile_base, &b->fx_lines,
                     &b->fx_contrib, &b->fx_rec, &b->fx_out_off, &b->fx_rec_idx, &b->fx_offs, &b->fx_scal, &b->fx_scan_tmp});
        b->tw.release();
        b->lw.release();
        b->cw.release();
        b->fw.release();
        b->hw.release();
        b->pw.release();
        b->vw.release();
        b->rw.release();
        b->mw.release();
        b->aw.release();
        b->ww.release();
        b->qw.release();
        release_all({&b->h_mem_off, &b->h_mems, &b->h_run_nums, &b->h_pos_off, &b->h_positions, &b->h_off[0], &b->h_off[1]});
        destroy_events(b->ev);
        if (b->own) { (void)hipStreamDestroy(b->own); b->own = nullptr; }
        if (b->side) { (void)hipStreamDestroy(b->side); b->side = nullptr; }
        destroy_events(b->ev_side);
        destroy_events(b->ev_up);
    }
    delete b;
}

extern "C" void pgx_batch_free(pgx_batch *b) { batch_release(b); }

// the new reads have proved valid and their offsets lie in the spare host buffer: swap it in and forget what belonged to the reads before
// (both uploads call this only behind their last check: a refused upload leaves the batch as it was)
static void batch_reset_for_upload(pgx_batch *b, uint64_t n_reads, uint64_t max_read_len, uint64_t read_bytes) {
    b->h_off_cur ^= 1;
    b->n_reads = n_reads;
    b->ran = b->ran_tags = false;
    b->lw.valid = false;
    b->hw.valid = false;
    b->pw.valid = false;
    b->vw.valid = false;
    b->rw.valid = false;
    b->mw.valid = false;
    b->aw.valid = false;
    b->ww.valid = false;
    b->qw.valid = false;
    b->plan_valid = false;
    b->slot_off_valid = false;
    b->class_valid = false;
    b->ms_upload_passes = 0;
    b->max_read_len = max_read_len;
    b->read_bytes = read_bytes;
}

// (re)fill a batch: device buffers only ever grow, so a long-lived batch costs no allocation per call
// offsets: validated, rebased to 0 (host copy for the chunk planner, device copy for the kernels), longest read -- one pass over them
static void batch_take_offsets(pgx_batch *b, const uint64_t *offsets, uint64_t n_reads, const char *who) {
    const uint64_t lo = offsets[0];
    HostBuf &hb = b->h_off[b->h_off_cur ^ 1]; // (swapped in once the offsets have proved valid: a refused upload leaves the batch as it was)
    hb.ensure((n_reads + 1) * 8);
    uint64_t *ho = hb.as<uint64_t>();
    ho[0] = 0;
    // ten million offsets are ~15 ms of one core: slices on a few host threads (a fresh batch per step is bound by what its host thread does
    // between the device's work: bench.py fresh_batch)
    const unsigned nt = n_reads >= (1u << 20) ? 4u : 1u;
    uint64_t longest[4] = {0, 0, 0, 0};
    bool bad[4] = {false, false, false, false};
    auto slice = [&](unsigned t) {
        const uint64_t i0 = 1 + n_reads * t / nt, i1 = 1 + n_reads * (t + 1) / nt;
        uint64_t prev = offsets[i0 - 1], mx = 0;
        bool b_ = false;
        for (uint64_t i = i0; i < i1; i++) {
            const uint64_t o = offsets[i];
            b_ |= o < prev;
            mx = std::max(mx, o - prev);
            ho[i] = o - lo;
            prev = o;
        }
        longest[t] = mx; bad[t] = b_;
    };
    if (nt == 1) slice(0);
    else {
        std::thread th[3];
        for (unsigned t = 1; t < nt; t++) th[t - 1] = std::thread(slice, t);
        slice(0);
        for (unsigned t = 1; t < nt; t++) th[t - 1].join();
    }
    uint64_t mx = 0;
    for (unsigned t = 0; t < nt; t++) {
        if (bad[t]) throw Error(PGX_ERR_ARG, std::string(who) + ": offsets must be non-decreasing");
        mx = std::max(mx, longest[t]);
    }
    if (mx >= (1ull << 31)) throw Error(PGX_ERR_UNSUPPORTED, "read longer than 2^31 bytes");
    batch_reset_for_upload(b, n_reads, mx, offsets[n_reads] - lo);
    b->offsets.ensure((n_reads + 1) * 8);
    HIPCHECK(hipMemcpyAsync(b->offsets.p, ho, (n_reads + 1) * 8, hipMemcpyHostToDevice, b->own));
}

static void batch_upload(pgx_batch *b, const uint8_t *reads, const uint64_t *offsets, uint64_t n_reads) {
    batch_take_offsets(b, offsets, n_reads, "pgx_batch_upload");
    // device offsets are rebased to 0; 32 bytes of zero padding after the last read
    // copies go through the batch's own non-blocking stream: batches of other host threads (other streams of the same device)
    // are not serialised behind them the way copies on the legacy default stream would be
    b->reads.ensure(b->read_bytes + 32);
    HIPCHECK(hipMemsetAsync((uint8_t *)b->reads.p + b->read_bytes, 0, 32, b->own));
    if (b->read_bytes) HIPCHECK(hipMemcpyAsync(b->reads.p, reads + offsets[0], b->read_bytes, hipMemcpyHostToDevice, b->own));
    HIPCHECK(hipStreamSynchronize(b->own));
}

// the reads as the host packed them (pgx_pack_reads): a quarter of the bytes over the link, and neither pgx_bad_chunks_kernel nor
// pgx_classify_reads_kernel nor their read-back on the device -- the packed words, the flags and the side list the two-step kernel wants arrive
// ready; the bytes the other kernels read are rebuilt on the device (pgx_unpack_reads_kernel + the listed reads' own bytes over them)
static void batch_upload_packed(pgx_batch *b, const uint32_t *packed, const uint64_t *offsets, uint64_t n_reads, const uint64_t *side_ids,
                                const uint8_t *side_bytes, uint64_t n_side) {
    if (offsets[0] != 0) throw Error(PGX_ERR_ARG, "pgx_batch_upload_packed: offsets[0] must be 0 (word w of the packed stream holds symbols 16 w .. 16 w + 15)");
    if (n_side > n_reads) throw Error(PGX_ERR_ARG, "pgx_batch_upload_packed: more listed reads than reads");
    for (uint64_t k = 0; k < n_side; k++) // (before anything of the batch changes: a refused upload leaves it as it was)
        if (side_ids[k] >= n_reads || (k && side_ids[k] <= side_ids[k - 1])) throw Error(PGX_ERR_ARG, "pgx_batch_upload_packed: listed read ids must ascend and lie inside the batch");
    batch_take_offsets(b, offsets, n_reads, "pgx_batch_upload_packed");
    b->h_side_off.resize(n_side + 1);
    b->h_side_off[0] = 0;
    for (uint64_t k = 0; k < n_side; k++) b->h_side_off[k + 1] = b->h_side_off[k] + (offsets[side_ids[k] + 1] - offsets[side_ids[k]]);
    const uint64_t n_chunks = (b->read_bytes + 15) >> 4, side_total = b->h_side_off[n_side];
    hipStream_t s = b->own;
    b->packed.ensure((n_chunks + 64) * 4);
    b->reads.ensure(n_chunks * 16 + 32);
    b->read_flags.ensure(((n_reads + 3) & ~3ull) + 4);
    b->side_list.ensure((n_reads ? n_reads : 1) * sizeof(pgx_heavy_item));
    b->side_count.ensure(16);
    if (n_chunks) HIPCHECK(hipMemcpyAsync(b->packed.p, packed, n_chunks * 4, hipMemcpyHostToDevice, s));
    if (n_side) {
        b->up_side_ids.ensure(n_side * 8);
        b->up_side_off.ensure((n_side + 1) * 8);
        b->up_side_bytes.ensure(side_total ? side_total : 1);
        HIPCHECK(hipMemcpyAsync(b->up_side_ids.p, side_ids, n_side * 8, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(b->up_side_off.p, b->h_side_off.data(), (n_side + 1) * 8, hipMemcpyHostToDevice, s));
        if (side_total) HIPCHECK(hipMemcpyAsync(b->up_side_bytes.p, side_bytes, side_total, hipMemcpyHostToDevice, s));
    }
    for (auto &e : b->ev_up)
        if (!e) HIPCHECK(hipEventCreate(&e));
    HIPCHECK(hipEventRecord(b->ev_up[0], s));
    HIPCHECK(hipMemsetAsync(b->side_count.p, 0, 16, s));
    HIPCHECK(hipMemsetAsync(b->read_flags.p, 0, ((n_reads + 3) & ~3ull) + 4, s));
    if (n_chunks) {
        int cus = 0;
        HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        hipLaunchKernelGGL(pgx_unpack_reads_kernel, dim3(std::min<unsigned>(grid_for(n_chunks, 256), (unsigned)cus * 16u)), dim3(256), 0, s, b->packed.as<uint32_t>(), n_chunks,
                           b->reads.as<uint8_t>());
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipMemsetAsync((uint8_t *)b->reads.p + b->read_bytes, 0, 32, s)); // (the tail of the last word unpacks to 'A's)
    if (n_side) {
        hipLaunchKernelGGL(pgx_side_reads_kernel, dim3(grid_for(n_side * 64, 256)), dim3(256), 0, s, b->reads.as<uint8_t>(), b->offsets.as<uint64_t>(), b->up_side_ids.as<uint64_t>(),
                           b->up_side_off.as<uint64_t>(), b->up_side_bytes.as<uint8_t>(), n_side, b->read_flags.as<uint8_t>(), b->side_list.as<pgx_heavy_item>(),
                           b->side_count.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipEventRecord(b->ev_up[1], s));
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipEventElapsedTime(&b->ms_upload_passes, b->ev_up[0], b->ev_up[1]));
    b->class_valid = true; // what pgx_batch_run would otherwise find out with two passes over the bytes and a read-back
    b->class_ok = true;
    b->side_reads_est = n_side;
}

// reads as text (pgx.h, PGX_READS_*), parsed by the passes of pgx_fastx_kernels.hip on the batch's own stream.  Everything up to the
// validation goes into buffers of its own (text, line table, scans, the new offsets): a refused upload leaves the batch as it was.
// Two small read-backs: the newline count (sizes the line arrays), then error word / reads / bytes / longest read in one copy.
static void batch_upload_text(pgx_batch *b, const uint8_t *text, uint64_t n_bytes, uint32_t format, uint64_t *n_reads_out) {
    static const char *const fmt_name[3] = {"LINES", "FASTA", "FASTQ"};
    if (n_bytes >= (1ull << 40)) throw Error(PGX_ERR_UNSUPPORTED, "pgx_batch_upload_text: text of 2^40 bytes or more");
    if (n_bytes == 0) {
        static const uint64_t none[1] = {0};
        batch_upload(b, nullptr, none, 0);
        *n_reads_out = 0;
        return;
    }
    hipStream_t s = b->own;
    const uint64_t n_tiles = (n_bytes + PGX_FASTX_TILE - 1) / PGX_FASTX_TILE;
    b->fx_text.ensure(n_bytes + 64); // (a 16-byte load that starts before n_bytes stays inside)
    b->fx_tiles.ensure(n_tiles * 4);
    b->fx_tile_base.ensure((n_tiles + 1) * 8);
    b->fx_scal.ensure(64);
    unsigned long long *scal = b->fx_scal.as<unsigned long long>(); // [0] first error (line << 8 | code), [1] reads, [2] sequence bytes, [3] longest read
    HIPCHECK(hipMemcpyAsync(b->fx_text.p, text, n_bytes, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(scal, 0, 64, s));
    HIPCHECK(hipMemsetAsync(scal, 0xFF, 8, s));
    const uint8_t *dt = b->fx_text.as<uint8_t>();
    hipLaunchKernelGGL(pgx_fastx_count_kernel, dim3(grid_for(n_tiles, 1)), dim3(256), 0, s, dt, n_bytes, b->fx_tiles.as<uint32_t>());
    HIPCHECK(hipGetLastError());
    scan_excl(0, b->fx_tiles.p, n_tiles, 0, b->fx_tile_base.as<uint64_t>(), b->fx_scan_tmp, s);
    const uint64_t n_nl = read_u64(b->fx_tile_base.as<uint64_t>() + n_tiles, s);
    const uint32_t tail = text[n_bytes - 1] != '\n';
    const uint64_t n_lines = n_nl + tail;
    b->fx_lines.ensure((n_lines + 1) * 8);
    b->fx_contrib.ensure(n_lines * 4);
    b->fx_rec.ensure(n_lines);
    b->fx_out_off.ensure((n_lines + 1) * 8);
    b->fx_rec_idx.ensure((n_lines + 1) * 8);
    b->fx_offs.ensure((n_lines + 1) * 8); // (reads <= lines)
    uint64_t *ls = b->fx_lines.as<uint64_t>(), *out_off = b->fx_out_off.as<uint64_t>(), *rec_idx = b->fx_rec_idx.as<uint64_t>(), *offs = b->fx_offs.as<uint64_t>();
    hipLaunchKernelGGL(pgx_fastx_lines_kernel, dim3(grid_for(n_tiles, 1)), dim3(256), 0, s, dt, n_bytes, b->fx_tile_base.as<uint64_t>(), ls, n_lines, tail);
    hipLaunchKernelGGL(pgx_fastx_role_kernel, dim3(grid_for(n_lines, 256)), dim3(256), 0, s, dt, (const uint64_t *)ls, n_lines, format, b->fx_contrib.as<uint32_t>(),
                       b->fx_rec.as<uint8_t>(), scal);
    HIPCHECK(hipGetLastError());
    scan_excl(0, b->fx_contrib.p, n_lines, 0, out_off, b->fx_scan_tmp, s, reinterpret_cast<uint64_t *>(scal + 2));
    scan_excl(4, b->fx_rec.p, n_lines, 0, rec_idx, b->fx_scan_tmp, s, reinterpret_cast<uint64_t *>(scal + 1));
    hipLaunchKernelGGL(pgx_fastx_records_kernel, dim3(grid_for(n_lines, 256)), dim3(256), 0, s, n_lines, format, (const uint32_t *)b->fx_contrib.as<uint32_t>(),
                       (const uint8_t *)b->fx_rec.as<uint8_t>(), (const uint64_t *)out_off, (const uint64_t *)rec_idx, offs, scal);
    hipLaunchKernelGGL(pgx_fastx_longest_kernel, dim3(std::min<unsigned>(grid_for(n_lines, 256), 2048u)), dim3(256), 0, s, (const uint64_t *)offs, (const uint64_t *)(rec_idx + n_lines), scal + 3);
    HIPCHECK(hipGetLastError());
    uint64_t sc[4];
    read_scalars(sc, scal, 32, s);
    if (sc[0] != ~0ull) { // the first bad line: its start (and the neighbours the message needs) from the line table
        const uint64_t line = sc[0] >> 8, code = sc[0] & 0xFF, w0 = line >= 2 ? line - 2 : 0;
        uint64_t win[4] = {0, 0, 0, 0}, ri = 0;
        read_scalars(win, ls + w0, (line + 2 - w0) * 8, s);
        ri = read_u64(rec_idx + line, s);
        const uint64_t at = win[line - w0], len = win[line - w0 + 1] - 1 - at;
        const unsigned long long rec = format == PGX_READS_FASTQ ? line / 4 + 1 : format == PGX_READS_FASTA ? std::max<uint64_t>(ri, 1) : ri + 1;
        char msg[256];
        const char *f = fmt_name[format];
        auto stripped = [&](uint64_t a, uint64_t l) { return l - ((l && text[a + l - 1] == '\r') ? 1 : 0); };
        switch (code) {
        case PGX_FASTX_ERR_NO_AT: std::snprintf(msg, sizeof msg, "%s record %llu (byte %llu): header line does not start with '@'", f, rec, (unsigned long long)at); break;
        case PGX_FASTX_ERR_NO_PLUS: std::snprintf(msg, sizeof msg, "%s record %llu (byte %llu): third line does not start with '+'", f, rec, (unsigned long long)at); break;
        case PGX_FASTX_ERR_QUAL_LEN: {
            const uint64_t sa = win[line - 2 - w0], sl = win[line - 1 - w0] - 1 - sa;
            std::snprintf(msg, sizeof msg, "%s record %llu (byte %llu): quality length %llu != sequence length %llu", f, rec, (unsigned long long)at,
                          (unsigned long long)stripped(at, len), (unsigned long long)stripped(sa, sl));
            break;
        }
        case PGX_FASTX_ERR_TRUNCATED:
            std::snprintf(msg, sizeof msg, "%s record %llu (byte %llu): truncated record (%llu of 4 lines)", f, rec, (unsigned long long)at, (unsigned long long)(n_lines - line));
            break;
        case PGX_FASTX_ERR_BEFORE_FIRST: std::snprintf(msg, sizeof msg, "%s record 1 (byte %llu): text before the first '>'", f, (unsigned long long)at); break;
        default: std::snprintf(msg, sizeof msg, "%s record %llu (byte %llu): line of 2^31 bytes or more", f, rec, (unsigned long long)at); break;
        }
        throw Error(code == PGX_FASTX_ERR_LONG_LINE ? PGX_ERR_UNSUPPORTED : PGX_ERR_FORMAT, std::string("pgx_batch_upload_text: ") + msg);
    }
    const uint64_t n_reads = sc[1], total = sc[2], longest = sc[3];
    if (longest >= (1ull << 31)) throw Error(PGX_ERR_UNSUPPORTED, "read longer than 2^31 bytes");
    // valid: from here on the batch changes
    HostBuf &hb = b->h_off[b->h_off_cur ^ 1];
    hb.ensure((n_reads + 1) * 8);
    b->reads.ensure(total + 32);
    if (total) {
        hipLaunchKernelGGL(pgx_fastx_copy_kernel, dim3(grid_for(total, 4096)), dim3(256), 0, s, dt, (const uint64_t *)ls, (const uint64_t *)out_off, n_lines, total,
                           b->reads.as<uint8_t>());
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipMemsetAsync((uint8_t *)b->reads.p + total, 0, 32, s));
    std::swap(b->offsets, b->fx_offs);
    HIPCHECK(hipMemcpyAsync(hb.p, b->offsets.p, (n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    batch_reset_for_upload(b, n_reads, longest, total);
    *n_reads_out = n_reads;
}

extern "C" pgx_status pgx_batch_create(pgx_index *h, int device, const uint8_t *reads, const uint64_t *offsets,
                                       uint64_t n_reads, pgx_batch **out) {
    PGX_GUARD_BEGIN
    if (!h || !out || !offsets || (!reads && n_reads && offsets[n_reads] != offsets[0]))
        throw Error(PGX_ERR_ARG, "pgx_batch_create: null argument");
    if (!h->has_rank) throw Error(PGX_ERR_ARG, "pgx_batch_create: index opened without an r-index");
    *out = nullptr;
    pgx_device_image *dimg = device_image(h, device);
    ensure_lce(h, dimg);
    std::unique_ptr<pgx_batch, void (*)(pgx_batch *)> b(new pgx_batch(), batch_release);
    b->h = h;
    b->dimg = dimg;
    b->device = device;
    HIPCHECK(hipStreamCreateWithFlags(&b->own, hipStreamNonBlocking));
    batch_upload(b.get(), reads, offsets, n_reads);
    *out = b.release();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_upload(pgx_batch *b, const uint8_t *reads, const uint64_t *offsets, uint64_t n_reads) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_upload");
    if (!b || !offsets || (!reads && n_reads && offsets[n_reads] != offsets[0])) throw Error(PGX_ERR_ARG, "pgx_batch_upload: null argument");
    use_device(b->device);
    batch_upload(b, reads, offsets, n_reads);
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_upload_packed(pgx_batch *b, const uint32_t *packed, const uint64_t *offsets, uint64_t n_reads, const uint64_t *side_ids,
                                              const uint8_t *side_bytes, uint64_t n_side) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_upload_packed");
    if (!b || !offsets || (!packed && n_reads && offsets[n_reads] != offsets[0]) || (n_side && (!side_ids || !side_bytes)))
        throw Error(PGX_ERR_ARG, "pgx_batch_upload_packed: null argument");
    use_device(b->device);
    batch_upload_packed(b, packed, offsets, n_reads, side_ids, side_bytes, n_side);
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_upload_text(pgx_batch *b, const uint8_t *text, uint64_t n_bytes, uint32_t format, uint64_t *n_reads) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_upload_text");
    if (!b || !n_reads || (!text && n_bytes)) throw Error(PGX_ERR_ARG, "pgx_batch_upload_text: null argument");
    if (format > PGX_READS_FASTQ) throw Error(PGX_ERR_ARG, "pgx_batch_upload_text: unknown format " + std::to_string(format));
    use_device(b->device);
    batch_upload_text(b, text, n_bytes, format, n_reads);
    return PGX_OK;
    PGX_GUARD_END
}

// the reads as they lie on the device, whichever upload put them there (tests)
extern "C" pgx_status pgx_batch_reads(pgx_batch *b, pgx_reads_info *info, uint64_t *offsets, uint64_t offsets_cap, uint8_t *bytes, uint64_t bytes_cap) {
    PGX_GUARD_BEGIN
    if (!b || !info) throw Error(PGX_ERR_ARG, "pgx_batch_reads: null argument");
    info->n_reads = b->n_reads;
    info->n_bytes = b->read_bytes;
    info->longest = b->max_read_len;
    if ((offsets && offsets_cap < b->n_reads + 1) || (bytes && bytes_cap < b->read_bytes)) throw Error(PGX_ERR_ARG, "pgx_batch_reads: capacity too small");
    use_device(b->device);
    if (offsets) HIPCHECK(hipMemcpyAsync(offsets, b->offsets.p, (b->n_reads + 1) * 8, hipMemcpyDeviceToHost, b->own));
    if (bytes && b->read_bytes) HIPCHECK(hipMemcpyAsync(bytes, b->reads.p, b->read_bytes, hipMemcpyDeviceToHost, b->own));
    HIPCHECK(hipStreamSynchronize(b->own));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// pgx_batch_run

// Every environment variable a run consults, read once at the top of each pgx_batch_run call (per call, not per process: the tests change
// them between the runs of one process).  Each keeps the parse rule it always had.  The image-build knobs are read where the image is
// built (pgx_images.hip ImageKnobs), PGX_LOCATE_BUDGET_MB by pgx_batch_locate, PGX_ROCTX and PGX_SCAN_THREE once per process.
struct RunKnobs {
    bool spec;               // PGX_SPEC=0 clears it: no speculative sizing, every run reads its intermediate totals back
    bool arena;              // PGX_SLOT_ARENA=0 clears it: MEM slots in the worst-case layout, no arena for the fifth and later MEMs
    bool has_arena_cap;      // PGX_SLOT_ARENA_CAP is set, and
    uint64_t arena_cap;      //   its value (strtoull): arena capacity in slots before rounding (tests: an arena that overflows)
    uint64_t budget_slots;   // PGX_SLOT_BUDGET_MB (strtoull, at least 1), in slots: bound of the slot buffer; 0 = not set
    bool narrow;             // PGX_FM_NARROW=0 clears it: 64-bit interval state even where the 32-bit kernels would do
    bool force_redo;         // PGX_FM_NARROW_FORCE_REDO is set at all (tests): the first attempt of every chunk in 32 bits is repeated in 64, no speculation
    bool pairs;              // PGX_FM_PAIRS=0 clears it: the dense2 kernel alone, even where the index has a PAIRS image
    bool side;               // PGX_FM_NO_SIDE set at all clears it: no launch on the second stream, the pairs kernel serves every read
    bool packed;             // PGX_FM_PACKED=0 clears it: the pairs kernel reads byte windows, not two bits per symbol from LDS
    int coop;                // PGX_FM_COOP: 1 if it starts with '1', 0 if set to anything else, -1 if not set (then the size of the PAIRS image decides)
    bool lce;                // PGX_FM_LCE=0 clears it: no forward stages through the LCE image even where it exists
    bool has_wg_per_cu;      // PGX_FM_WG_PER_CU is set at all (switches the reads-per-lane rule off), and
    int wg_per_cu;           //   its value (atoi): resident workgroups per CU, applied where it lies in [1, occupancy)
    uint32_t heavy_ext;      // PGX_FM_HEAVY_EXT (strtoul; default PGX_FM_HEAVY_EXT): extensions on one read before its rest goes to the heavy-read kernel, 0 = never
    bool has_side_heavy_ext; // PGX_FM_SIDE_HEAVY_EXT is set, and
    uint32_t side_heavy_ext; //   its value (strtoul): the same threshold for the second-stream launch alone
    bool debug_counters;     // PGX_DEBUG_COUNTERS set at all: the run's device counters on stderr
    bool fm_stats;           // PGX_FM_STATS set at all: the lane statistics of a -DPGX_FM_STATS build on stderr
};

static RunKnobs read_run_knobs() {
    auto is_set = [](const char *name) { return std::getenv(name) != nullptr; };
    auto not_zero = [](const char *name) { const char *e = std::getenv(name); return !(e && e[0] == '0'); };
    RunKnobs k{};
    k.spec = not_zero("PGX_SPEC");
    k.arena = not_zero("PGX_SLOT_ARENA");
    if (const char *e = std::getenv("PGX_SLOT_ARENA_CAP")) { k.has_arena_cap = true; k.arena_cap = std::strtoull(e, nullptr, 10); }
    if (const char *e = std::getenv("PGX_SLOT_BUDGET_MB")) k.budget_slots = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10)) * (1ull << 20) / sizeof(pgx_mem);
    k.narrow = not_zero("PGX_FM_NARROW");
    k.force_redo = is_set("PGX_FM_NARROW_FORCE_REDO");
    k.pairs = not_zero("PGX_FM_PAIRS");
    k.side = !is_set("PGX_FM_NO_SIDE");
    k.packed = not_zero("PGX_FM_PACKED");
    k.coop = -1;
    if (const char *e = std::getenv("PGX_FM_COOP")) k.coop = e[0] == '1';
    k.lce = not_zero("PGX_FM_LCE");
    if (const char *e = std::getenv("PGX_FM_WG_PER_CU")) { k.has_wg_per_cu = true; k.wg_per_cu = std::atoi(e); }
    k.heavy_ext = PGX_FM_HEAVY_EXT;
    if (const char *e = std::getenv("PGX_FM_HEAVY_EXT")) k.heavy_ext = (uint32_t)std::strtoul(e, nullptr, 10);
    if (const char *e = std::getenv("PGX_FM_SIDE_HEAVY_EXT")) { k.has_side_heavy_ext = true; k.side_heavy_ext = (uint32_t)std::strtoul(e, nullptr, 10); }
    k.debug_counters = is_set("PGX_DEBUG_COUNTERS");
    k.fm_stats = is_set("PGX_FM_STATS");
    return k;
}

// The variants of pgx_find_mems_kernel the runtime launches, each named here and in the instantiation list of pgx_fm_kernels.hip (for the pairs kernel below:
// of pgx_pairs_kernels.hip), and nowhere else.
// Only images of up to 48 KiB are staged in LDS, and only the run-length and the 64-byte dense image are (pgx_images.hip device_image); the run-length image has
// neither a 32-bit form nor seeds, the wide dense2 image (kind 3) no 32-bit form.
// (nullptr: no such instance)
static const void *find_mems_entry(bool in_lds, uint32_t kind, bool narrow, bool seeded) {
    using K = const void *;
    static const K tab[2][4][2][2] = { // [image in LDS][image kind][32-bit state][seeded]
        {{{(K)pgx_find_mems_kernel<false, 0, false, false>, nullptr}, {nullptr, nullptr}},
         {{(K)pgx_find_mems_kernel<false, 1, false, false>, (K)pgx_find_mems_kernel<false, 1, false, true>},
          {(K)pgx_find_mems_kernel<false, 1, true, false>, (K)pgx_find_mems_kernel<false, 1, true, true>}},
         {{(K)pgx_find_mems_kernel<false, 2, false, false>, (K)pgx_find_mems_kernel<false, 2, false, true>},
          {(K)pgx_find_mems_kernel<false, 2, true, false>, (K)pgx_find_mems_kernel<false, 2, true, true>}},
         {{(K)pgx_find_mems_kernel<false, 3, false, false>, (K)pgx_find_mems_kernel<false, 3, false, true>}, {nullptr, nullptr}}},
        {{{(K)pgx_find_mems_kernel<true, 0, false, false>, nullptr}, {nullptr, nullptr}},
         {{(K)pgx_find_mems_kernel<true, 1, false, false>, (K)pgx_find_mems_kernel<true, 1, false, true>},
          {(K)pgx_find_mems_kernel<true, 1, true, false>, (K)pgx_find_mems_kernel<true, 1, true, true>}},
         {{nullptr, nullptr}, {nullptr, nullptr}},
         {{nullptr, nullptr}, {nullptr, nullptr}}}};
    return kind < 4 ? tab[in_lds][kind][narrow][seeded] : nullptr;
}

// pgx_timing.kernels: the coordinates of an instance in the table above
static uint32_t find_mems_bits(bool in_lds, uint32_t kind, bool narrow, bool seeded) {
    return PGX_KERNELS_FM | (seeded ? PGX_KERNELS_FM_SEEDED : 0u) | (narrow ? PGX_KERNELS_FM_NARROW : 0u) | (kind << PGX_KERNELS_FM_KIND_SHIFT) | (in_lds ? PGX_KERNELS_FM_LDS : 0u);
}

static const void *find_mems_variant(bool in_lds, uint32_t kind, bool narrow, bool seeded, uint32_t &bits) {
    if (kind == 0) seeded = false; // (no stage of the run-length kernel looks at a seed table)
    const void *f = find_mems_entry(in_lds, kind, narrow, seeded);
    if (!f) throw Error(PGX_ERR_UNSUPPORTED, "pgx_batch_run: no find_mems kernel for this image");
    bits = find_mems_bits(in_lds, kind, narrow, seeded);
    return f;
}

// The same for pgx_find_mems_pairs_kernel (always seeded).  The cooperative line fetches and the LCE path exist only with the packed reads,
// the LCE path only for narrow images without the cooperative fetches.
// (nullptr: no such instance)
static const void *find_mems_pairs_entry(bool wide, bool packed, bool coop, bool s64, bool lce) {
    using K = const void *;
    static const K plain[2][2] = { // [wide][stride 64]
        {(K)pgx_find_mems_pairs_kernel<false, false, false, false, false>, (K)pgx_find_mems_pairs_kernel<false, false, false, true, false>},
        {(K)pgx_find_mems_pairs_kernel<true, false, false, false, false>, (K)pgx_find_mems_pairs_kernel<true, false, false, true, false>}};
    static const K pack[2][2][2] = { // [wide][cooperative][stride 64]
        {{(K)pgx_find_mems_pairs_kernel<false, true, false, false, false>, (K)pgx_find_mems_pairs_kernel<false, true, false, true, false>},
         {(K)pgx_find_mems_pairs_kernel<false, true, true, false, false>, (K)pgx_find_mems_pairs_kernel<false, true, true, true, false>}},
        {{(K)pgx_find_mems_pairs_kernel<true, true, false, false, false>, (K)pgx_find_mems_pairs_kernel<true, true, false, true, false>},
         {(K)pgx_find_mems_pairs_kernel<true, true, true, false, false>, (K)pgx_find_mems_pairs_kernel<true, true, true, true, false>}}};
    static const K with_lce[2] = {(K)pgx_find_mems_pairs_kernel<false, true, false, false, true>, (K)pgx_find_mems_pairs_kernel<false, true, false, true, true>}; // [stride 64]
    if (lce) return (wide || !packed || coop) ? nullptr : with_lce[s64];
    if (!packed) return coop ? nullptr : plain[wide][s64];
    return pack[wide][coop][s64];
}

static uint32_t find_mems_pairs_bits(bool wide, bool packed, bool coop, bool s64, bool lce) {
    return PGX_KERNELS_PAIRS | (s64 ? PGX_KERNELS_PAIRS_S64 : 0u) | (coop ? PGX_KERNELS_PAIRS_COOP : 0u) | (packed ? PGX_KERNELS_PAIRS_PACKED : 0u) |
           (wide ? PGX_KERNELS_PAIRS_WIDE : 0u) | (lce ? PGX_KERNELS_PAIRS_LCE : 0u);
}

static const void *find_mems_pairs_variant(bool wide, bool packed, bool coop, bool s64, bool lce, uint32_t &bits) {
    const void *f = find_mems_pairs_entry(wide, packed, coop, s64, lce);
    if (!f && lce) throw Error(PGX_ERR_UNSUPPORTED, "pgx_batch_run: no LCE pairs kernel for this image");
    if (!f) throw Error(PGX_ERR_UNSUPPORTED, "pgx_batch_run: no cooperative pairs kernel without the packed reads");
    bits = find_mems_pairs_bits(wide, packed, coop, s64, lce);
    return f;
}

// every instance of the two tables, as pgx_timing.kernels names it (tests: what "all variants" means comes from here)
extern "C" uint32_t pgx_kernel_variants(uint32_t *out, uint32_t cap) {
    uint32_t n = 0;
    auto put = [&](uint32_t bits) { if (out && n < cap) out[n] = bits; n++; };
    for (int c = 0; c < 32; c++) {
        const bool in_lds = c & 16, narrow = c & 2, seeded = c & 1;
        const uint32_t kind = (c >> 2) & 3;
        if (find_mems_entry(in_lds, kind, narrow, seeded)) put(find_mems_bits(in_lds, kind, narrow, seeded));
    }
    for (int c = 0; c < 32; c++) {
        const bool wide = c & 16, packed = c & 8, coop = c & 4, s64 = c & 2, lce = c & 1;
        if (find_mems_pairs_entry(wide, packed, coop, s64, lce)) put(find_mems_pairs_bits(wide, packed, coop, s64, lce));
    }
    return n;
}

// what a run carries from stage to stage
struct RunCtx {
    pgx_batch *b;
    hipStream_t s;
    RunKnobs k;
    PgxDevImage img; // (a copy: the seed table is chosen per run)
    uint64_t n, min_len, min_occ;
    bool want_tags;
    unsigned long long *ctr = nullptr; // the device counters (PgxCounterSlot, pgx_device.h)
    // chosen once per pass
    bool spec = false, arena_on = false;
    uint64_t cm_cap = 0; // capacity of the MEM array of a speculative pass
    const void *kfn = nullptr, *kfn_wide = nullptr, *kfn_pairs = nullptr; // the kernel of the first attempt, its 64-bit form, the pairs kernel (or none)
    uint32_t kfn_bits = 0, kfn_pairs_bits = 0; // their instances, as pgx_timing.kernels names them
    size_t pairs_lds = 0;
    int cus = 0;
    // gathered over the pass
    bool fresh_work = false, fresh_mark = false; // the pass performs work only the first run after an upload needs (pgx_timing.ms_per_upload); event 9 recorded behind it
    uint64_t n_ext = 0;
    float ms_fm = 0, ms_cp = 0, ms_main = 0;     // per-chunk times of a timed run with several chunks
};

// the arguments the find_mems kernels of one attempt share (hipLaunchKernel takes their addresses)
struct FmArgs {
    PgxDevImage img;
    const uint8_t *reads;
    const uint64_t *off, *slot_off;
    uint64_t n, min_len, min_occ, base, first;
    pgx_mem *slots;
    uint32_t *cnt;
    unsigned long long *next, *cur;
    uint32_t hext, hcap;
    pgx_heavy_item *hlist;
    unsigned long long *hcount;
    uint32_t *ovf; // (indexed by read id; the buffer holds this chunk's reads)
    uint64_t ovf_cap;
};

static void record(pgx_batch *b, int i, hipStream_t s) {
    static const char *const stage[10] = {"pgx: run begins (classify, sizing)", "pgx: find_mems launches follow", "pgx: find_mems enqueued", "pgx: compaction enqueued",
                                          "pgx: tag locate enqueued", "pgx: tag gather enqueued", "pgx: tag sort/unique enqueued", "pgx: run enqueued", "pgx: main find_mems kernel enqueued",
                                          "pgx: per-upload passes enqueued"};
    if (roctx().on) roctx().mark(stage[i]);
    if (!b->timed) return;
    if (!b->ev[i]) HIPCHECK(hipEventCreate(&b->ev[i]));
    HIPCHECK(hipEventRecord(b->ev[i], s));
}

// Persistent grid of a find_mems launch over cn reads: as many workgroups as the device keeps resident (no inter-workgroup dependency exists, so
// any grid size is correct; this one avoids a tail of late blocks), at most PGX_FM_WG_PER_CU per CU where that is set.  Without it, kernels for which
// `few_suffice` (the dense and the packed ones) need little occupancy, and every resident lane ends the launch inside a read (the tail): they aim at
// >= 5 reads per lane, at least 2 workgroups per CU (1 M reads: 3 workgroups per CU measured best, 493 vs 477 (x) and 179 vs 160 (synth) Mreads/s).
static unsigned find_mems_grid(const RunCtx &r, const void *kfn, size_t lds, bool few_suffice, uint64_t cn) {
    int wg = 0;
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg, kfn, PGX_FM_THREADS, lds));
    if (wg < 1) wg = 1;
    if (r.k.has_wg_per_cu) {
        if (r.k.wg_per_cu >= 1 && r.k.wg_per_cu < wg) wg = r.k.wg_per_cu;
    } else if (few_suffice)
        wg = (int)std::min<uint64_t>((uint64_t)wg, std::max<uint64_t>(2, cn / (5ull * (uint64_t)r.cus * PGX_FM_THREADS)));
    return std::min(grid_for(cn, 64), (unsigned)(wg * r.cus));
}

// 1. worst-case MEM slots per read: cap = min(len, len - min_len + 1).  The slot buffer is bounded by a budget; batches whose worst case
//    exceeds it are processed in chunks of consecutive reads.  Offsets and plan are kept across runs.
static void plan_slots(RunCtx &r) {
    pgx_batch *b = r.b;
    const uint64_t n = r.n, min_len = r.min_len;
    b->slot_off.ensure((n + 1) * 8);
    if (!b->slot_off_valid || b->slot_off_min_len != min_len) { // depends on the reads and min_len only: kept across runs
        r.fresh_work = true;
        scan_excl(2, b->offsets.p, n, min_len, b->slot_off.as<uint64_t>(), b->scan_tmp, r.s);
        b->slot_off_valid = true;
        b->slot_off_min_len = min_len;
    }
    b->mem_count.ensure((n ? n : 1) * 4);
    b->mem_off.ensure((n + 1) * 8);
    // a quarter of the device's memory (72 GB of the MI355X's 288 GB: ten million 150-bp reads are one chunk), 16 GiB at least
    uint64_t budget_slots = (16ull << 30) / sizeof(pgx_mem);
    {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess) budget_slots = std::max<uint64_t>(budget_slots, (uint64_t)(mem_total / 4) / sizeof(pgx_mem));
        else (void)hipGetLastError();
    }
    if (r.k.budget_slots) budget_slots = r.k.budget_slots;
    if (!b->plan_valid || b->plan_min_len != min_len || b->plan_budget != budget_slots) { // cached across runs
        b->chunks.clear();
        uint64_t r0 = 0, base = 0, acc = 0;
        // the slots of a read never exceed its length: a batch whose bytes fit the budget is one chunk, no per-read loop
        if (n && b->read_bytes <= budget_slots) b->chunks.push_back({0, n, 0, std::max<uint64_t>(b->read_bytes, 1)});
        else {
            for (uint64_t i = 0; i < n; i++) {
                const uint64_t len = b->h_offsets()[i + 1] - b->h_offsets()[i];
                const uint64_t cap = len < min_len ? 0 : std::min<uint64_t>(len, len - min_len + 1);
                if (acc && acc + cap > budget_slots) { b->chunks.push_back({r0, i, base, acc}); r0 = i; base += acc; acc = 0; }
                acc += cap;
            }
            if (n) b->chunks.push_back({r0, n, base, acc});
        }
        b->plan_valid = true; b->plan_min_len = min_len; b->plan_budget = budget_slots;
    }
    uint64_t max_chunk_reads = 1;
    for (auto &c : b->chunks) max_chunk_reads = std::max(max_chunk_reads, c.r1 - c.r0);
    b->ovf_base.ensure(max_chunk_reads * 4);
}

// the kernels of the pass: kfn for the first attempt of a chunk, kfn_wide for its repeat in 64 bits, kfn_pairs where the pairs kernel runs
// (kfn then serves the reads it skips, on the second stream)
static void choose_kernels(RunCtx &r) {
    pgx_batch *b = r.b;
    const PgxDevImage &img = r.img;
    const bool in_lds = b->dimg->lds_bytes != 0;
    const bool seeded = img.seed_k != 0 && r.min_len >= img.seed_k; // (no stage of a shorter search has room for a seed)
    r.kfn = r.kfn_wide = find_mems_variant(in_lds, img.dense, false, seeded, r.kfn_bits);
    // 32-bit interval state for dense images of BWTs shorter than 2^30 (PGX_FM_NARROW=0 switches it off)
    bool c_fits = true; // C[] comes straight from the file: a (corrupt) value beyond 2^32 must not be truncated by the 32-bit state
    for (int i = 0; i < 8; i++) c_fits = c_fits && !(b->h->img.consts.C[i] >> 32);
    if (img.dense && img.dense != 3 && img.n < (1ull << 30) && c_fits && r.k.narrow) r.kfn = find_mems_variant(in_lds, img.dense, true, seeded, r.kfn_bits);
    // two extensions per cache line where the index has a PAIRS image (PGX_FM_PAIRS=0: the dense2 kernel alone)
    // (only behind the seed table: the wide intervals at the start of an unseeded stage always have special positions between their ends)
    r.kfn_pairs = nullptr;
    if (img.pairs && seeded && !(r.n >> 32) && b->read_bytes < (1ull << 35) && r.k.pairs)
        r.kfn_pairs = find_mems_pairs_variant(img.wide != 0, false, false, img.pairs_stride == PGX_PAIRS_STRIDE64, false, r.kfn_pairs_bits);
    r.pairs_lds = img.wide ? (size_t)img.n_sbp * 192 : 0; // (superblock bases of the wide form, behind the other dynamic LDS)
    HIPCHECK(hipDeviceGetAttribute(&r.cus, hipDeviceAttributeMultiprocessorCount, b->device));
}

// once per upload: which reads hold a byte outside A C G T (two small passes and one scalar read back), and the reads at two bits per symbol
static void classify_reads(RunCtx &r, uint64_t cn) {
    pgx_batch *b = r.b;
    hipStream_t s = r.s;
    r.fresh_work = true;
    const uint64_t cap = std::max<uint64_t>(cn, 1024); // chunks with such a byte; beyond that (lower-case reads, say) no side launch
    b->read_flags.ensure(((cn + 3) & ~3ull) + 4);
    b->side_list.ensure((cn ? cn : 1) * sizeof(pgx_heavy_item));
    b->side_count.ensure(16);
    b->scan_tmp.ensure(cap * 8);
    b->scan_tmp.scan_epoch = 0; // (the list overwrites the scans' tile words: the next scan clears the buffer)
    b->packed.ensure(((b->read_bytes + 15) / 16 + 64) * 4); // the reads as two bits per symbol (written by the same pass)
    HIPCHECK(hipMemsetAsync(b->side_count.p, 0, 16, s));
    HIPCHECK(hipMemsetAsync(b->read_flags.p, 0, ((cn + 3) & ~3ull) + 4, s));
    unsigned long long *d_bad = b->side_count.as<unsigned long long>() + 1;
    hipLaunchKernelGGL(pgx_bad_chunks_kernel, dim3(std::min<unsigned>(grid_for((b->read_bytes + 15) / 16, 256), (unsigned)r.cus * 16u)), dim3(256), 0, s,
                       (const uint8_t *)b->reads.as<uint8_t>(), b->read_bytes, b->scan_tmp.as<uint64_t>(), d_bad, cap, b->packed.as<uint32_t>());
    HIPCHECK(hipGetLastError());
    unsigned long long n_bad = 0;
    read_scalars(&n_bad, d_bad, sizeof n_bad, s);
    b->class_ok = n_bad <= cap;
    b->side_reads_est = n_bad / 4; // (a read that overlaps an N run holds a handful of such 16-byte chunks)
    if (b->class_ok && n_bad) {
        hipLaunchKernelGGL(pgx_classify_reads_kernel, dim3(grid_for(n_bad, 256)), dim3(256), 0, s, (const uint8_t *)b->reads.as<uint8_t>(),
                           (const uint64_t *)b->offsets.as<uint64_t>(), cn, (const uint64_t *)b->scan_tmp.as<uint64_t>(), (const unsigned long long *)d_bad, cap,
                           b->read_flags.as<uint32_t>(), b->side_list.as<pgx_heavy_item>(), b->side_count.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
    }
    b->class_valid = true;
}

// Reads with a byte outside A C G T cannot be seeded: they go to the other kernel (kf) at once, on a second stream next to the pairs kernel, which
// skips them (a read cut from an N run is a chain of thousands of extensions: behind the pairs kernel it was 1.5 ms of tail).
static void launch_side(RunCtx &r, FmArgs &a, const void *kf, unsigned grid) {
    pgx_batch *b = r.b;
    HIPCHECK(hipEventRecord(b->ev_side[0], r.s));
    HIPCHECK(hipStreamWaitEvent(b->side, b->ev_side[0], 0));
    const pgx_heavy_item *s_list = b->side_list.as<pgx_heavy_item>();
    const unsigned long long *s_count = b->side_count.as<unsigned long long>();
    unsigned long long *s_cur = r.ctr + PGX_CTR_SIDE_CURSOR;
    // (a lane of this launch walks its read alone, one dependent extension after the other next to the pairs kernel: the launch lasts as long
    //  as its longest chain, so its reads go to the heavy-read kernel -- every start position at once -- earlier than the main launch's)
    uint32_t s_hext = r.k.heavy_ext ? std::min<uint32_t>(r.k.heavy_ext, PGX_FM_SIDE_HEAVY_EXT) : 0u;
    if (r.k.has_side_heavy_ext) s_hext = r.k.side_heavy_ext;
    void *sargs[] = {&a.img, &a.reads, &a.off, &a.n, &a.min_len, &a.min_occ, &a.slot_off, &a.slots, &a.cnt, &a.next, &s_cur, &a.first, &a.base,
                     &s_hext, &a.hcap, &a.hlist, &a.hcount, &s_list, &s_count, &a.ovf, &a.ovf_cap};
    // one workgroup per CU next to the pairs kernel while these reads are few (0.4 % of the chr22 workload: 43 k reads, less than one per lane);
    // with many of them the launch was the longest thing in the step (5 % = 500 k reads, 7.6 per lane one after the other: 21.8 ms next
    // to a 17 ms pairs kernel): up to four per CU, two reads per lane (profiles/r04_n_read_share.txt)
    const uint64_t cus = (uint64_t)r.cus;
    const unsigned side_wgs = (unsigned)std::min<uint64_t>(4 * cus, std::max<uint64_t>(cus, b->side_reads_est / (2ull * PGX_FM_THREADS) + 1));
    HIPCHECK(hipLaunchKernel(kf, dim3(std::min<unsigned>(grid, side_wgs)), dim3(PGX_FM_THREADS), sargs, b->dimg->lds_bytes, b->side));
    b->timing.kernels |= r.kfn_bits | PGX_KERNELS_SIDE | (kf != r.kfn ? PGX_KERNELS_FM_REDO : 0u);
    HIPCHECK(hipEventRecord(b->ev_side[1], b->side));
}

// The pairs kernel over the chunk.  It takes the reads from LDS, two bits per symbol, when every read the launch serves is pure A C G T (skip: the
// others are skipped) and a thread's column stays small enough for four workgroups per CU (reads up to ~350 bp); PGX_FM_PACKED=0 switches that off.
static void launch_pairs(RunCtx &r, FmArgs &a, const uint8_t *skip, uint64_t cn, unsigned grid) {
    pgx_batch *b = r.b;
    const PgxDevImage &img = r.img;
    const void *kp = r.kfn_pairs;
    uint32_t kp_bits = r.kfn_pairs_bits;
    size_t plds = r.pairs_lds;
    const uint32_t *a_packed = nullptr;
    uint32_t a_pkw = 0;
    const uint32_t pkw = (uint32_t)((15 + b->max_read_len + 15) >> 4) + 1u; // words of the longest read at the worst phase + one of padding
    if (skip && pkw <= 24 && r.k.packed) {
        // cooperative line fetches (one address translation per line instead of five) for PAIRS images beyond the reach of the
        // translation caches, ~3 GB (profiles/r03_ubench_gather_loads_per_line.txt); PGX_FM_COOP=0 / 1 overrides
        const bool coop = r.k.coop >= 0 ? r.k.coop != 0 : b->h->img.pairs.size() > (3ull << 30);
        // forward stages over narrow intervals through the suffix array and the text (pgx_image.h "LCE image"; min_occ <= 1: the longest match decides)
        const bool lce = img.lce_sa && !coop && !img.wide && r.min_occ <= 1 && r.k.lce;
        kp = find_mems_pairs_variant(img.wide != 0, true, coop, img.pairs_stride == PGX_PAIRS_STRIDE64, lce, kp_bits);
        // per thread of the LCE kernel: a seed entry, a suffix array entry, sixteen common prefixes from any byte on (five dwords)
        const size_t lce_lds = lce ? (size_t)PGX_FM_THREADS * (16 + 4 + 20) : 0;
        a_packed = b->packed.as<uint32_t>();
        a_pkw = pkw;
        plds = (size_t)pkw * PGX_FM_THREADS * 4 + (coop ? (size_t)(PGX_FM_THREADS / 64) * 8192 : 0) + (img.wide ? (size_t)img.n_sbp * 192 : 0) + lce_lds;
        b->timing.pairs_reads = lce ? 4u : coop ? 3u : 2u;
        grid = find_mems_grid(r, kp, plds, true, cn);
    }
    // the kernel's one argument: what it reads of the image, and the launch (pgx_device.h)
    PgxPairsArgs p = {};
    p.pairs = img.pairs; p.seed = img.seed; p.seed_end = img.seed_end;
    p.lce_sa = img.lce_sa; p.lce_text = img.lce_text; p.lce_flags = img.lce_flags; p.lce_lcp = img.lce_lcp;
    p.reads = a.reads; p.slots = a.slots; p.mem_count = a.cnt;
    p.n = img.n; p.min_len = a.min_len; p.min_occ = a.min_occ;
    p.first_read = a.first; p.n_reads = a.n;
    p.seed_k = img.seed_k; p.seed_end_k = img.seed_end_k; p.lce_max = img.lce_max; p.refill_min = img.refill_min;
    p.pk_words = a_pkw; p.heavy_ext = a.hext; p.pairs_sb_shift = img.pairs_sb_shift; p.dense = img.dense;
    p.consts = img.consts; p.first_ext = img.first_ext; p.pbase = img.pbase; p.n_sbp = img.n_sbp;
    p.offsets = a.off; p.skip = skip; p.packed = a_packed;
    p.cursor = a.cur; p.ctr = a.next;
    p.slot_off = a.slot_off; p.slot_base = a.base; p.ovf_base = a.ovf; p.ovf_cap = a.ovf_cap;
    p.heavy_list = a.hlist; p.heavy_count = a.hcount; p.heavy_cap = a.hcap; p.d2_sb_shift = img.d2_sb_shift;
    p.blocks = img.blocks; p.exc = img.exc; p.sbase2 = img.sbase2;
    void *pargs[] = {&p};
    HIPCHECK(hipLaunchKernel(kp, dim3(grid), dim3(PGX_FM_THREADS), pargs, plds, r.s)); // (PGX_FM_THREADS: the kernel takes its LDS strides from it)
    b->timing.kernels |= kp_bits;
}

// arena for the fifth and later MEMs of a chunk's reads, in slots (0 = worst-case layout): sized from the last run of this batch, or eight slots per read
static uint64_t arena_slots(const RunCtx &r, const pgx_chunk &c) {
    const pgx_batch *b = r.b;
    if (!r.arena_on) return 0;
    const uint64_t cn = c.r1 - c.r0;
    uint64_t want = b->shape_valid && b->shape_reads == r.n && b->shape_min_len == r.min_len && b->chunks.size() == 1 ? with_slack(b->last_ovf_used) + 4096 : 8 * cn + 4096; // (first run of a shape: eight slots per read; chr22 scale asks for 2.6, the x fixture for 6.7)
    if (r.k.has_arena_cap) want = r.k.arena_cap; // tests: an arena that overflows
    want = std::max<uint64_t>(want, b->max_read_len + 1); // (an overflowing extent is parked at the start of the arena: it must fit)
    want = std::max<uint64_t>(want, (uint64_t)PGX_ARENA_SUBS * (b->max_read_len + 1)); // (every sub-arena must hold a parked extent)
    want = (want + PGX_ARENA_SUBS - 1) / PGX_ARENA_SUBS * PGX_ARENA_SUBS;
    return want < c.slots && want < (1ull << 32) ? want : 0; // otherwise the worst case is no bigger
}

// 2. the hot kernel over one chunk, repeated where it has to be: in the worst-case slot layout after the arena proved too small, in 64 bits after a
//    coordinate left 32.  Returns the chunk's MEM total (a speculative pass: the capacity; the total stays on the device), and in ovf_cap the arena
//    the last attempt used.
static uint64_t find_mems_chunk(RunCtx &r, size_t ci, uint64_t &ovf_cap) {
    pgx_batch *b = r.b;
    hipStream_t s = r.s;
    const pgx_chunk &c = b->chunks[ci];
    const uint64_t cn = c.r1 - c.r0;
    const bool one_chunk = b->chunks.size() == 1;
    const uint32_t heavy_ext = r.k.heavy_ext;
    const unsigned grid = find_mems_grid(r, r.kfn_pairs ? r.kfn_pairs : r.kfn, r.kfn_pairs ? r.pairs_lds : b->dimg->lds_bytes, r.img.dense != 0, cn);
    uint64_t *local = b->mem_off.as<uint64_t>() + c.r0; // local CSR offsets of this chunk (scratch until the global scan)
    const void *kf = r.kfn;
    ovf_cap = arena_slots(r, c);
    for (int attempt = 0;; attempt++) {
        b->slots.ensure(((ovf_cap ? ovf_cap : c.slots) + 4 * cn) * sizeof(pgx_mem));
        // per-chunk counters (slots below PGX_CTR_TAG0): extensions, cursors, heavy reads, 32-bit overflow flag, MEMs of the chunk
        if (ci || attempt) {
            HIPCHECK(hipMemsetAsync(r.ctr, 0, PGX_CTR_TAG0 * 8, s));
            HIPCHECK(hipMemsetAsync(r.ctr + PGX_CTR_ARENA0, 0, (PGX_CTR_ALL - PGX_CTR_ARENA0) * 8, s));
        }
        FmArgs a;
        a.img = r.img;
        a.reads = b->reads.as<uint8_t>();
        a.off = b->offsets.as<uint64_t>(); a.slot_off = b->slot_off.as<uint64_t>();
        a.n = c.r1; a.min_len = r.min_len; a.min_occ = r.min_occ; a.base = c.slot_base; a.first = c.r0;
        a.slots = b->slots.as<pgx_mem>();
        a.cnt = b->mem_count.as<uint32_t>();
        a.next = r.ctr; a.cur = r.ctr + PGX_CTR_CURSOR;
        a.hext = heavy_ext; a.hcap = PGX_FM_HEAVY_CAP;
        a.hlist = b->heavy_list.as<pgx_heavy_item>();
        a.hcount = r.ctr + PGX_CTR_HEAVY;
        a.ovf = b->ovf_base.as<uint32_t>() - c.r0;
        a.ovf_cap = ovf_cap;
        bool side_running = false;
        if (r.kfn_pairs) { // the pairs kernel; the kernel chosen for the first attempt (or its 64-bit form) serves the reads it skips
            const uint8_t *skip = nullptr;
            if (one_chunk && r.k.side) {
                if (!b->side) {
                    HIPCHECK(hipStreamCreateWithFlags(&b->side, hipStreamNonBlocking));
                    for (auto &e : b->ev_side) HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                }
                if (!b->class_valid) classify_reads(r, cn);
                record(b, 9, s); r.fresh_mark = true;
                if (b->class_ok) {
                    skip = b->read_flags.as<uint8_t>();
                    launch_side(r, a, kf, grid);
                    side_running = true;
                }
            }
            launch_pairs(r, a, skip, cn, grid);
        } else { // (without it the one kernel serves every read of the launch itself)
            const pgx_heavy_item *a_rlist = nullptr;
            const unsigned long long *a_rcount = nullptr;
            void *args[] = {&a.img, &a.reads, &a.off, &a.n, &a.min_len, &a.min_occ, &a.slot_off, &a.slots, &a.cnt, &a.next, &a.cur, &a.first, &a.base,
                            &a.hext, &a.hcap, &a.hlist, &a.hcount, &a_rlist, &a_rcount, &a.ovf, &a.ovf_cap};
            if (ci == 0 && attempt == 0) { record(b, 9, s); r.fresh_mark = true; }
            HIPCHECK(hipLaunchKernel(kf, dim3(grid), dim3(PGX_FM_THREADS), args, b->dimg->lds_bytes, s)); // one of the variants
            b->timing.kernels |= r.kfn_bits | (kf != r.kfn ? PGX_KERNELS_FM_REDO : 0u);
        }
        record(b, 8, s);
        if (side_running) HIPCHECK(hipStreamWaitEvent(s, b->ev_side[1], 0)); // the other stream's reads are done (they may have queued heavy reads)
        if (heavy_ext) { // the rest of reads that spent heavy_ext extensions (usually none: the launch then costs a few microseconds)
            b->timing.kernels |= PGX_KERNELS_HEAVY;
            if (b->dimg->lds_bytes)
                hipLaunchKernelGGL(pgx_find_mems_heavy_kernel<true>, dim3(PGX_FM_HEAVY_GRID), dim3(256), b->dimg->lds_bytes, s, r.img, a.reads, a.off,
                                   r.min_len, r.min_occ, a.slot_off, c.slot_base, a.slots, a.cnt, r.ctr, (const pgx_heavy_item *)a.hlist,
                                   (const unsigned long long *)a.hcount, (uint32_t)PGX_FM_HEAVY_CAP, b->heavy_scratch.as<PgxHeavyResult>(), c.r0, cn, a.ovf, a.ovf_cap);
            else
                hipLaunchKernelGGL(pgx_find_mems_heavy_kernel<false>, dim3(PGX_FM_HEAVY_GRID), dim3(256), 0, s, r.img, a.reads, a.off, r.min_len, r.min_occ,
                                   a.slot_off, c.slot_base, a.slots, a.cnt, r.ctr, (const pgx_heavy_item *)a.hlist,
                                   (const unsigned long long *)a.hcount, (uint32_t)PGX_FM_HEAVY_CAP, b->heavy_scratch.as<PgxHeavyResult>(), c.r0, cn, a.ovf, a.ovf_cap);
        }
        if (ovf_cap) hipLaunchKernelGGL(pgx_arena_demand_kernel, dim3(1), dim3(PGX_ARENA_SUBS), 0, s, r.ctr);
        HIPCHECK(hipGetLastError());
        b->timing.find_mems_launches++;
        record(b, 2, s);
        scan_excl(0, b->mem_count.as<uint32_t>() + c.r0, cn, 0, local, b->scan_tmp, s, reinterpret_cast<uint64_t *>(r.ctr + PGX_CTR_MEMS));
        if (r.spec) return r.cm_cap; // nothing is read back: the MEM total stays on the device
        unsigned long long cc[16];
        read_scalars(cc, r.ctr, sizeof cc, s);
        if (ovf_cap) b->last_ovf_used = cc[PGX_CTR_OVF_TOP]; // (what the reads asked for, whether or not it fitted: sizes the next arena)
        if (ovf_cap && cc[PGX_CTR_OVF_ABORT]) { ovf_cap = 0; continue; } // the arena was too small: once more in the worst-case layout
        const bool forced = attempt == 0 && kf != r.kfn_wide && r.k.force_redo; // tests
        if ((cc[PGX_CTR_OVF32] || forced) && kf != r.kfn_wide) { kf = r.kfn_wide; continue; } // a coordinate left 32 bits: repeat the chunk in 64 bits
        r.n_ext += cc[PGX_CTR_EXT];
        b->timing.heavy_reads += (uint32_t)std::min<unsigned long long>(cc[PGX_CTR_HEAVY], PGX_FM_HEAVY_CAP);
        b->timing.pairs_other_steps += (uint32_t)cc[PGX_CTR_REDO];
        return cc[PGX_CTR_MEMS];
    }
}

// 3. the chunk's slots -> the dense MEM array in read order, behind the mem_base MEMs of the chunks before
static void compact_chunk(RunCtx &r, const pgx_chunk &c, uint64_t cm, uint64_t mem_base, uint64_t ovf_cap) {
    pgx_batch *b = r.b;
    hipStream_t s = r.s;
    const uint64_t cn = c.r1 - c.r0;
    b->mems.ensure_keep((mem_base + cm ? mem_base + cm : 1) * sizeof(pgx_mem), mem_base * sizeof(pgx_mem));
    hipLaunchKernelGGL(pgx_compact_mems_kernel, dim3(grid_for(cn, 256)), dim3(256), 0, s, c.r0, cn, b->slot_off.as<uint64_t>(),
                       c.slot_base, b->slots.as<pgx_mem>(), b->mem_count.as<uint32_t>(), (const uint64_t *)(b->mem_off.as<uint64_t>() + c.r0), mem_base,
                       b->mems.as<pgx_mem>(), r.spec ? r.cm_cap : ~0ull, reinterpret_cast<uint64_t *>(r.ctr + PGX_CTR_ABORT),
                       (const uint32_t *)(b->ovf_base.as<uint32_t>() - c.r0), ovf_cap);
    HIPCHECK(hipGetLastError());
    record(b, 3, s);
    if (b->timed && b->chunks.size() > 1) { // events are reused per chunk: accumulate now
        HIPCHECK(hipStreamSynchronize(s));
        float t1 = 0, t2 = 0, t3 = 0;
        HIPCHECK(hipEventElapsedTime(&t1, b->ev[1], b->ev[2]));
        HIPCHECK(hipEventElapsedTime(&t2, b->ev[2], b->ev[3]));
        HIPCHECK(hipEventElapsedTime(&t3, b->ev[1], b->ev[8]));
        r.ms_fm += t1; r.ms_cp += t2; r.ms_main += t3;
    }
}

// 5. the one read-back of all counters behind the pass: the totals of a speculative pass (false: one of its capacities was too small, the pass
//    counts for nothing), the kernels' traffic counters, the shape the next run may assume, the stderr statistics and the times
static bool read_back(RunCtx &r, bool &force_worst) {
    pgx_batch *b = r.b;
    const size_t n_chunks = b->chunks.size();
    unsigned long long cnt[PGX_CTR_SLOTS];
    read_scalars(cnt, b->counters.p, sizeof cnt, r.s);
    if (r.spec) {
        b->spec_runs++;
        if (cnt[PGX_CTR_OVF_ABORT]) { force_worst = true; b->last_ovf_used = cnt[PGX_CTR_OVF_TOP]; } // (the arena sized from the last run overflowed: the next one is sized from this demand)
        if (r.k.debug_counters)
            std::fprintf(stderr, "[pgx] speculative run: abort flags %llu, 32-bit overflow %llu, arena overflow %llu (top %llu), MEMs %llu of capacity %llu\n", cnt[PGX_CTR_ABORT], cnt[PGX_CTR_OVF32],
                         cnt[PGX_CTR_OVF_ABORT], cnt[PGX_CTR_OVF_TOP], cnt[PGX_CTR_MEMS], (unsigned long long)r.cm_cap);
        if (cnt[PGX_CTR_ABORT] || cnt[PGX_CTR_OVF32] || cnt[PGX_CTR_OVF_ABORT] || cnt[PGX_CTR_MEMS] > r.cm_cap) { b->spec_fallbacks++; b->ran_tags = false; return false; } // a capacity was too small: once more, exactly
        b->last_ovf_used = cnt[PGX_CTR_OVF_TOP];
        b->n_mems = cnt[PGX_CTR_MEMS];
        r.n_ext = cnt[PGX_CTR_EXT];
        b->timing.heavy_reads = (uint32_t)std::min<unsigned long long>(cnt[PGX_CTR_HEAVY], PGX_FM_HEAVY_CAP);
        b->timing.pairs_other_steps = (uint32_t)cnt[PGX_CTR_REDO];
        if (r.want_tags) {
            TagWork &w = b->tw;
            const unsigned long long *tc = cnt + PGX_CTR_TAG0; // (scalars of tag_pipeline)
            w.last_big = tc[0]; w.last_large = tc[1]; w.last_largest = tc[2]; w.last_G = tc[3]; w.last_small = tc[5];
            w.last_rep = tc[6]; w.last_dup = tc[7]; w.last_P = tc[8];
            w.n_positions = tc[8];
            b->n_positions = tc[8];
        }
    }
    // the kernels' own traffic counters (accumulated over the chunks of the run)
    if (r.kfn_pairs) {
        b->timing.main_lines = cnt[PGX_CTR_PAIRS_LINES]; b->timing.main_seed_loads = cnt[PGX_CTR_PAIRS_SEEDS];
        b->timing.other_lines = cnt[PGX_CTR_FM_LINES]; b->timing.other_seed_loads = cnt[PGX_CTR_FM_SEEDS];
        b->timing.two_step_trips = cnt[PGX_CTR_PAIRS_TWO];
    } else { b->timing.main_lines = cnt[PGX_CTR_FM_LINES]; b->timing.main_seed_loads = cnt[PGX_CTR_FM_SEEDS]; }
    b->last_mems = b->n_mems;
    b->shape_valid = true; b->shape_reads = r.n; b->shape_min_len = r.min_len; b->shape_min_occ = r.min_occ; b->shape_tags = r.want_tags;
    if (cnt[PGX_CTR_ST_TRIPS] && r.k.fm_stats) // only a -DPGX_FM_STATS build of the kernels fills these (scripts/fm_stats.sh)
        std::fprintf(stderr, "[pgx] find_mems wave trips %llu, live lane-trips %llu (%.1f%% of lanes), longest wave %llu trips, extensions %llu\n", cnt[PGX_CTR_ST_TRIPS],
                     cnt[PGX_CTR_ST_LIVE], 100.0 * (double)cnt[PGX_CTR_ST_LIVE] / (64.0 * (double)cnt[PGX_CTR_ST_TRIPS]), cnt[PGX_CTR_ST_LONGEST], cnt[PGX_CTR_EXT]);
    if (cnt[PGX_CTR_ST_PAIR_TRIPS] && r.k.fm_stats)
        std::fprintf(stderr, "[pgx] pairs kernel wave trips %llu, live lane-trips %llu (%.1f%%), with two extensions %llu, waiting for a second block %llu, fresh %llu, extensions through the other image %llu\n",
                     cnt[PGX_CTR_ST_PAIR_TRIPS], cnt[PGX_CTR_ST_PAIR_LIVE], 100.0 * (double)cnt[PGX_CTR_ST_PAIR_LIVE] / (64.0 * (double)cnt[PGX_CTR_ST_PAIR_TRIPS]),
                     cnt[PGX_CTR_PAIRS_TWO], cnt[PGX_CTR_ST_PAIR_WAIT], cnt[PGX_CTR_ST_PAIR_FRESH], cnt[PGX_CTR_REDO]);
    if (cnt[PGX_CTR_ST_PAIR_T_TOTAL] && r.k.fm_stats)
        std::fprintf(stderr, "[pgx] pairs kernel clock ticks: %.1f%% of the waves' time in the refill loop (%llu of %llu), %llu trips with a refill round; waiting for the seed entry %.1f%%, then for the block line %.1f%%\n",
                     100.0 * (double)cnt[PGX_CTR_ST_PAIR_T_REFILL] / (double)cnt[PGX_CTR_ST_PAIR_T_TOTAL], cnt[PGX_CTR_ST_PAIR_T_REFILL], cnt[PGX_CTR_ST_PAIR_T_TOTAL], cnt[PGX_CTR_ST_PAIR_REFILLS],
                     100.0 * (double)cnt[PGX_CTR_ST_PAIR_T_SEED] / (double)cnt[PGX_CTR_ST_PAIR_T_TOTAL], 100.0 * (double)cnt[PGX_CTR_ST_PAIR_T_LINE] / (double)cnt[PGX_CTR_ST_PAIR_T_TOTAL]);
    if (r.k.debug_counters)
        std::fprintf(stderr, "[pgx] counters: extensions %llu tag overflows %llu heavy %llu other-image steps %llu lines %llu + %llu seeds %llu + %llu\n", cnt[PGX_CTR_EXT], cnt[PGX_CTR_TAG_OVERFLOW],
                     cnt[PGX_CTR_HEAVY], cnt[PGX_CTR_REDO], cnt[PGX_CTR_PAIRS_LINES], cnt[PGX_CTR_FM_LINES], cnt[PGX_CTR_PAIRS_SEEDS], cnt[PGX_CTR_FM_SEEDS]);
    b->n_ext = r.n_ext;
    b->n_tag_overflow = cnt[PGX_CTR_TAG_OVERFLOW];
    if (b->timed) {
        auto el = [&](int a, int c) { float ms = 0; HIPCHECK(hipEventElapsedTime(&ms, b->ev[a], b->ev[c])); return ms; };
        b->timing.ms_find_mems = n_chunks > 1 ? r.ms_fm : el(1, 2);
        b->timing.ms_find_mems_main = n_chunks > 1 ? r.ms_main : (r.n ? el(1, 8) : 0.0f);
        b->timing.ms_compact = n_chunks > 1 ? r.ms_cp : el(2, 3);
        if (r.want_tags) {
            b->timing.ms_tag_locate = el(3, 4); // locate + scans
            b->timing.ms_tag_gather = el(4, 5); // 16-lane small path (gather + sort + unique)
            b->timing.ms_tag_sort = el(5, 6);   // big path + final scan + compaction
        }
        b->timing.ms_total = el(0, 7);
        // what a fresh batch pays before its first find_mems launch (one chunk on the side-stream path: where the passes are)
        if (r.fresh_work) b->timing.ms_per_upload = b->ms_upload_passes + (r.fresh_mark ? el(0, 9) : 0.0f);
    }
    if (r.fresh_work) b->ms_upload_passes = 0; // (reported once)
    return true;
}

// One pass over the batch: scan(cap) -> find_mems -> scan(count) + compact, per chunk -> tag stage -> read-back.
// Speculative sizing: a run normally reads a few scalars back in mid-flight (MEM total, tag-stage totals) because they size
// the next buffers -- each a host synchronisation with the device idle meanwhile.  When the previous run of this batch had the
// same shape (reads, min_len, min_occ, tags), the buffers and grids are sized from ITS totals (+ 25 %), all counts stay on the
// device, capacity checks raise an abort flag there, and the host reads everything once at the end; if the flag came up (or the
// 32-bit state overflowed) the pass returns false and the run is repeated in exact mode.  PGX_SPEC=0 switches it off.
// force_worst: the arena of the speculative pass overflowed, the exact pass uses the worst-case slot layout.
static bool run_pass(RunCtx &r, bool may_speculate, bool &force_worst) {
    pgx_batch *b = r.b;
    hipStream_t s = r.s;
    b->n_mems = b->n_positions = b->n_ext = b->n_tag_overflow = 0;
    std::memset(&b->timing, 0, sizeof b->timing);
    r.fresh_work = r.fresh_mark = false;
    r.n_ext = 0;
    r.ms_fm = r.ms_cp = r.ms_main = 0;
    b->counters.ensure(PGX_CTR_ALL * 8); // layout: PgxCounterSlot (pgx_device.h)
    HIPCHECK(hipMemsetAsync(b->counters.p, 0, PGX_CTR_ALL * 8, s));
    r.ctr = b->counters.as<unsigned long long>();

    record(b, 0, s);
    plan_slots(r);
    const std::vector<pgx_chunk> &chunks = b->chunks;
    // The slot buffer: a dense array of the first four MEMs of every read (PGX_FAST_SLOTS, pgx_slots_device.h pgx_slot_index) + either an ARENA for the
    // fifth and later MEMs (arena_slots), or -- PGX_SLOT_ARENA=0, tiny batches, and the repeat of a chunk whose arena proved too small -- the
    // worst-case region.  Sized per chunk.
    r.arena_on = r.k.arena && !force_worst;
    r.kfn = r.kfn_wide = r.kfn_pairs = nullptr;
    r.cus = 0;
    if (r.n) choose_kernels(r);
    if (r.k.heavy_ext) {
        b->heavy_list.ensure((size_t)PGX_FM_HEAVY_CAP * sizeof(pgx_heavy_item));
        b->heavy_scratch.ensure((size_t)PGX_FM_HEAVY_GRID * PGX_FM_HEAVY_MAXLEN * sizeof(PgxHeavyResult));
    }
    r.spec = may_speculate && chunks.size() == 1 && b->shape_valid && b->shape_reads == r.n && b->shape_min_len == r.min_len && b->shape_min_occ == r.min_occ &&
             b->shape_tags == r.want_tags && (!r.want_tags || (b->tw.have_last && b->tw.last_largest <= PGX_SORT_WG_LDS_CAP)) && r.k.spec && !r.k.force_redo;
    r.cm_cap = with_slack(b->last_mems);
    uint64_t mem_base = 0;
    for (size_t ci = 0; ci < chunks.size(); ci++) {
        record(b, 1, s);
        uint64_t ovf_cap = 0;
        const uint64_t cm = find_mems_chunk(r, ci, ovf_cap);
        compact_chunk(r, chunks[ci], cm, mem_base, ovf_cap);
        mem_base += cm;
    }
    b->n_mems = mem_base;
    if (!r.kfn_pairs) b->timing.pairs_reads = 0u;
    else if (!b->timing.pairs_reads) b->timing.pairs_reads = 1u; // (2 / 3 / 4 when the launch used the packed reads / the cooperative fetches / the LCE image too)
    b->timing.seed_depth = (r.img.seed_k != 0 && r.min_len >= r.img.seed_k && r.img.dense) ? r.img.seed_k : 0u;
    if (chunks.size() != 1) { // global CSR offsets (a single chunk's local offsets already are global)
        if (chunks.empty()) { record(b, 1, s); record(b, 2, s); }
        scan_excl(0, b->mem_count.p, r.n, 0, b->mem_off.as<uint64_t>(), b->scan_tmp, s);
        b->mems.ensure_keep((b->n_mems ? b->n_mems : 1) * sizeof(pgx_mem), b->n_mems * sizeof(pgx_mem));
        record(b, 3, s);
    }
    record(b, 3, s);
    // 4. tag queries (find_mems.cpp:129)
    if (r.want_tags) {
        tag_pipeline(r.img, b->mems.as<pgx_mem>(), nullptr, nullptr, b->n_mems, b->tw, r.ctr + PGX_CTR_TAG_OVERFLOW, r.ctr + PGX_CTR_TAG0, s,
                     [&](int stage) { record(b, 4 + stage, s); }, r.spec, reinterpret_cast<const uint64_t *>(r.ctr + PGX_CTR_MEMS),
                     reinterpret_cast<uint64_t *>(r.ctr + PGX_CTR_ABORT));
        b->n_positions = b->tw.n_positions;
        b->ran_tags = true;
    }
    record(b, 7, s);
    return read_back(r, force_worst);
}

extern "C" pgx_status pgx_batch_run(pgx_batch *b, uint64_t min_len, uint64_t min_occ, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_run");
    if (!b) throw Error(PGX_ERR_ARG, "pgx_batch_run: null batch");
    use_device(b->device);
    RunCtx r{b, batch_stream(b, stream), read_run_knobs(), b->dimg->img, b->n_reads, min_len, min_occ, (flags & PGX_RUN_TAGS) != 0};
    // seeds need min_len >= their depth (no stage of a shorter search has room for one): the shallower table serves searches below the depth of the first
    PgxDevImage &img = r.img;
    if (img.seed_k_main && min_len < img.seed_k_main && img.seed_k_small && min_len >= img.seed_k_small) { img.seed = img.seed_small; img.seed_k = img.seed_k_small; }
    if (r.want_tags && !b->h->has_tags) throw Error(PGX_ERR_ARG, "pgx_batch_run: PGX_RUN_TAGS without a tag array");
    b->timed = (flags & PGX_RUN_TIMING) != 0;
    b->ran = false;
    b->ran_tags = false;
    b->lw.valid = false; // (the locate result belongs to the run before)
    b->hw.valid = false; // (and so do the hits)
    b->pw.valid = false; // (and the places)
    b->vw.valid = false; // (and what was verified at them)
    b->rw.valid = false; // (and rescued next to it)
    b->mw.valid = false; // (and paired from that)
    b->aw.valid = false; // (and aligned there)
    b->ww.valid = false; // (and walked through the graph)
    b->qw.valid = false; // (and the qualities of the placements)
    b->n_mems = b->n_positions = b->n_ext = b->n_tag_overflow = 0;
    std::memset(&b->timing, 0, sizeof b->timing);
    bool force_worst = false;
    if (!run_pass(r, true, force_worst)) run_pass(r, false, force_worst); // (a speculative pass, then at most one exact pass)
    b->ran = true;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_device_result(pgx_batch *b, pgx_device_result *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_device_result: batch has not been run");
    std::memset(out, 0, sizeof *out);
    out->n_reads = b->n_reads;
    out->n_mems = b->n_mems;
    out->mem_offsets = b->mem_off.as<uint64_t>();
    out->mems = b->mems.as<pgx_mem>();
    if (b->ran_tags) {
        out->n_positions = b->n_positions;
        out->tag_run_counts = b->tw.run_nums.as<uint64_t>();
        out->pos_offsets = b->tw.pos_off.as<uint64_t>();
        out->positions = b->tw.positions.as<uint64_t>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_counts(pgx_batch *b, uint64_t *n_mems, uint64_t *n_positions, uint64_t *n_extensions) {
    PGX_GUARD_BEGIN
    if (!b || !b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_counts: batch has not been run");
    if (n_mems) *n_mems = b->n_mems;
    if (n_positions) *n_positions = b->n_positions;
    if (n_extensions) *n_extensions = b->n_ext;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_spec_stats(pgx_batch *b, uint32_t *speculative_runs, uint32_t *fallbacks) {
    PGX_GUARD_BEGIN
    if (!b) throw Error(PGX_ERR_ARG, "pgx_batch_spec_stats: null batch");
    if (speculative_runs) *speculative_runs = b->spec_runs;
    if (fallbacks) *fallbacks = b->spec_fallbacks;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_timing(pgx_batch *b, pgx_timing *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_timing: batch has not been run");
    if (!b->timed) throw Error(PGX_ERR_ARG, "pgx_batch_timing: run without PGX_RUN_TIMING");
    *out = b->timing;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_result(pgx_batch *b, pgx_result *out) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_result");
    if (!b || !out || !b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_result: batch has not been run");
    use_device(b->device);
    const uint64_t n = b->n_reads, m = b->n_mems;
    b->h_mem_off.ensure((n + 1) * 8);
    HIPCHECK(hipMemcpyAsync(b->h_mem_off.p, b->mem_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, b->own));
    b->h_mems.ensure((m ? m : 1) * sizeof(pgx_mem));
    if (m) HIPCHECK(hipMemcpyAsync(b->h_mems.p, b->mems.p, m * sizeof(pgx_mem), hipMemcpyDeviceToHost, b->own));
    std::memset(out, 0, sizeof *out);
    out->n_reads = n;
    out->n_mems = m;
    out->mem_offsets = b->h_mem_off.as<uint64_t>();
    out->mems = b->h_mems.as<pgx_mem>();
    out->n_extensions = b->n_ext;
    if (b->ran_tags) {
        b->h_run_nums.ensure((m ? m : 1) * 8);
        b->h_pos_off.ensure((m + 1) * 8);
        b->h_positions.ensure((b->n_positions ? b->n_positions : 1) * 8);
        if (m) HIPCHECK(hipMemcpyAsync(b->h_run_nums.p, b->tw.run_nums.p, m * 8, hipMemcpyDeviceToHost, b->own));
        HIPCHECK(hipMemcpyAsync(b->h_pos_off.p, b->tw.pos_off.p, (m + 1) * 8, hipMemcpyDeviceToHost, b->own));
        if (b->n_positions) HIPCHECK(hipMemcpyAsync(b->h_positions.p, b->tw.positions.p, b->n_positions * 8, hipMemcpyDeviceToHost, b->own));
        out->tag_run_counts = b->h_run_nums.as<uint64_t>();
        out->pos_offsets = b->h_pos_off.as<uint64_t>();
        out->positions = b->h_positions.as<uint64_t>();
        out->n_positions = b->n_positions;
        out->n_tag_overflow = b->n_tag_overflow;
    }
    HIPCHECK(hipStreamSynchronize(b->own)); // (the run itself completed inside pgx_batch_run, on whatever stream it used)
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
extern "C" pgx_status pgx_find_mems_batch(pgx_index *h, int device, const uint8_t *reads, const uint64_t *offsets,
                                          uint64_t n_reads, uint64_t min_len, uint64_t min_occ, uint32_t flags,
                                          pgx_batch **batch_out, pgx_result *result_out) {
    if (!batch_out || !result_out) { pgx::set_last_error("pgx_find_mems_batch: null argument"); return PGX_ERR_ARG; }
    *batch_out = nullptr;
    pgx_batch *b = nullptr;
    pgx_status st = pgx_batch_create(h, device, reads, offsets, n_reads, &b);
    if (st == PGX_OK) st = pgx_batch_run(b, min_len, min_occ, flags, nullptr);
    if (st == PGX_OK) st = pgx_batch_result(b, result_out);
    if (st != PGX_OK) { pgx_batch_free(b); return st; }
    *batch_out = b;
    return PGX_OK;
}

// reads sharded over devices: contiguous slices, one host thread + batch + stream per slice, the index image
// replicated per device, no collective; slice i covers reads [first_read[i], first_read[i + 1])
extern "C" pgx_status pgx_find_mems_sharded(pgx_index *h, const int *devices, uint32_t n_slices, const uint8_t *reads, const uint64_t *offsets,
                                            uint64_t n_reads, uint64_t min_len, uint64_t min_occ, uint32_t flags, pgx_batch **batches_out,
                                            pgx_result *results_out, uint64_t *first_read) {
    PGX_GUARD_BEGIN
    if (!h || !devices || !n_slices || !offsets || !batches_out || !results_out || !first_read)
        throw Error(PGX_ERR_ARG, "pgx_find_mems_sharded: null argument");
    for (uint32_t i = 0; i < n_slices; i++) { batches_out[i] = nullptr; first_read[i] = n_reads * i / n_slices; }
    first_read[n_slices] = n_reads;
    for (uint32_t i = 0; i < n_slices; i++) (void)device_image(h, devices[i]); // images first: one upload per distinct device
    std::vector<pgx_status> st(n_slices, PGX_OK);
    std::vector<std::string> err(n_slices);
    std::vector<std::thread> th;
    for (uint32_t i = 0; i < n_slices; i++)
        th.emplace_back([&, i]() {
            const uint64_t a = first_read[i], b = first_read[i + 1];
            st[i] = pgx_find_mems_batch(h, devices[i], reads, offsets + a, b - a, min_len, min_occ, flags, &batches_out[i], &results_out[i]);
            if (st[i] != PGX_OK) err[i] = pgx_last_error(); // (the message is thread-local)
        });
    for (auto &t : th) t.join();
    for (uint32_t i = 0; i < n_slices; i++)
        if (st[i] != PGX_OK) {
            for (uint32_t k = 0; k < n_slices; k++) { pgx_batch_free(batches_out[k]); batches_out[k] = nullptr; }
            throw Error(st[i], "slice " + std::to_string(i) + " (device " + std::to_string(devices[i]) + "): " + err[i]);
        }
    return PGX_OK;
    PGX_GUARD_END
}
