// pgx_runtime.hip -- the small things behind the C ABI that every host unit of the runtime uses: device selection, pinned host memory,
// roctx, the device-wide exclusive scan and the scalar read-back; the r-index locate entry points; and the per-call entry points
// (rank, extend, count, lf, find_mems_function, tag_query).  The device images are in pgx_images.hip, the batch pipeline in pgx_batch.hip
// (its other result forms, its locate and the read stages in pgx_batch_forms.hip, pgx_batch_locate.hip, pgx_read_stages.hip), merge_tags / build_tags
// in pgx_tools.hip; pgx_runtime_internal.hpp is what they share.
#include <dlfcn.h>

#include <string>

#include "pgx_runtime_internal.hpp"

const Roctx &roctx() {
    static const Roctx r = [] {
        Roctx x;
        const char *e = std::getenv("PGX_ROCTX");
        if (!e || !std::atoi(e)) return x;
        void *h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return x;
        x.push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
        x.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        x.mark = reinterpret_cast<void (*)(const char *)>(dlsym(h, "roctxMarkA"));
        x.on = x.push && x.pop && x.mark;
        return x;
    }();
    return r;
}

int checked_device_count() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        throw Error(PGX_ERR_NO_DEVICE, "no usable HIP device (libpgx has no CPU fallback)");
    }
    return n;
}

void use_device(int device) {
    int n = checked_device_count();
    if (device < 0 || device >= n) throw Error(PGX_ERR_ARG, "device ordinal out of range");
    HIPCHECK(hipSetDevice(device));
}

extern "C" pgx_status pgx_host_alloc(size_t bytes, void **out) {
    PGX_GUARD_BEGIN
    if (!out) throw Error(PGX_ERR_ARG, "pgx_host_alloc: null argument");
    *out = nullptr;
    (void)checked_device_count();
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable);
    if (e != hipSuccess) { (void)hipGetLastError(); throw Error(PGX_ERR_NOMEM, std::string("hipHostMalloc failed: ") + hipGetErrorString(e)); }
    *out = p;
    return PGX_OK;
    PGX_GUARD_END
}
extern "C" void pgx_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

extern "C" pgx_status pgx_device_count(int *n) {
    PGX_GUARD_BEGIN
    if (!n) throw Error(PGX_ERR_ARG, "pgx_device_count: null argument");
    *n = 0;
    *n = checked_device_count();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_device_name(int device, char *buf, size_t buflen) {
    PGX_GUARD_BEGIN
    if (!buf || !buflen) throw Error(PGX_ERR_ARG, "pgx_device_name: null argument");
    use_device(device);
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, device));
    std::snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// PGX_SCAN_THREE=1: the three-launch form of every scan (partial sums, their scan, apply)
bool scan_three_launches() {
    static const bool three = [] { const char *e = std::getenv("PGX_SCAN_THREE"); return e && e[0] == '1'; }();
    return three;
}
// the tile words of a one-launch scan of nt tiles (decoupled look-back, pgx_scan1_lookback) and the epoch it runs under: the words carry the epoch,
// so the buffer is cleared only when it is new or the 18-bit epoch comes round
static uint32_t scan_onepass_state(DevBuf &tmp, uint64_t nt, hipStream_t s) {
    tmp.ensure((nt + 2) * 8);
    if (tmp.scan_epoch == 0 || tmp.scan_epoch >= 0x3FFFFu) {
        HIPCHECK(hipMemsetAsync(tmp.p, 0, tmp.cap, s));
        tmp.scan_epoch = 0;
        // tests: PGX_SCAN_EPOCH0 = the epoch a cleared buffer starts from (below the last one), so that a few scans reach the wrap
        if (const char *e = std::getenv("PGX_SCAN_EPOCH0")) tmp.scan_epoch = (uint32_t)std::min<unsigned long>(std::strtoul(e, nullptr, 0), 0x3FFFEul);
    }
    return ++tmp.scan_epoch;
}
static void scan_in_three_launches(int mode, const void *in, const void *in2, uint64_t n, uint64_t min_len, uint64_t *out, DevBuf &tmp, hipStream_t s, uint64_t *total_out,
                              const uint64_t *n_dev) {
    const uint64_t nb = (n + PGX_SCAN_BLOCK_ITEMS - 1) / PGX_SCAN_BLOCK_ITEMS;
    tmp.ensure((nb + 1) * 8);
    tmp.scan_epoch = 0; // (the tile words are overwritten)
    uint64_t *sums = tmp.as<uint64_t>();
    hipLaunchKernelGGL(pgx_scan_partial_kernel, dim3((unsigned)nb), dim3(256), 0, s, mode, in, in2, n, min_len, sums, n_dev);
    const int raw = nb <= 2048; // up to 4 M items: no separate scan of the block totals
    if (!raw) hipLaunchKernelGGL(pgx_scan_sums_kernel, dim3(1), dim3(256), 0, s, sums, nb);
    hipLaunchKernelGGL(pgx_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, s, mode, in, in2, n, min_len, (const uint64_t *)sums, nb, out, total_out, raw, n_dev);
    HIPCHECK(hipGetLastError());
}

// exclusive scan helper: out[n+1] on device (out[n] = total); returns nothing, async on `s`
void scan_excl(int mode, const void *in, uint64_t n, uint64_t min_len, uint64_t *out, DevBuf &tmp, hipStream_t s, uint64_t *total_out, const uint64_t *n_dev) {
    if (mode < 0 || mode > 4) throw Error(PGX_ERR_ARG, "scan_excl: unknown mode"); // (mode 5 takes two inputs: scan_tag_tail)
    if (n == 0) {
        HIPCHECK(hipMemsetAsync(out, 0, 8, s));
        if (total_out) HIPCHECK(hipMemsetAsync(total_out, 0, 8, s));
        return;
    }
    if (!scan_three_launches()) { // one launch (pgx_scan_onepass_kernel)
        const uint64_t nt = (n + PGX_SCAN1_TILE_ITEMS - 1) / PGX_SCAN1_TILE_ITEMS;
        const uint32_t ep = scan_onepass_state(tmp, nt, s);
        unsigned long long *st = tmp.as<unsigned long long>();
        switch (mode) {
        case 0: hipLaunchKernelGGL(pgx_scan_onepass_kernel<0>, dim3((unsigned)nt), dim3(256), 0, s, in, n, min_len, out, total_out, n_dev, st, ep); break;
        case 1: hipLaunchKernelGGL(pgx_scan_onepass_kernel<1>, dim3((unsigned)nt), dim3(256), 0, s, in, n, min_len, out, total_out, n_dev, st, ep); break;
        case 2: hipLaunchKernelGGL(pgx_scan_onepass_kernel<2>, dim3((unsigned)nt), dim3(256), 0, s, in, n, min_len, out, total_out, n_dev, st, ep); break;
        case 3: hipLaunchKernelGGL(pgx_scan_onepass_kernel<3>, dim3((unsigned)nt), dim3(256), 0, s, in, n, min_len, out, total_out, n_dev, st, ep); break;
        case 4: hipLaunchKernelGGL(pgx_scan_onepass_kernel<4>, dim3((unsigned)nt), dim3(256), 0, s, in, n, min_len, out, total_out, n_dev, st, ep); break;
        default: break; // (rejected above)
        }
        HIPCHECK(hipGetLastError());
        return;
    }
    scan_in_three_launches(mode, in, nullptr, n, min_len, out, tmp, s, total_out, n_dev);
}

bool scan_tag_tail(const uint64_t *run_nums, const uint64_t *uval, uint64_t n, uint64_t *pos_off, DevBuf &tmp, hipStream_t s, uint64_t *total_out, const uint64_t *n_dev,
                   uint64_t *positions, uint64_t pos_cap, uint64_t *abort) {
    if (n == 0) {
        HIPCHECK(hipMemsetAsync(pos_off, 0, 8, s));
        HIPCHECK(hipMemsetAsync(total_out, 0, 8, s));
        return true;
    }
    if (scan_three_launches()) {
        scan_in_three_launches(5, run_nums, uval, n, 0, pos_off, tmp, s, total_out, n_dev);
        return false;
    }
    const uint64_t nt = (n + PGX_SCAN1_TILE_ITEMS - 1) / PGX_SCAN1_TILE_ITEMS;
    const uint32_t ep = scan_onepass_state(tmp, nt, s);
    hipLaunchKernelGGL(pgx_scan_tag_tail_kernel, dim3((unsigned)nt), dim3(256), 0, s, run_nums, uval, n, n_dev, pos_off, total_out, positions, pos_cap,
                       positions ? abort : nullptr, tmp.as<unsigned long long>(), ep);
    HIPCHECK(hipGetLastError());
    return positions != nullptr;
}

void pgx_use_device(int device) { use_device(device); }
void pgx_scan_u64(const uint64_t *in, uint64_t n, uint64_t *out, uint64_t *tmp, hipStream_t s) {
    if (n == 0) { HIPCHECK(hipMemsetAsync(out, 0, 8, s)); return; }
    const uint64_t nb = (n + PGX_SCAN_BLOCK_ITEMS - 1) / PGX_SCAN_BLOCK_ITEMS;
    hipLaunchKernelGGL(pgx_scan_partial_kernel, dim3((unsigned)nb), dim3(256), 0, s, 1, (const void *)in, (const void *)nullptr, n, (uint64_t)0, tmp, (const uint64_t *)nullptr);
    const int raw = nb <= 2048;
    if (!raw) hipLaunchKernelGGL(pgx_scan_sums_kernel, dim3(1), dim3(256), 0, s, tmp, nb);
    hipLaunchKernelGGL(pgx_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, s, 1, (const void *)in, (const void *)nullptr, n, (uint64_t)0, (const uint64_t *)tmp, nb, out, (uint64_t *)nullptr, raw, (const uint64_t *)nullptr);
    HIPCHECK(hipGetLastError());
}

// scalars the host needs to size the next buffer: device -> a small pinned buffer (a pageable destination makes every such
// copy a staged, blocking transfer) -> caller.  One buffer per host thread.
void read_scalars(void *dst, const void *dptr, size_t bytes, hipStream_t s) {
    static thread_local void *pin = nullptr;
    if (!pin) HIPCHECK(hipHostMalloc(&pin, 512, hipHostMallocPortable));
    if (bytes > 512) throw Error(PGX_ERR_ARG, "read_scalars: too many bytes");
    HIPCHECK(hipMemcpyAsync(pin, dptr, bytes, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    std::memcpy(dst, pin, bytes);
}

extern "C" pgx_status pgx_locate_next_batch(pgx_index *h, int device, const uint64_t *prev, uint64_t n, uint64_t *out) {
    PGX_GUARD_BEGIN
    if (!h || (n && (!prev || !out))) throw Error(PGX_ERR_ARG, "pgx_locate_next_batch: null argument");
    pgx_device_image *d = locate_image(h, device);
    if (!n) return PGX_OK;
    DevBuf di, dout;
    try {
        di.ensure(n * 8); dout.ensure(n * 8);
        HIPCHECK(hipMemcpy(di.p, prev, n * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(pgx_locate_next_kernel, dim3(grid_for(n, 256)), dim3(256), 0, nullptr, d->loc, di.as<uint64_t>(), n,
                           dout.as<uint64_t>());
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpy(out, dout.p, n * 8, hipMemcpyDeviceToHost));
    } catch (...) {
        di.release(); dout.release();
        throw;
    }
    di.release(); dout.release();
    return PGX_OK;
    PGX_GUARD_END
}

// the walk + optional segmented sort-unique; results stay in w_vals (values) / h_off (host offsets)
void locate_core(pgx_index *h, pgx_device_image *d, const uint64_t *first, const uint64_t *last, uint64_t n, uint32_t flags,
                 std::vector<uint64_t> &h_off, DevBuf &vals_out, uint64_t &n_vals_out) {
    const uint64_t bwt_n = d->loc.n;
    std::vector<uint64_t> cnt(n), voff(n + 1);
    voff[0] = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (last[i] < first[i]) cnt[i] = 0;
        else {
            if (last[i] >= bwt_n) throw Error(PGX_ERR_ARG, "pgx_locate_batch: range " + std::to_string(i) + " ends beyond the BWT");
            cnt[i] = last[i] - first[i] + 1;
        }
        voff[i + 1] = voff[i] + cnt[i];
    }
    const uint64_t V = voff[n];
    DevBuf dqs, dqe, drun0, dnp, dpoff, dvoff, dcnt, scan_tmp, dlist, dneed, dsoff, dscratch, ducount, duoff;
    DevBuf *all[] = {&dqs, &dqe, &drun0, &dnp, &dpoff, &dvoff, &dcnt, &scan_tmp, &dlist, &dneed, &dsoff, &dscratch, &ducount, &duoff};
    DevBuf gbuf;
    try {
        hipStream_t s = nullptr;
        dqs.ensure(n * 8); dqe.ensure(n * 8); drun0.ensure(n * 8); dnp.ensure(n * 8); dpoff.ensure((n + 1) * 8); dvoff.ensure((n + 1) * 8);
        HIPCHECK(hipMemcpy(dqs.p, first, n * 8, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(dqe.p, last, n * 8, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(dvoff.p, voff.data(), (n + 1) * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(pgx_locate_plan_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, d->loc, dqs.as<uint64_t>(), dqe.as<uint64_t>(), n,
                           drun0.as<uint64_t>(), dnp.as<uint64_t>());
        HIPCHECK(hipGetLastError());
        scan_excl(1, dnp.p, n, 0, dpoff.as<uint64_t>(), scan_tmp, s);
        const uint64_t n_pieces = read_u64(dpoff.as<uint64_t>() + n, s);
        gbuf.ensure((V ? V : 1) * 8);
        if (n_pieces) {
            hipLaunchKernelGGL(pgx_locate_walk_kernel, dim3(grid_for(n_pieces, 256)), dim3(256), 0, s, d->loc, dqs.as<uint64_t>(),
                               dqe.as<uint64_t>(), n, drun0.as<uint64_t>(), dpoff.as<uint64_t>(), n_pieces, dvoff.as<uint64_t>(), (uint64_t)0,
                               (flags & PGX_LOCATE_SEQ_IDS) ? 1 : 0, gbuf.as<uint64_t>());
            HIPCHECK(hipGetLastError());
        }
        if (!(flags & PGX_LOCATE_UNIQUE)) {
            HIPCHECK(hipStreamSynchronize(s));
            h_off = voff;
            vals_out = gbuf; gbuf = DevBuf();
            n_vals_out = V;
        } else {
            // segmented sort + unique with the tag path's kernels: one wave per segment up to 2048 values, one
            // 1024-thread workgroup beyond (LDS up to 16384 values, global scratch above)
            std::vector<uint64_t> wave_list, wg_list, need(n, 0), soff(n + 1, 0);
            uint64_t max_cnt = 0;
            for (uint64_t i = 0; i < n; i++) {
                if (cnt[i] == 0) continue;
                if (cnt[i] <= PGX_SORT_LDS_CAP) wave_list.push_back(i);
                else {
                    wg_list.push_back(i);
                    max_cnt = std::max(max_cnt, cnt[i]);
                    uint64_t p2 = 64;
                    while (p2 < cnt[i]) p2 <<= 1;
                    if (p2 > PGX_SORT_WG_LDS_CAP) need[i] = p2;
                }
            }
            for (uint64_t i = 0; i < n; i++) soff[i + 1] = soff[i] + need[i];
            dcnt.ensure(n * 8); ducount.ensure(n * 8); duoff.ensure((n + 1) * 8);
            dlist.ensure((n ? n : 1) * 8); dsoff.ensure((n + 1) * 8); dscratch.ensure((soff[n] ? soff[n] : 1) * 8);
            HIPCHECK(hipMemcpy(dcnt.p, cnt.data(), n * 8, hipMemcpyHostToDevice));
            HIPCHECK(hipMemset(ducount.p, 0, n * 8)); // empty ranges are on no list
            HIPCHECK(hipMemcpy(dsoff.p, soff.data(), (n + 1) * 8, hipMemcpyHostToDevice));
            uint64_t *d_wave = dlist.as<uint64_t>(), *d_wg = d_wave + wave_list.size();
            if (!wave_list.empty()) HIPCHECK(hipMemcpy(d_wave, wave_list.data(), wave_list.size() * 8, hipMemcpyHostToDevice));
            if (!wg_list.empty()) HIPCHECK(hipMemcpy(d_wg, wg_list.data(), wg_list.size() * 8, hipMemcpyHostToDevice));
            if (!wave_list.empty())
                hipLaunchKernelGGL(pgx_tag_sort_unique_kernel<PgxTagDense>, dim3(grid_for(wave_list.size(), 4)), dim3(256), 0, s,
                                   PgxTagDense{d_wave, dcnt.as<uint64_t>(), dvoff.as<uint64_t>()}, (uint64_t)wave_list.size(), (const uint64_t *)nullptr,
                                   (const uint64_t *)nullptr, gbuf.as<uint64_t>(), ducount.as<uint64_t>());
            if (!wg_list.empty()) {
                uint64_t p2max = 64;
                while (p2max < max_cnt && p2max < PGX_SORT_WG_LDS_CAP) p2max <<= 1;
                HIPCHECK(hipFuncSetAttribute((const void *)pgx_tag_sort_large_kernel<PgxTagDense>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(PGX_SORT_WG_LDS_CAP * 8)));
                hipLaunchKernelGGL(pgx_tag_sort_large_kernel<PgxTagDense>, dim3(grid_for(wg_list.size(), 1)), dim3(1024), (size_t)p2max * 8, s,
                                   PgxTagDense{d_wg, dcnt.as<uint64_t>(), dvoff.as<uint64_t>()}, (uint64_t)wg_list.size(), (const uint64_t *)nullptr,
                                   (const uint64_t *)nullptr, gbuf.as<uint64_t>(), dscratch.as<uint64_t>(), (const uint64_t *)dsoff.as<uint64_t>(), ducount.as<uint64_t>());
            }
            HIPCHECK(hipGetLastError());
            scan_excl(1, ducount.p, n, 0, duoff.as<uint64_t>(), scan_tmp, s);
            const uint64_t U = read_u64(duoff.as<uint64_t>() + n, s);
            vals_out.ensure((U ? U : 1) * 8);
            hipLaunchKernelGGL(pgx_tag_compact_kernel<PgxTagDense>, dim3(grid_for(n, 16)), dim3(256), 0, s, PgxTagDense{nullptr, nullptr, dvoff.as<uint64_t>()}, n,
                               (const uint64_t *)nullptr, (const uint64_t *)nullptr, (const uint64_t *)ducount.as<uint64_t>(), (const uint64_t *)gbuf.as<uint64_t>(),
                               (const uint64_t *)duoff.as<uint64_t>(), vals_out.as<uint64_t>(), ~0ull);
            HIPCHECK(hipGetLastError());
            h_off.resize(n + 1);
            HIPCHECK(hipMemcpy(h_off.data(), duoff.p, (n + 1) * 8, hipMemcpyDeviceToHost));
            n_vals_out = U;
        }
    } catch (...) {
        for (DevBuf *b : all) b->release();
        gbuf.release();
        throw;
    }
    for (DevBuf *b : all) b->release();
    gbuf.release();
}

void locate_check_supported(const pgx_index *h, const char *who) {
    if (h->mode == PGX_MODE_COMPAT && h->meta.encoded && !h->meta.hasN)
        throw Error(PGX_ERR_UNSUPPORTED, std::string(who) + ": the reference's encoded run scan skips six header varints where five were "
                                         "written on an index without N (src/r-index.cpp:83-88); open the index in PGX_MODE_STRICT");
}

extern "C" pgx_status pgx_locate_batch(pgx_index *h, int device, const uint64_t *first, const uint64_t *last, uint64_t n, uint32_t flags,
                                       uint64_t *val_offsets, uint64_t *values, uint64_t values_cap) {
    PGX_GUARD_BEGIN
    if (!h || !val_offsets || (n && (!first || !last))) throw Error(PGX_ERR_ARG, "pgx_locate_batch: null argument");
    if (flags & ~(PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE)) throw Error(PGX_ERR_ARG, "pgx_locate_batch: unknown flag");
    if (!h->has_rank) throw Error(PGX_ERR_ARG, "pgx_locate_batch: index opened without an r-index");
    locate_check_supported(h, "pgx_locate_batch");
    pgx_device_image *d = locate_image(h, device);
    val_offsets[0] = 0;
    if (!n) return PGX_OK;
    std::vector<uint64_t> off;
    DevBuf vals;
    uint64_t nv = 0;
    try {
        locate_core(h, d, first, last, n, flags, off, vals, nv);
        std::copy(off.begin(), off.end(), val_offsets);
        if (values) {
            if (values_cap < nv) throw Error(PGX_ERR_ARG, "pgx_locate_batch: values_cap too small");
            if (nv) HIPCHECK(hipMemcpy(values, vals.p, nv * 8, hipMemcpyDeviceToHost));
        }
    } catch (...) {
        vals.release();
        throw;
    }
    vals.release();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_decompress_sa(pgx_index *h, int device, uint32_t flags, uint64_t *out) {
    PGX_GUARD_BEGIN
    if (!h || !out) throw Error(PGX_ERR_ARG, "pgx_decompress_sa: null argument");
    if (flags & ~PGX_LOCATE_SEQ_IDS) throw Error(PGX_ERR_ARG, "pgx_decompress_sa: unknown flag");
    pgx_device_image *d = locate_image(h, device); // run boundaries come from the parsed blocks, not from the reference's scan
    if (!d->loc.n) return PGX_OK;
    const uint64_t first = 0, last = d->loc.n - 1;
    std::vector<uint64_t> off;
    DevBuf vals;
    uint64_t nv = 0;
    try {
        locate_core(h, d, &first, &last, 1, flags, off, vals, nv);
        HIPCHECK(hipMemcpy(out, vals.p, nv * 8, hipMemcpyDeviceToHost));
    } catch (...) {
        vals.release();
        throw;
    }
    vals.release();
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// primitives (tests)
extern "C" pgx_status pgx_rank_batch(pgx_index *h, int device, const uint64_t *pos, uint64_t n, int true_codes, uint64_t *out) {
    PGX_GUARD_BEGIN
    if (!h || (n && (!pos || !out))) throw Error(PGX_ERR_ARG, "pgx_rank_batch: null argument");
    if (!h->has_rank) throw Error(PGX_ERR_ARG, "pgx_rank_batch: index opened without an r-index");
    pgx_device_image *d = device_image(h, device);
    if (!n) return PGX_OK;
    DevBuf dp, dout;
    try {
        dp.ensure(n * 8);
        dout.ensure(n * 48);
        HIPCHECK(hipMemcpy(dp.p, pos, n * 8, hipMemcpyHostToDevice));
        HIPCHECK(hipMemset(dout.p, 0, n * 48));
        const char *probe = std::getenv("PGX_RANK_PROBE"); // scripts/anomaly_probe.py: the round-3 shapes of this kernel (wide dense2 image, true codes)
        if (probe && d->img.dense == 3 && true_codes) {
            const std::string v(probe);
            if (v == "loop_mulhi") hipLaunchKernelGGL((pgx_rank_probe_kernel<true, true>), dim3(grid_for(n, 256)), dim3(256), 0, 0, d->img, dp.as<uint64_t>(), n, dout.as<uint64_t>());
            else if (v == "loop") hipLaunchKernelGGL((pgx_rank_probe_kernel<true, false>), dim3(grid_for(n, 256)), dim3(256), 0, 0, d->img, dp.as<uint64_t>(), n, dout.as<uint64_t>());
            else if (v == "mulhi") hipLaunchKernelGGL((pgx_rank_probe_kernel<false, true>), dim3(grid_for(6 * n, 256)), dim3(256), 0, 0, d->img, dp.as<uint64_t>(), n, dout.as<uint64_t>());
            else throw Error(PGX_ERR_ARG, "PGX_RANK_PROBE: loop_mulhi | loop | mulhi");
        } else
        hipLaunchKernelGGL(pgx_rank_kernel, dim3(grid_for(6 * n, 256)), dim3(256), 0, 0, d->img, dp.as<uint64_t>(), n, true_codes, dout.as<uint64_t>());
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpy(out, dout.p, n * 48, hipMemcpyDeviceToHost));
    } catch (...) { dp.release(); dout.release(); throw; }
    dp.release(); dout.release();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_extend_batch(pgx_index *h, int device, const pgx_biint *in, const uint8_t *sym, const uint8_t *forward,
                                       uint64_t n, pgx_biint *out) {
    PGX_GUARD_BEGIN
    if (!h || (n && (!in || !sym || !forward || !out))) throw Error(PGX_ERR_ARG, "pgx_extend_batch: null argument");
    if (!h->has_rank) throw Error(PGX_ERR_ARG, "pgx_extend_batch: index opened without an r-index");
    pgx_device_image *d = device_image(h, device);
    if (!n) return PGX_OK;
    DevBuf din, dsym, dfw, dout;
    try {
        din.ensure(n * sizeof(pgx_biint)); dsym.ensure(n); dfw.ensure(n); dout.ensure(n * sizeof(pgx_biint));
        HIPCHECK(hipMemcpy(din.p, in, n * sizeof(pgx_biint), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(dsym.p, sym, n, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(dfw.p, forward, n, hipMemcpyHostToDevice));
        if (d->lds_bytes)
            hipLaunchKernelGGL(pgx_extend_kernel<true>, dim3(grid_for(n, 256)), dim3(256), d->lds_bytes, 0, d->img, din.as<pgx_biint>(),
                               dsym.as<uint8_t>(), dfw.as<uint8_t>(), n, dout.as<pgx_biint>());
        else
            hipLaunchKernelGGL(pgx_extend_kernel<false>, dim3(grid_for(n, 256)), dim3(256), 0, 0, d->img, din.as<pgx_biint>(),
                               dsym.as<uint8_t>(), dfw.as<uint8_t>(), n, dout.as<pgx_biint>());
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpy(out, dout.p, n * sizeof(pgx_biint), hipMemcpyDeviceToHost));
    } catch (...) { din.release(); dsym.release(); dfw.release(); dout.release(); throw; }
    din.release(); dsym.release(); dfw.release(); dout.release();
    return PGX_OK;
    PGX_GUARD_END
}

// COMPAT count_encoded / LF_encoded on an encoded index without N go through the literal image (pgx_images.hip literal_image;
// pgx_host.hpp literal_count says when)
extern "C" pgx_status pgx_count_batch(pgx_index *h, int device, const uint8_t *reads, const uint64_t *offsets, uint64_t n_reads,
                                      pgx_range *out) {
    PGX_GUARD_BEGIN
    if (!h || !offsets || (n_reads && (!out || (!reads && offsets[n_reads] != offsets[0]))))
        throw Error(PGX_ERR_ARG, "pgx_count_batch: null argument");
    if (!h->has_rank) throw Error(PGX_ERR_ARG, "pgx_count_batch: index opened without an r-index");
    const bool lit = literal_count(h);
    pgx_device_image *d = lit ? literal_image(h, device) : device_image(h, device);
    if (!n_reads) return PGX_OK;
    DevBuf dr, doff, dout;
    try {
        const uint64_t lo = offsets[0], bytes = offsets[n_reads] - lo;
        std::vector<uint64_t> reb(n_reads + 1);
        for (uint64_t i = 0; i <= n_reads; i++) {
            if (i && offsets[i] < offsets[i - 1]) throw Error(PGX_ERR_ARG, "pgx_count_batch: offsets must be non-decreasing");
            reb[i] = offsets[i] - lo;
        }
        dr.ensure(bytes + 16); doff.ensure((n_reads + 1) * 8); dout.ensure(n_reads * sizeof(pgx_range));
        if (bytes) HIPCHECK(hipMemcpy(dr.p, reads + lo, bytes, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(doff.p, reb.data(), (n_reads + 1) * 8, hipMemcpyHostToDevice));
        if (lit)
            hipLaunchKernelGGL(pgx_lit_count_kernel, dim3(grid_for(n_reads, 256)), dim3(256), 0, 0, d->lit, (const uint8_t *)dr.as<uint8_t>(),
                               (const uint64_t *)doff.as<uint64_t>(), (const pgx_range *)nullptr, (const uint8_t *)nullptr, n_reads, dout.as<pgx_range>());
        else if (d->lds_bytes)
            hipLaunchKernelGGL(pgx_count_kernel<true>, dim3(grid_for(n_reads, 256)), dim3(256), d->lds_bytes, 0, d->img, dr.as<uint8_t>(),
                               doff.as<uint64_t>(), n_reads, dout.as<pgx_range>());
        else
            hipLaunchKernelGGL(pgx_count_kernel<false>, dim3(grid_for(n_reads, 256)), dim3(256), 0, 0, d->img, dr.as<uint8_t>(),
                               doff.as<uint64_t>(), n_reads, dout.as<pgx_range>());
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpy(out, dout.p, n_reads * sizeof(pgx_range), hipMemcpyDeviceToHost));
    } catch (...) { dr.release(); doff.release(); dout.release(); throw; }
    dr.release(); doff.release(); dout.release();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_find_mems_function_batch(pgx_index *h, int device, const uint8_t *reads, const uint64_t *offsets, uint64_t n_reads,
                                                    const uint64_t *read_of, const uint64_t *x, uint64_t n, uint64_t min_len, uint64_t min_occ,
                                                    uint64_t *next_x, pgx_mem *mem, uint8_t *has_mem, uint64_t *n_ext) {
    PGX_GUARD_BEGIN
    if (!h || !offsets || (n && (!read_of || !x || !next_x || !mem || !has_mem))) throw Error(PGX_ERR_ARG, "pgx_find_mems_function_batch: null argument");
    if (!h->has_rank) throw Error(PGX_ERR_ARG, "pgx_find_mems_function_batch: index opened without an r-index");
    pgx_device_image *d = device_image(h, device);
    if (!n) return PGX_OK;
    for (uint64_t i = 0; i < n_reads; i++) {
        if (offsets[i + 1] < offsets[i]) throw Error(PGX_ERR_ARG, "pgx_find_mems_function_batch: offsets must be non-decreasing");
        if (offsets[i + 1] - offsets[i] >= (1ull << 31)) throw Error(PGX_ERR_UNSUPPORTED, "read longer than 2^31 bytes");
    }
    for (uint64_t i = 0; i < n; i++)
        if (read_of[i] >= n_reads) throw Error(PGX_ERR_ARG, "pgx_find_mems_function_batch: read index out of range");
    DevBuf dr, doff, dro, dx, dout;
    DevBuf *all[] = {&dr, &doff, &dro, &dx, &dout};
    try {
        const uint64_t lo = offsets[0], bytes = offsets[n_reads] - lo;
        if (bytes && !reads) throw Error(PGX_ERR_ARG, "pgx_find_mems_function_batch: null reads");
        std::vector<uint64_t> reb(n_reads + 1);
        for (uint64_t i = 0; i <= n_reads; i++) reb[i] = offsets[i] - lo;
        dr.ensure(bytes + 32); doff.ensure((n_reads + 1) * 8); dro.ensure(n * 8); dx.ensure(n * 8); dout.ensure(n * sizeof(PgxHeavyResult));
        HIPCHECK(hipMemset((uint8_t *)dr.p + bytes, 0, 32));
        if (bytes) HIPCHECK(hipMemcpy(dr.p, reads + lo, bytes, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(doff.p, reb.data(), (n_reads + 1) * 8, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(dro.p, read_of, n * 8, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(dx.p, x, n * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(pgx_fmf_kernel, dim3(grid_for(n, 256)), dim3(256), 0, 0, d->img, dr.as<uint8_t>(), doff.as<uint64_t>(), dro.as<uint64_t>(),
                           dx.as<uint64_t>(), n, min_len, min_occ, dout.as<PgxHeavyResult>());
        HIPCHECK(hipGetLastError());
        std::vector<PgxHeavyResult> res(n);
        HIPCHECK(hipMemcpy(res.data(), dout.p, n * sizeof(PgxHeavyResult), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; i++) {
            next_x[i] = res[i].next_x; mem[i] = res[i].mem; has_mem[i] = (uint8_t)res[i].has_mem;
            if (n_ext) n_ext[i] = res[i].n_ext;
        }
    } catch (...) { for (DevBuf *b : all) b->release(); throw; }
    for (DevBuf *b : all) b->release();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_lf_batch(pgx_index *h, int device, const pgx_range *in, const uint8_t *sym, uint64_t n, pgx_range *out) {
    PGX_GUARD_BEGIN
    if (!h || (n && (!in || !sym || !out))) throw Error(PGX_ERR_ARG, "pgx_lf_batch: null argument");
    if (!h->has_rank) throw Error(PGX_ERR_ARG, "pgx_lf_batch: index opened without an r-index");
    const bool lit = literal_count(h);
    pgx_device_image *d = lit ? literal_image(h, device) : device_image(h, device);
    if (!n) return PGX_OK;
    DevBuf din, dsym, dout;
    try {
        din.ensure(n * sizeof(pgx_range)); dsym.ensure(n); dout.ensure(n * sizeof(pgx_range));
        HIPCHECK(hipMemcpy(din.p, in, n * sizeof(pgx_range), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(dsym.p, sym, n, hipMemcpyHostToDevice));
        if (lit)
            hipLaunchKernelGGL(pgx_lit_count_kernel, dim3(grid_for(n, 256)), dim3(256), 0, 0, d->lit, (const uint8_t *)nullptr, (const uint64_t *)nullptr,
                               (const pgx_range *)din.as<pgx_range>(), (const uint8_t *)dsym.as<uint8_t>(), n, dout.as<pgx_range>());
        else
            hipLaunchKernelGGL(pgx_lf_kernel, dim3(grid_for(n, 256)), dim3(256), 0, 0, d->img, din.as<pgx_range>(), dsym.as<uint8_t>(), n, dout.as<pgx_range>());
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpy(out, dout.p, n * sizeof(pgx_range), hipMemcpyDeviceToHost));
    } catch (...) { din.release(); dsym.release(); dout.release(); throw; }
    din.release(); dsym.release(); dout.release();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_tag_query_batch(pgx_index *h, int device, const uint64_t *start, const uint64_t *end, uint64_t n,
                                          uint64_t *run_nums, uint64_t *pos_offsets, uint64_t *positions, uint64_t positions_cap,
                                          uint64_t *n_overflow) {
    PGX_GUARD_BEGIN
    if (!h || !pos_offsets || (n && (!start || !end || !run_nums))) throw Error(PGX_ERR_ARG, "pgx_tag_query_batch: null argument");
    if (!h->has_tags) throw Error(PGX_ERR_ARG, "pgx_tag_query_batch: index opened without a tag array");
    pgx_device_image *d = device_image(h, device);
    pos_offsets[0] = 0;
    if (n_overflow) *n_overflow = 0;
    if (!n) return PGX_OK;
    DevBuf ds, de, dctr;
    TagWork w;
    try {
        hipStream_t s = nullptr;
        ds.ensure(n * 8); de.ensure(n * 8); dctr.ensure(256);
        HIPCHECK(hipMemset(dctr.p, 0, 256));
        HIPCHECK(hipMemcpy(ds.p, start, n * 8, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(de.p, end, n * 8, hipMemcpyHostToDevice));
        unsigned long long *ctr = dctr.as<unsigned long long>();
        tag_pipeline(d->img, nullptr, ds.as<uint64_t>(), de.as<uint64_t>(), n, w, ctr, ctr + 1, s, [](int) {});
        HIPCHECK(hipMemcpy(run_nums, w.run_nums.p, n * 8, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(pos_offsets, w.pos_off.p, (n + 1) * 8, hipMemcpyDeviceToHost));
        if (positions) {
            if (positions_cap < w.n_positions) throw Error(PGX_ERR_ARG, "pgx_tag_query_batch: positions_cap too small");
            if (w.n_positions) HIPCHECK(hipMemcpy(positions, w.positions.p, w.n_positions * 8, hipMemcpyDeviceToHost));
        }
        if (n_overflow) {
            unsigned long long c = 0;
            HIPCHECK(hipMemcpy(&c, dctr.p, 8, hipMemcpyDeviceToHost));
            *n_overflow = c;
        }
    } catch (...) {
        ds.release(); de.release(); dctr.release(); w.release();
        throw;
    }
    ds.release(); de.release(); dctr.release(); w.release();
    return PGX_OK;
    PGX_GUARD_END
}
