// pgx_images.hip -- the device images of an index: the rank image with its seed tables, tag runs and PAIRS blocks (device_image), and what is
// added on first use: the locate image (locate_image), the LCE image (ensure_lce), the text image (ensure_text), the walk image (ensure_walk) and the literal count image
// (literal_image).
#include <chrono>
#include <memory>
#include <mutex>

#include "pgx_runtime_internal.hpp"

// The environment variables that shape an image, read in one place when the image is built (device_image: the seed tables and the tag runs;
// ensure_lce: the LCE image) -- never later: an image keeps the shape it was built with.  What a run consults is in pgx_batch.hip (RunKnobs).
struct ImageKnobs {
    bool has_seed_k;     // PGX_SEED_K is set, and
    int seed_k;          //   its value (atoi): depth of the k-mer seed table, below 2 = no table
    bool has_seed_end_k; // PGX_SEED_END_K is set, and
    int seed_end_k;      //   its value (atoi, held to [0, 12]): depth of the end table
    bool tpair;          // PGX_NO_TPAIR set at all clears it: no (start, value) pairs of the tag runs
    bool tbucket;        // PGX_NO_TBUCKET set at all clears it: no bucket lines of the tag runs
    bool lce;            // PGX_FM_LCE=0 clears it: no LCE image
    bool lcp;            // PGX_FM_LCP=0 clears it: no table of common prefixes next to the LCE image (every occurrence is compared with the text)
    bool has_lce_max;    // PGX_FM_LCE_MAX is set, and
    uint32_t lce_max;    //   its value (strtoul, at most PGX_LCE_MAX_OCC): widest interval that takes the text path
    bool has_refill_min; // PGX_FM_REFILL_MIN is set, and
    uint32_t refill_min; //   its value (strtoul, held to [1, 64]): idle lanes a wave of the LCE kernel gathers before it fetches new reads
};

static ImageKnobs read_image_knobs() {
    auto not_zero = [](const char *name) { const char *e = std::getenv(name); return !(e && e[0] == '0'); };
    ImageKnobs k{};
    if (const char *e = std::getenv("PGX_SEED_K")) { k.has_seed_k = true; k.seed_k = std::atoi(e); }
    if (const char *e = std::getenv("PGX_SEED_END_K")) { k.has_seed_end_k = true; k.seed_end_k = std::max(0, std::min(std::atoi(e), 12)); }
    k.tpair = !std::getenv("PGX_NO_TPAIR");
    k.tbucket = !std::getenv("PGX_NO_TBUCKET");
    k.lce = not_zero("PGX_FM_LCE");
    k.lcp = not_zero("PGX_FM_LCP");
    if (const char *e = std::getenv("PGX_FM_LCE_MAX")) { k.has_lce_max = true; k.lce_max = (uint32_t)std::min<unsigned long>(std::strtoul(e, nullptr, 10), (unsigned long)PGX_LCE_MAX_OCC); }
    if (const char *e = std::getenv("PGX_FM_REFILL_MIN")) { k.has_refill_min = true; k.refill_min = (uint32_t)std::max<unsigned long>(1ul, std::min<unsigned long>(std::strtoul(e, nullptr, 10), 64ul)); }
    return k;
}

static void release_locate_buffers(pgx_device_image *d) {
    d->rstart.release(); d->rsamp.release(); d->rdir.release(); d->lpos.release(); d->lnext.release(); d->ldir.release();
}
static void release_literal_buffers(pgx_device_image *d) {
    d->lit_bstart.release(); d->lit_cum.release(); d->lit_runs.release(); d->lit_roff.release(); d->lit_tabs.release();
}
// every device buffer of an image (the current device is the image's)
static void release_buffers(pgx_device_image *d) {
    d->blocks.release(); d->dir.release(); d->blow.release(); d->consts.release();
    d->tstart.release(); d->tvals.release(); d->tdir.release(); d->tpair.release(); d->tbucket.release(); d->seed.release(); d->seed_small.release(); d->seed_end.release(); d->exc.release(); d->pairs.release(); d->first_ext.release(); d->sbase2.release(); d->pbase.release();
    release_literal_buffers(d);
    release_locate_buffers(d);
    d->lce_sa.release(); d->lce_text.release(); d->lce_flags.release(); d->lce_lcp.release(); d->lce_seq_start.release();
    d->text4.release(); d->text_seq_start.release();
    d->walk_bits.release(); d->walk_dir.release(); d->walk_nodes.release();
}

// ------------------------------------------------------------------------------------------
// The device side of the image file's integrity check (include/pgx.h "image file").  A handle opened from an image has not summed its
// sections on the host (unless asked to): the device does, at memory speed, over the bytes it has just received and before any other
// kernel reads them -- the seed table builder, pgx_first_ext_kernel, the tag pair and bucket kernels and ensure_lce all index these
// buffers unchecked.  One pgx_image_sum_kernel per section on the stream of the uploads (the null stream: hipMemcpy orders them), the
// sums side by side in one small buffer, ONE synchronising read-back at the end.  A handle opened from .ri / tags runs none of this.
struct SectionSums {
    const pgx_index *h;
    DevBuf sums;
    std::vector<uint32_t> ids;
    // PGX_IMAGE_TIMING=1 (scripts/open_image_bench.py): HIP events around every sum kernel; their total and the bytes summed
    bool timed = false;
    std::vector<hipEvent_t> ev;
    uint64_t bytes_summed = 0;
    float ms_sums = 0;
    explicit SectionSums(const pgx_index *h_) : h(h_) {
        if (!h->from_image) return;
        timed = std::getenv("PGX_IMAGE_TIMING") != nullptr;
        sums.ensure(PGX_IMAGE_MAX_SECTIONS * 8);
        HIPCHECK(hipMemsetAsync(sums.p, 0, PGX_IMAGE_MAX_SECTIONS * 8, nullptr));
    }
    ~SectionSums() {
        sums.release();
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    void mark() {
        if (!timed) return;
        hipEvent_t e = nullptr;
        HIPCHECK(hipEventCreate(&e));
        ev.push_back(e);
        HIPCHECK(hipEventRecord(e, nullptr));
    }
    SectionSums(const SectionSums &) = delete;
    SectionSums &operator=(const SectionSums &) = delete;
    // the upload of section `id` (bytes of it, as the file's table has them) sits in b: launch its sum
    void add(uint32_t id, const DevBuf &b) {
        if (!h->from_image) return;
        const ImageSection *sec = h->section(id);
        if (!sec) throw Error(PGX_ERR_FORMAT, std::string("image file: section ") + pgx_image_section_name(id) + " is not in the file's table");
        if (ids.size() >= PGX_IMAGE_MAX_SECTIONS || sec->bytes > b.cap) throw Error(PGX_ERR_ARG, "image check: section does not fit its device buffer");
        mark();
        launch_image_sum(b.p, sec->bytes, sums.as<unsigned long long>() + ids.size(), nullptr);
        mark();
        bytes_summed += sec->bytes;
        ids.push_back(id);
    }
    // one synchronisation; PGX_ERR_FORMAT naming the first section whose bytes on the device are not what was saved
    void finish() {
        if (!h->from_image || ids.empty()) return;
        std::vector<uint64_t> got(ids.size());
        HIPCHECK(hipMemcpy(got.data(), sums.p, ids.size() * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i + 1 < ev.size(); i += 2) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) ms_sums += ms;
        }
        for (size_t i = 0; i < ids.size(); i++)
            if (got[i] != h->section(ids[i])->sum)
                throw Error(PGX_ERR_FORMAT, std::string("image file: section ") + pgx_image_section_name(ids[i]) +
                                                ": the sum of its bytes, computed on the device, does not match the table (damaged file); nothing has read it");
    }
};

void launch_image_sum(const void *data, uint64_t n_bytes, unsigned long long *sum, hipStream_t s) {
    const uint64_t units = n_bytes >> 4;
    // four 16-byte loads per thread and trip; at most eight blocks per compute unit of the largest part
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((units + 1023) / 1024, 2048));
    hipLaunchKernelGGL(pgx_image_sum_kernel, dim3(grid), dim3(256), 0, s, static_cast<const uint4 *>(data), n_bytes, sum);
    HIPCHECK(hipGetLastError());
}

extern "C" pgx_status pgx_image_sum(int device, const void *bytes, uint64_t n, uint64_t *sum) {
    PGX_GUARD_BEGIN
    if (!sum || (!bytes && n)) throw Error(PGX_ERR_ARG, "pgx_image_sum: null argument");
    if (device < 0) { *sum = image_sum_host(bytes, n); return PGX_OK; }
    use_device(device);
    DevBuf buf, out;
    try {
        buf.ensure(n ? n : 16); out.ensure(8);
        if (n) HIPCHECK(hipMemcpy(buf.p, bytes, n, hipMemcpyHostToDevice));
        HIPCHECK(hipMemsetAsync(out.p, 0, 8, nullptr));
        launch_image_sum(buf.p, n, out.as<unsigned long long>(), nullptr);
        HIPCHECK(hipMemcpy(sum, out.p, 8, hipMemcpyDeviceToHost));
    } catch (...) { buf.release(); out.release(); throw; }
    buf.release(); out.release();
    return PGX_OK;
    PGX_GUARD_END
}

void pgx_release_device_images(pgx_index *h) {
    for (auto *d : h->dev) {
        if (!d) continue;
        if (hipSetDevice(d->device) == hipSuccess) {
            release_buffers(d);
        }
        delete d;
    }
    h->dev.clear();
}

// k-mer seed table of a dense image (pgx_rank_device.h "k-mer seeds"): built level by level on the device,
// 4^L entries at level L, each one pgx_extend of its parent.  K = floor(log4 n), at most 14 (4 GiB of table; chr22 scale, 10 M
// reads, K = 11 / 12 / 13 / 14: 41.2 / 39.1 / 37.2 / 36.4 ms with the 64-byte dense image; n = 64 M, 1 M reads, K = 0 / 9 / 11 / 12: 3.64 / 3.44 /
// 3.14 / 3.07 ms), PGX_SEED_K overrides (0 = no table).
static void build_seed_table(pgx_device_image *d, const ImageKnobs &knobs) {
    PgxDevImage &g = d->img;
    // depth: one more than the first at which a random window is expected in the index less than once (4^K >= n), at most 15 (16 GiB): a seed that dies
    // inside the table ends a stage without another trip (n = 640 M: K = 14 / 15 / 16: 20.8 / 19.4-20.5 / 20.1 ms; n = 64 M: K = 12 / 13 / 14: 2.47 / 2.43 / 2.37 ms)
    // Round 4: at most 16 (64 GiB) and three tenths of the device's memory -- with the forward stages through the text a read is ~28 lane trips and the
    // two-step trips behind the seed are a third of them: depth 16 leaves 4 symbols = 2 trips of a 20-symbol step 1 instead of 5 = 3
    // (n = 640 M, K = 15 / 16: main kernel 10.26 / 9.44 ms, 791 / 830 M reads/s, 3.6 s more to build)
    int K = 0;
    while (K < 16 && (K == 0 || (1ull << (2 * (K - 1))) < g.n)) K++;
    {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); mem_free = mem_total = (size_t)16 << 30; }
        while (K > 2 && (((size_t)1 << (2 * K)) * sizeof(uint4)) * 5 / 4 > std::min(mem_total * 3 / 10, mem_free / 2)) K--; // table + the level below it while building
    }
    // an image small enough for LDS leaves the loop bound by instruction issue, and every extension a seed replaces is a gain: depth 10
    // (16 MiB of table, hot in L2) whatever n is (x index, 1 M reads, min_len 10, K = 0 / 4 / 6 / 8 / 10: 1.22 / 1.03 / 0.81 / 0.72 / 0.59 ms)
    if (d->lds_bytes) K = 10;
    if (knobs.has_seed_k) K = knobs.seed_k;
    if (K > PGX_SEED_MAX_K) K = PGX_SEED_MAX_K;
    if (K < 2) return;
    const uint64_t limit = g.n < (1ull << 30) ? (1ull << 32) : (1ull << 40); // what an entry (and the 32-bit kernels) can hold
    DevBuf tmp;
    // end table (stages that start at j = len, i.e. with the extension by 0): depth 8, 1 MiB -- such a stage almost always dies within a few
    // extensions (a read rarely ends where a sequence ends), which the entry's death depth answers at once
    int Ke = std::min(K, 8);
    if (knobs.has_seed_end_k) Ke = knobs.seed_end_k;
    auto build = [&](DevBuf &out, int depth, int end_table) {
        out.ensure(((size_t)1 << (2 * depth)) * sizeof(uint4));
        tmp.ensure(((size_t)1 << (2 * (depth - 1))) * sizeof(uint4));
        for (int L = 0; L < depth; L++) { // level L -> L + 1; level `depth` ends in out
            uint4 *dst = ((depth - (L + 1)) % 2 == 0) ? out.as<uint4>() : tmp.as<uint4>();
            const uint4 *src = ((depth - L) % 2 == 0) ? out.as<uint4>() : tmp.as<uint4>();
            const uint64_t n_dst = 1ull << (2 * (L + 1));
            hipLaunchKernelGGL(pgx_seed_build_kernel, dim3((unsigned)std::min<uint64_t>((n_dst + 255) / 256, 1u << 22)), dim3(256), 0, nullptr, g, src, dst, (uint32_t)L, n_dst, limit, end_table);
            HIPCHECK(hipGetLastError());
        }
        HIPCHECK(hipDeviceSynchronize());
    };
    const int Ks = K > PGX_SEED_SMALL_K ? PGX_SEED_SMALL_K : 0; // second, shallower table for searches with min_len < K
    try {
        build(d->seed, K, 0);
        if (Ks) build(d->seed_small, Ks, 0);
        if (Ke >= 2) build(d->seed_end, Ke, 1);
    } catch (...) { tmp.release(); d->seed.release(); d->seed_small.release(); d->seed_end.release(); throw; }
    tmp.release();
    if (Ke >= 2) { g.seed_end = d->seed_end.as<uint4>(); g.seed_end_k = (uint32_t)Ke; }
    g.seed = d->seed.as<uint4>();
    g.seed_k = (uint32_t)K;
    g.seed_main = g.seed; g.seed_k_main = g.seed_k;
    if (Ks) { g.seed_small = d->seed_small.as<uint4>(); g.seed_k_small = (uint32_t)Ks; }
}

// one device image per (index, device), created on first use; concurrent first calls from several host threads are serialised
static std::mutex g_image_mutex;
static void fill_device_image(pgx_index *h, pgx_device_image *d);

pgx_device_image *device_image(pgx_index *h, int device) {
    use_device(device);
    std::lock_guard<std::mutex> lock(g_image_mutex);
    if ((int)h->dev.size() <= device) h->dev.resize(device + 1, nullptr);
    if (h->dev[device]) return h->dev[device];
    std::unique_ptr<pgx_device_image> d(new pgx_device_image());
    d->device = device;
    try {
        fill_device_image(h, d.get());
    } catch (...) { // no half-built image stays behind (an image file whose section sums do not match ends here: the next call answers the same)
        (void)hipGetLastError();
        release_buffers(d.get());
        throw;
    }
    h->dev[device] = d.release();
    return h->dev[device];
}

static void fill_device_image(pgx_index *h, pgx_device_image *d) {
    const HostImage &m = h->img;
    const ImageKnobs knobs = read_image_knobs();
    const bool with_pairs = m.consts.has_pairs && !m.pairs.empty() && h->has_rank; // the two-step image next to dense2 (pgx_image.h)
    const auto t_begin = std::chrono::steady_clock::now();
    SectionSums check(h);
    upload(d->blocks, m.blocks.data(), m.blocks.size());       check.add(PGX_IMAGE_SEC_BLOCKS, d->blocks);
    upload(d->dir, m.dir.data(), m.dir.size() * 8);            check.add(PGX_IMAGE_SEC_DIR, d->dir);
    upload(d->blow, m.blow.data(), m.blow.size() * 2);         check.add(PGX_IMAGE_SEC_BLOW, d->blow);
    upload(d->exc, m.exc.data(), m.exc.size() * 4);            check.add(PGX_IMAGE_SEC_EXC, d->exc);
    upload(d->consts, &m.consts, sizeof(PgxConsts));           check.add(PGX_IMAGE_SEC_CONSTS, d->consts);
    upload(d->tstart, m.tstart.data(), m.tstart.size() * 8);   check.add(PGX_IMAGE_SEC_TSTART, d->tstart);
    upload(d->tvals, m.tvals.data(), m.tvals.size() * 8);      check.add(PGX_IMAGE_SEC_TVALS, d->tvals);
    upload(d->tdir, m.tdir.data(), m.tdir.size() * 4);         check.add(PGX_IMAGE_SEC_TDIR, d->tdir);
    upload(d->sbase2, m.sbase2.data(), m.sbase2.size() * 8);   check.add(PGX_IMAGE_SEC_SBASE2, d->sbase2);
    if (with_pairs) {
        upload(d->pairs, m.pairs.data(), m.pairs.size());      check.add(PGX_IMAGE_SEC_PAIRS, d->pairs);
        upload(d->pbase, m.pbase.data(), m.pbase.size() * 8);  check.add(PGX_IMAGE_SEC_PBASE, d->pbase);
    }
    check.finish(); // (image-opened handles: every section is what was saved, or PGX_ERR_FORMAT names the one that is not -- before the kernels below)
    const bool timing = std::getenv("PGX_IMAGE_TIMING") != nullptr; // one line on stderr: the uploads (with the sums of an image-opened handle), the device-side builds
    const auto t_uploaded = std::chrono::steady_clock::now();
    struct BuildTime { // (printed when the image is complete)
        bool on; std::chrono::steady_clock::time_point t0, t1; float ms_sums; uint64_t bytes; bool image;
        ~BuildTime() {
            if (!on) return;
            (void)hipDeviceSynchronize();
            const auto t2 = std::chrono::steady_clock::now();
            std::fprintf(stderr, "[pgx] to_device (%s handle): uploads%s %.3f ms wall; sum kernels %.3f ms by HIP events over %llu bytes; device-side builds %.3f ms wall\n",
                         image ? "image" : "file", image ? " + sums" : "", std::chrono::duration<double, std::milli>(t1 - t0).count(), (double)ms_sums,
                         (unsigned long long)bytes, std::chrono::duration<double, std::milli>(t2 - t1).count());
        }
    } build_time{timing, t_begin, t_uploaded, check.ms_sums, check.bytes_summed, h->from_image};
    PgxDevImage &g = d->img;
    g.blocks = d->blocks.as<uint4>();
    g.dir = d->dir.as<uint64_t>();
    g.blow = d->blow.as<uint16_t>();
    g.consts = d->consts.as<PgxConsts>();
    g.tstart = d->tstart.as<uint64_t>();
    g.tvals = d->tvals.as<uint64_t>();
    g.tdir = d->tdir.as<uint32_t>();
    g.tpair = nullptr;
    if (!m.tstart.empty() && !m.tvals.empty() && knobs.tpair) { // tag runs as (start, value) pairs for the locate kernel (built on the device)
        const uint64_t np = std::max<uint64_t>(m.tstart.size(), m.tvals.size());
        d->tpair.ensure(np * sizeof(ulonglong2));
        hipLaunchKernelGGL(pgx_tag_pair_kernel, dim3((unsigned)std::min<uint64_t>((np + 255) / 256, 65536)), dim3(256), 0, nullptr, d->tstart.as<uint64_t>(),
                           d->tvals.as<uint64_t>(), (uint64_t)m.tstart.size(), (uint64_t)m.tvals.size(), d->tpair.as<ulonglong2>());
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipDeviceSynchronize());
        g.tpair = d->tpair.as<ulonglong2>();
    }
    g.tbucket = nullptr; g.n_tbuckets = 0; g.tbucket_shift = 0;
    if (!m.tstart.empty() && !m.tvals.empty() && knobs.tbucket) { // tag runs by bucket, one line each (pgx_tag_bucket_kernel): about four runs per bucket
        const uint64_t nr = m.tstart.size(), span = m.tstart.back() + 1;
        uint32_t sh = 0;
        while (sh < 16 && (span >> (sh + 1)) >= nr / 4 + 1) sh++;
        const uint64_t nbk = (span >> sh) + 1;
        if (nbk * 128 <= (16ull << 30)) {
            d->tbucket.ensure(nbk * 128);
            hipLaunchKernelGGL(pgx_tag_bucket_kernel, dim3((unsigned)std::min<uint64_t>((nbk + 255) / 256, 1u << 20)), dim3(256), 0, nullptr, d->tstart.as<uint64_t>(),
                               d->tvals.as<uint64_t>(), nr, (uint64_t)m.tvals.size(), sh, nbk, d->tbucket.as<uint4>());
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipDeviceSynchronize());
            g.tbucket = d->tbucket.as<uint4>(); g.n_tbuckets = nbk; g.tbucket_shift = sh;
        }
    }
    g.n = m.consts.n;
    g.dir_entries = m.consts.dir_entries;
    g.n_tag_runs = m.consts.n_tag_runs;
    g.n_tag_items = m.tvals.size();
    g.tag_dir_entries = m.consts.tag_dir_entries;
    g.n_blocks = m.consts.n_blocks;
    g.dir_shift = m.consts.dir_shift;
    g.excl_mask = m.consts.excl_mask;
    g.tag_dir_shift = m.consts.tag_dir_shift;
    g.dense = m.consts.image_kind; // PGX_IMAGE_RL / _DENSE / _DENSE2
    g.wide = m.consts.wide;
    if (g.dense == PGX_IMAGE_DENSE2 && g.wide) g.dense = 3; // dense2 blocks with delta counts: the 64-bit kernels (pgx_image.h "WIDE")
    g.sbase2 = d->sbase2.as<uint64_t>();
    g.d2_sb_shift = m.consts.d2_sb_shift; g.n_sb2 = m.consts.n_sb2;
    g.pbase = nullptr; g.pairs_sb_shift = 0; g.n_sbp = 0; g.pairs_stride = 0;
    g.exc = d->exc.as<uint32_t>();
    size_t img_bytes = m.blocks.size() + m.dir.size() * 8 + m.blow.size() * 2;
    if (g.dense == 1) img_bytes = (size_t)m.consts.n_blocks * 16 * PGX_DENSE_LDS_U4 + 16; // padded blocks, no directory (pgx_dense_load)
    d->lds_bytes = (g.dense < 2 && img_bytes <= 48 * 1024) ? ((img_bytes + 15) & ~(size_t)15) : 0; // the dense2 image is never staged in LDS
    g.seed_k = 0;
    g.seed = nullptr;
    g.seed_end_k = 0;
    g.seed_end = nullptr;
    g.seed_k_main = g.seed_k_small = 0;
    g.seed_main = g.seed_small = nullptr;
    g.pairs = nullptr; g.first_ext = nullptr; g.pair_runs = 0;
    g.lce_sa = nullptr; g.lce_text = nullptr; g.lce_flags = nullptr; g.lce_lcp = nullptr; g.lce_max = 0; g.refill_min = 1;
    if (g.dense && h->has_rank) build_seed_table(d, knobs);
    if (with_pairs) {
        g.pbase = d->pbase.as<uint64_t>();
        g.pairs_sb_shift = m.consts.pairs_sb_shift; g.n_sbp = m.consts.n_sbp;
        g.pairs_stride = m.consts.pairs_stride;
        d->first_ext.ensure(512 * sizeof(uint4));
        hipLaunchKernelGGL(pgx_first_ext_kernel, dim3(1), dim3(256), 0, nullptr, g, d->first_ext.as<uint4>());
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipDeviceSynchronize());
        g.pairs = d->pairs.as<uint4>();
        g.first_ext = d->first_ext.as<uint4>();
        g.pair_runs = m.consts.pair_runs;
    }
}

extern "C" pgx_status pgx_index_to_device(pgx_index *h, int device) {
    PGX_GUARD_BEGIN
    if (!h) throw Error(PGX_ERR_ARG, "pgx_index_to_device: null index");
    (void)device_image(h, device);
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_index_device_view(pgx_index *h, int device, int which, void *out, uint64_t bytes) {
    PGX_GUARD_BEGIN
    if (!h || !out) throw Error(PGX_ERR_ARG, "pgx_index_device_view: null argument");
    pgx_device_image *d = device_image(h, device);
    const HostImage &m = h->img;
    const void *src = nullptr;
    uint64_t have = 0;
    switch (which) {
    case 0: src = d->blocks.p; have = m.blocks.size(); break;
    case 15: src = d->exc.p; have = m.exc.size() * 4; break;
    case 20: src = d->pairs.p; have = m.pairs.size(); break;
    case 22: src = d->sbase2.p; have = m.sbase2.size() * 8; break;
    case 23: src = d->pbase.p; have = m.pbase.size() * 8; break;
    case 30: case 31: case 32: case 33: { // the LCE image (device only; nothing where it does not exist for this index)
        if (h->has_rank) ensure_lce(h, d);
        if (d->img.lce_sa) {
            const uint64_t n = d->img.n, n_words = (n + 15) / 16 + 64;
            if (which == 30) { src = d->lce_sa.p; have = n * 4; }
            else if (which == 31) { src = d->lce_text.p; have = n_words * 4; }
            else if (which == 32) { src = d->lce_flags.p; have = (n_words / 1024 + 2) * 4; }
            else if (d->img.lce_lcp) { src = d->lce_lcp.p; have = n; }
        }
        break;
    }
    default: throw Error(PGX_ERR_ARG, "pgx_index_device_view: unknown view");
    }
    const uint64_t k = std::min(bytes, have);
    if (k && src) HIPCHECK(hipMemcpy(out, src, k, hipMemcpyDeviceToHost));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// locate path (pgx_locate_kernels.hip)
pgx_device_image *locate_image(pgx_index *h, int device) {
    if (!h->has_rank) throw Error(PGX_ERR_ARG, "locate: index opened without an r-index");
    pgx_device_image *d = device_image(h, device);
    std::lock_guard<std::mutex> lock(g_image_mutex);
    if (d->has_loc) return d;
    ensure_locate_host(h);
    const LocHostImage &m = h->loc;
    try {
        SectionSums check(h);
        upload(d->rstart, m.rstart.data(), m.rstart.size() * 8); check.add(PGX_IMAGE_SEC_RSTART, d->rstart);
        upload(d->rsamp, m.rsamp.data(), m.rsamp.size() * 8);    check.add(PGX_IMAGE_SEC_RSAMP, d->rsamp);
        upload(d->rdir, m.rdir.data(), m.rdir.size() * 4);       check.add(PGX_IMAGE_SEC_RDIR, d->rdir);
        upload(d->lpos, m.lpos.data(), m.lpos.size() * 8);       check.add(PGX_IMAGE_SEC_LPOS, d->lpos);
        upload(d->lnext, m.lnext.data(), m.lnext.size() * 8);    check.add(PGX_IMAGE_SEC_LNEXT, d->lnext);
        upload(d->ldir, m.ldir.data(), m.ldir.size() * 4);       check.add(PGX_IMAGE_SEC_LDIR, d->ldir);
        if (h->from_image) { // the constants travel as kernel arguments: summed where they are
            const ImageSection *sec = h->section(PGX_IMAGE_SEC_LOC_CONSTS);
            if (!sec || image_sum_host(&m.consts, sizeof(PgxLocConsts)) != sec->sum)
                throw Error(PGX_ERR_FORMAT, "image file: section loc_consts: the sum of its bytes does not match the table (damaged file)");
        }
        check.finish();
    } catch (...) { (void)hipGetLastError(); release_locate_buffers(d); throw; } // (has_loc stays false: the next call answers the same)
    PgxLocImage &g = d->loc;
    g.rstart = d->rstart.as<uint64_t>(); g.rsamp = d->rsamp.as<uint64_t>(); g.rdir = d->rdir.as<uint32_t>();
    g.lpos = d->lpos.as<uint64_t>(); g.lnext = d->lnext.as<uint64_t>(); g.ldir = d->ldir.as<uint32_t>();
    g.n = m.consts.n; g.n_runs = m.consts.n_runs; g.n_last = m.consts.n_last; g.max_length = m.consts.max_length;
    g.rdir_entries = m.consts.rdir_entries; g.ldir_entries = m.consts.ldir_entries;
    g.rdir_shift = m.consts.rdir_shift; g.ldir_shift = m.consts.ldir_shift;
    d->has_loc = true;
    return d;
}

// LCE image (pgx_image.h): suffix array in text coordinates + the text at two bits per symbol, for the pairs kernel's forward stages over narrow intervals.
// Built once per device image, on the device: the suffix array by the locate kernels (every BWT run is an independent chain from its sample), the text from
// it (the first symbol of suffix i is the one whose C-bucket holds i).  Only next to a narrow PAIRS image (textbook tables, n < 2^32); PGX_FM_LCE=0: never.
static std::mutex g_lce_mutex;
void ensure_lce(pgx_index *h, pgx_device_image *d) {
    std::lock_guard<std::mutex> lock(g_lce_mutex);
    if (d->lce_state) return;
    d->lce_state = 2;
    const ImageKnobs knobs = read_image_knobs();
    const uint64_t n = d->img.n;
    if (!knobs.lce || !d->img.pairs || d->img.wide || n < 4096 || n >= (1ull << 32) - (1ull << 20) || h->meta.max_length == 0) return;
    if (h->from_image && !h->loc.built) return; // an image saved without the locate image: the search runs on the PAIRS image alone
    uint64_t tot[6]; // symbol counts of the BWT = bucket bounds of the first column
    for (int i = 0; i < 6; i++) tot[i] = h->meta.sym_total[i];
    const uint64_t n_seq = tot[0];
    if (tot[0] + tot[1] + tot[2] + tot[3] + tot[4] + tot[5] != n || n_seq == 0 || n_seq > (1ull << 24)) return;
    {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); return; }
        if ((double)mem_free < 16.0 * (double)n + (double)(2ull << 30)) return; // 8 n (suffix array as the locate kernels write it) + n (text bytes) + 5.25 n (the image) + room
    }
    DevBuf vals, seq_len, seq_start, text8, bad;
    try {
        pgx_device_image *dl = locate_image(h, d->device);
        if (!dl->loc.n || dl->loc.n != n) throw Error(PGX_ERR_UNSUPPORTED, "no locate image");
        const uint64_t first = 0, last = n - 1;
        std::vector<uint64_t> off;
        uint64_t nv = 0;
        locate_core(h, dl, &first, &last, 1, 0, off, vals, nv);
        if (nv != n) throw Error(PGX_ERR_UNSUPPORTED, "suffix array incomplete");
        const uint64_t ml = h->meta.max_length;
        seq_len.ensure(n_seq * 8); seq_start.ensure((n_seq + 1) * 8); bad.ensure(16);
        HIPCHECK(hipMemset(seq_len.p, 0, n_seq * 8));
        HIPCHECK(hipMemset(bad.p, 0, 16));
        hipLaunchKernelGGL(pgx_lce_seqlen_kernel, dim3(grid_for(n_seq, 256)), dim3(256), 0, nullptr, vals.as<uint64_t>(), n_seq, ml, seq_len.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
        std::vector<uint64_t> hl(n_seq), hs(n_seq + 1, 0);
        HIPCHECK(hipMemcpy(hl.data(), seq_len.p, n_seq * 8, hipMemcpyDeviceToHost));
        for (uint64_t q = 0; q < n_seq; q++) { if (hl[q] == 0) throw Error(PGX_ERR_UNSUPPORTED, "a sequence without an endmarker suffix"); hs[q + 1] = hs[q] + hl[q]; }
        if (hs[n_seq] != n) throw Error(PGX_ERR_UNSUPPORTED, "sequence lengths do not add up to the BWT size");
        HIPCHECK(hipMemcpy(seq_start.p, hs.data(), (n_seq + 1) * 8, hipMemcpyHostToDevice));
        const uint64_t n_words = (n + 15) / 16 + 64, n_flag_words = n_words / 1024 + 2; // (64 words = two lines of padding behind the text, flagged)
        text8.ensure(n);
        d->lce_sa.ensure(n * 4 + 128); // (the kernel reads aligned windows of up to 20 entries from an interval's first entry on)
        d->lce_text.ensure(n_words * 4);
        d->lce_flags.ensure(n_flag_words * 4);
        HIPCHECK(hipMemset(d->lce_flags.p, 0, n_flag_words * 4));
        const uint64_t c1 = tot[0], c2 = c1 + tot[1], c3 = c2 + tot[2], c4 = c3 + tot[3], c5 = c4 + tot[4];
        hipLaunchKernelGGL(pgx_lce_scatter_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 20)), dim3(256), 0, nullptr, vals.as<uint64_t>(), n, ml,
                           seq_start.as<uint64_t>(), n_seq, c1, c2, c3, c4, c5, d->lce_sa.as<uint32_t>(), text8.as<uint8_t>(), bad.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
        unsigned long long n_bad = 0;
        HIPCHECK(hipMemcpy(&n_bad, bad.p, 8, hipMemcpyDeviceToHost));
        if (n_bad) throw Error(PGX_ERR_UNSUPPORTED, "suffix array values outside the collection");
        vals.release();
        // both orientations of every sequence (pgx_lce_rc_check_kernel): a forward-only collection is searched stepwise, as the reference's arithmetic has it
        if (n_seq & 1) throw Error(PGX_ERR_UNSUPPORTED, "odd number of sequences");
        hipLaunchKernelGGL(pgx_lce_rc_check_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 20)), dim3(256), 0, nullptr, text8.as<uint8_t>(),
                           seq_start.as<uint64_t>(), n_seq, n, bad.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpy(&n_bad, bad.p, 8, hipMemcpyDeviceToHost));
        if (n_bad) throw Error(PGX_ERR_UNSUPPORTED, "the collection does not hold every sequence next to its reverse complement");
        hipLaunchKernelGGL(pgx_lce_pack_kernel, dim3((unsigned)std::min<uint64_t>((n_words + 255) / 256, 1u << 20)), dim3(256), 0, nullptr, text8.as<uint8_t>(), n, n_words,
                           d->lce_text.as<uint32_t>(), d->lce_flags.as<uint32_t>());
        HIPCHECK(hipGetLastError());
        text8.release();
        const bool with_lcp = knobs.lcp; // (PGX_FM_LCP=0: every occurrence is compared with the text, as before the table existed)
        if (with_lcp) {
            d->lce_lcp.ensure(n + 64); // (the kernel reads aligned windows of up to 20 entries)
            hipLaunchKernelGGL(pgx_lce_lcp_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 20)), dim3(256), 0, nullptr, d->lce_sa.as<uint32_t>(),
                               d->lce_text.as<uint32_t>(), d->lce_flags.as<uint32_t>(), n, d->lce_lcp.as<uint8_t>());
            HIPCHECK(hipGetLastError());
        }
        HIPCHECK(hipDeviceSynchronize());
        d->img.lce_lcp = with_lcp ? d->lce_lcp.as<uint8_t>() : nullptr;
        d->img.lce_sa = d->lce_sa.as<uint32_t>();
        d->img.lce_text = d->lce_text.as<uint32_t>();
        d->img.lce_flags = d->lce_flags.as<uint32_t>();
        d->img.lce_max = with_lcp ? PGX_LCE_MAX_OCC : 16; // (without the table of common prefixes every occurrence costs a trip)
        if (knobs.has_lce_max) d->img.lce_max = knobs.lce_max;
        d->lce_seq_start = seq_start; seq_start = DevBuf(); // (kept: text position -> sequence for pgx_batch_locate, 8 bytes per sequence)
        d->lce_n_seq = n_seq;
        d->img.refill_min = 12; // (chr22 scale, 1 / 3 / 6 / 10 / 16 / 24: main kernel 10.76 / 10.44 / 10.24 / 10.15 / 10.10 / 10.08 ms, step 13.16 / 12.87 / 12.62 / 12.59 / 12.56 / 12.65)
        if (knobs.has_refill_min) d->img.refill_min = knobs.refill_min;
        d->lce_state = 1;
    } catch (...) { // (no LCE image: the search runs on the PAIRS image alone, as before)
        (void)hipGetLastError();
        d->lce_sa.release(); d->lce_text.release(); d->lce_flags.release(); d->lce_lcp.release(); d->lce_seq_start.release();
        d->lce_n_seq = 0;
        d->img.lce_sa = nullptr; d->img.lce_text = nullptr; d->img.lce_flags = nullptr; d->img.lce_lcp = nullptr;
    }
    vals.release(); seq_len.release(); seq_start.release(); text8.release(); bad.release();
}

// TEXT image (pgx_image.h): the collection itself at four bits per symbol, every symbol told apart, with the sequence starts.  Built once per device image on
// its first use, by the route of ensure_lce: the whole suffix array from the locate kernels, the sequence lengths from the endmarker suffixes, first symbols
// scattered to text positions (pgx_lce_seqlen_kernel / pgx_lce_scatter_kernel as they are), then pgx_text_mark_kernel tells endmarkers from N and
// pgx_text_pack_kernel packs.  Next to a resident LCE image its lce_sa / lce_seq_start stand in for the locate: the same bytes either way.
// Unlike ensure_lce this one throws: who asks for the text cannot do without it.
static std::mutex g_text_mutex;
void ensure_text(pgx_index *h, pgx_device_image *d) {
    std::lock_guard<std::mutex> lock(g_text_mutex);
    if (d->has_text) return;
    if (!h->has_rank) throw Error(PGX_ERR_ARG, "text image: index opened without an r-index");
    locate_check_supported(h, "text image");
    if (h->from_image && !h->loc.built)
        throw Error(PGX_ERR_UNSUPPORTED, "text image: the image file was saved without the locate image (--no-locate), and the text is recovered through it");
    const uint64_t n = d->img.n;
    if (n >= (1ull << 32) - (1ull << 20))
        throw Error(PGX_ERR_UNSUPPORTED, "text image: the BWT has " + std::to_string(n) + " symbols, the image holds fewer than 2^32 - 2^20");
    uint64_t tot[6]; // symbol counts of the BWT = bucket bounds of the first column
    for (int i = 0; i < 6; i++) tot[i] = h->meta.sym_total[i];
    const uint64_t n_seq = tot[0], ml = h->meta.max_length;
    if (tot[0] + tot[1] + tot[2] + tot[3] + tot[4] + tot[5] != n || n_seq == 0 || ml == 0)
        throw Error(PGX_ERR_UNSUPPORTED, "text image: the symbol counts of the index do not describe a collection");
    bool from_lce = false;
    {
        std::lock_guard<std::mutex> lce_lock(g_lce_mutex);
        from_lce = d->lce_state == 1 && d->img.lce_sa && d->lce_seq_start.p && d->lce_n_seq == n_seq;
    }
    const uint64_t n_words = (n + 7) / 8 + PGX_TEXT_PAD_WORDS;
    {
        // for a while: the suffix array as the locate kernels write it (8 n) and as the scatter kernel writes it again (4 n), a byte a symbol, the image
        const uint64_t need = (from_lce ? 0 : 12 * n + 128) + n + n_words * 4 + (n_seq + 1) * 16 + (1ull << 20);
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); throw Error(PGX_ERR_HIP, "text image: hipMemGetInfo failed"); }
        if ((uint64_t)mem_free < need)
            throw Error(PGX_ERR_NOMEM, "text image: building it takes " + std::to_string(need) + " bytes of device memory for a while, " + std::to_string(mem_free) + " are free");
    }
    DevBuf vals, seq_len, seq_start, text8, sa32, bad, text4;
    auto drop = [&]() { vals.release(); seq_len.release(); seq_start.release(); text8.release(); sa32.release(); bad.release(); text4.release(); };
    try {
        const uint64_t c1 = tot[0], c2 = c1 + tot[1], c3 = c2 + tot[2], c4 = c3 + tot[3], c5 = c4 + tot[4];
        const unsigned grid_n = (unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 20);
        seq_start.ensure((n_seq + 1) * 8);
        text8.ensure(n);
        if (from_lce) {
            HIPCHECK(hipMemcpy(seq_start.p, d->lce_seq_start.p, (n_seq + 1) * 8, hipMemcpyDeviceToDevice));
            hipLaunchKernelGGL(pgx_text_scatter32_kernel, dim3(grid_n), dim3(256), 0, nullptr, (const uint32_t *)d->lce_sa.as<uint32_t>(), n, c1, c2, c3, c4, c5, text8.as<uint8_t>());
            HIPCHECK(hipGetLastError());
        } else {
            pgx_device_image *dl = locate_image(h, d->device);
            if (!dl->loc.n || dl->loc.n != n) throw Error(PGX_ERR_UNSUPPORTED, "text image: the locate image does not cover the BWT");
            const uint64_t first = 0, last = n - 1;
            std::vector<uint64_t> off;
            uint64_t nv = 0;
            locate_core(h, dl, &first, &last, 1, 0, off, vals, nv);
            if (nv != n) throw Error(PGX_ERR_UNSUPPORTED, "text image: the suffix array is incomplete");
            seq_len.ensure(n_seq * 8); bad.ensure(16);
            HIPCHECK(hipMemset(seq_len.p, 0, n_seq * 8));
            HIPCHECK(hipMemset(bad.p, 0, 16));
            hipLaunchKernelGGL(pgx_lce_seqlen_kernel, dim3(grid_for(n_seq, 256)), dim3(256), 0, nullptr, vals.as<uint64_t>(), n_seq, ml, seq_len.as<unsigned long long>());
            HIPCHECK(hipGetLastError());
            std::vector<uint64_t> hl(n_seq), hs(n_seq + 1, 0);
            HIPCHECK(hipMemcpy(hl.data(), seq_len.p, n_seq * 8, hipMemcpyDeviceToHost));
            for (uint64_t q = 0; q < n_seq; q++) {
                if (hl[q] == 0) throw Error(PGX_ERR_UNSUPPORTED, "text image: sequence " + std::to_string(q) + " has no endmarker suffix");
                hs[q + 1] = hs[q] + hl[q];
            }
            if (hs[n_seq] != n) throw Error(PGX_ERR_UNSUPPORTED, "text image: the sequence lengths do not add up to the BWT size");
            HIPCHECK(hipMemcpy(seq_start.p, hs.data(), (n_seq + 1) * 8, hipMemcpyHostToDevice));
            sa32.ensure(n * 4 + 128);
            hipLaunchKernelGGL(pgx_lce_scatter_kernel, dim3(grid_n), dim3(256), 0, nullptr, vals.as<uint64_t>(), n, ml, seq_start.as<uint64_t>(), n_seq, c1, c2, c3, c4, c5,
                               sa32.as<uint32_t>(), text8.as<uint8_t>(), bad.as<unsigned long long>());
            HIPCHECK(hipGetLastError());
            unsigned long long n_bad = 0;
            HIPCHECK(hipMemcpy(&n_bad, bad.p, 8, hipMemcpyDeviceToHost));
            if (n_bad) throw Error(PGX_ERR_UNSUPPORTED, "text image: suffix array values outside the collection");
            vals.release(); sa32.release();
        }
        hipLaunchKernelGGL(pgx_text_mark_kernel, dim3(grid_for(n_seq, 256)), dim3(256), 0, nullptr, (const uint64_t *)seq_start.as<uint64_t>(), n_seq, n, text8.as<uint8_t>());
        HIPCHECK(hipGetLastError());
        text4.ensure(n_words * 4);
        hipLaunchKernelGGL(pgx_text_pack_kernel, dim3((unsigned)std::min<uint64_t>((n_words + 255) / 256, 1u << 20)), dim3(256), 0, nullptr, (const uint8_t *)text8.as<uint8_t>(), n,
                           n_words, 0u, text4.as<uint32_t>());
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipDeviceSynchronize());
    } catch (...) { (void)hipGetLastError(); drop(); throw; }
    d->text4 = text4; text4 = DevBuf();
    d->text_seq_start = seq_start; seq_start = DevBuf();
    d->text_n_seq = n_seq;
    d->has_text = true;
    drop();
}

extern "C" pgx_status pgx_index_text(pgx_index *h, int device, uint64_t *seq_lengths, uint64_t n_seq_cap, uint8_t *text, uint64_t text_cap) {
    PGX_GUARD_BEGIN
    if (!h || !seq_lengths) throw Error(PGX_ERR_ARG, "pgx_index_text: null argument");
    pgx_device_image *d = device_image(h, device);
    ensure_text(h, d);
    const uint64_t n = d->img.n, n_seq = d->text_n_seq;
    if (n_seq_cap < n_seq) throw Error(PGX_ERR_ARG, "pgx_index_text: the index has " + std::to_string(n_seq) + " sequences, n_seq_cap is " + std::to_string(n_seq_cap));
    if (text && text_cap < n) throw Error(PGX_ERR_ARG, "pgx_index_text: the text has " + std::to_string(n) + " bytes, text_cap is " + std::to_string(text_cap));
    std::vector<uint64_t> hs(n_seq + 1);
    HIPCHECK(hipMemcpy(hs.data(), d->text_seq_start.p, (n_seq + 1) * 8, hipMemcpyDeviceToHost));
    for (uint64_t q = 0; q < n_seq; q++) seq_lengths[q] = hs[q + 1] - hs[q] - 1;
    if (text && n) {
        DevBuf bytes;
        try {
            bytes.ensure(n);
            hipLaunchKernelGGL(pgx_text_unpack_kernel, dim3((unsigned)std::min<uint64_t>(((n + 7) / 8 + 255) / 256, 1u << 20)), dim3(256), 0, nullptr,
                               (const uint32_t *)d->text4.as<uint32_t>(), n, bytes.as<uint8_t>());
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipMemcpy(text, bytes.p, n, hipMemcpyDeviceToHost));
        } catch (...) { bytes.release(); throw; }
        bytes.release();
    }
    return PGX_OK;
    PGX_GUARD_END
}

// WALK image (pgx_image.h): one bit per text position that starts a node visit, a rank directory over the bits and the node of every visit.  Built once per
// device image on its first use, on the TEXT image's coordinates (ensure_text first: its text_seq_start is the sequence table here too).  The text position
// of every row comes from the resident lce_sa where the LCE image is resident, else from a whole-range locate as in ensure_text: the same bytes either way.
// Two passes over the rows (pgx_walk_kernels.hip): marks, then -- behind popcounts and the scan -- the nodes.  Throws like ensure_text.
void walk_directory(const uint64_t *bits, uint64_t n_blocks, DevBuf &counts, uint64_t *dir, DevBuf &scan_tmp, hipStream_t s) {
    counts.ensure(n_blocks * 8);
    hipLaunchKernelGGL(pgx_walk_popc_kernel, dim3((unsigned)std::min<uint64_t>((n_blocks + 255) / 256, 2048)), dim3(256), 0, s, bits, n_blocks, counts.as<uint64_t>());
    HIPCHECK(hipGetLastError());
    scan_excl(1, counts.p, n_blocks, 0, dir, scan_tmp, s);
}

static std::mutex g_walk_mutex;
void ensure_walk(pgx_index *h, pgx_device_image *d) {
    std::lock_guard<std::mutex> lock(g_walk_mutex);
    if (d->has_walk) return;
    if (!h->has_rank) throw Error(PGX_ERR_ARG, "walk image: index opened without an r-index");
    if (!h->has_tags) throw Error(PGX_ERR_UNSUPPORTED, "walk image: index opened without a tag array, and the walk is recovered from the tags");
    locate_check_supported(h, "walk image");
    if (h->from_image && !h->loc.built)
        throw Error(PGX_ERR_UNSUPPORTED, "walk image: the image file was saved without the locate image (--no-locate), and the walk is recovered through it");
    const uint64_t n = d->img.n;
    if (n >= (1ull << 32) - (1ull << 20))
        throw Error(PGX_ERR_UNSUPPORTED, "walk image: the BWT has " + std::to_string(n) + " symbols, the image holds fewer than 2^32 - 2^20");
    const uint32_t span_lo = h->img.consts.tag_span_lo;
    if (!span_lo) throw Error(PGX_ERR_UNSUPPORTED, "walk image: the image file was saved before the span of the tag runs was kept; save it again from the index and tag files");
    const auto t_begin = std::chrono::steady_clock::now();
    ensure_text(h, d);
    const uint64_t n_seq = d->text_n_seq, ml = h->meta.max_length;
    // the runs end with the last row (pgx_image.h "WHICH RUN HOLDS ROW i"): in front of row n_seq lie `head` rows, mod 2^32 like span_lo
    const uint32_t head = span_lo - 1u - (uint32_t)(n - n_seq);
    if (head >= (1u << 25))
        throw Error(PGX_ERR_FORMAT, "walk image: the tags do not belong to this index: their runs cover fewer rows than the " + std::to_string(n - n_seq) + " the index has behind its endmarkers");
    const int64_t delta = (int64_t)head - (int64_t)n_seq;
    bool from_lce = false;
    {
        std::lock_guard<std::mutex> lce_lock(g_lce_mutex);
        from_lce = d->lce_state == 1 && d->img.lce_sa && d->lce_seq_start.p && d->lce_n_seq == n_seq;
    }
    const uint64_t n_blocks = n / PGX_WALK_BLOCK_BITS + 1, n_words = n_blocks * PGX_WALK_BLOCK_WORDS;
    auto check_free = [&](uint64_t need, const char *what) {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); throw Error(PGX_ERR_HIP, "walk image: hipMemGetInfo failed"); }
        if ((uint64_t)mem_free < need)
            throw Error(PGX_ERR_NOMEM, std::string("walk image: ") + what + " takes " + std::to_string(need) + " bytes of device memory, " + std::to_string(mem_free) + " are free");
    };
    // the suffix array as the locate kernels write it (8 n, only without a resident LCE image), the marks, the directory and its counts, the scan's scratch
    check_free((from_lce ? 0 : 8 * n + 128) + n_words * 8 + (n_blocks + 1) * 16 + (1ull << 20), "building it");
    DevBuf vals, bits, dir, nodes, counts, scan_tmp, bad;
    auto drop = [&]() { vals.release(); bits.release(); dir.release(); nodes.release(); counts.release(); scan_tmp.release(); bad.release(); };
    uint64_t V = 0;
    try {
        const uint32_t *sa32 = nullptr;
        const uint64_t *sa64 = nullptr;
        if (from_lce) sa32 = d->lce_sa.as<uint32_t>();
        else {
            pgx_device_image *dl = locate_image(h, d->device);
            if (!dl->loc.n || dl->loc.n != n) throw Error(PGX_ERR_UNSUPPORTED, "walk image: the locate image does not cover the BWT");
            const uint64_t first = 0, last = n - 1;
            std::vector<uint64_t> off;
            uint64_t nv = 0;
            locate_core(h, dl, &first, &last, 1, 0, off, vals, nv);
            if (nv != n) throw Error(PGX_ERR_UNSUPPORTED, "walk image: the suffix array is incomplete");
            sa64 = vals.as<uint64_t>();
        }
        const uint64_t *seq_start = d->text_seq_start.as<uint64_t>();
        const uint64_t rows = n - n_seq;
        const unsigned grid_rows = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((rows + 255) / 256, 1u << 20));
        bits.ensure(n_words * 8); dir.ensure((n_blocks + 1) * 8); bad.ensure(16);
        HIPCHECK(hipMemsetAsync(bits.p, 0, n_words * 8, nullptr));
        HIPCHECK(hipMemsetAsync(bad.p, 0, 8, nullptr));
        HIPCHECK(hipMemsetAsync(bad.as<uint8_t>() + 8, 0xFF, 8, nullptr));
        hipLaunchKernelGGL(pgx_walk_mark_kernel, dim3(grid_rows), dim3(256), 0, nullptr, d->img, sa32, sa64, ml, seq_start, n_seq, n, delta, bits.as<uint32_t>(),
                           bad.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
        walk_directory(bits.as<uint64_t>(), n_blocks, counts, dir.as<uint64_t>(), scan_tmp, nullptr);
        PgxWalkImage w{bits.as<uint64_t>(), dir.as<uint64_t>(), nullptr, n, n_words, n_blocks, 0};
        hipLaunchKernelGGL(pgx_walk_check_kernel, dim3(grid_for(n_seq, 256)), dim3(256), 0, nullptr, w, seq_start, n_seq, 1u, bad.as<unsigned long long>() + 1);
        HIPCHECK(hipGetLastError());
        uint64_t hb[2] = {0, 0};
        HIPCHECK(hipMemcpy(hb, bad.p, 16, hipMemcpyDeviceToHost));
        if (hb[0]) throw Error(PGX_ERR_UNSUPPORTED, "walk image: suffix array values outside the collection");
        if (hb[1] != ~0ull)
            throw Error(PGX_ERR_FORMAT, "walk image: the tags do not belong to this index: the first position of sequence " + std::to_string(hb[1]) + " does not start a node visit");
        HIPCHECK(hipMemcpy(&V, dir.as<uint64_t>() + n_blocks, 8, hipMemcpyDeviceToHost));
        check_free((V ? V : 1) * 8, "the node of every visit");
        nodes.ensure((V ? V : 1) * 8);
        w.nodes = nodes.as<uint64_t>(); w.n_visits = V;
        hipLaunchKernelGGL(pgx_walk_nodes_kernel, dim3(grid_rows), dim3(256), 0, nullptr, d->img, w, sa32, sa64, ml, seq_start, n_seq, n, delta, nodes.as<uint64_t>());
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipDeviceSynchronize());
        d->walk = w;
    } catch (...) { (void)hipGetLastError(); drop(); throw; }
    d->walk_bits = bits; bits = DevBuf();
    d->walk_dir = dir; dir = DevBuf();
    d->walk_nodes = nodes; nodes = DevBuf();
    d->has_walk = true;
    drop();
    if (std::getenv("PGX_IMAGE_TIMING")) // (scripts/read_walk_bench.py; the TEXT image's build is inside when this call built it)
        std::fprintf(stderr, "[pgx] walk image (%s route): %.3f ms wall; %llu bytes (%llu marks + directory, %llu visits)\n", from_lce ? "lce" : "locate",
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(),
                     (unsigned long long)(n_words * 8 + (n_blocks + 1) * 8 + V * 8), (unsigned long long)(n_words * 8 + (n_blocks + 1) * 8), (unsigned long long)V);
}

extern "C" pgx_status pgx_index_paths(pgx_index *h, int device, uint64_t *path_offsets, uint64_t n_seq_cap, uint64_t *path_nodes, uint32_t *visit_length, uint64_t cap) {
    PGX_GUARD_BEGIN
    if (!h || !path_offsets) throw Error(PGX_ERR_ARG, "pgx_index_paths: null argument");
    pgx_device_image *d = device_image(h, device);
    ensure_walk(h, d);
    const uint64_t n_seq = d->text_n_seq, V = d->walk.n_visits;
    if (n_seq_cap < n_seq) throw Error(PGX_ERR_ARG, "pgx_index_paths: the index has " + std::to_string(n_seq) + " sequences, n_seq_cap is " + std::to_string(n_seq_cap));
    // the position of every visit comes down once; offsets and lengths follow on the host (an inspection call, not a stage)
    std::vector<uint64_t> hs(n_seq + 1), pos(V);
    HIPCHECK(hipMemcpy(hs.data(), d->text_seq_start.p, (n_seq + 1) * 8, hipMemcpyDeviceToHost));
    if (V) {
        DevBuf dpos;
        try {
            dpos.ensure(V * 8);
            hipLaunchKernelGGL(pgx_walk_positions_kernel, dim3((unsigned)std::min<uint64_t>((d->walk.n_words + 255) / 256, 1u << 20)), dim3(256), 0, nullptr, d->walk, dpos.as<uint64_t>());
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipMemcpy(pos.data(), dpos.p, V * 8, hipMemcpyDeviceToHost));
        } catch (...) { dpos.release(); throw; }
        dpos.release();
    }
    uint64_t k = 0;
    for (uint64_t q = 0; q < n_seq; q++) {
        path_offsets[q] = k;
        while (k < V && pos[k] < hs[q + 1]) k++;
    }
    path_offsets[n_seq] = k;
    if (!path_nodes && !visit_length) return PGX_OK;
    if (cap < V) throw Error(PGX_ERR_NOMEM, "pgx_index_paths: the index has " + std::to_string(V) + " visits, cap is " + std::to_string(cap));
    if (path_nodes && V) HIPCHECK(hipMemcpy(path_nodes, d->walk_nodes.p, V * 8, hipMemcpyDeviceToHost));
    if (visit_length)
        for (uint64_t q = 0; q < n_seq; q++)
            for (uint64_t j = path_offsets[q]; j < path_offsets[q + 1]; j++)
                visit_length[j] = (uint32_t)((j + 1 < path_offsets[q + 1] ? pos[j + 1] : hs[q + 1] - 1) - pos[j]);
    return PGX_OK;
    PGX_GUARD_END
}

// COMPAT count_encoded / LF_encoded on an encoded index without N: the reference mis-parses every block (quirk 3); the literal
// image reproduces what it computes (pgx_runtime.hip literal_count says when)
pgx_device_image *literal_image(pgx_index *h, int device) {
    pgx_device_image *d = device_image(h, device);
    std::lock_guard<std::mutex> lock(g_image_mutex);
    if (d->has_lit) return d;
    ensure_literal_host(h);
    LitHostImage &m = h->lit;
    try {
        SectionSums check(h);
        upload(d->lit_bstart, m.bstart.data(), m.bstart.size() * 8); check.add(PGX_IMAGE_SEC_LIT_BSTART, d->lit_bstart);
        upload(d->lit_cum, m.cum.data(), m.cum.size() * 8);          check.add(PGX_IMAGE_SEC_LIT_CUM, d->lit_cum);
        upload(d->lit_runs, m.runs.data(), m.runs.size() * 8);       check.add(PGX_IMAGE_SEC_LIT_RUNS, d->lit_runs);
        upload(d->lit_roff, m.roff.data(), m.roff.size() * 4);       check.add(PGX_IMAGE_SEC_LIT_ROFF, d->lit_roff);
        // the two byte tables and C in the order of the file's lit_tabs section (the kernels read the tables; C travels as an argument)
        d->lit_tabs.ensure(512 * 4 + 64);
        HIPCHECK(hipMemcpy(d->lit_tabs.p, m.code_of, 1024, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d->lit_tabs.as<uint32_t>() + 256, m.cslot_of, 1024, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d->lit_tabs.as<uint32_t>() + 512, m.C, 64, hipMemcpyHostToDevice));
        check.add(PGX_IMAGE_SEC_LIT_TABS, d->lit_tabs);
        check.finish();
    } catch (...) { (void)hipGetLastError(); release_literal_buffers(d); throw; } // (has_lit stays false)
    PgxLitImage &g = d->lit;
    g.bstart = d->lit_bstart.as<uint64_t>(); g.cum = d->lit_cum.as<uint64_t>(); g.runs = d->lit_runs.as<uint64_t>();
    g.roff = d->lit_roff.as<uint32_t>(); g.code_of = d->lit_tabs.as<uint32_t>(); g.cslot_of = d->lit_tabs.as<uint32_t>() + 256;
    for (int i = 0; i < 8; i++) g.C[i] = m.C[i];
    g.n = h->meta.sequence_size; g.n_blocks = m.bstart.size();
    d->has_lit = true;
    return d;
}
