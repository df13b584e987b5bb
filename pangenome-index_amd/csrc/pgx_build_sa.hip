// pgx_build_sa.hip -- pgx_build_index_from_text[s]_device: the BWT and the r-index of a text collection with the suffix sorting, the BWT
// and its runs computed on the device (pgx_build_sa_kernels.hip), the two files written by the host writers of pgx_build.cpp from the
// same hand-over (TextBwt) the CPU builder fills.  DESIGN section "Index construction on the device".
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <string>

#include "pgx_runtime_internal.hpp"

static thread_local double g_build_device_ms[6] = {0, 0, 0, 0, 0, 0};

namespace {
struct Clock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap() {
        const auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};

constexpr uint64_t kMaxSymbols = (1ull << 32) - (1ull << 20); // u32 text coordinates, the bound of ensure_lce
constexpr unsigned kMaxRounds = 40;

// bits that hold every value below `count` (0 for a single value: nothing to sort by)
unsigned bits_below(uint64_t count) { return count <= 1 ? 0u : 64u - (unsigned)__builtin_clzll(count - 1); }

// every device buffer of the build and its size as a function of n alone; `bytes()` is what DevBuf::ensure allocates for them
struct Plan {
    uint64_t n, n_words, n_tiles, n_sort_blocks, hist_entries;
    uint64_t text, codes, column, hist, offs, tile_cnt, tile_off, scan_tmp, scalars;
    explicit Plan(uint64_t n_) : n(n_) {
        n_words = n / 8 + 4;
        n_tiles = (n + PGX_SA_TILE - 1) / PGX_SA_TILE;
        n_sort_blocks = (n + PGX_SA_SORT_TILE - 1) / PGX_SA_SORT_TILE;
        hist_entries = 256 * n_sort_blocks;
        text = n + 8;
        codes = n_words * 8;                 // 3-bit codes, one a byte; the BWT later
        column = n * 4;                      // x 7: hi, lo, idx, their second copies, rank
        hist = hist_entries * 4;
        offs = (hist_entries + 1) * 8;
        tile_cnt = n_tiles * 4;
        tile_off = (n_tiles + 1) * 8;
        scan_tmp = (std::max(hist_entries, n_tiles) / PGX_SCAN1_TILE_ITEMS + 3) * 8;
        scalars = 16;
    }
    static uint64_t alloc_of(uint64_t b) { return b + b / 8 + 256; } // DevBuf::ensure
    uint64_t bytes() const {
        return alloc_of(text) + alloc_of(codes) + 7 * alloc_of(column) + alloc_of(hist) + alloc_of(offs) + alloc_of(tile_cnt) + alloc_of(tile_off) +
               alloc_of(scan_tmp) + alloc_of(scalars);
    }
};

struct Columns { // the triples of the sort as three columns, twice
    DevBuf *hi, *lo, *idx, *hi2, *lo2, *idx2;
};

struct PassTimer { // PGX_BUILD_TIMING=1: HIP-event time of every radix pass (histogram, scan, scatter)
    bool on = std::getenv("PGX_BUILD_TIMING") != nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    double ms = 0;
    uint64_t passes = 0;
    ~PassTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    void begin(hipStream_t s) {
        if (!on) return;
        if (!a) { HIPCHECK(hipEventCreate(&a)); HIPCHECK(hipEventCreate(&b)); }
        HIPCHECK(hipEventRecord(a, s));
    }
    void end(hipStream_t s) {
        if (!on) return;
        HIPCHECK(hipEventRecord(b, s));
        HIPCHECK(hipEventSynchronize(b));
        float t = 0;
        HIPCHECK(hipEventElapsedTime(&t, a, b));
        ms += t;
        passes++;
    }
};

// stable LSD radix sort of the triples by (hi, lo): the digits of lo first, then those of hi, eight bits a pass, only the digits in use
void sort_columns(Columns &c, const Plan &pl, unsigned lo_bits, unsigned hi_bits, DevBuf &hist, DevBuf &offs, DevBuf &scan_tmp, hipStream_t s, PassTimer &pt) {
    const uint64_t n = pl.n;
    const unsigned nb = grid_for(n, PGX_SA_SORT_TILE);
    for (int half = 0; half < 2; half++) {
        const unsigned bits = half ? hi_bits : lo_bits;
        for (unsigned shift = 0; shift < bits; shift += 8) {
            pt.begin(s);
            hipLaunchKernelGGL(pgx_sa_hist_kernel, dim3(nb), dim3(256), 0, s, (const uint32_t *)(half ? c.hi : c.lo)->as<uint32_t>(), n, (uint32_t)shift, (uint32_t)nb,
                               hist.as<uint32_t>());
            HIPCHECK(hipGetLastError());
            scan_excl(0, hist.p, pl.hist_entries, 0, offs.as<uint64_t>(), scan_tmp, s);
            hipLaunchKernelGGL(pgx_sa_scatter_kernel, dim3(nb), dim3(256), 0, s, (const uint32_t *)c.hi->as<uint32_t>(), (const uint32_t *)c.lo->as<uint32_t>(),
                               (const uint32_t *)c.idx->as<uint32_t>(), n, half, (uint32_t)shift, (uint32_t)nb, (const uint64_t *)offs.as<uint64_t>(),
                               c.hi2->as<uint32_t>(), c.lo2->as<uint32_t>(), c.idx2->as<uint32_t>());
            HIPCHECK(hipGetLastError());
            pt.end(s);
            std::swap(c.hi, c.hi2); std::swap(c.lo, c.lo2); std::swap(c.idx, c.idx2);
        }
    }
}

uint64_t file_size_of(const char *path) {
    struct stat st;
    if (stat(path, &st) != 0 || !S_ISREG(st.st_mode)) throw Error(PGX_ERR_IO, std::string("Cannot open text: ") + path);
    return (uint64_t)st.st_size;
}
// the one byte of a text that is looked at before the sizes are judged: a text that does not end in a newline gets one
bool ends_in_newline(const char *path, uint64_t size) {
    FILE *f = std::fopen(path, "rb");
    if (!f) throw Error(PGX_ERR_IO, std::string("Cannot open text: ") + path);
    int c = EOF;
    if (fseeko(f, (off_t)(size - 1), SEEK_SET) == 0) c = std::fgetc(f);
    std::fclose(f);
    if (c == EOF) throw Error(PGX_ERR_IO, std::string("Cannot read text: ") + path);
    return c == '\n';
}

void build_index_device_core(const char *const *paths, uint32_t n_texts, const char *out_rlbwt_path, const char *out_ri_path, int encoded, int device,
                             double *ms) {
    RoctxRange range("pgx_build_index_device");
    Clock clk;
    use_device(device);
    // ---- what can be refused is refused from the file sizes, before anything is read or allocated
    std::vector<uint64_t> fsize(n_texts);
    uint64_t total = 0;
    for (uint32_t t = 0; t < n_texts; t++) {
        fsize[t] = file_size_of(paths[t]);
        if (fsize[t] == 0) throw Error(PGX_ERR_FORMAT, std::string("empty text: ") + paths[t]);
        total += fsize[t];
        if (total < kMaxSymbols && !ends_in_newline(paths[t], fsize[t])) total++;
    }
    if (total >= kMaxSymbols)
        throw Error(PGX_ERR_UNSUPPORTED, "a collection of " + std::to_string(total) + " symbols: the device build holds text positions in 32 bits (fewer than 2^32 - 2^20 "
                                             "symbols); build it on the host as several texts: pgx_build_index_from_texts");
    const Plan bound(total); // (the newlines that texts without a final one get are counted)
    {
        uint64_t avail = 0;
        if (const char *e = std::getenv("PGX_BUILD_DEVICE_BUDGET_MB")) {
            const double mb = std::strtod(e, nullptr);
            if (mb > 0) avail = (uint64_t)(mb * 1048576.0);
        }
        if (!avail) {
            size_t mem_free = 0, mem_total = 0;
            HIPCHECK(hipMemGetInfo(&mem_free, &mem_total));
            avail = mem_free;
        }
        if (bound.bytes() > avail)
            throw Error(PGX_ERR_NOMEM, "the device build of " + std::to_string(total) + " symbols needs " + std::to_string(bound.bytes()) + " bytes of device memory, " +
                                           std::to_string(avail) + " are available (there is no chunked mode: pgx_build_index_from_texts builds on the host)");
    }
    DevBuf text, codes, col[7], hist, offs, tile_cnt, tile_off, scan_tmp, scalars, run_sym, run_start, run_head, run_tail;
    DevBuf *all[] = {&text, &codes, &col[0], &col[1], &col[2], &col[3], &col[4], &col[5], &col[6], &hist, &offs, &tile_cnt, &tile_off, &scan_tmp, &scalars,
                     &run_sym, &run_start, &run_head, &run_tail};
    struct Release { DevBuf **b; size_t k; ~Release() { for (size_t i = 0; i < k; i++) b[i]->release(); } } release_all{all, sizeof all / sizeof all[0]};
    TextBwt tb;
    hipStream_t s = nullptr;
    // ---- 0. read + upload: the texts one after the other, each closed by a newline
    text.ensure(bound.text);
    uint64_t n = 0;
    std::vector<uint64_t> text_base(n_texts);
    for (uint32_t t = 0; t < n_texts; t++) {
        std::vector<uint8_t> f;
        try { f = read_whole_file(paths[t]); }
        catch (const Error &) { throw Error(PGX_ERR_IO, std::string("Cannot open text: ") + paths[t]); }
        if (f.empty()) throw Error(PGX_ERR_FORMAT, std::string("empty text: ") + paths[t]);
        if (f.back() != '\n') f.push_back('\n');
        if (n + f.size() > bound.n) throw Error(PGX_ERR_IO, std::string("text changed while it was read: ") + paths[t]);
        text_base[t] = n;
        HIPCHECK(hipMemcpy(text.as<uint8_t>() + n, f.data(), f.size(), hipMemcpyHostToDevice));
        n += f.size();
    }
    if (n != total) throw Error(PGX_ERR_IO, "a text changed while it was read");
    const Plan pl(n);
    ms[0] = clk.lap();
    // ---- 1. codes, sequence table, first keys, first sort
    codes.ensure(pl.codes);
    for (DevBuf &b : col) b.ensure(pl.column);
    hist.ensure(pl.hist); offs.ensure(pl.offs); tile_cnt.ensure(pl.tile_cnt); tile_off.ensure(pl.tile_off); scan_tmp.ensure(pl.scan_tmp); scalars.ensure(pl.scalars);
    uint64_t allocated = 0;
    for (DevBuf *b : all) allocated += b->cap;
    const unsigned nt = grid_for(n, PGX_SA_TILE), nrow = grid_for(n, 256);
    HIPCHECK(hipMemsetAsync(codes.p, 0, pl.codes, s));
    HIPCHECK(hipMemsetAsync(scalars.p, 0xFF, 8, s));
    hipLaunchKernelGGL(pgx_sa_classify_kernel, dim3(nt), dim3(256), 0, s, (const uint8_t *)text.as<uint8_t>(), n, codes.as<uint64_t>(), pl.n_words,
                       tile_cnt.as<uint32_t>(), scalars.as<unsigned long long>());
    HIPCHECK(hipGetLastError());
    scan_excl(0, tile_cnt.p, pl.n_tiles, 0, tile_off.as<uint64_t>(), scan_tmp, s);
    const uint64_t first_bad = read_u64(scalars.as<uint64_t>(), s), n_seq = read_u64(tile_off.as<uint64_t>() + pl.n_tiles, s);
    if (first_bad != ~0ull) {
        uint8_t byte = 0;
        if (first_bad < n) HIPCHECK(hipMemcpy(&byte, text.as<uint8_t>() + first_bad, 1, hipMemcpyDeviceToHost));
        uint32_t t = n_texts - 1;
        while (t > 0 && text_base[t] > first_bad) t--;
        char hex[8];
        std::snprintf(hex, sizeof hex, "0x%02X", (unsigned)byte);
        throw Error(PGX_ERR_UNSUPPORTED, std::string("byte ") + hex + " at offset " + std::to_string(first_bad - text_base[t]) + " of " + paths[t] +
                                             " (offset " + std::to_string(first_bad) + " of the collection) is outside {\\n,A,C,G,N,T}");
    }
    if (n_seq == 0 || n_seq > n) throw Error(PGX_ERR_HIP, "sequence table of the device build is inconsistent");
    Columns c{&col[0], &col[1], &col[2], &col[3], &col[4], &col[5]};
    DevBuf &rank = col[6];
    // (the sequence starts lie in the rank column until they are downloaded: no rank exists before the first sort)
    hipLaunchKernelGGL(pgx_sa_keys_kernel, dim3(nt), dim3(256), 0, s, (const uint64_t *)codes.as<uint64_t>(), pl.n_words, n, (const uint64_t *)tile_off.as<uint64_t>(),
                       n_seq, c.hi->as<uint32_t>(), c.lo->as<uint32_t>(), c.idx->as<uint32_t>(), rank.as<uint32_t>());
    HIPCHECK(hipGetLastError());
    {
        std::vector<uint32_t> st(n_seq);
        HIPCHECK(hipMemcpy(st.data(), rank.p, n_seq * 4, hipMemcpyDeviceToHost));
        tb.seq_start.assign(st.begin(), st.end());
    }
    tb.n = n;
    PassTimer pt;
    sort_columns(c, pl, bits_below(n_seq), 3 * PGX_SA_K, hist, offs, scan_tmp, s, pt);
    auto count_groups = [&]() {
        hipLaunchKernelGGL(pgx_sa_heads_kernel, dim3(nt), dim3(256), 0, s, (const uint32_t *)c.hi->as<uint32_t>(), (const uint32_t *)c.lo->as<uint32_t>(), n,
                           tile_cnt.as<uint32_t>());
        HIPCHECK(hipGetLastError());
        scan_excl(0, tile_cnt.p, pl.n_tiles, 0, tile_off.as<uint64_t>(), scan_tmp, s);
        return read_u64(tile_off.as<uint64_t>() + pl.n_tiles, s); // the one scalar a round reads back
    };
    uint64_t groups = count_groups();
    ms[1] = clk.lap();
    // ---- 2. doubling: suffixes sorted by their first h symbols -> by their first 2 h
    unsigned rounds = 0;
    for (uint64_t h = PGX_SA_K; groups < n; h *= 2) {
        if (rounds == kMaxRounds || groups == 0) throw Error(PGX_ERR_HIP, "suffix sort did not converge after " + std::to_string(rounds) + " doubling rounds");
        hipLaunchKernelGGL(pgx_sa_ranks_kernel, dim3(nt), dim3(256), 0, s, (const uint32_t *)c.hi->as<uint32_t>(), (const uint32_t *)c.lo->as<uint32_t>(),
                           (const uint32_t *)c.idx->as<uint32_t>(), n, (const uint64_t *)tile_off.as<uint64_t>(), c.hi2->as<uint32_t>(), rank.as<uint32_t>());
        HIPCHECK(hipGetLastError());
        std::swap(c.hi, c.hi2);
        hipLaunchKernelGGL(pgx_sa_gather_kernel, dim3(nrow), dim3(256), 0, s, (const uint32_t *)c.idx->as<uint32_t>(), (const uint32_t *)rank.as<uint32_t>(), n, h,
                           c.lo->as<uint32_t>());
        HIPCHECK(hipGetLastError());
        const unsigned bits = bits_below(groups);
        sort_columns(c, pl, bits, bits, hist, offs, scan_tmp, s, pt);
        const uint64_t before = groups;
        groups = count_groups();
        rounds++;
        if (groups < before || groups > n) throw Error(PGX_ERR_HIP, "suffix sort lost groups in doubling round " + std::to_string(rounds));
    }
    ms[2] = clk.lap();
    ms[5] = (double)rounds;
    // ---- 3. BWT (over the codes), logical runs, their first and last suffixes; R entries come back, not n
    DevBuf &sa = *c.idx;
    for (DevBuf &b : col)
        if (&b != &sa) b.release();
    hist.release(); offs.release();
    hipLaunchKernelGGL(pgx_sa_bwt_kernel, dim3(nrow), dim3(256), 0, s, (const uint32_t *)sa.as<uint32_t>(), (const uint8_t *)text.as<uint8_t>(), n, codes.as<uint8_t>());
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(pgx_sa_run_heads_kernel, dim3(nt), dim3(256), 0, s, (const uint8_t *)codes.as<uint8_t>(), n, tile_cnt.as<uint32_t>());
    HIPCHECK(hipGetLastError());
    scan_excl(0, tile_cnt.p, pl.n_tiles, 0, tile_off.as<uint64_t>(), scan_tmp, s);
    const uint64_t R = read_u64(tile_off.as<uint64_t>() + pl.n_tiles, s);
    if (R == 0 || R > n) throw Error(PGX_ERR_HIP, "run table of the device build is inconsistent");
    run_sym.ensure(R); run_start.ensure(R * 4); run_head.ensure(R * 4); run_tail.ensure(R * 4);
    hipLaunchKernelGGL(pgx_sa_runs_kernel, dim3(nt), dim3(256), 0, s, (const uint8_t *)codes.as<uint8_t>(), (const uint32_t *)sa.as<uint32_t>(), n,
                       (const uint64_t *)tile_off.as<uint64_t>(), R, run_sym.as<uint8_t>(), run_start.as<uint32_t>(), run_head.as<uint32_t>(), run_tail.as<uint32_t>());
    HIPCHECK(hipGetLastError());
    {
        std::vector<uint8_t> sym(R);
        std::vector<uint32_t> start(R), head(R), tail(R);
        HIPCHECK(hipMemcpy(sym.data(), run_sym.p, R, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(start.data(), run_start.p, R * 4, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(head.data(), run_head.p, R * 4, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(tail.data(), run_tail.p, R * 4, hipMemcpyDeviceToHost));
        tb.head.assign(head.begin(), head.end());
        tb.tail.assign(tail.begin(), tail.end());
        tb.max_len = 1;
        for (uint64_t k = 0; k < R; k++) { // file runs: the logical runs with neighbouring endmarker runs merged
            const uint64_t len = (k + 1 < R ? (uint64_t)start[k + 1] : n) - start[k];
            if (sym[k] == '\n' && !tb.runs.empty() && tb.runs.back().first == '\n') tb.runs.back().second += len;
            else tb.runs.emplace_back(sym[k], len);
            tb.max_len = std::max(tb.max_len, tb.runs.back().second);
        }
    }
    HIPCHECK(hipStreamSynchronize(s));
    for (DevBuf *b : all) b->release();
    ms[3] = clk.lap();
    if (pt.on) {
        const double pass_bytes = (double)n * (4 + 24); // keys read by the histogram; three columns read and written by the scatter
        std::fprintf(stderr, "[pgx build] device: n %llu sequences %llu runs %llu rounds %u | device bytes allocated %llu planned %llu | radix passes %llu in %.3f ms, "
                             "%.0f bytes a pass, %.1f GB/s\n",
                     (unsigned long long)n, (unsigned long long)n_seq, (unsigned long long)R, rounds, (unsigned long long)allocated, (unsigned long long)pl.bytes(),
                     (unsigned long long)pt.passes, pt.ms, pass_bytes, pt.ms > 0 ? pass_bytes * (double)pt.passes / pt.ms / 1e6 : 0.0);
    }
    // ---- 4. the files, under temporary names until both are complete: an error anywhere leaves none behind
    // (the .ri is renamed first: a failure of the second rename then removes only a file this call wrote, never an .rl_bwt that was there before)
    static std::atomic<uint64_t> serial{0};
    const std::string suffix = ".tmp." + std::to_string((long)getpid()) + "." + std::to_string(serial.fetch_add(1));
    const std::string tmp_rl = out_rlbwt_path ? std::string(out_rlbwt_path) + suffix : std::string(), tmp_ri = std::string(out_ri_path) + suffix;
    try {
        if (out_rlbwt_path) write_rlbwt(tmp_rl.c_str(), tb);
        build_rindex_core(tb.runs, &tb, tmp_ri.c_str(), encoded);
        if (std::rename(tmp_ri.c_str(), out_ri_path) != 0) throw Error(PGX_ERR_IO, std::string("Cannot create file: ") + out_ri_path);
        if (out_rlbwt_path && std::rename(tmp_rl.c_str(), out_rlbwt_path) != 0) {
            std::remove(out_ri_path);
            throw Error(PGX_ERR_IO, std::string("Cannot create file: ") + out_rlbwt_path);
        }
    } catch (...) {
        if (out_rlbwt_path) std::remove(tmp_rl.c_str());
        std::remove(tmp_ri.c_str());
        throw;
    }
    ms[4] = clk.lap();
}
} // namespace

extern "C" pgx_status pgx_build_index_from_texts_device(const char *const *text_paths, uint32_t n_texts, const char *out_rlbwt_path, const char *out_ri_path,
                                                        int encoded, int device) {
    PGX_GUARD_BEGIN
    double *ms = g_build_device_ms;
    std::fill(ms, ms + 6, 0.0);
    if (!text_paths || !n_texts || !out_ri_path) throw Error(PGX_ERR_ARG, "pgx_build_index_from_texts_device: null argument");
    for (uint32_t i = 0; i < n_texts; i++)
        if (!text_paths[i]) throw Error(PGX_ERR_ARG, "pgx_build_index_from_texts_device: null path");
    build_index_device_core(text_paths, n_texts, out_rlbwt_path, out_ri_path, encoded, device, ms);
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_build_index_from_text_device(const char *text_path, const char *out_rlbwt_path, const char *out_ri_path, int encoded, int device) {
    PGX_GUARD_BEGIN
    double *ms = g_build_device_ms;
    std::fill(ms, ms + 6, 0.0);
    if (!text_path || !out_ri_path) throw Error(PGX_ERR_ARG, "pgx_build_index_from_text_device: null argument");
    const char *one[1] = {text_path};
    build_index_device_core(one, 1, out_rlbwt_path, out_ri_path, encoded, device, ms);
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_build_index_device_timing(double *ms, uint32_t n) {
    PGX_GUARD_BEGIN
    if (!ms && n) throw Error(PGX_ERR_ARG, "pgx_build_index_device_timing: null argument");
    for (uint32_t i = 0; i < n && i < 6; i++) ms[i] = g_build_device_ms[i];
    return PGX_OK;
    PGX_GUARD_END
}
