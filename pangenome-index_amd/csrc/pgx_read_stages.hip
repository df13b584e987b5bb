// pgx_read_stages.hip -- the read stages behind a run: hits, place, verify, rescue, mates, align, walk, mapq.  Each is a core on device arrays with two entry points, one on
// the batch (pgx_batch_read_X with its results pgx_batch_device_X / pgx_batch_X) and one on host arrays (pgx_read_X_arrays), and what they share comes first.
// A batch entry point clears its `valid` only behind its last refusal, so that what it refuses leaves the result before as it was (hits differs: see there).
#include <string>

#include "pgx_batch_internal.hpp"

// ------------------------------------------------------------------------------------------
// shared by the stages
// reads, MEMs, keys or candidates one launch takes at a thread an item or fewer: a grid holds fewer than 2^32 threads, and a larger one would lose items without an error
static const uint64_t PLACE_LAUNCH_ITEMS = 1ull << 31;

size_t free_device_memory() {
    size_t mem_free = 0, mem_total = 0;
    if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); mem_free = 1ull << 30; }
    return mem_free;
}

// what the _arrays entry points ask of an offsets array of k items (o[k] is read)
void check_offsets(const std::string &who, const uint64_t *o, uint64_t k, const char *name, const char *item) {
    if (o[0] != 0) throw Error(PGX_ERR_ARG, who + ": " + name + " must start at 0");
    for (uint64_t i = 0; i < k; i++)
        if (o[i] > o[i + 1]) throw Error(PGX_ERR_ARG, who + ": " + name + " decrease at " + item + " " + std::to_string(i));
}

// and of a text of n_text symbols: its size, then its bytes (text == nullptr: the size alone, walk takes no bytes)
static void check_text(const std::string &who, const uint8_t *text, uint64_t n_text) {
    if (n_text >= (1ull << 32) - (1ull << 20)) throw Error(PGX_ERR_UNSUPPORTED, who + ": a text of " + std::to_string(n_text) + " symbols, the image holds fewer than 2^32 - 2^20");
    for (uint64_t i = 0; text && i < n_text; i++) {
        const uint8_t c = text[i];
        if (c != '\n' && c != 'A' && c != 'C' && c != 'G' && c != 'N' && c != 'T')
            throw Error(PGX_ERR_UNSUPPORTED, who + ": text byte " + std::to_string((unsigned)c) + " at offset " + std::to_string(i) + " is none of \\n A C G N T");
    }
}

// the reads at the text's symbol width into rcode (grown first), once per read whatever is done with it: verify_core, and align where no verify call came before
static void code_reads(DevBuf &rcode, const uint8_t *reads, uint64_t read_bytes, hipStream_t s) {
    const uint64_t n_rw = (read_bytes + 7) / 8 + 1;
    rcode.ensure(n_rw * 4);
    hipLaunchKernelGGL(pgx_verify_code_kernel, dim3((unsigned)std::min<uint64_t>((n_rw + 255) / 256, 1u << 20)), dim3(256), 0, s, reads, read_bytes, n_rw, rcode.as<uint32_t>());
}

// The text and the reads of pgx_read_verify_arrays / pgx_read_align_arrays on the device, released on every way out: upload() on the null stream, then
// pack() the text's bytes to the 4-bit symbols of a TEXT image (pgx_image.h).
namespace {
struct TextInput {
    DevBuf text8, text4, seq_off, reads, read_off;
    uint64_t n_text = 0;
    ~TextInput() { release_all({&text8, &text4, &seq_off, &reads, &read_off}); }
    void upload(const uint8_t *text, const uint64_t *seq_offsets, uint64_t n_seq, const uint8_t *read_bytes, const uint64_t *read_offsets, uint64_t n_reads) {
        n_text = seq_offsets[n_seq];
        ::upload(text8, text, n_text);
        ::upload(seq_off, seq_offsets, (n_seq + 1) * 8);
        ::upload(reads, read_bytes, read_offsets[n_reads]);
        ::upload(read_off, read_offsets, (n_reads + 1) * 8);
    }
    void pack(hipStream_t s) {
        const uint64_t n_words = (n_text + 7) / 8 + PGX_TEXT_PAD_WORDS;
        text4.ensure(n_words * 4);
        hipLaunchKernelGGL(pgx_text_pack_kernel, dim3((unsigned)std::min<uint64_t>((n_words + 255) / 256, 1u << 20)), dim3(256), 0, s, (const uint8_t *)text8.as<uint8_t>(), n_text, n_words,
                           1u, text4.as<uint32_t>());
    }
};
} // namespace

// ------------------------------------------------------------------------------------------
// read hits (pgx_hits_kernels.hip; the definitions: include/pgx.h "read hits")
static const uint32_t HITS_FLAGS = PGX_HITS_BEST_SETS | PGX_HITS_SCORES;

// log2 of the lanes a read takes (Sp: the power of two >= n_seq, 64 with more than one word column); refuses what one launch cannot hold
static uint32_t hits_lane_shift(uint64_t n_reads, uint64_t n_seq, uint32_t W, const char *who) {
    uint32_t sp_shift = 0;
    while (W == 1 && (1ull << sp_shift) < n_seq) sp_shift++;
    if (W > 1) sp_shift = 6;
    // (a grid holds fewer than 2^32 threads: a larger launch would lose reads without an error)
    if (n_reads > (((1ull << 32) - PGX_HITS_THREADS) >> sp_shift))
        throw Error(PGX_ERR_UNSUPPORTED, std::string(who) + ": " + std::to_string(n_reads) + " reads at " + std::to_string(1u << sp_shift) +
                                             " lanes a read exceed the 2^32 threads of one launch: score the reads in smaller batches");
    return sp_shift;
}

// the one launch: sizes the outputs the flags ask for and enqueues the kernel on s (sets: n_mems x W words on the device)
static void hits_launch(HitsWork &w, const uint64_t *mem_off, const pgx_mem *mems, const uint64_t *sets, uint64_t n_reads, uint64_t n_mems, uint64_t n_seq, uint32_t W,
                        uint32_t flags, hipStream_t s) {
    const uint32_t sp_shift = hits_lane_shift(n_reads, n_seq, W, "read hits");
    w.hits.ensure((n_reads ? n_reads : 1) * sizeof(pgx_read_hit));
    if (flags & PGX_HITS_BEST_SETS) w.best_sets.ensure((n_reads ? n_reads * W : 1) * 8);
    if (flags & PGX_HITS_SCORES) w.scores.ensure((n_reads ? n_reads * n_seq : 1) * 4);
    if (!n_reads) return;
    unsigned long long *best = (flags & PGX_HITS_BEST_SETS) ? w.best_sets.as<unsigned long long>() : nullptr;
    uint32_t *scores = (flags & PGX_HITS_SCORES) ? w.scores.as<uint32_t>() : nullptr;
    const unsigned long long *dsets = reinterpret_cast<const unsigned long long *>(sets);
    if (W == 1) { // Sp lanes a read
        hipLaunchKernelGGL(pgx_read_hits_kernel, dim3(grid_for(n_reads, PGX_HITS_THREADS >> sp_shift)), dim3(PGX_HITS_THREADS), 0, s, mem_off, mems, dsets, n_reads, n_mems,
                           n_seq, sp_shift, flags, w.hits.as<pgx_read_hit>(), best, scores);
    } else // a wave a read
        hipLaunchKernelGGL(pgx_read_hits_wide_kernel, dim3(grid_for(n_reads, PGX_HITS_THREADS / 64)), dim3(PGX_HITS_THREADS), 0, s, mem_off, mems, dsets, n_reads, n_mems,
                           n_seq, W, flags, w.hits.as<pgx_read_hit>(), best, scores);
    HIPCHECK(hipGetLastError());
}

extern "C" pgx_status pgx_batch_read_hits(pgx_batch *b, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_read_hits");
    checked_device_count();
    if (!b) throw Error(PGX_ERR_ARG, "pgx_batch_read_hits: null batch");
    HitsWork &w = b->hw;
    w.valid = false; // (before the refusals, unlike the stages below: a refused call leaves no hits; tests/test_gpu_hits.py pins it)
    if (flags & ~HITS_FLAGS) throw Error(PGX_ERR_ARG, "pgx_batch_read_hits: unknown flag");
    if (!b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_read_hits: batch has not been run");
    const LocWork &lw = b->lw;
    if (!lw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_read_hits: needs a completed pgx_batch_locate(PGX_LOCATE_SEQ_SETS), the batch has no locate result");
    if (lw.flags != PGX_LOCATE_SEQ_SETS || lw.n_mems != b->n_mems || !lw.set_words)
        throw Error(PGX_ERR_ARG, "pgx_batch_read_hits: needs a completed pgx_batch_locate(PGX_LOCATE_SEQ_SETS), the last pgx_batch_locate ran with flags " +
                                     std::to_string(lw.flags));
    use_device(b->device);
    hipStream_t s = batch_stream(b, stream);
    const uint64_t n = b->n_reads, n_seq = b->h->meta.n_sequences();
    const uint32_t W = lw.set_words;
    (void)hits_lane_shift(n, n_seq, W, "pgx_batch_read_hits");
    if (flags & PGX_HITS_SCORES) {
        const size_t mem_free = free_device_memory();
        const uint64_t need = n * n_seq * 4;
        if (need > mem_free / 4)
            throw Error(PGX_ERR_NOMEM, "pgx_batch_read_hits: PGX_HITS_SCORES takes " + std::to_string(need) + " bytes, a quarter of the free device memory is " +
                                           std::to_string(mem_free / 4));
    }
    w.timer.begin(b->timed, s);
    hits_launch(w, b->mem_off.as<uint64_t>(), b->mems.as<pgx_mem>(), lw.vals.as<uint64_t>(), n, b->n_mems, n_seq, W, flags, s);
    w.ms = w.timer.end(s);
    if (!b->timed) HIPCHECK(hipStreamSynchronize(s)); // (a timed call has waited in end())
    w.flags = flags;
    w.set_words = W;
    w.n_reads = n;
    w.n_seq = n_seq;
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void hits_header(const pgx_batch *b, pgx_read_hits *out) {
    const HitsWork &w = b->hw;
    std::memset(out, 0, sizeof *out);
    out->n_reads = w.n_reads;
    out->n_seq = w.n_seq;
    out->set_words = w.set_words;
    out->flags = w.flags;
    out->ms_hits = w.ms;
}

extern "C" pgx_status pgx_batch_device_hits(pgx_batch *b, pgx_read_hits *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->hw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_hits: batch has no hits result");
    const HitsWork &w = b->hw;
    hits_header(b, out);
    out->hits = w.hits.as<pgx_read_hit>();
    out->best_sets = (w.flags & PGX_HITS_BEST_SETS) ? w.best_sets.as<uint64_t>() : nullptr;
    out->scores = (w.flags & PGX_HITS_SCORES) ? w.scores.as<uint32_t>() : nullptr;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_hits(pgx_batch *b, pgx_read_hits *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->hw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_hits: batch has no hits result");
    use_device(b->device);
    HitsWork &w = b->hw;
    const uint64_t n = w.n_reads;
    const bool best = (w.flags & PGX_HITS_BEST_SETS) != 0, scores = (w.flags & PGX_HITS_SCORES) != 0;
    w.h_hits.ensure((n ? n : 1) * sizeof(pgx_read_hit));
    if (n) HIPCHECK(hipMemcpyAsync(w.h_hits.p, w.hits.p, n * sizeof(pgx_read_hit), hipMemcpyDeviceToHost, b->own));
    if (best) {
        w.h_best_sets.ensure((n ? n * w.set_words : 1) * 8);
        if (n) HIPCHECK(hipMemcpyAsync(w.h_best_sets.p, w.best_sets.p, n * w.set_words * 8, hipMemcpyDeviceToHost, b->own));
    }
    if (scores) {
        w.h_scores.ensure((n ? n * w.n_seq : 1) * 4);
        if (n) HIPCHECK(hipMemcpyAsync(w.h_scores.p, w.scores.p, n * w.n_seq * 4, hipMemcpyDeviceToHost, b->own));
    }
    HIPCHECK(hipStreamSynchronize(b->own)); // (the kernel completed inside pgx_batch_read_hits, on whatever stream it used)
    hits_header(b, out);
    out->hits = w.h_hits.as<pgx_read_hit>();
    out->best_sets = best ? w.h_best_sets.as<uint64_t>() : nullptr;
    out->scores = scores ? w.h_scores.as<uint32_t>() : nullptr;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_read_hits_arrays(int device, const uint64_t *mem_offsets, uint64_t n_reads, const pgx_mem *mems, const uint64_t *sets, uint32_t set_words,
                                           uint64_t n_seq, uint32_t flags, pgx_read_hit *hits, uint64_t *best_sets, uint32_t *scores) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_hits_arrays");
    checked_device_count();
    if (flags & ~HITS_FLAGS) throw Error(PGX_ERR_ARG, "pgx_read_hits_arrays: unknown flag");
    if (set_words < 1 || set_words > PGX_ML_SET_WORDS_MAX || n_seq == 0 || (n_seq + 63) / 64 != set_words)
        throw Error(PGX_ERR_ARG, "pgx_read_hits_arrays: set_words must be ceil(n_seq / 64) and 1 .. " + std::to_string(PGX_ML_SET_WORDS_MAX) + ", got set_words " +
                                     std::to_string(set_words) + " for n_seq " + std::to_string(n_seq));
    if (!mem_offsets || (n_reads && !hits) || ((flags & PGX_HITS_BEST_SETS) && n_reads && !best_sets) || ((flags & PGX_HITS_SCORES) && n_reads && !scores))
        throw Error(PGX_ERR_ARG, "pgx_read_hits_arrays: null argument");
    (void)hits_lane_shift(n_reads, n_seq, set_words, "pgx_read_hits_arrays"); // (before the arrays are read)
    bool ok = mem_offsets[0] == 0;
    for (uint64_t i = 0; ok && i < n_reads; i++) ok = mem_offsets[i] <= mem_offsets[i + 1];
    if (!ok) throw Error(PGX_ERR_ARG, "pgx_read_hits_arrays: mem_offsets must start at 0 and never decrease");
    const uint64_t m = mem_offsets[n_reads];
    if (m && (!mems || !sets)) throw Error(PGX_ERR_ARG, "pgx_read_hits_arrays: null argument");
    use_device(device);
    struct HitsInput { // device copies of the input + the stage's buffers, released on every way out
        DevBuf mem_off, mems, sets;
        HitsWork w;
        ~HitsInput() { release_all({&mem_off, &mems, &sets}); w.release(); }
    } k;
    upload(k.mem_off, mem_offsets, (n_reads + 1) * 8);
    upload(k.mems, mems, m * sizeof(pgx_mem));
    upload(k.sets, sets, m * set_words * 8);
    hipStream_t s = nullptr;
    if (n_reads) { // the precondition, before anything is written
        k.w.bad.ensure(8);
        HIPCHECK(hipMemsetAsync(k.w.bad.p, 0xFF, 8, s));
        hipLaunchKernelGGL(pgx_read_hits_check_kernel, dim3(grid_for(n_reads, 256)), dim3(256), 0, s, (const uint64_t *)k.mem_off.as<uint64_t>(),
                           (const pgx_mem *)k.mems.as<pgx_mem>(), n_reads, m, k.w.bad.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
        const uint64_t bad = read_u64(k.w.bad.as<uint64_t>(), s);
        if (bad != ~0ull) throw Error(PGX_ERR_ARG, "pgx_read_hits_arrays: the MEM starts of read " + std::to_string(bad) + " do not ascend strictly");
    }
    hits_launch(k.w, k.mem_off.as<uint64_t>(), k.mems.as<pgx_mem>(), k.sets.as<uint64_t>(), n_reads, m, n_seq, set_words, flags, s);
    if (n_reads) {
        HIPCHECK(hipMemcpyAsync(hits, k.w.hits.p, n_reads * sizeof(pgx_read_hit), hipMemcpyDeviceToHost, s));
        if (flags & PGX_HITS_BEST_SETS) HIPCHECK(hipMemcpyAsync(best_sets, k.w.best_sets.p, n_reads * set_words * 8, hipMemcpyDeviceToHost, s));
        if (flags & PGX_HITS_SCORES) HIPCHECK(hipMemcpyAsync(scores, k.w.scores.p, n_reads * n_seq * 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// read placement (pgx_place_kernels.hip; the definitions: include/pgx.h "read placement")
static const uint32_t PLACE_FLAGS = PGX_PLACE_LIST;

// keys one pass may hold: PGX_PLACE_BUDGET_MB (read per call, fractions allowed), default a quarter of the free device memory
static uint64_t place_budget_keys(size_t mem_free) {
    uint64_t bytes = 0;
    if (const char *e = std::getenv("PGX_PLACE_BUDGET_MB")) {
        const double mb = std::strtod(e, nullptr);
        if (mb > 0) bytes = (uint64_t)(mb * 1048576.0);
    }
    if (!bytes) bytes = mem_free / 4;
    return std::min<uint64_t>(std::max<uint64_t>(bytes / 8, 1), PLACE_LAUNCH_ITEMS);
}

static uint32_t place_bits(unsigned __int128 v) {
    uint32_t b = 0;
    while (v) { b++; v >>= 1; }
    return b;
}

// log2 of the lanes a read of the sweep takes: the power of two >= twice the mean anchors a read of the pass, 4 .. 64 (a longer read takes more
// steps).  PGX_PLACE_LANES (tests; 1 .. 64, rounded up to a power of two) fixes it.  Results never depend on it.
static uint32_t place_lane_shift(uint64_t keys, uint64_t reads) {
    uint64_t want = reads ? 2 * ((keys + reads - 1) / reads) : 4;
    want = std::min<uint64_t>(std::max<uint64_t>(want, 4), 64);
    if (const char *e = std::getenv("PGX_PLACE_LANES")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= 64) want = (uint64_t)v;
    }
    uint32_t sh = 0;
    while ((1ull << sh) < want) sh++;
    return sh;
}

// The stage on device arrays, enqueued on s (synchronised where a size is read back): w.recs, and with PGX_PLACE_LIST w.place_off / w.places.
// loc_off: n_mems + 1 value offsets, values: n_values.  Refuses before a result buffer is written.
static void place_core(PlaceWork &w, const uint64_t *mem_off, const pgx_mem *mems, const uint64_t *loc_off, const uint64_t *values, uint64_t n, uint64_t n_mems,
                       uint64_t n_values, uint64_t n_seq, uint64_t L, uint32_t flags, size_t mem_free, hipStream_t s, const std::string &who) {
    if (n >= PLACE_LAUNCH_ITEMS || n_mems >= PLACE_LAUNCH_ITEMS)
        throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n) + " reads with " + std::to_string(n_mems) + " MEMs exceed the " + std::to_string(PLACE_LAUNCH_ITEMS) +
                                             " one launch holds: place the reads in smaller batches");
    const bool list = (flags & PGX_PLACE_LIST) != 0;
    // 1. plan: the anchors of every read, the first MEM of every MEM's read, the maxima of the key layout
    //    ctr: [0] most MEMs of a read [1] largest MEM start [2] aoff[n] [3] aoff[0]; later [0] wave list [1] workgroup list [2] scratch total [3] placements of a pass [6..7] cut
    w.aoff.ensure((n + 1) * 8); w.acnt.ensure((n ? n : 1) * 8); w.mfirst.ensure((n_mems ? n_mems : 1) * 8); w.ctr.ensure(64);
    unsigned long long *ctr = w.ctr.as<unsigned long long>();
    HIPCHECK(hipMemsetAsync(w.ctr.p, 0, 64, s));
    hipLaunchKernelGGL(pgx_place_plan_kernel, dim3(grid_for(n + 1, 256)), dim3(256), 0, s, mem_off, loc_off, mems, n, n_mems, n_values, w.aoff.as<uint64_t>(),
                       w.acnt.as<uint64_t>(), ctr);
    if (n_mems) hipLaunchKernelGGL(pgx_place_first_kernel, dim3(grid_for(n_mems, 256)), dim3(256), 0, s, mem_off, n, n_mems, w.mfirst.as<uint64_t>());
    HIPCHECK(hipGetLastError());
    uint64_t c[4];
    read_scalars(c, ctr, 32, s);
    const uint64_t most_mems = c[0], bias = c[1], a_end = c[2], a_begin = std::min(c[3], c[2]);
    const uint32_t ordinal_bits = place_bits(most_mems ? most_mems - 1 : 0);
    const uint64_t span = L + bias;
    const uint32_t group_bits = span < L ? 65u : place_bits((unsigned __int128)n_seq * span);
    if (group_bits + ordinal_bits > 64)
        throw Error(PGX_ERR_UNSUPPORTED, who + ": a key needs " + std::to_string(group_bits) + " bits for sequence and diagonal (" + std::to_string(n_seq) + " sequences x (max_length " +
                                             std::to_string(L) + " + largest MEM start " + std::to_string(bias) + ")) and " + std::to_string(ordinal_bits) +
                                             " bits for the MEM of a read (most MEMs of a read: " + std::to_string(most_mems) + "), 64 are available");
    const uint64_t budget = place_budget_keys(mem_free);
    const uint64_t *aoff = w.aoff.as<uint64_t>(), *acnt = w.acnt.as<uint64_t>();
    w.recs.ensure((n ? n : 1) * sizeof(pgx_read_place)); w.pcount.ensure((n ? n : 1) * 8);
    // 2. passes over consecutive whole reads whose keys fit the budget (one pass unless the batch exceeds it)
    uint64_t U = 0; // placements listed by the passes so far
    uint32_t passes = 0;
    for (uint64_t r0 = 0, o0 = a_begin; r0 < n;) {
        uint64_t r1 = n, o1 = a_end;
        if (a_end - o0 > budget) {
            hipLaunchKernelGGL(pgx_ml_cut_kernel, dim3(1), dim3(64), 0, s, aoff, n, r0, budget, reinterpret_cast<uint64_t *>(ctr + 6));
            HIPCHECK(hipGetLastError());
            uint64_t cut[2];
            read_scalars(cut, ctr + 6, 16, s);
            r1 = cut[0]; o1 = cut[1];
            if (o1 - o0 > budget) // (the cut is a read at least)
                throw Error(PGX_ERR_NOMEM, who + ": read " + std::to_string(r0) + " has " + std::to_string(o1 - o0) + " anchors, the keys of a pass hold " + std::to_string(budget) +
                                               " (PGX_PLACE_BUDGET_MB)");
        }
        const uint64_t np = r1 - r0, nk = o1 - o0;
        passes++;
        // keys, then the segmented sort of the tag stage: a read is a segment, the size-class lists are built on the device
        w.keys.ensure((nk ? nk : 1) * 8);
        w.seg.ensure((np + 1) * 8); w.lists.ensure(2 * np * 8); w.need.ensure(np * 8); w.soff.ensure((np + 1) * 8); w.ucount.ensure(np * 8);
        uint64_t *keys = w.keys.as<uint64_t>(), *seg = w.seg.as<uint64_t>(), *wave_list = w.lists.as<uint64_t>(), *wg_list = wave_list + np, *ucount = w.ucount.as<uint64_t>();
        if (nk) {
            hipLaunchKernelGGL(pgx_place_keys_kernel, dim3(grid_for(nk, PGX_ML_SPAN)), dim3(256), 0, s, mems, loc_off, (const uint64_t *)w.mfirst.as<uint64_t>(), values,
                               (uint64_t)0, n_mems, o0, nk, L, span, bias, ordinal_bits, keys);
            HIPCHECK(hipGetLastError());
        }
        HIPCHECK(hipMemsetAsync(w.ctr.p, 0, 32, s));
        hipLaunchKernelGGL(pgx_ml_classify_kernel, dim3(grid_for(np + 1, 256)), dim3(256), 0, s, acnt + r0, aoff + r0, np, seg, wave_list, wg_list, w.need.as<uint64_t>(),
                           ucount, ctr);
        HIPCHECK(hipGetLastError());
        scan_excl(1, w.need.p, np, 0, w.soff.as<uint64_t>(), w.scan_tmp, s, reinterpret_cast<uint64_t *>(ctr + 2));
        uint64_t lc[3];
        read_scalars(lc, ctr, 24, s);
        const uint64_t n_wave = lc[0], n_wg = lc[1], S = lc[2];
        if (n_wave)
            hipLaunchKernelGGL(pgx_tag_sort_unique_kernel<PgxTagDense>, dim3(grid_for(n_wave, 4)), dim3(256), 0, s, PgxTagDense{wave_list, acnt + r0, seg}, n_wave,
                               (const uint64_t *)nullptr, (const uint64_t *)nullptr, keys, ucount);
        if (n_wg) {
            w.scratch.ensure((S ? S : 1) * 8);
            HIPCHECK(hipFuncSetAttribute((const void *)pgx_tag_sort_large_kernel<PgxTagDense>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(PGX_SORT_WG_LDS_CAP * 8)));
            hipLaunchKernelGGL(pgx_tag_sort_large_kernel<PgxTagDense>, dim3(grid_for(n_wg, 1)), dim3(1024), (size_t)PGX_SORT_WG_LDS_CAP * 8, s,
                               PgxTagDense{wg_list, acnt + r0, seg}, n_wg, (const uint64_t *)nullptr, (const uint64_t *)nullptr, keys, w.scratch.as<uint64_t>(),
                               (const uint64_t *)w.soff.as<uint64_t>(), ucount);
        }
        HIPCHECK(hipGetLastError());
        // the sweep, in launches of fewer than 2^32 threads
        const uint32_t g_shift = place_lane_shift(nk, np);
        const uint64_t per_launch = PLACE_LAUNCH_ITEMS >> g_shift;
        auto sweep = [&](bool fill, const uint64_t *list_off, pgx_placement *places) {
            for (uint64_t q0 = 0; q0 < np; q0 += per_launch) {
                const uint64_t nr = std::min(per_launch, np - q0);
                const dim3 grid(grid_for(nr, PGX_PLACE_THREADS >> g_shift)), block(PGX_PLACE_THREADS);
                if (fill)
                    hipLaunchKernelGGL(pgx_place_sweep_kernel<true>, grid, block, 0, s, mem_off, mems, loc_off, acnt, (const uint64_t *)keys, (const uint64_t *)seg,
                                       (const uint64_t *)ucount, r0, r0 + q0, nr, n_mems, span, bias, ordinal_bits, g_shift, w.recs.as<pgx_read_place>(),
                                       w.pcount.as<uint64_t>(), list_off, places);
                else
                    hipLaunchKernelGGL(pgx_place_sweep_kernel<false>, grid, block, 0, s, mem_off, mems, loc_off, acnt, (const uint64_t *)keys, (const uint64_t *)seg,
                                       (const uint64_t *)ucount, r0, r0 + q0, nr, n_mems, span, bias, ordinal_bits, g_shift, w.recs.as<pgx_read_place>(),
                                       w.pcount.as<uint64_t>(), list_off, places);
                HIPCHECK(hipGetLastError());
            }
        };
        sweep(false, nullptr, nullptr);
        if (list) { // the pass's counts -> offsets behind the passes before, then the same walk writes the placements
            w.loff.ensure((np + 1) * 8);
            scan_excl(1, w.pcount.as<uint64_t>() + r0, np, 0, w.loff.as<uint64_t>(), w.scan_tmp, s, reinterpret_cast<uint64_t *>(ctr + 3));
            const uint64_t Up = read_u64(reinterpret_cast<const uint64_t *>(ctr + 3), s);
            if ((U + Up) > (mem_free / 4) / sizeof(pgx_placement))
                throw Error(PGX_ERR_NOMEM, who + ": PGX_PLACE_LIST takes at least " + std::to_string((U + Up) * sizeof(pgx_placement)) +
                                               " bytes, a quarter of the free device memory is " + std::to_string(mem_free / 4));
            w.places.ensure_keep((U + Up ? U + Up : 1) * sizeof(pgx_placement), U * sizeof(pgx_placement)); // (the stream is idle here: the read-back above synchronised it)
            if (Up) sweep(true, w.loff.as<uint64_t>(), w.places.as<pgx_placement>() + U);
            U += Up;
        }
        r0 = r1; o0 = o1;
    }
    if (list) {
        w.place_off.ensure((n + 1) * 8);
        w.places.ensure(sizeof(pgx_placement));
        scan_excl(1, w.pcount.p, n, 0, w.place_off.as<uint64_t>(), w.scan_tmp, s);
    }
    w.flags = flags;
    w.n_reads = n;
    w.n_anchors = a_end - a_begin;
    w.n_places = U;
    w.n_passes = passes;
}

extern "C" pgx_status pgx_batch_read_place(pgx_batch *b, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_read_place");
    checked_device_count();
    if (!b) throw Error(PGX_ERR_ARG, "pgx_batch_read_place: null batch");
    // (what is refused here leaves an earlier place result as it was)
    if (flags & ~PLACE_FLAGS) throw Error(PGX_ERR_ARG, "pgx_batch_read_place: unknown flag");
    if (!b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_read_place: batch has not been run");
    const LocWork &lw = b->lw;
    if (!lw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_read_place: needs a completed pgx_batch_locate(flags = 0), the batch has no locate result");
    if (lw.flags != 0 || lw.n_mems != b->n_mems)
        throw Error(PGX_ERR_ARG, "pgx_batch_read_place: needs a completed pgx_batch_locate(flags = 0), the last pgx_batch_locate ran with flags " + std::to_string(lw.flags));
    use_device(b->device);
    pgx_device_image *d = locate_image(b->h, b->device);
    hipStream_t s = batch_stream(b, stream);
    PlaceWork &w = b->pw;
    w.valid = false;
    const size_t mem_free = free_device_memory();
    w.timer.begin(b->timed, s);
    place_core(w, b->mem_off.as<uint64_t>(), b->mems.as<pgx_mem>(), lw.d_off, lw.vals.as<uint64_t>(), b->n_reads, b->n_mems, lw.n_values, b->h->meta.n_sequences(),
               d->loc.max_length, flags, mem_free, s, "pgx_batch_read_place");
    w.ms = w.timer.end(s);
    if (!b->timed) HIPCHECK(hipStreamSynchronize(s)); // (a timed call has waited in end())
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void places_header(const pgx_batch *b, pgx_read_places *out) {
    const PlaceWork &w = b->pw;
    std::memset(out, 0, sizeof *out);
    out->n_reads = w.n_reads;
    out->n_anchors = w.n_anchors;
    out->n_places = w.n_places;
    out->flags = w.flags;
    out->n_passes = w.n_passes;
    out->ms_place = w.ms;
}

extern "C" pgx_status pgx_batch_device_places(pgx_batch *b, pgx_read_places *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->pw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_places: batch has no place result");
    const PlaceWork &w = b->pw;
    places_header(b, out);
    out->reads = w.recs.as<pgx_read_place>();
    if (w.flags & PGX_PLACE_LIST) {
        out->place_offsets = w.place_off.as<uint64_t>();
        out->places = w.places.as<pgx_placement>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_places(pgx_batch *b, pgx_read_places *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->pw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_places: batch has no place result");
    use_device(b->device);
    PlaceWork &w = b->pw;
    download_pinned(b, w.result(), w.h_recs, w.h_place_off, w.h_places);
    places_header(b, out);
    out->reads = w.h_recs.as<pgx_read_place>();
    if (w.flags & PGX_PLACE_LIST) {
        out->place_offsets = w.h_place_off.as<uint64_t>();
        out->places = w.h_places.as<pgx_placement>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_read_place_arrays(int device, const uint64_t *mem_offsets, uint64_t n_reads, const pgx_mem *mems, const uint64_t *loc_offsets,
                                            const uint64_t *values, uint64_t n_seq, uint64_t max_length, uint32_t flags, pgx_read_place *out,
                                            uint64_t *place_offsets, pgx_placement *places, uint64_t places_cap) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_place_arrays");
    checked_device_count();
    if (flags & ~PLACE_FLAGS) throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: unknown flag");
    if (n_seq == 0 || max_length == 0) throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: n_seq and max_length must be positive");
    const bool list = (flags & PGX_PLACE_LIST) != 0;
    if (!mem_offsets || !loc_offsets || (n_reads && !out) || (list && (!place_offsets || (places_cap && !places))))
        throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: null argument");
    if (mem_offsets[0] != 0) throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: mem_offsets must start at 0");
    for (uint64_t i = 0; i < n_reads; i++)
        if (mem_offsets[i] > mem_offsets[i + 1])
            throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: mem_offsets decrease at read " + std::to_string(i));
    const uint64_t m = mem_offsets[n_reads];
    if (loc_offsets[0] != 0) throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: loc_offsets must start at 0");
    for (uint64_t r = 0; r < n_reads; r++)
        for (uint64_t i = mem_offsets[r]; i < mem_offsets[r + 1]; i++)
            if (loc_offsets[i] > loc_offsets[i + 1])
                throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: loc_offsets decrease at MEM " + std::to_string(i) + " of read " + std::to_string(r));
    const uint64_t nv = loc_offsets[m];
    if ((m && !mems) || (nv && !values)) throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: null argument");
    use_device(device);
    struct PlaceInput { // device copies of the input + the stage's buffers, released on every way out
        DevBuf mem_off, mems, loc_off, values;
        PlaceWork w;
        ~PlaceInput() { release_all({&mem_off, &mems, &loc_off, &values}); w.release(); }
    } k;
    const size_t mem_free = free_device_memory();
    upload(k.mem_off, mem_offsets, (n_reads + 1) * 8);
    upload(k.mems, mems, m * sizeof(pgx_mem));
    upload(k.loc_off, loc_offsets, (m + 1) * 8);
    upload(k.values, values, nv * 8);
    hipStream_t s = nullptr;
    if (n_reads) { // the preconditions, before anything is written
        if (n_reads >= PLACE_LAUNCH_ITEMS || nv >= (1ull << 32) - 256)
            throw Error(PGX_ERR_UNSUPPORTED, "pgx_read_place_arrays: " + std::to_string(n_reads) + " reads with " + std::to_string(nv) + " values exceed one checking launch");
        k.w.bad.ensure(8);
        HIPCHECK(hipMemsetAsync(k.w.bad.p, 0xFF, 8, s));
        hipLaunchKernelGGL(pgx_read_hits_check_kernel, dim3(grid_for(n_reads, 256)), dim3(256), 0, s, (const uint64_t *)k.mem_off.as<uint64_t>(),
                           (const pgx_mem *)k.mems.as<pgx_mem>(), n_reads, m, k.w.bad.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
        uint64_t bad = read_u64(k.w.bad.as<uint64_t>(), s);
        if (bad != ~0ull) throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: the MEM starts of read " + std::to_string(bad) + " do not ascend strictly");
        if (nv) { // (a read's anchors: loc_offsets at its first MEM, what the plan kernel computes too)
            std::vector<uint64_t> h_aoff(n_reads + 1);
            for (uint64_t r = 0; r <= n_reads; r++) h_aoff[r] = loc_offsets[mem_offsets[r]];
            upload(k.w.aoff, h_aoff.data(), (n_reads + 1) * 8);
            hipLaunchKernelGGL(pgx_place_check_values_kernel, dim3(grid_for(nv, 256)), dim3(256), 0, s, (const uint64_t *)k.values.as<uint64_t>(), nv, max_length, n_seq,
                               (const uint64_t *)k.w.aoff.as<uint64_t>(), n_reads, k.w.bad.as<unsigned long long>());
            HIPCHECK(hipGetLastError());
            bad = read_u64(k.w.bad.as<uint64_t>(), s);
            if (bad != ~0ull)
                throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: read " + std::to_string(bad) + " has a value whose sequence is not below n_seq " + std::to_string(n_seq));
        }
    }
    place_core(k.w, k.mem_off.as<uint64_t>(), k.mems.as<pgx_mem>(), k.loc_off.as<uint64_t>(), k.values.as<uint64_t>(), n_reads, m, nv, n_seq, max_length, flags, mem_free, s,
               "pgx_read_place_arrays");
    if (list && k.w.n_places > places_cap)
        throw Error(PGX_ERR_NOMEM, "pgx_read_place_arrays: the list holds " + std::to_string(k.w.n_places) + " placements, places_cap is " + std::to_string(places_cap));
    download_result(k.w.result(), out, place_offsets, places, s);
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// read verify (pgx_verify_kernels.hip; the definitions: include/pgx.h "read verify")
static const uint32_t VERIFY_FLAGS = PGX_VERIFY_LIST;

static void verify_check_args(const std::string &who, uint32_t penalty, uint32_t flags) {
    if (flags & ~VERIFY_FLAGS) throw Error(PGX_ERR_ARG, who + ": unknown flag");
    if (penalty == 0 || penalty > PGX_VERIFY_MAX_PENALTY)
        throw Error(PGX_ERR_ARG, who + ": mismatch_penalty " + std::to_string(penalty) + " is outside 1 .. " + std::to_string(PGX_VERIFY_MAX_PENALTY));
}

// The stage on device arrays, enqueued on s: the candidates w.cand_off / cand_seq / cand_diag / cand_read (n_cands of them) -> w.cands, w.recs.
// reads: read_bytes bytes, read_off: n + 1 offsets into them.  Every buffer was sized by the caller's checks; nothing is read back.
static void verify_core(VerifyWork &w, const uint32_t *text4, const uint64_t *seq_start, uint32_t endmark, const uint8_t *reads, uint64_t read_bytes, const uint64_t *read_off,
                        uint64_t n, uint64_t n_cands, uint32_t penalty, hipStream_t s) {
    code_reads(w.rcode, reads, read_bytes, s);
    w.cands.ensure((n_cands ? n_cands : 1) * sizeof(pgx_read_verify));
    w.recs.ensure((n ? n : 1) * sizeof(pgx_read_verify));
    if (n_cands)
        hipLaunchKernelGGL(pgx_verify_kernel, dim3(grid_for(n_cands, PGX_VERIFY_THREADS)), dim3(PGX_VERIFY_THREADS), 0, s, text4, seq_start, endmark,
                           (const uint32_t *)w.rcode.as<uint32_t>(), read_off, (const uint64_t *)w.cand_off.as<uint64_t>(), (const uint64_t *)w.cand_read.as<uint64_t>(),
                           (const uint32_t *)w.cand_seq.as<uint32_t>(), (const int64_t *)w.cand_diag.as<int64_t>(), n_cands, penalty, w.cands.as<pgx_read_verify>());
    if (n)
        hipLaunchKernelGGL(pgx_verify_reduce_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const pgx_read_verify *)w.cands.as<pgx_read_verify>(),
                           (const uint64_t *)w.cand_off.as<uint64_t>(), n, w.recs.as<pgx_read_verify>());
    HIPCHECK(hipGetLastError());
}

extern "C" pgx_status pgx_batch_read_verify(pgx_batch *b, uint32_t max_cand, uint32_t mismatch_penalty, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_read_verify");
    checked_device_count();
    const std::string who = "pgx_batch_read_verify";
    if (!b) throw Error(PGX_ERR_ARG, who + ": null batch");
    // (what is refused here leaves an earlier verify result as it was)
    verify_check_args(who, mismatch_penalty, flags);
    if (max_cand < 1 || max_cand > PGX_VERIFY_MAX_CAND) throw Error(PGX_ERR_ARG, who + ": max_cand " + std::to_string(max_cand) + " is outside 1 .. " + std::to_string(PGX_VERIFY_MAX_CAND));
    if (!b->ran) throw Error(PGX_ERR_ARG, who + ": batch has not been run");
    PlaceWork &pw = b->pw;
    if (!pw.valid || pw.n_reads != b->n_reads) throw Error(PGX_ERR_ARG, who + ": needs a completed pgx_batch_read_place, the batch has no place result");
    if (max_cand > 1 && !(pw.flags & PGX_PLACE_LIST))
        throw Error(PGX_ERR_ARG, who + ": max_cand " + std::to_string(max_cand) + " needs a place result made with PGX_PLACE_LIST, the last pgx_batch_read_place ran without it");
    if (b->max_read_len >= (1ull << 31)) throw Error(PGX_ERR_UNSUPPORTED, who + ": a read of " + std::to_string(b->max_read_len) + " bytes; the records hold read positions below 2^31");
    const uint64_t n = b->n_reads;
    if (n >= PLACE_LAUNCH_ITEMS) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n) + " reads exceed one launch");
    use_device(b->device);
    pgx_device_image *d = device_image(b->h, b->device);
    ensure_text(b->h, d); // (throws where the index has no text image, before anything of the batch changes)
    hipStream_t s = batch_stream(b, stream);
    VerifyWork &w = b->vw;
    w.valid = false;
    b->qw.valid = false; // (the qualities belong to the list before)
    w.gen++;
    w.timer.begin(b->timed, s);
    // the candidates: counted, scanned, filled
    const bool from_list = max_cand > 1;
    const pgx_read_place *recs = pw.recs.as<pgx_read_place>();
    const uint64_t *place_off = from_list ? pw.place_off.as<uint64_t>() : nullptr;
    const pgx_placement *places = from_list ? pw.places.as<pgx_placement>() : nullptr;
    w.count.ensure((n ? n : 1) * 8);
    w.cand_off.ensure((n + 1) * 8);
    uint64_t n_cands = 0;
    if (n) {
        hipLaunchKernelGGL(pgx_verify_choose_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, recs, place_off, places, n, max_cand, w.count.as<uint64_t>(),
                           (const uint64_t *)nullptr, (uint32_t *)nullptr, (int64_t *)nullptr);
        HIPCHECK(hipGetLastError());
        scan_excl(1, w.count.p, n, 0, w.cand_off.as<uint64_t>(), w.scan_tmp, s);
        n_cands = read_u64(w.cand_off.as<uint64_t>() + n, s);
    } else HIPCHECK(hipMemsetAsync(w.cand_off.p, 0, 8, s));
    if (n_cands >= PLACE_LAUNCH_ITEMS) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_cands) + " candidates exceed one launch; lower max_cand");
    {
        const uint64_t need = n_cands * (sizeof(pgx_read_verify) + 20) + n * sizeof(pgx_read_verify) + b->read_bytes / 2;
        const size_t mem_free = free_device_memory();
        if (need > w.cands.cap + w.recs.cap + w.rcode.cap && need - (w.cands.cap + w.recs.cap + w.rcode.cap) > mem_free)
            throw Error(PGX_ERR_NOMEM, who + ": " + std::to_string(n_cands) + " candidates take " + std::to_string(need) + " bytes of device memory, " + std::to_string(mem_free) + " are free");
    }
    w.cand_seq.ensure((n_cands ? n_cands : 1) * 4);
    w.cand_diag.ensure((n_cands ? n_cands : 1) * 8);
    w.cand_read.ensure((n_cands ? n_cands : 1) * 8);
    if (n_cands) {
        hipLaunchKernelGGL(pgx_verify_choose_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, recs, place_off, places, n, max_cand, w.count.as<uint64_t>(),
                           (const uint64_t *)w.cand_off.as<uint64_t>(), w.cand_seq.as<uint32_t>(), w.cand_diag.as<int64_t>());
        hipLaunchKernelGGL(pgx_verify_owner_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const uint64_t *)w.cand_off.as<uint64_t>(), n, n_cands, w.cand_read.as<uint64_t>());
        HIPCHECK(hipGetLastError());
    }
    verify_core(w, d->text4.as<uint32_t>(), d->text_seq_start.as<uint64_t>(), 1u, b->reads.as<uint8_t>(), b->read_bytes, b->offsets.as<uint64_t>(), n, n_cands, mismatch_penalty, s);
    w.ms = w.timer.end(s);
    if (!b->timed) HIPCHECK(hipStreamSynchronize(s)); // (a timed call has waited in end(); verify_core, unlike align_core and walk_core, reads nothing back)
    w.n_reads = n; w.n_cands = n_cands; w.flags = flags; w.max_cand = max_cand; w.penalty = mismatch_penalty;
    w.max_list = max_cand; w.merged = false;
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void verified_header(const pgx_batch *b, pgx_read_verifies *out) {
    const VerifyWork &w = b->vw;
    std::memset(out, 0, sizeof *out);
    out->n_reads = w.n_reads;
    out->n_cands = w.n_cands;
    out->flags = w.flags;
    out->max_cand = w.max_cand;
    out->mismatch_penalty = w.penalty;
    out->ms_verify = w.ms;
}

extern "C" pgx_status pgx_batch_device_verified(pgx_batch *b, pgx_read_verifies *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->vw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_verified: batch has no verify result");
    const VerifyWork &w = b->vw;
    verified_header(b, out);
    out->reads = w.recs.as<pgx_read_verify>();
    if (w.flags & PGX_VERIFY_LIST) {
        out->cand_offsets = w.cand_off.as<uint64_t>();
        out->cands = w.cands.as<pgx_read_verify>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_verified(pgx_batch *b, pgx_read_verifies *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->vw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_verified: batch has no verify result");
    use_device(b->device);
    VerifyWork &w = b->vw;
    download_pinned(b, w.result(), w.h_recs, w.h_cand_off, w.h_cands);
    verified_header(b, out);
    out->reads = w.h_recs.as<pgx_read_verify>();
    if (w.flags & PGX_VERIFY_LIST) {
        out->cand_offsets = w.h_cand_off.as<uint64_t>();
        out->cands = w.h_cands.as<pgx_read_verify>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_read_verify_arrays(int device, const uint8_t *text, const uint64_t *seq_offsets, uint64_t n_seq, const uint8_t *reads,
                                             const uint64_t *read_offsets, uint64_t n_reads, const uint64_t *cand_offsets, const uint32_t *cand_seq,
                                             const int64_t *cand_diag, uint32_t mismatch_penalty, uint32_t flags, pgx_read_verify *out,
                                             uint64_t *list_offsets, pgx_read_verify *list, uint64_t list_cap) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_verify_arrays");
    checked_device_count();
    const std::string who = "pgx_read_verify_arrays";
    verify_check_args(who, mismatch_penalty, flags);
    const bool want_list = (flags & PGX_VERIFY_LIST) != 0;
    if (!seq_offsets || !read_offsets || !cand_offsets || (n_reads && !out) || (want_list && (!list_offsets || (list_cap && !list))))
        throw Error(PGX_ERR_ARG, who + ": null argument");
    check_offsets(who, seq_offsets, n_seq, "seq_offsets", "sequence");
    check_offsets(who, read_offsets, n_reads, "read_offsets", "read");
    check_offsets(who, cand_offsets, n_reads, "cand_offsets", "read");
    const uint64_t n_text = seq_offsets[n_seq], read_bytes = read_offsets[n_reads], n_cands = cand_offsets[n_reads];
    if ((n_text && !text) || (read_bytes && !reads) || (n_cands && (!cand_seq || !cand_diag))) throw Error(PGX_ERR_ARG, who + ": null argument");
    check_text(who, text, n_text);
    for (uint64_t r = 0; r < n_reads; r++)
        if (read_offsets[r + 1] - read_offsets[r] >= (1ull << 31))
            throw Error(PGX_ERR_UNSUPPORTED, who + ": read " + std::to_string(r) + " has " + std::to_string(read_offsets[r + 1] - read_offsets[r]) + " bytes; the records hold read positions below 2^31");
    if (n_reads >= PLACE_LAUNCH_ITEMS || n_cands >= PLACE_LAUNCH_ITEMS)
        throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_reads) + " reads with " + std::to_string(n_cands) + " candidates exceed one launch");
    if (want_list && n_cands > list_cap)
        throw Error(PGX_ERR_NOMEM, who + ": the list holds " + std::to_string(n_cands) + " candidates, list_cap is " + std::to_string(list_cap));
    use_device(device);
    struct VerifyInput : TextInput { // device copies of the input + the stage's buffers, released on every way out
        VerifyWork w;
        ~VerifyInput() { w.release(); }
    } k;
    hipStream_t s = nullptr;
    k.upload(text, seq_offsets, n_seq, reads, read_offsets, n_reads);
    upload(k.w.cand_off, cand_offsets, (n_reads + 1) * 8);
    upload(k.w.cand_seq, cand_seq, n_cands * 4);
    upload(k.w.cand_diag, cand_diag, n_cands * 8);
    k.w.cand_read.ensure((n_cands ? n_cands : 1) * 8);
    if (n_cands) { // the preconditions, before anything is written
        hipLaunchKernelGGL(pgx_verify_owner_kernel, dim3(grid_for(n_reads, 256)), dim3(256), 0, s, (const uint64_t *)k.w.cand_off.as<uint64_t>(), n_reads, n_cands,
                           k.w.cand_read.as<uint64_t>());
        k.w.bad.ensure(8);
        HIPCHECK(hipMemsetAsync(k.w.bad.p, 0xFF, 8, s));
        hipLaunchKernelGGL(pgx_verify_check_kernel, dim3(grid_for(n_cands, 256)), dim3(256), 0, s, (const uint64_t *)k.w.cand_read.as<uint64_t>(),
                           (const uint32_t *)k.w.cand_seq.as<uint32_t>(), n_cands, n_seq, k.w.bad.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
        const uint64_t bad = read_u64(k.w.bad.as<uint64_t>(), s);
        if (bad != ~0ull) throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(bad) + " has a candidate whose sequence is not below n_seq " + std::to_string(n_seq));
    }
    k.pack(s);
    HIPCHECK(hipGetLastError());
    verify_core(k.w, k.text4.as<uint32_t>(), k.seq_off.as<uint64_t>(), 0u, k.reads.as<uint8_t>(), read_bytes, k.read_off.as<uint64_t>(), n_reads, n_cands, mismatch_penalty, s);
    k.w.n_reads = n_reads; k.w.n_cands = n_cands; k.w.flags = flags;
    download_result(k.w.result(), out, list_offsets, list, s);
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// read mates (pgx_mates_kernels.hip; the definitions: include/pgx.h "read mates")
static const uint32_t MATES_FLAGS = PGX_MATES_ELECT;

static void mates_check_args(const std::string &who, int64_t frag_min, int64_t frag_max, uint32_t flags) {
    if (flags & ~MATES_FLAGS) throw Error(PGX_ERR_ARG, who + ": unknown flag");
    if (frag_min > frag_max) throw Error(PGX_ERR_ARG, who + ": frag_min " + std::to_string(frag_min) + " exceeds frag_max " + std::to_string(frag_max));
}

// the first p with L[2p] != L[2p + 1] (n_seq / 2 for an odd n_seq), ~0 when the collection is twinned; start: n_seq + 1 offsets
// (with an endmarker behind every sequence or with none: both sides of a comparison carry it)
static uint64_t first_untwinned(const uint64_t *start, uint64_t n_seq) {
    for (uint64_t p = 0; 2 * p + 1 < n_seq; p++)
        if (start[2 * p + 1] - start[2 * p] != start[2 * p + 2] - start[2 * p + 1]) return p;
    return (n_seq & 1) ? n_seq / 2 : ~0ull;
}

bool index_twinned(pgx_device_image *d, uint64_t *first_bad) {
    if (!d->twin_state) {
        std::vector<uint64_t> start(d->text_n_seq + 1);
        HIPCHECK(hipMemcpy(start.data(), d->text_seq_start.p, start.size() * 8, hipMemcpyDeviceToHost));
        d->twin_bad = first_untwinned(start.data(), d->text_n_seq);
        d->twin_state = d->twin_bad == ~0ull ? 1 : 2;
    }
    if (first_bad) *first_bad = d->twin_bad;
    return d->twin_state == 1;
}

extern "C" pgx_status pgx_index_twinned(pgx_index *h, int device, uint64_t *first_bad) {
    PGX_GUARD_BEGIN
    checked_device_count();
    if (!h || !first_bad) throw Error(PGX_ERR_ARG, "pgx_index_twinned: null argument");
    use_device(device);
    pgx_device_image *d = device_image(h, device);
    ensure_text(h, d);
    (void)index_twinned(d, first_bad);
    return PGX_OK;
    PGX_GUARD_END
}

// log2 of the lanes a pair takes: the power of two >= max_cand, and >= PGX_MATES_LANES (tests; 1 .. 64, read per call).  Results never depend on it.
// Refuses the pairs one launch cannot hold.
static uint32_t mates_lane_shift(uint64_t n_pairs, uint64_t max_cand, const std::string &who) {
    uint64_t want = std::max<uint64_t>(max_cand, 1);
    if (const char *e = std::getenv("PGX_MATES_LANES")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= 64) want = std::max<uint64_t>(want, (uint64_t)v);
    }
    uint32_t sh = 0;
    while ((1ull << sh) < want) sh++;
    if (n_pairs >= (PLACE_LAUNCH_ITEMS >> sh)) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_pairs) + " pairs at " + std::to_string(1u << sh) + " lanes a pair exceed one launch");
    return sh;
}

// The stage on device arrays, enqueued on s, the four counters read back behind it (synchronises s): w.recs, w.counters; winners: with PGX_MATES_ELECT.
// No list is longer than max_cand <= 64.  Refuses a launch that is too large (the batch entry point has asked before it clears its result).
static void mates_core(MatesWork &w, const uint64_t *seq_start, uint32_t endmark, const uint64_t *cand_off, const pgx_read_verify *cands, uint64_t n_pairs, uint64_t max_cand,
                       int64_t frag_min, int64_t frag_max, uint32_t penalty, uint32_t flags, pgx_read_verify *winners, hipStream_t s, const std::string &who) {
    const uint32_t g_shift = mates_lane_shift(n_pairs, max_cand, who);
    w.recs.ensure((n_pairs ? n_pairs : 1) * sizeof(pgx_read_mates));
    w.ctr.ensure(32);
    HIPCHECK(hipMemsetAsync(w.ctr.p, 0, 32, s));
    if (n_pairs) {
        hipLaunchKernelGGL(pgx_mates_kernel, dim3(grid_for(n_pairs, PGX_MATES_THREADS >> g_shift)), dim3(PGX_MATES_THREADS), 0, s, seq_start, endmark, cand_off, cands, n_pairs,
                           g_shift, frag_min, frag_max, penalty, flags, w.recs.as<pgx_read_mates>(), winners, w.ctr.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
    }
    w.n_pairs = n_pairs; w.flags = flags; w.penalty = penalty; w.frag_min = frag_min; w.frag_max = frag_max;
}

extern "C" pgx_status pgx_batch_read_mates(pgx_batch *b, int64_t frag_min, int64_t frag_max, uint32_t penalty, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_read_mates");
    checked_device_count();
    const std::string who = "pgx_batch_read_mates";
    if (!b) throw Error(PGX_ERR_ARG, who + ": null batch");
    // (what is refused here leaves an earlier mates result and the verify result as they were)
    mates_check_args(who, frag_min, frag_max, flags);
    if (!b->ran) throw Error(PGX_ERR_ARG, who + ": batch has not been run");
    VerifyWork &vw = b->vw;
    if (!vw.valid || vw.n_reads != b->n_reads) throw Error(PGX_ERR_ARG, who + ": needs a completed pgx_batch_read_verify(PGX_VERIFY_LIST), the batch has no verify result");
    if (!(vw.flags & PGX_VERIFY_LIST))
        throw Error(PGX_ERR_ARG, who + ": needs a verify result made with PGX_VERIFY_LIST, the last pgx_batch_read_verify ran with flags " + std::to_string(vw.flags));
    const uint64_t n = b->n_reads;
    if (n & 1) throw Error(PGX_ERR_ARG, who + ": " + std::to_string(n) + " reads, an odd number: reads 2k and 2k + 1 are the mates of pair k");
    use_device(b->device);
    pgx_device_image *d = device_image(b->h, b->device);
    ensure_text(b->h, d); // (built by the verify call)
    uint64_t bad = 0;
    if (!index_twinned(d, &bad))
        throw Error(PGX_ERR_UNSUPPORTED, who + ": the index is not twinned, " +
                                             ((d->text_n_seq & 1) && bad == d->text_n_seq / 2 ? "it has an odd number of sequences (" + std::to_string(d->text_n_seq) + ")"
                                                                                                : "sequences " + std::to_string(2 * bad) + " and " + std::to_string(2 * bad + 1) +
                                                                                                      " (p = " + std::to_string(bad) + ") differ in length") +
                                             ": mates need a collection with every path forward and reversed (gbz_extract -b)");
    (void)mates_lane_shift(n / 2, vw.max_list, who); // (the last refusal: what is refused leaves an earlier mates result as it was)
    hipStream_t s = batch_stream(b, stream);
    MatesWork &w = b->mw;
    w.valid = false;
    b->qw.valid = false; // (the qualities were made before this call, and an election moves the winners)
    w.verify_gen = vw.gen;
    w.timer.begin(b->timed, s);
    mates_core(w, d->text_seq_start.as<uint64_t>(), 1u, vw.cand_off.as<uint64_t>(), vw.cands.as<pgx_read_verify>(), n / 2, vw.max_list, frag_min, frag_max, penalty, flags,
               (flags & PGX_MATES_ELECT) ? vw.recs.as<pgx_read_verify>() : nullptr, s, who);
    w.ms = w.timer.end(s);
    read_scalars(w.counters, w.ctr.p, 32, s); // (waits for the kernel: the call is complete on return)
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void mated_header(const pgx_batch *b, pgx_read_mates_result *out) {
    const MatesWork &w = b->mw;
    std::memset(out, 0, sizeof *out);
    out->n_pairs = w.n_pairs;
    out->n_proper = w.counters[0]; out->n_compatible = w.counters[1]; out->n_moved_a = w.counters[2]; out->n_moved_b = w.counters[3];
    out->frag_min = w.frag_min; out->frag_max = w.frag_max;
    out->flags = w.flags;
    out->penalty = w.penalty;
    out->ms_mates = w.ms;
}

extern "C" pgx_status pgx_batch_device_mated(pgx_batch *b, pgx_read_mates_result *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->mw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_mated: batch has no mates result");
    mated_header(b, out);
    out->pairs = b->mw.recs.as<pgx_read_mates>();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_mated(pgx_batch *b, pgx_read_mates_result *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->mw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_mated: batch has no mates result");
    use_device(b->device);
    MatesWork &w = b->mw;
    w.h_recs.ensure((w.n_pairs ? w.n_pairs : 1) * sizeof(pgx_read_mates));
    if (w.n_pairs) HIPCHECK(hipMemcpyAsync(w.h_recs.p, w.recs.p, w.n_pairs * sizeof(pgx_read_mates), hipMemcpyDeviceToHost, b->own));
    HIPCHECK(hipStreamSynchronize(b->own)); // (the kernel completed inside pgx_batch_read_mates, on whatever stream it used)
    mated_header(b, out);
    out->pairs = w.h_recs.as<pgx_read_mates>();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_read_mates_arrays(int device, const uint64_t *seq_lengths, uint64_t n_seq, uint64_t n_reads, const uint64_t *cand_offsets, const pgx_read_verify *cands,
                                            int64_t frag_min, int64_t frag_max, uint32_t penalty, uint32_t flags, pgx_read_mates *out, pgx_read_verify *winners) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_mates_arrays");
    checked_device_count();
    const std::string who = "pgx_read_mates_arrays";
    mates_check_args(who, frag_min, frag_max, flags);
    const bool elect = (flags & PGX_MATES_ELECT) != 0;
    if ((n_seq && !seq_lengths) || !cand_offsets || (n_reads && (!out || (elect && !winners)))) throw Error(PGX_ERR_ARG, who + ": null argument");
    if (n_seq & 1) throw Error(PGX_ERR_ARG, who + ": n_seq " + std::to_string(n_seq) + " is odd: sequences 2p and 2p + 1 are twins");
    if (n_seq >= (1ull << 32) - 1) throw Error(PGX_ERR_ARG, who + ": n_seq " + std::to_string(n_seq) + " does not fit a record's seq");
    std::vector<uint64_t> start(n_seq + 1, 0);
    for (uint64_t q = 0; q < n_seq; q++) start[q + 1] = start[q] + seq_lengths[q];
    if (const uint64_t bad = first_untwinned(start.data(), n_seq); bad != ~0ull)
        throw Error(PGX_ERR_ARG, who + ": sequences " + std::to_string(2 * bad) + " and " + std::to_string(2 * bad + 1) + " (p = " + std::to_string(bad) + ") have the lengths " +
                                     std::to_string(seq_lengths[2 * bad]) + " and " + std::to_string(seq_lengths[2 * bad + 1]) + ": twins have one length");
    check_offsets(who, cand_offsets, n_reads, "cand_offsets", "read");
    uint64_t max_cand = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t c = cand_offsets[r + 1] - cand_offsets[r];
        if (c > PGX_VERIFY_MAX_CAND) throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(r) + " has " + std::to_string(c) + " candidates, more than " + std::to_string(PGX_VERIFY_MAX_CAND));
        max_cand = std::max(max_cand, c);
    }
    const uint64_t n_cands = cand_offsets[n_reads];
    if (n_cands && !cands) throw Error(PGX_ERR_ARG, who + ": null argument");
    for (uint64_t r = 0; r < n_reads; r++)
        for (uint64_t c = cand_offsets[r]; c < cand_offsets[r + 1]; c++)
            if (cands[c].seq >= n_seq)
                throw Error(PGX_ERR_ARG, who + ": candidate " + std::to_string(c - cand_offsets[r]) + " of read " + std::to_string(r) + " has seq " + std::to_string(cands[c].seq) +
                                             ", not below n_seq " + std::to_string(n_seq));
    if (n_reads & 1) throw Error(PGX_ERR_ARG, who + ": n_reads " + std::to_string(n_reads) + " is odd: reads 2k and 2k + 1 are the mates of pair k");
    use_device(device);
    struct MatesInput { // device copies of the input + the stage's buffers, released on every way out
        DevBuf seq_start, cand_off, cands, winners;
        MatesWork w;
        ~MatesInput() { release_all({&seq_start, &cand_off, &cands, &winners}); w.release(); }
    } k;
    hipStream_t s = nullptr;
    upload(k.seq_start, start.data(), (n_seq + 1) * 8);
    upload(k.cand_off, cand_offsets, (n_reads + 1) * 8);
    upload(k.cands, cands, n_cands * sizeof(pgx_read_verify));
    if (elect) k.winners.ensure((n_reads ? n_reads : 1) * sizeof(pgx_read_verify));
    mates_core(k.w, k.seq_start.as<uint64_t>(), 0u, k.cand_off.as<uint64_t>(), k.cands.as<pgx_read_verify>(), n_reads / 2, max_cand, frag_min, frag_max, penalty, flags,
               elect ? k.winners.as<pgx_read_verify>() : nullptr, s, who);
    if (n_reads) {
        HIPCHECK(hipMemcpyAsync(out, k.w.recs.p, (n_reads / 2) * sizeof(pgx_read_mates), hipMemcpyDeviceToHost, s));
        if (elect) HIPCHECK(hipMemcpyAsync(winners, k.winners.p, n_reads * sizeof(pgx_read_verify), hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// read rescue (pgx_rescue_kernels.hip; the definitions: include/pgx.h "read rescue")
static const uint32_t RESCUE_FLAGS = PGX_RESCUE_MERGE;
static const uint64_t RESCUE_LAUNCH_TASKS = (1ull << 26) - 4; // a wave a task: fewer than 2^32 threads a launch

static void rescue_check_args(const std::string &who, int64_t frag_min, int64_t frag_max, uint32_t min_score, uint32_t max_anchors, uint32_t flags) {
    if (flags & ~RESCUE_FLAGS) throw Error(PGX_ERR_ARG, who + ": unknown flag");
    if (frag_min > frag_max) throw Error(PGX_ERR_ARG, who + ": frag_min " + std::to_string(frag_min) + " exceeds frag_max " + std::to_string(frag_max));
    if ((uint64_t)frag_max - (uint64_t)frag_min >= (uint64_t)PGX_RESCUE_MAX_WINDOW)
        throw Error(PGX_ERR_ARG, who + ": frag_min " + std::to_string(frag_min) + " .. frag_max " + std::to_string(frag_max) + " is a window of more than " +
                                     std::to_string(PGX_RESCUE_MAX_WINDOW) + " diagonals");
    if (min_score == 0) throw Error(PGX_ERR_ARG, who + ": min_score 0: a rescued placement needs a match");
    if (max_anchors < 1 || max_anchors > PGX_RESCUE_MAX_ANCHORS)
        throw Error(PGX_ERR_ARG, who + ": max_anchors " + std::to_string(max_anchors) + " is outside 1 .. " + std::to_string(PGX_RESCUE_MAX_ANCHORS));
}

// what the stage reads, on the device: the text with its sequences, the coded reads, verify's list (no list longer than max_list <= 64)
struct RescueInput {
    const uint32_t *text4;
    const uint64_t *seq_start;
    uint32_t endmark;
    const uint32_t *rcode;
    const uint64_t *read_off, *cand_off;
    const pgx_read_verify *cands;
    uint64_t n_reads, n_cands, max_list;
};

// The stage on device arrays, enqueued on s: w.recs and w.counters.  Two scalars are read back (each synchronises s): the number of tasks, which sizes the
// scan's launch and its buffers, and the counters.  Refuses the tasks one launch cannot hold, before anything of a result is written; *cleared is set
// behind that refusal (the batch entry point drops its earlier result there).
static void rescue_core(RescueWork &w, const RescueInput &in, int64_t frag_min, int64_t frag_max, uint32_t penalty, uint32_t min_score, uint32_t max_anchors, bool merge,
                        hipStream_t s, const std::string &who, bool *cleared) {
    const uint64_t n = in.n_reads;
    w.recs.ensure((n ? n : 1) * sizeof(pgx_read_rescue));
    w.ctr.ensure(40);
    HIPCHECK(hipMemsetAsync(w.ctr.p, 0, 40, s));
    uint64_t n_tasks = 0;
    if (n) {
        // compatible pairs and solo winners: the mates kernel itself, without an election, into records of the stage's own
        mates_core(w.mates, in.seq_start, in.endmark, in.cand_off, in.cands, n / 2, in.max_list, frag_min, frag_max, 0u, 0u, nullptr, s, who);
        // frag bounds beyond any L - diag - d (|diag| < 2^62, |d| < 2^32) select what +-(2^62 + 2^34) select, and those cannot overflow in the kernel
        const int64_t lim = (1ll << 62) + (1ll << 34);
        const int64_t fmin = std::min(std::max(frag_min, -lim), lim), fmax = std::min(std::max(frag_max, -lim), lim);
        const pgx_read_mates *mrecs = w.mates.recs.as<pgx_read_mates>();
        w.task_count.ensure(n * 8);
        w.task_off.ensure((n + 1) * 8);
        hipLaunchKernelGGL(pgx_rescue_targets_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, in.seq_start, in.endmark, in.read_off, in.cand_off, in.cands, mrecs, n, fmin, fmax,
                           max_anchors, w.task_count.as<uint64_t>(), (const uint64_t *)nullptr, (PgxRescueTask *)nullptr);
        HIPCHECK(hipGetLastError());
        scan_excl(1, w.task_count.p, n, 0, w.task_off.as<uint64_t>(), w.scan_tmp, s);
        n_tasks = read_u64(w.task_off.as<uint64_t>() + n, s);
        if (n_tasks >= RESCUE_LAUNCH_TASKS)
            throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_tasks) + " tasks at a wave a task exceed one launch: rescue the reads in smaller batches or lower max_anchors");
        if (cleared) *cleared = true;
        w.tasks.ensure((n_tasks ? n_tasks : 1) * sizeof(PgxRescueTask));
        w.best.ensure((n_tasks ? n_tasks : 1) * sizeof(PgxRescueBest));
        if (merge) w.rescued.ensure(n * 8);
        if (n_tasks) {
            hipLaunchKernelGGL(pgx_rescue_targets_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, in.seq_start, in.endmark, in.read_off, in.cand_off, in.cands, mrecs, n, fmin,
                               fmax, max_anchors, w.task_count.as<uint64_t>(), (const uint64_t *)w.task_off.as<uint64_t>(), w.tasks.as<PgxRescueTask>());
            hipLaunchKernelGGL(pgx_rescue_scan_kernel, dim3(grid_for(n_tasks, PGX_RESCUE_THREADS / 64)), dim3(PGX_RESCUE_THREADS), 0, s, in.text4, in.seq_start, in.endmark,
                               in.rcode, in.read_off, (const PgxRescueTask *)w.tasks.as<PgxRescueTask>(), n_tasks, penalty, w.best.as<PgxRescueBest>());
        }
        hipLaunchKernelGGL(pgx_rescue_reduce_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, in.cand_off, mrecs, (const uint64_t *)w.task_count.as<uint64_t>(),
                           (const uint64_t *)w.task_off.as<uint64_t>(), (const PgxRescueTask *)w.tasks.as<PgxRescueTask>(), (const PgxRescueBest *)w.best.as<PgxRescueBest>(), n,
                           min_score, w.recs.as<pgx_read_rescue>(), merge ? w.rescued.as<uint64_t>() : nullptr, w.ctr.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
    } else if (cleared) *cleared = true;
    read_scalars(w.counters, w.ctr.p, 40, s);
    w.n_reads = n; w.frag_min = frag_min; w.frag_max = frag_max; w.min_score = min_score; w.max_anchors = max_anchors; w.penalty = penalty;
    w.flags = merge ? PGX_RESCUE_MERGE : 0u;
}

// MERGE on device arrays, enqueued on s behind rescue_core: w.new_off (n + 1) and w.new_cands (n_cands + rescued records), and the winners of every read by
// the reduce kernel of verify.  old_read: the read of every candidate of the list.  Nothing is read back: the host knows the rescued count.
static void rescue_merge_core(RescueWork &w, const RescueInput &in, const uint64_t *old_read, uint32_t penalty, pgx_read_verify *winners, hipStream_t s) {
    const uint64_t n = in.n_reads, n_res = w.counters[1], n_new = in.n_cands + n_res;
    w.new_off.ensure((n + 1) * 8);
    w.new_cands.ensure((n_new ? n_new : 1) * sizeof(pgx_read_verify));
    if (!n) { HIPCHECK(hipMemsetAsync(w.new_off.p, 0, 8, s)); return; }
    w.res_off.ensure((n + 1) * 8);
    w.new_count.ensure(n * 8);
    w.fake_off.ensure(n * 8);
    w.cand_read.ensure((n_res ? n_res : 1) * 8);
    w.cand_seq.ensure((n_res ? n_res : 1) * 4);
    w.cand_diag.ensure((n_res ? n_res : 1) * 8);
    w.res_cands.ensure((n_res ? n_res : 1) * sizeof(pgx_read_verify));
    scan_excl(1, w.rescued.p, n, 0, w.res_off.as<uint64_t>(), w.scan_tmp, s);
    hipLaunchKernelGGL(pgx_rescue_cands_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const pgx_read_rescue *)w.recs.as<pgx_read_rescue>(), in.cand_off,
                       (const uint64_t *)w.rescued.as<uint64_t>(), (const uint64_t *)w.res_off.as<uint64_t>(), n, w.cand_read.as<uint64_t>(), w.cand_seq.as<uint32_t>(),
                       w.cand_diag.as<int64_t>(), w.fake_off.as<uint64_t>(), w.new_count.as<uint64_t>());
    if (n_res) // the appended records: verify's own kernel at the rescued (seq, diag)
        hipLaunchKernelGGL(pgx_verify_kernel, dim3(grid_for(n_res, PGX_VERIFY_THREADS)), dim3(PGX_VERIFY_THREADS), 0, s, in.text4, in.seq_start, in.endmark, in.rcode, in.read_off,
                           (const uint64_t *)w.fake_off.as<uint64_t>(), (const uint64_t *)w.cand_read.as<uint64_t>(), (const uint32_t *)w.cand_seq.as<uint32_t>(),
                           (const int64_t *)w.cand_diag.as<int64_t>(), n_res, penalty, w.res_cands.as<pgx_read_verify>());
    HIPCHECK(hipGetLastError());
    scan_excl(1, w.new_count.p, n, 0, w.new_off.as<uint64_t>(), w.scan_tmp, s);
    if (n_new)
        hipLaunchKernelGGL(pgx_rescue_copy_kernel, dim3(grid_for(n_new, 256)), dim3(256), 0, s, in.cands, in.cand_off, old_read, in.n_cands,
                           (const pgx_read_verify *)w.res_cands.as<pgx_read_verify>(), (const uint64_t *)w.cand_read.as<uint64_t>(), n_res,
                           (const uint64_t *)w.new_off.as<uint64_t>(), w.new_cands.as<pgx_read_verify>());
    hipLaunchKernelGGL(pgx_verify_reduce_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const pgx_read_verify *)w.new_cands.as<pgx_read_verify>(),
                       (const uint64_t *)w.new_off.as<uint64_t>(), n, winners);
    HIPCHECK(hipGetLastError());
}

extern "C" pgx_status pgx_batch_read_rescue(pgx_batch *b, int64_t frag_min, int64_t frag_max, uint32_t min_score, uint32_t max_anchors, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_read_rescue");
    checked_device_count();
    const std::string who = "pgx_batch_read_rescue";
    if (!b) throw Error(PGX_ERR_ARG, who + ": null batch");
    // (what is refused here leaves an earlier rescue result, the mates result and the verify result as they were)
    rescue_check_args(who, frag_min, frag_max, min_score, max_anchors, flags);
    if (!b->ran) throw Error(PGX_ERR_ARG, who + ": batch has not been run");
    VerifyWork &vw = b->vw;
    if (!vw.valid || vw.n_reads != b->n_reads) throw Error(PGX_ERR_ARG, who + ": needs a completed pgx_batch_read_verify(PGX_VERIFY_LIST), the batch has no verify result");
    if (!(vw.flags & PGX_VERIFY_LIST))
        throw Error(PGX_ERR_ARG, who + ": needs a verify result made with PGX_VERIFY_LIST, the last pgx_batch_read_verify ran with flags " + std::to_string(vw.flags));
    if (vw.merged) throw Error(PGX_ERR_ARG, who + ": the verify result was already merged by an earlier call: a verify result takes one PGX_RESCUE_MERGE");
    const uint64_t n = b->n_reads;
    if (n & 1) throw Error(PGX_ERR_ARG, who + ": " + std::to_string(n) + " reads, an odd number: reads 2k and 2k + 1 are the mates of pair k");
    use_device(b->device);
    pgx_device_image *d = device_image(b->h, b->device);
    ensure_text(b->h, d); // (built by the verify call)
    uint64_t bad = 0;
    if (!index_twinned(d, &bad))
        throw Error(PGX_ERR_UNSUPPORTED, who + ": the index is not twinned, " +
                                             ((d->text_n_seq & 1) && bad == d->text_n_seq / 2 ? "it has an odd number of sequences (" + std::to_string(d->text_n_seq) + ")"
                                                                                                : "sequences " + std::to_string(2 * bad) + " and " + std::to_string(2 * bad + 1) +
                                                                                                      " (p = " + std::to_string(bad) + ") differ in length") +
                                             ": rescue needs a collection with every path forward and reversed (gbz_extract -b)");
    (void)mates_lane_shift(n / 2, vw.max_list, who);
    hipStream_t s = batch_stream(b, stream);
    RescueWork &w = b->rw;
    const bool merge = (flags & PGX_RESCUE_MERGE) != 0, was_valid = w.valid;
    w.timer.begin(b->timed, s);
    const RescueInput in{d->text4.as<uint32_t>(), d->text_seq_start.as<uint64_t>(), 1u, vw.rcode.as<uint32_t>(), b->offsets.as<uint64_t>(), vw.cand_off.as<uint64_t>(),
                         vw.cands.as<pgx_read_verify>(), n, vw.n_cands, vw.max_list};
    bool cleared = false;
    w.valid = false;
    const bool mapq_was_valid = b->qw.valid;
    b->qw.valid = false; // (the qualities were made before this call)
    try {
        rescue_core(w, in, frag_min, frag_max, vw.penalty, min_score, max_anchors, merge, s, who, &cleared);
    } catch (...) {
        if (!cleared) { w.valid = was_valid; b->qw.valid = mapq_was_valid; } // (the last refusal: the records of the result before were not touched)
        throw;
    }
    if (merge) {
        rescue_merge_core(w, in, vw.cand_read.as<uint64_t>(), vw.penalty, vw.recs.as<pgx_read_verify>(), s);
        std::swap(vw.cands, w.new_cands);
        std::swap(vw.cand_off, w.new_off);
        vw.n_cands += w.counters[1];
        vw.merged = true;
        vw.gen++;
        if (w.counters[1]) vw.max_list = std::min<uint32_t>(vw.max_cand + 1, PGX_VERIFY_MAX_CAND);
        b->mw.valid = false; // (paired from the list before)
    }
    w.ms = w.timer.end(s);
    if (!b->timed) HIPCHECK(hipStreamSynchronize(s));
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void rescued_header(const pgx_batch *b, pgx_read_rescue_result *out) {
    const RescueWork &w = b->rw;
    std::memset(out, 0, sizeof *out);
    out->n_reads = w.n_reads;
    out->n_targets = w.counters[0]; out->n_rescued = w.counters[1]; out->n_full = w.counters[2]; out->n_tasks = w.counters[3]; out->n_diags = w.counters[4];
    out->frag_min = w.frag_min; out->frag_max = w.frag_max;
    out->min_score = w.min_score; out->max_anchors = w.max_anchors; out->flags = w.flags; out->mismatch_penalty = w.penalty;
    out->ms_rescue = w.ms;
}

extern "C" pgx_status pgx_batch_device_rescued(pgx_batch *b, pgx_read_rescue_result *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->rw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_rescued: batch has no rescue result");
    rescued_header(b, out);
    out->reads = b->rw.recs.as<pgx_read_rescue>();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_rescued(pgx_batch *b, pgx_read_rescue_result *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->rw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_rescued: batch has no rescue result");
    use_device(b->device);
    RescueWork &w = b->rw;
    w.h_recs.ensure((w.n_reads ? w.n_reads : 1) * sizeof(pgx_read_rescue));
    if (w.n_reads) HIPCHECK(hipMemcpyAsync(w.h_recs.p, w.recs.p, w.n_reads * sizeof(pgx_read_rescue), hipMemcpyDeviceToHost, b->own));
    HIPCHECK(hipStreamSynchronize(b->own)); // (the kernels completed inside pgx_batch_read_rescue, on whatever stream it used)
    rescued_header(b, out);
    out->reads = w.h_recs.as<pgx_read_rescue>();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_read_rescue_arrays(int device, const uint8_t *text, const uint64_t *seq_offsets, uint64_t n_seq, const uint8_t *reads, const uint64_t *read_offsets,
                                             uint64_t n_reads, const uint64_t *cand_offsets, const pgx_read_verify *cands, int64_t frag_min, int64_t frag_max,
                                             uint32_t mismatch_penalty, uint32_t min_score, uint32_t max_anchors, uint32_t flags, pgx_read_rescue *out,
                                             uint64_t *list_offsets, pgx_read_verify *list, uint64_t list_cap, pgx_read_verify *winners) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_rescue_arrays");
    checked_device_count();
    const std::string who = "pgx_read_rescue_arrays";
    rescue_check_args(who, frag_min, frag_max, min_score, max_anchors, flags);
    verify_check_args(who, mismatch_penalty, 0u);
    const bool merge = (flags & PGX_RESCUE_MERGE) != 0;
    if (!seq_offsets || !read_offsets || !cand_offsets || (n_reads && !out) || (merge && (!list_offsets || (list_cap && !list) || (n_reads && !winners))))
        throw Error(PGX_ERR_ARG, who + ": null argument");
    // what pgx_read_verify_arrays refuses
    check_offsets(who, seq_offsets, n_seq, "seq_offsets", "sequence");
    check_offsets(who, read_offsets, n_reads, "read_offsets", "read");
    check_offsets(who, cand_offsets, n_reads, "cand_offsets", "read");
    const uint64_t n_text = seq_offsets[n_seq], read_bytes = read_offsets[n_reads], n_cands = cand_offsets[n_reads];
    if ((n_text && !text) || (read_bytes && !reads) || (n_cands && !cands)) throw Error(PGX_ERR_ARG, who + ": null argument");
    check_text(who, text, n_text);
    for (uint64_t r = 0; r < n_reads; r++)
        if (read_offsets[r + 1] - read_offsets[r] >= (1ull << 31))
            throw Error(PGX_ERR_UNSUPPORTED, who + ": read " + std::to_string(r) + " has " + std::to_string(read_offsets[r + 1] - read_offsets[r]) + " bytes; the records hold read positions below 2^31");
    if (n_reads >= PLACE_LAUNCH_ITEMS || n_cands >= PLACE_LAUNCH_ITEMS)
        throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_reads) + " reads with " + std::to_string(n_cands) + " candidates exceed one launch");
    // what pgx_read_mates_arrays refuses
    if (n_seq & 1) throw Error(PGX_ERR_ARG, who + ": n_seq " + std::to_string(n_seq) + " is odd: sequences 2p and 2p + 1 are twins");
    if (n_seq >= (1ull << 32) - 1) throw Error(PGX_ERR_ARG, who + ": n_seq " + std::to_string(n_seq) + " does not fit a record's seq");
    if (const uint64_t bad = first_untwinned(seq_offsets, n_seq); bad != ~0ull)
        throw Error(PGX_ERR_ARG, who + ": sequences " + std::to_string(2 * bad) + " and " + std::to_string(2 * bad + 1) + " (p = " + std::to_string(bad) + ") have the lengths " +
                                     std::to_string(seq_offsets[2 * bad + 1] - seq_offsets[2 * bad]) + " and " + std::to_string(seq_offsets[2 * bad + 2] - seq_offsets[2 * bad + 1]) +
                                     ": twins have one length");
    uint64_t max_cand = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t c = cand_offsets[r + 1] - cand_offsets[r];
        if (c > PGX_VERIFY_MAX_CAND) throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(r) + " has " + std::to_string(c) + " candidates, more than " + std::to_string(PGX_VERIFY_MAX_CAND));
        max_cand = std::max(max_cand, c);
    }
    for (uint64_t r = 0; r < n_reads; r++)
        for (uint64_t c = cand_offsets[r]; c < cand_offsets[r + 1]; c++)
            if (cands[c].seq >= n_seq)
                throw Error(PGX_ERR_ARG, who + ": candidate " + std::to_string(c - cand_offsets[r]) + " of read " + std::to_string(r) + " has seq " + std::to_string(cands[c].seq) +
                                             ", not below n_seq " + std::to_string(n_seq));
    if (n_reads & 1) throw Error(PGX_ERR_ARG, who + ": n_reads " + std::to_string(n_reads) + " is odd: reads 2k and 2k + 1 are the mates of pair k");
    use_device(device);
    struct RescueArrays : TextInput { // device copies of the input + the stage's buffers, released on every way out
        DevBuf cand_off, cands, rcode, old_read, winners;
        RescueWork w;
        ~RescueArrays() { release_all({&cand_off, &cands, &rcode, &old_read, &winners}); w.release(); }
    } k;
    hipStream_t s = nullptr;
    (void)mates_lane_shift(n_reads / 2, max_cand, who);
    k.upload(text, seq_offsets, n_seq, reads, read_offsets, n_reads);
    upload(k.cand_off, cand_offsets, (n_reads + 1) * 8);
    upload(k.cands, cands, n_cands * sizeof(pgx_read_verify));
    k.pack(s);
    code_reads(k.rcode, k.reads.as<uint8_t>(), read_bytes, s);
    HIPCHECK(hipGetLastError());
    const RescueInput in{k.text4.as<uint32_t>(), k.seq_off.as<uint64_t>(), 0u, k.rcode.as<uint32_t>(), k.read_off.as<uint64_t>(), k.cand_off.as<uint64_t>(),
                         k.cands.as<pgx_read_verify>(), n_reads, n_cands, max_cand};
    rescue_core(k.w, in, frag_min, frag_max, mismatch_penalty, min_score, max_anchors, merge, s, who, nullptr);
    const uint64_t n_new = n_cands + k.w.counters[1];
    if (merge && n_new > list_cap)
        throw Error(PGX_ERR_NOMEM, who + ": the merged list holds " + std::to_string(n_new) + " candidates, list_cap is " + std::to_string(list_cap));
    if (merge) {
        k.old_read.ensure((n_cands ? n_cands : 1) * 8);
        k.winners.ensure((n_reads ? n_reads : 1) * sizeof(pgx_read_verify));
        if (n_cands)
            hipLaunchKernelGGL(pgx_verify_owner_kernel, dim3(grid_for(n_reads, 256)), dim3(256), 0, s, (const uint64_t *)k.cand_off.as<uint64_t>(), n_reads, n_cands,
                               k.old_read.as<uint64_t>());
        rescue_merge_core(k.w, in, k.old_read.as<uint64_t>(), mismatch_penalty, k.winners.as<pgx_read_verify>(), s);
        HIPCHECK(hipMemcpyAsync(list_offsets, k.w.new_off.p, (n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
        if (n_new) HIPCHECK(hipMemcpyAsync(list, k.w.new_cands.p, n_new * sizeof(pgx_read_verify), hipMemcpyDeviceToHost, s));
        if (n_reads) HIPCHECK(hipMemcpyAsync(winners, k.winners.p, n_reads * sizeof(pgx_read_verify), hipMemcpyDeviceToHost, s));
    }
    if (n_reads) HIPCHECK(hipMemcpyAsync(out, k.w.recs.p, n_reads * sizeof(pgx_read_rescue), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// read align (pgx_align_kernels.hip; the definitions: include/pgx.h "read align")
static const uint32_t ALIGN_FLAGS = PGX_ALIGN_CIGAR;
static const uint64_t ALIGN_MAX_READ = 1ull << 28; // an operation's length has 28 bits

static void align_check_args(const std::string &who, uint32_t band, uint32_t flags) {
    if (flags & ~ALIGN_FLAGS) throw Error(PGX_ERR_ARG, who + ": unknown flag");
    if (band > PGX_ALIGN_MAX_BAND) throw Error(PGX_ERR_ARG, who + ": band " + std::to_string(band) + " is outside 0 .. " + std::to_string(PGX_ALIGN_MAX_BAND));
}

// bytes of direction planes one pass may hold: PGX_ALIGN_BUDGET_MB (read per call, fractions allowed), default a quarter of the free device memory
static uint64_t align_budget_bytes(size_t mem_free) {
    uint64_t bytes = 0;
    if (const char *e = std::getenv("PGX_ALIGN_BUDGET_MB")) {
        const double mb = std::strtod(e, nullptr);
        if (mb > 0) bytes = (uint64_t)(mb * 1048576.0);
    }
    if (!bytes) bytes = mem_free / 4;
    return std::max<uint64_t>(bytes, 16);
}

// log2 of the lanes a row of the band takes (the power of two >= 2 * band + 1), and the bytes of its direction planes
static uint32_t align_lg(uint32_t band) {
    uint32_t lg = 0;
    while ((1u << lg) < 2 * band + 1) lg++;
    return lg;
}
static uint32_t align_row_bytes(uint32_t band) { return std::max(1u << align_lg(band), 8u) / 4; }

struct AlignPass { uint64_t r0, r1, bytes; };

// The passes over consecutive whole reads whose planes fit the budget, from the host's read offsets: a read of len bytes takes len rows of
// row_bytes, rounded up to 16 (pgx_align_need_kernel computes the same on the device).  Throws before anything is launched.
static std::vector<AlignPass> align_plan(const uint64_t *h_read_off, uint64_t n, uint32_t row_bytes, uint64_t budget, const std::string &who) {
    std::vector<AlignPass> passes;
    AlignPass cur{0, 0, 0};
    for (uint64_t r = 0; r < n; r++) {
        const uint64_t len = h_read_off[r + 1] - h_read_off[r];
        if (len >= ALIGN_MAX_READ) throw Error(PGX_ERR_UNSUPPORTED, who + ": read " + std::to_string(r) + " has " + std::to_string(len) + " bytes; an operation's length is below 2^28");
        const uint64_t need = (len * row_bytes + 15) & ~15ull;
        if (need > budget)
            throw Error(PGX_ERR_NOMEM, who + ": read " + std::to_string(r) + " needs " + std::to_string(need) + " bytes of direction planes, a pass holds " + std::to_string(budget) +
                                           " (PGX_ALIGN_BUDGET_MB)");
        if (cur.bytes + need > budget) { passes.push_back(cur); cur = AlignPass{r, r, 0}; }
        cur.bytes += need;
        cur.r1 = r + 1;
    }
    if (cur.r1 > cur.r0) passes.push_back(cur);
    return passes;
}

template <int LG>
static void align_launch_forward(const uint32_t *text4, const uint64_t *seq_start, uint32_t endmark, const uint32_t *rcode, const uint64_t *read_off, const AlignWork &w,
                                 const AlignPass &p, uint32_t band, hipStream_t s) {
    hipLaunchKernelGGL(pgx_align_forward_kernel<LG>, dim3(grid_for(p.r1 - p.r0, PGX_ALIGN_THREADS >> LG)), dim3(PGX_ALIGN_THREADS), 0, s, text4, seq_start, endmark, rcode, read_off,
                       (const uint32_t *)w.cand_seq.as<uint32_t>(), (const int64_t *)w.cand_diag.as<int64_t>(), p.r0, p.r1, band, (const uint64_t *)w.plane_off.as<uint64_t>(),
                       w.planes.as<uint8_t>(), w.fwd.as<uint2>());
}

// The stage on device arrays, enqueued on s (synchronised where the number of operations is read back): w.cand_seq / w.cand_diag (n of each) -> w.recs,
// w.op_off and, with PGX_ALIGN_CIGAR, w.ops.  rcode: the reads coded by pgx_verify_code_kernel.  The plan was made by the caller: nothing here refuses.
// With one pass the planes stay in place between the counting walk and the writing walk; with more, the forward kernel runs again before the writing walk.
static void align_core(AlignWork &w, const uint32_t *text4, const uint64_t *seq_start, uint32_t endmark, const uint32_t *rcode, const uint64_t *read_off, uint64_t n,
                       const std::vector<AlignPass> &plan, uint32_t band, uint32_t flags, bool timed, hipStream_t s) {
    const uint32_t lg = align_lg(band), row_bytes = align_row_bytes(band);
    uint64_t scratch = 16;
    for (const AlignPass &p : plan) scratch = std::max(scratch, p.bytes);
    w.recs.ensure((n ? n : 1) * sizeof(pgx_read_align));
    w.need.ensure((n ? n : 1) * 8); w.plane_off.ensure((n + 1) * 8); w.fwd.ensure((n ? n : 1) * sizeof(uint2));
    w.count.ensure((n ? n : 1) * 8); w.op_off.ensure((n + 1) * 8);
    w.planes.ensure(scratch);
    size_t n_ev = 0;
    auto stamp = [&]() { // the next event of the call, recorded on s
        if (!timed) return;
        if (w.ev.size() <= n_ev) w.ev.resize(n_ev + 1, nullptr);
        if (!w.ev[n_ev]) HIPCHECK(hipEventCreate(&w.ev[n_ev]));
        HIPCHECK(hipEventRecord(w.ev[n_ev++], s));
    };
    std::vector<int> kinds; // of every pair of events: 0 forward, 1 trace
    auto forward = [&](const AlignPass &p) {
        stamp();
        switch (lg) {
        case 0: align_launch_forward<0>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        case 1: align_launch_forward<1>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        case 2: align_launch_forward<2>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        case 3: align_launch_forward<3>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        case 4: align_launch_forward<4>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        case 5: align_launch_forward<5>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        default: align_launch_forward<6>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        }
        stamp();
        kinds.push_back(0);
    };
    auto trace = [&](const AlignPass &p, uint32_t write) {
        stamp();
        hipLaunchKernelGGL(pgx_align_trace_kernel, dim3(grid_for(p.r1 - p.r0, 256)), dim3(256), 0, s, seq_start, endmark, read_off, (const uint32_t *)w.cand_seq.as<uint32_t>(),
                           (const int64_t *)w.cand_diag.as<int64_t>(), p.r0, p.r1, band, row_bytes, (const uint64_t *)w.plane_off.as<uint64_t>(),
                           (const uint8_t *)w.planes.as<uint8_t>(), (const uint2 *)w.fwd.as<uint2>(), write, w.recs.as<pgx_read_align>(), w.count.as<uint64_t>(),
                           (const uint64_t *)w.op_off.as<uint64_t>(), w.ops.as<uint32_t>());
        stamp();
        kinds.push_back(1);
    };
    uint64_t n_ops = 0;
    if (n) {
        hipLaunchKernelGGL(pgx_align_need_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, read_off, n, row_bytes, w.need.as<uint64_t>());
        HIPCHECK(hipGetLastError());
        scan_excl(1, w.need.p, n, 0, w.plane_off.as<uint64_t>(), w.scan_tmp, s);
        for (const AlignPass &p : plan) { forward(p); trace(p, 0); }
        HIPCHECK(hipGetLastError());
        scan_excl(1, w.count.p, n, 0, w.op_off.as<uint64_t>(), w.scan_tmp, s);
        n_ops = read_u64(w.op_off.as<uint64_t>() + n, s);
    } else HIPCHECK(hipMemsetAsync(w.op_off.p, 0, 8, s));
    if ((flags & PGX_ALIGN_CIGAR) && n_ops) {
        w.ops.ensure(n_ops * 4);
        for (const AlignPass &p : plan) {
            if (plan.size() > 1) forward(p);
            trace(p, 1);
        }
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipStreamSynchronize(s));
    w.ms_forward = w.ms_trace = 0;
    for (size_t i = 0; timed && i < kinds.size(); i++) {
        float ms = 0;
        HIPCHECK(hipEventElapsedTime(&ms, w.ev[2 * i], w.ev[2 * i + 1]));
        (kinds[i] ? w.ms_trace : w.ms_forward) += ms;
    }
    w.n_reads = n; w.n_ops = n_ops; w.flags = flags; w.band = band; w.passes = (uint32_t)plan.size(); w.scratch_bytes = plan.empty() ? 0 : scratch;
}

extern "C" pgx_status pgx_batch_read_align(pgx_batch *b, uint32_t band, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_read_align");
    checked_device_count();
    const std::string who = "pgx_batch_read_align";
    if (!b) throw Error(PGX_ERR_ARG, who + ": null batch");
    // (what is refused here leaves an earlier align result as it was)
    align_check_args(who, band, flags);
    if (!b->ran) throw Error(PGX_ERR_ARG, who + ": batch has not been run");
    VerifyWork &vw = b->vw;
    if (!vw.valid || vw.n_reads != b->n_reads) throw Error(PGX_ERR_ARG, who + ": needs a completed pgx_batch_read_verify, the batch has no verify result");
    const uint64_t n = b->n_reads;
    if (n >= PLACE_LAUNCH_ITEMS) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n) + " reads exceed one launch");
    use_device(b->device);
    pgx_device_image *d = device_image(b->h, b->device);
    ensure_text(b->h, d); // (built by the verify stage)
    const std::vector<AlignPass> plan = align_plan(b->h_offsets(), n, align_row_bytes(band), align_budget_bytes(free_device_memory()), who);
    hipStream_t s = batch_stream(b, stream);
    AlignWork &w = b->aw;
    w.valid = false;
    w.timer.begin(b->timed, s);
    w.cand_seq.ensure((n ? n : 1) * 4); w.cand_diag.ensure((n ? n : 1) * 8);
    if (n) {
        hipLaunchKernelGGL(pgx_align_cand_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const pgx_read_verify *)vw.recs.as<pgx_read_verify>(), n, w.cand_seq.as<uint32_t>(),
                           w.cand_diag.as<int64_t>());
        HIPCHECK(hipGetLastError());
    }
    // (the reads were coded by the verify call for all of its candidates: vw.rcode describes this run's reads)
    align_core(w, d->text4.as<uint32_t>(), d->text_seq_start.as<uint64_t>(), 1u, (const uint32_t *)vw.rcode.as<uint32_t>(), b->offsets.as<uint64_t>(), n, plan, band, flags, b->timed, s);
    w.ms = w.timer.end(s); // (an untimed call has waited in align_core)
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void aligned_header(const pgx_batch *b, pgx_read_aligns *out) {
    const AlignWork &w = b->aw;
    std::memset(out, 0, sizeof *out);
    out->n_reads = w.n_reads;
    out->n_ops = w.n_ops;
    out->flags = w.flags;
    out->band = w.band;
    out->passes = w.passes;
    out->scratch_bytes = w.scratch_bytes;
    out->ms_align = w.ms;
    out->ms_forward = w.ms_forward;
    out->ms_trace = w.ms_trace;
}

extern "C" pgx_status pgx_batch_device_aligned(pgx_batch *b, pgx_read_aligns *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->aw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_aligned: batch has no align result");
    const AlignWork &w = b->aw;
    aligned_header(b, out);
    out->reads = w.recs.as<pgx_read_align>();
    if (w.flags & PGX_ALIGN_CIGAR) {
        out->op_offsets = w.op_off.as<uint64_t>();
        out->ops = w.ops.as<uint32_t>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_aligned(pgx_batch *b, pgx_read_aligns *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->aw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_aligned: batch has no align result");
    use_device(b->device);
    AlignWork &w = b->aw;
    download_pinned(b, w.result(), w.h_recs, w.h_op_off, w.h_ops);
    aligned_header(b, out);
    out->reads = w.h_recs.as<pgx_read_align>();
    if (w.flags & PGX_ALIGN_CIGAR) {
        out->op_offsets = w.h_op_off.as<uint64_t>();
        out->ops = w.h_ops.as<uint32_t>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_read_align_arrays(int device, const uint8_t *text, const uint64_t *seq_offsets, uint64_t n_seq, const uint8_t *reads,
                                            const uint64_t *read_offsets, uint64_t n_reads, const uint32_t *cand_seq, const int64_t *cand_diag, uint32_t band,
                                            uint32_t flags, pgx_read_align *out, uint64_t *op_offsets, uint32_t *ops, uint64_t ops_cap) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_align_arrays");
    checked_device_count();
    const std::string who = "pgx_read_align_arrays";
    align_check_args(who, band, flags);
    const bool want_ops = (flags & PGX_ALIGN_CIGAR) != 0;
    if (!seq_offsets || !read_offsets || (n_reads && (!out || !cand_seq || !cand_diag)) || (want_ops && (!op_offsets || (ops_cap && !ops))))
        throw Error(PGX_ERR_ARG, who + ": null argument");
    check_offsets(who, seq_offsets, n_seq, "seq_offsets", "sequence");
    check_offsets(who, read_offsets, n_reads, "read_offsets", "read");
    const uint64_t n_text = seq_offsets[n_seq], read_bytes = read_offsets[n_reads];
    if ((n_text && !text) || (read_bytes && !reads)) throw Error(PGX_ERR_ARG, who + ": null argument");
    check_text(who, text, n_text);
    for (uint64_t r = 0; r < n_reads; r++)
        if (cand_seq[r] != PGX_NO_SEQUENCE && cand_seq[r] >= n_seq)
            throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(r) + " has a candidate whose sequence is not below n_seq " + std::to_string(n_seq));
    if (n_reads >= PLACE_LAUNCH_ITEMS) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_reads) + " reads exceed one launch");
    use_device(device);
    const std::vector<AlignPass> plan = align_plan(read_offsets, n_reads, align_row_bytes(band), align_budget_bytes(free_device_memory()), who);
    struct AlignInput : TextInput { // device copies of the input + the stage's buffers, released on every way out
        AlignWork w;
        ~AlignInput() { w.release(); }
    } k;
    hipStream_t s = nullptr;
    k.upload(text, seq_offsets, n_seq, reads, read_offsets, n_reads);
    upload(k.w.cand_seq, cand_seq, n_reads * 4);
    upload(k.w.cand_diag, cand_diag, n_reads * 8);
    k.pack(s);
    code_reads(k.w.rcode, k.reads.as<uint8_t>(), read_bytes, s);
    HIPCHECK(hipGetLastError());
    align_core(k.w, k.text4.as<uint32_t>(), k.seq_off.as<uint64_t>(), 0u, (const uint32_t *)k.w.rcode.as<uint32_t>(), k.read_off.as<uint64_t>(), n_reads, plan, band, flags, false, s);
    if (want_ops && k.w.n_ops > ops_cap)
        throw Error(PGX_ERR_NOMEM, who + ": the list holds " + std::to_string(k.w.n_ops) + " operations, ops_cap is " + std::to_string(ops_cap));
    download_result(k.w.result(), out, op_offsets, ops, s);
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// read walk (pgx_walk_kernels.hip; the definitions: include/pgx.h "read walk")
static const uint32_t WALK_FLAGS = PGX_WALK_STEPS;

// The stage on device arrays, enqueued on s (synchronised where the number of steps is read back): the align records, or seq / text_start / text_end
// (n of each), -> w.recs, w.step_off and, with PGX_WALK_STEPS, w.steps.  Nothing here refuses.
static void walk_core(WalkWork &w, const PgxWalkImage &img, const uint64_t *seq_start, uint32_t endmark, uint64_t n_seq, const pgx_read_align *recs, const uint32_t *seq,
                      const uint64_t *text_start, const uint64_t *text_end, uint64_t n, uint32_t flags, hipStream_t s) {
    w.recs.ensure((n ? n : 1) * sizeof(pgx_read_walk));
    w.count.ensure((n ? n : 1) * 8); w.first.ensure((n ? n : 1) * 8); w.step_off.ensure((n + 1) * 8);
    uint64_t n_steps = 0;
    if (n) {
        hipLaunchKernelGGL(pgx_walk_count_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, img, seq_start, endmark, n_seq, recs, seq, text_start, text_end, n,
                           w.recs.as<pgx_read_walk>(), w.count.as<uint64_t>(), w.first.as<uint64_t>());
        HIPCHECK(hipGetLastError());
        scan_excl(1, w.count.p, n, 0, w.step_off.as<uint64_t>(), w.scan_tmp, s);
        n_steps = read_u64(w.step_off.as<uint64_t>() + n, s); // (the stage's one read-back)
    } else HIPCHECK(hipMemsetAsync(w.step_off.p, 0, 8, s));
    if ((flags & PGX_WALK_STEPS) && n_steps) {
        w.steps.ensure(n_steps * 8);
        hipLaunchKernelGGL(pgx_walk_fill_kernel, dim3(grid_for(n, 256 / PGX_WALK_FILL_LANES)), dim3(256), 0, s, img, (const uint64_t *)w.count.as<uint64_t>(),
                           (const uint64_t *)w.first.as<uint64_t>(), (const uint64_t *)w.step_off.as<uint64_t>(), n, w.steps.as<uint64_t>());
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipStreamSynchronize(s));
    w.n_reads = n; w.n_steps = n_steps; w.flags = flags;
}

extern "C" pgx_status pgx_batch_read_walk(pgx_batch *b, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_read_walk");
    checked_device_count();
    const std::string who = "pgx_batch_read_walk";
    if (!b) throw Error(PGX_ERR_ARG, who + ": null batch");
    // (what is refused here leaves an earlier walk result as it was)
    if (flags & ~WALK_FLAGS) throw Error(PGX_ERR_ARG, who + ": unknown flag");
    if (!b->ran) throw Error(PGX_ERR_ARG, who + ": batch has not been run");
    AlignWork &aw = b->aw;
    if (!aw.valid || aw.n_reads != b->n_reads) throw Error(PGX_ERR_ARG, who + ": needs a completed pgx_batch_read_align, the batch has no align result");
    const uint64_t n = b->n_reads;
    if (n >= PLACE_LAUNCH_ITEMS / PGX_WALK_FILL_LANES) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n) + " reads exceed one launch");
    use_device(b->device);
    pgx_device_image *d = device_image(b->h, b->device);
    ensure_walk(b->h, d); // (throws before anything of the batch changes)
    hipStream_t s = batch_stream(b, stream);
    WalkWork &w = b->ww;
    w.valid = false;
    w.timer.begin(b->timed, s);
    walk_core(w, d->walk, d->text_seq_start.as<uint64_t>(), 1u, d->text_n_seq, (const pgx_read_align *)aw.recs.as<pgx_read_align>(), nullptr, nullptr, nullptr, n, flags, s);
    w.ms = w.timer.end(s); // (an untimed call has waited in walk_core)
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void walked_header(const pgx_batch *b, pgx_read_walks *out) {
    const WalkWork &w = b->ww;
    std::memset(out, 0, sizeof *out);
    out->n_reads = w.n_reads;
    out->n_steps = w.n_steps;
    out->flags = w.flags;
    out->ms_walk = w.ms;
}

extern "C" pgx_status pgx_batch_device_walked(pgx_batch *b, pgx_read_walks *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->ww.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_walked: batch has no walk result");
    const WalkWork &w = b->ww;
    walked_header(b, out);
    out->reads = w.recs.as<pgx_read_walk>();
    if (w.flags & PGX_WALK_STEPS) {
        out->step_offsets = w.step_off.as<uint64_t>();
        out->steps = w.steps.as<uint64_t>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_walked(pgx_batch *b, pgx_read_walks *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->ww.valid) throw Error(PGX_ERR_ARG, "pgx_batch_walked: batch has no walk result");
    use_device(b->device);
    WalkWork &w = b->ww;
    download_pinned(b, w.result(), w.h_recs, w.h_step_off, w.h_steps);
    walked_header(b, out);
    out->reads = w.h_recs.as<pgx_read_walk>();
    if (w.flags & PGX_WALK_STEPS) {
        out->step_offsets = w.h_step_off.as<uint64_t>();
        out->steps = w.h_steps.as<uint64_t>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

// What the _arrays entry points that take path tables (walk, mapq) ask of them, and the text position of every visit: sequence q is seq_offsets[q] ..
// seq_offsets[q + 1] and consists of the visits [visit_offsets[q], visit_offsets[q + 1]).
std::vector<uint64_t> walk_table_marks(const std::string &who, const uint64_t *seq_offsets, uint64_t n_seq, const uint64_t *visit_offsets, const uint64_t *visit_nodes,
                                              const uint32_t *visit_length) {
    check_offsets(who, seq_offsets, n_seq, "seq_offsets", "sequence");
    check_offsets(who, visit_offsets, n_seq, "visit_offsets", "sequence");
    const uint64_t n_text = seq_offsets[n_seq], V = visit_offsets[n_seq];
    if (V && (!visit_nodes || !visit_length)) throw Error(PGX_ERR_ARG, who + ": null argument");
    check_text(who, nullptr, n_text); // (the walk reads no text: the size alone)
    std::vector<uint64_t> marks(V);
    for (uint64_t q = 0; q < n_seq; q++) {
        uint64_t p = seq_offsets[q];
        for (uint64_t k = visit_offsets[q]; k < visit_offsets[q + 1]; k++) {
            if (visit_length[k] == 0 || visit_length[k] > PGX_WALK_MAX_VISIT)
                throw Error(PGX_ERR_ARG, who + ": visit " + std::to_string(k) + " of sequence " + std::to_string(q) + " has length " + std::to_string(visit_length[k]) + ", outside 1 .. 1024");
            marks[k] = p;
            p += visit_length[k];
        }
        if (p != seq_offsets[q + 1])
            throw Error(PGX_ERR_ARG, who + ": the visits of sequence " + std::to_string(q) + " sum to " + std::to_string(p - seq_offsets[q]) + " symbols, the sequence has " +
                                         std::to_string(seq_offsets[q + 1] - seq_offsets[q]));
    }
    return marks;
}

// (the WALK image of stated path tables, WalkTables: pgx_batch_internal.hpp)

extern "C" pgx_status pgx_read_walk_arrays(int device, const uint64_t *seq_offsets, uint64_t n_seq, const uint64_t *visit_offsets, const uint64_t *visit_nodes,
                                           const uint32_t *visit_length, uint64_t n_reads, const uint32_t *seq, const uint64_t *text_start, const uint64_t *text_end,
                                           uint32_t flags, pgx_read_walk *out, uint64_t *step_offsets, uint64_t *steps, uint64_t steps_cap) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_walk_arrays");
    checked_device_count();
    const std::string who = "pgx_read_walk_arrays";
    if (flags & ~WALK_FLAGS) throw Error(PGX_ERR_ARG, who + ": unknown flag");
    const bool want_steps = (flags & PGX_WALK_STEPS) != 0;
    if (!seq_offsets || !visit_offsets || (n_reads && (!out || !seq || !text_start || !text_end)) || (want_steps && (!step_offsets || (steps_cap && !steps))))
        throw Error(PGX_ERR_ARG, who + ": null argument");
    const std::vector<uint64_t> marks = walk_table_marks(who, seq_offsets, n_seq, visit_offsets, visit_nodes, visit_length);
    for (uint64_t r = 0; r < n_reads; r++) {
        if (seq[r] == PGX_NO_SEQUENCE) continue;
        if (seq[r] >= n_seq) throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(r) + " names a sequence that is not below n_seq " + std::to_string(n_seq));
        const uint64_t ls = seq_offsets[(uint64_t)seq[r] + 1] - seq_offsets[seq[r]];
        if (text_start[r] > text_end[r] || text_end[r] > ls)
            throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(r) + " has the stretch [" + std::to_string(text_start[r]) + ", " + std::to_string(text_end[r]) +
                                         "), its sequence has " + std::to_string(ls) + " symbols");
    }
    if (n_reads >= PLACE_LAUNCH_ITEMS / PGX_WALK_FILL_LANES) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_reads) + " reads exceed one launch");
    use_device(device);
    struct WalkInput : WalkTables { // device copies of the input, the image + the stage's buffers, released on every way out
        DevBuf seq, ts, te;
        WalkWork w;
        ~WalkInput() { release_all({&seq, &ts, &te}); w.release(); }
    } k;
    hipStream_t s = nullptr;
    upload(k.seq, seq, n_reads * 4);
    upload(k.ts, text_start, n_reads * 8);
    upload(k.te, text_end, n_reads * 8);
    const PgxWalkImage img = k.build(seq_offsets, n_seq, marks, visit_nodes, s);
    walk_core(k.w, img, k.seq_off.as<uint64_t>(), 0u, n_seq, nullptr, (const uint32_t *)k.seq.as<uint32_t>(), (const uint64_t *)k.ts.as<uint64_t>(),
              (const uint64_t *)k.te.as<uint64_t>(), n_reads, flags, s);
    if (want_steps && k.w.n_steps > steps_cap)
        throw Error(PGX_ERR_NOMEM, who + ": the list holds " + std::to_string(k.w.n_steps) + " steps, steps_cap is " + std::to_string(steps_cap));
    download_result(k.w.result(), out, step_offsets, steps, s);
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// read mapq (pgx_mapq_kernels.hip; the definitions: include/pgx.h "read mapq")
static const uint32_t MAPQ_FLAGS = PGX_MAPQ_PAIRED;

static void mapq_check_args(const std::string &who, uint32_t scale, uint32_t slack, uint32_t max_extra, uint32_t flags) {
    if (flags & ~MAPQ_FLAGS) throw Error(PGX_ERR_ARG, who + ": unknown flag");
    if (scale < 1 || scale > PGX_MAPQ_MAX_SCALE) throw Error(PGX_ERR_ARG, who + ": scale " + std::to_string(scale) + " is outside 1 .. " + std::to_string(PGX_MAPQ_MAX_SCALE));
    if (slack > PGX_MAPQ_MAX_SLACK) throw Error(PGX_ERR_ARG, who + ": slack " + std::to_string(slack) + " exceeds " + std::to_string(PGX_MAPQ_MAX_SLACK));
    if (max_extra > PGX_MAPQ_MAX_EXTRA) throw Error(PGX_ERR_ARG, who + ": max_extra " + std::to_string(max_extra) + " exceeds " + std::to_string(PGX_MAPQ_MAX_EXTRA));
}

// log2 of the lanes a read (a pair under PAIRED) takes: the power of two >= max_entries, and >= PGX_MAPQ_LANES (tests; 1 .. 64, read per call).  Results never
// depend on it.  Refuses the reads one launch cannot hold.
static uint32_t mapq_lane_shift(uint64_t n_units, uint64_t max_entries, const std::string &who) {
    uint64_t want = std::max<uint64_t>(max_entries, 1);
    if (const char *e = std::getenv("PGX_MAPQ_LANES")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= 64) want = std::max<uint64_t>(want, (uint64_t)v);
    }
    uint32_t sh = 0;
    while ((1ull << sh) < want) sh++;
    if (n_units >= (PLACE_LAUNCH_ITEMS >> sh)) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_units) + " reads at " + std::to_string(1u << sh) + " lanes a read exceed one launch");
    return sh;
}

// The hot kernel on device arrays, enqueued on s: `a` says where the entries lie (out, counters and g_shift are put in here) -> w.recs, w.ctr.  No read has
// more than max_entries <= 64 entries.  Nothing is read back.
static void mapq_core(MapqWork &w, PgxMapqArgs a, uint64_t max_entries, bool paired, hipStream_t s, const std::string &who) {
    const uint64_t n = a.n_reads, n_units = paired ? n / 2 : n;
    a.g_shift = mapq_lane_shift(n_units, max_entries, who);
    w.recs.ensure((n ? n : 1) * sizeof(pgx_read_mapq));
    w.ctr.ensure(32);
    HIPCHECK(hipMemsetAsync(w.ctr.p, 0, 32, s));
    a.out = w.recs.as<pgx_read_mapq>();
    a.counters = w.ctr.as<unsigned long long>();
    if (n_units) {
        const dim3 grid(grid_for(n_units, PGX_MAPQ_THREADS >> a.g_shift)), block(PGX_MAPQ_THREADS);
        if (paired) hipLaunchKernelGGL(pgx_mapq_kernel<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(pgx_mapq_kernel<false>, grid, block, 0, s, a);
        HIPCHECK(hipGetLastError());
    }
    w.n_reads = n;
}

extern "C" pgx_status pgx_batch_read_mapq(pgx_batch *b, uint32_t scale, uint32_t slack, uint32_t max_extra, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_read_mapq");
    checked_device_count();
    const std::string who = "pgx_batch_read_mapq";
    if (!b) throw Error(PGX_ERR_ARG, who + ": null batch");
    // (the verify, rescue, mates and place results are only read.  What is refused leaves an earlier mapq result as it was: every refusal but one comes
    // before anything of the stage is touched, and the last one -- too many extras for one launch -- comes behind the count pass, which has then written
    // the stage's scratch (count, more, extra_off) and started the timer, and nothing of the result: its records, counters and header stay valid)
    mapq_check_args(who, scale, slack, max_extra, flags);
    const bool paired = (flags & PGX_MAPQ_PAIRED) != 0;
    if (!b->ran) throw Error(PGX_ERR_ARG, who + ": batch has not been run");
    VerifyWork &vw = b->vw;
    if (!vw.valid || vw.n_reads != b->n_reads) throw Error(PGX_ERR_ARG, who + ": needs a completed pgx_batch_read_verify(PGX_VERIFY_LIST), the batch has no verify result");
    if (!(vw.flags & PGX_VERIFY_LIST))
        throw Error(PGX_ERR_ARG, who + ": needs a verify result made with PGX_VERIFY_LIST, the last pgx_batch_read_verify ran with flags " + std::to_string(vw.flags));
    PlaceWork &pw = b->pw;
    if (max_extra > 0) {
        if (!pw.valid || pw.n_reads != b->n_reads) throw Error(PGX_ERR_ARG, who + ": max_extra " + std::to_string(max_extra) + " needs a completed pgx_batch_read_place(PGX_PLACE_LIST), the batch has no place result");
        if (!(pw.flags & PGX_PLACE_LIST))
            throw Error(PGX_ERR_ARG, who + ": max_extra " + std::to_string(max_extra) + " needs a place result made with PGX_PLACE_LIST, the last pgx_batch_read_place ran without it");
    }
    const uint64_t n = b->n_reads;
    const MatesWork &mw = b->mw;
    if (paired) {
        if (!mw.valid || mw.n_pairs != n / 2) throw Error(PGX_ERR_ARG, who + ": PGX_MAPQ_PAIRED needs a completed pgx_batch_read_mates, the batch has no mates result");
        if (mw.verify_gen != vw.gen) throw Error(PGX_ERR_ARG, who + ": PGX_MAPQ_PAIRED needs a mates result made on the current verify result, the batch's was made on an earlier one");
        if (n & 1) throw Error(PGX_ERR_ARG, who + ": " + std::to_string(n) + " reads, an odd number: reads 2k and 2k + 1 are the mates of pair k");
    }
    const uint64_t max_entries = std::min<uint64_t>((uint64_t)vw.max_list + max_extra, PGX_MAPQ_MAX_ENTRIES);
    (void)mapq_lane_shift(paired ? n / 2 : n, max_entries, who);
    use_device(b->device);
    pgx_device_image *d = device_image(b->h, b->device);
    ensure_walk(b->h, d); // (throws before anything of the batch changes)
    hipStream_t s = batch_stream(b, stream);
    MapqWork &w = b->qw;
    w.timer.begin(b->timed, s);
    // the extras: counted, scanned, filled, verified by verify's own kernel on a list of their own
    uint64_t n_extras = 0;
    if (max_extra > 0 && n) {
        w.count.ensure(n * 8); w.more.ensure(n * 4); w.extra_off.ensure((n + 1) * 8);
        hipLaunchKernelGGL(pgx_mapq_choose_extras_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const pgx_read_place *)pw.recs.as<pgx_read_place>(),
                           (const uint64_t *)pw.place_off.as<uint64_t>(), (const pgx_placement *)pw.places.as<pgx_placement>(), (const uint64_t *)vw.cand_off.as<uint64_t>(), n, max_extra,
                           w.count.as<uint64_t>(), w.more.as<uint32_t>(), (const uint64_t *)nullptr, (uint32_t *)nullptr, (int64_t *)nullptr);
        HIPCHECK(hipGetLastError());
        scan_excl(1, w.count.p, n, 0, w.extra_off.as<uint64_t>(), w.scan_tmp, s);
        n_extras = read_u64(w.extra_off.as<uint64_t>() + n, s);
        if (n_extras >= PLACE_LAUNCH_ITEMS) // (the last refusal, mid-pipeline: see above)
            throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_extras) + " extras exceed one launch; lower max_extra");
    }
    w.valid = false; // (behind the last refusal)
    if (n_extras) {
        w.cand_seq.ensure(n_extras * 4); w.cand_diag.ensure(n_extras * 8); w.cand_read.ensure(n_extras * 8); w.extras.ensure(n_extras * sizeof(pgx_read_verify));
        hipLaunchKernelGGL(pgx_mapq_choose_extras_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const pgx_read_place *)pw.recs.as<pgx_read_place>(),
                           (const uint64_t *)pw.place_off.as<uint64_t>(), (const pgx_placement *)pw.places.as<pgx_placement>(), (const uint64_t *)vw.cand_off.as<uint64_t>(), n, max_extra,
                           w.count.as<uint64_t>(), w.more.as<uint32_t>(), (const uint64_t *)w.extra_off.as<uint64_t>(), w.cand_seq.as<uint32_t>(), w.cand_diag.as<int64_t>());
        hipLaunchKernelGGL(pgx_verify_owner_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const uint64_t *)w.extra_off.as<uint64_t>(), n, n_extras, w.cand_read.as<uint64_t>());
        hipLaunchKernelGGL(pgx_verify_kernel, dim3(grid_for(n_extras, PGX_VERIFY_THREADS)), dim3(PGX_VERIFY_THREADS), 0, s, (const uint32_t *)d->text4.as<uint32_t>(),
                           (const uint64_t *)d->text_seq_start.as<uint64_t>(), 1u, (const uint32_t *)vw.rcode.as<uint32_t>(), (const uint64_t *)b->offsets.as<uint64_t>(),
                           (const uint64_t *)w.extra_off.as<uint64_t>(), (const uint64_t *)w.cand_read.as<uint64_t>(), (const uint32_t *)w.cand_seq.as<uint32_t>(),
                           (const int64_t *)w.cand_diag.as<int64_t>(), n_extras, vw.penalty, w.extras.as<pgx_read_verify>());
        HIPCHECK(hipGetLastError());
    }
    PgxMapqArgs a{};
    a.walk = d->walk;
    a.seq_start = d->text_seq_start.as<uint64_t>(); a.endmark = 1u;
    a.off_a = vw.cand_off.as<uint64_t>(); a.recs_a = vw.cands.as<pgx_read_verify>();
    if (max_extra > 0 && n) { a.off_b = w.extra_off.as<uint64_t>(); a.recs_b = w.extras.as<pgx_read_verify>(); a.more = w.more.as<uint32_t>(); }
    a.winners = vw.recs.as<pgx_read_verify>();
    // the rescue records that go with a merged list are those of the call that merged it: pgx_batch_read_rescue refuses any further call on a merged list,
    // with or without MERGE, so no later rescue result can stand in their place until the next verify call clears `merged`
    if (vw.merged && b->rw.valid && (b->rw.flags & PGX_RESCUE_MERGE) && b->rw.n_reads == n) a.rescue = b->rw.recs.as<pgx_read_rescue>();
    if (paired) { a.frag_min = mw.frag_min; a.frag_max = mw.frag_max; a.penalty = mw.penalty; }
    a.n_reads = n; a.scale = scale; a.slack = slack; a.max_cand = vw.max_cand;
    mapq_core(w, a, max_entries, paired, s, who);
    w.ms = w.timer.end(s);
    read_scalars(w.counters, w.ctr.p, 32, s); // (waits for the kernel: the call is complete on return)
    w.scale = scale; w.slack = slack; w.max_extra = max_extra; w.flags = flags; w.n_extras = n_extras;
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void mapqs_header(const pgx_batch *b, pgx_read_mapqs *out) {
    const MapqWork &w = b->qw;
    std::memset(out, 0, sizeof *out);
    out->n_reads = w.n_reads;
    out->n_has = w.counters[0]; out->n_unique = w.counters[1]; out->n_capped = w.counters[2]; out->sum_mapq = w.counters[3];
    out->n_extras = w.n_extras;
    out->scale = w.scale; out->slack = w.slack; out->max_extra = w.max_extra; out->flags = w.flags;
    out->ms_mapq = w.ms;
}

extern "C" pgx_status pgx_batch_device_mapqs(pgx_batch *b, pgx_read_mapqs *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->qw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_mapqs: batch has no mapq result");
    mapqs_header(b, out);
    out->records = b->qw.recs.as<pgx_read_mapq>();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_mapqs(pgx_batch *b, pgx_read_mapqs *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->qw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_mapqs: batch has no mapq result");
    use_device(b->device);
    MapqWork &w = b->qw;
    HostBuf none_off, none_items; // (the result has no list)
    download_pinned(b, StageResult{w.n_reads, w.recs.p, sizeof(pgx_read_mapq), false, nullptr, 0, nullptr, 0}, w.h_recs, none_off, none_items);
    mapqs_header(b, out);
    out->records = w.h_recs.as<pgx_read_mapq>();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_read_mapq_arrays(int device, const uint64_t *seq_offsets, uint64_t n_seq, const uint64_t *visit_offsets, const uint64_t *visit_nodes,
                                           const uint32_t *visit_length, uint64_t n_reads, const uint64_t *entry_offsets, const pgx_read_verify *entries,
                                           const uint32_t *chosen, const pgx_read_rescue *rescue, int64_t frag_min, int64_t frag_max, uint32_t penalty,
                                           const uint32_t *list_len, uint32_t scale, uint32_t slack, uint32_t flags, pgx_read_mapq *out) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_mapq_arrays");
    checked_device_count();
    const std::string who = "pgx_read_mapq_arrays";
    mapq_check_args(who, scale, slack, 0u, flags);
    const bool paired = (flags & PGX_MAPQ_PAIRED) != 0;
    if (!seq_offsets || !visit_offsets || !entry_offsets || (n_reads && (!out || !chosen))) throw Error(PGX_ERR_ARG, who + ": null argument");
    // what pgx_read_walk_arrays refuses of the tables
    const std::vector<uint64_t> marks = walk_table_marks(who, seq_offsets, n_seq, visit_offsets, visit_nodes, visit_length);
    // what pgx_read_mates_arrays refuses
    if (n_seq >= (1ull << 32) - 1) throw Error(PGX_ERR_ARG, who + ": n_seq " + std::to_string(n_seq) + " does not fit a record's seq");
    if (paired) {
        mates_check_args(who, frag_min, frag_max, 0u);
        if (n_seq & 1) throw Error(PGX_ERR_ARG, who + ": n_seq " + std::to_string(n_seq) + " is odd: sequences 2p and 2p + 1 are twins");
        if (const uint64_t bad = first_untwinned(seq_offsets, n_seq); bad != ~0ull)
            throw Error(PGX_ERR_ARG, who + ": sequences " + std::to_string(2 * bad) + " and " + std::to_string(2 * bad + 1) + " (p = " + std::to_string(bad) + ") have the lengths " +
                                         std::to_string(seq_offsets[2 * bad + 1] - seq_offsets[2 * bad]) + " and " + std::to_string(seq_offsets[2 * bad + 2] - seq_offsets[2 * bad + 1]) +
                                         ": twins have one length");
    }
    check_offsets(who, entry_offsets, n_reads, "entry_offsets", "read");
    const uint64_t n_entries = entry_offsets[n_reads];
    if (n_entries && !entries) throw Error(PGX_ERR_ARG, who + ": null argument");
    uint64_t max_entries = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t c = entry_offsets[r + 1] - entry_offsets[r], nl = list_len ? list_len[r] : c;
        if (c > PGX_MAPQ_MAX_ENTRIES) throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(r) + " has " + std::to_string(c) + " entries, more than " + std::to_string(PGX_MAPQ_MAX_ENTRIES));
        if (nl > c) throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(r) + " has list_len " + std::to_string(nl) + ", above its " + std::to_string(c) + " entries");
        if (chosen[r] != PGX_MAPQ_NO_CHOSEN && chosen[r] >= nl)
            throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(r) + " has chosen " + std::to_string(chosen[r]) + ", not below its list_len " + std::to_string(nl));
        max_entries = std::max(max_entries, c);
        for (uint64_t i = entry_offsets[r]; i < entry_offsets[r + 1]; i++) {
            const pgx_read_verify &e = entries[i];
            const std::string which = "entry " + std::to_string(i - entry_offsets[r]) + " of read " + std::to_string(r);
            if (e.seq >= n_seq) throw Error(PGX_ERR_ARG, who + ": " + which + " has seq " + std::to_string(e.seq) + ", not below n_seq " + std::to_string(n_seq));
            const int64_t ls = (int64_t)(seq_offsets[(uint64_t)e.seq + 1] - seq_offsets[e.seq]), lim = 1ll << 62;
            if (e.diag <= -lim || e.diag >= lim) throw Error(PGX_ERR_ARG, who + ": " + which + " has diag " + std::to_string(e.diag) + ", not inside +-2^62");
            if (e.span_hi > e.span_lo && (e.diag + (int64_t)e.span_lo < 0 || e.diag + (int64_t)e.span_hi > ls))
                throw Error(PGX_ERR_ARG, who + ": " + which + " has the span [" + std::to_string(e.span_lo) + ", " + std::to_string(e.span_hi) + ") at diag " + std::to_string(e.diag) +
                                             ", its sequence has " + std::to_string(ls) + " symbols");
        }
    }
    if (paired && (n_reads & 1)) throw Error(PGX_ERR_ARG, who + ": n_reads " + std::to_string(n_reads) + " is odd: reads 2k and 2k + 1 are the mates of pair k");
    (void)mapq_lane_shift(paired ? n_reads / 2 : n_reads, max_entries, who);
    use_device(device);
    struct MapqInput : WalkTables { // device copies of the input, the image + the stage's buffers, released on every way out
        DevBuf entry_off, entries, chosen, list_len, rescue;
        MapqWork w;
        ~MapqInput() { release_all({&entry_off, &entries, &chosen, &list_len, &rescue}); w.release(); }
    } k;
    hipStream_t s = nullptr;
    upload(k.entry_off, entry_offsets, (n_reads + 1) * 8);
    upload(k.entries, entries, n_entries * sizeof(pgx_read_verify));
    upload(k.chosen, chosen, n_reads * 4);
    if (list_len) upload(k.list_len, list_len, n_reads * 4);
    if (rescue) upload(k.rescue, rescue, n_reads * sizeof(pgx_read_rescue));
    PgxMapqArgs a{};
    a.walk = k.build(seq_offsets, n_seq, marks, visit_nodes, s);
    a.seq_start = k.seq_off.as<uint64_t>(); a.endmark = 0u;
    a.off_a = k.entry_off.as<uint64_t>(); a.recs_a = k.entries.as<pgx_read_verify>();
    a.list_len = list_len ? k.list_len.as<uint32_t>() : nullptr;
    a.chosen = k.chosen.as<uint32_t>();
    a.rescue = rescue ? k.rescue.as<pgx_read_rescue>() : nullptr;
    a.frag_min = frag_min; a.frag_max = frag_max; a.penalty = penalty;
    a.n_reads = n_reads; a.scale = scale; a.slack = slack;
    mapq_core(k.w, a, max_entries, paired, s, who);
    if (n_reads) HIPCHECK(hipMemcpyAsync(out, k.w.recs.p, n_reads * sizeof(pgx_read_mapq), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}
