// pgx_device.h -- kernel-side view of the device image + kernel declarations (HIP only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pgx.h"
#include "pgx_image.h"

// Counters of one pgx_batch_run: u64 slots of pgx_batch::counters (the find_mems kernels receive the base pointer as `n_ext_total`).
// Slots below 16 are cleared per chunk of reads and per attempt; the others once per run.
enum PgxCounterSlot {
    PGX_CTR_EXT = 0,          // extensions performed (equal to the oracle's count)
    PGX_CTR_TAG_OVERFLOW = 1, // tag queries that read past the stored runs (quirk 7)
    PGX_CTR_CURSOR = 5,       // read cursor of the main launch
    PGX_CTR_HEAVY = 8,        // reads handed to pgx_find_mems_heavy_kernel
    PGX_CTR_OVF32 = 9,        // a coordinate left 32 bits (NARROW kernels): the chunk is repeated in 64 bits
    PGX_CTR_MEMS = 10,        // MEMs of the chunk (scan total)
    PGX_CTR_REDO = 11,        // extensions the pairs kernel took through the image it accompanies (flagged blocks, wide intervals)
    PGX_CTR_REDO_CURSOR = 12, // (unused since the pairs kernel no longer hands reads on)
    PGX_CTR_SIDE_CURSOR = 13, // read cursor of the side-stream launch (reads with a byte outside A C G T)
    PGX_CTR_OVF_TOP = 14,     // slots handed out of the arena of fifth-and-later MEMs (pgx_slot_extent)
    PGX_CTR_OVF_ABORT = 15,   // the arena was too small: the chunk is repeated in the worst-case slot layout
    PGX_CTR_TAG0 = 16,        // 16..24: tag stage (tag_pipeline)
    PGX_CTR_ABORT = 30,       // abort flag of a speculative run
    // what the kernels ask of the memory system (always on; bench.py's roofline): lane trips that fetch a rank-image line that is
    // not one every lane shares (a stage's first trip probes the full interval: block 0 / the last block), seed / end table entries read
    PGX_CTR_PAIRS_LINES = 32, // pgx_find_mems_pairs_kernel: 128-byte block lines (second-block trips included)
    PGX_CTR_PAIRS_SEEDS = 33, //                             seed / end table entries (16 bytes each, one line each)
    PGX_CTR_FM_LINES = 34,    // pgx_find_mems_kernel (global-memory images): 128-byte lines holding the blocks of its probes
    PGX_CTR_FM_SEEDS = 35,
    PGX_CTR_PAIRS_TWO = 36,   // pairs kernel: lane trips that performed two extensions
    // -DPGX_FM_STATS builds only (scripts/fm_stats.sh)
    PGX_CTR_ST_TRIPS = 40, PGX_CTR_ST_LIVE = 41, PGX_CTR_ST_LONGEST = 42,                  // pgx_find_mems_kernel: wave trips, live lane trips, longest wave
    PGX_CTR_ST_PAIR_TRIPS = 43, PGX_CTR_ST_PAIR_LIVE = 44, PGX_CTR_ST_PAIR_WAIT = 45, PGX_CTR_ST_PAIR_FRESH = 46,
    PGX_CTR_ST_PAIR_T_REFILL = 47, PGX_CTR_ST_PAIR_T_TOTAL = 48, PGX_CTR_ST_PAIR_REFILLS = 49, PGX_CTR_ST_PAIR_T_SEED = 50, PGX_CTR_ST_PAIR_T_LINE = 51, // clock ticks (s_memtime) of the waves in the refill loop / in all, refill rounds, ticks waiting for the seed entry / for the block line
    PGX_CTR_SLOTS = 64,  // (what the host reads back)
    PGX_CTR_ARENA0 = 64, // counters of the PGX_ARENA_SUBS sub-arenas, 16 slots (one cache line) apart
    PGX_CTR_ALL = 64 + 16 * 64
};
#define PGX_ARENA_SUBS 64u
#define PGX_TBUCKET_RUNS 10u // run starts a bucket line holds (pgx_tag_bucket_kernel); a bucket with more is flagged and answered through tdir / tpair

#define PGX_DENSE_LDS_U4 5 // uint4 slots per dense block in LDS (64 data bytes + 16 of padding)
#define PGX_FM_THREADS 256
#define PGX_LCE_MAX_OCC 128u // widest interval whose forward stage goes through the text (occurrence indexes and counts are bytes of the lane's state word)
#define PGX_FM_WAVES_PER_SIMD 4 // __launch_bounds__ 2nd argument: caps the kernel at 128 VGPRs

// passed by value to every kernel (all pointers are device pointers)
struct PgxDevImage {
    const uint4 *blocks;      // n_blocks * 4 (64-byte rank blocks)
    const uint64_t *dir;      // dir_entries (64-bit entries, see pgx_image.h)
    const uint16_t *blow;     // n_blocks (low dir_shift bits of each block start)
    const PgxConsts *consts;  // tables (ext_tab, C, slot_code)
    const uint64_t *tstart;   // n_tag_runs
    const uint64_t *tvals;    // n_tag_items
    const uint32_t *tdir;     // tag_dir_entries
    const ulonglong2 *tpair;  // (tstart[r], tvals[r]) side by side, max(n_tag_runs, n_tag_items) entries (NULL: not built)
    const uint4 *tbucket;     // tag runs by bucket of 2^tbucket_shift BWT positions, one 128-byte line each (pgx_tag_kernels.hip; NULL: not built)
    uint64_t n_tbuckets;
    uint32_t tbucket_shift;
    uint64_t n;
    uint64_t dir_entries;
    uint64_t n_tag_runs, n_tag_items, tag_dir_entries;
    uint32_t n_blocks;
    uint32_t dir_shift;
    uint32_t excl_mask;
    uint32_t tag_dir_shift;
    uint32_t dense; // image kind: 0 run-length blocks, 1 dense bit-plane blocks (PGX_IMAGE_DENSE), 2 dense2 (PGX_IMAGE_DENSE2); dir / blow unused unless 0
    const uint32_t *exc; // dense2: exception runs
    // k-mer seed table (dense images in global memory): entry idx = bi-interval after backward-extending the full interval by
    // the k bytes of a window, last byte first (pgx_seed_build_kernel); 0 = no table
    uint32_t seed_k;
    const uint4 *seed; // 4^seed_k entries {k lo, k' lo, s lo, k hi | k' hi << 8 | s hi << 16 | depth << 24}
    // end table: the same for a stage that starts at j = len: the full interval extended by 0 (what pattern[len] reads as) and then by the
    // seed_end_k bytes before the end of the read; depths count the extension by 0
    uint32_t seed_end_k;
    const uint4 *seed_end;
    // host side only (pgx_batch_run puts one of the two tables into seed / seed_k of the copy it launches with): the first table and a shallower one
    uint32_t seed_k_main, seed_k_small;
    const uint4 *seed_main, *seed_small;
    // PAIRS image (NULL without one): blocks, first extensions of the full interval
    const uint4 *pairs;
    const uint4 *first_ext;
    uint32_t pair_runs;
    // WIDE images (pgx_image.h): superblock bases and shifts; dense = 3 then (dense2 blocks with delta counts, 64-bit positions)
    const uint64_t *sbase2, *pbase;
    uint32_t d2_sb_shift, pairs_sb_shift, n_sb2, n_sbp;
    uint32_t wide;
    uint32_t pairs_stride; // positions between PAIRS block starts: PGX_PAIRS_SYMS or PGX_PAIRS_STRIDE64 (pgx_image.h)
    // suffix array + text (NULL without; narrow images with a PAIRS image only: pgx_image.h "LCE image"): the forward stage of a MEM whose interval is
    // narrow is finished by comparing the read with the text at the interval's occurrences, one occurrence per trip, instead of two symbols per trip
    const uint32_t *lce_sa;    // n entries: position of suffix i in lce_text
    const uint32_t *lce_text;  // two bits per symbol (A C T G = 0 1 2 3, the order of the packed reads), 16 symbols per word, sequences with their endmarkers
    const uint32_t *lce_flags; // one bit per 128-byte line of lce_text: the line holds a symbol outside A C G T or lies behind the text
    const uint8_t *lce_lcp;    // n entries (NULL without): symbols suffix i shares with suffix i - 1, capped at PGX_LCP_CAP; PGX_LCP_UNKNOWN where the comparison met a flagged line
    uint32_t lce_max;          // widest interval that goes this way
    uint32_t refill_min;       // LCE kernel: idle lanes of a wave wait for this many before the wave fetches new reads
};
#define PGX_LCP_CAP 254u     // lce_lcp: "this many symbols or more"
#define PGX_LCP_UNKNOWN 255u // lce_lcp: not known (the comparison touched a flagged line of the text)
#define PGX_SEED_UNUSABLE 255u // depth value of entries the kernels must not use (a coordinate does not fit the entry)
#define PGX_SEED_MAX_K 16
#define PGX_SEED_SMALL_K 10 // depth of the second table (searches whose min_len is below the depth of the first)

// run start r: from the interleaved (start, value) array when the image has one -- the locate kernel then finds the run's value in the
// cache line its search ended in (three random lines per MEM -> two)
#define PGX_TSTART(img, r) ((img).tpair ? (img).tpair[(r)].x : (img).tstart[(r)])
// rank_1(bwt_intervals, x + 1) = number of run starts <= x  (src/tag_arrays.cpp:857-858)
__device__ __forceinline__ uint64_t pgx_tag_rank(const PgxDevImage &img, uint64_t x) {
    const uint64_t nr = img.n_tag_runs;
    uint64_t di = x >> img.tag_dir_shift;
    if (di + 1 >= img.tag_dir_entries) return nr; // beyond bwt_intervals.size(): all ones
    uint64_t lo = img.tdir[di], hi = img.tdir[di + 1];
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (PGX_TSTART(img, mid) <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// heavy reads (pgx_fm_kernels.hip): handed from pgx_find_mems_kernel to pgx_find_mems_heavy_kernel
struct pgx_heavy_item {
    uint64_t rid;
    uint32_t x, nm; // next start position, MEMs already written
};
struct PgxHeavyResult { // find_mems_function(x) of one start position
    pgx_mem mem;
    uint32_t next_x, n_ext, has_mem, pad;
};
#define PGX_FM_HEAVY_EXT 2048u    // extensions spent on one read before the rest is handed on (ordinary 150-bp reads: ~200)
#define PGX_FM_SIDE_HEAVY_EXT 2048u // the same for the launch on the second stream (reads with a byte outside A C G T); see pgx_batch_run
#define PGX_FM_HEAVY_MAXLEN 4096u // reads up to this length take part (per-start results live in scratch)
#define PGX_FM_HEAVY_CAP 8192u    // heavy reads per launch; beyond that lanes simply continue sequentially
#define PGX_FM_HEAVY_GRID 64u

// ---- pgx_fm_kernels.hip: the one-step find_mems kernel, the rest of heavy reads, find_mems_function per call
template <bool LDS_IMAGE, int DENSE, bool NARROW, bool SEED> // DENSE = image kind
__global__ void pgx_find_mems_kernel(PgxDevImage img, const uint8_t *reads, const uint64_t *offsets, uint64_t n_reads,
                                     uint64_t min_len, uint64_t min_occ, const uint64_t *slot_off, pgx_mem *slots,
                                     uint32_t *mem_count, unsigned long long *n_ext_total, unsigned long long *cursor, uint64_t first_read,
                                     uint64_t slot_base, uint32_t heavy_ext, uint32_t heavy_cap, pgx_heavy_item *heavy_list, unsigned long long *heavy_count,
                                     const pgx_heavy_item *rid_list, const unsigned long long *rid_count, uint32_t *ovf_base, uint64_t ovf_cap);
template <bool LDS_IMAGE>
__global__ void pgx_find_mems_heavy_kernel(PgxDevImage img, const uint8_t *reads, const uint64_t *offsets, uint64_t min_len, uint64_t min_occ,
                                           const uint64_t *slot_off, uint64_t slot_base, pgx_mem *slots, uint32_t *mem_count,
                                           unsigned long long *n_ext_total, const pgx_heavy_item *heavy_list,
                                           const unsigned long long *heavy_count, uint32_t heavy_cap, PgxHeavyResult *scratch, uint64_t chunk_first,
                                           uint64_t chunk_reads, uint32_t *ovf_base, uint64_t ovf_cap);
__global__ void pgx_fmf_kernel(PgxDevImage img, const uint8_t *reads, const uint64_t *offsets, const uint64_t *read_of, const uint64_t *xs, uint64_t n,
                               uint64_t min_len, uint64_t min_occ, PgxHeavyResult *out);
__global__ void pgx_arena_demand_kernel(unsigned long long *ctr);

// ---- pgx_pairs_kernels.hip: the two-step find_mems kernel
// PAIRS image (pgx_image.h): two extensions per loop trip; an extension its blocks cannot answer (special positions) goes through the other image
// Its one argument (launch_pairs fills it): what the kernel reads of the image, and the launch.  The first group is used in every trip of the
// main loop and lives in scalar registers for the whole kernel; the second is read before the loop only; the third belongs to paths a wave takes
// rarely (a new group of reads, the fifth MEM of a read, a heavy read, an extension through the other image, the end of the kernel) and is
// fetched from the kernel argument segment where it is used (PGX_PAIRS_COLD in pgx_pairs_kernels.hip), so that it holds no register in between:
// with everything in registers the loop kept 82 scalar values in the lanes of two vector registers and fetched 165 of them back per trip.
// (Those paths read first_read, n_reads, min_len, heavy_ext and slots of the first group that way as well.)
struct PgxPairsArgs {
    // every trip
    const uint4 *pairs;                    // PgxDevImage: the PAIRS image, the seed tables, the LCE image (see there)
    const uint4 *seed, *seed_end;          // (the LCE instances keep the two tables in LDS: s_seedt)
    const uint32_t *lce_sa, *lce_text, *lce_flags;
    const uint8_t *lce_lcp;
    const uint8_t *reads;                  // the byte-window instances only (the packed ones read LDS)
    pgx_mem *slots;
    uint32_t *mem_count;
    uint64_t n, min_len, min_occ;          // (the LCE instances are launched for min_occ <= 1 only and do not read it)
    uint64_t first_read, n_reads;          // the launch serves reads [first_read, n_reads), fewer than 2^32
    uint32_t seed_k, seed_end_k, lce_max, refill_min;
    uint32_t pk_words, heavy_ext, pairs_sb_shift, dense;
    // before the loop
    const PgxConsts *consts;
    const uint4 *first_ext;
    const uint64_t *pbase;
    uint32_t n_sbp, pad0;
    // rare paths
    const uint64_t *offsets;
    const uint8_t *skip;
    const uint32_t *packed;
    unsigned long long *cursor, *ctr;      // ctr: the counters (PgxCounterSlot)
    const uint64_t *slot_off;
    uint64_t slot_base;
    uint32_t *ovf_base;
    uint64_t ovf_cap;
    pgx_heavy_item *heavy_list;
    unsigned long long *heavy_count;
    uint32_t heavy_cap, d2_sb_shift;
    const uint4 *blocks;                   // the image the PAIRS image accompanies (dense, dense2, wide dense2)
    const uint32_t *exc;
    const uint64_t *sbase2;
};
template <bool WIDE, bool PACKED, bool COOP, bool S64, bool LCE>
__global__ void pgx_find_mems_pairs_kernel(PgxPairsArgs a);

// ---- pgx_reads_kernels.hip: per-upload passes over the reads
__global__ void pgx_bad_chunks_kernel(const uint8_t *reads, uint64_t n_bytes, uint64_t *chunks, unsigned long long *count, uint64_t cap, uint32_t *packed);
__global__ void pgx_unpack_reads_kernel(const uint32_t *packed, uint64_t n_chunks, uint8_t *reads);
__global__ void pgx_side_reads_kernel(uint8_t *reads, const uint64_t *offsets, const uint64_t *side_ids, const uint64_t *side_off, const uint8_t *side_bytes, uint64_t n_side,
                                      uint8_t *flags, pgx_heavy_item *list, unsigned long long *count);
__global__ void pgx_classify_reads_kernel(const uint8_t *reads, const uint64_t *offsets, uint64_t n_reads, const uint64_t *chunks, const unsigned long long *n_chunks,
                                          uint64_t cap, uint32_t *flag_words, pgx_heavy_item *list, unsigned long long *count);

// ---- pgx_image_sum_kernels.hip: the section sum of an image file over bytes [0, n_bytes) of data (16-byte aligned), added to *sum; blocks of 256 threads
__global__ void pgx_image_sum_kernel(const uint4 *data, uint64_t n_bytes, unsigned long long *sum);

// ---- pgx_query_kernels.hip: seed table / first_ext builders, per-call rank / extend / count / LF (pgx_lit_count_kernel: below, with its image)
__global__ void pgx_seed_build_kernel(PgxDevImage img, const uint4 *src, uint4 *dst, uint32_t level, uint64_t n_dst, uint64_t limit, int end_table);
__global__ void pgx_first_ext_kernel(PgxDevImage img, uint4 *out); // out[byte] = {k, k', s, 0} of the full interval extended backward by byte; out[256 + byte]: by 0, then by byte
__global__ void pgx_rank_kernel(PgxDevImage img, const uint64_t *pos, uint64_t n, int true_codes, uint64_t *out);
template <bool LOOP, bool MULHI> __global__ void pgx_rank_probe_kernel(PgxDevImage img, const uint64_t *pos, uint64_t n, uint64_t *out);
template <bool LDS_IMAGE>
__global__ void pgx_extend_kernel(PgxDevImage img, const pgx_biint *in, const uint8_t *sym, const uint8_t *forward, uint64_t n,
                                  pgx_biint *out);
template <bool LDS_IMAGE>
__global__ void pgx_count_kernel(PgxDevImage img, const uint8_t *reads, const uint64_t *offsets, uint64_t n_reads, pgx_range *out);
__global__ void pgx_lf_kernel(PgxDevImage img, const pgx_range *in, const uint8_t *sym, uint64_t n, pgx_range *out);

// ---- pgx_scan_kernels.hip: exclusive scans, MEM compaction
// n_dev (may be NULL): the element count lives on the device, `n` is then the capacity the launch was sized for
// in2: the second input of mode 5 (NULL otherwise)
__global__ void pgx_scan_partial_kernel(int mode, const void *in, const void *in2, uint64_t n, uint64_t min_len, uint64_t *block_sums, const uint64_t *n_dev);
template <int MODE>
__global__ void pgx_scan_onepass_kernel(const void *in, uint64_t n, uint64_t min_len, uint64_t *out, uint64_t *total_out, const uint64_t *n_dev,
                                        unsigned long long *state, uint32_t epoch);
__global__ void pgx_scan_sums_kernel(uint64_t *block_sums, uint64_t nb);
// the tail of the tag stage in one launch: pos_off = exclusive scan of the queries' position counts (pgx_scan_load mode 5), and, with `positions`, every
// one-run query's value stored at its offset (below pos_cap); the tile with the grand total raises bit 0 of *abort when it exceeds pos_cap
__global__ void pgx_scan_tag_tail_kernel(const uint64_t *run_nums, const uint64_t *uval, uint64_t n, const uint64_t *n_dev, uint64_t *pos_off, uint64_t *total_out,
                                         uint64_t *positions, uint64_t pos_cap, uint64_t *abort, unsigned long long *state, uint32_t epoch);
__global__ void pgx_scan_apply_kernel(int mode, const void *in, const void *in2, uint64_t n, uint64_t min_len, const uint64_t *block_sums,
                                      uint64_t nb, uint64_t *out, uint64_t *total_out, int raw_sums, const uint64_t *n_dev);
__global__ void pgx_compact_mems_kernel(uint64_t first_read, uint64_t n_reads, const uint64_t *slot_off, uint64_t slot_base,
                                        const pgx_mem *slots, const uint32_t *mem_count, const uint64_t *local_off,
                                        uint64_t mem_base, pgx_mem *mems, uint64_t cap_mems, uint64_t *abort, const uint32_t *ovf_base, uint64_t ovf_cap);

// ---- pgx_compact_kernels.hip: the compact result form (pgx_batch_result_compact, pgx_compact_encode); one wave per block of 64 reads
__global__ void pgx_compact_size_kernel(const uint64_t *mem_off, const pgx_mem *mems, const uint64_t *run_nums, const uint64_t *pos_off,
                                        const uint64_t *positions, uint64_t n_reads, uint64_t n_blocks, int tags, uint64_t *sizes, uint64_t *first_mem,
                                        uint64_t *first_pos);
__global__ void pgx_compact_fill_kernel(const uint64_t *mem_off, const pgx_mem *mems, const uint64_t *run_nums, const uint64_t *pos_off,
                                        const uint64_t *positions, uint64_t n_reads, uint64_t n_blocks, int tags, const uint64_t *block_offsets,
                                        uint8_t *bytes);
__global__ void pgx_compact_fill_staged_kernel(const uint64_t *mem_off, const pgx_mem *mems, const uint64_t *run_nums, const uint64_t *pos_off,
                                               const uint64_t *positions, uint64_t n_reads, uint64_t n_blocks, int tags, const uint64_t *block_offsets,
                                               uint8_t *bytes);

// ---- pgx_format_kernels.hip: the find_mems text of a result (pgx_batch_format, pgx_format_result); lengths, three scans, fill by item class
struct PgxFormatArgs {
    const uint64_t *mem_off;   // n_reads + 1
    const pgx_mem *mems;       // n_mems
    const uint64_t *pos_off;   // n_mems + 1
    const uint64_t *loc_off;   // n_mems + 1; only read with a locate flag
    uint64_t n_reads, n_mems, first_seq;
    uint32_t flags;            // PGX_FORMAT_*
};
__global__ void pgx_format_item_len_kernel(const uint64_t *vals, uint64_t n, uint64_t max_length, uint8_t *len);
__global__ void pgx_format_mem_len_kernel(PgxFormatArgs a, const uint64_t *pcum, const uint64_t *vcum, uint64_t *mlen);
__global__ void pgx_format_read_len_kernel(PgxFormatArgs a, const uint64_t *mcum, uint64_t *rlen, uint8_t *elen);
__global__ void pgx_format_fill_reads_kernel(PgxFormatArgs a, const uint64_t *read_off, const uint64_t *err_off, char *text, char *err_text);
__global__ void pgx_format_fill_mems_kernel(PgxFormatArgs a, const uint64_t *read_off, const uint64_t *mcum, const uint64_t *pcum, const uint64_t *vcum,
                                            char *text, uint64_t *pbase, uint64_t *vbase);
__global__ void pgx_format_fill_items_kernel(const uint64_t *vals, uint64_t n, const uint64_t *off, uint64_t n_mems, const uint64_t *cum,
                                             const uint64_t *base, uint64_t max_length, char *text);

// ---- pgx_tag_kernels.hip: the tag stage
__global__ void pgx_tag_pair_kernel(const uint64_t *tstart, const uint64_t *tvals, uint64_t n_runs, uint64_t n_items, ulonglong2 *out);
__global__ void pgx_tag_bucket_kernel(const uint64_t *tstart, const uint64_t *tvals, uint64_t n_runs, uint64_t n_items, uint32_t shift, uint64_t n_buckets, uint4 *out);
#define PGX_TAG_LOCATE_THREADS 1024 // workgroup of pgx_tag_locate_kernel (one list atomic per workgroup)
#define PGX_SORT_LDS_CAP 2048 // values per wave sorted in an LDS slice (pgx_tag_sort_unique_kernel)
#define PGX_TAG_SMALL 16      // queries with at most this many runs take the 16-lane path
#define PGX_SORT_WG_LDS_CAP 16384 // values one workgroup sorts in (dynamic) LDS (pgx_tag_sort_large_kernel)

// A listed query (2 or more runs) as its list carries it: everything the gather, sort and compaction kernels need, read coalesced in list order.
// `seg` is the start of the query's segment of the gather buffer, assigned when the entry is appended (pgx_tag_locate_kernel); a duplicate of a large
// query is pointed at its representative's segment (pgx_tag_copy_dups_kernel).
struct __attribute__((aligned(32))) PgxTagRec { uint64_t q, first, cnt, seg; };
// How entry e of a list resolves to (query, count, segment start) in the sort and compaction kernels, and where its global sort scratch is listed:
// the records of the tag stage, or the dense per-query arrays of the locate paths (pgx_locate_batch, pgx_batch_locate; list == NULL: every query).
struct PgxTagRecs {
    const PgxTagRec *recs;
    __device__ __forceinline__ void get(uint64_t e, uint64_t &q, uint64_t &cnt, uint64_t &seg) const { const PgxTagRec r = recs[e]; q = r.q; cnt = r.cnt; seg = r.seg; }
    __device__ __forceinline__ uint64_t scratch_index(uint64_t e, uint64_t q) const { return e; }
};
struct PgxTagDense {
    const uint64_t *list, *cnt, *seg;
    __device__ __forceinline__ void get(uint64_t e, uint64_t &q, uint64_t &c, uint64_t &s) const { q = list ? list[e] : e; c = cnt ? cnt[q] : 0; s = seg[q]; }
    __device__ __forceinline__ uint64_t scratch_index(uint64_t e, uint64_t q) const { return q; }
};

// every kernel of the tag stage: (count as a value = capacity, device pointer to the actual count or NULL, abort flag or NULL)
// per query: run_nums[q] and uval[q] -- the value of a one-run query, 0 for an inverted one, the unique count of a listed one (written by the sort kernels).
// sc: the stage's scalars (tag_pipeline): [0] big-list length [1] large-list length [2] largest run count [3] gathered values [5] small-list length
__global__ void pgx_tag_locate_kernel(PgxDevImage img, const pgx_mem *mems, const uint64_t *qstart, const uint64_t *qend,
                                      uint64_t n, const uint64_t *n_dev, const uint64_t *abort, uint64_t *run_nums, uint64_t *uval,
                                      PgxTagRec *small_recs, PgxTagRec *big_recs, PgxTagRec *large_recs, unsigned long long *sc,
                                      unsigned long long *n_overflow);
__global__ void pgx_tag_small_kernel(PgxDevImage img, const PgxTagRec *recs, uint64_t n, const uint64_t *n_dev, const uint64_t *abort, uint64_t *buf,
                                     uint64_t *uval, unsigned long long *n_overflow);
__global__ void pgx_tag_gather_kernel(PgxDevImage img, const PgxTagRec *recs, uint64_t n_list, const uint64_t *n_dev, const uint64_t *abort, uint64_t *buf,
                                      unsigned long long *n_overflow);
template <class L>
__global__ void pgx_tag_sort_unique_kernel(L src, uint64_t n_list, const uint64_t *n_dev, const uint64_t *abort, uint64_t *buf, uint64_t *ucount);
template <class L>
__global__ void pgx_tag_sort_large_kernel(L src, uint64_t n_list, const uint64_t *n_dev, const uint64_t *abort, uint64_t *buf, uint64_t *scratch,
                                          const uint64_t *scratch_off, uint64_t *ucount);
__global__ void pgx_tag_need_kernel(const PgxTagRec *recs, uint64_t n_list, uint64_t *need);
__global__ void pgx_tag_dedup_kernel(const PgxTagRec *recs, uint64_t n_list, const uint64_t *n_dev, const uint64_t *abort, unsigned long long *table,
                                     uint64_t table_mask, PgxTagRec *reps, unsigned long long *n_rep, uint64_t *pairs, unsigned long long *n_dup);
__global__ void pgx_tag_copy_dups_kernel(const uint64_t *pairs, uint64_t n_pairs, const uint64_t *n_dev, const uint64_t *abort, uint64_t n_tag_items,
                                         PgxTagRec *recs, uint64_t *uval, unsigned long long *n_overflow);
template <class L>
__global__ void pgx_tag_compact_kernel(L src, uint64_t n, const uint64_t *n_dev, const uint64_t *abort, const uint64_t *ucount, const uint64_t *buf,
                                       const uint64_t *pos_off, uint64_t *positions, uint64_t max_count);
__global__ void pgx_tag_compact_single_kernel(uint64_t n, const uint64_t *n_dev, const uint64_t *abort, const uint64_t *run_nums, const uint64_t *uval,
                                              const uint64_t *pos_off, uint64_t *positions);
template <class L>
__global__ void pgx_tag_compact_list_kernel(L src, uint64_t n_list, const uint64_t *n_dev, const uint64_t *abort, const uint64_t *ucount,
                                            const uint64_t *buf, const uint64_t *pos_off, uint64_t *positions, uint64_t max_count);
// *v_i > c_i raises bit i of the abort flag; *v4 > c4 raises bit 0 as well
__global__ void pgx_spec_check_kernel(const uint64_t *v0, uint64_t c0, const uint64_t *v1, uint64_t c1, const uint64_t *v2, uint64_t c2,
                                      const uint64_t *v3, uint64_t c3, const uint64_t *v4, uint64_t c4, uint64_t *abort);
#define PGX_TAG_COMPACT_SMALL 256 // segments up to this many unique values are copied by the 16-lane kernel

// locate image (pgx_image.h), passed by value to the locate kernels (pgx_locate_kernels.hip, with the builders of the LCE image)
struct PgxLocImage {
    const uint64_t *rstart, *rsamp; // n_runs + 1, n_runs
    const uint32_t *rdir;
    const uint64_t *lpos, *lnext;   // n_last each
    const uint32_t *ldir;
    uint64_t n, n_runs, n_last, max_length, rdir_entries, ldir_entries;
    uint32_t rdir_shift, ldir_shift;
};
__global__ void pgx_locate_next_kernel(PgxLocImage loc, const uint64_t *prev, uint64_t n, uint64_t *out);
// LCE image (pgx_image.h): sequence lengths from the suffixes that start with an endmarker, suffix array in text coordinates + the text's symbols
// (the first symbol of suffix i is the one whose C-bucket holds i), text packed to two bits + line flags
__global__ void pgx_lce_seqlen_kernel(const uint64_t *sa, uint64_t n_seq, uint64_t max_length, unsigned long long *seq_len);
__global__ void pgx_lce_scatter_kernel(const uint64_t *sa, uint64_t n, uint64_t max_length, const uint64_t *seq_start, uint64_t n_seq, uint64_t c1, uint64_t c2, uint64_t c3,
                                       uint64_t c4, uint64_t c5, uint32_t *sa32, uint8_t *text8, unsigned long long *bad);
__global__ void pgx_lce_pack_kernel(const uint8_t *text8, uint64_t n, uint64_t n_words, uint32_t *text32, uint32_t *flags);
__global__ void pgx_lce_lcp_kernel(const uint32_t *sa32, const uint32_t *text32, const uint32_t *flags, uint64_t n, uint8_t *lcp);
__global__ void pgx_lce_rc_check_kernel(const uint8_t *text8, const uint64_t *seq_start, uint64_t n_seq, uint64_t n, unsigned long long *bad);
__global__ void pgx_locate_plan_kernel(PgxLocImage loc, const uint64_t *qs, const uint64_t *qe, uint64_t n, uint64_t *run0,
                                       uint64_t *n_pieces);
__global__ void pgx_locate_walk_kernel(PgxLocImage loc, const uint64_t *qs, const uint64_t *qe, uint64_t n_queries,
                                       const uint64_t *run0, const uint64_t *piece_off, uint64_t n_pieces, const uint64_t *val_off,
                                       uint64_t val_base, int seq_ids, uint64_t *out);

// MEM occurrences (pgx_mem_locate_kernels.hip, pgx_batch_locate)
#define PGX_ML_SPAN 4096 // values per block of the resident gather
#define PGX_ML_WIN 1024  // value offsets / sequence starts a block of it stages in LDS
__global__ void pgx_ml_plan_kernel(const pgx_mem *mems, uint64_t n, uint64_t bwt_n, uint64_t max_occ, uint64_t *cnt, uint64_t *qs, uint64_t *qe,
                                   unsigned long long *n_not_located);
__global__ void pgx_ml_cut_kernel(const uint64_t *off, uint64_t n, uint64_t m0, uint64_t budget, uint64_t *out);
__global__ void pgx_ml_gather_kernel(const pgx_mem *mems, const uint64_t *off, uint64_t m0, uint64_t m1, uint64_t o_first, uint64_t nv,
                                     const uint32_t *sa32, uint64_t bwt_n, const uint64_t *seq_start, uint64_t n_seq, uint64_t max_length,
                                     int seq_ids, uint64_t *out);
__global__ void pgx_ml_classify_kernel(const uint64_t *cnt, const uint64_t *off, uint64_t np, uint64_t *seg, uint64_t *wave_list,
                                       uint64_t *wg_list, uint64_t *need, uint64_t *ucount, unsigned long long *ctr);
// sequence sets: W = ceil(n_seq / 64) words a MEM.  The cap is one word per lane of a wave (pgx_ml_set_expand_kernel); beyond it a bitmap per
// MEM costs more than the ids it replaces.
#define PGX_ML_SET_WORDS_MAX 64
#define PGX_ML_SET_BATCH 8  // values a thread of the set kernel loads before it merges them
#define PGX_ML_SET_WIN 2048 // set words a block accumulates in LDS at a time (16 KiB next to the 16 KiB of offsets and sequence starts: five blocks a CU)
__global__ void pgx_ml_sets_kernel(const pgx_mem *mems, const uint64_t *off, uint64_t m0, uint64_t m1, uint64_t o_first, uint64_t nv,
                                   const uint32_t *sa32, uint64_t bwt_n, const uint64_t *seq_start, uint64_t n_seq, uint32_t W,
                                   unsigned long long *sets);
__global__ void pgx_ml_sets_ids_kernel(const uint64_t *off, uint64_t m0, uint64_t m1, uint64_t o_first, uint64_t nv, const uint64_t *ids, uint32_t W,
                                       unsigned long long *sets);
__global__ void pgx_ml_set_count_kernel(const unsigned long long *sets, uint64_t np, uint32_t W, uint32_t Wp, uint64_t *ucount);
__global__ void pgx_ml_set_expand_kernel(const unsigned long long *sets, uint64_t np, uint32_t W, const uint64_t *uloc, uint64_t *out);
__global__ void pgx_ml_stride_kernel(uint64_t *out, uint64_t n, uint64_t stride);

// ---- pgx_hits_kernels.hip: read hits (pgx_batch_read_hits, pgx_read_hits_arrays); sets: n_mems x W words in the PGX_LOCATE_SEQ_SETS form
#define PGX_HITS_THREADS 256
// n_seq <= 64: Sp = 1 << sp_shift lanes a read (Sp = the power of two >= n_seq), PGX_HITS_THREADS / Sp reads a block
__global__ void pgx_read_hits_kernel(const uint64_t *mem_off, const pgx_mem *mems, const unsigned long long *sets, uint64_t n_reads, uint64_t n_mems, uint64_t n_seq,
                                     uint32_t sp_shift, uint32_t flags, pgx_read_hit *hits, unsigned long long *best_sets, uint32_t *scores);
// n_seq > 64 (2 <= W <= PGX_ML_SET_WORDS_MAX): a wave a read
__global__ void pgx_read_hits_wide_kernel(const uint64_t *mem_off, const pgx_mem *mems, const unsigned long long *sets, uint64_t n_reads, uint64_t n_mems,
                                          uint64_t n_seq, uint32_t W, uint32_t flags, pgx_read_hit *hits, unsigned long long *best_sets, uint32_t *scores);
__global__ void pgx_read_hits_check_kernel(const uint64_t *mem_off, const pgx_mem *mems, uint64_t n_reads, uint64_t n_mems, unsigned long long *bad);

// ---- pgx_place_kernels.hip: read placement (pgx_batch_read_place, pgx_read_place_arrays); loc_off / values: the packed-position form
#define PGX_PLACE_THREADS 256
// aoff[n_reads + 1] / acnt[n_reads]: the anchors of a read; mx: [0] most MEMs of a read [1] largest MEM start [2] aoff[n_reads] [3] aoff[0]
__global__ void pgx_place_plan_kernel(const uint64_t *mem_off, const uint64_t *loc_off, const pgx_mem *mems, uint64_t n_reads, uint64_t n_mems, uint64_t n_values,
                                      uint64_t *aoff, uint64_t *acnt, unsigned long long *mx);
__global__ void pgx_place_first_kernel(const uint64_t *mem_off, uint64_t n_reads, uint64_t n_mems, uint64_t *mfirst);
__global__ void pgx_place_keys_kernel(const pgx_mem *mems, const uint64_t *loc_off, const uint64_t *mfirst, const uint64_t *values, uint64_t m0, uint64_t m1,
                                      uint64_t a_first, uint64_t na, uint64_t L, uint64_t span, uint64_t bias, uint32_t ordinal_bits, uint64_t *keys);
// 1 << g_shift lanes a read (g_shift 0 .. 6), PGX_PLACE_THREADS >> g_shift reads a block
template <bool LIST>
__global__ void pgx_place_sweep_kernel(const uint64_t *mem_off, const pgx_mem *mems, const uint64_t *loc_off, const uint64_t *acnt, const uint64_t *keys,
                                       const uint64_t *seg, const uint64_t *ucount, uint64_t r_pass, uint64_t r_first, uint64_t nr, uint64_t n_mems, uint64_t span,
                                       uint64_t bias, uint32_t ordinal_bits, uint32_t g_shift, pgx_read_place *recs, uint64_t *pcount, const uint64_t *list_off,
                                       pgx_placement *places);
__global__ void pgx_place_check_values_kernel(const uint64_t *values, uint64_t n_values, uint64_t L, uint64_t n_seq, const uint64_t *aoff, uint64_t n_reads,
                                              unsigned long long *bad);

// ---- pgx_verify_kernels.hip: the text image (pgx_image.h "TEXT image") and read verify (pgx_batch_read_verify, pgx_read_verify_arrays)
#define PGX_TEXT_END 0u // 4-bit codes of the text image: \n A C G N T = 0 .. 5
#define PGX_TEXT_A 1u
#define PGX_TEXT_C 2u
#define PGX_TEXT_G 3u
#define PGX_TEXT_N 4u
#define PGX_TEXT_T 5u
#define PGX_TEXT_SCATTER_END 4u // what pgx_text_mark_kernel writes over the 0xFF of an endmarker in the scattered text bytes
#define PGX_TEXT_PAD_WORDS 4u   // words behind the text: the verify kernel's aligned 4-byte loads reach at most one word beyond it
#define PGX_VERIFY_THREADS 256
__global__ void pgx_text_mark_kernel(const uint64_t *seq_start, uint64_t n_seq, uint64_t n, uint8_t *text8);
__global__ void pgx_text_scatter32_kernel(const uint32_t *sa32, uint64_t n, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t c4, uint64_t c5, uint8_t *text8);
// ascii = 0: text8 holds the scatter codes; 1: the bytes of a collection
__global__ void pgx_text_pack_kernel(const uint8_t *text8, uint64_t n, uint64_t n_words, uint32_t ascii, uint32_t *text4);
__global__ void pgx_text_unpack_kernel(const uint32_t *text4, uint64_t n, uint8_t *bytes);
__global__ void pgx_verify_code_kernel(const uint8_t *reads, uint64_t n_bytes, uint64_t n_words, uint32_t *rcode);
__global__ void pgx_verify_choose_kernel(const pgx_read_place *recs, const uint64_t *place_off, const pgx_placement *places, uint64_t n_reads, uint32_t max_cand,
                                         uint64_t *count, const uint64_t *cand_off, uint32_t *cand_seq, int64_t *cand_diag);
__global__ void pgx_verify_owner_kernel(const uint64_t *cand_off, uint64_t n_reads, uint64_t n_cands, uint64_t *cand_read);
__global__ void pgx_verify_check_kernel(const uint64_t *cand_read, const uint32_t *cand_seq, uint64_t n_cands, uint64_t n_seq, unsigned long long *bad);
__global__ void pgx_verify_kernel(const uint32_t *text4, const uint64_t *seq_start, uint32_t endmark, const uint32_t *rcode, const uint64_t *read_off,
                                  const uint64_t *cand_off, const uint64_t *cand_read, const uint32_t *cand_seq, const int64_t *cand_diag, uint64_t n_cands,
                                  uint32_t penalty, pgx_read_verify *out);
__global__ void pgx_verify_reduce_kernel(const pgx_read_verify *cands, const uint64_t *cand_off, uint64_t n_reads, pgx_read_verify *out);

// ---- pgx_mates_kernels.hip: read mates (pgx_batch_read_mates, pgx_read_mates_arrays)
#define PGX_MATES_THREADS 256
// 2^g_shift lanes a pair, at least the candidates of either mate; sequence q has seq_start[q + 1] - seq_start[q] - endmark symbols; winners: NULL without
// PGX_MATES_ELECT; counters: pairs PROPER, COMPATIBLE, with A moved, with B moved (added to)
__global__ void pgx_mates_kernel(const uint64_t *seq_start, uint32_t endmark, const uint64_t *cand_off, const pgx_read_verify *cands, uint64_t n_pairs, uint32_t g_shift,
                                 int64_t frag_min, int64_t frag_max, uint32_t penalty, uint32_t flags, pgx_read_mates *out, pgx_read_verify *winners,
                                 unsigned long long *counters);

// ---- pgx_rescue_kernels.hip: read rescue (pgx_batch_read_rescue, pgx_read_rescue_arrays)
#define PGX_RESCUE_THREADS 256
// a task: read t on sequence seq over the diagonals [d_lo, d_hi] (empty: d_hi < d_lo), and what the scan found there (PgxRescueBest, n == 0: nothing)
struct PgxRescueTask {
    int64_t d_lo, d_hi;
    uint64_t read;
    uint32_t seq, anchor;
};
struct PgxRescueBest {
    int64_t d;          // the smallest diagonal that holds (score, matches)
    uint32_t score, matches;
    uint32_t next;      // the largest score below `score` (0: none)
    uint32_t n_best, n; // a task scores at most 2^31 + 2^32 diagonals only in theory: its window holds at most PGX_RESCUE_MAX_WINDOW
    uint32_t pad;
};
// tasks == nullptr: task_count[t] = anchors of read t (0: no target); else the tasks of read t behind task_off[t].  mates: the pair records of
// pgx_mates_kernel under the same frag bounds (n_compatible is read).
__global__ void pgx_rescue_targets_kernel(const uint64_t *seq_start, uint32_t endmark, const uint64_t *read_off, const uint64_t *cand_off, const pgx_read_verify *cands,
                                          const pgx_read_mates *mates, uint64_t n_reads, int64_t frag_min, int64_t frag_max, uint32_t max_anchors, uint64_t *task_count,
                                          const uint64_t *task_off, PgxRescueTask *tasks);
// a wave a task, a lane a diagonal
__global__ void pgx_rescue_scan_kernel(const uint32_t *text4, const uint64_t *seq_start, uint32_t endmark, const uint32_t *rcode, const uint64_t *read_off,
                                       const PgxRescueTask *tasks, uint64_t n_tasks, uint32_t penalty, PgxRescueBest *best);
// a thread a read: its record from its tasks; counters: targets, rescued, full, tasks, diagonals (added to); rescued: NULL, or 1 where RESCUED else 0
__global__ void pgx_rescue_reduce_kernel(const uint64_t *cand_off, const pgx_read_mates *mates, const uint64_t *task_count, const uint64_t *task_off,
                                         const PgxRescueTask *tasks, const PgxRescueBest *best, uint64_t n_reads, uint32_t min_score, pgx_read_rescue *out,
                                         uint64_t *rescued, unsigned long long *counters);
// MERGE: the candidate arrays of the rescued reads (slot res_off[t]) for pgx_verify_kernel; fake_off[t] makes its n_cand the list ordinal
__global__ void pgx_rescue_cands_kernel(const pgx_read_rescue *recs, const uint64_t *cand_off, const uint64_t *rescued, const uint64_t *res_off, uint64_t n_reads,
                                        uint64_t *cand_read, uint32_t *cand_seq, int64_t *cand_diag, uint64_t *fake_off, uint64_t *new_count);
// MERGE: the list rebuilt, a thread a record: the n_old old ones (owner: old_read) and the n_res rescued ones (owner: res_read), each behind new_off
__global__ void pgx_rescue_copy_kernel(const pgx_read_verify *old_cands, const uint64_t *old_off, const uint64_t *old_read, uint64_t n_old, const pgx_read_verify *res_cands,
                                       const uint64_t *res_read, uint64_t n_res, const uint64_t *new_off, pgx_read_verify *out);

// ---- pgx_align_kernels.hip: read align (pgx_batch_read_align, pgx_read_align_arrays)
#define PGX_ALIGN_THREADS 256
__global__ void pgx_align_cand_kernel(const pgx_read_verify *recs, uint64_t n_reads, uint32_t *cand_seq, int64_t *cand_diag);
__global__ void pgx_align_need_kernel(const uint64_t *read_off, uint64_t n_reads, uint32_t row_bytes, uint64_t *need);
// LG: log2 of the lanes a read takes, the smallest with 2^LG >= 2 W + 1; reads [r0, r1), their planes behind plane_off[r] - plane_off[r0]
template <int LG>
__global__ void pgx_align_forward_kernel(const uint32_t *text4, const uint64_t *seq_start, uint32_t endmark, const uint32_t *rcode, const uint64_t *read_off,
                                         const uint32_t *cand_seq, const int64_t *cand_diag, uint64_t r0, uint64_t r1, uint32_t W, const uint64_t *plane_off,
                                         uint8_t *planes, uint2 *fwd);
__global__ void pgx_align_trace_kernel(const uint64_t *seq_start, uint32_t endmark, const uint64_t *read_off, const uint32_t *cand_seq, const int64_t *cand_diag,
                                       uint64_t r0, uint64_t r1, uint32_t W, uint32_t row_bytes, const uint64_t *plane_off, const uint8_t *planes, const uint2 *fwd,
                                       uint32_t write, pgx_read_align *out, uint64_t *count, const uint64_t *op_off, uint32_t *ops);

// ---- pgx_walk_kernels.hip: the WALK image (pgx_image.h) and the read walk stage (pgx_batch_read_walk, pgx_read_walk_arrays, pgx_index_paths)
struct PgxWalkImage {
    const uint64_t *bits;  // n_words
    const uint64_t *dir;   // n_blocks + 1
    const uint64_t *nodes; // n_visits
    uint64_t n, n_words, n_blocks, n_visits;
};
__global__ void pgx_walk_mark_kernel(PgxDevImage img, const uint32_t *sa32, const uint64_t *sa64, uint64_t max_length, const uint64_t *seq_start, uint64_t n_seq, uint64_t n,
                                     int64_t delta, uint32_t *bits32, unsigned long long *bad);
__global__ void pgx_walk_set_kernel(const uint64_t *marks, uint64_t n_marks, uint32_t *bits32);
__global__ void pgx_walk_popc_kernel(const uint64_t *bits, uint64_t n_blocks, uint64_t *counts);
__global__ void pgx_walk_nodes_kernel(PgxDevImage img, PgxWalkImage w, const uint32_t *sa32, const uint64_t *sa64, uint64_t max_length, const uint64_t *seq_start,
                                      uint64_t n_seq, uint64_t n, int64_t delta, uint64_t *nodes);
__global__ void pgx_walk_check_kernel(PgxWalkImage w, const uint64_t *seq_start, uint64_t n_seq, uint32_t endmark, unsigned long long *bad);
__global__ void pgx_walk_positions_kernel(PgxWalkImage w, uint64_t *pos);
// recs (the batch's align records) or seq / text_start / text_end (arrays); first[r] = k0, the read's first visit
__global__ void pgx_walk_count_kernel(PgxWalkImage w, const uint64_t *seq_start, uint32_t endmark, uint64_t n_seq, const pgx_read_align *recs, const uint32_t *seq,
                                      const uint64_t *text_start, const uint64_t *text_end, uint64_t n_reads, pgx_read_walk *out, uint64_t *n_steps, uint64_t *first);
__global__ void pgx_walk_fill_kernel(PgxWalkImage w, const uint64_t *n_steps, const uint64_t *first, const uint64_t *step_off, uint64_t n_reads, uint64_t *steps);

// ---- pgx_mapq_kernels.hip: read mapq (pgx_batch_read_mapq, pgx_read_mapq_arrays)
#define PGX_MAPQ_THREADS 256
// The entries of read r: recs_a[off_a[r] .. off_a[r + 1]), then (off_b != NULL) recs_b[off_b[r] .. off_b[r + 1]); the first list_len[r] of them (NULL: those
// of recs_a) are list candidates, the rest extras.  The chosen ordinal: the winner record's cand_index (winners != NULL), or chosen[r].
struct PgxMapqArgs {
    PgxWalkImage walk;
    const uint64_t *seq_start; // n_seq + 1; sequence q has seq_start[q + 1] - seq_start[q] - endmark symbols
    const uint64_t *off_a, *off_b;
    const pgx_read_verify *recs_a, *recs_b;
    const uint32_t *list_len;
    const pgx_read_verify *winners;
    const uint32_t *chosen;
    const pgx_read_rescue *rescue; // NULL: no rescue terms
    const uint32_t *more;          // NULL, or per read: more next-level placements exist than extras were taken (PGX_MAPQ_CAPPED)
    int64_t frag_min, frag_max;    // PAIRED
    uint64_t n_reads;
    uint32_t endmark, g_shift, scale, slack, penalty;
    uint32_t max_cand;             // 0, or PGX_MAPQ_CAPPED from this many list candidates on
    pgx_read_mapq *out;
    unsigned long long *counters;  // reads with HAS, of them with E == 0, reads CAPPED, the sum of mapq (added to)
};
// count[r] / more[r] (cand_seq == NULL), or the extras of read r behind extra_off[r]
__global__ void pgx_mapq_choose_extras_kernel(const pgx_read_place *recs, const uint64_t *place_off, const pgx_placement *places, const uint64_t *cand_off,
                                              uint64_t n_reads, uint32_t max_extra, uint64_t *count, uint32_t *more, const uint64_t *extra_off, uint32_t *cand_seq,
                                              int64_t *cand_diag);
// 2^g_shift lanes a read (PAIRED: a pair of mates), at least the entries of any read
template <bool PAIRED>
__global__ void pgx_mapq_kernel(PgxMapqArgs a);

// ---- pgx_pack_kernels.hip: read pack (pgx_pack_add, pgx_pack_finish, pgx_read_pack_arrays)
#define PGX_PACK_THREADS 256
#define PGX_PACK_NODE_LANES 16u // lanes that summarise one node (pgx_pack_summary_kernel)
// the node table: len[id] (0: no visit names the id) and base[id], the exclusive prefix sum of len; n_nodes = max_id + 1
struct PgxPackTable {
    const uint32_t *len;
    const uint64_t *base; // n_nodes + 1
    uint64_t n_nodes;
};
__global__ void pgx_pack_max_id_kernel(const uint64_t *nodes, uint64_t n_visits, unsigned long long *max_id);
// a thread a word of marks: every visit's length into len_min / len_max of its id; a visit longer than PGX_WALK_MAX_VISIT: atomicMin of its id into too_long
__global__ void pgx_pack_visit_len_kernel(PgxWalkImage w, const uint64_t *seq_start, uint64_t n_seq, uint32_t endmark, uint64_t n_nodes, uint32_t *len_min, uint32_t *len_max,
                                          unsigned long long *bad, unsigned long long *too_long);
// len_min -> len in place (0 for an id without a visit); an id with len_min != len_max: atomicMin into bad
__global__ void pgx_pack_node_len_kernel(uint32_t *len_min, const uint32_t *len_max, uint64_t n_nodes, unsigned long long *bad);
// a lane a read: recs + mapqs (the batch) or seq / text_start / keep (arrays; mapqs == NULL); counters: reads counted, reads filtered, bases added
__global__ void pgx_pack_add_kernel(const pgx_read_align *recs, const uint32_t *seq, const uint64_t *text_start, const uint64_t *op_off, const uint32_t *ops,
                                    const pgx_read_mapq *mapqs, const uint8_t *keep, uint32_t min_mapq, uint64_t n_reads, const uint64_t *seq_start, uint64_t n_seq,
                                    uint64_t n, int *tdiff, unsigned long long *counters);
// a workgroup a tile of PGX_SCAN_BLOCK_ITEMS entries of tdiff (n1 = n + 1 entries): its sum, sign-extended
__global__ void pgx_pack_tile_sum_kernel(const int *tdiff, uint64_t n1, uint64_t *tile_sums);
// the same tiles: tdiff -> text coverage, every covered position projected onto cov, the tile zeroed; *projected += the positions projected
__global__ void pgx_pack_fold_kernel(int *tdiff, uint64_t n1, const uint64_t *tile_off, PgxWalkImage w, PgxPackTable t, uint32_t *cov, unsigned long long *projected);
// PGX_PACK_NODE_LANES lanes a node
__global__ void pgx_pack_summary_kernel(PgxPackTable t, const uint32_t *cov, uint32_t *covered, uint64_t *sum, uint32_t *max);

// literal count image: COMPAT count_encoded / LF_encoded on an encoded index without N, block by block as the
// reference's rankAt_encoded (src/r-index.cpp:570-590) sees it -- true cumulative counts, run scan one varint late
struct PgxLitImage {
    const uint64_t *bstart, *cum, *runs; // n_blocks ; 6 n_blocks ; all runs (code << 56 | length)
    const uint32_t *roff;                // n_blocks + 1
    const uint32_t *code_of, *cslot_of;  // 256 each
    uint64_t C[8];
    uint64_t n, n_blocks;
};
// (pgx_query_kernels.hip) out[i] = LF over `steps` symbols: count mode (in == NULL): the whole read i from {0, n - 1}; LF mode: one symbol sym[i] from in[i]
__global__ void pgx_lit_count_kernel(PgxLitImage lit, const uint8_t *reads, const uint64_t *offsets, const pgx_range *in, const uint8_t *sym,
                                     uint64_t n, pgx_range *out);

// merge_tags passes (pgx_merge_kernels.hip)
__global__ void pgx_mt_file_of_kernel(const uint64_t *da, uint64_t n, uint64_t n_seq, const uint32_t *seq_to_file, uint32_t n_files,
                                      uint8_t *file_of, unsigned long long *n_bad);
__global__ void pgx_mt_expand_kernel(const uint64_t *start, const uint64_t *val, uint64_t n_runs, uint64_t *out);
__global__ void pgx_mt_gather_kernel(const uint8_t *file_of, uint32_t f, const uint64_t *rank, const uint64_t *expanded, uint64_t total,
                                     uint64_t n, uint64_t *tags);
__global__ void pgx_mt_flags_kernel(const uint64_t *tags, uint64_t n, uint64_t n_seq, uint8_t *flags);
__global__ void pgx_mt_compact_kernel(const uint64_t *tags, const uint8_t *flags, const uint64_t *idx, uint64_t n, uint64_t n_seq,
                                      uint64_t *out_val, uint64_t *out_start);

// build_tags passes (pgx_build_tags_kernels.hip)
__global__ void pgx_bt_endmarker_kernel(const uint64_t *sa, uint64_t n_seq, uint64_t max_length, uint64_t *idx_len);
__global__ void pgx_bt_tag_kernel(uint64_t *sa, uint64_t n, uint64_t n_seq, uint64_t max_length, const uint64_t *seq_len, const uint64_t *dir_off,
                                  const uint64_t *dir, const uint64_t *node_start, const uint64_t *path_nodes, unsigned long long *bad);
__global__ void pgx_bt_heads_kernel(const uint64_t *tags, uint64_t n, uint64_t n_seq, uint8_t *head);
__global__ void pgx_bt_compact_kernel(const uint64_t *tags, const uint8_t *head, const uint64_t *idx, uint64_t n, uint64_t *run_val, uint64_t *run_start);
__global__ void pgx_bt_length_kernel(const uint64_t *run_start, uint64_t n_runs, uint64_t n, uint32_t reference_runs, uint64_t *run_len);
__global__ void pgx_bt_size_kernel(const uint64_t *run_val, const uint64_t *run_len, uint64_t n_runs, uint64_t *bytes);
__global__ void pgx_bt_write_kernel(const uint64_t *run_val, const uint64_t *run_len, const uint64_t *byte_off, uint64_t n_runs, uint8_t *body);

// tag query files from a run list (pgx_tags_encode_kernels.hip, pgx_tags_encode)
struct PgxTeRuns { // run i: value val[i]; length aux[i], or aux[i + 1] - aux[i] with the last run ending at n_end; mod16: length mod 65 536
    const uint64_t *val, *aux;
    uint64_t n_runs, n_end;
    uint32_t aux_is_start, mod16;
};
struct PgxTeSd { // an sd_vector of m ascending ones (ones == NULL: ones[i] = 10 i) with low width wl
    const uint64_t *ones;
    uint64_t m;
    uint32_t wl;
};
struct PgxTeField { // `bytes` low bytes of `value` at byte `offset` of the file
    uint64_t offset, value;
    uint32_t bytes, pad;
};
#define PGX_TE_EXPAND_PIECES 0u
#define PGX_TE_EXPAND_STREAM 1u
__global__ void pgx_te_count_kernel(PgxTeRuns runs, uint32_t zero_counts, uint64_t *n_pieces, uint64_t *lens, uint64_t *n_bytes, unsigned long long *max_node);
__global__ void pgx_te_expand_kernel(PgxTeRuns runs, const uint64_t *piece_off, const uint64_t *pos_off, const uint64_t *byte_off, uint32_t what, uint64_t *pos,
                                     uint64_t *items, uint64_t *sstart, uint8_t *stream);
__global__ void pgx_te_pack_items_kernel(const uint64_t *items, uint64_t count, uint32_t width, uint8_t *out, uint64_t n_words);
__global__ void pgx_te_sd_low_kernel(PgxTeSd sd, uint8_t *out, uint64_t n_words);
__global__ void pgx_te_sd_high_kernel(PgxTeSd sd, uint8_t *out, uint64_t n_words);
__global__ void pgx_te_sel_size_kernel(PgxTeSd sd, uint32_t b, uint64_t arg_cnt, uint64_t n_sb, uint64_t logn4, uint64_t *first, uint8_t *meta, uint64_t *sizes,
                                       unsigned int *any_long);
__global__ void pgx_te_sel_super_kernel(const uint64_t *first, uint64_t n_sb, uint32_t logn, uint8_t *out, uint64_t n_words);
__global__ void pgx_te_sel_kind_kernel(const uint8_t *meta, uint64_t n_sb, uint8_t *out, uint64_t n_words);
__global__ void pgx_te_sel_body_kernel(PgxTeSd sd, uint32_t b, uint64_t arg_cnt, const uint64_t *first, const uint8_t *meta, const uint64_t *off, uint8_t *out);
__global__ void pgx_te_fields_kernel(const PgxTeField *fields, uint32_t n, uint8_t *out);

// reads as text -> CSR reads (pgx_fastx_kernels.hip, pgx_batch_upload_text)
#define PGX_FASTX_ROUNDS 4                        // 16-byte loads per thread and tile
#define PGX_FASTX_TILE (256 * 16 * PGX_FASTX_ROUNDS) // bytes of text per block of the newline passes
// error word: first bad line << 8 | code (atomicMin)
#define PGX_FASTX_ERR_NO_AT 1u        // FASTQ header line without '@'
#define PGX_FASTX_ERR_NO_PLUS 2u      // FASTQ third line without '+'
#define PGX_FASTX_ERR_QUAL_LEN 3u     // FASTQ quality length != sequence length
#define PGX_FASTX_ERR_TRUNCATED 4u    // FASTQ text ends inside a record (line: its header)
#define PGX_FASTX_ERR_BEFORE_FIRST 5u // FASTA text before the first '>'
#define PGX_FASTX_ERR_LONG_LINE 6u    // a line of 2^31 bytes or more
__global__ void pgx_fastx_count_kernel(const uint8_t *text, uint64_t n, uint32_t *tile_count);
__global__ void pgx_fastx_lines_kernel(const uint8_t *text, uint64_t n, const uint64_t *tile_base, uint64_t *ls, uint64_t n_lines, uint32_t tail);
__global__ void pgx_fastx_role_kernel(const uint8_t *text, const uint64_t *ls, uint64_t n_lines, uint32_t format, uint32_t *contrib, uint8_t *rec,
                                      unsigned long long *err);
__global__ void pgx_fastx_records_kernel(uint64_t n_lines, uint32_t format, const uint32_t *contrib, const uint8_t *rec, const uint64_t *out_off,
                                         const uint64_t *rec_idx, uint64_t *offs, unsigned long long *err);
__global__ void pgx_fastx_longest_kernel(const uint64_t *offs, const uint64_t *n_reads, unsigned long long *longest);
__global__ void pgx_fastx_copy_kernel(const uint8_t *text, const uint64_t *ls, const uint64_t *out_off, uint64_t n_lines, uint64_t total, uint8_t *out);

// text collection -> suffix order, BWT, runs (pgx_build_sa_kernels.hip, pgx_build_index_from_text[s]_device)
#define PGX_SA_K 10           // symbols of the first key (3 bits each): the depth the doubling starts from
#define PGX_SA_TILE 2048      // symbols / rows per block of the counting passes (256 threads x 8)
#define PGX_SA_SORT_TILE 4096 // elements per block of a radix pass (256 threads x 16 rounds)
__global__ void pgx_sa_classify_kernel(const uint8_t *text, uint64_t n, uint64_t *codes, uint64_t n_words, uint32_t *tile_nl, unsigned long long *first_bad);
__global__ void pgx_sa_keys_kernel(const uint64_t *codes, uint64_t n_words, uint64_t n, const uint64_t *tile_off, uint64_t n_seq, uint32_t *hi, uint32_t *lo,
                                   uint32_t *idx, uint32_t *seq_start);
__global__ void pgx_sa_hist_kernel(const uint32_t *key, uint64_t n, uint32_t shift, uint32_t n_blocks, uint32_t *hist);
__global__ void pgx_sa_scatter_kernel(const uint32_t *hi, const uint32_t *lo, const uint32_t *idx, uint64_t n, int key_is_hi, uint32_t shift, uint32_t n_blocks,
                                      const uint64_t *offs, uint32_t *hi_out, uint32_t *lo_out, uint32_t *idx_out);
__global__ void pgx_sa_heads_kernel(const uint32_t *hi, const uint32_t *lo, uint64_t n, uint32_t *tile_cnt);
__global__ void pgx_sa_ranks_kernel(const uint32_t *hi, const uint32_t *lo, const uint32_t *idx, uint64_t n, const uint64_t *tile_off, uint32_t *hi_out,
                                    uint32_t *rank);
__global__ void pgx_sa_gather_kernel(const uint32_t *idx, const uint32_t *rank, uint64_t n, uint64_t h, uint32_t *lo);
__global__ void pgx_sa_bwt_kernel(const uint32_t *sa, const uint8_t *text, uint64_t n, uint8_t *bwt);
__global__ void pgx_sa_run_heads_kernel(const uint8_t *bwt, uint64_t n, uint32_t *tile_cnt);
__global__ void pgx_sa_runs_kernel(const uint8_t *bwt, const uint32_t *sa, uint64_t n, const uint64_t *tile_off, uint64_t n_runs, uint8_t *run_sym,
                                   uint32_t *run_start, uint32_t *run_head, uint32_t *run_tail);

#define PGX_SCAN_BLOCK_ITEMS 2048 // 256 threads x 8 items (pgx_scan_kernels.hip PGX_SCAN_ITEMS)
#define PGX_SCAN1_TILE_ITEMS 4096 // 256 threads x 16 rounds (pgx_scan_onepass_kernel)
