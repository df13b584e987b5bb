// pgx_runtime_internal.hpp -- what the host units of the runtime share (pgx_runtime.hip, pgx_images.hip, pgx_tools.hip, and through
// pgx_batch_internal.hpp the units of the batch): roctx ranges, the small launch helpers, the device image of an index and the tag stage.
// Nothing here is part of the C ABI, and nothing is exported from libpgx.so.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "pgx_device.h"
#include "pgx_host.hpp"
#include "pgx_runtime.hpp"

#pragma GCC visibility push(hidden)

using namespace pgx;

// roctx ranges and stage marks for rocprofv3 --marker-trace (the reference's TIME stopwatches, src/find_mems.cpp:20-24,100-136).
// Off unless PGX_ROCTX=1: the library is looked up at run time so that nothing links against the profiler.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    void (*mark)(const char *) = nullptr;
    bool on = false;
};
const Roctx &roctx(); // pgx_runtime.hip
struct RoctxRange {
    bool on;
    explicit RoctxRange(const char *name) : on(roctx().on) { if (on) roctx().push(name); }
    ~RoctxRange() { if (on) roctx().pop(); }
    RoctxRange(const RoctxRange &) = delete;
    RoctxRange &operator=(const RoctxRange &) = delete;
};

// pgx_runtime.hip
int checked_device_count();   // PGX_ERR_NO_DEVICE where there is none
void use_device(int device);  // hipSetDevice after checking that the ordinal exists
// exclusive scan: out[n + 1] on the device (out[n] = total), async on `s`
void scan_excl(int mode, const void *in, uint64_t n, uint64_t min_len, uint64_t *out, DevBuf &tmp, hipStream_t s, uint64_t *total_out = nullptr,
               const uint64_t *n_dev = nullptr);
bool scan_three_launches(); // PGX_SCAN_THREE=1: every scan in its three-launch form
// the tail of the tag stage: pos_off[n + 1] = exclusive scan of the queries' position counts (from run_nums and uval), total also in *total_out.
// With `positions` (pos_cap values) the one-launch form stores the one-run queries' values in the same pass and raises bit 0 of *abort when the
// total exceeds pos_cap; returns whether those values are stored (false: the caller runs pgx_tag_compact_single_kernel, and checks the capacity).
bool scan_tag_tail(const uint64_t *run_nums, const uint64_t *uval, uint64_t n, uint64_t *pos_off, DevBuf &tmp, hipStream_t s, uint64_t *total_out, const uint64_t *n_dev,
                   uint64_t *positions, uint64_t pos_cap, uint64_t *abort);
// scalars the host needs to size the next buffer, through a small pinned buffer per host thread (synchronises `s`)
void read_scalars(void *dst, const void *dptr, size_t bytes, hipStream_t s);
inline uint64_t read_u64(const uint64_t *dptr, hipStream_t s) {
    uint64_t v = 0;
    read_scalars(&v, dptr, 8, s);
    return v;
}

struct pgx_device_image {
    int device = -1;
    PgxDevImage img{};
    DevBuf blocks, dir, blow, consts, tstart, tvals, tdir, tpair, tbucket, seed, seed_small, seed_end, exc, pairs, first_ext, sbase2, pbase;
    DevBuf rstart, rsamp, rdir, lpos, lnext, ldir; // locate image, uploaded on first use
    DevBuf lce_sa, lce_text, lce_flags, lce_lcp;   // LCE image (ensure_lce), built on the first batch
    DevBuf lce_seq_start;                          // with it: n_seq + 1 text positions, sequence q at [start[q], start[q + 1]) (pgx_batch_locate)
    uint64_t lce_n_seq = 0;
    int lce_state = 0;                             // 0 not tried, 1 built, 2 not available for this index / device
    DevBuf text4, text_seq_start;                  // TEXT image (ensure_text), built on its first use: 4-bit symbols; n_seq + 1 text positions
    uint64_t text_n_seq = 0;
    bool has_text = false;
    int twin_state = 0;                            // index_twinned: 0 not looked at, 1 twinned, 2 not (twin_bad: the first p with L[2p] != L[2p + 1])
    uint64_t twin_bad = 0;
    DevBuf walk_bits, walk_dir, walk_nodes;        // WALK image (ensure_walk), built on its first use: marks, rank directory, node << 1 | rev of every visit
    PgxWalkImage walk{};
    bool has_walk = false;
    DevBuf lit_bstart, lit_cum, lit_runs, lit_roff, lit_tabs; // literal count image (quirk 3), uploaded on first use
    PgxLitImage lit{};
    bool has_lit = false;
    PgxLocImage loc{};
    bool has_loc = false;
    size_t lds_bytes = 0; // dynamic LDS of the LDS-image kernels (0 = image stays in global memory)
};

// pgx_images.hip: one image per (index, device), created on first use; the locate, LCE and literal parts on their first use
pgx_device_image *device_image(pgx_index *h, int device);
pgx_device_image *locate_image(pgx_index *h, int device);
pgx_device_image *literal_image(pgx_index *h, int device);
void ensure_lce(pgx_index *h, pgx_device_image *d);
void ensure_text(pgx_index *h, pgx_device_image *d); // throws where the image cannot be built (include/pgx.h pgx_index_text)
// whether the collection holds every sequence next to a twin of its length (include/pgx.h "read mates"); needs the TEXT image; *first_bad as pgx_index_twinned
bool index_twinned(pgx_device_image *d, uint64_t *first_bad);
void ensure_walk(pgx_index *h, pgx_device_image *d); // builds the TEXT image too; throws where it cannot be built (include/pgx.h "read walk")
// the rank directory of a WALK image over n_blocks blocks of marks: dir[n_blocks + 1] on stream s (counts: n_blocks u64 of scratch)
void walk_directory(const uint64_t *bits, uint64_t n_blocks, DevBuf &counts, uint64_t *dir, DevBuf &scan_tmp, hipStream_t s);
// the section sum of an image file over n_bytes of device memory (16-byte aligned), added to *sum on stream s (pgx_image_sum_kernels.hip)
void launch_image_sum(const void *data, uint64_t n_bytes, unsigned long long *sum, hipStream_t s);

// pgx_runtime.hip: the r-index walk + optional segmented sort-unique behind pgx_locate_batch; values stay on the device in vals_out
void locate_core(pgx_index *h, pgx_device_image *d, const uint64_t *first, const uint64_t *last, uint64_t n, uint32_t flags, std::vector<uint64_t> &h_off,
                 DevBuf &vals_out, uint64_t &n_vals_out);
void locate_check_supported(const pgx_index *h, const char *who);

// pgx_tags_encode.hip: the query-format tag file (PGX_TAGS_COMPACT / PGX_TAGS_BYTECODE) of a run list in device memory, on stream `s` (synchronises it).
// zero_len_counts: the node of a run of length 0 still widens the compact item (pgx_write_compact_tags sees such runs; the files
// build_tags and merge_tags write never held them).  Writes out_path last; fills this thread's pgx_tags_encode_timing.
void tags_encode_device(const PgxTeRuns &runs, bool zero_len_counts, uint64_t max_node_floor, uint32_t format, const char *out_path, hipStream_t s);

inline void upload(DevBuf &b, const void *src, size_t bytes) {
    b.ensure(bytes ? bytes : 16);
    if (bytes) HIPCHECK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
}

inline unsigned grid_for(uint64_t n, unsigned per_block) {
    uint64_t g = (n + per_block - 1) / per_block;
    if (g == 0) g = 1;
    if (g > 0x7FFFFFFFull) throw Error(PGX_ERR_UNSUPPORTED, "batch too large for one launch");
    return (unsigned)g;
}

// what every release() is made of: the buffers of a brace list, the events of an array or a vector (destroyed and forgotten)
inline void release_all(std::initializer_list<DevBuf *> bufs) { for (DevBuf *d : bufs) d->release(); }
inline void release_all(std::initializer_list<HostBuf *> bufs) { for (HostBuf *h : bufs) h->release(); }
template <class Events> void destroy_events(Events &ev) {
    for (auto &e : ev)
        if (e) { (void)hipEventDestroy(e); e = nullptr; }
}

// ------------------------------------------------------------------------------------------
// tag pipeline shared by pgx_batch_run and pgx_tag_query_batch
// per query: run_nums (a result array) and uval (pgx_tag_locate_kernel); per list entry: a record (PgxTagRec).  need / scratch_off / scratch: global
// sort scratch of the representatives of the large list, only when one of them exceeds PGX_SORT_WG_LDS_CAP.
struct TagWork {
    DevBuf run_nums, uval, gbuf, need, scratch_off, scratch, pos_off, positions, small_recs, big_recs, large_recs, scan_tmp, dedup, dd_table;
    uint64_t n_positions = 0, n_big = 0;
    // what the last run needed (speculative sizing of the next one, pgx_batch_run): gathered values, positions, list lengths,
    // largest run count on the large list
    uint64_t last_G = 0, last_P = 0, last_small = 0, last_big = 0, last_large = 0, last_largest = 0, last_rep = 0, last_dup = 0;
    bool have_last = false;
    void release() {
        release_all({&run_nums, &uval, &gbuf, &need, &scratch_off, &scratch, &pos_off, &positions, &small_recs, &big_recs, &large_recs, &scan_tmp, &dedup, &dd_table});
    }
};

inline uint64_t with_slack(uint64_t v) { return v + v / 4 + 64; }

// Device scalars of the stage, sc[] (zeroed by the caller): [0] big-list length [1] large-list length [2] largest run count on the
// large list [3] total of gathered values G (the locate kernel hands out the lists' segments of gbuf from it) [5] small-list length
// [6] representatives [7] duplicates [8] positions.
//
// Exact mode (spec == false): the host reads the scalars back where they size the next buffer (three synchronisations).
// Speculative mode: every buffer and grid is sized from the previous run of this batch (+ 25 %), the counts stay on the device
// (kernels take a capacity and a device pointer to the actual count, pgx_tag_kernels.hip), capacity checks raise *d_abort on the
// device, and nothing is read back here: the caller reads all scalars once at the end and repeats the run in exact mode if the
// abort flag came up.  `m` is then the capacity of the per-query arrays and d_m points to the actual number of queries.
template <class Rec>
void tag_pipeline(const PgxDevImage &img, const pgx_mem *d_mems, const uint64_t *d_qs, const uint64_t *d_qe, uint64_t m, TagWork &w,
                         unsigned long long *d_nover, unsigned long long *sc, hipStream_t s, Rec &&rec, bool spec = false,
                         const uint64_t *d_m = nullptr, uint64_t *d_abort = nullptr) {
    const uint64_t mm = m ? m : 1;
    w.run_nums.ensure(mm * 8);
    w.uval.ensure(mm * 8);
    w.pos_off.ensure((m + 1) * 8);
    w.small_recs.ensure(mm * sizeof(PgxTagRec)); // (a query is on at most one list; which one is only known on the device)
    w.big_recs.ensure(mm * sizeof(PgxTagRec));
    w.large_recs.ensure(mm * sizeof(PgxTagRec));
    const uint64_t *u_sc = reinterpret_cast<const uint64_t *>(sc);
    const uint64_t *dn_small = spec ? u_sc + 5 : nullptr, *dn_big = spec ? u_sc + 0 : nullptr, *dn_large = spec ? u_sc + 1 : nullptr;
    const uint64_t *dn_rep = spec ? u_sc + 6 : nullptr, *dn_dup = spec ? u_sc + 7 : nullptr;
    const uint64_t *ab = spec ? d_abort : nullptr;
    if (!spec) d_m = nullptr; // exact mode: m is the count
    auto fixed_grid = [](uint64_t n, unsigned per_block, unsigned max_blocks) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>((n + per_block - 1) / per_block, 1), max_blocks); };
    uint64_t *run_nums = w.run_nums.as<uint64_t>(), *uval = w.uval.as<uint64_t>(), *pos_off = w.pos_off.as<uint64_t>();
    PgxTagRec *small_recs = w.small_recs.as<PgxTagRec>(), *big_recs = w.big_recs.as<PgxTagRec>(), *large_recs = w.large_recs.as<PgxTagRec>();
    if (m) { // run counts, the one-run values, the three lists with their segments of gbuf (sc[3] = G, the total of gathered values)
        const unsigned g = spec ? fixed_grid(m, PGX_TAG_LOCATE_THREADS, 8192) : grid_for(m, PGX_TAG_LOCATE_THREADS);
        hipLaunchKernelGGL(pgx_tag_locate_kernel, dim3(g), dim3(PGX_TAG_LOCATE_THREADS), 0, s, img, d_mems, d_qs, d_qe, m, d_m, ab, run_nums, uval, small_recs, big_recs,
                           large_recs, sc, d_nover);
        HIPCHECK(hipGetLastError());
    }
    uint64_t G, nbig, nlarge, nsmall, largest;
    if (!spec) {
        uint64_t hv[6] = {0, 0, 0, 0, 0, 0};
        read_scalars(hv, sc, 48, s);
        G = hv[3]; nbig = hv[0]; nlarge = hv[1]; nsmall = hv[5]; largest = hv[2];
    if (std::getenv("PGX_DEBUG_COUNTERS")) std::fprintf(stderr, "[pgx] tag stage: m %llu big %llu large %llu largest %llu G %llu small %llu\n", (unsigned long long)m,
                                                            (unsigned long long)nbig, (unsigned long long)nlarge, (unsigned long long)largest, (unsigned long long)G, (unsigned long long)nsmall);
    } else { // capacities from the previous run; the device checks what it can before anything is written through them
        G = with_slack(w.last_G); nbig = with_slack(w.last_big); nlarge = with_slack(w.last_large); nsmall = with_slack(w.last_small);
        // the large path sorts in dynamic LDS sized for the largest run count: twice the last one (a power of two), at most the
        // workgroup capacity -- a larger query aborts the speculative run (the caller never speculates beyond that capacity)
        uint64_t p2 = 64;
        while (p2 < 2 * w.last_largest && p2 < PGX_SORT_WG_LDS_CAP) p2 <<= 1;
        largest = p2;
        // [bit 0] gathered values, small list, [1] large list, [2] largest run count, [3] big list
        hipLaunchKernelGGL(pgx_spec_check_kernel, dim3(1), dim3(64), 0, s, u_sc + 3, G, u_sc + 1, nlarge, u_sc + 2, largest, u_sc + 0, nbig, u_sc + 5, nsmall, d_abort);
        HIPCHECK(hipGetLastError());
        if (largest > PGX_SORT_WG_LDS_CAP) throw Error(PGX_ERR_ARG, "speculative tag stage with a query beyond the LDS sort capacity"); // (the caller never asks for this)
    }
    w.n_big = nbig;
    rec(0);
    w.gbuf.ensure((G ? G : 1) * 8);
    uint64_t *gbuf = w.gbuf.as<uint64_t>();
    if (nsmall) { // queries with 2 .. 16 runs (single runs were answered by the locate kernel)
        const unsigned g = spec ? fixed_grid(nsmall, 16, 16384) : grid_for(nsmall, 16);
        hipLaunchKernelGGL(pgx_tag_small_kernel, dim3(g), dim3(256), 0, s, img, (const PgxTagRec *)small_recs, nsmall, dn_small, ab, gbuf, uval, d_nover);
        HIPCHECK(hipGetLastError());
    }
    rec(1);
    if (nbig) {
        const unsigned g = spec ? fixed_grid(nbig, 4, 8192) : grid_for(nbig, 4);
        hipLaunchKernelGGL(pgx_tag_gather_kernel, dim3(g), dim3(256), 0, s, img, (const PgxTagRec *)big_recs, nbig, dn_big, ab, gbuf, d_nover);
        hipLaunchKernelGGL(pgx_tag_sort_unique_kernel<PgxTagRecs>, dim3(g), dim3(256), 0, s, PgxTagRecs{big_recs}, nbig, dn_big, ab, gbuf, uval);
        HIPCHECK(hipGetLastError());
    }
    uint64_t nrep = 0, ndup = 0;
    if (nlarge) {
        uint64_t p2max = 64;
        while (p2max < largest && p2max < PGX_SORT_WG_LDS_CAP) p2max <<= 1;
        const size_t lds = (size_t)p2max * 8; // smaller segments -> more workgroups per CU
        // opt in to > 64 KiB of dynamic LDS (per device; cheap enough to repeat)
        HIPCHECK(hipFuncSetAttribute((const void *)pgx_tag_sort_large_kernel<PgxTagRecs>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(PGX_SORT_WG_LDS_CAP * 8)));
        // identical large queries are grouped on the device (pgx_tag_dedup_kernel): representatives are sorted, duplicates copy
        uint64_t tcap = 64;
        while (tcap < 2 * nlarge) tcap <<= 1;
        w.dd_table.ensure(tcap * 8);
        w.dedup.ensure(nlarge * (sizeof(PgxTagRec) + 16)); // [representatives' records | (duplicate, representative) pairs of list positions]
        PgxTagRec *d_reps = w.dedup.as<PgxTagRec>();
        uint64_t *d_pairs = reinterpret_cast<uint64_t *>(d_reps + nlarge);
        HIPCHECK(hipMemsetAsync(w.dd_table.p, 0, tcap * 8, s));
        hipLaunchKernelGGL(pgx_tag_dedup_kernel, dim3(fixed_grid(nlarge, 256, 1024)), dim3(256), 0, s, (const PgxTagRec *)large_recs, nlarge, dn_large, ab,
                           w.dd_table.as<unsigned long long>(), tcap - 1, d_reps, sc + 6, d_pairs, sc + 7);
        HIPCHECK(hipGetLastError());
        if (!spec) {
            uint64_t rd[2] = {0, 0};
            read_scalars(rd, sc + 6, 16, s);
            nrep = rd[0]; ndup = rd[1];
    if (std::getenv("PGX_DEBUG_COUNTERS")) std::fprintf(stderr, "[pgx] tag stage: representatives %llu duplicates %llu\n", (unsigned long long)nrep, (unsigned long long)ndup);
        } else { nrep = nlarge; ndup = nlarge; } // (capacities: the lists cannot be longer than the large list)
        uint64_t S = 0; // global sort scratch: only queries with more than PGX_SORT_WG_LDS_CAP runs need any (rare: a scan over the representatives then)
        w.scratch_off.ensure((nrep + 1) * 8);
        if (largest > PGX_SORT_WG_LDS_CAP && nrep) { // (exact mode only)
            w.need.ensure(nrep * 8);
            hipLaunchKernelGGL(pgx_tag_need_kernel, dim3(fixed_grid(nrep, 256, 1024)), dim3(256), 0, s, (const PgxTagRec *)d_reps, nrep, w.need.as<uint64_t>());
            HIPCHECK(hipGetLastError());
            scan_excl(1, w.need.p, nrep, 0, w.scratch_off.as<uint64_t>(), w.scan_tmp, s);
            S = read_u64(w.scratch_off.as<uint64_t>() + nrep, s);
        }
        w.scratch.ensure((S ? S : 1) * 8);
        if (nrep) {
            hipLaunchKernelGGL(pgx_tag_gather_kernel, dim3(spec ? fixed_grid(nrep, 4, 8192) : grid_for(nrep, 4)), dim3(256), 0, s, img, (const PgxTagRec *)d_reps, nrep,
                               dn_rep, ab, gbuf, d_nover);
            hipLaunchKernelGGL(pgx_tag_sort_large_kernel<PgxTagRecs>, dim3(spec ? fixed_grid(nrep, 1, 2048) : grid_for(nrep, 1)), dim3(1024), lds, s, PgxTagRecs{d_reps}, nrep,
                               dn_rep, ab, gbuf, w.scratch.as<uint64_t>(), (const uint64_t *)w.scratch_off.as<uint64_t>(), uval);
        }
        if (ndup)
            hipLaunchKernelGGL(pgx_tag_copy_dups_kernel, dim3(spec ? fixed_grid(ndup, 256, 4096) : grid_for(ndup, 256)), dim3(256), 0, s, (const uint64_t *)d_pairs, ndup,
                               dn_dup, ab, img.n_tag_items, large_recs, uval, d_nover);
        HIPCHECK(hipGetLastError());
    }
    // positions: the scan of the queries' counts.  A speculative run has sized `positions` already, so the scan stores the one-run queries' values as it
    // goes and checks the total against the capacity itself.  An exact run sizes `positions` from the scan's total, and a second pass of the same
    // scan stores those values (an exact run is the first of a batch or the repeat of an aborted one: the pass is off the repeated path).
    uint64_t P = spec ? with_slack(w.last_P) : 0;
    if (spec) w.positions.ensure((P ? P : 1) * 8);
    bool singles_stored = scan_tag_tail(run_nums, uval, m, pos_off, w.scan_tmp, s, reinterpret_cast<uint64_t *>(sc + 8), d_m,
                                        spec ? w.positions.as<uint64_t>() : nullptr, P, d_abort);
    if (!spec) {
        w.n_positions = read_u64(reinterpret_cast<const uint64_t *>(sc + 8), s);
        P = w.n_positions;
        w.positions.ensure((P ? P : 1) * 8);
        if (!scan_three_launches())
            singles_stored = scan_tag_tail(run_nums, uval, m, pos_off, w.scan_tmp, s, reinterpret_cast<uint64_t *>(sc + 8), nullptr, w.positions.as<uint64_t>(), P, nullptr);
    } else if (!singles_stored)
        hipLaunchKernelGGL(pgx_spec_check_kernel, dim3(1), dim3(64), 0, s, u_sc + 8, P, (const uint64_t *)nullptr, (uint64_t)0, (const uint64_t *)nullptr, (uint64_t)0,
                           (const uint64_t *)nullptr, (uint64_t)0, (const uint64_t *)nullptr, (uint64_t)0, d_abort);
    if (m) {
        // every query with positions is on exactly one list: small, big, large (16 lanes per query up to PGX_TAG_COMPACT_SMALL unique values, one
        // workgroup per query beyond); the one-run queries (a thread per query) only where the scan has not stored them (PGX_SCAN_THREE=1)
        const PgxTagRec *lists[3] = {small_recs, big_recs, large_recs};
        const uint64_t counts[3] = {nsmall, nbig, nlarge};
        const uint64_t *dcounts[3] = {dn_small, dn_big, dn_large};
        for (int li = 0; li < 3; li++)
            if (counts[li])
                hipLaunchKernelGGL(pgx_tag_compact_kernel<PgxTagRecs>, dim3(spec ? fixed_grid(counts[li], 16, 16384) : grid_for(counts[li], 16)), dim3(256), 0, s,
                                   PgxTagRecs{lists[li]}, counts[li], dcounts[li], ab, (const uint64_t *)uval, (const uint64_t *)gbuf, (const uint64_t *)pos_off,
                                   w.positions.as<uint64_t>(), (uint64_t)PGX_TAG_COMPACT_SMALL);
        if (!singles_stored)
            hipLaunchKernelGGL(pgx_tag_compact_single_kernel, dim3(spec ? fixed_grid(m, 256, 16384) : grid_for(m, 256)), dim3(256), 0, s, m, d_m, ab,
                               (const uint64_t *)run_nums, (const uint64_t *)uval, (const uint64_t *)pos_off, w.positions.as<uint64_t>());
        for (int li = 1; li < 3; li++)
            if (counts[li])
                hipLaunchKernelGGL(pgx_tag_compact_list_kernel<PgxTagRecs>, dim3(spec ? fixed_grid(counts[li], 1, 4096) : grid_for(counts[li], 1)), dim3(256), 0, s,
                                   PgxTagRecs{lists[li]}, counts[li], dcounts[li], ab, (const uint64_t *)uval, (const uint64_t *)gbuf, (const uint64_t *)pos_off,
                                   w.positions.as<uint64_t>(), (uint64_t)PGX_TAG_COMPACT_SMALL);
        HIPCHECK(hipGetLastError());
    }
    rec(2);
    if (!spec) { // what the next run of this batch may assume
        w.last_G = G; w.last_P = P; w.last_small = nsmall; w.last_big = nbig; w.last_large = nlarge; w.last_largest = largest;
        w.last_rep = nrep; w.last_dup = ndup;
        w.have_last = true;
    }
}

#pragma GCC visibility pop
