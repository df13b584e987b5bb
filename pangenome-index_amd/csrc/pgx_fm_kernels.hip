// pgx_fm_kernels.hip -- the one-step find_mems kernels for gfx950 (CDNA4).
//
//   pgx_find_mems_kernel   one lane = one read; every loop trip performs exactly one FMD extension
//                          (= two rank probes) for every live lane of the 64-wide wavefront.
//                          Replaces find_all_mems / find_mems_function (algorithm.hpp:653-757) +
//                          backward/forward_extend_encoded (src/r-index.cpp:713-764) +
//                          rank_at_cached_encoded (:619-641).
//   pgx_find_mems_heavy_kernel, pgx_fmf_kernel   find_mems_function per start position: the rest of a heavy read, the per-call entry point.
//   pgx_arena_demand_kernel                      what the reads asked of the arena of fifth-and-later MEMs.
//
// All of it is 64-bit integer work bound by random access into the rank image (HBM / L2 / LDS);
// there is no floating point and nothing MFMA-shaped.  Wave width is hard-coded to 64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pgx_device.h"
#include "pgx_rank_device.h"
#include "pgx_slots_device.h"

// ------------------------------------------------------------------------------------------
// find_all_mems for a batch.  State machine of find_mems_function (algorithm.hpp:653-736):
//   phase 1  backward from j = x+min_len-1 down to x          (:666-676)
//   phase 2  forward  from j = x+min_len   up to len-1        (:684-696)  -> emit MEM (:713)
//   phase 3  backward from j = e down to x+1, fresh interval  (:718-735); pattern[len] reads 0
//
// Persistent work-queue kernel: one lane owns one live read; every trip of the main loop performs
// exactly one extension for every live lane.  A lane whose read is finished is refilled at once
// (reads differ 2-3x in their extension counts, so a static read->lane map leaves most lanes idle):
// the wavefront keeps a private reservoir [rnext, rend) of read ids that lane 0 replenishes with
// one atomicAdd of PGX_FM_BATCH on the global cursor, and idle lanes take ids from it in lane order
// (ballot + prefix popcount).  Every wave leaves the loop once the cursor has passed n_reads and
// all its lanes are idle.  MEMs go to per-read slots, so the output does not depend on scheduling.
//
// Heavy reads: a read whose suffix ends a sequence makes step 3 walk the whole read for every start position
// (pattern[len] = 0 is the endmarker): ~len^2 / 2 extensions in one dependent chain, 100 x an
// ordinary read, tens of milliseconds for one lane.  A lane that has spent `heavy_ext` extensions on its read hands the
// rest (rid, next start, MEMs so far) to pgx_find_mems_heavy_kernel at the next start-position boundary.
#define PGX_FM_BATCH (LDS_IMAGE ? 128u : 32u) // reads per grab: fewer leave less in the wave's reserve when the queue runs dry (synth: 32 < 64 < 128 < 256),
                                               // but the LDS kernels are fast enough to feel the contention on the cursor (x: 128 < 64)
// NARROW (dense images of BWTs shorter than 2^30 only): interval coordinates and rank sums in 32 bits -- half the moves,
// selects and adds of the loop.  Sound because every true value is < 2^32 there; the junk coordinates the COMPAT quirks can
// produce are caught at the two additions that could wrap (counter slot 9 is raised and the host repeats the chunk in 64 bits).
template <bool LDS_IMAGE, int DENSE, bool NARROW, bool SEED>
__global__ void __launch_bounds__(PGX_FM_THREADS, DENSE == 0 ? 3 : PGX_FM_WAVES_PER_SIMD) // the run-length decode does not fit 128 VGPRs without spilling
pgx_find_mems_kernel(PgxDevImage img, const uint8_t *__restrict__ reads, const uint64_t *__restrict__ offsets,
                     uint64_t n_reads, uint64_t min_len, uint64_t min_occ, const uint64_t *__restrict__ slot_off,
                     pgx_mem *__restrict__ slots, uint32_t *__restrict__ mem_count, unsigned long long *__restrict__ n_ext_total,
                     unsigned long long *__restrict__ cursor, uint64_t first_read, uint64_t slot_base, uint32_t heavy_ext, uint32_t heavy_cap,
                     pgx_heavy_item *__restrict__ heavy_list, unsigned long long *__restrict__ heavy_count,
                     const pgx_heavy_item *__restrict__ rid_list, const unsigned long long *__restrict__ rid_count, uint32_t *__restrict__ ovf_base, uint64_t ovf_cap) {
    __shared__ uint32_t s_ext[512];
    __shared__ uint64_t s_C[8];
    __shared__ uint64_t s_sb[DENSE == 3 ? PGX_SB_MAX * 8 : 1]; // WIDE dense2: superblock bases
    PGX_LDS_CARVE(img);
    if (DENSE == 3) for (uint32_t i = threadIdx.x; i < img.n_sb2 * 8u; i += blockDim.x) s_sb[i] = img.sbase2[i];
    pgx_stage_tables<LDS_IMAGE>(img, s_ext, s_C, lds_blocks, lds_dir, lds_blow);
    // rid_list (may be NULL): the launch serves the reads listed there (the reads with a byte outside A C G T, which the pairs kernel skips: the launch
    // on the second stream), *rid_count of them, each from the start position listed, keeping the MEMs written before
    const uint64_t chunk_first = first_read, chunk_reads = n_reads - first_read; // (n_reads is the END of the chunk)
    if (rid_list) { first_read = 0; n_reads = *rid_count; }

    static_assert(!NARROW || DENSE, "the 32-bit state exists for the dense image only");
    static_assert(!SEED || DENSE, "k-mer seeds exist for the dense images");
    static_assert(DENSE < 2 || !LDS_IMAGE, "the dense2 image is never staged in LDS");
    static_assert(DENSE != 3 || !NARROW, "the wide dense2 image is walked in 64 bits");
    typedef typename std::conditional<NARROW, uint32_t, uint64_t>::type pos_t;
    const int lane = threadIdx.x & 63;
    const pos_t n = (pos_t)img.n;
    uint64_t rid = 0, base = 0;
    int32_t len = 0, x = 0, j = 0;
    pos_t k = 0, kp = 0, s = 0, Jk = 0, Js = 0;
    uint32_t nm = 0, next = 0, next0 = 0; // next0: value of `next` when the current read was taken
    int ph = 0;                      // 0 = idle (no read, or read finished)
    // read bytes cached in registers: 32 (absolute, 32-aligned offset) when the image is in global memory and the loop waits
    // on memory anyway (8 -> 16 -> 32 bytes: 3.94 -> 3.77 -> 3.72 ms on the synthetic pangenome), 8 when it is in LDS and the
    // loop is bound by issue slots.  The reads buffer is padded with 32 zero bytes, so the window never overruns.
    uint64_t win = 0, win_hi = 0, win2 = 0, win3 = 0, win_at = ~0ull;
    pos_t A0 = 0, B0 = 0;             // first-probe sums of an extension whose second probe is pending
    bool pend = false;
    uint32_t fresh = 0;              // (a 32-bit flag: as a bool captured by the lambdas below it ended up in scratch memory) SEED: the interval is the full one and a backward stage is about to start (the seed table may apply)
    bool ovf = false;                // NARROW: some addition left 32 bits (reported once, when the wave leaves)
    uint64_t rnext = 0, rend = 0;    // wave-uniform reservoir of read ids
    bool exhausted = false;          // wave-uniform: the global cursor has passed n_reads
    unsigned long long ln_blk = 0, ln_seed = 0; // wave-uniform (scalar registers): image lines / seed entries the wave asked for (PGX_CTR_FM_LINES / _SEEDS; images in global memory)
#ifdef PGX_FM_STATS
    unsigned long long st_trips = 0, st_live = 0; // diagnostics build only (scripts/fm_stats.sh)
#endif

    // begin(x): entry of find_mems_function; finishing a read records its MEM count
    auto begin = [&]() __attribute__((always_inline)) {
        if (x >= len || (uint64_t)(len - x) < min_len) { ph = 0; mem_count[rid] = nm; return; } // :745 / :658
        if (heavy_ext && next - next0 >= heavy_ext && len <= (int32_t)PGX_FM_HEAVY_MAXLEN) { // hand the rest of a heavy read on
            const unsigned long long at = atomicAdd(heavy_count, 1ull);
            if (at < (unsigned long long)heavy_cap) {
                pgx_heavy_item it;
                it.rid = rid; it.x = (uint32_t)x; it.nm = nm;
                heavy_list[at] = it;
                ph = 0;
                return;
            }
        }
        k = 0; kp = 0; s = n;
        if (min_len == 0) { // step 1 runs zero times (:666); step 2 starts at j = x
            Jk = 0; Js = n; j = x; ph = 2;
        } else {
            j = x + (int32_t)min_len - 1; ph = 1;
            fresh = 1u;
        }
    };
    // the state machine below funnels every "next start position" through one begin() (the lambda is inlined per call site)
    uint32_t restart = 0;
    // emit the MEM [x, e) and set up step 3
    auto emit = [&]() __attribute__((always_inline)) {
        pgx_mem m;
        m.start = (uint64_t)x; m.end = (uint64_t)j; m.bwt_start = (uint64_t)Jk; m.size = (int64_t)(uint64_t)Js; // e == j at every emit
        // (the extent of the read is looked up -- or, in an arena, reserved -- only by a fifth MEM: the first PGX_FAST_SLOTS have their own line)
        const uint64_t slot = nm < PGX_FAST_SLOTS ? 0ull : pgx_slot_extent(slot_off, slot_base, ovf_base, ovf_cap, n_ext_total, rid, nm, len, x, min_len);
        slots[pgx_slot_index(rid - chunk_first, chunk_reads, slot, nm)] = m;
        nm++;
        k = 0; kp = 0; s = n;
        // (as selects: an if / else that stores 1 into one of two flags is turned into ONE store through a selected address,
        //  which puts both flags into scratch memory)
        const bool more = j > x; // otherwise the loop of :722 runs zero times and the function returns j + 1
        ph = more ? 3 : ph;
        fresh = more ? 1u : fresh;
        x = more ? x : x + 1;
        restart = more ? restart : 1u;
    };

    for (;;) {
        // up until the probes' loads are out (pgx_dense2_pair lowers it again): see pgx_find_mems_pairs_kernel.  A launch that serves a list of reads (the
        // reads with a byte outside A C G T, on the second stream next to the pairs kernel: few, each a long chain) stays up: it is one wave per SIMD among
        // the other kernel's five, and at equal terms it took 5 to 19 ms from run to run -- longer than the pairs kernel it is meant to hide behind
        if (DENSE >= 2) __builtin_amdgcn_s_setprio(3);
        // ---- refill idle lanes ----
        unsigned long long idle = __ballot(ph == 0);
        while (idle) {
            if (rnext == rend) {
                if (exhausted) break;
                unsigned long long got = 0;
                if (lane == 0) got = first_read + atomicAdd(cursor, (unsigned long long)PGX_FM_BATCH); // the cursor counts from 0
                // wave-uniform values are moved to scalar registers explicitly
                got = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(got >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)got);
                if (got >= n_reads) { exhausted = true; break; }
                rnext = got;
                rend = got + PGX_FM_BATCH < n_reads ? got + PGX_FM_BATCH : n_reads;
            }
            const uint64_t avail = rend - rnext;
            const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
            if (ph == 0 && (uint64_t)rank < avail) {
                x = 0; nm = 0;
                rid = rnext + rank;
                if (rid_list) { const pgx_heavy_item it = rid_list[rid]; rid = it.rid; x = (int32_t)it.x; nm = it.nm; }
                base = offsets[rid];
                len = (int32_t)(offsets[rid + 1] - base);
                next0 = next;
                begin(); // may leave the lane idle again (read shorter than min_len)
                if (ph == 0) ph = -1; // served in this round; becomes idle again below
            }
            const uint32_t want = (uint32_t)__popcll(idle);
            rnext += (uint64_t)want < avail ? (uint64_t)want : avail;
            idle = __ballot(ph == 0);
        }
        if (ph == -1) ph = 0;
        if (!__any(ph > 0)) {
            if (exhausted && rnext == rend) break; // nothing live, nothing left
            continue;                               // only zero-work reads were handed out: refill again
        }
        // ---- one block decode for every live lane: an extension whose second probe falls outside the block
        //      of the first takes two trips of this loop (pend = 1 in between), so no lane ever waits for
        //      another lane's second trip ----
#ifdef PGX_FM_STATS
        st_trips++;
        st_live += (unsigned long long)__popcll(__ballot(ph > 0));
#endif
        // what the wave asks of the memory system in this trip (wave-uniform sums in scalar registers; images in global memory): seed / end table
        // entries -- one per first trip of a backward stage, an upper bound: windows that hold a byte outside A C G T and stages with fewer than
        // K extensions to go read the shared entry 0 -- and, counted behind the block, the lines holding the blocks of the two probes
        if (SEED) ln_seed += (unsigned long long)__popcll(__ballot(ph > 0 && fresh != 0u)); // (the seed table is in global memory whether or not the image is staged in LDS)
        bool c_blk = false, c_blk2 = false;
        if (ph > 0) {
            // ---- k-mer seed of a backward stage that starts now: the entry is loaded next to the block loads of the ordinary
            //      extension by P[j] (which every lane performs regardless) and replaces its result further down ----
            bool seed_lane = false;
            uint32_t kuse = 0u; // extensions the seed entry stands for
            uint4 se = make_uint4(0u, 0u, 0u, 0u);
            if (SEED) {
                const uint4 *sp = img.seed;
                if (fresh) {
                    // a stage that starts at j = len (step 3 of a MEM that reaches the end of its read) extends by 0 first, pattern[len]:
                    // the end table holds that extension followed by the seed_end_k bytes before the end of the read
                    const bool endw = j >= len;
                    const int32_t K = endw ? (int32_t)img.seed_end_k : (int32_t)img.seed_k;
                    const int32_t avail = (ph == 1) ? (j - x + 1) : (j - x); // extensions this stage may still perform
                    if (K && avail >= K + (endw ? 1 : 0)) {
                        const uint64_t a = base + (uint64_t)((endw ? len - 1 : j) - K + 1);
                        const uint32_t sh = (uint32_t)(a & 7ull) * 8u;
                        const uint64_t *wp = reinterpret_cast<const uint64_t *>(reads + (a & ~7ull)); // 32 zero bytes follow the last read
                        const uint64_t w0 = wp[0], w1 = wp[1], w2 = wp[2];
                        const uint64_t lo = sh ? (w0 >> sh) | (w1 << (64u - sh)) : w0, hi = sh ? (w1 >> sh) | (w2 << (64u - sh)) : w1;
                        uint32_t sidx;
                        if (pgx_seed_index(lo, hi, (uint32_t)K, sidx)) { seed_lane = true; sp = (endw ? img.seed_end : img.seed) + sidx; kuse = (uint32_t)K + (endw ? 1u : 0u); }
                    }
                }
                fresh = 0u;
                se = *sp; // lanes without a seed read entry 0 (one cached line for all of them)
            }
            uint32_t byte = 0u; // pattern[len] reads as 0 (quirk 4)
            if (j < len) {
                const uint64_t at = base + (uint64_t)j;
                if (LDS_IMAGE) {
                    if ((at & ~7ull) != win_at) { // reads are padded with 16 zero bytes: the window never overruns
                        win_at = at & ~7ull;
                        win = *reinterpret_cast<const uint64_t *>(reads + win_at);
                    }
                    byte = (uint32_t)(win >> (8u * (uint32_t)(at & 7ull))) & 0xFFu;
                } else {
                    if ((at & ~31ull) != win_at) {
                        win_at = at & ~31ull;
                        const ulonglong2 w2 = *reinterpret_cast<const ulonglong2 *>(reads + win_at);
                        const ulonglong2 w3 = *reinterpret_cast<const ulonglong2 *>(reads + win_at + 16);
                        win = w2.x; win_hi = w2.y; win2 = w3.x; win3 = w3.y;
                    }
                    const uint64_t wlo = (at & 8ull) ? win_hi : win, whi = (at & 8ull) ? win3 : win2;
                    byte = (uint32_t)(((at & 16ull) ? whi : wlo) >> (8u * (uint32_t)(at & 7ull))) & 0xFFu;
                }
            }
            const bool fwd = (ph == 2);
            // extension by `byte` (backward, or forward = backward on the swapped interval by the complement,
            // folded into ext_tab[256 + byte]): src/r-index.cpp:713-764
            const uint32_t ee = s_ext[(fwd ? 256u : 0u) + byte];
            const uint32_t cv = PGX_EXT_CV(ee), mrow = PGX_EXT_M(ee);
            const pos_t kk = fwd ? kp : k, kq = fwd ? k : kp;
            bool fin;
            pos_t A1, dB;
            if (DENSE == 3) {
                // wide dense2: the same probes with 64-bit positions and superblock bases from LDS
                const uint64_t p0 = kk > n ? n : kk, p1 = (kk + s) > n ? n : (kk + s);
                uint64_t q0, q1, dq;
                pgx_dense2w_pair(img, s_sb, p0, p1, cv, mrow, q0, q1, dq, !rid_list);
                A0 = (pos_t)q0; A1 = (pos_t)q1; dB = (pos_t)dq;
                fin = true;
                c_blk = s != n;
                c_blk2 = c_blk && (uint32_t)(((p0 >> 7) * 0xAAAAAAABull) >> 33) != (uint32_t)(((p1 >> 7) * 0xAAAAAAABull) >> 33);
            } else if (DENSE == 2) {
                // dense2: header + one sub-block per probe, all within one 128-byte line (usually the same line for both probes)
                uint64_t q0, q1, dq;
                if (NARROW) {
                    const uint32_t ks = (uint32_t)kk + (uint32_t)s;
                    ovf |= ks < (uint32_t)kk;
                    const uint32_t p0 = (uint32_t)kk > (uint32_t)n ? (uint32_t)n : (uint32_t)kk, p1 = ks > (uint32_t)n ? (uint32_t)n : ks;
                    pgx_dense2_pair<true>(img, p0, p1, cv, mrow, q0, q1, dq, !rid_list);
                } else {
                    const uint64_t p0 = kk > n ? n : kk, p1 = (kk + s) > n ? n : (kk + s); // (kk + s wraps only from junk coordinates: either way >= n or tiny)
                    pgx_dense2_pair<false>(img, (uint32_t)p0, (uint32_t)p1, cv, mrow, q0, q1, dq, !rid_list);
                }
                A0 = (pos_t)q0; A1 = (pos_t)q1; dB = (pos_t)dq;
                fin = true;
                if (s != n) { // (the full interval probes block 0 and the last block: lines every lane shares)
                    const uint64_t e0 = (uint64_t)kk > (uint64_t)n ? (uint64_t)n : (uint64_t)kk, e1 = (uint64_t)kk + (uint64_t)s > (uint64_t)n ? (uint64_t)n : (uint64_t)kk + (uint64_t)s;
                    c_blk = true; c_blk2 = (uint32_t)((e0 * 0xAAAAAAABull) >> 40) != (uint32_t)((e1 * 0xAAAAAAABull) >> 40);
                }
            } else if (NARROW) {
                const uint32_t ks = (uint32_t)kk + (uint32_t)s;
                ovf |= ks < (uint32_t)kk; // kk + s left 32 bits (junk coordinates of a COMPAT quirk): the host repeats the chunk in 64 bits
                const uint32_t p0 = (uint32_t)kk > (uint32_t)n ? (uint32_t)n : (uint32_t)kk, p1 = ks > (uint32_t)n ? (uint32_t)n : ks;
                const PgxDenseBlk k0 = pgx_dense_load<LDS_IMAGE>(img, lds_blocks, p0), k1 = pgx_dense_load<LDS_IMAGE>(img, lds_blocks, p1);
                uint32_t a0, a1, d;
                pgx_dense_pair32(k0, p0, k1, p1, cv, mrow, a0, a1, d);
                A0 = (pos_t)a0; A1 = (pos_t)a1; dB = (pos_t)d;
                fin = true;
                c_blk = s != n; c_blk2 = c_blk && (p0 >> 7) != (p1 >> 7);
            } else if (DENSE == 1) {
                // dense image: the two block addresses are known at once (pos >> 6), so both 64-byte loads are in flight
                // together and every extension is a single trip
                const uint64_t p0 = kk > n ? n : kk, p1 = (kk + s) > n ? n : (kk + s);
                const PgxDenseBlk k0 = pgx_dense_load<LDS_IMAGE>(img, lds_blocks, p0), k1 = pgx_dense_load<LDS_IMAGE>(img, lds_blocks, p1);
                uint64_t Aq0, Aq1, Bq0, Bq1;
                pgx_dense_rank(k0, p0, cv, mrow, Aq0, Bq0);
                pgx_dense_rank(k1, p1, cv, mrow, Aq1, Bq1);
                A0 = (pos_t)Aq0; A1 = (pos_t)Aq1; dB = (pos_t)(Bq1 - Bq0);
                fin = true;
                c_blk = s != n; c_blk2 = c_blk && (p0 >> 7) != (p1 >> 7);
            } else if (LDS_IMAGE) {
                // image in LDS: no memory latency to hide and most extensions of a tiny index need both blocks,
                // so both trips run back to back (measured 6 % faster than the one-trip-per-iteration form)
                uint64_t Aq0, Aq1, dq;
                pgx_rank_pair<LDS_IMAGE, false>(img, lds_blocks, lds_dir, lds_blow, kk, kk + s, cv, mrow, Aq0, Aq1, dq);
                A0 = (pos_t)Aq0; A1 = (pos_t)Aq1; dB = (pos_t)dq;
                fin = true;
            } else {
                const uint64_t p0 = kk > n ? n : kk, p1 = (kk + s) > n ? n : (kk + s);
                uint64_t Ap, Bp, As, Bs;
                bool covered;
                pgx_probe<LDS_IMAGE>(img, lds_blocks, lds_dir, lds_blow, pend ? p1 : p0, p1, !pend, cv, mrow, Ap, Bp, As, Bs, covered);
                c_blk = c_blk2 = s != n; // a directory entry and a 64-byte block per trip
                if (!pend) {
                    A0 = (pos_t)Ap; B0 = (pos_t)Bp;
                    A1 = (pos_t)As; dB = (pos_t)(Bs - Bp);
                    fin = covered;
                    pend = !covered;
                } else {
                    A1 = (pos_t)Ap; dB = (pos_t)(Bp - B0);
                    fin = true;
                    pend = false;
                }
            }
            if (fin) {
                next++;
                if (PGX_EXT_KILL(ee) || A0 >= A1) { // rank_k >= rank_ks -> bi_interval(0,0,0), src/r-index.cpp:751
                    k = 0; kp = 0; s = 0;
                } else {
                    const pos_t nk = A0 + (pos_t)s_C[PGX_EXT_V(ee)], nq = kq + dB;
                    if (NARROW) ovf |= nq < kq; // the other coordinate left 32 bits (see above)
                    s = A1 - A0;
                    k = fwd ? nq : nk;
                    kp = fwd ? nk : nq;
                }
                bool small = ((uint64_t)s < min_occ) || (s == 0); // :671 (unsigned compare) || size <= 0
                if (SEED && seed_lane) {
                    const uint32_t depth = se.w >> 24;
                    const pos_t ss = NARROW ? (pos_t)se.z : (pos_t)((uint64_t)se.z | ((uint64_t)((se.w >> 16) & 0xFFu) << 32));
                    if (ss != 0 && (uint64_t)ss >= min_occ) {
                        // all K extensions at once: sizes only shrink along a stage, so none of the K - 1 skipped ones was "small"
                        k = NARROW ? (pos_t)se.x : (pos_t)((uint64_t)se.x | ((uint64_t)(se.w & 0xFFu) << 32));
                        kp = NARROW ? (pos_t)se.y : (pos_t)((uint64_t)se.y | ((uint64_t)((se.w >> 8) & 0xFFu) << 32));
                        s = ss;
                        small = false;
                        j -= (int32_t)kuse - 1;
                        next += kuse - 1u;
                    } else if (ss == 0 && depth != PGX_SEED_UNUSABLE && min_occ <= 1) {
                        // the window leaves the index at its depth-th extension (only "empty" is small when min_occ <= 1)
                        k = 0; kp = 0; s = 0;
                        small = true;
                        j -= (int32_t)depth - 1;
                        next += depth - 1u;
                    } // otherwise (entry unusable, or min_occ decides where the stage ends): the ordinary extension stands
                }
                // The transitions of the three steps as selects (the 64 lanes of a wave are in all three steps at once, so
                // branches would run every path on every trip anyway, each with its own copies and exec-mask juggling):
                //   step 1  small -> restart at j + 1 | j == x -> J = interval, j = x + min_len, step 2 (or emit) | else j--
                //   step 2  small -> emit [x, j)      | else J = interval, j++, emit when j reaches len
                //   step 3  small -> restart at j + 1 | else j--, restart at x + 1 once j reaches x
                const bool adv = !small, p1 = ph == 1, p2 = ph == 2, at_x = j == x;
                const bool to2 = p1 && adv && at_x;
                const bool keep = adv && (to2 || p2);
                Jk = keep ? k : Jk;
                Js = keep ? s : Js;
                const int32_t jn = adv ? (p1 ? (at_x ? x + (int32_t)min_len : j - 1) : (p2 ? j + 1 : j - 1)) : j;
                const bool em = (p2 && (small || jn >= len)) || (to2 && jn >= len);
                const bool rs_small = small && !p2, rs_end = !p1 && !p2 && adv && jn <= x;
                restart = (rs_small || rs_end) ? 1u : 0u;
                x = rs_small ? j + 1 : (rs_end ? x + 1 : x);
                ph = to2 ? 2 : ph;
                j = jn;
                if (em) emit();       // x is unchanged in every emitting case
                if (restart) begin(); // next start position of this read (or the read is finished / handed on)
            }
        }
        if (!LDS_IMAGE) ln_blk += (unsigned long long)(__popcll(__ballot(c_blk)) + __popcll(__ballot(c_blk2)));
    }
    if (NARROW && __any(ovf) && lane == 0) n_ext_total[PGX_CTR_OVF32] = 1;
    // one atomic per wave for the extension counter
    unsigned long long tot = next;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_down(tot, off, 64);
    if (lane == 0 && tot) atomicAdd(n_ext_total + PGX_CTR_EXT, tot);
    if (lane == 0 && (ln_blk | ln_seed)) { atomicAdd(n_ext_total + PGX_CTR_FM_LINES, ln_blk); atomicAdd(n_ext_total + PGX_CTR_FM_SEEDS, ln_seed); }
#ifdef PGX_FM_STATS // wave trips, live lane-trips, longest wave (stats runs are made without tags)
    if (lane == 0) { atomicAdd(n_ext_total + PGX_CTR_ST_TRIPS, st_trips); atomicAdd(n_ext_total + PGX_CTR_ST_LIVE, st_live); atomicMax(n_ext_total + PGX_CTR_ST_LONGEST, st_trips); }
#endif
}

#define PGX_FM_INSTANTIATE(...)                                                                                                               \
    template __global__ void pgx_find_mems_kernel<__VA_ARGS__>(PgxDevImage, const uint8_t *, const uint64_t *, uint64_t, uint64_t, uint64_t,     \
                                                               const uint64_t *, pgx_mem *, uint32_t *, unsigned long long *, unsigned long long *, \
                                                               uint64_t, uint64_t, uint32_t, uint32_t, pgx_heavy_item *, unsigned long long *,     \
                                                               const pgx_heavy_item *, const unsigned long long *, uint32_t *, uint64_t);
PGX_FM_INSTANTIATE(false, 0, false, false)
PGX_FM_INSTANTIATE(false, 1, false, false)
PGX_FM_INSTANTIATE(true, 0, false, false)
PGX_FM_INSTANTIATE(true, 1, false, false)
PGX_FM_INSTANTIATE(true, 1, true, false)
PGX_FM_INSTANTIATE(true, 1, false, true)
PGX_FM_INSTANTIATE(true, 1, true, true)
PGX_FM_INSTANTIATE(false, 1, true, false)
PGX_FM_INSTANTIATE(false, 1, false, true)
PGX_FM_INSTANTIATE(false, 1, true, true)
PGX_FM_INSTANTIATE(false, 2, false, false)
PGX_FM_INSTANTIATE(false, 2, true, false)
PGX_FM_INSTANTIATE(false, 2, false, true)
PGX_FM_INSTANTIATE(false, 2, true, true)
PGX_FM_INSTANTIATE(false, 3, false, false)
PGX_FM_INSTANTIATE(false, 3, false, true)

// what the reads asked of the arena, for the host to size the next one: PGX_CTR_OVF_TOP = PGX_ARENA_SUBS x the fullest sub-arena's demand
__global__ void pgx_arena_demand_kernel(unsigned long long *__restrict__ ctr) {
    unsigned long long m = ctr[PGX_CTR_ARENA0 + 16u * threadIdx.x]; // (launched with PGX_ARENA_SUBS = 64 threads: one wave)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_down(m, off, 64); m = o > m ? o : m; }
    if (threadIdx.x == 0) ctr[PGX_CTR_OVF_TOP] = m * PGX_ARENA_SUBS;
}

// find_mems_function(pattern, min_len, min_occ, x) (algorithm.hpp:653-736) for ONE start position: the MEM it emits (if any), the
// start position it returns and the extensions it performs.
template <bool LDS_IMAGE>
__device__ __forceinline__ PgxHeavyResult pgx_fmf_eval(const PgxDevImage &img, const uint4 *lds_blocks, const uint64_t *lds_dir, const uint16_t *lds_blow,
                                                       const uint32_t *s_ext, const uint64_t *s_C, const uint8_t *__restrict__ pat, int32_t len, int32_t xs,
                                                       uint64_t min_len, uint64_t min_occ) {
    const uint64_t n = img.n;
    PgxHeavyResult r;
    r.mem.start = (uint64_t)xs; r.mem.end = 0; r.mem.bwt_start = 0; r.mem.size = 0;
    r.next_x = (uint32_t)len; r.n_ext = 0; r.has_mem = 0; r.pad = 0;
    if ((uint64_t)(len - xs) >= min_len) {
        uint64_t k = 0, kp = 0, s = n;
        uint32_t ne = 0;
        bool dead = false;
        for (int32_t j = xs + (int32_t)min_len - 1; j >= xs; j--) { // step 1 (:666-676)
            pgx_extend<LDS_IMAGE>(img, lds_blocks, lds_dir, lds_blow, s_ext, s_C, k, kp, s, pat[j], false);
            ne++;
            if (s < min_occ || s == 0) { r.next_x = (uint32_t)(j + 1); dead = true; break; }
        }
        if (!dead) {
            uint64_t Jk = k, Js = s;
            int32_t j = xs + (int32_t)min_len;
            for (; j < len; j++) { // step 2 (:684-696)
                pgx_extend<LDS_IMAGE>(img, lds_blocks, lds_dir, lds_blow, s_ext, s_C, k, kp, s, pat[j], true);
                ne++;
                if (s < min_occ || s == 0) break;
                Jk = k; Js = s;
            }
            r.has_mem = 1;
            r.mem.end = (uint64_t)j; r.mem.bwt_start = Jk; r.mem.size = (int64_t)Js; // :713
            k = 0; kp = 0; s = n;
            uint32_t nxt = (uint32_t)(xs + 1);
            for (; j > xs; j--) { // step 3 (:718-735); pattern[len] reads 0
                pgx_extend<LDS_IMAGE>(img, lds_blocks, lds_dir, lds_blow, s_ext, s_C, k, kp, s, j < len ? pat[j] : (uint8_t)0, false);
                ne++;
                if (s < min_occ || s == 0) { nxt = (uint32_t)(j + 1); break; }
            }
            r.next_x = nxt;
        }
        r.n_ext = ne;
    }
    return r;
}

// ------------------------------------------------------------------------------------------
// The rest of a heavy read (see pgx_find_mems_kernel): one workgroup per read evaluates find_mems_function(x)
// (algorithm.hpp:653-736) for EVERY remaining start position x at once -- the calls are independent of each other,
// only the choice of the next start is a chain -- and thread 0 then follows the chain through the stored results,
// writing the MEMs of the visited starts in order and adding only their extensions to the extension counter.  About
// twice the extensions of the sequential walk, ~300 of them on the critical path instead of ~len^2 / 2.
template <bool LDS_IMAGE>
__global__ void __launch_bounds__(256)
pgx_find_mems_heavy_kernel(PgxDevImage img, const uint8_t *__restrict__ reads, const uint64_t *__restrict__ offsets, uint64_t min_len,
                           uint64_t min_occ, const uint64_t *__restrict__ slot_off, uint64_t slot_base, pgx_mem *__restrict__ slots,
                           uint32_t *__restrict__ mem_count, unsigned long long *__restrict__ n_ext_total,
                           const pgx_heavy_item *__restrict__ heavy_list, const unsigned long long *__restrict__ heavy_count,
                           uint32_t heavy_cap, PgxHeavyResult *__restrict__ scratch, uint64_t chunk_first, uint64_t chunk_reads,
                           uint32_t *__restrict__ ovf_base, uint64_t ovf_cap) {
    unsigned long long cnt = *heavy_count;
    if (cnt == 0) return; // the usual case: nothing was handed on (uniform exit before any staging)
    if (cnt > heavy_cap) cnt = heavy_cap;
    __shared__ uint32_t s_ext[512];
    __shared__ uint64_t s_C[8];
    PGX_LDS_CARVE(img);
    pgx_stage_tables<LDS_IMAGE>(img, s_ext, s_C, lds_blocks, lds_dir, lds_blow);
    PgxHeavyResult *res = scratch + (size_t)blockIdx.x * PGX_FM_HEAVY_MAXLEN;
    for (unsigned long long h = blockIdx.x; h < cnt; h += gridDim.x) {
        const pgx_heavy_item it = heavy_list[h];
        const uint64_t base = offsets[it.rid];
        const int32_t len = (int32_t)(offsets[it.rid + 1] - base), x0 = (int32_t)it.x;
        const uint8_t *pat = reads + base;
        for (int32_t xs = x0 + (int32_t)threadIdx.x; xs < len; xs += (int32_t)blockDim.x) {
            const PgxHeavyResult r = pgx_fmf_eval<LDS_IMAGE>(img, lds_blocks, lds_dir, lds_blow, s_ext, s_C, pat, len, xs, min_len, min_occ);
            res[xs - x0] = r;
        }
        __threadfence_block();
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t nm = it.nm;
            unsigned long long ne = 0;
            int32_t x = x0;
            while (x < len && (uint64_t)(len - x) >= min_len) {
                const PgxHeavyResult r = res[x - x0];
                ne += r.n_ext;
                if (r.has_mem) {
                    const uint64_t slot = nm < PGX_FAST_SLOTS ? 0ull : pgx_slot_extent(slot_off, slot_base, ovf_base, ovf_cap, n_ext_total, it.rid, nm, len, x, min_len);
                    slots[pgx_slot_index(it.rid - chunk_first, chunk_reads, slot, nm)] = r.mem; nm++;
                }
                x = (int32_t)r.next_x;
            }
            mem_count[it.rid] = nm;
            atomicAdd(n_ext_total, ne);
        }
        __syncthreads(); // res is reused by the next item of this workgroup
    }
}
template __global__ void pgx_find_mems_heavy_kernel<false>(PgxDevImage, const uint8_t *, const uint64_t *, uint64_t, uint64_t, const uint64_t *, uint64_t,
                                                           pgx_mem *, uint32_t *, unsigned long long *, const pgx_heavy_item *,
                                                           const unsigned long long *, uint32_t, PgxHeavyResult *, uint64_t, uint64_t, uint32_t *, uint64_t);
template __global__ void pgx_find_mems_heavy_kernel<true>(PgxDevImage, const uint8_t *, const uint64_t *, uint64_t, uint64_t, const uint64_t *, uint64_t,
                                                          pgx_mem *, uint32_t *, unsigned long long *, const pgx_heavy_item *,
                                                          const unsigned long long *, uint32_t, PgxHeavyResult *, uint64_t, uint64_t, uint32_t *, uint64_t);

// find_mems_function for n independent (read, start) pairs, one lane each (the compat header's per-call entry point and the
// tests of the state machine; the batch kernel above is the product path).
__global__ void __launch_bounds__(256)
pgx_fmf_kernel(PgxDevImage img, const uint8_t *__restrict__ reads, const uint64_t *__restrict__ offsets, const uint64_t *__restrict__ read_of,
               const uint64_t *__restrict__ xs, uint64_t n, uint64_t min_len, uint64_t min_occ, PgxHeavyResult *__restrict__ out) {
    __shared__ uint32_t s_ext[512];
    __shared__ uint64_t s_C[8];
    pgx_stage_tables<false>(img, s_ext, s_C, nullptr, nullptr, nullptr);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t rid = read_of[i], base = offsets[rid];
    const int32_t len = (int32_t)(offsets[rid + 1] - base);
    PgxHeavyResult r;
    if (xs[i] > (uint64_t)len) { // undefined in the reference (len - x wraps, :658); defined here as "return len"
        r.mem.start = xs[i]; r.mem.end = 0; r.mem.bwt_start = 0; r.mem.size = 0;
        r.next_x = (uint32_t)len; r.n_ext = 0; r.has_mem = 0; r.pad = 0;
    } else {
        r = pgx_fmf_eval<false>(img, nullptr, nullptr, nullptr, s_ext, s_C, reads + base, len, (int32_t)xs[i], min_len, min_occ);
    }
    out[i] = r;
}
