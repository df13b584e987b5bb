// pgx_pairs_kernels.hip -- pgx_find_mems_pairs_kernel, the two-step find_mems kernel for gfx950 (CDNA4) over the PAIRS image: one 128-byte
// line answers both ends of an interval and up to two extensions.  The dominant kernel of every benchmark, alone in this file.
//
// All of it is 64-bit integer work bound by random access into the rank image (HBM / L2 / LDS);
// there is no floating point and nothing MFMA-shaped.  Wave width is hard-coded to 64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pgx_device.h"
#include "pgx_rank_device.h"
#include "pgx_slots_device.h"

// Tunables (each with what was measured when it was set)
#ifndef PGX_PAIRS_PACKED_WAVES
#define PGX_PAIRS_PACKED_WAVES 5 // waves per SIMD the packed narrow pairs kernel is compiled for (95 VGPRs with the inline dense2 step; 79 and six waves without it were no faster)
#endif
#ifndef PGX_LCE_WAVES
#define PGX_LCE_WAVES PGX_FM_WAVES_PER_SIMD // (the text path holds its three pieces of text across the trip's body: 110 VGPRs; bounded to 96 it spills 56 bytes per lane: scripts/r4_exp7.sh)
#endif
#ifndef PGX_LCE_ENTRY_CAP
#define PGX_LCE_ENTRY_CAP 3u // with the common-prefix table a stage through the text is ~2 trips however wide the interval: worth it from 2 x 3 symbols to go
#endif
#define PGX_PK_GROUP 12u // packed words of a read fetched per round of loads when a lane takes the read

// find_all_mems over the PAIRS image (pgx_image.h): the loop of pgx_find_mems_kernel, but a trip reads ONE 128-byte block that
// answers both ends of an interval (p1 within the block of p0; otherwise the interval runs on into the next block, which takes a
// second trip) and, where the stage has two more symbols to go, performs BOTH extensions from it.  With (c1, c2) the pair at a
// position, a the first symbol extended by and b the second:
//   first:   s1 = #{c1 = a} in [p0, p1),          k1 = C[a] + #{c1 = a} before p0,                      k' += #{c1 > a} in [p0, p1)
//   second:  s2 = #{c1 = a, c2 = b} in [p0, p1),  k2 = C[b] + #b before k1 + #{c1 = a, c2 = b} before p0,  k' += #{c1 = a, c2 > b} in [p0, p1)
//            (#b before k1 = pair_t2[a][b] + pairs (a, b) before p0: LF maps the positions with c1 = a onto [k1, k1 + s1), and BWT there is c2)
// ("> a": the regular symbols that sort after a, which is what the extension tables of such an index weight; counts that involve \n or N
// are zero in the ranges the kernel accepts.)  The first extension's result decides as in the stepwise search: if it is "small" the
// stage ends there and the second is dropped; otherwise the pair counts as two extensions, and the transitions below see the second
// one at its own j.  MEMs, restart positions and n_extensions are those of pgx_find_mems_kernel.  Positions, counts and C are below
// 2^32 (the image exists for such indexes only), so the state is 32-bit.  A stage that starts from the full interval takes its first
// extension from img.first_ext (or the seed tables): the image is never probed with the full interval.
// A lane that meets a flagged block or an interval wider than two blocks takes THAT extension through the image the PAIRS image accompanies
// (one rank probe after the other in a rolled loop, exact for every symbol) and carries on with pairs; until the end of round 3 it gave its read
// up to a list that pgx_find_mems_kernel served behind this kernel.
__device__ __forceinline__ uint32_t pgx_window_byte(uint64_t w0, uint64_t w1, uint64_t a) { // byte a of the 16-byte window
    return (uint32_t)(((a & 8ull) ? w1 : w0) >> (8u * (uint32_t)(a & 7ull))) & 0xFFu;
}
// PACKED: the seed index of the K-symbol window that starts at symbol q of this thread's LDS column: the window's 2 K bits of the packed read ARE the index
__device__ __forceinline__ uint32_t pgx_packed_seed_index(const uint32_t *s_rd, uint32_t rd_stride, uint32_t q, int32_t K) {
    const uint32_t w0 = s_rd[(q >> 4) * rd_stride + threadIdx.x], w1 = s_rd[((q >> 4) + 1u) * rd_stride + threadIdx.x]; // (one word of padding per thread)
    return (uint32_t)((((uint64_t)w1 << 32) | w0) >> (2u * (q & 15u))) & (uint32_t)((1ull << (2 * K)) - 1ull); // (K = 16: all 32 bits)
}
// WIDE: the 64-bit form (pgx_image.h "WIDE"): header counts are deltas against the bases of the block's superblock (staged in LDS), interval state,
// C and pair_t2 in 64 bits; everything else is the same kernel.
// PACKED: the reads as two bits per symbol (pgx_pack_reads_kernel: A C T G = 0 1 2 3, the order of the seed index), every lane's read copied
// into LDS when the lane takes it: the loop then reads its symbols (and whole seed windows, which ARE the seed index) from LDS instead of
// re-fetching 16-byte windows of the read bytes through L2 -- a fifth of the kernel's memory requests at chr22 scale (941 M requests per step of
// which 213 M were such windows: the ~300 k live reads do not stay in L2).  Only for launches that skip every read with a byte outside A C G T.
// COOP (needs PACKED): the wave fetches the 64 block lines of its lanes TOGETHER -- eight load instructions in which lanes 8 q .. 8 q + 7 read the
// eight 16-byte pieces of probe q's line (perfectly coalesced), through LDS -- instead of five loads per lane that each touch 64 different lines.
// For images beyond the reach of the address-translation caches (~3 GB: profiles/r03_ubench_gather_loads_per_line.txt) a random line costs one
// translation per load INSTRUCTION that touches it: 1 x 16 B of a line runs at 48 G lines/s, 5 x 16 B at 16-18 G/s, which is where the five-load
// probe sat on the 5.8 GB image of the 4.35e9-symbol index (17 G lines/s).
// S64: the image with a block every 64 positions (pgx_image.h): block b covers [64 b, 64 b + 96), so an interval of up to 32 positions
// never needs a second block; the second block of one that does overlaps the first by 32 positions and is read from position 32 on.
// LCE (needs PACKED; narrow images without COOP): the forward stage of a MEM over an interval of s <= img.lce_max occurrences is finished from the suffix array
// and the text (pgx_image.h "LCE image") instead of two symbols per line.  A trip compares what is left of the read with the text behind ONE occurrence of the
// interval (SA[k + i], three 16-byte loads from one or two lines of the 2-bit text) and then reads up to sixteen entries of img.lce_lcp, the common prefixes of
// neighbouring suffixes: occurrence t matches min(match of t - 1, lcp[k + t] - symbols matched before the stage), so an entry above the best match is one more
// occurrence of the final interval, one below it ends the stage (the matches of sorted suffixes with one pattern rise, stay, fall), one equal to it (or unknown)
// has occurrence t compared itself in the next trip.  The longest match and the occurrences that reach it -- consecutive in suffix order -- ARE what the stepwise
// extension would end with: MEM end = j + longest match, bwt_start = k + index of the first of them, size = their number; the extensions count as if made one by
// one (the failing one included).  ~1.6 trips per stage at 8 haplotypes instead of ~33.  min_occ <= 1 only (the longest match decides); a window that touches a
// line with an N or an endmarker sends the lane back to the stepwise path for that stage.  Without the table (PGX_FM_LCP=0) every occurrence is compared and only
// intervals of up to sixteen go this way.  In this variant a stage's first step (seed / first_ext entry) is applied at the top of the trip after the one in which
// the stage started (FUSE below).  Results are bit-identical (tests run all three ways).
template <bool WIDE, bool PACKED, bool COOP, bool S64, bool LCE>
__global__ void __launch_bounds__(PGX_FM_THREADS, LCE ? PGX_LCE_WAVES : ((PACKED && !WIDE && !COOP) ? PGX_PAIRS_PACKED_WAVES : PGX_FM_WAVES_PER_SIMD)) // (<= 96 VGPRs: five waves per SIMD fit and are what the launch uses; four are as fast -- 20.7 against 20.6-21.0 ms at chr22 scale --, three 21.8)
pgx_find_mems_pairs_kernel(PgxPairsArgs pa) {
    typedef typename std::conditional<WIDE, uint64_t, uint32_t>::type pos_t;
    // The arguments of the rare paths (PgxPairsArgs, third group) are read from the kernel argument segment at the point of use: a volatile scalar
    // load there -- an s_load and a wait on a path the wave seldom takes -- instead of a scalar register held across the loop.
    const volatile PgxPairsArgs __attribute__((address_space(4))) *const ka = (const volatile PgxPairsArgs __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
#define PGX_PAIRS_COLD(f) (ka->f)
    // LCE: the pointers a trip's line loads start from are made opaque here, so that they stay in scalar registers: a plain kernel argument the compiler may
    // fetch again from the argument segment inside the loop (it did: one s_load of eight dwords and a wait in front of the address of every trip's line)
    if (LCE) asm volatile("" : "+s"(pa.pairs), "+s"(pa.lce_text), "+s"(pa.lce_flags));
    const uint8_t *__restrict__ const reads = pa.reads;
    // (the first MEMs of read r of the launch: slots[nm * chunk_reads + r - first_read]; with the pointer moved back the loop needs no first_read)
    pgx_mem *__restrict__ const slots_fr = reinterpret_cast<pgx_mem *>(reinterpret_cast<uintptr_t>(pa.slots) - (uintptr_t)pa.first_read * sizeof(pgx_mem));
    uint32_t *__restrict__ const mem_count = pa.mem_count;
    const uint32_t pk_words = pa.pk_words;
    // extensions a read may spend before the rest of it is handed on; 0 = never, which is 2^32 - 1 (a read that takes part is at most
    // PGX_FM_HEAVY_MAXLEN long: all its start positions together stay far below that).  LCE: no register for it, see hmark
    const uint32_t heavy_ext = LCE ? 0u : (pa.heavy_ext ? pa.heavy_ext : 0xFFFFFFFFu);
    // (the launch serves fewer than 2^32 reads, below read number 2^32: pgx_batch_run)
    const uint32_t chunk_reads = (uint32_t)(pa.n_reads - pa.first_read);
    // min_len as 32 bits: a read is shorter than 2^31, so anything from 2^31 on means "longer than every read" like 2^31 itself
    const uint32_t min_len = pa.min_len > 0x80000000ull ? 0x80000000u : (uint32_t)pa.min_len;
    __shared__ uint32_t s_ext[512];
    __shared__ pos_t s_C[8];
    __shared__ pos_t s_t2[32];
    // first_ext: [byte] the full interval extended by byte, [256 + byte] extended by 0 and then by byte (packed like a seed entry); PACKED (every byte is
    // one of A C G T): [code] by "ACTG"[code], [4] by 0, [5 + code] by 0 and then by "ACTG"[code]
    __shared__ uint4 s_fe[PACKED ? 16 : 512];
    // FUSE: the two seed tables as a lane that starts a stage selects them, [0] the table proper and [1] the end table: {pointer lo, hi, K, extensions an entry
    // stands for (K, K + 1)} -- one LDS read where the stage starts instead of six scalar registers across the loop and the selects between them
    typedef uint32_t pgx_u32x4 __attribute__((ext_vector_type(4)));
    __shared__ pgx_u32x4 s_seedt[2];
    extern __shared__ __align__(16) unsigned char pgx_dyn_lds[];
    static_assert(!COOP || PACKED, "the cooperative loads come with the packed reads");
    static_assert(!LCE || (PACKED && !WIDE && !COOP), "the text comparison reads the packed reads and 32-bit suffix array entries");
    constexpr uint32_t SYMS = PGX_PAIRS_SYMS, STRIDE = S64 ? PGX_PAIRS_STRIDE64 : PGX_PAIRS_SYMS;
    uint32_t *s_rd = reinterpret_cast<uint32_t *>(pgx_dyn_lds); // PACKED: word w of this thread's read at s_rd[w * PGX_FM_THREADS + threadIdx.x] (pk_words words per thread)
    constexpr uint32_t rd_stride = PGX_FM_THREADS; // (the workgroup size of every launch: launch_pairs)
    // COOP: behind the packed reads, 8 KiB per wave: piece p of the line of lane q's probe at [q * 8 + (p ^ (q & 7))] (the swizzle spreads the banks)
    uint4 *s_stage = reinterpret_cast<uint4 *>(pgx_dyn_lds + (size_t)pk_words * PGX_FM_THREADS * 4) + (size_t)(threadIdx.x >> 6) * 512;
    // WIDE: behind those, per superblock the sixteen pair-count bases and their four row sums (24 words each, img.n_sbp superblocks)
    uint64_t *s_pb = reinterpret_cast<uint64_t *>(pgx_dyn_lds + (size_t)pk_words * PGX_FM_THREADS * 4 + (COOP ? (size_t)(PGX_FM_THREADS / 64) * 8192 : 0));
    // LCE (never with COOP / WIDE): behind the packed reads, what a lane has asked for at the end of a trip and uses in the next, fetched straight into LDS
    // (global_load_lds: no registers in between, nothing the compiler could copy too early): one 16-byte slot per lane -- the seed entry of a stage that starts --,
    // one dword -- the suffix array entry of the occurrence it compares with the text next --, five dwords -- sixteen entries of img.lce_lcp from any byte on
    // (dword t of lane l of wave w at s_lcp[(5 w + t) * 64 + l])
    uint4 *s_sa4 = reinterpret_cast<uint4 *>(pgx_dyn_lds + (size_t)pk_words * PGX_FM_THREADS * 4);
    uint32_t *s_sae = reinterpret_cast<uint32_t *>(s_sa4 + PGX_FM_THREADS);
    uint32_t *s_lcp = s_sae + PGX_FM_THREADS;
    for (uint32_t i = threadIdx.x; i < 512; i += PGX_FM_THREADS) s_ext[i] = pa.consts->ext_tab[i];
    if (threadIdx.x < 8) s_C[threadIdx.x] = (pos_t)pa.consts->C[threadIdx.x];
    if (threadIdx.x < 32) s_t2[threadIdx.x] = (pos_t)pa.consts->pair_t2w[threadIdx.x];
    if (WIDE) for (uint32_t i = threadIdx.x; i < pa.n_sbp * 24u; i += PGX_FM_THREADS) s_pb[i] = pa.pbase[i];
    if (PACKED) { if (threadIdx.x < 9) s_fe[threadIdx.x] = pa.first_ext[threadIdx.x == 4 ? 0u : (threadIdx.x > 4 ? 256u : 0u) + ((0x47544341u >> (8u * ((threadIdx.x > 4 ? threadIdx.x - 5u : threadIdx.x) & 3u))) & 0xFFu)]; }
    else for (uint32_t i = threadIdx.x; i < 512; i += PGX_FM_THREADS) s_fe[i] = pa.first_ext[i];
    if (LCE && threadIdx.x < 2) {
        const uint64_t tp = (uint64_t)(threadIdx.x ? pa.seed_end : pa.seed);
        const uint32_t tk = threadIdx.x ? pa.seed_end_k : pa.seed_k;
        const pgx_u32x4 te = {(uint32_t)tp, (uint32_t)(tp >> 32), tk, tk + threadIdx.x};
        s_seedt[threadIdx.x] = te;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const pos_t n = (pos_t)pa.n;
    // (LCE: launched for min_occ <= 1 only, where "small" is "empty" -- every test against mo stands next to one against 0 --: a constant, no register)
    const pos_t mo = LCE ? (pos_t)1 : WIDE ? (pos_t)pa.min_occ : (pos_t)(pa.min_occ > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)pa.min_occ); // narrow: sizes are below 2^32, a larger min_occ makes everything "small" either way
    const bool mo_huge = !LCE && !WIDE && pa.min_occ > 0xFFFFFFFFull; // (min_occ <= 1 is mo <= 1 in all forms)
    // an entry of the seed tables / first_ext: {k lo, k' lo, s lo, k hi | k' hi << 8 | s hi << 16 | depth << 24}
    auto ent_k = [](const uint4 &e) { return WIDE ? (pos_t)((uint64_t)e.x | ((uint64_t)(e.w & 0xFFu) << 32)) : (pos_t)e.x; };
    auto ent_q = [](const uint4 &e) { return WIDE ? (pos_t)((uint64_t)e.y | ((uint64_t)((e.w >> 8) & 0xFFu) << 32)) : (pos_t)e.y; };
    auto ent_s = [](const uint4 &e) { return WIDE ? (pos_t)((uint64_t)e.z | ((uint64_t)((e.w >> 16) & 0xFFu) << 32)) : (pos_t)e.z; };
    uint32_t rid = 0; // (the launch serves fewer than 2^32 reads: pgx_batch_run)
    uint64_t base = 0;
    int32_t len = 0, x = 0, j = 0;
    pos_t k = 0, kp = 0, s = 0, Jk = 0, Js = 0;
    uint32_t nm = 0, next = 0;
    // `next` when the lane took its read.  LCE: `next` at which the read will have spent heavy_ext extensions, worked out from the argument segment when the lane
    // takes the read and compared as a signed difference (never = 2^31 - 1, and so is anything above it: see heavy_ext)
    uint32_t hmark = 0;
    int ph = 0;
    uint64_t win = 0, win_hi = 0;
    uint32_t win_at = ~0u; // the cached 16 bytes of the reads buffer: their offset / 16 (16 rather than 32 bytes: four registers less, no difference in time)
    uint32_t X0 = 0; // the four sums (each <= 96: one byte) over the first block of an interval that runs on into the next
    pos_t X0e = 0, X0f = 0;                                   // ... and the two absolute ranks at its start
    uint32_t pend = 0, fresh = 0, restart = 0;
    uint32_t rnext = 0, rend = 0; // (read numbers: below 2^32)
    constexpr uint32_t EXHAUSTED = 0xFFFFFFFFu; // rnext == rend == this: the launch has no more reads (a read number only where it is the launch's last, n_reads: true then as well)
    // wave-uniform (scalar registers): block lines / seed entries the wave asked for, trips with two extensions (PGX_CTR_PAIRS_*); in 32 bits -- a trip adds
    // a few hundred at most --, added to the counters at the end of the kernel and whenever one of them has reached 2^31 (ln_flush)
    uint32_t ln_blk = 0, ln_seed = 0, ln_two = 0;
    auto ln_flush = [&]() __attribute__((always_inline)) { // (as at the end of the kernel nothing is added for a wave that has asked for no line; one line is kept back, so that the end still adds)
        if (ln_blk) {
            unsigned long long *const ctr = PGX_PAIRS_COLD(ctr);
            if ((threadIdx.x & 63u) == 0u) { atomicAdd(ctr + PGX_CTR_PAIRS_LINES, (unsigned long long)(ln_blk - 1u)); atomicAdd(ctr + PGX_CTR_PAIRS_SEEDS, (unsigned long long)ln_seed); atomicAdd(ctr + PGX_CTR_PAIRS_TWO, (unsigned long long)ln_two); }
            ln_blk = 1u; ln_seed = 0u; ln_two = 0u;
        }
    };
    uint32_t did2 = 0; // this lane's last trip performed two extensions (summed at the top of the next trip, where the wave is converged)
    // LCE: bit 0 = the lane's stage goes through the text (ph == 2), bit 1 = this stage must not (a flagged text line), bit 2 = this trip only reads on in the
    // table of common prefixes (no occurrence is compared), bits 8..15 the occurrence / entry the trip starts with, 16..23 index of the first occurrence with
    // the longest match, 24..31 how many reach it; the longest match; the text position of the occurrence compared
    uint32_t lce_st = 0, lce_best = 0, lce_pos = 0;
    // FUSE: a stage's first trip (no line of the image: the seed / first_ext entry, then the transitions) is not a trip of its own.  The entry is asked for
    // at the END of the trip in which the stage starts (`fresh` 1 -> 2 | extensions the entry stands for << 8, the entry into se_pre) and applied at the top
    // of the next one, after which the lane takes part in that trip like any other: 6.7 of a 150-symbol read's 25 lane trips were such first trips.
    constexpr bool FUSE = LCE;
    // (the entry travels through LDS -- global_load_lds into the first of the lane's five suffix array pieces, which no stage that starts is using --: kept in
    //  registers, the compiler loaded it into others than the ones it lives in across the loop's back edge and copied it over there, behind a wait for the
    //  load, which put the entry's latency back into every trip: HISTORY.md, round 4 table, row "the compiler's schedule of that kernel, read in the ISA")
    // (Two first steps per trip -- a stage that ENDS in its first step, a dead seed entry or step 3 behind a seed, starts the next one at once and applies ITS
    //  entry behind the trip's lines -- made 11 % fewer wave trips in the same time, what a trip saves in number it costs in instructions, and was taken out:
    //  HISTORY.md, round 4 table, row "two first steps per trip".)
    // (and the lines of the LCE variant are loaded in place by asm statements and waited for by hand: its two kinds of lanes load into the same registers at
    //  different points of a trip, and between them the compiler used those registers as scratch for the other kind -- after waiting for the first kind's loads,
    //  one memory latency in front of the other: the same row of HISTORY.md; scripts/isa_lint.py checks that nothing touches the registers in between)
    pgx_u32x4 row = {0u, 0u, 0u, 0u}, hs = row, d0 = row, d1 = row, d2 = row; // (whoever reads them in a trip has loaded them in that trip)
    uint32_t lce_f0 = 0u, lce_f1 = 0u; // the flag words of the lines of a lane's text window
    auto ld4 = [](const uint4 *q) __attribute__((always_inline)) { return *reinterpret_cast<const pgx_u32x4 *>(q); };
#ifdef PGX_FM_STATS
    unsigned long long st_trips = 0, st_live = 0, st_wait = 0, st_fresh = 0; // diagnostics build only (scripts/fm_stats.sh)
    unsigned long long st_t_refill = 0, st_refills = 0, st_t_seed = 0, st_t_line = 0;
    const unsigned long long st_t0 = __builtin_readcyclecounter();
#endif

    auto begin = [&]() __attribute__((always_inline)) {
        if (x >= len || (uint32_t)(len - x) < min_len) { ph = 0; mem_count[rid] = nm; return; }
        if ((LCE ? (int32_t)(next - hmark) >= 0 : next - hmark >= heavy_ext) && len <= (int32_t)PGX_FM_HEAVY_MAXLEN) {
            const unsigned long long at = atomicAdd(PGX_PAIRS_COLD(heavy_count), 1ull);
            if (at < (unsigned long long)PGX_PAIRS_COLD(heavy_cap)) {
                pgx_heavy_item it;
                it.rid = (uint64_t)rid; it.x = (uint32_t)x; it.nm = nm;
                PGX_PAIRS_COLD(heavy_list)[at] = it;
                ph = 0;
                return;
            }
        }
        k = 0; kp = 0; s = n;
        if (LCE) lce_st = 0u;
        uint32_t ml = min_len;
        asm volatile("" : "+s"(ml)); // (what follows from min_len is worked out here: held from before the loop it is a lane mask and two more scalar registers)
        if (ml == 0) { Jk = 0; Js = n; j = x; ph = 2; }
        else { j = x + (int32_t)ml - 1; ph = 1; fresh = 1u; }
    };
    // a lane on the text path asks for what its next trip reads: the suffix array entry of occurrence t (when it compares that one) and sixteen entries of the table
    // of common prefixes -- those of the occurrences behind t, or from entry t on
    // (asked where it is needed: hoisted out of the loop the answer is a 64-bit lane mask held in two scalar registers)
    auto has_lcp = [&]() __attribute__((always_inline)) { const uint8_t *q = pa.lce_lcp; asm volatile("" : "+s"(q)); return q != nullptr; };
    auto lce_ask = [&](uint32_t k32, uint32_t t, bool cmp) __attribute__((always_inline)) {
        if (cmp) __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)(pa.lce_sa + k32 + t), (void __attribute__((address_space(3))) *)(s_sae + (threadIdx.x >> 6) * 64u), 4, 0, 0);
        if (has_lcp()) {
            const uint32_t e0 = k32 + t + (cmp ? 1u : 0u), lb = e0 & ~3u;
#pragma unroll
            for (uint32_t q = 0; q < 5u; q++)
                if (q < 4u || (e0 & 3u) != 0u) // (sixteen bytes from e0 on: four dwords, five when e0 is not aligned)
                    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)(pa.lce_lcp + lb + 4u * q),
                                                     (void __attribute__((address_space(3))) *)(s_lcp + ((threadIdx.x >> 6) * 5u + q) * 64u), 4, 0, 0);
        }
    };
    auto emit = [&]() __attribute__((always_inline)) {
        pgx_mem m;
        m.start = (uint64_t)x; m.end = (uint64_t)j; m.bwt_start = (uint64_t)Jk; m.size = (int64_t)(uint64_t)Js;
        // (the worst-case offset of the read is looked up only by a fifth MEM: the first PGX_FAST_SLOTS have their own line)
        if (nm < PGX_FAST_SLOTS) slots_fr[pgx_slot_index((uint64_t)rid, (uint64_t)chunk_reads, 0ull, nm)] = m;
        else { // (everything this branch needs comes from the argument segment)
            const uint64_t fr = PGX_PAIRS_COLD(first_read), cr = PGX_PAIRS_COLD(n_reads) - fr;
            const uint64_t slot = pgx_slot_extent(PGX_PAIRS_COLD(slot_off), PGX_PAIRS_COLD(slot_base), PGX_PAIRS_COLD(ovf_base), PGX_PAIRS_COLD(ovf_cap), PGX_PAIRS_COLD(ctr), (uint64_t)rid, nm, len, x, PGX_PAIRS_COLD(min_len));
            PGX_PAIRS_COLD(slots)[pgx_slot_index((uint64_t)rid - fr, cr, slot, nm)] = m;
        }
        nm++;
        k = 0; kp = 0; s = n;
        if (LCE) lce_st = 0u;
        const bool more = j > x;
        ph = more ? 3 : ph;
        fresh = more ? 1u : fresh;
        x = more ? x : x + 1;
        restart = more ? restart : 1u;
    };

    for (;;) {
        // Wave priority: up from here until the trip's loads are out, down for the arithmetic on what they return.  The waves of a SIMD take turns
        // issuing; with equal priority they drift into step -- all computing, then all waiting -- and the memory pipeline idles in between.  A wave
        // that is about to ask for its lines now overtakes the ones that are counting bits: 17.3 -> 16.0-16.5 ms at chr22 scale
        // (profiles/r03_wave_priority.txt; the same priority for every wave, or the opposite order, is slower).
        __builtin_amdgcn_s_setprio(3);
        unsigned long long idle = __ballot(ph == 0);
        // (LCE: a read is ~28 lane trips now instead of ~73, so two or three lanes of a wave finish one in EVERY trip and a refill round -- two memory
        //  latencies in front of the trip's own -- ran in nine trips out of ten, a quarter of the waves' time: idle lanes now wait until img.refill_min of
        //  them have gathered, or until no lane of the wave is live)
        if (LCE && idle && (uint32_t)__popcll(idle) < pa.refill_min && __popcll(idle) != 64) idle = 0ull;
#ifdef PGX_FM_STATS
        const unsigned long long st_r0 = __builtin_readcyclecounter();
        if (idle) st_refills++;
#endif
        while (idle) {
            if (rnext == rend) {
                if (rnext == EXHAUSTED) break;
                unsigned long long got = 0;
                const unsigned long long n_reads = PGX_PAIRS_COLD(n_reads);
                if (lane == 0) got = PGX_PAIRS_COLD(first_read) + atomicAdd(PGX_PAIRS_COLD(cursor), 32ull);
                got = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(got >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)got);
                if (got >= n_reads) { rnext = rend = EXHAUSTED; break; }
                rnext = (uint32_t)got;
                rend = (uint32_t)(got + 32ull < n_reads ? got + 32ull : n_reads);
            }
            const uint32_t avail = rend - rnext;
            const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
            if (ph == 0 && rank < avail) {
                rid = rnext + rank;
                const uint8_t *const skip = PGX_PAIRS_COLD(skip);
                const uint64_t *const offsets = PGX_PAIRS_COLD(offsets);
                // (the three loads go out together, and so do the packed words below: a refill round is two memory latencies, not one per word --
                //  word by word, 58 % of the waves' time at chr22 scale went by in this loop: profiles/r03_refill_share.txt)
                const uint8_t *skp = skip ? skip + rid : reinterpret_cast<const uint8_t *>(offsets); // (always a load, never a branch with a wait of its own)
                const uint32_t skv = (uint32_t)*skp;
                const uint64_t o0 = offsets[rid], o1 = offsets[rid + 1];
                const uint32_t sk = skip ? skv : 0u;
                base = o0; // (assigned on both paths, so that the offsets are not fetched behind the branch on sk)
                len = (int32_t)(o1 - o0);
                if (sk) ph = -1; // served by the dense2 kernel on the other stream (pgx_classify_reads_kernel)
                else {
                    if (PACKED) { // the read's packed words into this thread's LDS column (the host sized pk_words for the longest read of the launch)
                        const uint32_t *src = PGX_PAIRS_COLD(packed) + (base >> 4);
                        const uint32_t nw = ((uint32_t)(base & 15ull) + (uint32_t)len + 15u) >> 4;
#pragma unroll 1
                        for (uint32_t w0 = 0; w0 < nw; w0 += PGX_PK_GROUP) { // (a read of 150 symbols: ten or eleven words, one group)
                            uint32_t t[PGX_PK_GROUP];
#pragma unroll
                            for (uint32_t i = 0; i < PGX_PK_GROUP; i++) t[i] = src[w0 + i < nw ? w0 + i : nw - 1u];
#pragma unroll
                            for (uint32_t i = 0; i < PGX_PK_GROUP; i++) if (w0 + i < nw) s_rd[(w0 + i) * rd_stride + threadIdx.x] = t[i];
                        }
                    }
                    x = 0; nm = 0;
                    hmark = next;
                    if (LCE) { const uint32_t hx = PGX_PAIRS_COLD(heavy_ext); hmark += hx != 0u && hx < 0x7FFFFFFFu ? hx : 0x7FFFFFFFu; }
                    begin();
                    if (ph == 0) ph = -1;
                }
            }
            const uint32_t want = (uint32_t)__popcll(idle);
            rnext += want < avail ? want : avail;
            idle = __ballot(ph == 0);
        }
#ifdef PGX_FM_STATS
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        st_t_refill += __builtin_readcyclecounter() - st_r0;
#endif
        if (ph == -1) ph = 0;
        if (!__any(ph > 0)) {
            if (rnext == EXHAUSTED) break;
            continue;
        }
#ifdef PGX_FM_STATS
        st_trips++;
        st_live += (unsigned long long)__popcll(__ballot(ph > 0));
        st_fresh += (unsigned long long)__popcll(__ballot(ph > 0 && fresh != 0u));
#endif
        // what the wave asks of the memory system in this trip (wave-uniform sums in scalar registers): a live lane fetches one block line, except in a
        // stage's first trip, which reads block 0 like every other such lane and takes its result from first_ext / the seed table
        // (seed / end table entries: one per first trip -- an upper bound: a stage with fewer than K extensions to go reads the shared entry 0)
        if (!FUSE) ln_blk += (uint32_t)__popcll(__ballot(ph > 0 && fresh == 0u));
        if ((ln_blk | ln_seed | ln_two) >> 31) ln_flush();
        ln_two += (uint32_t)__popcll(__ballot(did2 != 0u));
        did2 = 0u;
        if (!FUSE) ln_seed += (uint32_t)__popcll(__ballot(ph > 0 && fresh != 0u));
        if (COOP) { // every lane names the block it is about to probe (idle lanes: block 0, like the first trip of a stage), the wave fetches all 64 lines
            const pos_t kk_c = (ph == 2) ? kp : k;
            const uint32_t myblk = ph > 0 ? (S64 ? (uint32_t)(kk_c >> 6) : (uint32_t)(((uint64_t)(kk_c >> 5) * 0xAAAAAAABull) >> 33)) + pend : 0u;
            // (global_load_lds_dwordx4: straight into LDS, no registers for the data; lane l of instruction i lands at [64 i + l] = slot l & 7 of
            //  probe q = 8 i + (l >> 3), so the swizzle is applied to the piece it fetches)
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const uint32_t q = 8u * (uint32_t)i + ((uint32_t)lane >> 3), piece = ((uint32_t)lane & 7u) ^ (q & 7u);
                const uint32_t blk = (uint32_t)__shfl((int)myblk, (int)q, 64);
                __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)(pa.pairs + ((size_t)blk * 8 + piece)),
                                                 (void __attribute__((address_space(3))) *)(s_stage + 64 * i), 16, 0, 0);
            }
            __builtin_amdgcn_s_setprio(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
        }
        // the five 16-byte pieces a lane loads in a trip: its block's row, counts and planes -- or, for a lane that compares with the text, three pieces of the
        // text, the flag words of the lines they lie in and the next occurrence's suffix array entry (the same registers: nothing added to the trip's pressure)
        if (LCE) asm volatile("" : "=v"(row), "=v"(hs), "=v"(d0), "=v"(lce_f0), "=v"(lce_f1)); // (nothing of the last trip's lines is needed: the registers are free until here)
        const bool lce_lane = LCE && ph == 2 && (lce_st & 1u) != 0u;
        uint32_t lce_g0 = 0u;
        bool em_now = false; // this trip ends with a MEM (set by either kind of lane); `restart`: with the next start position of the read
        restart = 0u;
        if (LCE && __any(lce_lane)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (what the lanes on the text path asked for at the end of the last trip is in LDS)
#ifdef PGX_FM_STATS
        if (FUSE && __any(ph > 0 && fresh >= 2u)) {
            const unsigned long long st_s0 = __builtin_readcyclecounter();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            st_t_seed += __builtin_readcyclecounter() - st_s0;
        }
#endif
        if (FUSE && __any(ph > 0 && fresh >= 0x100u)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (the entries asked for at the end of the last trip are in LDS)
        // the first extension(s) of a stage whose seed entry has arrived: what the stage's first trip does in the other variants
        auto prestep = [&]() __attribute__((always_inline)) {
            const uint32_t kuse = fresh >> 8; // extensions the seed entry stands for (0: none was asked for)
            const uint4 se_pre = s_sa4[threadIdx.x];
            fresh = 0u;
            const bool at_end = j >= len, q1 = ph == 1;
            const uint32_t qa = (uint32_t)(base & 15ull) + (uint32_t)(at_end ? len : j);
            const uint32_t qs1 = at_end ? qa - 1u : qa, qs2 = qa ? qa - 1u : 0u;
            const uint32_t wa = s_rd[(qs1 >> 4) * rd_stride + threadIdx.x], wb = s_rd[(qs2 >> 4) * rd_stride + threadIdx.x];
            const uint4 f1 = s_fe[at_end ? 4u : ((wa >> (2u * (qs1 & 15u))) & 3u)], f2 = s_fe[5u + ((wb >> (2u * (qs2 & 15u))) & 3u)];
            const bool small1 = f1.z == 0u || f1.z < mo || mo_huge;
            const uint32_t sdepth = se_pre.w >> 24, se_s = se_pre.z;
            const bool seed_alive = kuse != 0u && se_s != 0u && se_s >= mo && !mo_huge;
            const bool seed_dead = kuse != 0u && se_s == 0u && sdepth != PGX_SEED_UNUSABLE && mo <= 1u;
            const bool rem2 = q1 ? (j - 1 >= x) : (j - 1 > x);
            const bool do2 = at_end && rem2 && !seed_alive && !seed_dead && !small1; // (by 0, then by the last symbol of the read: quirk 4)
            uint32_t ns = do2 ? f2.z : f1.z, nk = do2 ? f2.x : f1.x, nq = do2 ? f2.y : f1.y;
            if (ns == 0u) { nk = 0u; nq = 0u; }
            j -= do2 ? 1 : 0;
            next += do2 ? 2u : 1u;
            did2 = do2 ? 1u : 0u;
            s = ns; k = nk; kp = nq;
            bool small = ns == 0u || ns < mo || mo_huge;
            if (seed_alive) {
                k = se_pre.x; kp = se_pre.y; s = se_s;
                small = false;
                j -= (int32_t)kuse - 1;
                next += kuse - 1u;
            } else if (seed_dead) {
                k = 0u; kp = 0u; s = 0u;
                small = true;
                j -= (int32_t)sdepth - 1;
                next += sdepth - 1u;
            }
            const bool adv = !small, at_x = j == x;
            const bool to2 = q1 && adv && at_x;
            Jk = to2 ? k : Jk;
            Js = to2 ? s : Js;
            const int32_t jn = adv ? (q1 ? (at_x ? x + (int32_t)min_len : j - 1) : j - 1) : j;
            const bool rs_end = !q1 && adv && jn <= x;
            restart = (small || rs_end) ? 1u : 0u;
            x = small ? j + 1 : (rs_end ? x + 1 : x);
            ph = to2 ? 2 : ph;
            j = jn;
            em_now = to2 && jn >= len;
        };
        // the stages that have just started (in the refill round, by a restart or behind a MEM): their seed entries are asked for
        auto prefetch = [&]() __attribute__((always_inline)) {
            const bool ask = ph > 0 && fresh == 1u;
            bool asked = false;
            if (ask) {
                const bool endw = j >= len; // (the end table: see pgx_find_mems_kernel)
                const pgx_u32x4 tab = *(const volatile pgx_u32x4 *)&s_seedt[endw ? 1u : 0u]; // (volatile: read here, not kept in registers from before the loop)
                const int32_t K = (int32_t)tab.z;
                const int32_t avail = (ph == 1) ? (j - x + 1) : (j - x);
                uint32_t kuse = 0u;
                if (K && avail >= (int32_t)tab.w) {
                    const uint32_t sidx = pgx_packed_seed_index(s_rd, rd_stride, (uint32_t)(base & 15ull) + (uint32_t)((endw ? len - 1 : j) - K + 1), K);
                    const uint4 *sp = reinterpret_cast<const uint4 *>(((uint64_t)tab.y << 32) | tab.x) + sidx;
                    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)sp, (void __attribute__((address_space(3))) *)(s_sa4 + (threadIdx.x >> 6) * 64u), 16, 0, 0);
                    kuse = tab.w;
                    asked = true;
                }
                fresh = 2u | (kuse << 8);
            }
            ln_seed += (uint32_t)__popcll(__ballot(asked));
        };
        if (FUSE && ph > 0 && fresh >= 2u) prestep();
        const bool sit_out = FUSE && (fresh != 0u || em_now || restart != 0u); // no line of the image for this lane in this trip
        if (FUSE) ln_blk += (uint32_t)__popcll(__ballot(ph > 0 && !sit_out));
        const bool lce_cmp = lce_lane && (lce_st & 4u) == 0u; // this trip compares an occurrence with the text
        if (LCE && lce_cmp) {
            lce_pos = s_sae[threadIdx.x];
            lce_g0 = lce_pos + (uint32_t)(j - x);           // text position that faces read symbol j
            const uint32_t w0 = lce_g0 >> 4;                // its word (16 symbols); the window: words w0 .. w0 + 11
            const uint32_t *tp = pa.lce_text + w0;
            // (dword-aligned 16-byte pieces; nothing waits for them here: section C does)
            asm volatile("global_load_dwordx4 %0, %3, off\n\tglobal_load_dwordx4 %1, %3, off offset:16\n\tglobal_load_dwordx4 %2, %3, off offset:32"
                         : "+v"(row), "+v"(hs), "+v"(d0) : "v"(tp) : "memory");
            const uint32_t l0 = w0 >> 5, l1 = (w0 + 11u) >> 5; // the lines of the window
            const uint32_t *fp0 = pa.lce_flags + (l0 >> 5), *fp1 = pa.lce_flags + (l1 >> 5);
            asm volatile("global_load_dword %0, %2, off\n\tglobal_load_dword %1, %3, off" : "+v"(lce_f0), "+v"(lce_f1) : "v"(fp0), "v"(fp1) : "memory");
        }
        if (LCE) ln_blk += (uint32_t)(__popcll(__ballot(lce_cmp && ((lce_g0 >> 4) >> 5) != (((lce_g0 >> 4) + 11u) >> 5))) + // a window over two lines
                                                __popcll(__ballot(lce_cmp)) +                                                    // the line of the suffix array entry
                                                (has_lcp() ? __popcll(__ballot(lce_lane && s > 1u)) : 0)) -                      // ... and of the common prefixes
                             (uint32_t)__popcll(__ballot(lce_lane && !lce_cmp));                                        // (no text line in such a trip: counted above as one)
        if (ph > 0 && !lce_lane && !sit_out) {
            const bool fr = !FUSE && fresh != 0u; // first extension of a backward stage: from first_ext / the seed table
            bool seed_lane = false;
            uint32_t kuse = 0u; // extensions the seed entry stands for
            uint4 se = make_uint4(0u, 0u, 0u, 0u);
            if (!FUSE) {
                const uint4 *sp = pa.seed;
                if (fr) {
                    const bool endw = j >= len; // (the end table: see pgx_find_mems_kernel)
                    const int32_t K = endw ? (int32_t)pa.seed_end_k : (int32_t)pa.seed_k;
                    const int32_t avail = (ph == 1) ? (j - x + 1) : (j - x);
                    if (K && avail >= K + (endw ? 1 : 0)) {
                        if (PACKED) {
                            const uint32_t sidx = pgx_packed_seed_index(s_rd, rd_stride, (uint32_t)(base & 15ull) + (uint32_t)((endw ? len - 1 : j) - K + 1), K);
                            seed_lane = true; sp = (endw ? pa.seed_end : pa.seed) + sidx; kuse = (uint32_t)K + (endw ? 1u : 0u);
                        } else {
                        const uint64_t a = base + (uint64_t)((endw ? len - 1 : j) - K + 1);
                        const uint32_t sh = (uint32_t)(a & 7ull) * 8u;
                        const uint64_t *wp = reinterpret_cast<const uint64_t *>(reads + (a & ~7ull));
                        const uint64_t w0 = wp[0], w1 = wp[1], w2 = wp[2];
                        const uint64_t lo = sh ? (w0 >> sh) | (w1 << (64u - sh)) : w0, hi = sh ? (w1 >> sh) | (w2 << (64u - sh)) : w1;
                        uint32_t sidx;
                        if (pgx_seed_index(lo, hi, (uint32_t)K, sidx)) { seed_lane = true; sp = (endw ? pa.seed_end : pa.seed) + sidx; kuse = (uint32_t)K + (endw ? 1u : 0u); }
                        }
                    }
                }
#ifdef PGX_FM_STATS
                const unsigned long long st_s0 = __builtin_readcyclecounter();
#endif
                se = *sp;
#ifdef PGX_FM_STATS
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                st_t_seed += __builtin_readcyclecounter() - st_s0;
#endif
            }
            if (!FUSE) fresh = 0u;
            const bool fwd = (ph == 2);
            const uint64_t at = base + (uint64_t)j;
            // pattern[len] reads as 0 (quirk 4): step 3 of a MEM that reaches the end of its read starts there, from the full interval;
            // its first TWO extensions (by 0, then by the last symbol of the read) come from first_ext: the rows of the endmarkers
            // (block 0 of the image) have the sequences' last symbols before them, often N
            const bool at_end = j >= len;
            uint32_t byte, byte2;
            bool have2;
            if (PACKED) { // both symbols from the packed read in LDS ("ACTG"[code]); the second one is always at hand
                const uint32_t qa = (uint32_t)(base & 15ull) + (uint32_t)(at_end ? len : j);
                const uint32_t q1 = at_end ? qa - 1u : qa, q2 = (fwd && !at_end) ? qa + 1u : (qa ? qa - 1u : 0u); // (q2 is meaningless where the stage has no second symbol: rem2)
                const uint32_t wa = s_rd[(q1 >> 4) * rd_stride + threadIdx.x], wb = s_rd[(q2 >> 4) * rd_stride + threadIdx.x];
                byte = at_end ? 0u : ((0x47544341u >> (8u * ((wa >> (2u * (q1 & 15u))) & 3u))) & 0xFFu);
                byte2 = (0x47544341u >> (8u * ((wb >> (2u * (q2 & 15u))) & 3u))) & 0xFFu;
                have2 = true;
            } else {
            const uint64_t atw = at_end ? at - 1ull : at; // (a live read has len >= 1)
            if ((uint32_t)(atw >> 4) != win_at) {
                win_at = (uint32_t)(atw >> 4);
                const ulonglong2 w2 = *reinterpret_cast<const ulonglong2 *>(reads + (atw & ~15ull));
                win = w2.x; win_hi = w2.y;
            }
            // (a function of values: as a lambda capturing the window by reference it turned into loads through a selected address,
            //  with the window in scratch memory)
            byte = at_end ? 0u : pgx_window_byte(win, win_hi, at);
            // the symbol after this one in the direction of the stage, when the cached window holds it
            const uint64_t at2 = (fwd && !at_end) ? at + 1ull : at - 1ull;
            have2 = (uint32_t)(at2 >> 4) == win_at;
            byte2 = pgx_window_byte(win, win_hi, at2);
            }
            const uint32_t e1 = s_ext[(fwd ? 256u : 0u) + byte], e2 = s_ext[(fwd ? 256u : 0u) + byte2];
            const uint32_t cv1 = PGX_EXT_CV(e1), cv2 = PGX_EXT_CV(e2);
            const bool reg1 = !PGX_EXT_KILL(e1) && ((0x2Eu >> cv1) & 1u), reg2 = !PGX_EXT_KILL(e2) && ((0x2Eu >> cv2) & 1u); // A C G T
            const uint32_t t1 = reg1 ? cv1 - 1u - (cv1 >> 2) : 0u, t2 = reg2 ? cv2 - 1u - (cv2 >> 2) : 0u;                    // their 2-bit codes
            const bool rem2 = ph == 1 ? (j - 1 >= x) : (fwd ? (j + 1 < len) : (j - 1 > x)); // the stage has a second extension to make
            const bool two = !fr && rem2 && have2 && reg1 && reg2;
            const pos_t kk = fwd ? kp : k, kq = fwd ? k : kp;
            const pos_t p0 = kk, p1 = kk + s;
            // the block of p0 (96 positions); a second trip (pend) reads the block after it
            const uint32_t bfirst = S64 ? (uint32_t)(p0 >> 6) : (uint32_t)(((uint64_t)(p0 >> 5) * 0xAAAAAAABull) >> 33); // p0 / 96 (p0 < 2^37)
            const pos_t endrel_p = p1 - (pos_t)bfirst * STRIDE;                               // p1 relative to the first block
            const uint32_t endrel = endrel_p > (pos_t)0xFFFFu ? 0xFFFFu : (uint32_t)endrel_p; // (anything beyond two blocks is "far")
            // the second block starts STRIDE positions after the first and the first has answered up to its position SYMS
            const uint32_t relA = pend ? SYMS - STRIDE : p0 - bfirst * STRIDE;
            const uint32_t relB = pend ? endrel - STRIDE : (endrel < SYMS ? endrel : SYMS);
            if (COOP) { // the line of this lane's probe is in LDS (fetched by the whole wave above)
                const uint4 *mine = s_stage + (uint32_t)lane * 8u;
                const uint32_t sw = (uint32_t)lane & 7u;
                row = ld4(mine + (t1 ^ sw)); hs = ld4(mine + (4u ^ sw)); d0 = ld4(mine + (5u ^ sw)); d1 = ld4(mine + (6u ^ sw)); d2 = ld4(mine + (7u ^ sw));
            } else {
#ifdef PGX_FM_STATS
                const unsigned long long st_l0 = __builtin_readcyclecounter();
#endif
                const uint4 *bp = pa.pairs + (size_t)(bfirst + pend) * 8;
                // row: pairs (t1, A C G T) before the block; hs: positions before the block with c2 special and c1 = A, C, G, T; bit 31 of .x: flag;
                // d0 d1 d2: the planes: c1 bit 0, c1 bit 1, c2 bit 0, c2 bit 1, three dwords each
                if (LCE) { // (in place, and waited for by hand below: see the declaration of row)
                    const uint4 *rp = bp + t1;
                    asm volatile("global_load_dwordx4 %0, %3, off\n\tglobal_load_dwordx4 %1, %4, off offset:64\n\tglobal_load_dwordx4 %2, %4, off offset:80"
                                 : "+v"(row), "+v"(hs), "+v"(d0) : "v"(rp), "v"(bp) : "memory");
                    d1 = ld4(bp + 6); d2 = ld4(bp + 7); // (only this kind of lane uses these two)
                } else {
                    row = ld4(bp + t1); hs = ld4(bp + 4); d0 = ld4(bp + 5); d1 = ld4(bp + 6); d2 = ld4(bp + 7);
                }
                __builtin_amdgcn_s_setprio(0);
#ifdef PGX_FM_STATS
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(row), "+v"(hs), "+v"(d0), "+v"(d1), "+v"(d2) :: "memory");
                st_t_line += __builtin_readcyclecounter() - st_l0;
#endif
            }
            // masks that turn "code == t" / "code > t" into plane expressions: (x ^ i0) & (y ^ i1) and (y & ua) | (x & (y | va) & wa)
            const uint32_t i0 = (t1 & 1u) ? 0u : 0xFFFFFFFFu, i1 = (t1 & 2u) ? 0u : 0xFFFFFFFFu, j0 = (t2 & 1u) ? 0u : 0xFFFFFFFFu, j1 = (t2 & 2u) ? 0u : 0xFFFFFFFFu;
            const uint32_t ua = t1 < 2u ? 0xFFFFFFFFu : 0u, va = t1 == 0u ? 0xFFFFFFFFu : 0u, wa = (t1 & 1u) ? 0u : 0xFFFFFFFFu;
            const uint32_t ub = t2 < 2u ? 0xFFFFFFFFu : 0u, vb = t2 == 0u ? 0xFFFFFFFFu : 0u, wb = (t2 & 1u) ? 0u : 0xFFFFFFFFu;
            if (LCE && !COOP) asm volatile("s_waitcnt vmcnt(0)" : "+v"(row), "+v"(hs), "+v"(d0) :: "memory"); // (behind what does not need the line)
            const bool flagged = (hs.x >> 31) != 0u;
            const uint32_t pts = (t1 == 0u ? hs.x : (t1 == 1u ? hs.y : (t1 == 2u ? hs.z : hs.w))) & 0x00FFFFFFu; // (24-bit counts: pgx_image.h)
            const uint32_t PX[3] = {d0.x, d0.y, d0.z}, PY[3] = {d0.w, d1.x, d1.y}, PU[3] = {d1.z, d1.w, d2.x}, PV[3] = {d2.y, d2.z, d2.w};
            // counts below relA (absolute ranks need them) and in [relA, relB) (sizes and the other coordinate are differences)
            uint32_t e1p = 0, e2p = 0, e1r = 0, g1r = 0, e2r = 0, g2r = 0;
#pragma unroll
            for (int h = 0; h < 3; h++) {
                const int32_t ta = (int32_t)relA - 32 * h, tb = (int32_t)relB - 32 * h;
                const uint32_t mP = ta >= 32 ? 0xFFFFFFFFu : (ta > 0 ? ((1u << ta) - 1u) : 0u);
                const uint32_t mR = (tb >= 32 ? 0xFFFFFFFFu : (tb > 0 ? ((1u << tb) - 1u) : 0u)) & ~mP;
                const uint32_t x = PX[h], y = PY[h], u = PU[h], v = PV[h];
                const uint32_t m1 = (x ^ i0) & (y ^ i1);             // first symbol == the one extended by
                const uint32_t g1 = (y & ua) | (x & (y | va) & wa);   // first symbol sorts after it
                const uint32_t q2 = m1 & (u ^ j0) & (v ^ j1);         // ... and second symbol == the second one extended by
                const uint32_t g2 = m1 & ((v & ub) | (u & (v | vb) & wb)); // ... and second symbol sorts after it
                e1p += __popc(m1 & mP); e2p += __popc(q2 & mP);
                e1r += __popc(m1 & mR); g1r += __popc(g1 & mR); e2r += __popc(q2 & mR); g2r += __popc(g2 & mR);
            }
            pos_t a01 = (pos_t)(row.x + row.y + row.z + row.w + pts + e1p);                       // rank of the first symbol at p0
            pos_t a02 = (pos_t)((t2 == 0u ? row.x : (t2 == 1u ? row.y : (t2 == 2u ? row.z : row.w))) + e2p); // rank of the pair at p0
            if (WIDE) { // the counts of a block are deltas against its superblock
                const uint64_t *pb = s_pb + (size_t)((bfirst + pend) >> pa.pairs_sb_shift) * 24u;
                a01 += (pos_t)pb[16u + t1];
                a02 += (pos_t)pb[4u * t1 + t2];
            }
            const bool straddle = endrel > SYMS, far = endrel > STRIDE + SYMS;
            // Run continuation (pgx_image.h): the pair of the block's last position goes on for hs.y >> 24 positions behind the block, its first symbol
            // alone for hs.z >> 24.  An interval that ends inside that stretch is answered from THIS line -- both extensions, or the first one --: the
            // positions behind the block all count like the last one.  (Intervals are ~#haplotypes wide and mostly one run: with 96 haplotypes 44 % of
            // the lane trips fetched a second block before, profiles/r04_haps_sweep.txt.)
            const uint32_t over = endrel - SYMS; // (meaningful where straddle)
            const bool cont2 = !pend && straddle && over <= (hs.y >> 24), cont1 = !pend && straddle && !cont2 && over <= (hs.z >> 24);
            const bool cont = cont1 || cont2;
            if (cont) {
                const uint32_t l1 = (PX[2] >> 31) | ((PY[2] >> 31) << 1), l2 = (PU[2] >> 31) | ((PV[2] >> 31) << 1); // the pair at position 95
                e1r += l1 == t1 ? over : 0u;
                g1r += l1 > t1 ? over : 0u;
                e2r += (cont2 && l1 == t1 && l2 == t2) ? over : 0u;
                g2r += (cont2 && l1 == t1 && l2 > t2) ? over : 0u;
            }
            const bool bail = !fr && (flagged || (far && !cont)); // (a second block is used only when it is not flagged either: nothing special between the two ends)
            const bool wait = !fr && !pend && straddle && !bail && !cont; // the interval runs on into the next block: next trip
#ifdef PGX_FM_STATS
            st_wait += wait ? 1ull : 0ull;
#endif
            if (wait) {
                X0 = e1r | (g1r << 8) | (e2r << 16) | (g2r << 24); X0e = a01; X0f = a02;
                pend = 1u;
            } else {
                const uint32_t Xp = pend ? X0 : 0u;
                const uint32_t c1 = (Xp & 0xFFu) + e1r, w1 = ((Xp >> 8) & 0xFFu) + g1r, c2 = ((Xp >> 16) & 0xFFu) + e2r, w2 = (Xp >> 24) + g2r;
                const pos_t r1 = pend ? X0e : a01, r2 = pend ? X0f : a02;
                pend = 0u;
                // first extension (src/r-index.cpp:713-764); a symbol that is not A C G T has no occurrence in a range free of special positions
                pos_t s1 = reg1 ? (pos_t)c1 : (pos_t)0;
                pos_t k1 = r1 + s_C[PGX_EXT_V(e1)], q1v = kq + (pos_t)w1;
                if (bail) { // special positions in the way (or an interval wider than two blocks): THIS extension alone through the dense2 image the
                    // PAIRS image accompanies (two more lines, exact for every symbol), then on with pairs.  (Until round 3 the read went to a list
                    // and pgx_find_mems_kernel searched the rest of it behind this kernel: 0.8 ms of a 20 ms step for 0.1 % of the reads.)
                    // (one probe after the other in a rolled loop: this path is rare and must not cost the common one its registers)
                    const uint64_t q0 = (uint64_t)p0 > (uint64_t)n ? (uint64_t)n : (uint64_t)p0, q1 = (uint64_t)p1 > (uint64_t)n ? (uint64_t)n : (uint64_t)p1;
                    uint64_t A0 = 0, A1 = 0, B0 = 0, B1 = 0;
                    PgxDevImage img = {}; // what the rank functions read of it
                    img.blocks = PGX_PAIRS_COLD(blocks); img.exc = PGX_PAIRS_COLD(exc); img.sbase2 = PGX_PAIRS_COLD(sbase2); img.d2_sb_shift = PGX_PAIRS_COLD(d2_sb_shift);
#pragma unroll 1
                    for (int it = 0; it < 2; it++) {
                        const uint64_t q = it ? q1 : q0;
                        uint64_t a, bq;
                        if (WIDE) pgx_dense2w_rank(img, q, PGX_EXT_CV(e1), PGX_EXT_M(e1), a, bq);
                        else if (pa.dense == 1) { // (a small index: the 64-byte dense image)
                            const PgxDenseBlk db = pgx_dense_load<false>(img, nullptr, q);
                            pgx_dense_rank(db, q, PGX_EXT_CV(e1), PGX_EXT_M(e1), a, bq);
                        } else pgx_dense2_rank(img, (uint32_t)q, PGX_EXT_CV(e1), PGX_EXT_M(e1), a, bq);
                        A1 = a; B1 = bq;
                        if (!it) { A0 = a; B0 = bq; }
                    }
                    const uint64_t dB = B1 - B0;
                    { // (rare, and inside diverged control flow: counted with one atomic by the first lane that is here, not in the wave-uniform sums)
                        const unsigned long long here = __ballot(true);
                        if (lane == (int)__ffsll((long long)here) - 1) {
                            atomicAdd(PGX_PAIRS_COLD(ctr) + PGX_CTR_REDO, (unsigned long long)__popcll(here));
                            atomicAdd(PGX_PAIRS_COLD(ctr) + PGX_CTR_PAIRS_LINES, 2ull * (unsigned long long)__popcll(here)); // the two lines of the other image
                        }
                    }
                    const bool none = PGX_EXT_KILL(e1) || A0 >= A1; // rank_k >= rank_ks -> bi_interval(0,0,0), src/r-index.cpp:751
                    s1 = none ? (pos_t)0 : (pos_t)(A1 - A0);
                    k1 = (pos_t)A0 + s_C[PGX_EXT_V(e1)];
                    q1v = kq + (pos_t)dB;
                }
                if (fr) { const uint4 f = s_fe[PACKED ? (at_end ? 4u : ((byte >> 1) & 3u)) : byte]; k1 = ent_k(f); q1v = ent_q(f); s1 = ent_s(f); }
                const bool small1 = s1 == 0u || s1 < mo || mo_huge;
                // a usable seed entry stands for the first extension and the ones after it
                const uint32_t sdepth = se.w >> 24;
                const pos_t se_s = ent_s(se);
                const bool seed_alive = seed_lane && se_s != 0u && se_s >= mo && !mo_huge;
                const bool seed_dead = seed_lane && se_s == 0u && sdepth != PGX_SEED_UNUSABLE && mo <= 1u;
                const bool do2 = (fr ? (at_end && rem2 && have2 && !seed_alive && !seed_dead) : (two && !bail && !cont1)) && !small1;
                pos_t s2 = (pos_t)c2, k2 = r2 + s_C[PGX_EXT_V(e2)] + s_t2[8u * t1 + cv2], q2v = q1v + (pos_t)w2;
                if (fr) { const uint4 f = s_fe[PACKED ? 5u + ((byte2 >> 1) & 3u) : 256u + byte2]; k2 = ent_k(f); q2v = ent_q(f); s2 = ent_s(f); }
                pos_t ns = do2 ? s2 : s1, nk = do2 ? k2 : k1, nq = do2 ? q2v : q1v;
                if (ns == 0u) { nk = 0u; nq = 0u; }
                if (do2) { // the first of the two: what a trip of its own would have left behind
                    Jk = fwd ? q1v : Jk;
                    Js = fwd ? s1 : Js;
                    j = fwd ? j + 1 : j - 1;
                }
                next += do2 ? 2u : 1u;
                did2 = do2 ? 1u : 0u;
                s = ns;
                k = fwd ? nq : nk;
                kp = fwd ? nk : nq;
                bool small = ns == 0u || ns < mo || mo_huge;
                if (seed_alive) { // all its extensions at once: sizes only shrink along a stage, so none of the skipped ones was "small"
                    k = ent_k(se); kp = ent_q(se); s = se_s;
                    small = false;
                    j -= (int32_t)kuse - 1;
                    next += kuse - 1u;
                } else if (seed_dead) { // the window leaves the index at its depth-th extension
                    k = 0u; kp = 0u; s = 0u;
                    small = true;
                    j -= (int32_t)sdepth - 1;
                    next += sdepth - 1u;
                }
                const bool adv = !small, q1 = ph == 1, q2 = ph == 2, at_x = j == x;
                const bool to2 = q1 && adv && at_x;
                const bool keep = adv && (to2 || q2);
                Jk = keep ? k : Jk;
                Js = keep ? s : Js;
                const int32_t jn = adv ? (q1 ? (at_x ? x + (int32_t)min_len : j - 1) : (q2 ? j + 1 : j - 1)) : j;
                const bool em = (q2 && (small || jn >= len)) || (to2 && jn >= len);
                const bool rs_small = small && !q2, rs_end = !q1 && !q2 && adv && jn <= x;
                restart = (rs_small || rs_end) ? 1u : 0u;
                x = rs_small ? j + 1 : (rs_end ? x + 1 : x);
                ph = to2 ? 2 : ph;
                j = jn;
                em_now = em;
                // a forward stage over a narrow interval goes on through the text: from the next trip on one occurrence per trip (its first suffix array entry
                // is asked for now); only where that is fewer trips than two symbols per trip, and where the window of three pieces holds what is left
                if (LCE && ph == 2 && !em && !restart && !(lce_st & 2u) && s >= 1u && (uint32_t)s <= pa.lce_max && mo <= 1u && j < len &&
                    (uint32_t)(len - j) >= 2u * (has_lcp() && (uint32_t)s > PGX_LCE_ENTRY_CAP ? PGX_LCE_ENTRY_CAP : (uint32_t)s) && (uint32_t)(len - j) <= 144u &&
                    ((uint32_t)s <= 16u || (has_lcp() && (uint32_t)(len - x) <= PGX_LCP_CAP - 1u))) { // (wider than sixteen only where the table of common prefixes can be used)
                    lce_st = 1u;
                    lce_best = 0u;
                    lce_ask((uint32_t)k, 0u, true); // SA[k] and the common prefixes of the sixteen entries behind it
                }
            }
        }
        if (LCE) asm volatile("s_waitcnt vmcnt(0)" : "+v"(row), "+v"(hs), "+v"(d0), "+v"(lce_f0), "+v"(lce_f1) :: "memory"); // (the whole wave: the text of section A is in)
        if (LCE && lce_lane) { // the text behind occurrence i of the interval against the read from symbol j on, then sixteen entries of the table
            const uint32_t rem = (uint32_t)(len - j), i = (lce_st >> 8) & 0xFFu;
            uint32_t a = (lce_st >> 16) & 0xFFu, cnt = lce_st >> 24, t0 = i;
            bool fin = false, banned = false;
            if (lce_cmp) {
                const uint32_t T[12] = {row.x, row.y, row.z, row.w, hs.x, hs.y, hs.z, hs.w, d0.x, d0.y, d0.z, d0.w};
                const uint32_t fl0 = lce_g0 >> 9, fl1 = ((lce_g0 >> 4) + 11u) >> 5; // the lines of the window (section A)
                banned = (((lce_f0 >> (fl0 & 31u)) | (lce_f1 >> (fl1 & 31u))) & 1u) != 0u; // a line with an N / an endmarker / behind the text: this stage goes on stepwise (nothing has changed yet)
                const uint32_t q0 = (uint32_t)(base & 15ull) + (uint32_t)j;
                const uint32_t tsh = 2u * (lce_g0 & 15u), rsh = 2u * (q0 & 15u), rw0 = q0 >> 4;
                uint32_t R[10];
#pragma unroll
                for (uint32_t u = 0; u < 10; u++) { const uint32_t wi = rw0 + u; R[u] = s_rd[(wi < pk_words ? wi : pk_words - 1u) * rd_stride + threadIdx.x]; }
                uint32_t l = 144u;
#pragma unroll
                for (int u = 8; u >= 0; u--) { // (from the last unit down: the first differing one wins)
                    const uint32_t df = __builtin_amdgcn_alignbit(R[u + 1], R[u], rsh) ^ __builtin_amdgcn_alignbit(T[u + 1], T[u], tsh);
                    l = df ? 16u * (uint32_t)u + ((uint32_t)__builtin_ctz(df) >> 1) : l;
                }
                l = l < rem ? l : rem;
                // (the matches of one pattern with suffixes in sorted order rise, stay, fall and never rise again: one below the best ends the stage)
                const bool better = i == 0u || l > lce_best;
                fin = !better && l < lce_best;
                cnt = better ? 1u : (l == lce_best ? cnt + 1u : cnt);
                a = better ? i : a;
                lce_best = better ? l : lce_best;
                t0 = i + 1u;
            }
            if (banned) lce_st = 2u;
            else {
                // The occurrences behind, from the common prefixes of neighbouring suffixes: with c symbols shared between occurrence t - 1 and t, occurrence t matches
                // min(match of t - 1, c - m) symbols (m = the symbols matched before the stage).  Here the match of t - 1 is the best one (anything shorter has ended the
                // stage): an entry above it (or at it, once the read is used up) is one more occurrence of the final interval; one below it ends the stage; one AT it --
                // occurrence t may match further -- or an unknown one is compared with the text itself in the next trip.  Sixteen entries per trip.
                uint32_t tt = t0; // the entry the next trip starts with
                bool cmp_next = true;
                if (!fin && tt < (uint32_t)s && has_lcp() && (uint32_t)(len - x) <= PGX_LCP_CAP - 1u) { // (m + what is left of the read stays below the cap: a capped entry is "longer than anything asked")
                    const uint32_t m = (uint32_t)(j - x), bsh = ((uint32_t)k + t0) & 3u;
                    uint32_t L5[5];
#pragma unroll
                    for (uint32_t t = 0; t < 5u; t++) L5[t] = s_lcp[((threadIdx.x >> 6) * 5u + t) * 64u + (uint32_t)lane];
                    const uint32_t W[4] = {__builtin_amdgcn_alignbyte(L5[1], L5[0], bsh), __builtin_amdgcn_alignbyte(L5[2], L5[1], bsh), __builtin_amdgcn_alignbyte(L5[3], L5[2], bsh),
                                           __builtin_amdgcn_alignbyte(L5[4], L5[3], bsh)};
                    bool stop = false;
                    cmp_next = false;
#pragma unroll
                    for (uint32_t u = 0; u < 16u; u++) {
                        if ((u & 3u) == 0u && u > 0u && !__any(!stop && t0 + u < (uint32_t)s)) break; // (four at a time)
                        const uint32_t c = (W[u >> 2] >> (8u * (u & 3u))) & 0xFFu, rel = c - m;
                        const bool act = !stop && t0 + u < (uint32_t)s;
                        const bool hard = c == PGX_LCP_UNKNOWN || c < m || (rel == lce_best && lce_best < rem);
                        const bool drop = !hard && rel < lce_best;
                        cmp_next = cmp_next || (act && hard);
                        fin = fin || (act && drop);
                        stop = stop || (act && (hard || drop));
                        if (act && !hard && !drop) { cnt++; tt = t0 + u + 1u; }
                    }
                }
                if (!fin && tt < (uint32_t)s) { // on with occurrence / entry tt
                    lce_st = 1u | (cmp_next ? 0u : 4u) | (tt << 8) | (a << 16) | (cnt << 24);
                    lce_ask((uint32_t)k, tt, cmp_next);
                } else { // the MEM ends where the longest match ends; the occurrences that reach it are its interval
                    Jk = k + (pos_t)a; Js = (pos_t)cnt;
                    next += lce_best + (lce_best < rem ? 1u : 0u); // (the extension that fails counts, as in the stepwise stage)
                    j += (int32_t)lce_best;
                    lce_st = 0u;
                    em_now = true;
                }
            }
        }
        if (em_now) emit();
        if (restart) begin();
        if (FUSE) prefetch(); // (their seed entries are on the way while the wave loops)
    }
    unsigned long long *const n_ext_total = PGX_PAIRS_COLD(ctr);
    unsigned long long tot = next;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_down(tot, off, 64);
    if (lane == 0 && tot) atomicAdd(n_ext_total + PGX_CTR_EXT, tot);
    ln_two += (uint32_t)__popcll(__ballot(did2 != 0u));
    if (lane == 0 && ln_blk) { atomicAdd(n_ext_total + PGX_CTR_PAIRS_LINES, (unsigned long long)ln_blk); atomicAdd(n_ext_total + PGX_CTR_PAIRS_SEEDS, (unsigned long long)ln_seed); atomicAdd(n_ext_total + PGX_CTR_PAIRS_TWO, (unsigned long long)ln_two); }
#ifdef PGX_FM_STATS // wave trips / live lane-trips, lane-trips waiting for the second block / fresh
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) st_wait += __shfl_down(st_wait, off, 64);
    if (lane == 0) { atomicAdd(n_ext_total + PGX_CTR_ST_PAIR_T_REFILL, st_t_refill); atomicAdd(n_ext_total + PGX_CTR_ST_PAIR_T_TOTAL, __builtin_readcyclecounter() - st_t0); atomicAdd(n_ext_total + PGX_CTR_ST_PAIR_REFILLS, st_refills);
                     atomicAdd(n_ext_total + PGX_CTR_ST_PAIR_T_SEED, st_t_seed); atomicAdd(n_ext_total + PGX_CTR_ST_PAIR_T_LINE, st_t_line); }
    if (lane == 0) { atomicAdd(n_ext_total + PGX_CTR_ST_PAIR_TRIPS, st_trips); atomicAdd(n_ext_total + PGX_CTR_ST_PAIR_LIVE, st_live); atomicAdd(n_ext_total + PGX_CTR_ST_PAIR_WAIT, st_wait); atomicAdd(n_ext_total + PGX_CTR_ST_PAIR_FRESH, st_fresh); }
#endif
}
#define PGX_PAIRS_INSTANTIATE(...) \
    template __global__ void pgx_find_mems_pairs_kernel<__VA_ARGS__>(PgxPairsArgs);
PGX_PAIRS_INSTANTIATE(false, false, false, false, false)
PGX_PAIRS_INSTANTIATE(true, false, false, false, false)
PGX_PAIRS_INSTANTIATE(false, true, false, false, false)
PGX_PAIRS_INSTANTIATE(true, true, false, false, false)
PGX_PAIRS_INSTANTIATE(false, true, true, false, false)
PGX_PAIRS_INSTANTIATE(true, true, true, false, false)
PGX_PAIRS_INSTANTIATE(false, false, false, true, false)
PGX_PAIRS_INSTANTIATE(true, false, false, true, false)
PGX_PAIRS_INSTANTIATE(false, true, false, true, false)
PGX_PAIRS_INSTANTIATE(true, true, false, true, false)
PGX_PAIRS_INSTANTIATE(false, true, true, true, false)
PGX_PAIRS_INSTANTIATE(true, true, true, true, false)
PGX_PAIRS_INSTANTIATE(false, true, false, false, true)
PGX_PAIRS_INSTANTIATE(false, true, false, true, true)
