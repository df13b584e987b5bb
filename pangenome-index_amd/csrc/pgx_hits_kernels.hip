// pgx_hits_kernels.hip -- read hits (include/pgx.h "read hits"): the MEMs and sequence sets of every read reduced to one pgx_read_hit,
// optionally the bitmap of best sequences and the score row.  One launch over the reads, no atomics, no LDS, nothing shared between
// workgroups.
//
// Lane = sequence within a 64-bit word column.  A read gets Sp lanes (Sp = the power of two >= min(n_seq, 64)), a wave 64 / Sp reads;
// with more than 64 sequences (WIDE) a wave serves one read and goes through its W word columns one after the other.  Every lane
// keeps two numbers for its sequence, cov and reach, and walks the MEMs of the read in order:
//     cov += max(0, end - max(start, reach)) ; reach = max(reach, end)             for the MEMs whose set has the lane's bit
// which counts every read position once because starts ascend within a read (ends need not).  The MEM record and its set word are the
// same address for all lanes of a read: one request a MEM.  Registers do not depend on the number of MEMs.
#include "pgx_device.h"

namespace {

// max over the Sp lanes of a read (Sp a power of two <= 64; all 64 lanes of the wave take part)
__device__ __forceinline__ unsigned long long hits_group_max(unsigned long long v, uint32_t Sp) {
    for (uint32_t d = 1; d < Sp; d <<= 1) {
        const unsigned long long o = __shfl_xor(v, (int)d, 64);
        v = o > v ? o : v;
    }
    return v;
}

struct HitsSweep { // one sequence's state over the MEMs of a read
    unsigned long long cov = 0, reach = 0;
    __device__ __forceinline__ void add(unsigned long long start, unsigned long long end) {
        const unsigned long long from = start > reach ? start : reach;
        cov += end > from ? end - from : 0;
        reach = end > reach ? end : reach;
    }
};

struct HitsSummary { // best, ties, first tie and runner-up over the columns seen so far
    unsigned long long best = 0, next = 0;
    uint32_t n_best = 0, first = PGX_NO_SEQUENCE;
    // column `col` has maximum colmax on the lanes of `ties` (lanes of valid sequences only) and runner-up nxt (< colmax, 0 if none)
    __device__ __forceinline__ void merge(uint32_t col, unsigned long long colmax, unsigned long long ties, unsigned long long nxt) {
        const uint32_t cnt = (uint32_t)__popcll(ties);
        const uint32_t fst = ties ? col * 64u + (uint32_t)(__ffsll((long long)ties) - 1) : PGX_NO_SEQUENCE;
        if (colmax > best) {
            next = best > nxt ? best : nxt;
            best = colmax; n_best = cnt; first = fst;
        } else if (colmax == best) {
            n_best += cnt;
            first = fst < first ? fst : first;
            next = nxt > next ? nxt : next;
        } else
            next = colmax > next ? colmax : next;
    }
};

} // namespace

#define PGX_HITS_UNROLL 4 // MEMs whose loads are in flight together

template <bool WIDE>
__device__ __forceinline__ void pgx_read_hits_body(const uint64_t *__restrict__ mem_off, const pgx_mem *__restrict__ mems,
                                                   const unsigned long long *__restrict__ sets, uint64_t n_reads, uint64_t n_mems, uint64_t n_seq, uint32_t W,
                                                   uint32_t sp_shift, uint32_t flags, pgx_read_hit *__restrict__ hits, unsigned long long *__restrict__ best_sets,
                                                   uint32_t *__restrict__ scores) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t Sp = 1u << sp_shift; // lanes a read
    const uint64_t r = t >> sp_shift;
    const uint32_t sl = WIDE ? lane : lane & (Sp - 1u); // the lane's place within its read
    const bool live = r < n_reads;
    if (WIDE && !live) return; // (a whole wave)
    // the MEMs of the read, kept inside the array whatever the offsets say
    uint64_t m0 = live ? mem_off[r] : 0, m1 = live ? mem_off[r + 1] : 0;
    m1 = m1 < n_mems ? m1 : n_mems;
    m0 = m0 < m1 ? m0 : m1;
    const uint64_t last_bits = n_seq - (uint64_t)(W - 1u) * 64u; // valid bits of the last word column, 1 .. 64
    const unsigned long long last_mask = last_bits >= 64 ? ~0ull : (1ull << last_bits) - 1ull;

    unsigned long long covered = 0;
    uint32_t n_located = 0;
    if (WIDE) { // which MEMs have any bit: lane = word of the set, one coalesced load a MEM
        HitsSweep all;
        for (uint64_t m = m0; m < m1; m += PGX_HITS_UNROLL) {
            unsigned long long st[PGX_HITS_UNROLL], en[PGX_HITS_UNROLL], wd[PGX_HITS_UNROLL];
#pragma unroll
            for (int i = 0; i < PGX_HITS_UNROLL; i++) {
                const uint64_t mm = m + (uint64_t)i;
                const bool ok = mm < m1;
                st[i] = ok ? mems[mm].start : 0;
                en[i] = ok ? mems[mm].end : 0;
                wd[i] = ok && lane < W ? sets[mm * W + lane] & (lane == W - 1u ? last_mask : ~0ull) : 0;
            }
#pragma unroll
            for (int i = 0; i < PGX_HITS_UNROLL; i++)
                if (__ballot(wd[i] != 0)) { all.add(st[i], en[i]); n_located++; }
        }
        covered = all.cov;
    }

    HitsSummary sum;
    unsigned long long keep_max = 0, keep_ties = 0; // WIDE: lane j keeps column j's maximum and its ties
    unsigned long long ties_here = 0;                // !WIDE: the ties of the only column
    HitsSweep all; // !WIDE: the sweep over every located MEM
    for (uint32_t col = 0; col < W; col++) {
        const uint64_t s = (uint64_t)col * 64u + sl;
        const bool valid = live && s < n_seq;
        const unsigned long long col_mask = col == W - 1u ? last_mask : ~0ull;
        HitsSweep mine;
        for (uint64_t m = m0; m < m1; m += PGX_HITS_UNROLL) {
            unsigned long long st[PGX_HITS_UNROLL], en[PGX_HITS_UNROLL], wd[PGX_HITS_UNROLL];
#pragma unroll
            for (int i = 0; i < PGX_HITS_UNROLL; i++) {
                const uint64_t mm = m + (uint64_t)i;
                const bool ok = mm < m1;
                st[i] = ok ? mems[mm].start : 0;
                en[i] = ok ? mems[mm].end : 0;
                wd[i] = ok ? sets[mm * W + col] & col_mask : 0;
            }
#pragma unroll
            for (int i = 0; i < PGX_HITS_UNROLL; i++) {
                if (!WIDE && wd[i]) { all.add(st[i], en[i]); n_located++; }
                if ((wd[i] >> (sl & 63u)) & 1ull) mine.add(st[i], en[i]);
            }
        }
        const unsigned long long cov = valid ? mine.cov : 0;
        if ((flags & PGX_HITS_SCORES) && valid) scores[r * n_seq + s] = cov > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cov;
        const unsigned long long colmax = hits_group_max(cov, Sp);
        const bool tie = valid && cov == colmax;
        unsigned long long ties = __ballot(tie);
        if (!WIDE && Sp < 64u) ties = (ties >> (lane & ~(Sp - 1u))) & ((1ull << Sp) - 1ull);
        const unsigned long long nxt = hits_group_max(tie ? 0 : cov, Sp);
        sum.merge(col, colmax, ties, nxt);
        if (WIDE) {
            if (lane == col) { keep_max = colmax; keep_ties = ties; }
        } else
            ties_here = ties;
    }
    if (!WIDE) covered = all.cov;
    if (!live) return;
    if (flags & PGX_HITS_BEST_SETS) {
        if (WIDE) {
            if (lane < W) best_sets[r * W + lane] = sum.best > 0 && keep_max == sum.best ? keep_ties : 0;
        } else if (sl == 0)
            best_sets[r] = sum.best > 0 ? ties_here : 0;
    }
    if (sl == 0) {
        pgx_read_hit h;
        h.best_score = sum.best;
        h.next_score = sum.best > 0 ? sum.next : 0;
        h.covered = covered;
        h.best_seq = sum.best > 0 ? sum.first : PGX_NO_SEQUENCE;
        h.n_best = sum.best > 0 ? sum.n_best : 0;
        h.n_located = n_located;
        h.n_mems = (uint32_t)(m1 - m0);
        hits[r] = h;
    }
}

// n_seq <= 64 (W == 1): Sp = 1 << sp_shift lanes a read
__global__ void __launch_bounds__(PGX_HITS_THREADS)
pgx_read_hits_kernel(const uint64_t *__restrict__ mem_off, const pgx_mem *__restrict__ mems, const unsigned long long *__restrict__ sets, uint64_t n_reads,
                     uint64_t n_mems, uint64_t n_seq, uint32_t sp_shift, uint32_t flags, pgx_read_hit *__restrict__ hits, unsigned long long *__restrict__ best_sets,
                     uint32_t *__restrict__ scores) {
    pgx_read_hits_body<false>(mem_off, mems, sets, n_reads, n_mems, n_seq, 1u, sp_shift, flags, hits, best_sets, scores);
}

// 64 < n_seq <= 64 W, W <= 64: a wave a read, column after column
__global__ void __launch_bounds__(PGX_HITS_THREADS)
pgx_read_hits_wide_kernel(const uint64_t *__restrict__ mem_off, const pgx_mem *__restrict__ mems, const unsigned long long *__restrict__ sets, uint64_t n_reads,
                          uint64_t n_mems, uint64_t n_seq, uint32_t W, uint32_t flags, pgx_read_hit *__restrict__ hits, unsigned long long *__restrict__ best_sets,
                          uint32_t *__restrict__ scores) {
    pgx_read_hits_body<true>(mem_off, mems, sets, n_reads, n_mems, n_seq, W, 6u, flags, hits, best_sets, scores);
}

// pgx_read_hits_arrays: *bad = the first read whose MEM starts do not ascend strictly (left as it is when there is none); a thread a read
__global__ void __launch_bounds__(256)
pgx_read_hits_check_kernel(const uint64_t *__restrict__ mem_off, const pgx_mem *__restrict__ mems, uint64_t n_reads, uint64_t n_mems,
                           unsigned long long *__restrict__ bad) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    uint64_t m0 = mem_off[r], m1 = mem_off[r + 1];
    m1 = m1 < n_mems ? m1 : n_mems;
    m0 = m0 < m1 ? m0 : m1;
    for (uint64_t m = m0 + 1; m < m1; m++)
        if (mems[m].start <= mems[m - 1].start) {
            atomicMin(bad, (unsigned long long)r);
            return;
        }
}
