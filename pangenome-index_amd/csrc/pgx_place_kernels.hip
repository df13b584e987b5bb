// pgx_place_kernels.hip -- read placement (include/pgx.h "read placement"): the packed positions of a batch's MEMs voted onto diagonals
// per read, every diagonal scored, one pgx_read_place a read and optionally the list of all placements.
//
//   plan     a thread a read: its range of anchors (the values of its consecutive MEMs are one contiguous range), and the two maxima the
//            key layout needs -- most MEMs of a read, largest MEM start (the last MEM's: starts ascend)
//   first    a thread a MEM: the first MEM of its read (mem_offsets searched), so that an anchor finds its ordinal with one load
//   keys     output-centric like pgx_ml_gather_kernel: a block per PGX_ML_SPAN anchors finds its MEMs by binary search of loc_offsets staged
//            in LDS; key = ((seq * span + off - start + bias) << ordinal_bits) | (m - first MEM of the read)
//   (sort)   the keys of a read are one segment: pgx_ml_classify_kernel and the tag stage's segmented sort-unique sort them unchanged
//            (keys of a read differ unless a value is repeated inside one MEM; such repeats are dropped there)
//   sweep    G lanes a read (G a power of two, 64 / G reads a wave), lane = anchor, G anchors a step.  Inside a placement the keys ascend
//            by ordinal, hence by MEM start, so anchor i adds max(0, end_i - max(start_i, R_i)), R_i = the largest end of the earlier
//            anchors of its placement: a segmented max-scan, then a prefix sum; a placement is closed by the head of the next one, and
//            what is open at the end of a step is carried (key group, sum, count, reach).  The closed placements of a step are folded into
//            (best, ties, first, runner-up) the way HitsSummary::merge folds columns.  Registers do not depend on anchors or MEMs.
//            LIST: the same walk once more, writing every closed placement behind the read's offset.
//   check    pgx_read_place_arrays: the first read with a value whose sequence is >= n_seq
// Every index is 64-bit; offsets that point beyond the arrays are clamped; atomics are max / min only (order-independent).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

namespace {

// last index j in [lo, hi) with a[j] <= x (a[lo] <= x assumed)
template <class Ptr>
__device__ __forceinline__ uint64_t place_last_le(Ptr a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo + 1 < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ unsigned long long place_wave_max(unsigned long long v) {
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// over the G lanes of a read (G a power of two <= 64; all 64 lanes of the wave take part)
__device__ __forceinline__ unsigned long long place_group_max(unsigned long long v, uint32_t G) {
    for (uint32_t d = 1; d < G; d <<= 1) {
        const unsigned long long o = __shfl_xor(v, (int)d, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long place_group_sum(unsigned long long v, uint32_t G) {
    for (uint32_t d = 1; d < G; d <<= 1) v += __shfl_xor(v, (int)d, 64);
    return v;
}

struct PlaceSummary { // best, ties, first tie and runner-up over the placements closed so far (in placement order)
    unsigned long long best = 0, next = 0, n_best = 0, first_group = 0, n_placements = 0;
    uint32_t first_mems = 0;
    // a step's placements: maximum smax on cnt of them, the first of those (group fg, fm MEMs), runner-up nxt (< smax, 0 if none)
    __device__ __forceinline__ void merge(unsigned long long smax, unsigned long long cnt, unsigned long long fg, uint32_t fm, unsigned long long nxt) {
        if (smax > best) {
            next = best > nxt ? best : nxt;
            best = smax; n_best = cnt; first_group = fg; first_mems = fm;
        } else if (smax == best) {
            if (smax) n_best += cnt; // (earlier steps hold earlier placements: the first stays)
            next = nxt > next ? nxt : next;
        } else
            next = smax > next ? smax : next;
    }
};

} // namespace

__global__ void __launch_bounds__(256)
pgx_place_plan_kernel(const uint64_t *__restrict__ mem_off, const uint64_t *__restrict__ loc_off, const pgx_mem *__restrict__ mems, uint64_t n_reads,
                      uint64_t n_mems, uint64_t n_values, uint64_t *__restrict__ aoff, uint64_t *__restrict__ acnt, unsigned long long *__restrict__ mx) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long nm = 0, last_start = 0;
    if (r <= n_reads) {
        uint64_t m0 = mem_off[r];
        m0 = m0 < n_mems ? m0 : n_mems;
        uint64_t a0 = loc_off[m0];
        a0 = a0 < n_values ? a0 : n_values;
        aoff[r] = a0;
        if (r == n_reads) mx[2] = a0; // (the anchors of the batch lie in [mx[3], mx[2]))
        if (r == 0) mx[3] = a0;
        if (r < n_reads) {
            uint64_t m1 = mem_off[r + 1];
            m1 = m1 < n_mems ? m1 : n_mems;
            m1 = m1 > m0 ? m1 : m0;
            uint64_t a1 = loc_off[m1];
            a1 = a1 < n_values ? a1 : n_values;
            acnt[r] = a1 > a0 ? a1 - a0 : 0;
            nm = m1 - m0;
            if (nm) last_start = mems[m1 - 1].start;
        }
    }
    nm = place_wave_max(nm);
    last_start = place_wave_max(last_start);
    if ((threadIdx.x & 63u) == 0) {
        if (nm) atomicMax(mx + 0, nm);
        if (last_start) atomicMax(mx + 1, last_start);
    }
}

__global__ void __launch_bounds__(256)
pgx_place_first_kernel(const uint64_t *__restrict__ mem_off, uint64_t n_reads, uint64_t n_mems, uint64_t *__restrict__ mfirst) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_mems) return;
    // the read that holds m: the last r with mem_off[r] <= m (empty reads before it share its offset and come earlier)
    uint64_t f = m;
    if (n_reads && mem_off[0] <= m) {
        const uint64_t r = place_last_le(mem_off, 0, n_reads, m);
        f = mem_off[r];
    }
    mfirst[m] = f <= m ? f : m;
}

// Anchors [a_first, a_first + na) of the batch (the values of the pass's MEMs [m0, m1): loc_off[m0] <= a_first, a_first + na <= loc_off[m1]),
// keys[a - a_first].  L > 0; span = L + bias; bias >= every MEM start.
__global__ void __launch_bounds__(256)
pgx_place_keys_kernel(const pgx_mem *__restrict__ mems, const uint64_t *__restrict__ loc_off, const uint64_t *__restrict__ mfirst,
                      const uint64_t *__restrict__ values, uint64_t m0, uint64_t m1, uint64_t a_first, uint64_t na, uint64_t L, uint64_t span,
                      uint64_t bias, uint32_t ordinal_bits, uint64_t *__restrict__ keys) {
    __shared__ uint64_t s_off[PGX_ML_WIN];
    __shared__ uint64_t s_ab[2];
    const uint64_t a_begin = a_first + (uint64_t)blockIdx.x * PGX_ML_SPAN;
    if (a_begin >= a_first + na || m1 <= m0) return;
    const uint64_t a_end = a_begin + PGX_ML_SPAN < a_first + na ? a_begin + PGX_ML_SPAN : a_first + na;
    if (threadIdx.x == 0) s_ab[0] = place_last_le(loc_off, m0, m1, a_begin);
    if (threadIdx.x == 64) s_ab[1] = place_last_le(loc_off, m0, m1, a_end - 1);
    __syncthreads();
    const uint64_t ma = s_ab[0], mb = s_ab[1] + 1; // the block's MEMs: [ma, mb); loc_off[ma .. mb] bound them (mb <= m1)
    const bool off_lds = mb - ma + 1 <= PGX_ML_WIN;
    if (off_lds)
        for (uint64_t t = threadIdx.x; t <= mb - ma; t += blockDim.x) s_off[t] = loc_off[ma + t];
    __syncthreads();
    for (uint64_t a = a_begin + threadIdx.x; a < a_end; a += blockDim.x) {
        const uint64_t m = off_lds ? ma + place_last_le(s_off, 0, mb - ma, a) : place_last_le(loc_off, ma, mb, a);
        const uint64_t v = values[a];
        const uint64_t seq = v / L, off = v - seq * L;
        const uint64_t start = mems[m].start;
        const uint64_t group = seq * span + (off + bias - (start < bias ? start : bias));
        keys[a - a_first] = (group << ordinal_bits) | (m - mfirst[m]);
    }
}

// Reads [r_first, r_first + nr) of the pass that starts at read r_pass (seg / ucount are pass-local: read r at r - r_pass; keys: the pass's).
// G = 1 << g_shift lanes a read.  !LIST: recs[r] and pcount[r] (= n_placements).  LIST: the placements of read r at places[list_off[r - r_pass] ..).
template <bool LIST>
__global__ void __launch_bounds__(PGX_PLACE_THREADS)
pgx_place_sweep_kernel(const uint64_t *__restrict__ mem_off, const pgx_mem *__restrict__ mems, const uint64_t *__restrict__ loc_off,
                       const uint64_t *__restrict__ acnt, const uint64_t *__restrict__ keys, const uint64_t *__restrict__ seg,
                       const uint64_t *__restrict__ ucount, uint64_t r_pass, uint64_t r_first, uint64_t nr, uint64_t n_mems, uint64_t span, uint64_t bias,
                       uint32_t ordinal_bits, uint32_t g_shift, pgx_read_place *__restrict__ recs, uint64_t *__restrict__ pcount,
                       const uint64_t *__restrict__ list_off, pgx_placement *__restrict__ places) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t G = 1u << g_shift;
    const uint32_t gl = lane & (G - 1u), gbase = lane & ~(G - 1u);
    const unsigned long long gmask = G >= 64u ? ~0ull : (1ull << G) - 1ull;
    const uint64_t ri = t >> g_shift;
    const bool live = ri < nr;
    const uint64_t r = r_first + (live ? ri : 0), q = r - r_pass;
    uint64_t m0 = live ? mem_off[r] : 0, m1 = live ? mem_off[r + 1] : 0;
    m1 = m1 < n_mems ? m1 : n_mems;
    m0 = m0 < m1 ? m0 : m1;
    const uint64_t K = live ? ucount[q] : 0, kbase = live ? seg[q] : 0;
    const unsigned long long omask = ordinal_bits ? (~0ull >> (64u - ordinal_bits)) : 0ull;

    unsigned long long n_located = 0;
    if (!LIST) { // MEMs with a value
        for (uint64_t m = m0 + gl; m < m1; m += G) n_located += loc_off[m + 1] > loc_off[m] ? 1ull : 0ull;
        n_located = place_group_sum(n_located, G);
    }

    PlaceSummary sum;
    unsigned long long c_group = 0, c_sum = 0, c_reach = 0; // the placement still open behind the steps so far
    uint32_t c_cnt = 0;
    const uint64_t out0 = LIST && live ? list_off[q] : 0;
    for (uint64_t s0 = 0; __any(s0 < K); s0 += G) {
        const uint64_t i = s0 + gl;
        const bool in_step = s0 < K, act = i < K; // (in_step: the same for the G lanes of a read)
        const unsigned long long key = act ? keys[kbase + i] : 0ull;
        const unsigned long long g = key >> ordinal_bits; // (ordinal_bits < 64)
        const uint64_t m = m0 + (key & omask);
        unsigned long long st = 0, en = 0;
        if (act && m < m1) { st = mems[m].start; en = mems[m].end; }
        unsigned long long prev_g = __shfl_up(g, 1, (int)G);
        if (gl == 0) prev_g = c_group;
        const bool head = act && ((i == 0) || g != prev_g);
        const unsigned long long hm = (__ballot(head) >> gbase) & gmask; // heads of this read's step
        // segmented inclusive max-scan of the ends
        unsigned long long incl = en;
        bool f = head;
        for (uint32_t d = 1; d < G; d <<= 1) {
            const unsigned long long ov = __shfl_up(incl, d, (int)G);
            const int of = __shfl_up((int)f, d, (int)G);
            if (gl >= d && !f) { incl = ov > incl ? ov : incl; f = of != 0; }
        }
        const unsigned long long below = gl ? hm & ((1ull << gl) - 1ull) : 0ull;     // heads before this lane
        const bool cont = (below | (head ? 1ull << gl : 0ull)) == 0;                  // the lane's placement began in an earlier step
        unsigned long long reach = __shfl_up(incl, 1, (int)G);
        if (gl == 0) reach = 0;
        if (cont) reach = reach > c_reach ? reach : c_reach;
        if (head) reach = 0;
        const unsigned long long from = st > reach ? st : reach;
        const unsigned long long c = act && en > from ? en - from : 0ull;
        // inclusive prefix sum of the contributions over the read's lanes
        unsigned long long P = c;
        for (uint32_t d = 1; d < G; d <<= 1) {
            const unsigned long long ov = __shfl_up(P, d, (int)G);
            if (gl >= d) P += ov;
        }
        // a head closes the placement before it: the one of lane gl - 1, or the carried one
        const bool emit = head && i > 0;
        const int hp = below ? 63 - __clzll((long long)below) : -1; // head of the placement of lane gl - 1 (-1: it is the carried one)
        const unsigned long long P_prev = __shfl_up(P, 1, (int)G);   // P[gl - 1]
        const unsigned long long P_hp = __shfl(P, hp > 0 ? hp - 1 : 0, (int)G);
        unsigned long long e_tot = 0;
        uint32_t e_cnt = 0;
        if (emit) {
            if (gl == 0) { e_tot = c_sum; e_cnt = c_cnt; }
            else if (hp < 0) { e_tot = c_sum + P_prev; e_cnt = c_cnt + gl; }
            else { e_tot = P_prev - (hp > 0 ? P_hp : 0ull); e_cnt = gl - (uint32_t)hp; }
        }
        const unsigned long long e_group = prev_g;
        const unsigned long long em = (__ballot(emit) >> gbase) & gmask;
        if (LIST) {
            if (emit) {
                const uint64_t at = out0 + sum.n_placements + (uint64_t)__popcll(em & ((1ull << gl) - 1ull));
                const uint64_t sq = e_group / span;
                pgx_placement p;
                p.diag = (int64_t)(e_group - sq * span) - (int64_t)bias;
                p.score = e_tot;
                p.seq = (uint32_t)sq;
                p.mems = e_cnt;
                places[at] = p;
            }
            sum.n_placements += (unsigned long long)__popcll(em);
        } else {
            const unsigned long long smax = place_group_max(emit ? e_tot : 0ull, G);
            const unsigned long long ties = (__ballot(emit && e_tot == smax) >> gbase) & gmask;
            const unsigned long long nxt = place_group_max(emit && e_tot < smax ? e_tot : 0ull, G);
            const int fl = ties ? __ffsll((long long)ties) - 1 : 0;
            const unsigned long long fg = __shfl(e_group, fl, (int)G);
            const uint32_t fm = (uint32_t)__shfl((int)e_cnt, fl, (int)G);
            if (em) sum.merge(smax, (unsigned long long)__popcll(ties), fg, fm, nxt);
            sum.n_placements += (unsigned long long)__popcll(em);
        }
        // what stays open behind this step
        const uint64_t left = in_step ? K - s0 : 1;
        const uint32_t la = left >= G ? G - 1u : (uint32_t)left - 1u; // the last lane of the step with a key
        const unsigned long long upto = la >= 63u ? hm : hm & ((2ull << la) - 1ull);
        const int hl = upto ? 63 - __clzll((long long)upto) : -1;
        const unsigned long long P_la = __shfl(P, (int)la, (int)G), P_hl = __shfl(P, hl > 0 ? hl - 1 : 0, (int)G);
        const unsigned long long incl_la = __shfl(incl, (int)la, (int)G), g_la = __shfl(g, (int)la, (int)G);
        if (in_step) {
            if (hl < 0) {
                c_sum += P_la; c_cnt += la + 1u;
                c_reach = incl_la > c_reach ? incl_la : c_reach;
            } else {
                c_sum = P_la - (hl > 0 ? P_hl : 0ull); c_cnt = la - (uint32_t)hl + 1u;
                c_reach = incl_la; c_group = g_la;
            }
        }
    }
    if (!live || gl != 0) return;
    if (K) { // the last placement
        if (LIST) {
            const uint64_t sq = c_group / span;
            pgx_placement p;
            p.diag = (int64_t)(c_group - sq * span) - (int64_t)bias;
            p.score = c_sum;
            p.seq = (uint32_t)sq;
            p.mems = c_cnt;
            places[out0 + sum.n_placements] = p;
        } else
            sum.merge(c_sum, 1ull, c_group, c_cnt, 0ull);
        sum.n_placements++;
    }
    if (LIST) return;
    pgx_read_place h;
    const bool any = sum.best > 0;
    const uint64_t bs = sum.first_group / span;
    h.best_score = sum.best;
    h.next_score = any ? sum.next : 0;
    h.best_diag = any ? (int64_t)(sum.first_group - bs * span) - (int64_t)bias : 0;
    h.n_anchors = acnt[r];
    h.n_placements = sum.n_placements;
    h.best_seq = any ? (uint32_t)bs : PGX_NO_SEQUENCE;
    h.n_best = any ? (sum.n_best > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum.n_best) : 0u;
    h.best_mems = any ? sum.first_mems : 0u;
    h.n_located = (uint32_t)n_located;
    h.n_mems = (uint32_t)(m1 - m0);
    h.reserved = 0;
    recs[r] = h;
    pcount[r] = sum.n_placements;
}

template __global__ void pgx_place_sweep_kernel<false>(const uint64_t *, const pgx_mem *, const uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *,
                                                       const uint64_t *, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint32_t, uint32_t, pgx_read_place *,
                                                       uint64_t *, const uint64_t *, pgx_placement *);
template __global__ void pgx_place_sweep_kernel<true>(const uint64_t *, const pgx_mem *, const uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *,
                                                      const uint64_t *, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint32_t, uint32_t, pgx_read_place *,
                                                      uint64_t *, const uint64_t *, pgx_placement *);

// pgx_read_place_arrays: *bad = the first read with a value whose sequence is >= n_seq (left as it is when there is none); a thread a value
__global__ void __launch_bounds__(256)
pgx_place_check_values_kernel(const uint64_t *__restrict__ values, uint64_t n_values, uint64_t L, uint64_t n_seq, const uint64_t *__restrict__ aoff,
                              uint64_t n_reads, unsigned long long *__restrict__ bad) {
    const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_values || n_reads == 0) return;
    if (values[a] / L < n_seq) return;
    if (aoff[0] > a || a >= aoff[n_reads]) return; // (a value no read owns)
    atomicMin(bad, (unsigned long long)place_last_le(aoff, 0, n_reads, a));
}
