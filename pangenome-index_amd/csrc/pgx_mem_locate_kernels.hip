// pgx_mem_locate_kernels.hip -- the occurrences of a batch's MEMs (pgx_batch_locate), from the device-resident MEM array.
//
//   plan     one thread per MEM: the cap and the range checks -> count, the BWT range [qs, qe] (empty when not located), not-located total
//   (scan)   counts -> value offsets (scan_excl, pgx_runtime.hip)
//   cut      one thread: the end of the next pass over consecutive MEMs whose values fit the budget (only when the batch does not)
//   gather   resident suffix array (LCE image): output-centric, a block per PGX_ML_SPAN values, its MEMs found by binary search of the
//            value offsets (staged in LDS), one read of lce_sa per value, text position -> (sequence, offset) by search in the sequence
//            starts -- a MEM of 10^5 occurrences is spread over many blocks like any other
//   (chains) pgx_locate_plan_kernel / pgx_locate_walk_kernel (pgx_locate_kernels.hip) on the ranges of the plan
//   classify PGX_LOCATE_UNIQUE: pass-local segment offsets and the size-class lists of the tag stage's sort kernels, built by compaction
//            (wave-aggregated appends; every segment is sorted on its own, so the list order does not matter)
//   sets     PGX_LOCATE_SEQ_SETS, and PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE over few sequences: one bit per sequence per MEM, W words a MEM.
//            The block shape of the gather, but no value is written: a block ORs the bits of its PGX_ML_SPAN values into an LDS window of
//            its MEMs' words and writes every non-zero word once -- a plain store where the MEM lies inside the block, a global atomicOr
//            where neighbouring blocks share it.  From the resident suffix array, or from the sequence ids the chain walk left in the pass
//            buffer.  OR does not depend on the order: the bytes are the same from run to run.
//   count / expand   the routed unique form: popcount per MEM -> ucount, (scan), then a wave per MEM writes the set bits as ascending ids
//   stride   loc_offsets of the set form: m * W
// Every index is 64-bit; no kernel reads outside its arrays whatever the pgx_mem contents.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

// wave-aggregated increment of *ctr by the lanes where `pred` holds; returns this lane's slot (valid where pred)
__device__ __forceinline__ uint64_t pgx_ml_append(bool pred, unsigned long long *ctr) {
    const unsigned long long mask = __ballot(pred);
    if (!mask) return 0;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)mask) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(ctr, (unsigned long long)__popcll(mask));
    base = __shfl(base, leader, 64);
    return base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(256)
pgx_ml_plan_kernel(const pgx_mem *__restrict__ mems, uint64_t n, uint64_t bwt_n, uint64_t max_occ, uint64_t *__restrict__ cnt,
                   uint64_t *__restrict__ qs, uint64_t *__restrict__ qe, unsigned long long *__restrict__ n_not_located) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool skipped = false;
    if (i < n) {
        const uint64_t bs = mems[i].bwt_start;
        const int64_t sz = mems[i].size;
        // size <= 0, or bwt_start + size - 1 >= bwt_n (written without overflow), or over the cap: no values
        const bool ok = sz > 0 && bs < bwt_n && (uint64_t)sz <= bwt_n - bs && (max_occ == 0 || (uint64_t)sz <= max_occ);
        cnt[i] = ok ? (uint64_t)sz : 0;
        qs[i] = ok ? bs : 1;
        qe[i] = ok ? bs + (uint64_t)sz - 1 : 0; // (last < first: the empty state of pgx_locate_plan_kernel)
        skipped = !ok;
    }
    pgx_ml_append(skipped, n_not_located);
}

// the pass [m0, m1): m1 = the last m in [m0 + 1, n] with off[m] <= off[m0] + budget, at least m0 + 1 (a MEM above the budget is a pass of
// its own); out = {m1, off[m1]}
__global__ void pgx_ml_cut_kernel(const uint64_t *__restrict__ off, uint64_t n, uint64_t m0, uint64_t budget, uint64_t *__restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t lim = off[m0] + budget;
    uint64_t lo = m0 + 1, hi = n + 1; // first m in [m0 + 1, n] with off[m] > lim (n + 1 if none)
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] <= lim) lo = mid + 1; else hi = mid;
    }
    const uint64_t m1 = lo - 1 > m0 ? lo - 1 : m0 + 1;
    out[0] = m1;
    out[1] = off[m1];
}

// last index j in [lo, hi) with a[j] <= x (a[lo] <= x assumed)
template <class Ptr>
__device__ __forceinline__ uint64_t pgx_ml_last_le(Ptr a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo + 1 < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// Values [o_first, o_first + nv) of the batch (o = absolute value index; off = value offsets of all MEMs; the pass's MEMs are [m0, m1), so
// off[m0] <= o_first and o_first + nv <= off[m1]), written to out[o - o_first].  seq_start: n_seq + 1 text positions (the last = bwt_n).
__global__ void __launch_bounds__(256)
pgx_ml_gather_kernel(const pgx_mem *__restrict__ mems, const uint64_t *__restrict__ off, uint64_t m0, uint64_t m1, uint64_t o_first, uint64_t nv,
                     const uint32_t *__restrict__ sa32, uint64_t bwt_n, const uint64_t *__restrict__ seq_start, uint64_t n_seq, uint64_t max_length,
                     int seq_ids, uint64_t *__restrict__ out) {
    __shared__ uint64_t s_off[PGX_ML_WIN];
    __shared__ uint64_t s_seq[PGX_ML_WIN];
    __shared__ uint64_t s_ab[2];
    const uint64_t o_begin = o_first + (uint64_t)blockIdx.x * PGX_ML_SPAN;
    if (o_begin >= o_first + nv) return;
    const uint64_t o_end = o_begin + PGX_ML_SPAN < o_first + nv ? o_begin + PGX_ML_SPAN : o_first + nv;
    if (threadIdx.x == 0) s_ab[0] = pgx_ml_last_le(off, m0, m1, o_begin);
    if (threadIdx.x == 64) s_ab[1] = pgx_ml_last_le(off, m0, m1, o_end - 1);
    const bool seq_lds = n_seq + 1 <= PGX_ML_WIN;
    if (seq_lds)
        for (uint64_t t = threadIdx.x; t <= n_seq; t += blockDim.x) s_seq[t] = seq_start[t];
    __syncthreads();
    const uint64_t ma = s_ab[0], mb = s_ab[1] + 1; // the block's MEMs: [ma, mb); off[ma .. mb] bound them (mb <= m1)
    const bool off_lds = mb - ma + 1 <= PGX_ML_WIN;
    if (off_lds)
        for (uint64_t t = threadIdx.x; t <= mb - ma; t += blockDim.x) s_off[t] = off[ma + t];
    __syncthreads();
    for (uint64_t o = o_begin + threadIdx.x; o < o_end; o += blockDim.x) {
        const uint64_t m = off_lds ? ma + pgx_ml_last_le(s_off, 0, mb - ma, o) : pgx_ml_last_le(off, ma, mb, o);
        const uint64_t row = mems[m].bwt_start + (o - (off_lds ? s_off[m - ma] : off[m]));
        const uint64_t g = row < bwt_n ? sa32[row] : 0; // (always: a located MEM's range lies inside the BWT, pgx_ml_plan_kernel)
        const uint64_t q = seq_lds ? pgx_ml_last_le(s_seq, 0, n_seq, g) : pgx_ml_last_le(seq_start, 0, n_seq, g);
        const uint64_t st = seq_lds ? s_seq[q] : seq_start[q];
        out[o - o_first] = seq_ids ? q : q * max_length + (g - st);
    }
}

// PGX_LOCATE_UNIQUE, a pass of np MEMs (cnt, off and ucount point at its first MEM): seg[i] = off[i] - off[0] (np + 1 entries), the wave list
// (1 .. PGX_SORT_LDS_CAP values) and the workgroup list (more) as pass-local indices, need[i] = the global scratch of a workgroup segment
// above the LDS cap (its power of two), ucount[i] = 0.  ctr[0] / ctr[1]: list lengths.
__global__ void __launch_bounds__(256)
pgx_ml_classify_kernel(const uint64_t *__restrict__ cnt, const uint64_t *__restrict__ off, uint64_t np, uint64_t *__restrict__ seg,
                       uint64_t *__restrict__ wave_list, uint64_t *__restrict__ wg_list, uint64_t *__restrict__ need, uint64_t *__restrict__ ucount,
                       unsigned long long *__restrict__ ctr) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t c = 0;
    if (i <= np) seg[i] = off[i] - off[0];
    if (i < np) {
        c = cnt[i];
        ucount[i] = 0;
        uint64_t p2 = 64;
        while (p2 < c) p2 <<= 1;
        need[i] = (c > PGX_SORT_LDS_CAP && p2 > PGX_SORT_WG_LDS_CAP) ? p2 : 0;
    }
    const bool wave = i < np && c >= 1 && c <= PGX_SORT_LDS_CAP, wg = i < np && c > PGX_SORT_LDS_CAP;
    const uint64_t a = pgx_ml_append(wave, ctr + 0);
    if (wave) wave_list[a] = i;
    const uint64_t b = pgx_ml_append(wg, ctr + 1);
    if (wg) wg_list[b] = i;
}

// ---- sequence sets ---------------------------------------------------------------------------------------------------------------
// Values [o_first, o_first + nv) of the batch as in pgx_ml_gather_kernel, ORed into sets[(m - m0) * W + (q >> 6)], bit q & 63, for the
// sequence q of each value of MEM m (sets: (m1 - m0) * W words, cleared by the caller).  FROM_IDS: q = ids[o - o_first], what
// pgx_locate_walk_kernel wrote for the pass; else q = the sequence of lce_sa[row] as in the gather.  A block walks its MEMs [ma, mb) in
// windows of at most PGX_ML_WIN - 1 MEMs and PGX_ML_SET_WIN words; a window's values are one contiguous range.  Each thread merges the
// bits of consecutive values of one word in a register before it touches LDS (a MEM of thousands of occurrences costs a block one LDS
// atomic per thread, not one per value).  1 <= W <= PGX_ML_SET_WORDS_MAX; a q at or beyond 64 W (never, for the index the caller sized W
// from) is dropped.
template <bool FROM_IDS>
__device__ __forceinline__ void pgx_ml_sets_body(const pgx_mem *__restrict__ mems, const uint64_t *__restrict__ off, uint64_t m0, uint64_t m1, uint64_t o_first,
                                                 uint64_t nv, const uint32_t *__restrict__ sa32, const uint64_t *__restrict__ ids, uint64_t bwt_n,
                                                 const uint64_t *__restrict__ seq_start, uint64_t n_seq, uint32_t W, unsigned long long *__restrict__ sets) {
    __shared__ uint64_t s_off[PGX_ML_WIN];
    __shared__ uint64_t s_seq[FROM_IDS ? 1 : PGX_ML_WIN];
    __shared__ unsigned long long s_set[PGX_ML_SET_WIN];
    __shared__ uint64_t s_ab[2];
    const uint64_t o_begin = o_first + (uint64_t)blockIdx.x * PGX_ML_SPAN;
    if (o_begin >= o_first + nv || W == 0 || W > PGX_ML_SET_WORDS_MAX) return;
    const uint64_t o_end = o_begin + PGX_ML_SPAN < o_first + nv ? o_begin + PGX_ML_SPAN : o_first + nv;
    if (threadIdx.x == 0) s_ab[0] = pgx_ml_last_le(off, m0, m1, o_begin);
    if (threadIdx.x == 64) s_ab[1] = pgx_ml_last_le(off, m0, m1, o_end - 1);
    const bool seq_lds = !FROM_IDS && n_seq + 1 <= PGX_ML_WIN;
    if (seq_lds)
        for (uint64_t t = threadIdx.x; t <= n_seq; t += blockDim.x) s_seq[t] = seq_start[t];
    __syncthreads();
    const uint64_t ma = s_ab[0], mb = s_ab[1] + 1; // the block's MEMs: [ma, mb), mb <= m1
    const uint64_t n_bits = (uint64_t)W * 64;
    const uint64_t win = (PGX_ML_SET_WIN / W) < (PGX_ML_WIN - 1) ? (PGX_ML_SET_WIN / W) : (PGX_ML_WIN - 1); // MEMs per window
    for (uint64_t wa = ma; wa < mb; wa += win) {
        const uint64_t wb = wa + win < mb ? wa + win : mb, nm = wb - wa, nw = nm * W;
        for (uint64_t t = threadIdx.x; t <= nm; t += blockDim.x) s_off[t] = off[wa + t];
        for (uint64_t t = threadIdx.x; t < nw; t += blockDim.x) s_set[t] = 0;
        __syncthreads();
        const uint64_t v_lo = s_off[0] > o_begin ? s_off[0] : o_begin, v_hi = s_off[nm] < o_end ? s_off[nm] : o_end; // the window's values of this block
        uint64_t k = 0, key = ~0ull;   // k: window-local MEM of the value before (values ascend, so does k)
        unsigned long long acc = 0;    // bits gathered for word `key` of the window
        // PGX_ML_SET_BATCH values of a thread at a time, stage by stage, so that their loads are in flight together: the merge below makes one
        // value depend on the one before, and a loop of whole values would wait for every suffix-array entry on its own
        for (uint64_t ob = v_lo + threadIdx.x; ob < v_hi; ob += (uint64_t)PGX_ML_SET_BATCH * blockDim.x) {
            uint64_t kk[PGX_ML_SET_BATCH], q[PGX_ML_SET_BATCH];
#pragma unroll
            for (int i = 0; i < PGX_ML_SET_BATCH; i++) {
                const uint64_t o = ob + (uint64_t)i * blockDim.x;
                if (o < v_hi && o >= s_off[k + 1]) k = pgx_ml_last_le(s_off, k + 1, nm, o);
                kk[i] = k;
            }
            if (FROM_IDS) {
#pragma unroll
                for (int i = 0; i < PGX_ML_SET_BATCH; i++) {
                    const uint64_t o = ob + (uint64_t)i * blockDim.x;
                    q[i] = o < v_hi ? ids[o - o_first] : ~0ull;
                }
            } else {
                uint64_t row[PGX_ML_SET_BATCH];
#pragma unroll
                for (int i = 0; i < PGX_ML_SET_BATCH; i++) {
                    const uint64_t o = ob + (uint64_t)i * blockDim.x;
                    row[i] = o < v_hi ? mems[wa + kk[i]].bwt_start + (o - s_off[kk[i]]) : ~0ull;
                }
#pragma unroll
                for (int i = 0; i < PGX_ML_SET_BATCH; i++) q[i] = row[i] < bwt_n ? sa32[row[i]] : ~0ull; // (always inside for a located MEM, pgx_ml_plan_kernel)
#pragma unroll
                for (int i = 0; i < PGX_ML_SET_BATCH; i++)
                    if (q[i] != ~0ull) q[i] = seq_lds ? pgx_ml_last_le(s_seq, 0, n_seq, q[i]) : pgx_ml_last_le(seq_start, 0, n_seq, q[i]);
            }
#pragma unroll
            for (int i = 0; i < PGX_ML_SET_BATCH; i++) {
                if (q[i] >= n_bits) continue; // (also the values beyond v_hi)
                const uint64_t w = kk[i] * W + (q[i] >> 6);
                if (w != key) {
                    if (acc) atomicOr(&s_set[key], acc);
                    key = w; acc = 0;
                }
                acc |= 1ull << (q[i] & 63);
            }
        }
        if (acc) atomicOr(&s_set[key], acc);
        __syncthreads();
        for (uint64_t t = threadIdx.x; t < nw; t += blockDim.x) {
            const unsigned long long v = s_set[t];
            if (!v) continue;
            const uint64_t j = t / W;
            unsigned long long *dst = sets + (wa + j - m0) * W + (t - j * W);
            if (s_off[j] >= o_begin && s_off[j + 1] <= o_end) *dst = v; // the whole MEM is this block's
            else atomicOr(dst, v);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
pgx_ml_sets_kernel(const pgx_mem *__restrict__ mems, const uint64_t *__restrict__ off, uint64_t m0, uint64_t m1, uint64_t o_first, uint64_t nv,
                   const uint32_t *__restrict__ sa32, uint64_t bwt_n, const uint64_t *__restrict__ seq_start, uint64_t n_seq, uint32_t W,
                   unsigned long long *__restrict__ sets) {
    pgx_ml_sets_body<false>(mems, off, m0, m1, o_first, nv, sa32, nullptr, bwt_n, seq_start, n_seq, W, sets);
}

__global__ void __launch_bounds__(256)
pgx_ml_sets_ids_kernel(const uint64_t *__restrict__ off, uint64_t m0, uint64_t m1, uint64_t o_first, uint64_t nv, const uint64_t *__restrict__ ids, uint32_t W,
                       unsigned long long *__restrict__ sets) {
    pgx_ml_sets_body<true>(nullptr, off, m0, m1, o_first, nv, nullptr, ids, 0, nullptr, 0, W, sets);
}

// ucount[i] = the number of set bits of MEM i's W words (np MEMs): Wp lanes a MEM (Wp = the power of two >= W), a wave holds 64 / Wp MEMs
__global__ void __launch_bounds__(256)
pgx_ml_set_count_kernel(const unsigned long long *__restrict__ sets, uint64_t np, uint32_t W, uint32_t Wp, uint64_t *__restrict__ ucount) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t i = t / Wp;
    const uint32_t j = (uint32_t)(t % Wp);
    int c = (i < np && j < W) ? __popcll(sets[i * W + j]) : 0;
    for (uint32_t d = 1; d < Wp; d <<= 1) c += __shfl_xor(c, (int)d, 64);
    if (i < np && j == 0) ucount[i] = (uint64_t)c;
}

// MEM i's set bits as ascending sequence ids at out[uloc[i] ..): a wave per MEM; lane = word for the load and the prefix of the popcounts,
// then lane = bit, one non-empty word after the other
__global__ void __launch_bounds__(256)
pgx_ml_set_expand_kernel(const unsigned long long *__restrict__ sets, uint64_t np, uint32_t W, const uint64_t *__restrict__ uloc, uint64_t *__restrict__ out) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (i >= np) return; // (a whole wave)
    const int lane = threadIdx.x & 63;
    const unsigned long long word = (uint32_t)lane < W ? sets[i * W + lane] : 0;
    int pre = __popcll(word); // -> exclusive prefix over the lanes
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(pre, d, 64);
        if (lane >= d) pre += up;
    }
    pre -= __popcll(word);
    const uint64_t base = uloc[i];
    unsigned long long nz = __ballot(word != 0);
    while (nz) {
        const int j = __ffsll((long long)nz) - 1;
        nz &= nz - 1;
        const unsigned long long wj = __shfl(word, j, 64);
        const int pj = __shfl(pre, j, 64);
        if ((wj >> lane) & 1ull) out[base + (uint64_t)pj + (uint64_t)__popcll(wj & ((1ull << lane) - 1ull))] = (uint64_t)j * 64 + (uint64_t)lane;
    }
}

// out[i] = i * stride, i < n
__global__ void __launch_bounds__(256)
pgx_ml_stride_kernel(uint64_t *__restrict__ out, uint64_t n, uint64_t stride) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i * stride;
}
