// pgx_rescue_kernels.hip -- the read rescue stage (include/pgx.h "read rescue") on gfx950.
//
//   targets    a thread a read: whether it is a target (the pair record of pgx_mates_kernel says whether a candidate pair is compatible and names the
//              mate's solo winner), its anchors, and -- behind a scan of the counts -- one task an anchor: the twin sequence and the clipped window
//   scan       a wave a task, a lane a diagonal, 64 consecutive diagonals a round.  Every lane walks the same coded read words (one scalar load a word);
//              its text word is the funnel shift of two neighbouring TEXT words as in pgx_verify_kernel, so the 64 lanes of a step touch 8 to 9
//              consecutive text words.  One XOR and the nibble fold give the mismatch mask of 8 positions, a popcount the matches, and seg_score is the
//              running maximum of E = max(E, 0) + (match ? 1 : -P), position by position without a branch: off the true diagonal three positions of four
//              mismatch, and a jump from mismatch to mismatch as in verify would diverge in nearly every word.  A lane folds its diagonals of all rounds
//              into the monoid of the header, a butterfly over the wave merges the lanes, lane 0 stores the task's result.
//   reduce     a thread a read: the results of its at most 8 tasks merged in anchor order, the record, the counters (one atomicAdd a wave each)
//   cands      MERGE, a thread a read: the candidate arrays of the rescued reads for pgx_verify_kernel, and the new list lengths
//   copy       MERGE, a thread a record: the old list and the verified rescued candidates into the new list
// A wave a task and a per-read pass behind it, not LDS: the tasks of a read need not lie in one block, a task's rounds need no exchange until its end,
// and the per-read pass moves 32 bytes a task.  No LDS, no inline assembly, vector stores only; every index is 64-bit.  Text words are loaded only for
// a read word that holds a position of the diagonal's span, which keeps the word index within [-1 (guarded), last word + 1] as in pgx_verify_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

namespace {

// n == 0 is the neutral element; the anchor is one within a task, so the smaller d wins a tie
__device__ __forceinline__ void rescue_merge(PgxRescueBest &x, const PgxRescueBest &y) {
    if (!y.n) return;
    if (!x.n) { x = y; return; }
    const bool same = y.score == x.score && y.matches == x.matches;
    const bool y_wins = y.score > x.score || (y.score == x.score && y.matches > x.matches) || (same && y.d < x.d);
    const PgxRescueBest &w = y_wins ? y : x, &l = y_wins ? x : y;
    const uint32_t below = l.score < w.score ? l.score : l.next; // what the loser knows below the winner's score
    PgxRescueBest r;
    r.d = w.d; r.score = w.score; r.matches = w.matches;
    r.next = w.next > below ? w.next : below;
    r.n_best = same ? x.n_best + y.n_best : w.n_best;
    r.n = x.n + y.n;
    r.pad = 0;
    x = r;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int mask = 32; mask; mask >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, mask, 64);
    return v;
}

} // namespace

__global__ void __launch_bounds__(256)
pgx_rescue_targets_kernel(const uint64_t *__restrict__ seq_start, uint32_t endmark, const uint64_t *__restrict__ read_off, const uint64_t *__restrict__ cand_off,
                          const pgx_read_verify *__restrict__ cands, const pgx_read_mates *__restrict__ mates, uint64_t n_reads, int64_t frag_min, int64_t frag_max,
                          uint32_t max_anchors, uint64_t *__restrict__ task_count, const uint64_t *__restrict__ task_off, PgxRescueTask *__restrict__ tasks) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_reads) return;
    const uint64_t a = t ^ 1ull;
    const uint64_t nt = cand_off[t + 1] - cand_off[t], a0 = cand_off[a], na = cand_off[a + 1] - a0;
    const pgx_read_mates *m = mates + (t >> 1);
    uint32_t n_anch = 0;
    if (m->n_compatible == 0 && na > 0 && nt < PGX_VERIFY_MAX_CAND) {
        const uint32_t solo = (a & 1) ? m->solo_b : m->solo_a;
        const uint32_t ks = cands[a0 + solo].seg_score, km = cands[a0 + solo].matches;
        const int64_t len = (int64_t)(read_off[t + 1] - read_off[t]);
        for (uint64_t i = 0; i < na && n_anch < max_anchors; i++) {
            const pgx_read_verify *c = cands + a0 + i;
            if (c->seg_score != ks || c->matches != km) continue;
            if (tasks) {
                const uint32_t s = c->seq ^ 1u;
                const int64_t Ls = (int64_t)(seq_start[(uint64_t)s + 1] - seq_start[s]) - (int64_t)endmark;
                const int64_t base = Ls - c->diag; // (the host held frag_min and frag_max where base - frag cannot overflow)
                int64_t d_lo = base - frag_max, d_hi = base - frag_min;
                if (d_lo < -(len - 1)) d_lo = -(len - 1);
                if (d_hi > Ls - 1) d_hi = Ls - 1;
                if (len == 0 || d_hi < d_lo) { d_lo = 0; d_hi = -1; }
                PgxRescueTask k;
                k.d_lo = d_lo; k.d_hi = d_hi; k.read = t; k.seq = s; k.anchor = (uint32_t)i;
                tasks[task_off[t] + n_anch] = k;
            }
            n_anch++;
        }
    }
    if (!tasks) task_count[t] = n_anch;
}

__global__ void __launch_bounds__(PGX_RESCUE_THREADS)
pgx_rescue_scan_kernel(const uint32_t *__restrict__ text4, const uint64_t *__restrict__ seq_start, uint32_t endmark, const uint32_t *__restrict__ rcode,
                       const uint64_t *__restrict__ read_off, const PgxRescueTask *__restrict__ tasks, uint64_t n_tasks, uint32_t penalty,
                       PgxRescueBest *__restrict__ best) {
    const uint32_t lane = threadIdx.x & 63u;
    // (the task of the wave, as scalars: what follows from it is loaded once a wave)
    const uint64_t k = (uint64_t)blockIdx.x * (PGX_RESCUE_THREADS / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (k >= n_tasks) return;
    const PgxRescueTask task = tasks[k];
    const uint64_t roff = read_off[task.read];
    const int64_t len = (int64_t)(read_off[task.read + 1] - roff);
    const uint64_t s0 = seq_start[task.seq];
    const int64_t Ls = (int64_t)(seq_start[(uint64_t)task.seq + 1] - s0) - (int64_t)endmark;
    const int32_t P = (int32_t)penalty;
    PgxRescueBest acc{0, 0, 0, 0, 0, 0, 0};
    for (int64_t d0 = task.d_lo; d0 <= task.d_hi; d0 += 64) { // (a non-empty window: len >= 1)
        const int64_t d = d0 + (int64_t)lane;
        const bool on = d <= task.d_hi;
        int64_t lo = d < 0 ? -d : 0;
        int64_t hi = Ls - d < len ? Ls - d : len;
        if (!on || hi <= lo) lo = hi = 0;
        const uint64_t g0 = roff + (uint64_t)lo, g1 = roff + (uint64_t)hi; // the span as bytes of the concatenated reads
        const int64_t delta = (int64_t)s0 + d - (int64_t)roff;             // read byte g lies on text symbol g + delta
        int32_t E = 0, top = 0;
        uint32_t matches = 0;
        for (uint64_t w = roff >> 3; w <= (roff + (uint64_t)len - 1) >> 3; w++) {
            const uint32_t rc = rcode[w];
            if (hi > lo && 8 * w + 8 > g0 && 8 * w < g1) {
                const int64_t t0 = (int64_t)(8 * w) + delta, tw = t0 >> 3; // (arithmetic shift: floor)
                const uint32_t sh = 4u * (uint32_t)(t0 & 7);
                const uint32_t ta = tw >= 0 ? text4[tw] : 0u, tb = text4[tw + 1];
                const uint32_t tword = (uint32_t)((((uint64_t)tb << 32) | ta) >> sh);
                uint32_t x = rc ^ tword;
                x = (x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x11111111u; // bit 4 j: position j of the word is a mismatch
                const uint32_t k0 = 8 * w < g0 ? (uint32_t)(g0 - 8 * w) : 0u, k1 = g1 - 8 * w < 8 ? (uint32_t)(g1 - 8 * w) : 8u;
                const uint32_t in = ((k1 == 8 ? 0xFFFFFFFFu : (1u << (4u * k1)) - 1u) & ~((1u << (4u * k0)) - 1u)) & 0x11111111u; // the positions of the span
                matches += (uint32_t)__popc(~x & in);
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) {
                    const uint32_t bit = 1u << (4u * j);
                    const int32_t e = (E > 0 ? E : 0) + ((x & bit) ? -P : 1);
                    E = (in & bit) ? e : E;
                    top = E > top ? E : top;
                }
            }
        }
        if (on) rescue_merge(acc, PgxRescueBest{d, (uint32_t)top, matches, 0, 1, 1, 0});
    }
    for (int mask = 32; mask; mask >>= 1) {
        PgxRescueBest y;
        y.d = __shfl_xor((long long)acc.d, mask, 64);
        y.score = (uint32_t)__shfl_xor((int)acc.score, mask, 64);
        y.matches = (uint32_t)__shfl_xor((int)acc.matches, mask, 64);
        y.next = (uint32_t)__shfl_xor((int)acc.next, mask, 64);
        y.n_best = (uint32_t)__shfl_xor((int)acc.n_best, mask, 64);
        y.n = (uint32_t)__shfl_xor((int)acc.n, mask, 64);
        y.pad = 0;
        rescue_merge(acc, y);
    }
    if (lane == 0) best[k] = acc;
}

__global__ void __launch_bounds__(256)
pgx_rescue_reduce_kernel(const uint64_t *__restrict__ cand_off, const pgx_read_mates *__restrict__ mates, const uint64_t *__restrict__ task_count,
                         const uint64_t *__restrict__ task_off, const PgxRescueTask *__restrict__ tasks, const PgxRescueBest *__restrict__ best, uint64_t n_reads,
                         uint32_t min_score, pgx_read_rescue *__restrict__ out, uint64_t *__restrict__ rescued, unsigned long long *__restrict__ counters) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = t < n_reads;
    bool target = false, full = false, resc = false;
    uint64_t n_tasks = 0, n = 0;
    if (live) {
        const uint64_t a = t ^ 1ull;
        const uint64_t nt = cand_off[t + 1] - cand_off[t], na = cand_off[a + 1] - cand_off[a];
        const bool open = mates[t >> 1].n_compatible == 0 && na > 0;
        full = open && nt >= PGX_VERIFY_MAX_CAND;
        target = open && !full;
        n_tasks = task_count[t];
        // the tasks in anchor order: a later one wins only with a larger (score, matches)
        int64_t d = 0;
        uint64_t n_best = 0;
        uint32_t score = 0, matches = 0, next = 0, seq = PGX_NO_SEQUENCE, anchor = 0;
        for (uint64_t i = 0; i < n_tasks; i++) {
            const PgxRescueBest y = best[task_off[t] + i];
            if (!y.n) continue;
            if (!n) {
                d = y.d; score = y.score; matches = y.matches; next = y.next; n_best = y.n_best;
                seq = tasks[task_off[t] + i].seq; anchor = tasks[task_off[t] + i].anchor;
            } else {
                const bool same = y.score == score && y.matches == matches;
                const bool y_wins = y.score > score || (y.score == score && y.matches > matches);
                const uint32_t ws = y_wins ? y.score : score, wn = y_wins ? y.next : next;
                const uint32_t ls = y_wins ? score : y.score, ln = y_wins ? next : y.next;
                const uint32_t below = ls < ws ? ls : ln;
                next = wn > below ? wn : below;
                n_best = same ? n_best + y.n_best : (y_wins ? (uint64_t)y.n_best : n_best);
                if (y_wins) {
                    d = y.d; score = y.score; matches = y.matches;
                    seq = tasks[task_off[t] + i].seq; anchor = tasks[task_off[t] + i].anchor;
                }
            }
            n += y.n;
        }
        resc = target && n > 0 && score >= min_score;
        pgx_read_rescue r;
        r.diag = d; r.n_diags = n; r.seq = seq;
        r.flags = (target ? PGX_RESCUE_TARGET : 0u) | (resc ? PGX_RESCUE_RESCUED : 0u) | (full ? PGX_RESCUE_FULL : 0u);
        r.anchor = anchor; r.n_anchors = (uint32_t)n_tasks; r.seg_score = score; r.matches = matches;
        r.n_best = n_best > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n_best; r.next_score = next;
        r.reserved[0] = r.reserved[1] = r.reserved[2] = r.reserved[3] = 0;
        out[t] = r;
        if (rescued) rescued[t] = resc ? 1 : 0;
    }
    const unsigned long long v0 = __ballot(target), v1 = __ballot(resc), v2 = __ballot(full);
    const uint64_t s3 = wave_sum(n_tasks), s4 = wave_sum(n);
    if ((threadIdx.x & 63u) == 0) {
        if (v0) atomicAdd(counters + 0, (unsigned long long)__popcll(v0));
        if (v1) atomicAdd(counters + 1, (unsigned long long)__popcll(v1));
        if (v2) atomicAdd(counters + 2, (unsigned long long)__popcll(v2));
        if (s3) atomicAdd(counters + 3, (unsigned long long)s3);
        if (s4) atomicAdd(counters + 4, (unsigned long long)s4);
    }
}

__global__ void __launch_bounds__(256)
pgx_rescue_cands_kernel(const pgx_read_rescue *__restrict__ recs, const uint64_t *__restrict__ cand_off, const uint64_t *__restrict__ rescued,
                        const uint64_t *__restrict__ res_off, uint64_t n_reads, uint64_t *__restrict__ cand_read, uint32_t *__restrict__ cand_seq,
                        int64_t *__restrict__ cand_diag, uint64_t *__restrict__ fake_off, uint64_t *__restrict__ new_count) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_reads) return;
    const uint64_t nt = cand_off[t + 1] - cand_off[t];
    new_count[t] = nt + rescued[t];
    if (!rescued[t]) return;
    const uint64_t j = res_off[t];
    cand_read[j] = t; cand_seq[j] = recs[t].seq; cand_diag[j] = recs[t].diag;
    fake_off[t] = j - nt; // (pgx_verify_kernel: n_cand = j - fake_off[t] = the ordinal behind the read's list; modulo 2^64)
}

__global__ void __launch_bounds__(256)
pgx_rescue_copy_kernel(const pgx_read_verify *__restrict__ old_cands, const uint64_t *__restrict__ old_off, const uint64_t *__restrict__ old_read, uint64_t n_old,
                       const pgx_read_verify *__restrict__ res_cands, const uint64_t *__restrict__ res_read, uint64_t n_res, const uint64_t *__restrict__ new_off,
                       pgx_read_verify *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_old) {
        const uint64_t r = old_read[i];
        out[new_off[r] + (i - old_off[r])] = old_cands[i];
    } else if (i - n_old < n_res) {
        const uint64_t r = res_read[i - n_old];
        out[new_off[r + 1] - 1] = res_cands[i - n_old];
    }
}
