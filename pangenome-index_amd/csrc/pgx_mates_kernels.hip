// pgx_mates_kernels.hip -- the read mates stage (include/pgx.h "read mates") as one gfx950 kernel.
//
//   mates      a pair takes a group of G = 2^g_shift lanes of a wave64, G >= the candidates of either mate; a wave serves 64 / G pairs.  Lane i of the
//              group holds candidate i of A and candidate i of B (four fields of each 64-byte list record).  It loops over j, takes B's candidate j by
//              a shuffle inside the group, tests compatibility and folds the monoid of the header; the loop ends for the whole wave behind the longest
//              B list of its groups.  Two butterflies over the group reduce the solo winners and the monoid, so that every lane of the group holds the
//              result.  The group writes the 16 words of its record, lane w word w (with G < 16 in 16 / G rounds): the records of a wave are one
//              contiguous stretch.  With PGX_MATES_ELECT the lanes also copy the 2 x 16 words of the two chosen list records over the pair's winner
//              records, with n_cand, cand_index and n_tied (a ballot over the group) put in.  The four counters take one atomicAdd a wave each.
// No LDS, no inline assembly, vector stores only; every index is 64-bit.  Lanes of a group behind the last pair take part in every shuffle and store nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

namespace {

// the monoid over compatible pairs: n == 0 is the neutral element
struct MatesBest {
    uint64_t s, m;  // score sum and matches sum of the best pair
    uint64_t next;  // the largest score sum below s (0: none)
    uint32_t ij;    // i << 6 | j of the best pair: the smaller wins a tie in both sums
    uint32_t n_best, n;
};

__device__ __forceinline__ void mates_merge(MatesBest &x, const MatesBest &y) {
    if (!y.n) return;
    if (!x.n) { x = y; return; }
    const bool same = y.s == x.s && y.m == x.m;
    const bool y_wins = y.s > x.s || (y.s == x.s && y.m > x.m) || (same && y.ij < x.ij);
    const MatesBest &w = y_wins ? y : x, &l = y_wins ? x : y;
    const uint64_t below = l.s < w.s ? l.s : l.next; // what the loser knows below the winner's score
    MatesBest r;
    r.s = w.s; r.m = w.m; r.ij = w.ij;
    r.next = w.next > below ? w.next : below;
    r.n_best = same ? x.n_best + y.n_best : w.n_best;
    r.n = x.n + y.n;
    x = r;
}

// a solo winner: largest key = seg_score << 32 | matches, then the smallest ordinal; idx == ~0: no candidate
struct MatesSolo {
    uint64_t key;
    uint32_t idx;
};

__device__ __forceinline__ MatesSolo mates_solo(uint64_t key, uint32_t idx, uint32_t G) {
    MatesSolo x{key, idx};
    for (uint32_t mask = G >> 1; mask; mask >>= 1) {
        const uint64_t k = (uint64_t)__shfl_xor((unsigned long long)x.key, (int)mask, 64);
        const uint32_t i = (uint32_t)__shfl_xor((int)x.idx, (int)mask, 64);
        if (i != ~0u && (x.idx == ~0u || k > x.key || (k == x.key && i < x.idx))) { x.key = k; x.idx = i; }
    }
    return x;
}

__device__ __forceinline__ uint32_t mates_sat(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

} // namespace

__global__ void __launch_bounds__(PGX_MATES_THREADS)
pgx_mates_kernel(const uint64_t *__restrict__ seq_start, uint32_t endmark, const uint64_t *__restrict__ cand_off, const pgx_read_verify *__restrict__ cands, uint64_t n_pairs,
                 uint32_t g_shift, int64_t frag_min, int64_t frag_max, uint32_t penalty, uint32_t flags, pgx_read_mates *__restrict__ out,
                 pgx_read_verify *__restrict__ winners, unsigned long long *__restrict__ counters) {
    const uint32_t G = 1u << g_shift, lane = threadIdx.x & 63u, lig = lane & (G - 1);
    const uint64_t p = ((uint64_t)blockIdx.x * PGX_MATES_THREADS + threadIdx.x) >> g_shift;
    const bool live = p < n_pairs;
    uint64_t a0 = 0, b0 = 0;
    uint32_t na = 0, nb = 0;
    if (live) {
        a0 = cand_off[2 * p]; b0 = cand_off[2 * p + 1];
        const uint64_t b1 = cand_off[2 * p + 2];
        na = (uint32_t)(b0 - a0 < G ? b0 - a0 : G); // (the host sized G for the longest list)
        nb = (uint32_t)(b1 - b0 < G ? b1 - b0 : G);
    }
    // candidate lig of A and of B
    const bool ha = lig < na, hb = lig < nb;
    uint32_t a_seq = 0, b_seq = 0;
    uint64_t a_key = 0, b_key = 0; // seg_score << 32 | matches
    long long a_base = 0, b_diag = 0; // L[seq] - diag of A's; diag of B's
    if (ha) {
        const pgx_read_verify *c = cands + a0 + lig;
        a_seq = c->seq;
        a_key = (uint64_t)c->seg_score << 32 | c->matches;
        a_base = (long long)(seq_start[(uint64_t)a_seq + 1] - seq_start[a_seq] - endmark) - (long long)c->diag;
    }
    if (hb) {
        const pgx_read_verify *c = cands + b0 + lig;
        b_seq = c->seq;
        b_key = (uint64_t)c->seg_score << 32 | c->matches;
        b_diag = (long long)c->diag;
    }
    const MatesSolo solo_a = mates_solo(a_key, ha ? lig : ~0u, G), solo_b = mates_solo(b_key, hb ? lig : ~0u, G);
    // this lane's row of the i x j grid
    MatesBest best{0, 0, 0, 0, 0, 0};
    for (uint32_t j = 0; j < G; j++) {
        if (!__any(j < nb)) break; // (the same for the whole wave)
        const uint32_t q = (uint32_t)__shfl((int)b_seq, (int)j, (int)G);
        const uint64_t k = (uint64_t)__shfl((unsigned long long)b_key, (int)j, (int)G);
        const long long frag = a_base - __shfl(b_diag, (int)j, (int)G);
        if (ha && j < nb && (a_seq ^ 1u) == q && frag >= frag_min && frag <= frag_max)
            mates_merge(best, MatesBest{(a_key >> 32) + (k >> 32), (a_key & 0xFFFFFFFFull) + (k & 0xFFFFFFFFull), 0, lig << 6 | j, 1, 1});
    }
    for (uint32_t mask = G >> 1; mask; mask >>= 1) {
        MatesBest y;
        y.s = (uint64_t)__shfl_xor((unsigned long long)best.s, (int)mask, 64);
        y.m = (uint64_t)__shfl_xor((unsigned long long)best.m, (int)mask, 64);
        y.next = (uint64_t)__shfl_xor((unsigned long long)best.next, (int)mask, 64);
        y.ij = (uint32_t)__shfl_xor((int)best.ij, (int)mask, 64);
        y.n_best = (uint32_t)__shfl_xor((int)best.n_best, (int)mask, 64);
        y.n = (uint32_t)__shfl_xor((int)best.n, (int)mask, 64);
        mates_merge(best, y);
    }
    // the choice
    const bool has_a = na > 0, has_b = nb > 0, compatible = best.n > 0;
    const uint64_t solo_score = (has_a ? solo_a.key >> 32 : 0) + (has_b ? solo_b.key >> 32 : 0);
    const bool proper = compatible && best.s + penalty >= solo_score;
    const uint32_t sa = has_a ? solo_a.idx : 0, sb = has_b ? solo_b.idx : 0;
    const uint32_t ca = proper ? best.ij >> 6 : sa, cb = proper ? best.ij & 63u : sb;
    const uint32_t seq_a = (uint32_t)__shfl((int)a_seq, (int)ca, (int)G), seq_b = (uint32_t)__shfl((int)b_seq, (int)cb, (int)G);
    const long long frag = __shfl(a_base, (int)(best.ij >> 6), (int)G) - __shfl(b_diag, (int)(best.ij & 63u), (int)G);
    const bool moved_a = proper && ca != sa, moved_b = proper && cb != sb;
    const uint32_t rflags = (proper ? PGX_MATES_PROPER : 0u) | (compatible ? PGX_MATES_COMPATIBLE : 0u) | (has_a ? PGX_MATES_HAS_A : 0u) | (has_b ? PGX_MATES_HAS_B : 0u) |
                            (moved_a ? PGX_MATES_MOVED_A : 0u) | (moved_b ? PGX_MATES_MOVED_B : 0u);
    if (live) {
        uint32_t *o = reinterpret_cast<uint32_t *>(out + p);
        for (uint32_t w = lig; w < 16; w += G) {
            uint32_t v = 0;
            switch (w) {
            case 0: v = compatible ? (uint32_t)(uint64_t)frag : 0u; break;
            case 1: v = compatible ? (uint32_t)((uint64_t)frag >> 32) : 0u; break;
            case 2: v = mates_sat(best.s); break;
            case 3: v = mates_sat(solo_score); break;
            case 4: v = ca; break;
            case 5: v = cb; break;
            case 6: v = sa; break;
            case 7: v = sb; break;
            case 8: v = best.n; break;
            case 9: v = best.n_best; break;
            case 10: v = mates_sat(best.next); break;
            case 11: v = mates_sat(best.m); break;
            case 12: v = has_a ? seq_a : PGX_NO_SEQUENCE; break;
            case 13: v = has_b ? seq_b : PGX_NO_SEQUENCE; break;
            case 14: v = rflags; break;
            default: break;
            }
            o[w] = v;
        }
    }
    if (flags & PGX_MATES_ELECT) {
        // candidates of a read that equal the chosen one in (seg_score, matches): a ballot, cut to the group
        const unsigned long long gmask = (G == 64 ? ~0ull : (1ull << G) - 1) << (lane & ~(G - 1));
        const uint64_t ka = (uint64_t)__shfl((unsigned long long)a_key, (int)ca, (int)G), kb = (uint64_t)__shfl((unsigned long long)b_key, (int)cb, (int)G);
        const uint32_t tied_a = (uint32_t)__popcll(__ballot(ha && a_key == ka) & gmask), tied_b = (uint32_t)__popcll(__ballot(hb && b_key == kb) & gmask);
        if (live) {
            for (uint32_t w = lig; w < 32; w += G) {
                const bool second = w >= 16;
                const uint32_t k = w & 15u, n_c = second ? nb : na, ch = second ? cb : ca;
                uint32_t v;
                if (!n_c) v = k == 2 ? PGX_NO_SEQUENCE : 0u; // the record of a read without a candidate
                else if (k == 3) v = n_c;
                else if (k == 14) v = ch;
                else if (k == 15) v = second ? tied_b : tied_a;
                else v = reinterpret_cast<const uint32_t *>(cands + (second ? b0 : a0) + ch)[k];
                reinterpret_cast<uint32_t *>(winners + 2 * p + (second ? 1 : 0))[k] = v;
            }
        }
    }
    const bool lead = live && lig == 0;
    const unsigned long long v0 = __ballot(lead && proper), v1 = __ballot(lead && compatible), v2 = __ballot(lead && moved_a), v3 = __ballot(lead && moved_b);
    if (lane == 0) {
        if (v0) atomicAdd(counters + 0, (unsigned long long)__popcll(v0));
        if (v1) atomicAdd(counters + 1, (unsigned long long)__popcll(v1));
        if (v2) atomicAdd(counters + 2, (unsigned long long)__popcll(v2));
        if (v3) atomicAdd(counters + 3, (unsigned long long)__popcll(v3));
    }
}
