// pgx_mapq_kernels.hip -- the read mapq stage (include/pgx.h "read mapq") as gfx950 kernels.
//
//   choose_extras   a thread a read: the placements of the place list with score == next_score > 0, the first min(max_extra, 64 - n_list) of them; called
//              twice around the project's scan like pgx_verify_choose_kernel: to count (and to say whether more exist than were taken), then to fill the
//              candidate arrays that pgx_verify_kernel takes.
//   mapq       a group of G = 2^g_shift lanes of a wave64 serves a read, or a pair of mates under PGX_MAPQ_PAIRED; G >= the entries of the read (of either
//              mate).  Lane i holds entry i: sequence, diagonal, seg_score and, behind one rank, one back scan and one nodes[] load in the WALK image, its
//              locus.  Under PAIRED a first loop over j takes the mate's list candidate j by shuffles inside the group and folds the best compatible
//              partner into the lane's score.  The main loop over j takes entry j by shuffles and gathers, per lane, the mask of the entries of its class,
//              the class maximum and whether the lane lies within `slack` diagonals of an entry of the chosen's class; both loops end for the whole wave
//              behind the longest list of its groups.  Ballots cut to the group turn the masks into the counts, two butterflies give the excess and the
//              best competing score, a binary search over K gives mapq.  The group stores the 8 words of its record, lane w word w (with G < 8 in
//              8 / G rounds).  The four counters take one atomicAdd a wave each.
// No LDS, no inline assembly, vector stores only; every index is 64-bit.  Lanes of a group behind the last read take part in every shuffle and store nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"
#include "pgx_walk_device.h"

namespace {

__constant__ uint32_t MAPQ_T[50] = PGX_MAPQ_T;
__constant__ uint64_t MAPQ_K[61] = PGX_MAPQ_K;

#define MAPQ_NO_LOCUS 0xFFFFFFFFu

// what a lane holds of its entry of one read, and what the group knows of the read
struct MapqEntry {
    uint64_t node;     // the oriented node under the anchor
    long long diag, base, score; // base: L[seq] - diag (frag = base - the partner's diag); score: seg_score, plus the mate's term under PAIRED
    uint32_t seq, off; // off: the offset in the node, MAPQ_NO_LOCUS without a locus
    uint32_t seg;      // seg_score
    bool has, list;
    // the same in every lane of the group
    uint64_t r;
    uint32_t n, n_list, chosen; // chosen: PGX_MAPQ_NO_CHOSEN without one
    bool paired;                // the mate has a list candidate
};

__device__ __forceinline__ uint32_t mapq_weight(uint32_t scale, uint64_t d) { return MAPQ_T[d >= 50 ? 49u : (uint32_t)(scale * d > 49 ? 49 : scale * d)]; }

__device__ __forceinline__ void mapq_load(const PgxMapqArgs &a, bool live, uint64_t r, uint32_t lig, uint32_t G, MapqEntry &e) {
    e.r = r;
    e.node = 0; e.diag = 0; e.base = 0; e.score = 0; e.seq = 0; e.off = MAPQ_NO_LOCUS; e.seg = 0;
    e.n = e.n_list = 0; e.chosen = PGX_MAPQ_NO_CHOSEN; e.paired = false;
    uint64_t a0 = 0, b0 = 0, n_a = 0;
    if (live) {
        a0 = a.off_a[r];
        n_a = a.off_a[r + 1] - a0;
        uint64_t n = n_a;
        if (a.off_b) { b0 = a.off_b[r]; n += a.off_b[r + 1] - b0; }
        const uint64_t n_list = a.list_len ? a.list_len[r] : n_a;
        e.n = (uint32_t)(n < G ? n : G); // (the host sized G for the longest list)
        e.n_list = (uint32_t)(n_list < e.n ? n_list : e.n);
        uint32_t c = a.winners ? (a.winners[r].seq == PGX_NO_SEQUENCE ? PGX_MAPQ_NO_CHOSEN : a.winners[r].cand_index) : a.chosen[r];
        e.chosen = c < e.n_list ? c : PGX_MAPQ_NO_CHOSEN;
    }
    e.has = lig < e.n; e.list = lig < e.n_list;
    uint32_t span_lo = 0, span_hi = 0, seg_start = 0;
    uint64_t s0 = 0, ls = 0;
    if (e.has) {
        const pgx_read_verify *c = lig < n_a ? a.recs_a + a0 + lig : a.recs_b + b0 + (lig - n_a);
        e.seq = c->seq; e.diag = (long long)c->diag; e.seg = c->seg_score;
        span_lo = c->span_lo; span_hi = c->span_hi; seg_start = c->seg_start;
        s0 = a.seq_start[e.seq];
        ls = a.seq_start[(uint64_t)e.seq + 1] - s0 - a.endmark;
        e.base = (long long)(ls - (uint64_t)e.diag);
        e.score = (long long)e.seg;
    }
    // the anchor is the chosen entry's seg_start; the locus is what lies under it on this lane's diagonal
    const uint32_t anchor = (uint32_t)__shfl((int)seg_start, (int)(e.chosen == PGX_MAPQ_NO_CHOSEN ? 0u : e.chosen), (int)G);
    if (e.has && e.chosen != PGX_MAPQ_NO_CHOSEN && span_lo <= anchor && anchor < span_hi) {
        const uint64_t t = (uint64_t)e.diag + anchor; // (inside the sequence for a record of verify; tested, as the arrays route's records are stated)
        if (t < ls) {
            const uint64_t p = s0 + t, k = walk_rank(a.walk, p + 1);
            if (k >= 1) {
                e.node = a.walk.nodes[k - 1];
                e.off = (uint32_t)(p - walk_prev_mark(a.walk, p, s0));
            }
        }
    }
}

// PAIRED: the mate's term m_i of every entry of `e`, from the list candidates of `mate` (include/pgx.h "read mapq", score)
__device__ __forceinline__ void mapq_pair(const PgxMapqArgs &a, MapqEntry &e, const MapqEntry &mate, uint32_t G) {
    uint32_t solo = mate.list ? mate.seg : 0u; // the solo winner's seg_score: the largest of the list
    for (uint32_t mask = G >> 1; mask; mask >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)solo, (int)mask, 64);
        solo = o > solo ? o : solo;
    }
    long long m = (long long)solo - (long long)a.penalty;
    for (uint32_t j = 0; j < G; j++) {
        if (!__any(j < mate.n_list)) break; // (the same for the whole wave)
        const uint32_t q = (uint32_t)__shfl((int)mate.seq, (int)j, (int)G), s = (uint32_t)__shfl((int)mate.seg, (int)j, (int)G);
        const long long frag = (long long)((uint64_t)e.base - (uint64_t)__shfl(mate.diag, (int)j, (int)G));
        if (j < mate.n_list && (e.seq ^ 1u) == q && frag >= a.frag_min && frag <= a.frag_max && (long long)s > m) m = (long long)s;
    }
    e.paired = mate.n_list > 0;
    if (e.has && e.paired) e.score += m;
}

// the record of one read from the entries the lanes of its group hold; returns mapq and the flags in every lane of the group
__device__ __forceinline__ void mapq_read(const PgxMapqArgs &a, const MapqEntry &e, uint32_t lane, uint32_t lig, uint32_t G, uint32_t &mapq, uint32_t &rflags, bool &unique) {
    const uint32_t gbase = lane & ~(G - 1);
    const unsigned long long gmask = G == 64 ? ~0ull : (1ull << G) - 1;
    const bool chosen = e.chosen != PGX_MAPQ_NO_CHOSEN;
    const int cl = (int)(chosen ? e.chosen : 0u);
    const uint64_t node_c = (uint64_t)__shfl((unsigned long long)e.node, cl, (int)G);
    const uint32_t off_c = (uint32_t)__shfl((int)e.off, cl, (int)G);
    const long long s_w = __shfl(e.score, cl, (int)G);
    // the chosen's class: the chosen entry and the entries that share its locus
    const bool in_w = e.has && chosen && (lig == e.chosen || (e.off != MAPQ_NO_LOCUS && e.off == off_c && e.node == node_c));
    const unsigned long long wmask = (__ballot(in_w) >> gbase) & gmask;
    unsigned long long same = e.has ? 1ull << lig : 0ull; // the entries of this lane's class
    long long cmax = e.score;                             // and their largest score
    bool near = false;                                    // within `slack` diagonals of an entry of the chosen's class, on its sequence
    for (uint32_t j = 0; j < G; j++) {
        if (!__any(j < e.n)) break; // (the same for the whole wave)
        const uint64_t nj = (uint64_t)__shfl((unsigned long long)e.node, (int)j, (int)G);
        const uint32_t oj = (uint32_t)__shfl((int)e.off, (int)j, (int)G), qj = (uint32_t)__shfl((int)e.seq, (int)j, (int)G);
        const long long sj = __shfl(e.score, (int)j, (int)G), dj = __shfl(e.diag, (int)j, (int)G);
        if (e.has && j < e.n) {
            if (j != lig && e.off != MAPQ_NO_LOCUS && oj == e.off && nj == e.node) {
                same |= 1ull << j;
                cmax = sj > cmax ? sj : cmax;
            }
            const uint64_t apart = e.diag > dj ? (uint64_t)e.diag - (uint64_t)dj : (uint64_t)dj - (uint64_t)e.diag;
            if (((wmask >> j) & 1ull) && qj == e.seq && apart != 0 && apart <= a.slack) near = true;
        }
    }
    const unsigned long long nearmask = (__ballot(near) >> gbase) & gmask;
    const bool adjacent = e.has && !in_w && (same & nearmask) != 0;
    const bool rep = e.has && (same & ((1ull << lig) - 1ull)) == 0; // the first entry of its class
    const bool comp = rep && !in_w && !adjacent;
    const uint32_t n_loci = (uint32_t)__popcll((__ballot(rep) >> gbase) & gmask), n_with = (uint32_t)__popcll((__ballot(in_w || adjacent) >> gbase) & gmask),
                   n_comp = (uint32_t)__popcll((__ballot(comp) >> gbase) & gmask);
    const bool outscored = ((__ballot(comp && cmax > s_w) >> gbase) & gmask) != 0;
    uint64_t excess = comp ? mapq_weight(a.scale, cmax >= s_w ? 0ull : (uint64_t)(s_w - cmax)) : 0u;
    long long other = comp ? cmax : INT64_MIN;
    for (uint32_t mask = G >> 1; mask; mask >>= 1) {
        excess += (uint64_t)__shfl_xor((unsigned long long)excess, (int)mask, 64);
        const long long o = __shfl_xor(other, (int)mask, 64);
        other = o > other ? o : other;
    }
    rflags = PGX_MAPQ_HAS | (off_c != MAPQ_NO_LOCUS ? PGX_MAPQ_LOCUS : 0u) | (e.paired ? PGX_MAPQ_PAIRED : 0u) | (outscored ? PGX_MAPQ_OUTSCORED : 0u);
    if (chosen && a.rescue && e.chosen + 1 == e.n_list) { // the candidate a rescue merge appended: the diagonals of its window compete
        const pgx_read_rescue *rr = a.rescue + e.r;
        if (rr->flags & PGX_RESCUE_RESCUED) {
            const uint32_t n_best = rr->n_best, seg = rr->seg_score, next = rr->next_score;
            excess += (uint64_t)(n_best ? n_best - 1u : 0u) << 16;
            if (next > 0) excess += mapq_weight(a.scale, seg > next ? (uint64_t)(seg - next) : 0ull);
            rflags |= PGX_MAPQ_RESCUED;
        }
    }
    if (chosen && ((a.max_cand && e.n_list >= a.max_cand) || (a.more && a.more[e.r]))) rflags |= PGX_MAPQ_CAPPED;
    // the largest q with E K[q] <= (E + 65536) 65536; E held at 2^26 (mapq is 0 long before)
    const uint64_t ec = excess < (1ull << 26) ? excess : 1ull << 26;
    uint32_t lo = 0, hi = 60;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (ec * MAPQ_K[mid] <= (ec + 65536ull) << 16) lo = mid;
        else hi = mid - 1;
    }
    mapq = chosen ? lo : 0u;
    if (!chosen) rflags = 0;
    unique = chosen && excess == 0;
    if (e.r < a.n_reads) {
        uint32_t *o = reinterpret_cast<uint32_t *>(a.out + e.r);
        for (uint32_t w = lig; w < 8; w += G) {
            uint32_t v = 0;
            switch (w) {
            case 0: v = mapq; break;
            case 1: v = rflags; break;
            case 2: v = e.n; break;
            case 3: v = n_loci; break;
            case 4: v = n_with; break;
            case 5: v = n_comp; break;
            case 6: v = n_comp ? (other < 0 ? 0u : other > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)other) : 0u; break;
            default: v = excess > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)excess; break;
            }
            o[w] = chosen ? v : 0u;
        }
    }
}

} // namespace

__global__ void __launch_bounds__(256)
pgx_mapq_choose_extras_kernel(const pgx_read_place *__restrict__ recs, const uint64_t *__restrict__ place_off, const pgx_placement *__restrict__ places,
                              const uint64_t *__restrict__ cand_off, uint64_t n_reads, uint32_t max_extra, uint64_t *__restrict__ count, uint32_t *__restrict__ more,
                              const uint64_t *__restrict__ extra_off, uint32_t *__restrict__ cand_seq, int64_t *__restrict__ cand_diag) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint64_t next = recs[r].next_score, n_list = cand_off[r + 1] - cand_off[r];
    const uint64_t room = n_list >= PGX_MAPQ_MAX_ENTRIES ? 0 : (max_extra < PGX_MAPQ_MAX_ENTRIES - n_list ? max_extra : PGX_MAPQ_MAX_ENTRIES - n_list);
    uint64_t k = 0;
    uint32_t over = 0;
    if (next > 0) {
        for (uint64_t p = place_off[r]; p < place_off[r + 1]; p++)
            if (places[p].score == next) {
                if (k >= room) { over = 1; break; }
                if (cand_seq) { cand_seq[extra_off[r] + k] = places[p].seq; cand_diag[extra_off[r] + k] = places[p].diag; }
                k++;
            }
    }
    if (!cand_seq) { count[r] = k; more[r] = over; }
}

template <bool PAIRED>
__global__ void __launch_bounds__(PGX_MAPQ_THREADS)
pgx_mapq_kernel(PgxMapqArgs a) {
    const uint32_t G = 1u << a.g_shift, lane = threadIdx.x & 63u, lig = lane & (G - 1);
    const uint64_t u = ((uint64_t)blockIdx.x * PGX_MAPQ_THREADS + threadIdx.x) >> a.g_shift; // the read, or the pair
    const bool live = u < (PAIRED ? a.n_reads / 2 : a.n_reads);
    uint32_t mapq = 0, rflags = 0, sum = 0, n_has = 0, n_unique = 0, n_capped = 0;
    bool unique = false;
    MapqEntry x;
    mapq_load(a, live, live ? (PAIRED ? 2 * u : u) : a.n_reads, lig, G, x);
    if (PAIRED) {
        MapqEntry y;
        mapq_load(a, live, live ? 2 * u + 1 : a.n_reads, lig, G, y);
        mapq_pair(a, x, y, G);
        mapq_pair(a, y, x, G);
        mapq_read(a, y, lane, lig, G, mapq, rflags, unique);
        sum = mapq; n_has = rflags & PGX_MAPQ_HAS ? 1u : 0u; n_unique = unique ? 1u : 0u; n_capped = rflags & PGX_MAPQ_CAPPED ? 1u : 0u;
    }
    mapq_read(a, x, lane, lig, G, mapq, rflags, unique);
    sum += mapq; n_has += rflags & PGX_MAPQ_HAS ? 1u : 0u; n_unique += unique ? 1u : 0u; n_capped += rflags & PGX_MAPQ_CAPPED ? 1u : 0u;
    // the counters: the first lane of every live group speaks for it
    const bool lead = live && lig == 0;
    uint32_t s0 = lead ? sum : 0u, s1 = lead ? n_has : 0u, s2 = lead ? n_unique : 0u, s3 = lead ? n_capped : 0u;
    for (uint32_t mask = 32; mask; mask >>= 1) {
        s0 += (uint32_t)__shfl_xor((int)s0, (int)mask, 64);
        s1 += (uint32_t)__shfl_xor((int)s1, (int)mask, 64);
        s2 += (uint32_t)__shfl_xor((int)s2, (int)mask, 64);
        s3 += (uint32_t)__shfl_xor((int)s3, (int)mask, 64);
    }
    if (lane == 0) {
        if (s1) atomicAdd(a.counters + 0, (unsigned long long)s1);
        if (s2) atomicAdd(a.counters + 1, (unsigned long long)s2);
        if (s3) atomicAdd(a.counters + 2, (unsigned long long)s3);
        if (s0) atomicAdd(a.counters + 3, (unsigned long long)s0);
    }
}

template __global__ void pgx_mapq_kernel<false>(PgxMapqArgs a);
template __global__ void pgx_mapq_kernel<true>(PgxMapqArgs a);
