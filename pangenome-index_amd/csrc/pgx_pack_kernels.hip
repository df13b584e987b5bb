// pgx_pack_kernels.hip -- read pack (include/pgx.h "read pack") as gfx950 kernels: the coverage of every graph base by the aligned reads.
//
// The node table (pgx_pack_create, once):
//   max_id     a thread a visit: atomicMax of node >> 1, one atomic a wave
//   visit_len  a thread a word of marks: every visit's length (the next mark, cut at its sequence's end, found by a bit scan of at most 17 words and a
//              binary search over the sequence starts) into len_min / len_max of its id
//   node_len   a thread an id: len = len_min, 0 where no visit names it; len_min != len_max is the refusal
// Per batch:
//   add        a lane a read: its slice of the CIGAR list; every maximal stretch of text under = / X operations (an I between them consumes no text and
//              does not cut it) adds +1 at its first text position and -1 behind its last: two atomics a stretch, not one a base.  Three counters, one
//              atomicAdd a wave each.
// The fold (pgx_pack_finish):
//   tile_sum   a workgroup a tile of PGX_SCAN_BLOCK_ITEMS differences: their sum (the project's scan turns the sums into every tile's carry-in)
//   fold       the same tiles: a block-local scan gives the text coverage c[p]; every p with c != 0 is projected -- walk_rank, walk_prev_mark, one
//              walk_nodes load, the node table -- and adds c to cov[g]; a thread keeps the visit it projected last, so that a run of covered positions
//              inside one node pays for one lookup.  Then the tile is zeroed.
//   summary    PGX_PACK_NODE_LANES lanes a node: covered, sum, max
// tdiff is i32 with wrap-around arithmetic, carried as u32 through the scan; the tile sums are sign-extended to u64 so that the scan's u64 adds wrap
// the same way.  Static LDS only (the 256 partial sums of a tile), no inline assembly; every index is 64-bit and checked against its array.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"
#include "pgx_image.h"
#include "pgx_walk_device.h"

namespace {

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the first marked position in [e, cap], cap = min(limit, e + 1024); cap + 1 where there is none up to limit's cut (the visit is longer than 1024)
__device__ __forceinline__ uint64_t pack_next_mark(const PgxWalkImage &w, uint64_t e, uint64_t limit) {
    if (e >= limit) return limit;
    const bool cut = limit - e > PGX_WALK_MAX_VISIT;
    const uint64_t cap = cut ? e + PGX_WALK_MAX_VISIT : limit;
    uint64_t wi = e >> 6;
    uint64_t word = w.bits[wi] & (~0ull << ((uint32_t)e & 63u));
    for (;;) { // at most 18 words, all below n_words: cap <= n
        if (word) {
            const uint64_t p = (wi << 6) + (uint64_t)__builtin_ctzll(word);
            if (p < cap) return p;
            break;
        }
        if (((wi + 1) << 6) >= cap) break;
        word = w.bits[++wi];
    }
    return cut ? cap + 1 : limit;
}

// the tile's 256 thread totals -> the exclusive prefix of thread t (u32, wrap-around) and the tile's total
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t *lds) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc += u;
    }
    if (lane == 63u) lds[wv] = inc;
    __syncthreads();
    uint32_t carry = 0;
    for (uint32_t j = 0; j < wv; j++) carry += lds[j];
    return carry + inc - v;
}

} // namespace

__global__ void __launch_bounds__(256)
pgx_pack_max_id_kernel(const uint64_t *__restrict__ nodes, uint64_t n_visits, unsigned long long *__restrict__ max_id) {
    uint64_t m = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_visits; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t id = nodes[k] >> 1;
        m = id > m ? id : m;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t u = __shfl_xor(m, o);
        m = u > m ? u : m;
    }
    if ((threadIdx.x & 63u) == 0) atomicMax(max_id, (unsigned long long)m);
}

__global__ void __launch_bounds__(256)
pgx_pack_visit_len_kernel(PgxWalkImage w, const uint64_t *__restrict__ seq_start, uint64_t n_seq, uint32_t endmark, uint64_t n_nodes, uint32_t *__restrict__ len_min,
                          uint32_t *__restrict__ len_max, unsigned long long *__restrict__ bad, unsigned long long *__restrict__ too_long) {
    for (uint64_t wi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; wi < w.n_words; wi += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t word = w.bits[wi];
        if (!word) continue;
        uint64_t k = walk_rank(w, wi << 6);
        while (word) {
            const uint64_t p = (wi << 6) + (uint64_t)__builtin_ctzll(word);
            word &= word - 1;
            const uint64_t kk = k++;
            if (kk >= w.n_visits || p >= w.n) continue;
            // the last sequence that starts at or before p (an empty one in front of it shares its start and is passed over)
            uint64_t lo = 0, hi = n_seq;
            while (hi - lo > 1) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (seq_start[mid] <= p) lo = mid; else hi = mid;
            }
            const uint64_t limit = seq_start[lo + 1] - endmark;
            if (p >= limit) continue; // (a mark on an endmarker: no visit of a sequence)
            const uint64_t id = w.nodes[kk] >> 1;
            if (id >= n_nodes) continue;
            const uint64_t L = pack_next_mark(w, p + 1, limit) - p;
            if (L > PGX_WALK_MAX_VISIT) { atomicMin(too_long, (unsigned long long)id); continue; }
            atomicMin(len_min + id, (uint32_t)L);
            atomicMax(len_max + id, (uint32_t)L);
        }
    }
}

__global__ void __launch_bounds__(256)
pgx_pack_node_len_kernel(uint32_t *__restrict__ len_min, const uint32_t *__restrict__ len_max, uint64_t n_nodes, unsigned long long *__restrict__ bad) {
    for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < n_nodes; id += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t lo = len_min[id], hi = len_max[id];
        if (lo == 0xFFFFFFFFu) { len_min[id] = 0; continue; }
        if (lo != hi) atomicMin(bad, (unsigned long long)id);
    }
}

__global__ void __launch_bounds__(PGX_PACK_THREADS)
pgx_pack_add_kernel(const pgx_read_align *__restrict__ recs, const uint32_t *__restrict__ seq, const uint64_t *__restrict__ text_start, const uint64_t *__restrict__ op_off,
                    const uint32_t *__restrict__ ops, const pgx_read_mapq *__restrict__ mapqs, const uint8_t *__restrict__ keep, uint32_t min_mapq, uint64_t n_reads,
                    const uint64_t *__restrict__ seq_start, uint64_t n_seq, uint64_t n, int *__restrict__ tdiff, unsigned long long *__restrict__ counters) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t counted = 0, filtered = 0, bases = 0;
    if (r < n_reads) {
        uint32_t q;
        uint64_t a;
        bool placed;
        if (recs) { q = recs[r].seq; a = recs[r].text_start; placed = q != PGX_NO_SEQUENCE && recs[r].text_end > a; }
        else { q = seq[r]; a = text_start[r]; placed = q != PGX_NO_SEQUENCE; }
        placed = placed && (uint64_t)q < n_seq;
        if (placed && !recs) { // the arrays route has no text_end: the read is placed iff its operations consume text
            uint64_t consumed = 0;
            for (uint64_t j = op_off[r]; j < op_off[r + 1]; j++) {
                const uint32_t op = ops[j] & 15u;
                if (op == PGX_ALIGN_OP_EQ || op == PGX_ALIGN_OP_X || op == PGX_ALIGN_OP_D) consumed += ops[j] >> 4;
            }
            placed = consumed > 0;
        }
        bool pass = true;
        if (mapqs) pass = min_mapq == 0 || mapqs[r].mapq >= min_mapq;
        else if (keep) pass = keep[r] != 0;
        if (placed && pass) {
            const uint64_t s = seq_start[q];
            uint64_t t = a, run = 0;
            bool in_run = false;
            // (s + t <= n below is a guard only: a valid align record and the arrays route's host checks keep every stretch inside its sequence.  A stretch
            // it dropped would still be in `bases`, and bases_added would then exceed sum(cov))
            const uint64_t o1 = op_off[r + 1];
            for (uint64_t j = op_off[r]; j < o1; j++) {
                const uint32_t word = ops[j], op = word & 15u;
                const uint64_t len = word >> 4;
                if (op == PGX_ALIGN_OP_EQ || op == PGX_ALIGN_OP_X) {
                    if (!in_run) { run = t; in_run = true; }
                    t += len;
                    bases += len;
                } else if (op == PGX_ALIGN_OP_D) {
                    if (in_run && t > run && s + t <= n) { atomicAdd(tdiff + (s + run), 1); atomicAdd(tdiff + (s + t), -1); }
                    in_run = false;
                    t += len;
                } // (S and I consume no text)
            }
            if (in_run && t > run && s + t <= n) { atomicAdd(tdiff + (s + run), 1); atomicAdd(tdiff + (s + t), -1); }
            counted = 1;
        } else if (placed) filtered = 1;
    }
    counted = wave_sum(counted); filtered = wave_sum(filtered); bases = wave_sum(bases);
    if ((threadIdx.x & 63u) == 0) {
        if (counted) atomicAdd(counters + 0, (unsigned long long)counted);
        if (filtered) atomicAdd(counters + 1, (unsigned long long)filtered);
        if (bases) atomicAdd(counters + 2, (unsigned long long)bases);
    }
}

__global__ void __launch_bounds__(256)
pgx_pack_tile_sum_kernel(const int *__restrict__ tdiff, uint64_t n1, uint64_t *__restrict__ tile_sums) {
    __shared__ uint64_t part[4];
    const uint64_t base = (uint64_t)blockIdx.x * PGX_SCAN_BLOCK_ITEMS;
    int64_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < PGX_SCAN_BLOCK_ITEMS / 256; j++) {
        const uint64_t i = base + (uint64_t)j * 256 + threadIdx.x;
        if (i < n1) v += (int64_t)tdiff[i];
    }
    const uint64_t s = wave_sum((uint64_t)v);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ void __launch_bounds__(256)
pgx_pack_fold_kernel(int *__restrict__ tdiff, uint64_t n1, const uint64_t *__restrict__ tile_off, PgxWalkImage w, PgxPackTable tb, uint32_t *__restrict__ cov,
                     unsigned long long *__restrict__ projected) {
    __shared__ uint32_t lds[4];
    constexpr uint32_t ITEMS = PGX_SCAN_BLOCK_ITEMS / 256;
    const uint64_t first = (uint64_t)blockIdx.x * PGX_SCAN_BLOCK_ITEMS + (uint64_t)threadIdx.x * ITEMS; // a thread takes ITEMS consecutive positions
    uint32_t c[ITEMS], tot = 0;
#pragma unroll
    for (uint32_t j = 0; j < ITEMS; j++) {
        const uint64_t i = first + j;
        tot += i < n1 ? (uint32_t)tdiff[i] : 0u;
        c[j] = tot;
    }
    const uint32_t carry = (uint32_t)tile_off[blockIdx.x] + block_scan_excl(tot, lds);
    // the visit projected last: [vm, vm + vlen) on node base vbase, reversed or not
    uint64_t vm = 0, vbase = 0, done = 0;
    uint32_t vlen = 0, vrev = 0;
#pragma unroll
    for (uint32_t j = 0; j < ITEMS; j++) {
        const uint64_t p = first + j;
        if (p >= n1) break;
        const uint32_t cp = carry + c[j];
        if (tdiff[p] != 0) tdiff[p] = 0;
        if (cp == 0 || p >= w.n) continue;
        if (!(vlen && p >= vm && p - vm < vlen)) {
            vlen = 0;
            const uint64_t k1 = walk_rank(w, p + 1);
            if (k1 == 0 || k1 > w.n_visits) continue;
            const uint64_t v = w.nodes[k1 - 1], id = v >> 1;
            if (id >= tb.n_nodes) continue;
            vm = walk_prev_mark(w, p, 0);
            vlen = tb.len[id];
            vbase = tb.base[id];
            vrev = (uint32_t)v & 1u;
            if (p - vm >= vlen) { vlen = 0; continue; } // (an endmarker, or a position behind a visit the table cut: nothing covers it)
        }
        const uint64_t d = p - vm;
        atomicAdd(cov + vbase + (vrev ? vlen - 1 - d : d), cp);
        done++;
    }
    done = wave_sum(done);
    if ((threadIdx.x & 63u) == 0 && done) atomicAdd(projected, (unsigned long long)done);
}

__global__ void __launch_bounds__(256)
pgx_pack_summary_kernel(PgxPackTable tb, const uint32_t *__restrict__ cov, uint32_t *__restrict__ covered, uint64_t *__restrict__ sum, uint32_t *__restrict__ max) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, id = t / PGX_PACK_NODE_LANES;
    uint32_t n_cov = 0, mx = 0;
    uint64_t sm = 0;
    if (id < tb.n_nodes) {
        const uint32_t L = tb.len[id];
        const uint64_t g = tb.base[id];
        for (uint32_t o = (uint32_t)(t % PGX_PACK_NODE_LANES); o < L; o += PGX_PACK_NODE_LANES) {
            const uint32_t c = cov[g + o];
            n_cov += c != 0;
            sm += c;
            mx = c > mx ? c : mx;
        }
    }
#pragma unroll
    for (int o = PGX_PACK_NODE_LANES / 2; o >= 1; o >>= 1) { // (the lanes of a node are neighbours inside one wave)
        n_cov += __shfl_xor(n_cov, o);
        sm += __shfl_xor(sm, o);
        const uint32_t u = __shfl_xor(mx, o);
        mx = u > mx ? u : mx;
    }
    if (id < tb.n_nodes && t % PGX_PACK_NODE_LANES == 0) { covered[id] = n_cov; sum[id] = sm; max[id] = mx; }
}
