// pgx_build_sa_kernels.hip -- pgx_sa_*: suffix sorting of a text collection by prefix doubling, its BWT and the runs of it (gfx950).
// Driver: pgx_build_sa.hip (pgx_build_index_from_text[s]_device).  Wave64, 256-thread blocks.  Text positions, suffix ranks and BWT rows
// are uint32_t (the driver refuses n >= 2^32 - 2^20); every index that is multiplied by a tile size is uint64_t.
//
// No kernel here waits for another block: every device-wide sum goes through per-tile counts and scan_excl (pgx_scan_kernels.hip).
//
//   classify   text bytes -> 3-bit codes (\n A C G N T = 0 .. 5), first byte outside the alphabet by atomicMin, newlines per tile
//   keys       (hi, lo, idx) of every suffix: hi = its first PGX_SA_K symbols at 3 bits, nothing behind an endmarker; lo = the number of
//              the sequence when an endmarker lies within those symbols (what breaks the tie between two such keys), else 0; sequence starts
//   hist / scatter   one pass of a stable LSD radix sort of the triples by 8 bits of hi or lo
//   heads / ranks    groups of equal (hi, lo) in the sorted order -> dense group numbers = the ranks of the next round
//   gather     lo = rank[idx + h]
//   bwt / run_heads / runs   bwt[r] = text[SA[r] - 1], logical runs (every endmarker row its own), their symbol, first row, first and last suffix
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

// exclusive prefix of v over the 256 threads of the block, and the block total
__device__ __forceinline__ uint32_t pgx_sa_block_excl(uint32_t v, uint32_t *s_wave, uint32_t &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    uint32_t wbase = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i < w) wbase += s_wave[i];
        tot += s_wave[i];
    }
    total = tot;
    __syncthreads();
    return wbase + inc - v;
}

__device__ __forceinline__ uint32_t pgx_sa_code(uint32_t c) {
    return c == '\n' ? 0u : c == 'A' ? 1u : c == 'C' ? 2u : c == 'G' ? 3u : c == 'N' ? 4u : c == 'T' ? 5u : 8u;
}

// a tile = PGX_SA_TILE symbols, a thread its 8 consecutive ones.  codes holds n_words u64 (eight codes each), cleared by the caller.
__global__ void __launch_bounds__(256)
pgx_sa_classify_kernel(const uint8_t *__restrict__ text, uint64_t n, uint64_t *__restrict__ codes, uint64_t n_words, uint32_t *__restrict__ tile_nl,
                       unsigned long long *__restrict__ first_bad) {
    __shared__ uint32_t s_wave[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * PGX_SA_TILE + (uint64_t)threadIdx.x * 8;
    uint64_t w = 0;
    uint32_t nl = 0;
    if (i0 < n) {
        uint64_t raw = 0;
        if (i0 + 8 <= n) raw = *reinterpret_cast<const uint64_t *>(text + i0);
        else
            for (uint32_t k = 0; i0 + k < n; k++) raw |= (uint64_t)text[i0 + k] << (8 * k);
        const uint32_t m = n - i0 < 8 ? (uint32_t)(n - i0) : 8u;
        uint64_t bad = ~0ull;
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t c = pgx_sa_code((uint32_t)(raw >> (8 * k)) & 0xFFu);
            if (c == 8u) { if (bad == ~0ull) bad = i0 + k; }
            else { w |= (uint64_t)c << (8 * k); nl += c == 0u; }
        }
        if (bad != ~0ull) atomicMin(first_bad, (unsigned long long)bad);
        if ((i0 >> 3) < n_words) codes[i0 >> 3] = w;
    }
    uint32_t tot;
    (void)pgx_sa_block_excl(nl, s_wave, tot);
    if (threadIdx.x == 0) tile_nl[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256)
pgx_sa_keys_kernel(const uint64_t *__restrict__ codes, uint64_t n_words, uint64_t n, const uint64_t *__restrict__ tile_off, uint64_t n_seq,
                   uint32_t *__restrict__ hi, uint32_t *__restrict__ lo, uint32_t *__restrict__ idx, uint32_t *__restrict__ seq_start) {
    __shared__ uint32_t s_wave[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * PGX_SA_TILE + (uint64_t)threadIdx.x * 8;
    const uint64_t j = i0 >> 3;
    uint64_t w[3];
#pragma unroll
    for (int q = 0; q < 3; q++) w[q] = j + q < n_words ? codes[j + q] : 0; // (codes behind the text are 0: nothing is read behind the last endmarker anyway)
    uint32_t c[24], nl = 0;
#pragma unroll
    for (int k = 0; k < 24; k++) c[k] = (uint32_t)(w[k >> 3] >> (8 * (k & 7))) & 0xFFu;
#pragma unroll
    for (int k = 0; k < 8; k++) nl += (i0 + k < n && c[k] == 0u);
    uint32_t tot;
    uint64_t seq = tile_off[blockIdx.x] + pgx_sa_block_excl(nl, s_wave, tot); // the sequence that holds symbol i0
    if (i0 == 0) seq_start[0] = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t i = i0 + k;
        if (i >= n) break;
        uint32_t key = 0;
        bool ends = false;
#pragma unroll
        for (int d = 0; d < PGX_SA_K; d++) {
            const uint32_t v = c[k + d];
            if (!ends && v == 0u) ends = true;
            if (!ends) key |= v << (3 * (PGX_SA_K - 1 - d));
        }
        hi[i] = key;
        lo[i] = ends ? (uint32_t)seq : 0u;
        idx[i] = (uint32_t)i;
        if (c[k] == 0u) {
            seq++;
            if (seq < n_seq) seq_start[seq] = (uint32_t)(i + 1);
        }
    }
}

// ------------------------------------------------------------------------------------------
// radix pass.  hist[digit * n_blocks + block] = elements of the block's PGX_SA_SORT_TILE keys with that digit; after scan_excl over the
// table offs[digit * n_blocks + block] is where the block's first element with that digit goes.
__global__ void __launch_bounds__(256)
pgx_sa_hist_kernel(const uint32_t *__restrict__ key, uint64_t n, uint32_t shift, uint32_t n_blocks, uint32_t *__restrict__ hist) {
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * PGX_SA_SORT_TILE;
    for (uint32_t r = 0; r < PGX_SA_SORT_TILE / 256; r++) {
        const uint64_t i = base + r * 256u + threadIdx.x;
        if (i < n) atomicAdd(&s_h[(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * n_blocks + blockIdx.x] = s_h[threadIdx.x];
}

// The block walks its tile 256 elements at a time, in input order.  Within a wave the lanes with the same digit find each other by eight
// ballots (rank = lanes before me with my digit); the first of them leaves their number in the wave's row of s_cnt; a position is the
// digit's running base + the counts of the waves before mine + the rank.  Input order is kept within every digit, no global atomics.
__global__ void __launch_bounds__(256)
pgx_sa_scatter_kernel(const uint32_t *__restrict__ hi, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ idx, uint64_t n, int key_is_hi,
                      uint32_t shift, uint32_t n_blocks, const uint64_t *__restrict__ offs, uint32_t *__restrict__ hi_out,
                      uint32_t *__restrict__ lo_out, uint32_t *__restrict__ idx_out) {
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_cnt[4][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    s_base[threadIdx.x] = (uint32_t)offs[(uint64_t)threadIdx.x * n_blocks + blockIdx.x];
#pragma unroll
    for (int q = 0; q < 4; q++) s_cnt[q][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * PGX_SA_SORT_TILE;
    for (uint32_t r = 0; r < PGX_SA_SORT_TILE / 256; r++) {
        if (base + r * 256u >= n) break; // (the whole block leaves together)
        const uint64_t i = base + r * 256u + threadIdx.x;
        const bool valid = i < n;
        uint32_t a = 0, b = 0, x = 0;
        if (valid) { a = hi[i]; b = lo[i]; x = idx[i]; }
        const uint32_t d = ((key_is_hi ? a : b) >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long bal = __ballot(valid && one);
            peers &= one ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0) s_cnt[w][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t pos = s_base[d] + rank;
#pragma unroll
            for (int q = 0; q < 4; q++) pos += q < w ? s_cnt[q][d] : 0u;
            if (pos < n) { hi_out[pos] = a; lo_out[pos] = b; idx_out[pos] = x; } // (a histogram that matches the keys never fails this)
        }
        __syncthreads();
        s_base[threadIdx.x] += s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
#pragma unroll
        for (int q = 0; q < 4; q++) s_cnt[q][threadIdx.x] = 0;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// row r starts a group when its (hi, lo) differs from row r - 1's.  A tile = PGX_SA_TILE rows, a thread its 8 consecutive ones.
__device__ __forceinline__ uint32_t pgx_sa_group_flags(const uint32_t *__restrict__ hi, const uint32_t *__restrict__ lo, uint64_t r0, uint64_t n, uint32_t &count) {
    uint32_t flags = 0, ph = 0, pl = 0;
    count = 0;
    if (r0 < n && r0 > 0) { ph = hi[r0 - 1]; pl = lo[r0 - 1]; }
    for (uint32_t k = 0; k < 8 && r0 + k < n; k++) {
        const uint32_t a = hi[r0 + k], b = lo[r0 + k];
        if (r0 + k == 0 || a != ph || b != pl) { flags |= 1u << k; count++; }
        ph = a; pl = b;
    }
    return flags;
}

__global__ void __launch_bounds__(256)
pgx_sa_heads_kernel(const uint32_t *__restrict__ hi, const uint32_t *__restrict__ lo, uint64_t n, uint32_t *__restrict__ tile_cnt) {
    __shared__ uint32_t s_wave[4];
    uint32_t c, tot;
    (void)pgx_sa_group_flags(hi, lo, (uint64_t)blockIdx.x * PGX_SA_TILE + (uint64_t)threadIdx.x * 8, n, c);
    (void)pgx_sa_block_excl(c, s_wave, tot);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}

// rank of a row = the number of its group (groups counted from 0 in sorted order): hi_out[r], and rank[idx[r]] for the gather
__global__ void __launch_bounds__(256)
pgx_sa_ranks_kernel(const uint32_t *__restrict__ hi, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ idx, uint64_t n,
                    const uint64_t *__restrict__ tile_off, uint32_t *__restrict__ hi_out, uint32_t *__restrict__ rank) {
    __shared__ uint32_t s_wave[4];
    const uint64_t r0 = (uint64_t)blockIdx.x * PGX_SA_TILE + (uint64_t)threadIdx.x * 8;
    uint32_t c, tot;
    const uint32_t flags = pgx_sa_group_flags(hi, lo, r0, n, c);
    uint32_t g = (uint32_t)tile_off[blockIdx.x] + pgx_sa_block_excl(c, s_wave, tot); // groups that start before row r0
    for (uint32_t k = 0; k < 8 && r0 + k < n; k++) {
        g += (flags >> k) & 1u;
        hi_out[r0 + k] = g - 1u;
        rank[idx[r0 + k]] = g - 1u;
    }
}

__global__ void __launch_bounds__(256)
pgx_sa_gather_kernel(const uint32_t *__restrict__ idx, const uint32_t *__restrict__ rank, uint64_t n, uint64_t h, uint32_t *__restrict__ lo) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint64_t p = (uint64_t)idx[r] + h;
    lo[r] = p < n ? rank[p] : 0u; // (a suffix meets its endmarker before the end of the text: never taken for a group that is still open)
}

// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
pgx_sa_bwt_kernel(const uint32_t *__restrict__ sa, const uint8_t *__restrict__ text, uint64_t n, uint8_t *__restrict__ bwt) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t p = sa[r];
    bwt[r] = p ? text[p - 1] : (uint8_t)'\n'; // the symbol before the text is the endmarker of the sequence before it
}

__device__ __forceinline__ uint32_t pgx_sa_run_flags(const uint8_t *__restrict__ bwt, uint64_t r0, uint64_t n, uint32_t &count) {
    uint32_t flags = 0, prev = 0;
    count = 0;
    if (r0 < n && r0 > 0) prev = bwt[r0 - 1];
    for (uint32_t k = 0; k < 8 && r0 + k < n; k++) {
        const uint32_t c = bwt[r0 + k];
        if (r0 + k == 0 || c != prev || c == '\n') { flags |= 1u << k; count++; }
        prev = c;
    }
    return flags;
}

__global__ void __launch_bounds__(256) pgx_sa_run_heads_kernel(const uint8_t *__restrict__ bwt, uint64_t n, uint32_t *__restrict__ tile_cnt) {
    __shared__ uint32_t s_wave[4];
    uint32_t c, tot;
    (void)pgx_sa_run_flags(bwt, (uint64_t)blockIdx.x * PGX_SA_TILE + (uint64_t)threadIdx.x * 8, n, c);
    (void)pgx_sa_block_excl(c, s_wave, tot);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}

// run k: symbol, first row, suffix of its first row; the suffix of the row before a run's first is the tail of run k - 1
__global__ void __launch_bounds__(256)
pgx_sa_runs_kernel(const uint8_t *__restrict__ bwt, const uint32_t *__restrict__ sa, uint64_t n, const uint64_t *__restrict__ tile_off, uint64_t n_runs,
                   uint8_t *__restrict__ run_sym, uint32_t *__restrict__ run_start, uint32_t *__restrict__ run_head, uint32_t *__restrict__ run_tail) {
    __shared__ uint32_t s_wave[4];
    const uint64_t r0 = (uint64_t)blockIdx.x * PGX_SA_TILE + (uint64_t)threadIdx.x * 8;
    uint32_t c, tot;
    const uint32_t flags = pgx_sa_run_flags(bwt, r0, n, c);
    uint64_t k = tile_off[blockIdx.x] + pgx_sa_block_excl(c, s_wave, tot);
    for (uint32_t q = 0; q < 8 && r0 + q < n; q++) {
        const uint64_t r = r0 + q;
        if ((flags >> q) & 1u) {
            if (k < n_runs) {
                run_sym[k] = bwt[r];
                run_start[k] = (uint32_t)r;
                run_head[k] = sa[r];
                if (k > 0) run_tail[k - 1] = sa[r - 1];
            }
            k++;
        }
        if (r == n - 1 && n_runs) run_tail[n_runs - 1] = sa[r];
    }
}
