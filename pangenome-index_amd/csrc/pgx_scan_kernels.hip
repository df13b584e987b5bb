// pgx_scan_kernels.hip -- pgx_scan_*: device-wide exclusive scans that size / place variable-length outputs, and the MEM compaction
// that uses them (gfx950).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"
#include "pgx_slots_device.h"

// ------------------------------------------------------------------------------------------
// exclusive scan of u64 values produced by a loader (3 launches: partial sums, scan of sums, apply)
//   mode 0: in32[i]                       (u32 array)
//   mode 1: in64[i]                       (u64 array)
//   mode 2: MEM capacity of read i from offsets (min(len, len - min_len + 1), 0 if len < min_len)
//   mode 3: in8[i] == (uint8_t)min_len  (indicator; merge_tags)        mode 4: in8[i]
//   mode 5: positions of tag query i from run_nums (in) and uval (in2): 1 for one run, 0 for none, else the unique count in uval
// (mode 5 only in the three-launch form; pgx_scan_tag_tail_kernel is its one-launch form)
__device__ __forceinline__ uint64_t pgx_tag_position_count(uint64_t run_num, uint64_t uval) { return run_num == 1 ? 1 : (run_num == 0 ? 0 : uval); }
__device__ __forceinline__ uint64_t pgx_scan_load(int mode, const void *in, const void *in2, uint64_t i, uint64_t min_len) {
    if (mode == 0) return ((const uint32_t *)in)[i];
    if (mode == 1) return ((const uint64_t *)in)[i];
    if (mode == 3) return ((const uint8_t *)in)[i] == (uint8_t)min_len ? 1u : 0u;
    if (mode == 4) return ((const uint8_t *)in)[i];
    if (mode == 5) return pgx_tag_position_count(((const uint64_t *)in)[i], ((const uint64_t *)in2)[i]);
    const uint64_t *off = (const uint64_t *)in;
    const uint64_t len = off[i + 1] - off[i];
    if (len < min_len) return 0;
    const uint64_t c = len - min_len + 1;
    return c < len ? c : len;
}

__device__ __forceinline__ uint64_t pgx_block_excl_scan(uint64_t v, uint64_t *s_wave, uint64_t &block_total) {
    // 256 threads = 4 waves; returns exclusive prefix of v within the block
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    uint64_t wbase = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i < w) wbase += s_wave[i];
        tot += s_wave[i];
    }
    block_total = tot;
    __syncthreads();
    return wbase + inc - v;
}

#define PGX_SCAN_ITEMS 8 // per thread -> 2048 per block
__global__ void __launch_bounds__(256)
pgx_scan_partial_kernel(int mode, const void *in, const void *in2, uint64_t n_cap, uint64_t min_len, uint64_t *__restrict__ block_sums, const uint64_t *__restrict__ n_dev) {
    __shared__ uint64_t s_wave[4];
    const uint64_t n = n_dev ? (*n_dev < n_cap ? *n_dev : n_cap) : n_cap; // the actual count may live on the device (speculative sizing)
    const uint64_t b0 = (uint64_t)blockIdx.x * 256 * PGX_SCAN_ITEMS;
    uint64_t v = 0;
    for (int t = 0; t < PGX_SCAN_ITEMS; t++) {
        const uint64_t i = b0 + (uint64_t)threadIdx.x * PGX_SCAN_ITEMS + t;
        if (i < n) v += pgx_scan_load(mode, in, in2, i, min_len);
    }
    uint64_t tot;
    (void)pgx_block_excl_scan(v, s_wave, tot);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

// single block: in-place exclusive scan of block_sums[0..nb), total appended at block_sums[nb]
__global__ void __launch_bounds__(256) pgx_scan_sums_kernel(uint64_t *block_sums, uint64_t nb) {
    __shared__ uint64_t s_wave[4];
    uint64_t carry = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += 256) {
        const uint64_t i = b0 + threadIdx.x;
        const uint64_t v = i < nb ? block_sums[i] : 0;
        uint64_t tot;
        const uint64_t ex = pgx_block_excl_scan(v, s_wave, tot);
        if (i < nb) block_sums[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) block_sums[nb] = carry;
}

// out has n+1 entries; out[n] = total
__global__ void __launch_bounds__(256)
pgx_scan_apply_kernel(int mode, const void *in, const void *in2, uint64_t n_cap, uint64_t min_len, const uint64_t *__restrict__ block_sums,
                      uint64_t nb, uint64_t *__restrict__ out, uint64_t *__restrict__ total_out, int raw_sums, const uint64_t *__restrict__ n_dev) {
    __shared__ uint64_t s_wave[4];
    const uint64_t n = n_dev ? (*n_dev < n_cap ? *n_dev : n_cap) : n_cap;
    const uint64_t b0 = (uint64_t)blockIdx.x * 256 * PGX_SCAN_ITEMS;
    // raw_sums: block_sums holds the per-block totals as pgx_scan_partial_kernel wrote them (few blocks: every block adds up
    // the totals before it, which saves the single-block launch in between); otherwise their exclusive scan + grand total
    uint64_t base, grand = 0;
    if (raw_sums) {
        uint64_t part = 0, all = 0;
        for (uint64_t i = threadIdx.x; i < nb; i += 256) {
            const uint64_t t = block_sums[i];
            part += i < blockIdx.x ? t : 0;
            all += t;
        }
        uint64_t tot;
        (void)pgx_block_excl_scan(part, s_wave, tot);
        base = tot;
        if (blockIdx.x == 0) { (void)pgx_block_excl_scan(all, s_wave, tot); grand = tot; }
    } else {
        base = block_sums[blockIdx.x];
        grand = block_sums[nb];
    }
    uint64_t vals[PGX_SCAN_ITEMS], v = 0;
    for (int t = 0; t < PGX_SCAN_ITEMS; t++) {
        const uint64_t i = b0 + (uint64_t)threadIdx.x * PGX_SCAN_ITEMS + t;
        vals[t] = i < n ? pgx_scan_load(mode, in, in2, i, min_len) : 0;
        v += vals[t];
    }
    uint64_t tot;
    uint64_t ex = base + pgx_block_excl_scan(v, s_wave, tot);
    for (int t = 0; t < PGX_SCAN_ITEMS; t++) {
        const uint64_t i = b0 + (uint64_t)threadIdx.x * PGX_SCAN_ITEMS + t;
        if (i < n) out[i] = ex;
        ex += vals[t];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[n] = grand;
        if (total_out) *total_out = grand; // a second copy next to other scalars the host reads back together
    }
}

// The same scan in ONE launch (decoupled look-back): tiles of 4096 items take their numbers from a counter in the order they start, publish their
// total, look back over the tiles before them until one has published its inclusive prefix, and publish their own.  A tile word is
// epoch (18 bits) | state (2: 1 = total, 2 = inclusive prefix) | value (44 bits) in one 64-bit store, so a word of an earlier scan over the same
// buffer reads as "nothing yet" and nothing has to be cleared between scans.  Loads and stores are coalesced (a wave scans 64 consecutive items per
// round with lane shifts, sixteen rounds), which the three-launch form above was not: 10 M counts take 177 us there.
// state[0]: tile counter (the last tile sets it back to 0), state[1 + t]: word of tile t.
#define PGX_SCAN1_ROUNDS 16
// Look-back of wave 0 of tile `tile` (all 64 lanes call it): publishes the tile's total, adds up the tiles before it, publishes the tile's inclusive
// prefix and returns the exclusive one.  A tile only ever waits for tiles that took their numbers before it.
__device__ __forceinline__ uint64_t pgx_scan1_lookback(unsigned long long *__restrict__ state, uint32_t tile, uint64_t tile_total, uint32_t epoch, int lane) {
    const unsigned long long ep = (unsigned long long)(epoch & 0x3FFFFu) << 46;
    const unsigned long long vmask = (1ull << 44) - 1ull;
    uint64_t prefix = 0;
    if (tile != 0) {
        if (lane == 0) __hip_atomic_store(state + 1 + tile, ep | (1ull << 44) | (tile_total & vmask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int64_t j = (int64_t)tile - 1;
        for (;;) { // 64 predecessors at a time, nearest first (lane 0 = tile j)
            const int64_t idx = j - lane;
            unsigned long long word = ep | (2ull << 44); // (before tile 0: an inclusive prefix of 0)
            if (idx >= 0) word = __hip_atomic_load(state + 1 + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t st = (word >> 46) == (ep >> 46) ? (uint32_t)(word >> 44) & 3u : 0u;
            const unsigned long long ready = __ballot(st != 0u), full = __ballot(st == 2u);
            // the run of published words that starts at lane 0 and ends at the first inclusive prefix (or at lane 63)
            const unsigned long long gap = ~ready;
            const int stop_gap = gap ? (int)__ffsll((long long)gap) - 1 : 64, stop_full = full ? (int)__ffsll((long long)full) - 1 : 64;
            if (stop_full < stop_gap) { // an inclusive prefix before any unpublished tile: sum up to it and stop
                uint64_t v = lane <= stop_full ? (uint64_t)(word & vmask) : 0;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
                prefix += __shfl(v, 0, 64);
                break;
            }
            if (stop_gap == 64) { // 64 totals, no prefix among them: take them all and look further back
                uint64_t v = (uint64_t)(word & vmask);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
                prefix += __shfl(v, 0, 64);
                j -= 64;
                continue;
            }
            __builtin_amdgcn_s_sleep(2); // a tile in the window has not published yet
        }
    }
    if (lane == 0) __hip_atomic_store(state + 1 + tile, ep | (2ull << 44) | ((prefix + tile_total) & vmask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return prefix;
}

template <int MODE>
__global__ void __launch_bounds__(256)
pgx_scan_onepass_kernel(const void *in, uint64_t n_cap, uint64_t min_len, uint64_t *__restrict__ out, uint64_t *__restrict__ total_out,
                        const uint64_t *__restrict__ n_dev, unsigned long long *__restrict__ state, uint32_t epoch) {
    constexpr int mode = MODE;
    __shared__ uint64_t s_wave[4];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_tile;
    const uint64_t n = n_dev ? (*n_dev < n_cap ? *n_dev : n_cap) : n_cap;
    if (threadIdx.x == 0) s_tile = atomicAdd(reinterpret_cast<uint32_t *>(state), 1u);
    __syncthreads();
    const uint32_t tile = s_tile;
    // tiles behind the one that holds item n - 1 have nothing to do (n may be a device count well below the capacity the grid was sized for): they
    // leave at once, and nobody looks back at them
    const uint32_t last_tile = n ? (uint32_t)((n - 1) / (256u * PGX_SCAN1_ROUNDS)) : 0u;
    if (tile > last_tile) {
        if (tile == gridDim.x - 1 && threadIdx.x == 0) __hip_atomic_store(reinterpret_cast<uint32_t *>(state), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t b0 = (uint64_t)tile * (256u * PGX_SCAN1_ROUNDS) + (uint64_t)w * (64u * PGX_SCAN1_ROUNDS);
    uint64_t x[PGX_SCAN1_ROUNDS], carry = 0;
#pragma unroll
    for (int r = 0; r < PGX_SCAN1_ROUNDS; r++) { // (all sixteen loads first: one memory latency per tile, not one per round)
        const uint64_t i = b0 + (uint64_t)(r * 64 + lane);
        x[r] = i < n ? pgx_scan_load(mode, in, nullptr, i, min_len) : 0;
    }
#pragma unroll
    for (int r = 0; r < PGX_SCAN1_ROUNDS; r++) {
        const uint64_t v = x[r];
        uint64_t inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint64_t t = __shfl_up(inc, off, 64);
            if (lane >= off) inc += t;
        }
        x[r] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) s_wave[w] = carry;
    __syncthreads();
    uint64_t wbase = 0, tile_total = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) { if (i < w) wbase += s_wave[i]; tile_total += s_wave[i]; }
    if (w == 0) {
        const uint64_t prefix = pgx_scan1_lookback(state, tile, tile_total, epoch, lane);
        if (lane == 0) s_prefix = prefix;
    }
    __syncthreads();
    const uint64_t P = s_prefix + wbase;
#pragma unroll
    for (int r = 0; r < PGX_SCAN1_ROUNDS; r++) {
        const uint64_t i = b0 + (uint64_t)(r * 64 + lane);
        if (i < n) out[i] = P + x[r];
    }
    if (tile == last_tile && threadIdx.x == 0) {
        const uint64_t grand = s_prefix + tile_total;
        out[n] = grand;
        if (total_out) *total_out = grand;
    }
    if (tile == gridDim.x - 1 && threadIdx.x == 0) // (every tile has its number by now)
        __hip_atomic_store(reinterpret_cast<uint32_t *>(state), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#define PGX_SCAN1_INSTANTIATE(M) \
    template __global__ void pgx_scan_onepass_kernel<M>(const void *, uint64_t, uint64_t, uint64_t *, uint64_t *, const uint64_t *, unsigned long long *, uint32_t);
PGX_SCAN1_INSTANTIATE(0) PGX_SCAN1_INSTANTIATE(1) PGX_SCAN1_INSTANTIATE(2) PGX_SCAN1_INSTANTIATE(3) PGX_SCAN1_INSTANTIATE(4)

// The tail of the tag stage as one such scan over (run_nums, uval): query q contributes pgx_tag_position_count positions, pos_off is their exclusive
// scan, and -- with `positions` -- a one-run query's value goes to positions[pos_off[q]] in the same pass (listed queries are copied from their
// segments by pgx_tag_compact_kernel).  In a speculative run `positions` holds pos_cap values sized before the total is known: every store is
// guarded by it, and the tile that produces the grand total raises bit 0 of *abort when the total exceeds it.  A run that was aborted before this
// launch left uval unwritten for the listed queries: the scan still runs (every tile takes part in the look-back), but stores no values and raises nothing.
__global__ void __launch_bounds__(256)
pgx_scan_tag_tail_kernel(const uint64_t *__restrict__ run_nums, const uint64_t *__restrict__ uval, uint64_t n_cap, const uint64_t *__restrict__ n_dev,
                         uint64_t *__restrict__ pos_off, uint64_t *__restrict__ total_out, uint64_t *__restrict__ positions, uint64_t pos_cap,
                         uint64_t *__restrict__ abort, unsigned long long *__restrict__ state, uint32_t epoch) {
    __shared__ uint64_t s_wave[4];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_tile;
    const uint64_t n = n_dev ? (*n_dev < n_cap ? *n_dev : n_cap) : n_cap;
    const bool live = !(abort && __hip_atomic_load(abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (!live) positions = nullptr;
    if (threadIdx.x == 0) s_tile = atomicAdd(reinterpret_cast<uint32_t *>(state), 1u);
    __syncthreads();
    const uint32_t tile = s_tile;
    const uint32_t last_tile = n ? (uint32_t)((n - 1) / (256u * PGX_SCAN1_ROUNDS)) : 0u;
    if (tile > last_tile) { // (as in pgx_scan_onepass_kernel)
        if (tile == gridDim.x - 1 && threadIdx.x == 0) __hip_atomic_store(reinterpret_cast<uint32_t *>(state), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t b0 = (uint64_t)tile * (256u * PGX_SCAN1_ROUNDS) + (uint64_t)w * (64u * PGX_SCAN1_ROUNDS);
    uint64_t x[PGX_SCAN1_ROUNDS], u[PGX_SCAN1_ROUNDS], carry = 0;
    uint32_t one_run = 0; // bit r: item r of this lane is a one-run query, u[r] its value
#pragma unroll
    for (int r = 0; r < PGX_SCAN1_ROUNDS; r++) {
        const uint64_t i = b0 + (uint64_t)(r * 64 + lane);
        x[r] = i < n ? run_nums[i] : 0;
        u[r] = i < n ? uval[i] : 0;
    }
#pragma unroll
    for (int r = 0; r < PGX_SCAN1_ROUNDS; r++) {
        if (x[r] == 1) one_run |= 1u << r;
        const uint64_t v = pgx_tag_position_count(x[r], u[r]);
        uint64_t inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint64_t t = __shfl_up(inc, off, 64);
            if (lane >= off) inc += t;
        }
        x[r] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) s_wave[w] = carry;
    __syncthreads();
    uint64_t wbase = 0, tile_total = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) { if (i < w) wbase += s_wave[i]; tile_total += s_wave[i]; }
    if (w == 0) {
        const uint64_t prefix = pgx_scan1_lookback(state, tile, tile_total, epoch, lane);
        if (lane == 0) s_prefix = prefix;
    }
    __syncthreads();
    const uint64_t P = s_prefix + wbase;
#pragma unroll
    for (int r = 0; r < PGX_SCAN1_ROUNDS; r++) {
        const uint64_t i = b0 + (uint64_t)(r * 64 + lane);
        if (i < n) {
            const uint64_t at = P + x[r];
            pos_off[i] = at;
            if (positions && ((one_run >> r) & 1u) && at < pos_cap) positions[at] = u[r];
        }
    }
    if (tile == last_tile && threadIdx.x == 0) {
        const uint64_t grand = s_prefix + tile_total;
        pos_off[n] = grand;
        if (total_out) *total_out = grand;
        if (abort && live && grand > pos_cap) atomicOr((unsigned long long *)abort, 1ull);
    }
    if (tile == gridDim.x - 1 && threadIdx.x == 0)
        __hip_atomic_store(reinterpret_cast<uint32_t *>(state), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------
// MEM compaction: slots (pgx_slot_index: four per read in a dense slot-major array, the rest in the arena / at the read's worst-case offset) -> dense CSR in read order
__global__ void __launch_bounds__(256)
pgx_compact_mems_kernel(uint64_t first_read, uint64_t n_reads, const uint64_t *__restrict__ slot_off, uint64_t slot_base,
                        const pgx_mem *__restrict__ slots, const uint32_t *__restrict__ mem_count,
                        const uint64_t *__restrict__ local_off, uint64_t mem_base, pgx_mem *__restrict__ mems, uint64_t cap_mems,
                        uint64_t *__restrict__ abort, const uint32_t *__restrict__ ovf_base, uint64_t ovf_cap) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; // read first_read + t of this chunk
    if (t >= n_reads) return;
    const uint64_t i = first_read + t;
    const uint32_t c = mem_count[i];
    const uint64_t src = c <= PGX_FAST_SLOTS ? 0ull : (ovf_cap ? (uint64_t)ovf_base[i] - PGX_FAST_SLOTS : slot_off[i] - slot_base), dst = mem_base + local_off[t];
    if (dst + c > cap_mems) { // speculative sizing: the MEM array was sized from an earlier run and this one has more
        if (c && abort) atomicOr((unsigned long long *)abort, 16ull);
        return;
    }
    for (uint32_t u = 0; u < c; u++) mems[dst + u] = slots[pgx_slot_index(t, n_reads, src, u)];
}
