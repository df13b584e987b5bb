// pgx_compact_kernels.hip -- pgx_compact_*: the compact result form (include/pgx.h "compact result"): the device-resident result of a run as
// a stream of LEB128 varints, cut into blocks of PGX_COMPACT_BLOCK_READS reads that decode independently (gfx950).
//
// One wave per block, four blocks per workgroup.  A block's input is contiguous in every device array -- mem_off[64k .. 64k + 64], one span of
// mems / run_nums / pos_off, one span of positions -- so the wave walks each of the three sections 64 items a round with coalesced loads,
// takes the wave prefix sum of the items' varint lengths and adds the round's total to a running byte offset.  The same walk runs twice:
// pgx_compact_size_kernel keeps only the final offset (the block's byte count, padded to 8), the exclusive scan of those counts gives
// block_offsets, and pgx_compact_fill_kernel repeats the walk from block_offsets[k] and stores the bytes.  Nothing of a block is staged: a
// block's positions may exceed LDS many times over (96 haplotypes: ~21 000 a block), a round needs 64 of them.
//
// Which positions open a MEM (and are written as they are, not as a difference): the pos_off entries of the block's MEMs ascend with the
// MEM index, so a cursor over them follows the rounds; a round's entries that fall into its window of 64 positions each set one bit of a
// 64-bit mask (an OR across the wave, in registers), and lane j reads bit j.
//
// Two fill kernels write the same stream.  pgx_compact_fill_kernel stores every byte straight to global memory (neighbouring lanes write
// neighbouring bytes); pgx_compact_fill_staged_kernel (PGX_COMPACT_STAGE=1) collects a round's bytes in an LDS stage of the wave and stores
// 8-byte words.  Timed side by side (scripts/compact_result_bench.py, 10 M reads, 352 MB of stream): 1.149 ms against 1.167 ms for the whole
// encode, so the stores are not what the time is made of and the direct kernel is the default (DESIGN.md "Compact result form").
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

__device__ __forceinline__ uint32_t pgx_varint_len(uint64_t v) {
    const uint32_t bits = 64u - (uint32_t)__clzll((long long)(v | 1));
    return (bits + 6u) / 7u;
}

__device__ __forceinline__ uint8_t *pgx_varint_put(uint8_t *p, uint64_t v) {
    while (v >= 128) {
        *p++ = (uint8_t)(v | 0x80u);
        v >>= 7;
    }
    *p++ = (uint8_t)v;
    return p;
}

// inclusive prefix sum over the wave; total = the sum over all 64 lanes
__device__ __forceinline__ uint32_t pgx_wave_incl_scan(uint32_t v, uint32_t &total) {
    const int lane = threadIdx.x & 63;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    total = __shfl(inc, 63, 64);
    return inc;
}

__device__ __forceinline__ uint64_t pgx_wave_or(uint64_t v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
    return v;
}

// LDS writes of some lanes of the wave are complete before LDS reads of others (the varint bytes may go through flat stores)
__device__ __forceinline__ void pgx_wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

#define PGX_COMPACT_STAGE_WORDS 482 // 64 lanes x 6 varints x 10 bytes (a round of tagged MEM records at their longest) + 7 carried bytes, in 8-byte words

// Where the bytes of a round go.  MODE 1: straight to global memory.  MODE 2: into the wave's LDS stage, which holds the stream from `wbase` (a multiple
// of 8) on; after every round the whole words go out as 8-byte stores and the up to 7 bytes behind them move to the front of the stage.
template <int MODE>
struct PgxCompactSink {
    uint8_t *bytes;
    uint8_t *stage;
    uint64_t wbase;
    __device__ __forceinline__ uint8_t *at(uint64_t off, uint32_t rel) const { return MODE == 2 ? stage + (off - wbase) + rel : bytes + off + rel; }
    __device__ __forceinline__ void round_done(uint64_t off) {
        if (MODE != 2) return;
        const uint32_t lane = threadIdx.x & 63;
        pgx_wave_lds_order();
        const uint32_t have = (uint32_t)(off - wbase), nw = have >> 3, rem = have & 7;
        const uint64_t *sw = reinterpret_cast<const uint64_t *>(stage);
        uint64_t *gw = reinterpret_cast<uint64_t *>(bytes + wbase);
        for (uint32_t i = lane; i < nw; i += 64) gw[i] = sw[i];
        uint8_t c = 0;
        if (lane < rem) c = stage[nw * 8 + lane];
        pgx_wave_lds_order();
        if (lane < rem) stage[lane] = c;
        wbase += (uint64_t)nw * 8;
    }
    // the last, partial word of the block with its zero padding
    __device__ __forceinline__ void finish(uint64_t off) {
        if (MODE != 2) return;
        pgx_wave_lds_order();
        const uint32_t rem = (uint32_t)(off - wbase);
        if ((threadIdx.x & 63) == 0 && rem) {
            uint64_t w = 0;
            for (uint32_t j = 0; j < rem; j++) w |= (uint64_t)stage[j] << (8 * j);
            *reinterpret_cast<uint64_t *>(bytes + wbase) = w;
        }
    }
};

// The walk over block k.  MODE 0: returns the unpadded byte count.  MODE 1 / 2: writes the bytes from `off` on (a multiple of 8) and returns where they end.
template <int MODE>
__device__ __forceinline__ uint64_t pgx_compact_walk(const uint64_t *__restrict__ mem_off, const pgx_mem *__restrict__ mems, const uint64_t *__restrict__ run_nums,
                                                     const uint64_t *__restrict__ pos_off, const uint64_t *__restrict__ positions, uint64_t n_reads, uint64_t k,
                                                     bool tags, uint64_t off, uint8_t *__restrict__ bytes, uint8_t *stage, uint64_t &m0_out, uint64_t &p0_out) {
    constexpr bool FILL = MODE != 0;
    PgxCompactSink<MODE> sink{bytes, stage, off};
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t r0 = k * PGX_COMPACT_BLOCK_READS;
    const uint64_t left = n_reads - r0;
    const uint32_t nr = left < PGX_COMPACT_BLOCK_READS ? (uint32_t)left : PGX_COMPACT_BLOCK_READS;
    const uint64_t m0 = mem_off[r0], m1 = mem_off[r0 + nr];
    m0_out = m0;
    uint32_t total;
    { // section 1: MEMs per read
        uint64_t c = 0;
        uint32_t l = 0;
        if (lane < nr) {
            c = mem_off[r0 + lane + 1] - mem_off[r0 + lane];
            l = pgx_varint_len(c);
        }
        const uint32_t inc = pgx_wave_incl_scan(l, total);
        if (FILL && lane < nr) pgx_varint_put(sink.at(off, inc - l), c);
        off += total;
        sink.round_done(off);
    }
    // section 2: the MEM records
    for (uint64_t mb = m0; mb < m1; mb += 64) {
        const uint64_t m = mb + lane;
        const bool live = m < m1;
        uint64_t f[6] = {0, 0, 0, 0, 0, 0};
        uint32_t l = 0;
        if (live) {
            const ulonglong2 *q = reinterpret_cast<const ulonglong2 *>(mems + m);
            const ulonglong2 x = q[0], y = q[1];
            f[0] = x.x; f[1] = x.y - x.x; f[2] = y.x; f[3] = y.y;
            l = pgx_varint_len(f[0]) + pgx_varint_len(f[1]) + pgx_varint_len(f[2]) + pgx_varint_len(f[3]);
            if (tags) {
                f[4] = run_nums[m];
                f[5] = pos_off[m + 1] - pos_off[m];
                l += pgx_varint_len(f[4]) + pgx_varint_len(f[5]);
            }
        }
        const uint32_t inc = pgx_wave_incl_scan(l, total);
        if (FILL && live) {
            uint8_t *p = sink.at(off, inc - l);
            p = pgx_varint_put(p, f[0]);
            p = pgx_varint_put(p, f[1]);
            p = pgx_varint_put(p, f[2]);
            p = pgx_varint_put(p, f[3]);
            if (tags) {
                p = pgx_varint_put(p, f[4]);
                pgx_varint_put(p, f[5]);
            }
        }
        off += total;
        sink.round_done(off);
    }
    // section 3: the positions, the first of a MEM as it is, the others as differences (mod 2^64)
    uint64_t p0 = 0;
    if (tags) {
        p0 = pos_off[m0];
        const uint64_t p1 = pos_off[m1];
        uint64_t mc = m0; // first MEM whose pos_off is not below the round's window
        for (uint64_t pb = p0; pb < p1; pb += 64) {
            uint64_t mask = 0;
            for (;;) {
                const uint64_t mi = mc + lane;
                const uint64_t po = mi < m1 ? pos_off[mi] : ~(uint64_t)0;
                const bool in_win = po - pb < 64; // (po >= pb: the cursor; an entry below it, which no valid result has, falls outside as well)
                mask |= in_win ? (uint64_t)1 << (po - pb) : 0;
                const uint32_t cnt = (uint32_t)__popcll(__ballot(po < pb + 64));
                mc += cnt;
                if (cnt < 64) break;
            }
            mask = pgx_wave_or(mask);
            const uint64_t p = pb + lane;
            const bool live = p < p1;
            uint64_t d = 0;
            uint32_t l = 0;
            if (live) {
                d = positions[p];
                if (!((mask >> lane) & 1)) d -= positions[p - 1]; // (p > p0: position p0 opens the block's first MEM that has any)
                l = pgx_varint_len(d);
            }
            const uint32_t inc = pgx_wave_incl_scan(l, total);
            if (FILL && live) pgx_varint_put(sink.at(off, inc - l), d);
            off += total;
            sink.round_done(off);
        }
    }
    p0_out = p0;
    sink.finish(off);
    return off;
}

// sizes[k] = bytes of block k padded to 8 (k < n_blocks); first_mem / first_pos[k] for k <= n_blocks
__global__ void __launch_bounds__(256)
pgx_compact_size_kernel(const uint64_t *__restrict__ mem_off, const pgx_mem *__restrict__ mems, const uint64_t *__restrict__ run_nums,
                        const uint64_t *__restrict__ pos_off, const uint64_t *__restrict__ positions, uint64_t n_reads, uint64_t n_blocks, int tags,
                        uint64_t *__restrict__ sizes, uint64_t *__restrict__ first_mem, uint64_t *__restrict__ first_pos) {
    const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (k > n_blocks) return;
    if (k == n_blocks) { // the closing entries of the tables
        if (lane == 0) {
            const uint64_t m = mem_off[n_reads];
            first_mem[k] = m;
            first_pos[k] = tags ? pos_off[m] : 0;
        }
        return;
    }
    uint64_t m0, p0;
    const uint64_t end = pgx_compact_walk<0>(mem_off, mems, run_nums, pos_off, positions, n_reads, k, tags != 0, 0, nullptr, nullptr, m0, p0);
    if (lane == 0) {
        sizes[k] = (end + 7) & ~(uint64_t)7;
        first_mem[k] = m0;
        first_pos[k] = p0;
    }
}

__global__ void __launch_bounds__(256)
pgx_compact_fill_kernel(const uint64_t *__restrict__ mem_off, const pgx_mem *__restrict__ mems, const uint64_t *__restrict__ run_nums,
                        const uint64_t *__restrict__ pos_off, const uint64_t *__restrict__ positions, uint64_t n_reads, uint64_t n_blocks, int tags,
                        const uint64_t *__restrict__ block_offsets, uint8_t *__restrict__ bytes) {
    const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (k >= n_blocks) return;
    uint64_t m0, p0;
    const uint64_t end = pgx_compact_walk<1>(mem_off, mems, run_nums, pos_off, positions, n_reads, k, tags != 0, block_offsets[k], bytes, nullptr, m0, p0);
    const uint64_t stop = block_offsets[k + 1]; // zero padding (fewer than 8 bytes)
    if (end + lane < stop) bytes[end + lane] = 0;
}

// the same through the LDS stage (PgxCompactSink<2>): every global store is 8 bytes, the padding is part of the block's last word
__global__ void __launch_bounds__(256)
pgx_compact_fill_staged_kernel(const uint64_t *__restrict__ mem_off, const pgx_mem *__restrict__ mems, const uint64_t *__restrict__ run_nums,
                               const uint64_t *__restrict__ pos_off, const uint64_t *__restrict__ positions, uint64_t n_reads, uint64_t n_blocks, int tags,
                               const uint64_t *__restrict__ block_offsets, uint8_t *__restrict__ bytes) {
    __shared__ uint64_t s_stage[4][PGX_COMPACT_STAGE_WORDS];
    const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n_blocks) return;
    uint64_t m0, p0;
    pgx_compact_walk<2>(mem_off, mems, run_nums, pos_off, positions, n_reads, k, tags != 0, block_offsets[k], bytes,
                        reinterpret_cast<uint8_t *>(s_stage[threadIdx.x >> 6]), m0, p0);
}
