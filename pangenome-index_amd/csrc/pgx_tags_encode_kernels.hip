// pgx_tags_encode_kernels.hip -- the query formats of a tag array (sdsl-compact and ByteCode, pgx_build.cpp write_compact_tags /
// pgx_convert_tags; sd_vector and select_support_mcl as pgx_sdsl.cpp writes them) from a run list on the device.
//
// Nothing in these formats depends on its left neighbour once three prefix sums exist (pieces, BWT positions and ByteCode bytes per
// run), so every pass is one thread per unit of OUTPUT:
//   count     per run: pieces (of <= 511), length, ByteCode bytes; the largest node id (block maximum, then one atomicMax)
//   expand    per piece (a block per 256 runs, their offsets in LDS): BWT start, item value, byte offset of every 10th, ByteCode bytes
//   pack      per 64-bit word of an int_vector: the items that overlap it are gathered and shifted into place
//   sd high   per word of the high bit vector: first one at or behind the word by binary search (the i-th one sits at (ones[i] >> wl) + i)
//   select    per superblock of 4096 arguments: size and kind first (scan -> file offsets), then a wave per superblock fills it.
//             The a-th one sits at (ones[a] >> wl) + a, the a-th zero at a + |{i : ones[i] < (a + 1) << wl}| (one binary search).
// Words of the file start at odd byte offsets (the one-byte width fields), so they are stored through pgx_te_store64.  No kernel
// reads what another block of the same launch wrote, and the only atomics are a maximum and an OR: the bytes do not depend on
// any order.  Every index, count and offset is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

__device__ __forceinline__ uint32_t pgx_te_bits(uint64_t x) { return x ? 64u - (uint32_t)__builtin_clzll(x) : 1u; } // sdsl::bits::hi(x) + 1
__device__ __forceinline__ void pgx_te_store64(uint8_t *p, uint64_t v) { __builtin_memcpy(p, &v, 8); }

__device__ __forceinline__ uint32_t pgx_te_bytecode_bytes(uint64_t x) {
    uint32_t b = 1;
    while (x >= 0x80) { x >>= 7; b++; }
    return b;
}
// encode_run_length (src/tag_arrays.cpp:28-36)
__device__ __forceinline__ uint64_t pgx_te_piece_code(uint64_t v, uint64_t len) { return (v & 0x7FF) | (len << 11) | ((v >> 11) << 20); }

__device__ __forceinline__ uint64_t pgx_te_len(const PgxTeRuns &r, uint64_t i) {
    uint64_t len = r.aux_is_start ? (i + 1 < r.n_runs ? r.aux[i + 1] : r.n_end) - r.aux[i] : r.aux[i];
    if (r.mod16) len &= 0xFFFF;
    return len;
}

__global__ void __launch_bounds__(256)
pgx_te_count_kernel(PgxTeRuns runs, uint32_t zero_counts, uint64_t *__restrict__ n_pieces, uint64_t *__restrict__ lens, uint64_t *__restrict__ n_bytes,
                    unsigned long long *__restrict__ max_node) {
    __shared__ uint64_t s_max[4];
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t node = 0;
    if (i < runs.n_runs) {
        const uint64_t len = pgx_te_len(runs, i), v = runs.val[i];
        const uint64_t p = len ? (len + 510) / 511 : 0;
        n_pieces[i] = p;
        lens[i] = len;
        if (n_bytes)
            n_bytes[i] = p ? (p - 1) * pgx_te_bytecode_bytes(pgx_te_piece_code(v, 511)) + pgx_te_bytecode_bytes(pgx_te_piece_code(v, len - 511 * (p - 1))) : 0;
        if (len || zero_counts) node = v >> 11;
    }
    for (int d = 32; d; d >>= 1) {
        const uint64_t o = __shfl_xor(node, d, 64);
        node = o > node ? o : node;
    }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = node;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) node = s_max[w] > node ? s_max[w] : node;
        if (node) atomicMax(max_node, (unsigned long long)node);
    }
}

// what == PGX_TE_EXPAND_PIECES: pos[j], items[j] (compact), sstart[j / 10] (ByteCode); PGX_TE_EXPAND_STREAM: the ByteCodes into `stream`
__global__ void __launch_bounds__(256)
pgx_te_expand_kernel(PgxTeRuns runs, const uint64_t *__restrict__ piece_off, const uint64_t *__restrict__ pos_off, const uint64_t *__restrict__ byte_off,
                     uint32_t what, uint64_t *__restrict__ pos, uint64_t *__restrict__ items, uint64_t *__restrict__ sstart, uint8_t *__restrict__ stream) {
    __shared__ uint64_t s_off[257];
    const uint64_t r0 = (uint64_t)blockIdx.x * 256;
    for (uint32_t t = threadIdx.x; t < 257; t += 256) s_off[t] = piece_off[r0 + t < runs.n_runs ? r0 + t : runs.n_runs];
    __syncthreads();
    const uint64_t j0 = s_off[0], j1 = s_off[256];
    for (uint64_t j = j0 + threadIdx.x; j < j1; j += 256) {
        uint32_t lo = 0, hi = 256; // last t with s_off[t] <= j (s_off[256] > j, so t <= 255: a run of the tile, with at least one piece)
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (s_off[mid] <= j) lo = mid; else hi = mid - 1;
        }
        const uint64_t r = r0 + lo, k = j - s_off[lo], v = runs.val[r];
        if (what == PGX_TE_EXPAND_PIECES) {
            pos[j] = pos_off[r] + 511 * k;
            if (items) items[j] = v;
            if (sstart && j % 10 == 0) sstart[j / 10] = byte_off[r] + k * pgx_te_bytecode_bytes(pgx_te_piece_code(v, 511));
        } else {
            const uint64_t np = s_off[lo + 1] - s_off[lo];
            const uint64_t len = k + 1 < np ? 511 : pgx_te_len(runs, r) - 511 * (np - 1);
            uint64_t o = byte_off[r] + k * pgx_te_bytecode_bytes(pgx_te_piece_code(v, 511)), x = pgx_te_piece_code(v, len);
            while (x >= 0x80) { stream[o++] = (uint8_t)((x & 0x7F) | 0x80); x >>= 7; }
            stream[o] = (uint8_t)x;
        }
    }
}

// word w of int_vector::pack: values i with [i * width, (i + 1) * width) overlapping bits [64 w, 64 w + 64), i < count
template <class Get>
__device__ __forceinline__ uint64_t pgx_te_pack_word(uint64_t w, uint32_t width, uint64_t count, Get get) {
    const uint64_t b0 = w << 6, mask = width >= 64 ? ~0ull : (1ull << width) - 1;
    uint64_t word = 0;
    for (uint64_t i = b0 / width; i < count; i++) {
        const uint64_t bit = i * width;
        if (bit >= b0 + 64) break;
        const uint64_t x = get(i) & mask;
        word |= bit >= b0 ? x << (bit - b0) : x >> (b0 - bit);
    }
    return word;
}

__global__ void __launch_bounds__(256)
pgx_te_pack_items_kernel(const uint64_t *__restrict__ items, uint64_t count, uint32_t width, uint8_t *__restrict__ out, uint64_t n_words) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    pgx_te_store64(out + w * 8, pgx_te_pack_word(w, width, count, [&](uint64_t i) { return items[i]; }));
}

__device__ __forceinline__ uint64_t pgx_te_one(const PgxTeSd &sd, uint64_t i) { return sd.ones ? sd.ones[i] : i * 10; }
// ones below x
__device__ __forceinline__ uint64_t pgx_te_ones_below(const PgxTeSd &sd, uint64_t x) {
    uint64_t lo = 0, hi = sd.m;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (pgx_te_one(sd, mid) < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// position of the a-th one (b = 1) / zero (b = 0) of the high bit vector
__device__ __forceinline__ uint64_t pgx_te_arg(const PgxTeSd &sd, uint32_t b, uint64_t a) {
    return b ? (pgx_te_one(sd, a) >> sd.wl) + a : a + pgx_te_ones_below(sd, (a + 1) << sd.wl);
}

__global__ void __launch_bounds__(256)
pgx_te_sd_low_kernel(PgxTeSd sd, uint8_t *__restrict__ out, uint64_t n_words) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    pgx_te_store64(out + w * 8, pgx_te_pack_word(w, sd.wl, sd.m, [&](uint64_t i) { return pgx_te_one(sd, i); }));
}

__global__ void __launch_bounds__(256)
pgx_te_sd_high_kernel(PgxTeSd sd, uint8_t *__restrict__ out, uint64_t n_words) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const uint64_t b0 = w << 6;
    uint64_t lo = 0, hi = sd.m; // first one at or behind bit b0 (positions ascend strictly)
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if ((pgx_te_one(sd, mid) >> sd.wl) + mid < b0) lo = mid + 1; else hi = mid;
    }
    uint64_t word = 0;
    for (uint64_t i = lo; i < sd.m; i++) {
        const uint64_t p = (pgx_te_one(sd, i) >> sd.wl) + i;
        if (p >= b0 + 64) break;
        word |= 1ull << (p - b0);
    }
    pgx_te_store64(out + w * 8, word);
}

// superblock q of select_support_mcl<b>: first argument, kind and width (meta = width | long << 7), serialised bytes of its int_vector
__global__ void __launch_bounds__(256)
pgx_te_sel_size_kernel(PgxTeSd sd, uint32_t b, uint64_t arg_cnt, uint64_t n_sb, uint64_t logn4, uint64_t *__restrict__ first, uint8_t *__restrict__ meta,
                       uint64_t *__restrict__ sizes, unsigned int *__restrict__ any_long) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_sb) return;
    const uint64_t a0 = q << 12, a1 = a0 + 4095 < arg_cnt ? a0 + 4095 : arg_cnt - 1;
    const uint64_t f = pgx_te_arg(sd, b, a0), l = pgx_te_arg(sd, b, a1);
    const bool lng = l - f > logn4;
    const uint32_t width = lng ? pgx_te_bits(l) : pgx_te_bits(l - f);
    first[q] = f;
    meta[q] = (uint8_t)(width | (lng ? 0x80u : 0u));
    sizes[q] = 9 + (uint64_t)width * (lng ? 512 : 8);
    if (lng) atomicOr(any_long, 1u);
}

__global__ void __launch_bounds__(256)
pgx_te_sel_super_kernel(const uint64_t *__restrict__ first, uint64_t n_sb, uint32_t logn, uint8_t *__restrict__ out, uint64_t n_words) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    pgx_te_store64(out + w * 8, pgx_te_pack_word(w, logn, n_sb, [&](uint64_t i) { return first[i]; }));
}

// mini_or_long: bit q set where superblock q is NOT long
__global__ void __launch_bounds__(256)
pgx_te_sel_kind_kernel(const uint8_t *__restrict__ meta, uint64_t n_sb, uint8_t *__restrict__ out, uint64_t n_words) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    pgx_te_store64(out + w * 8, pgx_te_pack_word(w, 1, n_sb, [&](uint64_t i) { return (uint64_t)((meta[i] >> 7) ^ 1); }));
}

// one wave per superblock: header of its int_vector (bit count, width), then its words.  long: 4096 absolute positions (0 beyond the
// last argument); mini: 64 offsets from the first argument, one per 64 arguments
__global__ void __launch_bounds__(64)
pgx_te_sel_body_kernel(PgxTeSd sd, uint32_t b, uint64_t arg_cnt, const uint64_t *__restrict__ first, const uint8_t *__restrict__ meta,
                       const uint64_t *__restrict__ off, uint8_t *__restrict__ out) {
    const uint64_t q = blockIdx.x, a0 = q << 12, last = a0 + 4095 < arg_cnt ? 4095 : arg_cnt - 1 - a0;
    const uint32_t width = meta[q] & 0x7F;
    const bool lng = (meta[q] & 0x80) != 0;
    const uint64_t f = first[q], count = lng ? 4096 : 64, n_words = (count * width) >> 6;
    uint8_t *o = out + off[q];
    if (threadIdx.x == 0) {
        pgx_te_store64(o, count * width);
        o[8] = (uint8_t)width;
    }
    for (uint64_t w = threadIdx.x; w < n_words; w += 64) {
        const uint64_t word = lng ? pgx_te_pack_word(w, width, count, [&](uint64_t i) { return i <= last ? pgx_te_arg(sd, b, a0 + i) : 0ull; })
                                  : pgx_te_pack_word(w, width, count, [&](uint64_t i) { return i * 64 <= last ? pgx_te_arg(sd, b, a0 + i * 64) - f : 0ull; });
        pgx_te_store64(o + 9 + w * 8, word);
    }
}

// the scalar fields of the file: `bytes` low bytes of `value` at `offset`
__global__ void __launch_bounds__(64)
pgx_te_fields_kernel(const PgxTeField *__restrict__ fields, uint32_t n, uint8_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PgxTeField f = fields[i];
    for (uint32_t k = 0; k < f.bytes; k++) out[f.offset + k] = (uint8_t)(f.value >> (8 * k));
}
