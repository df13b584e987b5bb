// pgx_walk_device.h -- the __device__ lookups into the WALK image (pgx_image.h, PgxWalkImage) that more than one kernel file needs: the rank of a
// text position among the marks and the back scan to the mark of the visit that holds it.  Included by pgx_walk_kernels.hip and pgx_mapq_kernels.hip.
// Words are only read below the image's n_words (positions <= n).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

// set bits of [0, p), p <= n
__device__ __forceinline__ uint64_t walk_rank(const PgxWalkImage &w, uint64_t p) {
    const uint64_t blk = p / PGX_WALK_BLOCK_BITS, wi = p >> 6;
    uint64_t r = w.dir[blk];
    for (uint64_t j = blk * PGX_WALK_BLOCK_WORDS; j < wi; j++) r += (uint64_t)__popcll(w.bits[j]);
    const uint32_t b = (uint32_t)p & 63u;
    if (b) r += (uint64_t)__popcll(w.bits[wi] & ((1ull << b) - 1ull));
    return r;
}

// the last marked position in [max(lo, s - 1023), s]; that lower bound itself where there is none (a tag array that describes no paths)
__device__ __forceinline__ uint64_t walk_prev_mark(const PgxWalkImage &w, uint64_t s, uint64_t lo) {
    const uint64_t floor = (s >= PGX_WALK_MAX_VISIT - 1 && s - (PGX_WALK_MAX_VISIT - 1) > lo) ? s - (PGX_WALK_MAX_VISIT - 1) : lo;
    uint64_t wi = s >> 6;
    uint64_t word = w.bits[wi] & (~0ull >> (63u - ((uint32_t)s & 63u)));
    for (;;) { // at most 17 words
        if (word) {
            const uint64_t p = (wi << 6) + 63u - (uint64_t)__clzll((long long)word);
            return p > floor ? p : floor;
        }
        if ((wi << 6) <= floor) return floor;
        word = w.bits[--wi];
    }
}
