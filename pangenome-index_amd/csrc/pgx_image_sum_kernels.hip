// pgx_image_sum_kernels.hip -- the section sum of an image file (include/pgx.h "SECTION SUM") over device memory: what pgx_images.hip runs over
// every section of an image-opened handle right after its upload, before any other kernel reads it, and what pgx_image_sum(device >= 0) runs.
//
// A plain streaming reduction: every thread walks 16-byte units (two words of the sum) grid-stride with four loads in flight, adds its
// terms in a register, then the wave adds by shuffles, the waves of a block through LDS, and one thread per block adds to the result with
// one 64-bit atomicAdd.  The sum is a wrap-around addition of terms that depend on (word, word index) alone, so the order in which lanes,
// waves and blocks add does not matter: the result is the host's, bit for bit.  Word and unit indices are 64-bit throughout (the wide
// PAIRS image of a 2^32-symbol index is 8.7 GB).  It reads bytes [0, n_bytes) of `data` and nothing else, and writes 8 bytes.
#include "pgx_device.h"

static __device__ __forceinline__ uint64_t pgx_sum_mix(uint64_t z) {
    z = (z ^ (z >> 32)) * 0xD6E8FEB86659FD93ull;
    return z ^ (z >> 32);
}

#define PGX_SUM_GOLD 0x9E3779B97F4A7C15ull

// data: 16-byte aligned; *sum must be zero before the launch (or hold what the result is to be added to)
__global__ void __launch_bounds__(256) pgx_image_sum_kernel(const uint4 *__restrict__ data, uint64_t n_bytes, unsigned long long *sum) {
    const uint64_t n_units = n_bytes >> 4;                                  // whole 16-byte units = word pairs (2 u, 2 u + 1)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t acc = 0;
    // term of word i = mix(w + (i + 1) * GOLD): kept as a running value per thread, moved on by additions
    uint64_t g = (2 * u + 1) * PGX_SUM_GOLD;                                // (i + 1) * GOLD for i = 2 u
    const uint64_t g_step = 2 * stride * PGX_SUM_GOLD;
    for (; u + 3 * stride < n_units; u += 4 * stride) {                     // four independent loads in flight
        const uint4 a = data[u], b = data[u + stride], c = data[u + 2 * stride], d = data[u + 3 * stride];
        const uint64_t g1 = g + g_step, g2 = g1 + g_step, g3 = g2 + g_step;
        acc += pgx_sum_mix((((uint64_t)a.y << 32) | a.x) + g) + pgx_sum_mix((((uint64_t)a.w << 32) | a.z) + g + PGX_SUM_GOLD);
        acc += pgx_sum_mix((((uint64_t)b.y << 32) | b.x) + g1) + pgx_sum_mix((((uint64_t)b.w << 32) | b.z) + g1 + PGX_SUM_GOLD);
        acc += pgx_sum_mix((((uint64_t)c.y << 32) | c.x) + g2) + pgx_sum_mix((((uint64_t)c.w << 32) | c.z) + g2 + PGX_SUM_GOLD);
        acc += pgx_sum_mix((((uint64_t)d.y << 32) | d.x) + g3) + pgx_sum_mix((((uint64_t)d.w << 32) | d.z) + g3 + PGX_SUM_GOLD);
        g = g3 + g_step;
    }
    for (; u < n_units; u += stride) {
        const uint4 a = data[u];
        acc += pgx_sum_mix((((uint64_t)a.y << 32) | a.x) + g) + pgx_sum_mix((((uint64_t)a.w << 32) | a.z) + g + PGX_SUM_GOLD);
        g += g_step;
    }
    // the last 1 .. 15 bytes: at most two words, the last one padded with zero bytes; read byte by byte so that nothing behind n_bytes is touched
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n_bytes & 15)) {
        const uint8_t *p = reinterpret_cast<const uint8_t *>(data);
        const uint64_t first = n_units << 1, n_words = (n_bytes + 7) >> 3;
        for (uint64_t i = first; i < n_words; i++) {
            uint64_t w = 0;
            for (uint64_t k = 0; k < 8 && (i << 3) + k < n_bytes; k++) w |= (uint64_t)p[(i << 3) + k] << (8 * k);
            acc += pgx_sum_mix(w + (i + 1) * PGX_SUM_GOLD);
        }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ uint64_t wave_sum[4];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_sum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t s = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        atomicAdd(sum, (unsigned long long)s);
    }
}
