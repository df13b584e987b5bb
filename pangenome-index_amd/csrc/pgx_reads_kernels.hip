// pgx_reads_kernels.hip -- per-upload passes over the reads (gfx950): the reads with a byte outside A C G T are found and listed,
// reads are packed to two bits per symbol or unpacked back to bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"
#include "pgx_rank_device.h"

// ------------------------------------------------------------------------------------------
// Reads with a byte outside A C G T (upper case): no seed applies to a window that holds one, so the two-step kernel could only hand
// them on after two trips -- and they are the long chains of the hand-on launch (a read cut from an N run has thousands of extensions).
// Found once per upload, they go to the dense2 kernel on a second stream WHILE the two-step kernel runs, which skips them.
// Two passes: a streaming one over the read bytes (16 per lane, coalesced) that lists the 16-byte chunks holding such a byte, and one
// thread per listed chunk that finds the reads its bad bytes belong to (binary search in the offsets), flags them and lists each once.
// (packed != NULL: the same pass writes the reads as two bits per symbol, 16 symbols per dword, A C T G = 0 1 2 3 -- the code order of the seed
//  index --, for pgx_find_mems_pairs_kernel<.., PACKED>; symbols of a chunk that holds another byte are junk, and so is what the reads flagged here stand for)
__global__ void __launch_bounds__(256)
pgx_bad_chunks_kernel(const uint8_t *__restrict__ reads, uint64_t n_bytes, uint64_t *__restrict__ chunks, unsigned long long *__restrict__ count, uint64_t cap,
                      uint32_t *__restrict__ packed) {
    const uint64_t n_chunks = (n_bytes + 15) >> 4; // (32 zero bytes follow the last read: the last chunk may be read whole)
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * blockDim.x) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(reads + (c << 4));
        uint64_t b0, b1;
        const uint32_t c0 = pgx_seed_codes(v.x, b0);
        const uint32_t c1 = pgx_seed_codes(v.y, b1);
        if (packed) packed[c] = c0 | (c1 << 16);
        const uint64_t left = n_bytes - (c << 4); // bytes of the chunk that belong to reads
        if (left < 8) { b0 &= (1ull << (8 * left)) - 1ull; b1 = 0; }
        else if (left < 16) b1 &= (1ull << (8 * (left - 8))) - 1ull;
        if (b0 | b1) {
            const unsigned long long at = atomicAdd(count, 1ull);
            if (at < cap) chunks[at] = c;
        }
    }
}
__global__ void __launch_bounds__(256)
pgx_classify_reads_kernel(const uint8_t *__restrict__ reads, const uint64_t *__restrict__ offsets, uint64_t n_reads, const uint64_t *__restrict__ chunks,
                          const unsigned long long *__restrict__ n_chunks, uint64_t cap, uint32_t *__restrict__ flag_words, pgx_heavy_item *__restrict__ list,
                          unsigned long long *__restrict__ count) {
    const uint64_t nc = *n_chunks < cap ? *n_chunks : cap;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const uint64_t p0 = chunks[i] << 4, total = offsets[n_reads];
    uint64_t rid = ~0ull, rend = 0;
    for (uint32_t k = 0; k < 16 && p0 + k < total; k++) {
        const uint64_t p = p0 + k;
        uint64_t bad;
        (void)pgx_seed_codes((uint64_t)reads[p] | 0x4141414141414100ull, bad); // the other seven bytes read as 'A'
        if (!(bad & 0xFFull)) continue;
        if (rid == ~0ull || p >= rend) { // the read holding byte p: the last one whose offset is <= p (empty reads hold nothing)
            uint64_t lo = 0, hi = n_reads;
            while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (offsets[mid + 1] <= p) lo = mid + 1; else hi = mid; }
            rid = lo; rend = offsets[rid + 1];
        }
        const uint32_t bit = 1u << (8u * (uint32_t)(rid & 3));
        if (!(atomicOr(flag_words + (rid >> 2), bit) & bit)) {
            pgx_heavy_item it;
            it.rid = rid; it.x = 0; it.nm = 0;
            list[atomicAdd(count, 1ull)] = it;
        }
    }
}

// Reads that arrive packed (pgx_batch_upload_packed: two bits per symbol from the host, a quarter of the bytes over the link): back to bytes for the
// kernels that read bytes ("ACTG"[code]; one packed word = 16 symbols per thread, one 16-byte store) ...
__global__ void __launch_bounds__(256)
pgx_unpack_reads_kernel(const uint32_t *__restrict__ packed, uint64_t n_chunks, uint8_t *__restrict__ reads) {
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t w = packed[c];
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) v |= ((0x47544341u >> (8u * ((w >> (2 * (4 * q + k))) & 3u))) & 0xFFu) << (8 * k);
            o[q] = v;
        }
        *reinterpret_cast<uint4 *>(reads + (c << 4)) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}
// ... and the reads that hold a byte outside A C G T, which the host lists with their bytes as they are: copied over what the packed words gave,
// flagged for the two-step kernel to skip and listed for the kernel that serves them (what pgx_bad_chunks_kernel + pgx_classify_reads_kernel
// find on the device when the reads arrive as bytes).  One 64-lane wave per listed read.
__global__ void __launch_bounds__(256)
pgx_side_reads_kernel(uint8_t *__restrict__ reads, const uint64_t *__restrict__ offsets, const uint64_t *__restrict__ side_ids, const uint64_t *__restrict__ side_off,
                      const uint8_t *__restrict__ side_bytes, uint64_t n_side, uint8_t *__restrict__ flags, pgx_heavy_item *__restrict__ list,
                      unsigned long long *__restrict__ count) {
    const uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    if (k >= n_side) return;
    const uint64_t rid = side_ids[k], dst = offsets[rid], len = offsets[rid + 1] - dst, src = side_off[k];
    for (uint64_t i = lane; i < len; i += 64) reads[dst + i] = side_bytes[src + i];
    if (lane == 0) {
        flags[rid] = 1;
        pgx_heavy_item it;
        it.rid = rid; it.x = 0; it.nm = 0;
        list[k] = it;
        if (k == 0) *count = n_side;
    }
}
