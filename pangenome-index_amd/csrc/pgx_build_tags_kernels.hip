// pgx_build_tags_kernels.hip -- build_tags (src/build_tags.cpp) as data-parallel passes over the suffix array.
//
// The reference finds unique k-mers, builds a B+-tree, extends by BFS and walks every sequence with psi to learn the graph
// position of each BWT row.  That position is simply the text position SA[i] = (sequence s, offset off) read on the graph:
// the node of path s that covers off.  So, with the SA of the whole BWT from the locate kernels (pgx_locate_kernels.hip):
//   endmarker rows [0, n_seq): SA[i] = (s, |s|) -- the index's sequence lengths, checked against the paths by the host
//   tag of row i >= n_seq      per-sequence directory (one entry per 1024 text positions) + binary search among the path's
//                              node starts inside the bucket (nodes are <= 1024 bp, so a bucket spans at most 1024 of them +1),
//                              written over SA[i] in place
//   run heads -> exclusive scan -> compaction into (value, start); lengths (mod 65 536 in reference mode)
//   ByteCode bytes of every run (pieces of <= 511) -> exclusive scan -> ByteCode write
// Every index is 64-bit: n >= 2^32 rows is fine.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

// gbwt::ByteCode length of x
__device__ __forceinline__ uint32_t pgx_bt_bytecode_bytes(uint64_t x) {
    uint32_t b = 1;
    while (x >= 0x80) { x >>= 7; b++; }
    return b;
}

// encode_run_length (src/tag_arrays.cpp:28-36): offset:10 | rev:1 | len:9 | node << 20, from tag = node << 11 | rev << 10 | offset
__device__ __forceinline__ uint64_t pgx_bt_piece_code(uint64_t tag, uint64_t len) { return (tag & 0x7FF) | (len << 11) | ((tag >> 11) << 20); }

// the index's length of every sequence: idx_len[s] = off of the endmarker row of s (host fills ~0 first; a sequence left
// without one, or a row naming a sequence beyond n_seq, is reported by the host)
__global__ void __launch_bounds__(256)
pgx_bt_endmarker_kernel(const uint64_t *__restrict__ sa, uint64_t n_seq, uint64_t max_length, uint64_t *__restrict__ idx_len) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_seq) return;
    const uint64_t v = sa[i], s = v / max_length;
    if (s < n_seq) idx_len[s] = v % max_length;
}

// tag of every row >= n_seq, over the SA value in place.  A row whose sequence is unknown or whose offset lies beyond its
// path: tag 0 and atomicMin of the sequence into *bad (the host reports it and writes nothing)
__global__ void __launch_bounds__(256)
pgx_bt_tag_kernel(uint64_t *__restrict__ sa, uint64_t n, uint64_t n_seq, uint64_t max_length, const uint64_t *__restrict__ seq_len,
                  const uint64_t *__restrict__ dir_off, const uint64_t *__restrict__ dir, const uint64_t *__restrict__ node_start,
                  const uint64_t *__restrict__ path_nodes, unsigned long long *__restrict__ bad) {
    const uint64_t i = n_seq + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t v = sa[i], s = v / max_length, off = v - s * max_length;
    if (s >= n_seq || off >= seq_len[s]) {
        atomicMin(bad, (unsigned long long)s);
        sa[i] = 0;
        return;
    }
    const uint64_t d = dir_off[s] + (off >> 10);
    uint64_t lo = dir[d], hi = dir[d + 1]; // the node covering off is in [lo, hi]: last one with node_start <= off
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (node_start[mid] <= off) lo = mid; else hi = mid - 1;
    }
    const uint64_t node = path_nodes[lo]; // id << 1 | rev
    sa[i] = ((node >> 1) << 11) | ((node & 1) << 10) | (off - node_start[lo]);
}

// run heads among the rows >= n_seq (the endmarker rows belong to no run)
__global__ void __launch_bounds__(256)
pgx_bt_heads_kernel(const uint64_t *__restrict__ tags, uint64_t n, uint64_t n_seq, uint8_t *__restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    head[i] = i >= n_seq && (i == n_seq || tags[i] != tags[i - 1]) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
pgx_bt_compact_kernel(const uint64_t *__restrict__ tags, const uint8_t *__restrict__ head, const uint64_t *__restrict__ idx, uint64_t n,
                      uint64_t *__restrict__ run_val, uint64_t *__restrict__ run_start) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !head[i]) return;
    run_val[idx[i]] = tags[i];
    run_start[idx[i]] = i;
}

// length of run r (next start - start); reference mode: mod 65 536 (0 = the run is written as nothing)
__global__ void __launch_bounds__(256)
pgx_bt_length_kernel(const uint64_t *__restrict__ run_start, uint64_t n_runs, uint64_t n, uint32_t reference_runs, uint64_t *__restrict__ run_len) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    uint64_t len = (r + 1 < n_runs ? run_start[r + 1] : n) - run_start[r];
    if (reference_runs) len &= 0xFFFF;
    run_len[r] = len;
}

// ByteCode bytes of run r: ceil(len / 511) pieces, all of 511 but the last (tag_arrays.cpp:941-957: while len >= 512 emit 511)
__global__ void __launch_bounds__(256)
pgx_bt_size_kernel(const uint64_t *__restrict__ run_val, const uint64_t *__restrict__ run_len, uint64_t n_runs, uint64_t *__restrict__ bytes) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    const uint64_t len = run_len[r], t = run_val[r];
    if (!len) { bytes[r] = 0; return; }
    const uint64_t p = (len + 510) / 511, last = len - 511 * (p - 1);
    bytes[r] = (p - 1) * pgx_bt_bytecode_bytes(pgx_bt_piece_code(t, 511)) + pgx_bt_bytecode_bytes(pgx_bt_piece_code(t, last));
}

__global__ void __launch_bounds__(256)
pgx_bt_write_kernel(const uint64_t *__restrict__ run_val, const uint64_t *__restrict__ run_len, const uint64_t *__restrict__ byte_off, uint64_t n_runs,
                    uint8_t *__restrict__ body) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    uint64_t len = run_len[r], o = byte_off[r];
    const uint64_t t = run_val[r];
    while (len) {
        const uint64_t piece = len >= 512 ? 511 : len;
        uint64_t x = pgx_bt_piece_code(t, piece);
        while (x >= 0x80) { body[o++] = (uint8_t)((x & 0x7F) | 0x80); x >>= 7; }
        body[o++] = (uint8_t)x;
        len -= piece;
    }
}
