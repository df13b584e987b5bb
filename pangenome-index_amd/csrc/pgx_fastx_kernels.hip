// pgx_fastx_kernels.hip -- reads as text (one read per line, FASTA, FASTQ) -> the CSR reads of a batch, on the device.
//
// The text crosses the link once, as it is; every pass below runs over what is already in device memory:
//   count    one block per 16 KiB tile, four coalesced 16-byte loads per thread, newlines counted in registers (SWAR compare + popcount)
//   (scan)   exclusive scan of the tile counts (scan_excl, pgx_runtime.hip)
//   lines    the same tiles again: block-wide scan of the per-thread counts, the start of every line into the line table
//   role     one thread per line: what the line is in its format, how many sequence bytes it gives, whether a record starts there;
//            structural errors as (line << 8 | code) into one word by atomicMin, so the first bad line wins
//   (scan)   exclusive scans of the sequence bytes and of the record starts over the lines
//   records  read offsets (rebased to 0) from the record-start lines; FASTA text before the first '>'
//   longest  the longest read (a strided grid, one atomicMax per block)
//   copy     output-centric: a block per 4 KiB of sequence, its lines found by binary search of the scanned byte counts, 16 bytes per
//            thread assembled in registers and written with one aligned store -- a 100 kbp line is spread over many blocks like any other
// Every index is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

// bit k of the result: byte k of the 16 at `base` is '\n' and lies before n
__device__ __forceinline__ uint32_t pgx_fx_newlines(uint4 v, uint64_t base, uint64_t n) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t x = w[q] ^ 0x0A0A0A0Au;
        const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; // high bit of every zero byte, exact
        m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * q);
    }
    if (base + 16 > n) m &= base < n ? (1u << (uint32_t)(n - base)) - 1u : 0u;
    return m;
}

__device__ __forceinline__ uint4 pgx_fx_load16(const uint8_t *text, uint64_t base, uint64_t n) {
    // (the text buffer has at least 16 bytes behind n: a chunk that starts before n may be loaded whole)
    return base < n ? *reinterpret_cast<const uint4 *>(text + base) : make_uint4(0u, 0u, 0u, 0u);
}

// exclusive prefix of v over the 256 threads of the block; *total = the block's sum.  s_w: 4 words of LDS
__device__ __forceinline__ uint32_t pgx_fx_block_excl(uint32_t v, uint32_t *s_w, uint32_t *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    __syncthreads(); // (s_w of the previous round has been read)
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) { if (i < w) base += s_w[i]; tot += s_w[i]; }
    *total = tot;
    return base + inc - v;
}

__global__ void __launch_bounds__(256)
pgx_fastx_count_kernel(const uint8_t *__restrict__ text, uint64_t n, uint32_t *__restrict__ tile_count) {
    __shared__ uint32_t s_w[4];
    const uint64_t t0 = (uint64_t)blockIdx.x * PGX_FASTX_TILE;
    uint4 v[PGX_FASTX_ROUNDS];
#pragma unroll
    for (int r = 0; r < PGX_FASTX_ROUNDS; r++) v[r] = pgx_fx_load16(text, t0 + (uint64_t)(r * 4096 + threadIdx.x * 16), n);
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < PGX_FASTX_ROUNDS; r++) c += __popc(pgx_fx_newlines(v[r], t0 + (uint64_t)(r * 4096 + threadIdx.x * 16), n));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_count[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// line i = bytes [ls[i], ls[i + 1] - 1): ls[0] = 0, ls[k + 1] = 1 + position of newline k; a last line without its newline ends at
// ls[n_lines] = n + 1 (tail != 0), as if the newline were there
__global__ void __launch_bounds__(256)
pgx_fastx_lines_kernel(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ tile_base, uint64_t *__restrict__ ls,
                       uint64_t n_lines, uint32_t tail) {
    __shared__ uint32_t s_w[4];
    const uint64_t t0 = (uint64_t)blockIdx.x * PGX_FASTX_TILE;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ls[0] = 0;
        if (tail) ls[n_lines] = n + 1;
    }
    uint4 v[PGX_FASTX_ROUNDS];
#pragma unroll
    for (int r = 0; r < PGX_FASTX_ROUNDS; r++) v[r] = pgx_fx_load16(text, t0 + (uint64_t)(r * 4096 + threadIdx.x * 16), n);
    uint64_t k = tile_base[blockIdx.x] + 1;
#pragma unroll
    for (int r = 0; r < PGX_FASTX_ROUNDS; r++) {
        const uint64_t base = t0 + (uint64_t)(r * 4096 + threadIdx.x * 16);
        uint32_t m = pgx_fx_newlines(v[r], base, n), tot;
        uint64_t at = k + pgx_fx_block_excl((uint32_t)__popc(m), s_w, &tot);
        while (m) {
            const int b = __ffs(m) - 1;
            ls[at++] = base + (uint64_t)b + 1;
            m &= m - 1;
        }
        k += tot;
    }
}

// per line: sequence bytes it adds (contrib) and whether a record starts on it (rec); the first structural error into *err
__global__ void __launch_bounds__(256)
pgx_fastx_role_kernel(const uint8_t *__restrict__ text, const uint64_t *__restrict__ ls, uint64_t n_lines, uint32_t format,
                      uint32_t *__restrict__ contrib, uint8_t *__restrict__ rec, unsigned long long *__restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lines) return;
    const uint64_t s = ls[i], len = ls[i + 1] - 1 - s;
    const uint8_t c0 = len ? text[s] : 0;
    const uint64_t cr = (len && text[s + len - 1] == '\r') ? 1 : 0;
    uint64_t add = 0;
    uint32_t code = 0, r = 0;
    if (format == PGX_READS_LINES) { // std::getline: '\r' kept, empty lines are no read
        r = len != 0;
        add = len;
    } else if (format == PGX_READS_FASTQ) {
        const uint32_t role = (uint32_t)(i & 3);
        if (role == 0) { r = 1; if (c0 != '@') code = PGX_FASTX_ERR_NO_AT; }
        else if (role == 1) add = len - cr;
        else if (role == 2) { if (c0 != '+') code = PGX_FASTX_ERR_NO_PLUS; }
        else {
            const uint64_t qs = ls[i - 2], ql = ls[i - 1] - 1 - qs, qcr = (ql && text[qs + ql - 1] == '\r') ? 1 : 0; // the sequence line
            if (len - cr != ql - qcr) code = PGX_FASTX_ERR_QUAL_LEN;
        }
        // a text that ends inside its record: reported for the record's header line, whatever the last line says of itself (the smaller word wins)
        if (i == n_lines - 1 && role != 3 && len < (1ull << 31)) atomicMin(err, (unsigned long long)((i - role) << 8 | PGX_FASTX_ERR_TRUNCATED));
    } else { // FASTA: a '>' line starts a record, every other line adds its bytes ('\r' stripped)
        if (c0 == '>') r = 1;
        else add = len - cr;
    }
    if (len >= (1ull << 31)) code = PGX_FASTX_ERR_LONG_LINE;
    contrib[i] = code == PGX_FASTX_ERR_LONG_LINE ? 0u : (uint32_t)add;
    rec[i] = (uint8_t)r;
    if (code) atomicMin(err, (unsigned long long)(i << 8 | code));
}

// offs[rec_idx[i]] = out_off[i] at every record start; offs[n_reads] = the total.  FASTA: a line with sequence bytes and no '>' line
// at or before it is text before the first record
__global__ void __launch_bounds__(256)
pgx_fastx_records_kernel(uint64_t n_lines, uint32_t format, const uint32_t *__restrict__ contrib, const uint8_t *__restrict__ rec,
                         const uint64_t *__restrict__ out_off, const uint64_t *__restrict__ rec_idx, uint64_t *__restrict__ offs,
                         unsigned long long *__restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lines) return;
    if (rec[i]) offs[rec_idx[i]] = out_off[i];
    else if (format == PGX_READS_FASTA && contrib[i] && rec_idx[i] == 0) atomicMin(err, (unsigned long long)(i << 8 | PGX_FASTX_ERR_BEFORE_FIRST));
    if (i == n_lines - 1) offs[rec_idx[n_lines]] = out_off[n_lines];
}

// the longest read: *longest = max over r < *n_reads of offs[r + 1] - offs[r].  A grid of at most a few thousand blocks strides over
// the reads and each block makes one atomicMax (one per wave over four million lines queued 65 536 atomics on one word: 188 us)
__global__ void __launch_bounds__(256)
pgx_fastx_longest_kernel(const uint64_t *__restrict__ offs, const uint64_t *__restrict__ n_reads, unsigned long long *__restrict__ longest) {
    __shared__ unsigned long long s_w[4];
    const uint64_t n = *n_reads;
    unsigned long long len = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long l = (unsigned long long)(offs[r + 1] - offs[r]);
        len = l > len ? l : len;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long t = __shfl_down(len, off, 64);
        len = t > len ? t : len;
    }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = len;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = s_w[0];
        for (int i = 1; i < 4; i++) m = s_w[i] > m ? s_w[i] : m;
        if (m) atomicMax(longest, m);
    }
}

// last line i < n_lines with out_off[i] <= p, searched in [lo, hi]: the line that holds output byte p (a line that adds no byte has
// out_off[i] == out_off[i + 1], so the last one at or below p is the line whose bytes cover p)
__device__ __forceinline__ uint64_t pgx_fx_find(const uint64_t *__restrict__ out_off, uint64_t p, uint64_t lo, uint64_t hi) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (out_off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// out[0, total) = the sequence bytes of every line in line order; bytes [total, the end of the last 16) are written 0
__global__ void __launch_bounds__(256)
pgx_fastx_copy_kernel(const uint8_t *__restrict__ text, const uint64_t *__restrict__ ls, const uint64_t *__restrict__ out_off, uint64_t n_lines,
                      uint64_t total, uint8_t *__restrict__ out) {
    __shared__ uint64_t s_lo, s_hi;
    const uint64_t t0 = (uint64_t)blockIdx.x * 4096;
    if (threadIdx.x == 0) s_lo = pgx_fx_find(out_off, t0, 0, n_lines - 1);
    if (threadIdx.x == 64) s_hi = pgx_fx_find(out_off, (t0 + 4095 < total ? t0 + 4095 : total - 1), 0, n_lines - 1);
    __syncthreads();
    const uint64_t q = t0 + (uint64_t)threadIdx.x * 16;
    if (q >= total) return;
    uint64_t j = pgx_fx_find(out_off, q, s_lo, s_hi);
    uint64_t lim = out_off[j + 1], src = ls[j] + (q - out_off[j]);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint64_t p = q + (uint64_t)k;
        if (p >= total) break;
        while (p >= lim) { j++; lim = out_off[j + 1]; src = ls[j]; }
        w[k >> 2] |= (uint32_t)text[src++] << (8 * (k & 3));
    }
    *reinterpret_cast<uint4 *>(out + q) = make_uint4(w[0], w[1], w[2], w[3]);
}
