// pgx_align_kernels.hip -- read align (include/pgx.h "read align"): the banded unit-cost alignment of every read against the text around its
// candidate (sequence, diagonal), with traceback, one pgx_read_align a read and on request the CIGAR operations.
//
//   cand     a thread a read: the winner of its pgx_read_verify as (cand_seq, cand_diag)
//   need     a thread a read: the bytes of its direction planes (len rows, rounded up to 16 bytes), scanned into plane_off
//   forward  a group of G lanes a read, G the power of two >= 2 W + 1 (1 .. 64), so that 64 / G reads share a wave; lane l is diagonal
//            k = l - W and keeps D[i][i + d0 + k] of the current row.  A row is: the neighbour above (lane l + 1 of the row before, one
//            shuffle), one compare of the read's 4-bit code against the lane's text code (the coded reads of pgx_verify_code_kernel and the text
//            image, a word of eight symbols reloaded when the position crosses it: no byte loads), and the deletion term as a prefix minimum
//            of X[l] - l over the group (log2 G shuffles).  Every cell leaves two direction bits (0 '=', 1 'X', 2 'I', 3 'D': the first move
//            of the traceback order that reproduces D), gathered by two ballots into two bit planes; lane 0 of the group stores the row.
//            The end cell is a minimum over the group of (D, |k|, k > 0).
//   trace    a lane a read: walks the planes from the end cell to row 0; mode 0 counts operations and fills the record, mode 1 writes the
//            operations from the read's last slot backwards
// The loop of the forward kernel runs to the longest read of the wave with finished groups idle, so that every shuffle and ballot sees all
// 64 lanes.  D stays below 2^28 (reads of 2^28 bytes or more are refused), ALIGN_INF = 2^30 stands for "no such cell" and survives the additions.
// A row of planes is plane 0 then plane 1, max(G, 8) bits each; a read's rows start at plane_off[r] - plane_off[first read of the pass].
// Text words are loaded only for a cell inside the sequence; every index is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

namespace {

constexpr uint32_t ALIGN_INF = 1u << 30;

struct AlignSpan { // the clips of a candidate (include/pgx.h): Q = R[lo, hi), m = hi - lo symbols on the main diagonal d0 of a sequence of Ls symbols at s0
    uint64_t roff, s0;
    int64_t len, Ls, lo, hi, d0;
};

__device__ __forceinline__ AlignSpan align_span(const uint64_t *__restrict__ seq_start, uint32_t endmark, const uint64_t *__restrict__ read_off, uint64_t r, uint32_t seq,
                                                int64_t diag) {
    AlignSpan a;
    a.roff = read_off[r];
    a.len = (int64_t)(read_off[r + 1] - a.roff);
    a.s0 = seq_start[seq];
    a.Ls = (int64_t)(seq_start[seq + 1] - a.s0) - (int64_t)endmark;
    a.lo = diag < 0 ? -diag : 0;
    a.hi = a.Ls - diag < a.len ? a.Ls - diag : a.len; // (|diag| stays far below 2^62, as in pgx_verify_kernel)
    if (a.hi <= a.lo) a.lo = a.hi = 0;
    a.d0 = a.hi > a.lo ? diag + a.lo : 0;
    return a;
}

} // namespace

__global__ void __launch_bounds__(256)
pgx_align_cand_kernel(const pgx_read_verify *__restrict__ recs, uint64_t n_reads, uint32_t *__restrict__ cand_seq, int64_t *__restrict__ cand_diag) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    cand_seq[r] = recs[r].seq;
    cand_diag[r] = recs[r].diag;
}

__global__ void __launch_bounds__(256)
pgx_align_need_kernel(const uint64_t *__restrict__ read_off, uint64_t n_reads, uint32_t row_bytes, uint64_t *__restrict__ need) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    need[r] = ((read_off[r + 1] - read_off[r]) * row_bytes + 15) & ~15ull;
}

template <int LG>
__global__ void __launch_bounds__(PGX_ALIGN_THREADS)
pgx_align_forward_kernel(const uint32_t *__restrict__ text4, const uint64_t *__restrict__ seq_start, uint32_t endmark, const uint32_t *__restrict__ rcode,
                         const uint64_t *__restrict__ read_off, const uint32_t *__restrict__ cand_seq, const int64_t *__restrict__ cand_diag, uint64_t r0, uint64_t r1,
                         uint32_t W, const uint64_t *__restrict__ plane_off, uint8_t *__restrict__ planes, uint2 *__restrict__ fwd) {
    constexpr int G = 1 << LG;
    constexpr uint32_t ROW = (G < 8 ? 8 : G) / 4; // bytes of a row: two planes
    const uint64_t r = r0 + (uint64_t)blockIdx.x * (PGX_ALIGN_THREADS >> LG) + (threadIdx.x >> LG);
    const uint32_t l = threadIdx.x & (G - 1);
    const uint32_t gb = threadIdx.x & 63u & ~(uint32_t)(G - 1); // the group's first lane in its wave
    const int64_t k = (int64_t)l - (int64_t)W;
    const bool lane_ok = l <= 2 * W;
    // (no thread leaves before the loop: the shuffles and ballots below want every lane of the wave)
    uint32_t m = 0;
    AlignSpan a{};
    if (r < r1 && cand_seq[r] != PGX_NO_SEQUENCE) {
        a = align_span(seq_start, endmark, read_off, r, cand_seq[r], cand_diag[r]);
        m = (uint32_t)(a.hi - a.lo);
    }
    uint32_t m_max = m;
#pragma unroll
    for (int o = 32; o >= G; o >>= 1) {
        const uint32_t t = (uint32_t)__shfl_xor((int)m_max, o, 64);
        m_max = t > m_max ? t : m_max;
    }
    uint8_t *const rows = m ? planes + (plane_off[r] - plane_off[r0]) : planes;
    const uint64_t g_first = a.roff + (uint64_t)a.lo; // Q[i - 1] is byte g_first + i - 1 of the concatenated reads
    uint32_t D = (m && lane_ok && a.d0 + k >= 0 && a.d0 + k <= a.Ls) ? 0u : ALIGN_INF; // row 0: the start in the text is free
    uint32_t rword = 0, tword = 0;
    int64_t tw_cur = -1;
    for (uint32_t i = 1; i <= m_max; i++) {
        const bool active = i <= m;
        const int64_t j = (int64_t)i + a.d0 + k;
        const bool cell = active && lane_ok && j >= 0 && j <= a.Ls;
        uint32_t rc = 15u, tc = 0u;
        if (active) {
            const uint64_t g = g_first + i - 1;
            if (i == 1 || (g & 7) == 0) rword = rcode[g >> 3];
            rc = (rword >> (4u * (uint32_t)(g & 7))) & 15u;
        }
        if (cell && j >= 1) {
            const int64_t t = (int64_t)a.s0 + j - 1, tw = t >> 3;
            if (tw != tw_cur) { tword = text4[tw]; tw_cur = tw; }
            tc = (tword >> (4u * (uint32_t)(t & 7))) & 15u;
        }
        const uint32_t sub = rc != tc; // (a read code is one of 1 2 3 5 15, a text code one of 0 .. 5: N, lower case and the endmarker match nothing)
        uint32_t up = (uint32_t)__shfl_down((int)D, 1, G); // D[i - 1][j]: diagonal k + 1 of the row before
        if (l == G - 1) up = ALIGN_INF;
        const uint32_t da = (cell && D < ALIGN_INF) ? D + sub : ALIGN_INF; // from D[i - 1][j - 1], this lane's cell of the row before
        const uint32_t db = up < ALIGN_INF ? up + 1 : ALIGN_INF;
        uint32_t y = (cell ? (da < db ? da : db) : ALIGN_INF) + (63u - l);
        // the deletion term: D[i][j] = min over j' <= j of X[j'] + (j - j'), a prefix minimum of X[l] - l (the valid cells of a row are consecutive lanes)
#pragma unroll
        for (int o = 1; o < G; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)y, o, G);
            if (l >= (uint32_t)o) y = t < y ? t : y;
        }
        uint32_t d = y - (63u - l);
        d = (cell && d < ALIGN_INF) ? d : ALIGN_INF;
        uint32_t code = 0;
        if (cell) code = (da < ALIGN_INF && d == da) ? sub : ((db < ALIGN_INF && d == db) ? 2u : 3u);
        const unsigned long long b0 = __ballot(code & 1u), b1 = __ballot(code >> 1);
        if (active) {
            D = d;
            if (l == 0) {
                uint8_t *const row = rows + (uint64_t)(i - 1) * ROW;
                if (G <= 8) *reinterpret_cast<uint16_t *>(row) = (uint16_t)(((b0 >> gb) & ((1u << G) - 1u)) | (((b1 >> gb) & ((1u << G) - 1u)) << 8));
                else if (G == 16) *reinterpret_cast<uint32_t *>(row) = (uint32_t)((b0 >> gb) & 0xFFFFu) | ((uint32_t)((b1 >> gb) & 0xFFFFu) << 16);
                else if (G == 32) *reinterpret_cast<uint2 *>(row) = make_uint2((uint32_t)(b0 >> gb), (uint32_t)(b1 >> gb));
                else *reinterpret_cast<uint4 *>(row) = make_uint4((uint32_t)b0, (uint32_t)(b0 >> 32), (uint32_t)b1, (uint32_t)(b1 >> 32));
            }
        }
    }
    // the end cell: smallest D, then smallest |k|, then the negative k
    const int64_t je = (int64_t)m + a.d0 + k;
    unsigned long long key = ~0ull;
    if (m && lane_ok && je >= 0 && je <= a.Ls && D < ALIGN_INF) key = ((unsigned long long)D << 8) | ((unsigned long long)(k < 0 ? -k : k) << 1) | (k > 0 ? 1ull : 0ull);
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
        const unsigned long long t = __shfl_xor(key, o, G);
        key = t < key ? t : key;
    }
    if (m && l == 0) fwd[r] = make_uint2((uint32_t)(key >> 8), (uint32_t)(key & 0xFFu)); // edits; |k| << 1 | (k > 0)
}

template __global__ void pgx_align_forward_kernel<0>(const uint32_t *, const uint64_t *, uint32_t, const uint32_t *, const uint64_t *, const uint32_t *, const int64_t *, uint64_t, uint64_t,
                                                     uint32_t, const uint64_t *, uint8_t *, uint2 *);
template __global__ void pgx_align_forward_kernel<1>(const uint32_t *, const uint64_t *, uint32_t, const uint32_t *, const uint64_t *, const uint32_t *, const int64_t *, uint64_t, uint64_t,
                                                     uint32_t, const uint64_t *, uint8_t *, uint2 *);
template __global__ void pgx_align_forward_kernel<2>(const uint32_t *, const uint64_t *, uint32_t, const uint32_t *, const uint64_t *, const uint32_t *, const int64_t *, uint64_t, uint64_t,
                                                     uint32_t, const uint64_t *, uint8_t *, uint2 *);
template __global__ void pgx_align_forward_kernel<3>(const uint32_t *, const uint64_t *, uint32_t, const uint32_t *, const uint64_t *, const uint32_t *, const int64_t *, uint64_t, uint64_t,
                                                     uint32_t, const uint64_t *, uint8_t *, uint2 *);
template __global__ void pgx_align_forward_kernel<4>(const uint32_t *, const uint64_t *, uint32_t, const uint32_t *, const uint64_t *, const uint32_t *, const int64_t *, uint64_t, uint64_t,
                                                     uint32_t, const uint64_t *, uint8_t *, uint2 *);
template __global__ void pgx_align_forward_kernel<5>(const uint32_t *, const uint64_t *, uint32_t, const uint32_t *, const uint64_t *, const uint32_t *, const int64_t *, uint64_t, uint64_t,
                                                     uint32_t, const uint64_t *, uint8_t *, uint2 *);
template __global__ void pgx_align_forward_kernel<6>(const uint32_t *, const uint64_t *, uint32_t, const uint32_t *, const uint64_t *, const uint32_t *, const int64_t *, uint64_t, uint64_t,
                                                     uint32_t, const uint64_t *, uint8_t *, uint2 *);

// write == 0: the record of every read of [r0, r1) and count[r] = its operations.  write == 1: the operations, behind op_off[r], last slot first.
__global__ void __launch_bounds__(256)
pgx_align_trace_kernel(const uint64_t *__restrict__ seq_start, uint32_t endmark, const uint64_t *__restrict__ read_off, const uint32_t *__restrict__ cand_seq,
                       const int64_t *__restrict__ cand_diag, uint64_t r0, uint64_t r1, uint32_t W, uint32_t row_bytes, const uint64_t *__restrict__ plane_off,
                       const uint8_t *__restrict__ planes, const uint2 *__restrict__ fwd, uint32_t write, pgx_read_align *__restrict__ out, uint64_t *__restrict__ count,
                       const uint64_t *__restrict__ op_off, uint32_t *__restrict__ ops) {
    const uint64_t r = r0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= r1) return;
    pgx_read_align v;
    v.diag = 0; v.text_start = v.text_end = 0; v.seq = cand_seq[r];
    v.clip_lo = v.clip_hi = v.edits = v.n_match = v.n_mismatch = v.n_ins = v.n_del = v.n_ops = v.band_hit = 0;
    // write: the slots of the read are filled from the last one down; `slot` is one behind the next to fill and never passes the read's first
    const uint64_t first = write ? op_off[r] : 0;
    uint64_t slot = write ? op_off[r + 1] : 0;
    auto put = [&](uint32_t length, uint32_t op) {
        if (write && slot > first) ops[--slot] = (length << 4) | op;
    };
    auto op_of = [](uint32_t code) { return code == 0 ? PGX_ALIGN_OP_EQ : (code == 1 ? PGX_ALIGN_OP_X : (code == 2 ? PGX_ALIGN_OP_I : PGX_ALIGN_OP_D)); };
    if (v.seq != PGX_NO_SEQUENCE) {
        v.diag = cand_diag[r];
        const AlignSpan a = align_span(seq_start, endmark, read_off, r, v.seq, v.diag);
        const uint32_t m = (uint32_t)(a.hi - a.lo);
        if (!m) { // no overlap: the whole read is one soft clip
            v.clip_hi = (uint32_t)a.len;
            v.n_ops = a.len > 0;
            if (a.len > 0) put((uint32_t)a.len, PGX_ALIGN_OP_S);
        } else {
            v.clip_lo = (uint32_t)a.lo; v.clip_hi = (uint32_t)(a.len - a.hi);
            const uint2 f = fwd[r];
            v.edits = f.x;
            int32_t k = (int32_t)(f.y >> 1);
            if (!(f.y & 1u)) k = -k;
            v.text_end = (uint64_t)((int64_t)m + a.d0 + k);
            const uint8_t *const rows = planes + (plane_off[r] - plane_off[r0]);
            const uint32_t half = row_bytes / 2;
            const int32_t w = (int32_t)W;
            bool hit = k == w || k == -w;
            uint32_t runs = 0, last = 4u, run_len = 0; // last: the code of the run being walked (4: none yet)
            if (v.clip_hi) put(v.clip_hi, PGX_ALIGN_OP_S);
            uint32_t i = m;
            while (i > 0) {
                const uint32_t l = (uint32_t)(k + w);
                if (l > 2 * W) break; // (planes of the forward kernel never lead out of the band)
                const uint8_t *const row = rows + (uint64_t)(i - 1) * row_bytes + (l >> 3);
                const uint32_t code = ((row[0] >> (l & 7u)) & 1u) | (((row[half] >> (l & 7u)) & 1u) << 1);
                if (code != last) {
                    if (run_len) put(run_len, op_of(last));
                    runs++; last = code; run_len = 0;
                }
                run_len++;
                if (code == 0) { v.n_match++; i--; }
                else if (code == 1) { v.n_mismatch++; i--; }
                else if (code == 2) { v.n_ins++; i--; k++; }
                else { v.n_del++; k--; }
                hit = hit || k == w || k == -w;
            }
            if (run_len) put(run_len, op_of(last));
            if (v.clip_lo) put(v.clip_lo, PGX_ALIGN_OP_S);
            v.text_start = (uint64_t)(a.d0 + k);
            v.band_hit = (W > 0 && hit) ? 1u : 0u;
            v.n_ops = runs + (v.clip_lo != 0) + (v.clip_hi != 0);
        }
    }
    if (!write) { out[r] = v; count[r] = v.n_ops; }
}
