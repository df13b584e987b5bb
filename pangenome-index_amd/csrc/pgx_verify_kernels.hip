// pgx_verify_kernels.hip -- the text image (pgx_image.h "TEXT image") and read verify (include/pgx.h "read verify"): a read laid on the
// indexed text at a candidate (sequence, diagonal), every position compared, one pgx_read_verify a candidate and one a read.
//
//   mark     a thread a sequence: the endmarker positions of the scattered text bytes get a code of their own (the LCE scatter kernel
//            writes N and endmarkers alike)
//   scatter32  the same scatter as pgx_lce_scatter_kernel from the 32-bit suffix array of a resident LCE image (no second whole-range locate)
//   pack     a thread a word: eight text bytes (scatter codes, or ASCII in the arrays form) -> eight 4-bit codes \n A C G N T = 0 .. 5
//   unpack   a thread a word: the image back into the bytes of the collection
//   code     a thread a word of the concatenated reads: eight read bytes -> eight 4-bit codes, A C G T as in the text, every other byte 15
//            (equal to no text code, so that N opposite N is a mismatch).  Once per read, whatever the number of its candidates.
//   choose   a thread a read: its candidates from the place records (max_cand == 1) or the place list; count, then fill behind a scan
//   owner    a thread a read: the read of every candidate
//   verify   a lane a candidate, walking the coded words of its read: the text window of a word starts at an arbitrary symbol, so it is a
//            funnel shift of two neighbouring text words; one XOR and a nibble-nonzero mask compare eight positions, and the walk over
//            them jumps from mismatch to mismatch (a word without one is a single step)
//   reduce   a thread a read: the winner among its candidates
//   check    pgx_read_verify_arrays: the first read with a candidate whose sequence is >= n_seq
// Every index is 64-bit.  Text words are only loaded for a word that holds a position of the span: the word index is >= -1 (guarded) and at
// most one beyond the last word of the text (PGX_TEXT_PAD_WORDS behind it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

namespace {

// scatter codes (pgx_lce_scatter_kernel: A C T G = 0 1 2 3, 0xFF = N or endmarker; PGX_TEXT_SCATTER_END = endmarker) -> text codes
__device__ __forceinline__ uint32_t text_code_of_scatter(uint32_t c) {
    return c == 0u ? PGX_TEXT_A : (c == 1u ? PGX_TEXT_C : (c == 2u ? PGX_TEXT_T : (c == 3u ? PGX_TEXT_G : (c == PGX_TEXT_SCATTER_END ? PGX_TEXT_END : PGX_TEXT_N))));
}
// bytes of a collection; anything outside \n A C G N T was refused before
__device__ __forceinline__ uint32_t text_code_of_byte(uint32_t c) {
    return c == 'A' ? PGX_TEXT_A : (c == 'C' ? PGX_TEXT_C : (c == 'G' ? PGX_TEXT_G : (c == 'T' ? PGX_TEXT_T : (c == 'N' ? PGX_TEXT_N : PGX_TEXT_END))));
}
// read bytes: upper-case A C G T match their text codes, every other byte matches nothing
__device__ __forceinline__ uint32_t read_code_of_byte(uint32_t c) {
    return c == 'A' ? PGX_TEXT_A : (c == 'C' ? PGX_TEXT_C : (c == 'G' ? PGX_TEXT_G : (c == 'T' ? PGX_TEXT_T : 15u)));
}

} // namespace

__global__ void __launch_bounds__(256)
pgx_text_mark_kernel(const uint64_t *__restrict__ seq_start, uint64_t n_seq, uint64_t n, uint8_t *__restrict__ text8) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_seq) return;
    const uint64_t e = seq_start[q + 1];
    if (e >= 1 && e <= n) text8[e - 1] = (uint8_t)PGX_TEXT_SCATTER_END;
}

__global__ void __launch_bounds__(256)
pgx_text_scatter32_kernel(const uint32_t *__restrict__ sa32, uint64_t n, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t c4, uint64_t c5, uint8_t *__restrict__ text8) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g = sa32[i];
        if (g >= n) continue; // (a built LCE image holds none)
        text8[g] = i < c1 ? 0xFFu : (i < c2 ? 0u : (i < c3 ? 1u : (i < c4 ? 3u : (i < c5 ? 0xFFu : 2u)))); // as pgx_lce_scatter_kernel
    }
}

__global__ void __launch_bounds__(256)
pgx_text_pack_kernel(const uint8_t *__restrict__ text8, uint64_t n, uint64_t n_words, uint32_t ascii, uint32_t *__restrict__ text4) {
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint64_t g = 8 * w + k;
            if (g < n) {
                const uint32_t c = text8[g];
                v |= (ascii ? text_code_of_byte(c) : text_code_of_scatter(c)) << (4u * k);
            } // (behind the text: PGX_TEXT_END)
        }
        text4[w] = v;
    }
}

__global__ void __launch_bounds__(256)
pgx_text_unpack_kernel(const uint32_t *__restrict__ text4, uint64_t n, uint8_t *__restrict__ bytes) {
    const uint64_t n_words = (n + 7) / 8;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t v = text4[w];
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint64_t g = 8 * w + k;
            const uint32_t c = (v >> (4u * k)) & 15u;
            if (g < n) bytes[g] = c == PGX_TEXT_A ? 'A' : (c == PGX_TEXT_C ? 'C' : (c == PGX_TEXT_G ? 'G' : (c == PGX_TEXT_T ? 'T' : (c == PGX_TEXT_N ? 'N' : '\n'))));
        }
    }
}

__global__ void __launch_bounds__(256)
pgx_verify_code_kernel(const uint8_t *__restrict__ reads, uint64_t n_bytes, uint64_t n_words, uint32_t *__restrict__ rcode) {
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint64_t g = 8 * w + k;
            v |= (g < n_bytes ? read_code_of_byte(reads[g]) : 15u) << (4u * k);
        }
        rcode[w] = v;
    }
}

// The candidates of read r: its placements with score == best_score > 0 in placement order, the first max_cand of them.  cand_seq == nullptr:
// count[r] only; else the candidates behind cand_off[r].  place_off == nullptr (max_cand == 1): the place record names the only candidate.
__global__ void __launch_bounds__(256)
pgx_verify_choose_kernel(const pgx_read_place *__restrict__ recs, const uint64_t *__restrict__ place_off, const pgx_placement *__restrict__ places, uint64_t n_reads,
                         uint32_t max_cand, uint64_t *__restrict__ count, const uint64_t *__restrict__ cand_off, uint32_t *__restrict__ cand_seq,
                         int64_t *__restrict__ cand_diag) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint64_t best = recs[r].best_score;
    uint64_t k = 0;
    if (best > 0) {
        if (!place_off) {
            if (cand_seq) { cand_seq[cand_off[r]] = recs[r].best_seq; cand_diag[cand_off[r]] = recs[r].best_diag; }
            k = 1;
        } else {
            for (uint64_t p = place_off[r]; p < place_off[r + 1] && k < max_cand; p++)
                if (places[p].score == best) {
                    if (cand_seq) { cand_seq[cand_off[r] + k] = places[p].seq; cand_diag[cand_off[r] + k] = places[p].diag; }
                    k++;
                }
        }
    }
    if (!cand_seq) count[r] = k;
}

__global__ void __launch_bounds__(256)
pgx_verify_owner_kernel(const uint64_t *__restrict__ cand_off, uint64_t n_reads, uint64_t n_cands, uint64_t *__restrict__ cand_read) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint64_t e = cand_off[r + 1] < n_cands ? cand_off[r + 1] : n_cands;
    for (uint64_t c = cand_off[r]; c < e; c++) cand_read[c] = r;
}

__global__ void __launch_bounds__(256)
pgx_verify_check_kernel(const uint64_t *__restrict__ cand_read, const uint32_t *__restrict__ cand_seq, uint64_t n_cands, uint64_t n_seq, unsigned long long *__restrict__ bad) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cands) return;
    if (cand_seq[c] >= n_seq) atomicMin(bad, (unsigned long long)cand_read[c]);
}

// seq_start: n_seq + 1 text positions; endmark = 1: every sequence is followed by its endmarker (the image), 0: it is not (the arrays form)
__global__ void __launch_bounds__(PGX_VERIFY_THREADS)
pgx_verify_kernel(const uint32_t *__restrict__ text4, const uint64_t *__restrict__ seq_start, uint32_t endmark, const uint32_t *__restrict__ rcode,
                  const uint64_t *__restrict__ read_off, const uint64_t *__restrict__ cand_off, const uint64_t *__restrict__ cand_read,
                  const uint32_t *__restrict__ cand_seq, const int64_t *__restrict__ cand_diag, uint64_t n_cands, uint32_t penalty, pgx_read_verify *__restrict__ out) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cands) return;
    const uint64_t r = cand_read[c];
    const uint32_t seq = cand_seq[c];
    const int64_t diag = cand_diag[c];
    const uint64_t roff = read_off[r];
    const int64_t len = (int64_t)(read_off[r + 1] - roff);
    const uint64_t s0 = seq_start[seq];
    const int64_t Ls = (int64_t)(seq_start[seq + 1] - s0) - (int64_t)endmark;
    int64_t lo = diag < 0 ? -diag : 0;
    int64_t hi = Ls - diag < len ? Ls - diag : len; // (|diag| stays far below 2^62: sequence offsets and read positions)
    if (hi <= lo) lo = hi = 0;
    // state of the walk over read positions [lo, hi): E = the best score of a segment that ends here (smallest start on ties), < 0 before the first position
    const int32_t P = (int32_t)penalty;
    int32_t E = -1, best = 0;
    uint32_t e_start = 0, e_mm = 0, seg_start = (uint32_t)lo, seg_end = (uint32_t)lo, seg_mm = 0;
    uint32_t mismatches = 0, run = 0, longest = 0, run_start = 0;
    if (hi > lo) {
        const uint64_t g0 = roff + (uint64_t)lo, g1 = roff + (uint64_t)hi; // the span as bytes of the concatenated reads
        const int64_t delta = (int64_t)s0 + diag - (int64_t)roff;           // read byte g lies on text symbol g + delta
        for (uint64_t w = g0 >> 3; w <= (g1 - 1) >> 3; w++) {
            const int64_t t0 = (int64_t)(8 * w) + delta, tw = t0 >> 3; // (arithmetic shift: floor)
            const uint32_t sh = 4u * (uint32_t)(t0 & 7);
            const uint32_t ta = tw >= 0 ? text4[tw] : 0u, tb = text4[tw + 1];
            const uint32_t tword = (uint32_t)((((uint64_t)tb << 32) | ta) >> sh);
            uint32_t x = rcode[w] ^ tword;
            x = (x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x11111111u; // bit 4 k: position k of the word is a mismatch
            const uint32_t k0 = 8 * w < g0 ? (uint32_t)(g0 - 8 * w) : 0u, k1 = g1 - 8 * w < 8 ? (uint32_t)(g1 - 8 * w) : 8u;
            uint32_t k = k0;
            while (k < k1) {
                const uint32_t rest = x >> (4u * k);
                uint32_t nm = rest ? (uint32_t)__builtin_ctz(rest) >> 2 : 8u;
                nm = nm < k1 - k ? nm : k1 - k;
                const uint32_t i = (uint32_t)(8 * w + k - roff); // read position
                if (nm) { // nm matches from i on
                    if (E < 0) { E = 0; e_start = i; e_mm = 0; }
                    E += (int32_t)nm;
                    if (E > best) { best = E; seg_start = e_start; seg_end = i + nm; seg_mm = e_mm; }
                    run += nm;
                    if (run > longest) { longest = run; run_start = i + nm - run; }
                    k += nm;
                } else { // a mismatch at i (a segment that ends on it never beats what was seen before)
                    if (E < 0) { E = 0; e_start = i; e_mm = 0; }
                    E -= P; e_mm++;
                    mismatches++; run = 0;
                    k++;
                }
            }
        }
    }
    pgx_read_verify v;
    v.diag = diag; v.seq = seq; v.n_cand = (uint32_t)(c - cand_off[r]);
    v.span_lo = (uint32_t)lo; v.span_hi = (uint32_t)hi;
    v.matches = (uint32_t)(hi - lo) - mismatches; v.mismatches = mismatches;
    v.seg_start = seg_start; v.seg_end = seg_end; v.seg_score = (uint32_t)best; v.seg_mismatches = seg_mm;
    v.longest_run = longest; v.run_start = run_start;
    v.cand_index = v.n_cand; v.n_tied = 0;
    out[c] = v;
}

// the winner of a read: largest seg_score, then most matches, then the first
__global__ void __launch_bounds__(256)
pgx_verify_reduce_kernel(const pgx_read_verify *__restrict__ cands, const uint64_t *__restrict__ cand_off, uint64_t n_reads, pgx_read_verify *__restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint64_t c0 = cand_off[r], c1 = cand_off[r + 1];
    pgx_read_verify v;
    if (c1 <= c0) {
        v.diag = 0; v.seq = PGX_NO_SEQUENCE; v.n_cand = 0; v.span_lo = v.span_hi = v.matches = v.mismatches = 0;
        v.seg_start = v.seg_end = v.seg_score = v.seg_mismatches = v.longest_run = v.run_start = v.cand_index = v.n_tied = 0;
    } else {
        uint64_t win = c0;
        uint32_t ws = cands[c0].seg_score, wm = cands[c0].matches, tied = 1;
        for (uint64_t c = c0 + 1; c < c1; c++) {
            const uint32_t s = cands[c].seg_score, m = cands[c].matches;
            if (s > ws || (s == ws && m > wm)) { win = c; ws = s; wm = m; tied = 1; }
            else if (s == ws && m == wm) tied++;
        }
        v = cands[win];
        v.n_cand = (uint32_t)(c1 - c0); v.cand_index = (uint32_t)(win - c0); v.n_tied = tied;
    }
    out[r] = v;
}
