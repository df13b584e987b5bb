// pgx_walk_kernels.hip -- the WALK image (pgx_image.h) and the read walk stage (include/pgx.h "read walk") as gfx950 kernels.
//
// The image's kernels (pgx_images.hip ensure_walk; pgx_read_walk_arrays sets its bits from stated tables):
//   mark       a thread a BWT row i >= n_seq: its text position (the resident 32-bit suffix array, or seq * max_length + off as the locate kernels
//              write it), the tag of the TRUE run that holds the row -- run pgx_tag_rank(x) - 1, without the reference's f % 10 slip -- and, where
//              the tag's offset is 0, an atomicOr of the position's bit.  Consecutive rows fall into the same or neighbouring runs.
//   set        the same atomicOr from a list of marked positions (the arrays route)
//   popc       a thread a directory block: set bits of its PGX_WALK_BLOCK_WORDS words; the project's scan turns the counts into the directory
//   nodes      the second row pass: walk_nodes[rank(p)] = tag >> 10 for every row whose tag has offset 0
//   check      a thread a sequence: the first position of a non-empty sequence is marked, else atomicMin of the sequence
//   positions  a thread a word: the text position of every visit (pgx_index_paths)
// The stage's kernels:
//   count      a lane a read: two rank lookups (k0 = marks <= start, k1 = marks < end) and two bit scans (back to the mark of visit k0, on to the
//              end of visit k1), the 32-byte record, the step count and k0.  A node has at most 1024 symbols (the tag's offset has ten bits), so
//              each scan reads at most PGX_WALK_MAX_VISIT bits = 17 words.
//   fill       PGX_WALK_FILL_LANES lanes a read copy walk_nodes[k0 .. k1] behind the read's offset: a read's steps are contiguous in the image
// No LDS, no inline assembly; every index is 64-bit.  Words are only read below the image's n_words (positions <= n).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"
#include "pgx_walk_device.h"

namespace {

// the first marked position in [e, cap], cap = min(limit, e + 1023); cap itself where there is none: the end of the visit that holds e - 1
__device__ __forceinline__ uint64_t walk_next_mark(const PgxWalkImage &w, uint64_t e, uint64_t limit) {
    const uint64_t cap = (limit - e > PGX_WALK_MAX_VISIT - 1) ? e + (PGX_WALK_MAX_VISIT - 1) : limit;
    if (e >= cap) return cap;
    uint64_t wi = e >> 6;
    uint64_t word = w.bits[wi] & (~0ull << ((uint32_t)e & 63u));
    for (;;) { // at most 17 words
        if (word) {
            const uint64_t p = (wi << 6) + (uint64_t)__builtin_ctzll(word);
            return p < cap ? p : cap;
        }
        if (((wi + 1) << 6) > cap) return cap;
        word = w.bits[++wi];
    }
}

// row i >= n_seq -> its text position p (false: a suffix array value outside the collection) and the tag of the run that holds it
__device__ __forceinline__ bool walk_row(const PgxDevImage &img, const uint32_t *sa32, const uint64_t *sa64, uint64_t max_length, const uint64_t *seq_start,
                                         uint64_t n_seq, uint64_t n, int64_t delta, uint64_t i, uint64_t &p, uint64_t &tag) {
    if (sa32) p = sa32[i];
    else {
        const uint64_t v = sa64[i], q = v / max_length;
        p = q < n_seq ? seq_start[q] + v % max_length : n;
    }
    if (p >= n) return false;
    const uint64_t f = pgx_tag_rank(img, (uint64_t)((int64_t)i + delta)); // run starts <= x: the row lies in run f - 1
    tag = 0;
    if (f >= 1 && f - 1 < img.n_tag_items) tag = img.tpair ? img.tpair[f - 1].y : img.tvals[f - 1];
    return true;
}

} // namespace

__global__ void __launch_bounds__(256)
pgx_walk_mark_kernel(PgxDevImage img, const uint32_t *__restrict__ sa32, const uint64_t *__restrict__ sa64, uint64_t max_length, const uint64_t *__restrict__ seq_start,
                     uint64_t n_seq, uint64_t n, int64_t delta, uint32_t *__restrict__ bits32, unsigned long long *__restrict__ bad) {
    for (uint64_t i = n_seq + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t p, tag;
        if (!walk_row(img, sa32, sa64, max_length, seq_start, n_seq, n, delta, i, p, tag)) { atomicAdd(bad, 1ull); continue; }
        if ((tag & 0x3FFull) == 0) atomicOr(bits32 + (p >> 5), 1u << ((uint32_t)p & 31u));
    }
}

__global__ void __launch_bounds__(256)
pgx_walk_set_kernel(const uint64_t *__restrict__ marks, uint64_t n_marks, uint32_t *__restrict__ bits32) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_marks; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = marks[k];
        atomicOr(bits32 + (p >> 5), 1u << ((uint32_t)p & 31u));
    }
}

__global__ void __launch_bounds__(256)
pgx_walk_popc_kernel(const uint64_t *__restrict__ bits, uint64_t n_blocks, uint64_t *__restrict__ counts) {
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t c = 0;
#pragma unroll
        for (uint32_t j = 0; j < PGX_WALK_BLOCK_WORDS; j++) c += (uint64_t)__popcll(bits[b * PGX_WALK_BLOCK_WORDS + j]);
        counts[b] = c;
    }
}

__global__ void __launch_bounds__(256)
pgx_walk_nodes_kernel(PgxDevImage img, PgxWalkImage w, const uint32_t *__restrict__ sa32, const uint64_t *__restrict__ sa64, uint64_t max_length,
                      const uint64_t *__restrict__ seq_start, uint64_t n_seq, uint64_t n, int64_t delta, uint64_t *__restrict__ nodes) {
    for (uint64_t i = n_seq + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t p, tag;
        if (!walk_row(img, sa32, sa64, max_length, seq_start, n_seq, n, delta, i, p, tag)) continue;
        if ((tag & 0x3FFull) == 0) nodes[walk_rank(w, p)] = tag >> 10;
    }
}

__global__ void __launch_bounds__(256)
pgx_walk_check_kernel(PgxWalkImage w, const uint64_t *__restrict__ seq_start, uint64_t n_seq, uint32_t endmark, unsigned long long *__restrict__ bad) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_seq) return;
    const uint64_t a = seq_start[q], e = seq_start[q + 1] - endmark;
    if (e > a && !((w.bits[a >> 6] >> (a & 63u)) & 1ull)) atomicMin(bad, (unsigned long long)q);
}

__global__ void __launch_bounds__(256)
pgx_walk_positions_kernel(PgxWalkImage w, uint64_t *__restrict__ pos) {
    for (uint64_t wi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; wi < w.n_words; wi += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t word = w.bits[wi];
        if (!word) continue;
        uint64_t k = walk_rank(w, wi << 6);
        while (word) {
            pos[k++] = (wi << 6) + (uint64_t)__builtin_ctzll(word);
            word &= word - 1;
        }
    }
}

__global__ void __launch_bounds__(256)
pgx_walk_count_kernel(PgxWalkImage w, const uint64_t *__restrict__ seq_start, uint32_t endmark, uint64_t n_seq, const pgx_read_align *__restrict__ recs,
                      const uint32_t *__restrict__ seq, const uint64_t *__restrict__ text_start, const uint64_t *__restrict__ text_end, uint64_t n_reads,
                      pgx_read_walk *__restrict__ out, uint64_t *__restrict__ n_steps, uint64_t *__restrict__ first) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    uint32_t q;
    uint64_t a, b;
    if (recs) { q = recs[r].seq; a = recs[r].text_start; b = recs[r].text_end; }
    else { q = seq[r]; a = text_start[r]; b = text_end[r]; }
    pgx_read_walk o;
    o.path_len = o.path_start = o.path_end = 0;
    o.n_steps = 0; o.seq = q;
    uint64_t k0 = 0;
    if (q != PGX_NO_SEQUENCE && (uint64_t)q < n_seq && b > a) {
        const uint64_t base = seq_start[q], limit = seq_start[(uint64_t)q + 1] - endmark;
        const uint64_t s = base + a, e = base + b;
        if (e <= limit) { // (what the align stage and the arrays route's checks guarantee)
            const uint64_t r0 = walk_rank(w, s + 1), r1 = walk_rank(w, e);
            if (r0 >= 1) {
                const uint64_t m0 = walk_prev_mark(w, s, base), end = walk_next_mark(w, e, limit);
                k0 = r0 - 1;
                o.n_steps = (uint32_t)(r1 - r0 + 1);
                o.path_start = s - m0;
                o.path_end = o.path_start + (b - a);
                o.path_len = end - m0;
            }
        }
    }
    out[r] = o;
    n_steps[r] = o.n_steps;
    first[r] = k0;
}

__global__ void __launch_bounds__(256)
pgx_walk_fill_kernel(PgxWalkImage w, const uint64_t *__restrict__ n_steps, const uint64_t *__restrict__ first, const uint64_t *__restrict__ step_off, uint64_t n_reads,
                     uint64_t *__restrict__ steps) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, r = t / PGX_WALK_FILL_LANES;
    if (r >= n_reads) return;
    const uint64_t cnt = n_steps[r], k0 = first[r], o = step_off[r];
    for (uint64_t j = t % PGX_WALK_FILL_LANES; j < cnt; j += PGX_WALK_FILL_LANES) steps[o + j] = w.nodes[k0 + j];
}
