// pgx_format_kernels.hip -- pgx_format_*: the find_mems CLI's text for a finished batch, written on the device (include/pgx.h "text output";
// pgx_batch_format, pgx_format_result) (gfx950).  The grammar is the one of format_range in src/find_mems.cpp; tests/text_emu.py restates it.
//
// The text is hierarchical -- a read holds its MEMs, a MEM its positions and (with locate) its values -- so every byte offset is a sum of
// lengths taken at three levels, each by one exclusive scan (scan_excl), and the text is then filled by item class.  No workgroup waits for another
// outside those scans.
//
//   pass 1 (lengths)
//     pgx_format_item_len_kernel   one lane per position / per located value: its decimal length and separator, one byte      -> scan -> pcum / vcum
//     pgx_format_mem_len_kernel    one lane per MEM: fixed strings + digits + its two list lengths (differences of pcum / vcum) -> scan -> mcum
//     pgx_format_read_len_kernel   one lane per read: header + its MEMs (a difference of mcum) + the closing newline           -> scan -> read_offsets
//                                  (and the length of the read's stderr line                                                   -> scan -> err_offsets)
//   pass 2 (fill), after the host has sized the text from read_offsets[n_reads]
//     pgx_format_fill_reads_kernel one lane per read: "Seq: <n>\n", the closing "\n", the stderr line
//     pgx_format_fill_mems_kernel  one lane per MEM: its lines and the newline behind each list; the owning read by a binary search in mem_offsets;
//                                  leaves pbase[m] / vbase[m], the text offset of the MEM's list minus the cumulative length of the items before it
//     pgx_format_fill_items_kernel one lane per position / value: the owning MEM by a binary search in pos_offsets / loc_offsets, then
//                                  text[base[m] + cum[q] ..) = "<number>, " (or "<seq>:<offset>, ")
//
// A number's length comes from pgx_dec_len (clz + a table of powers of ten) in both passes, and pgx_put_dec writes exactly that many bytes backwards from
// the end of its field: whatever the value, a lane writes inside the span pass 1 gave it.  Values below 2^32 are converted with 32-bit arithmetic (the
// division by ten is a multiplication), larger ones are first cut into pieces of nine digits by a division by the constant 10^9 (gfx950 has no 64-bit
// divide: this too is a multiply-high sequence).  Only "<v / max_length>:<v % max_length>" of the locate form divides by a run-time value.
// Stores are single bytes straight to global memory, neighbouring lanes writing neighbouring spans (the compact encoder measured an LDS stage with
// 8-byte stores against this and found no difference: DESIGN.md 6d).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

// 10^0 .. 10^19
static __constant__ uint64_t pgx_p10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull,
                                            10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull, 1000000000000000ull,
                                            10000000000000000ull, 100000000000000000ull, 1000000000000000000ull, 10000000000000000000ull};

// decimal digits of v: the bit length gives floor(log10) to within one, the table settles it
__device__ __forceinline__ uint32_t pgx_dec_len(uint64_t v) {
    const uint32_t bits = 64u - (uint32_t)__clzll((long long)(v | 1));
    const uint32_t t = (bits * 1233u) >> 12; // floor(bits * log10(2)): 0 .. 19
    return t + ((v | 1) >= pgx_p10[t] ? 1u : 0u); // (v | 1: zero has one digit; no power of ten above 1 is odd)
}
__device__ __forceinline__ uint64_t pgx_i64_abs(int64_t v) { return v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v; } // INT64_MIN -> 2^63
__device__ __forceinline__ uint32_t pgx_i64_len(int64_t v) { return pgx_dec_len(pgx_i64_abs(v)) + (v < 0 ? 1u : 0u); }

// the nd = pgx_dec_len(v) digits of v at p; returns p + nd
__device__ __forceinline__ char *pgx_put_dec(char *p, uint64_t v, uint32_t nd) {
    char *e = p + nd;
    while (v >> 32) { // nine digits a piece (v >= 2^32 > 10^9: all nine belong to the number)
        const uint64_t q = v / 1000000000ull;
        uint32_t r = (uint32_t)(v - q * 1000000000ull);
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const uint32_t t = r / 10u;
            *--e = (char)('0' + (r - t * 10u));
            r = t;
        }
        v = q;
    }
    uint32_t w = (uint32_t)v;
    while (e > p) {
        const uint32_t t = w / 10u;
        *--e = (char)('0' + (w - t * 10u));
        w = t;
    }
    return p + nd;
}
__device__ __forceinline__ char *pgx_put_u64(char *p, uint64_t v) { return pgx_put_dec(p, v, pgx_dec_len(v)); }
__device__ __forceinline__ char *pgx_put_i64(char *p, int64_t v) {
    if (v < 0) *p++ = '-';
    return pgx_put_u64(p, pgx_i64_abs(v));
}
template <uint32_t N>
__device__ __forceinline__ char *pgx_put_lit(char *p, const char (&s)[N]) {
#pragma unroll
    for (uint32_t i = 0; i + 1 < N; i++) p[i] = s[i];
    return p + (N - 1);
}
#define PGX_LIT_LEN(s) ((uint32_t)sizeof(s) - 1u)

// the fixed strings of the grammar (format_range, src/find_mems.cpp)
#define PGX_T_SEQ "Seq: "
#define PGX_T_START "MEM START: "
#define PGX_T_END ", MEM END: "
#define PGX_T_BWT " BWT START: "
#define PGX_T_SIZE " SIZE: "
#define PGX_T_NPOS "Number of unique positions: "
#define PGX_T_OCC "Occurrences: "
#define PGX_T_NOTLOC " (not located)\n"
#define PGX_T_SEQS "Sequences: "
#define PGX_T_ERR "[find_all_mems] total mems="

// the largest m in [0, n) with off[m] <= q (off ascending, off[0] <= q < off[n]): the owner of item q, entries without items skipped
__device__ __forceinline__ uint64_t pgx_format_owner(const uint64_t *__restrict__ off, uint64_t n, uint64_t q) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= q) lo = mid;
        else hi = mid;
    }
    return lo;
}

// len[i]: bytes of item i in its list.  max_length == 0: "<v>, "; else "<v / max_length>:<v % max_length>, "
__global__ void __launch_bounds__(256)
pgx_format_item_len_kernel(const uint64_t *__restrict__ vals, uint64_t n, uint64_t max_length, uint8_t *__restrict__ len) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t v = vals[i];
    uint32_t l;
    if (max_length == 0) l = pgx_dec_len(v) + 2u;
    else {
        const uint64_t s = v / max_length;
        l = pgx_dec_len(s) + 1u + pgx_dec_len(v - s * max_length) + 2u;
    }
    len[i] = (uint8_t)l;
}

// bytes of the locate line of MEM m in front of its value list; nv = its number of values (0: not located, no list)
__device__ __forceinline__ uint32_t pgx_format_loc_head(const PgxFormatArgs &a, uint64_t m, int64_t size, uint64_t &nv) {
    nv = a.loc_off[m + 1] - a.loc_off[m];
    if (nv == 0) return PGX_LIT_LEN(PGX_T_OCC) + pgx_i64_len(size) + PGX_LIT_LEN(PGX_T_NOTLOC);
    if (a.flags & PGX_FORMAT_LOCATE_POSITIONS) return PGX_LIT_LEN(PGX_T_OCC) + pgx_i64_len(size) + 1u;
    return PGX_LIT_LEN(PGX_T_SEQS) + pgx_dec_len(nv) + 1u;
}

__global__ void __launch_bounds__(256)
pgx_format_mem_len_kernel(PgxFormatArgs a, const uint64_t *__restrict__ pcum, const uint64_t *__restrict__ vcum, uint64_t *__restrict__ mlen) {
    const uint64_t m = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= a.n_mems) return;
    const ulonglong2 *q = reinterpret_cast<const ulonglong2 *>(a.mems + m);
    const ulonglong2 x = q[0], y = q[1];
    const uint64_t p0 = a.pos_off[m], p1 = a.pos_off[m + 1];
    uint64_t l = PGX_LIT_LEN(PGX_T_START) + pgx_dec_len(x.x) + PGX_LIT_LEN(PGX_T_END) + pgx_dec_len(x.y) + PGX_LIT_LEN(PGX_T_BWT) + pgx_dec_len(y.x) +
                 PGX_LIT_LEN(PGX_T_SIZE) + pgx_i64_len((int64_t)y.y) + 1u;
    l += PGX_LIT_LEN(PGX_T_NPOS) + pgx_dec_len(p1 - p0) + 1u + (pcum[p1] - pcum[p0]) + 1u;
    if (a.flags & (PGX_FORMAT_LOCATE_POSITIONS | PGX_FORMAT_LOCATE_SEQS)) {
        uint64_t nv;
        l += pgx_format_loc_head(a, m, (int64_t)y.y, nv);
        l += vcum[a.loc_off[m + 1]] - vcum[a.loc_off[m]] + 1u;
    }
    mlen[m] = l;
}

__global__ void __launch_bounds__(256)
pgx_format_read_len_kernel(PgxFormatArgs a, const uint64_t *__restrict__ mcum, uint64_t *__restrict__ rlen, uint8_t *__restrict__ elen) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_reads) return;
    const uint64_t m0 = a.mem_off[i], m1 = a.mem_off[i + 1];
    rlen[i] = PGX_LIT_LEN(PGX_T_SEQ) + pgx_dec_len(a.first_seq + i + 1) + 1u + (mcum[m1] - mcum[m0]) + 1u;
    if (elen) elen[i] = (uint8_t)(PGX_LIT_LEN(PGX_T_ERR) + pgx_dec_len(m1 - m0) + 1u);
}

__global__ void __launch_bounds__(256)
pgx_format_fill_reads_kernel(PgxFormatArgs a, const uint64_t *__restrict__ read_off, const uint64_t *__restrict__ err_off, char *__restrict__ text,
                             char *__restrict__ err_text) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_reads) return;
    char *p = pgx_put_lit(text + read_off[i], PGX_T_SEQ);
    p = pgx_put_u64(p, a.first_seq + i + 1);
    *p = '\n';
    text[read_off[i + 1] - 1] = '\n';
    if (err_text) {
        char *e = pgx_put_lit(err_text + err_off[i], PGX_T_ERR);
        e = pgx_put_u64(e, a.mem_off[i + 1] - a.mem_off[i]);
        *e = '\n';
    }
}

__global__ void __launch_bounds__(256)
pgx_format_fill_mems_kernel(PgxFormatArgs a, const uint64_t *__restrict__ read_off, const uint64_t *__restrict__ mcum, const uint64_t *__restrict__ pcum,
                            const uint64_t *__restrict__ vcum, char *__restrict__ text, uint64_t *__restrict__ pbase, uint64_t *__restrict__ vbase) {
    const uint64_t m = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= a.n_mems) return;
    const uint64_t r = pgx_format_owner(a.mem_off, a.n_reads, m);
    uint64_t at = read_off[r] + PGX_LIT_LEN(PGX_T_SEQ) + pgx_dec_len(a.first_seq + r + 1) + 1u + (mcum[m] - mcum[a.mem_off[r]]);
    const ulonglong2 *q = reinterpret_cast<const ulonglong2 *>(a.mems + m);
    const ulonglong2 x = q[0], y = q[1];
    const uint64_t p0 = a.pos_off[m], p1 = a.pos_off[m + 1];
    char *p = text + at;
    p = pgx_put_lit(p, PGX_T_START); p = pgx_put_u64(p, x.x);
    p = pgx_put_lit(p, PGX_T_END); p = pgx_put_u64(p, x.y);
    p = pgx_put_lit(p, PGX_T_BWT); p = pgx_put_u64(p, y.x);
    p = pgx_put_lit(p, PGX_T_SIZE); p = pgx_put_i64(p, (int64_t)y.y);
    *p++ = '\n';
    p = pgx_put_lit(p, PGX_T_NPOS); p = pgx_put_u64(p, p1 - p0);
    *p++ = '\n';
    at = (uint64_t)(p - text);
    pbase[m] = at - pcum[p0];
    at += pcum[p1] - pcum[p0];
    text[at++] = '\n';
    if (a.flags & (PGX_FORMAT_LOCATE_POSITIONS | PGX_FORMAT_LOCATE_SEQS)) {
        const uint64_t v0 = a.loc_off[m], v1 = a.loc_off[m + 1], nv = v1 - v0;
        p = text + at;
        if (nv == 0) { p = pgx_put_lit(p, PGX_T_OCC); p = pgx_put_i64(p, (int64_t)y.y); p = pgx_put_lit(p, PGX_T_NOTLOC); }
        else if (a.flags & PGX_FORMAT_LOCATE_POSITIONS) { p = pgx_put_lit(p, PGX_T_OCC); p = pgx_put_i64(p, (int64_t)y.y); *p++ = '\n'; }
        else { p = pgx_put_lit(p, PGX_T_SEQS); p = pgx_put_u64(p, nv); *p++ = '\n'; }
        at = (uint64_t)(p - text);
        vbase[m] = at - vcum[v0];
        at += vcum[v1] - vcum[v0];
        text[at] = '\n';
    }
}

// item q of a list level (positions under pos_off, or located values under loc_off): text[base[owner] + cum[q] ..)
__global__ void __launch_bounds__(256)
pgx_format_fill_items_kernel(const uint64_t *__restrict__ vals, uint64_t n, const uint64_t *__restrict__ off, uint64_t n_mems, const uint64_t *__restrict__ cum,
                             const uint64_t *__restrict__ base, uint64_t max_length, char *__restrict__ text) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t m = pgx_format_owner(off, n_mems, i);
    char *p = text + base[m] + cum[i];
    const uint64_t v = vals[i];
    if (max_length == 0) p = pgx_put_u64(p, v);
    else {
        const uint64_t s = v / max_length;
        p = pgx_put_u64(p, s);
        *p++ = ':';
        p = pgx_put_u64(p, v - s * max_length);
    }
    p[0] = ',';
    p[1] = ' ';
}
