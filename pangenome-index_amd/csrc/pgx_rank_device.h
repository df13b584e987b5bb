// pgx_rank_device.h -- the __device__ primitives the gfx950 (CDNA4) kernels share: block lookup, the dense / dense2 / wide dense2 loads
// and ranks, the rank probe and the FMD extension built on them (backward/forward_extend_encoded, src/r-index.cpp:713-764 +
// rank_at_cached_encoded, :619-641), the staging of the tables in LDS and the index of a k-mer seed window.
// Included by the kernel files only (pgx_fm_kernels.hip, pgx_pairs_kernels.hip, pgx_reads_kernels.hip, pgx_query_kernels.hip).
//
// All of it is 64-bit integer work bound by random access into the rank image (HBM / L2 / LDS);
// there is no floating point and nothing MFMA-shaped.  Wave width is hard-coded to 64.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

// block holding position pos (pos <= n).  One 8-byte directory entry resolves buckets with at most
// two block starts; denser buckets search the 16-bit low parts of their blocks.
template <bool LDS_IMAGE>
__device__ __forceinline__ uint32_t pgx_find_block(const PgxDevImage &img, const uint64_t *__restrict__ lds_dir,
                                                   const uint16_t *__restrict__ lds_blow, uint64_t pos) {
    const uint64_t di = pos >> img.dir_shift; // <= (n >> shift) = dir_entries - 2
    const uint64_t e = LDS_IMAGE ? lds_dir[di] : img.dir[di];
    const uint32_t lowp = (uint32_t)pos & ((1u << img.dir_shift) - 1u);
    uint32_t lo = (uint32_t)e;
    const uint32_t cnt = (uint32_t)(e >> 32) & 0xFFu;
    if (cnt <= 2) {
        const uint32_t l0 = (uint32_t)(e >> 40) & 0xFFFu, l1 = (uint32_t)(e >> 52);
        return lo - 1u + ((cnt >= 1 && l0 <= lowp) ? 1u : 0u) + ((cnt >= 2 && l1 <= lowp) ? 1u : 0u);
    }
    uint32_t hi = cnt < 255 ? lo + cnt : (uint32_t)(LDS_IMAGE ? lds_dir[di + 1] : img.dir[di + 1]);
    while (lo < hi) { // upper bound over the blocks that start inside this bucket
        const uint32_t mid = (lo + hi) >> 1;
        const uint32_t v = LDS_IMAGE ? lds_blow[mid] : img.blow[mid];
        if (v <= lowp) lo = mid + 1; else hi = mid;
    }
    return lo - 1; // block 0 starts at 0, so lo >= 1
}

// ------------------------------------------------------------------------------------------
// DENSE image (pgx_image.h): block = pos >> 6, three 64-bit planes of code bits under the same count header.
// A dense block in registers: header dwords 0..7 and plane dwords 8..13.
struct PgxDenseBlk {
    uint4 h0, h1, p01; // p01 = plane0.lo, plane0.hi, plane1.lo, plane1.hi
    uint2 p2;
};

template <bool LDS_IMAGE>
__device__ __forceinline__ PgxDenseBlk pgx_dense_load(const PgxDevImage &img, const uint4 *__restrict__ lds_blocks, uint64_t pos) {
    // in LDS the blocks are 80 bytes apart (PGX_DENSE_LDS_U4): with 64 they would start in only two bank groups
    const uint4 *bp = LDS_IMAGE ? lds_blocks + (size_t)(pos >> 6) * PGX_DENSE_LDS_U4 : img.blocks + (size_t)(pos >> 6) * 4;
    PgxDenseBlk b;
    b.h0 = bp[0]; b.h1 = bp[1]; b.p01 = bp[2];
    b.p2 = *reinterpret_cast<const uint2 *>(bp + 3);
    return b;
}

// rank sums at pos from its (loaded) block: A = count of code cv, B = sum over codes of mult[code] * count(code)
__device__ __forceinline__ void pgx_dense_rank(const PgxDenseBlk &blk, uint64_t pos, uint32_t cv, uint32_t mrow, uint64_t &A, uint64_t &B) {
    const uint4 h0 = blk.h0, h1 = blk.h1;
    uint64_t c[6];
    c[0] = (uint64_t)h0.x | ((uint64_t)(h1.z & 0xFFu) << 32);
    c[1] = (uint64_t)h0.y | ((uint64_t)((h1.z >> 8) & 0xFFu) << 32);
    c[2] = (uint64_t)h0.z | ((uint64_t)((h1.z >> 16) & 0xFFu) << 32);
    c[3] = (uint64_t)h0.w | ((uint64_t)(h1.z >> 24) << 32);
    c[4] = (uint64_t)h1.x | ((uint64_t)(h1.w & 0xFFu) << 32);
    c[5] = (uint64_t)h1.y | ((uint64_t)((h1.w >> 8) & 0xFFu) << 32);
    const uint32_t rel = (uint32_t)pos & 63u;
    // prefix mask of rel bits, as two dwords
    const uint32_t mlo = rel >= 32u ? 0xFFFFFFFFu : ((1u << rel) - 1u);
    const uint32_t mhi = rel > 32u ? ((1u << (rel - 32u)) - 1u) : 0u;
    const uint32_t a0 = blk.p01.x & mlo, a1 = blk.p01.y & mhi; // code bit 0
    const uint32_t b0 = blk.p01.z & mlo, b1 = blk.p01.w & mhi; // code bit 1
    const uint32_t d0 = blk.p2.x & mlo, d1 = blk.p2.y & mhi;   // code bit 2
    const uint32_t n1 = __popc(a0) + __popc(a1), n2 = __popc(b0) + __popc(b1), n4 = __popc(d0) + __popc(d1);
    const uint32_t n3 = __popc(a0 & b0) + __popc(a1 & b1); // code 3 = 011
    const uint32_t n5 = __popc(a0 & d0) + __popc(a1 & d1); // code 5 = 101  (codes 6, 7 never occur)
    uint32_t t[6];
    t[3] = n3; t[5] = n5;
    t[1] = n1 - n3 - n5; t[2] = n2 - n3; t[4] = n4 - n5;
    t[0] = rel - (n1 + n2 + n4 - n3 - n5);
    uint64_t a = 0, b = 0;
    uint32_t ia = 0, ib = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        a = (cv == (uint32_t)i) ? c[i] : a;
        ia = (cv == (uint32_t)i) ? t[i] : ia;
        const uint32_t w = (mrow >> (3 * i)) & 7u;
        b += c[i] * (uint64_t)w;
        ib += t[i] * w;
    }
    A = a + ia;
    B = b + ib;
}

// in-block counts of the six codes in the first (pos & 63) symbols of a dense block
__device__ __forceinline__ void pgx_dense_inblock(const PgxDenseBlk &blk, uint32_t pos_lo, uint32_t t[6]) {
    const uint32_t rel = pos_lo & 63u;
    const uint32_t mlo = rel >= 32u ? 0xFFFFFFFFu : ((1u << rel) - 1u);
    const uint32_t mhi = rel > 32u ? ((1u << (rel - 32u)) - 1u) : 0u;
    const uint32_t a0 = blk.p01.x & mlo, a1 = blk.p01.y & mhi, b0 = blk.p01.z & mlo, b1 = blk.p01.w & mhi;
    const uint32_t d0 = blk.p2.x & mlo, d1 = blk.p2.y & mhi;
    const uint32_t n1 = __popc(a0) + __popc(a1), n2 = __popc(b0) + __popc(b1), n4 = __popc(d0) + __popc(d1);
    const uint32_t n3 = __popc(a0 & b0) + __popc(a1 & b1), n5 = __popc(a0 & d0) + __popc(a1 & d1);
    t[3] = n3; t[5] = n5;
    t[1] = n1 - n3 - n5; t[2] = n2 - n3; t[4] = n4 - n5;
    t[0] = rel - (n1 + n2 + n4 - n3 - n5);
}

// Both probes of an extension in 32-bit arithmetic (BWTs shorter than 2^30: the header counts fit their low dwords):
// A0, A1 = count of code cv before p0 / p1, dB = sum over codes of mult[code] * (count before p1 - count before p0).
// One multiply per code for the pair instead of one 64-bit multiply-add per code and probe.
__device__ __forceinline__ void pgx_dense_pair32(const PgxDenseBlk &k0, uint32_t p0, const PgxDenseBlk &k1, uint32_t p1, uint32_t cv,
                                                 uint32_t mrow, uint32_t &A0, uint32_t &A1, uint32_t &dB) {
    uint32_t t0[6], t1[6];
    pgx_dense_inblock(k0, p0, t0);
    pgx_dense_inblock(k1, p1, t1);
    const uint32_t c0[6] = {k0.h0.x + t0[0], k0.h0.y + t0[1], k0.h0.z + t0[2], k0.h0.w + t0[3], k0.h1.x + t0[4], k0.h1.y + t0[5]};
    const uint32_t c1[6] = {k1.h0.x + t1[0], k1.h0.y + t1[1], k1.h0.z + t1[2], k1.h0.w + t1[3], k1.h1.x + t1[4], k1.h1.y + t1[5]};
    uint32_t a0 = 0, a1 = 0, d = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        a0 = (cv == (uint32_t)i) ? c0[i] : a0;
        a1 = (cv == (uint32_t)i) ? c1[i] : a1;
        d += (c1[i] - c0[i]) * ((mrow >> (3 * i)) & 7u);
    }
    A0 = a0; A1 = a1; dB = d;
}

// ------------------------------------------------------------------------------------------
// DENSE2 image (pgx_image.h): 384 symbols per 128-byte block = 32-byte header + three 32-byte sub-blocks of 128 symbols in two
// bit planes, exception runs for \n and N; positions below 2^32.  A probe loads the header and one sub-block.
struct PgxDense2Blk {
    uint4 h0, h1; // header: counts A C G T | N, exceptions, sub-block counts (64 bits)
    uint4 p0, p1; // the sub-block of the probe: plane 0, plane 1
};
__device__ __forceinline__ PgxDense2Blk pgx_dense2_load(const PgxDevImage &img, uint32_t pos, uint32_t &rel) {
    const uint32_t blk = (uint32_t)(((uint64_t)pos * 0xAAAAAAABull) >> 40); // pos / 384
    rel = pos - blk * PGX_D2_SYMS;
    const uint4 *bp = img.blocks + (size_t)blk * 8;
    PgxDense2Blk b;
    b.h0 = bp[0]; b.h1 = bp[1];
    const uint4 *sp = bp + 2 + 2 * (rel >> 7);
    b.p0 = sp[0]; b.p1 = sp[1];
    return b;
}
// counts of the six nuc codes (\n A C G N T) in BWT[0, pos) for the probe whose block / sub-block was loaded
__device__ __forceinline__ void pgx_dense2_counts(const PgxDevImage &img, const PgxDense2Blk &b, uint32_t pos, uint32_t rel, uint32_t c[6]) {
    const uint32_t sub = rel >> 7, r = rel & 127u;
    // in-block counts before the sub-block (three 9-bit fields per sub-block boundary)
    const uint64_t sc = ((uint64_t)b.h1.z | ((uint64_t)b.h1.w << 32)) >> (sub == 2u ? 27 : 0);
    uint32_t n0 = sub ? (uint32_t)sc & 511u : 0u, n1 = sub ? (uint32_t)(sc >> 9) & 511u : 0u, n3 = sub ? (uint32_t)(sc >> 18) & 511u : 0u;
    const uint32_t a[4] = {b.p0.x, b.p0.y, b.p0.z, b.p0.w}, d[4] = {b.p1.x, b.p1.y, b.p1.z, b.p1.w};
#pragma unroll
    for (int h = 0; h < 4; h++) {
        const int32_t t = (int32_t)r - 32 * h; // bits of this dword that lie below the position
        const uint32_t m = t >= 32 ? 0xFFFFFFFFu : (t > 0 ? ((1u << t) - 1u) : 0u);
        const uint32_t x = a[h] & m, y = d[h] & m;
        n0 += __popc(x); n1 += __popc(y); n3 += __popc(x & y);
    }
    uint32_t e0 = 0, e4 = 0;
    const uint32_t ec = b.h1.y >> 24;
    if (ec) { // rare: the block holds endmarkers or N
        const uint32_t *ep = img.exc + (b.h1.y & 0xFFFFFFu);
        for (uint32_t i = 0; i < ec; i++) {
            const uint32_t u = ep[i], st = u & 511u, ln = (u >> 9) & 511u;
            const uint32_t cnt = rel > st ? min(rel - st, ln) : 0u;
            if ((u >> 18) & 1u) e4 += cnt; else e0 += cnt;
        }
    }
    const uint32_t hsum = b.h0.x + b.h0.y + b.h0.z + b.h0.w + b.h1.x;
    c[0] = (pos - rel) - hsum + e0;               // \n: block start minus the five stored counts
    c[1] = b.h0.x + rel - (n0 + n1 - n3) - e0 - e4; // A
    c[2] = b.h0.y + n0 - n3;                      // C
    c[3] = b.h0.z + n1 - n3;                      // G
    c[4] = b.h1.x + e4;                           // N
    c[5] = b.h0.w + n3;                           // T
}
// both probes of an extension: A0, A1 = count of code cv before p0 / p1; dB = sum over codes of mult[code] * (count before p1 -
// count before p0).  NARROW: modulo 2^32 (like pgx_dense_pair32); otherwise modulo 2^64 from the exact 32-bit counts.
template <bool NARROW>
__device__ __forceinline__ void pgx_dense2_pair(const PgxDevImage &img, uint32_t p0, uint32_t p1, uint32_t cv, uint32_t mrow, uint64_t &A0, uint64_t &A1,
                                                uint64_t &dB, bool lower = true) {
    uint32_t r0, r1;
    const PgxDense2Blk k0 = pgx_dense2_load(img, p0, r0), k1 = pgx_dense2_load(img, p1, r1);
    if (lower) __builtin_amdgcn_s_setprio(0); // (the find_mems kernels raise their priority on the way to the loads: see pgx_find_mems_pairs_kernel)
    uint32_t c0[6], c1[6];
    pgx_dense2_counts(img, k0, p0, r0, c0);
    pgx_dense2_counts(img, k1, p1, r1, c1);
    uint32_t a0 = 0, a1 = 0, d32 = 0;
    uint64_t d64 = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        a0 = (cv == (uint32_t)i) ? c0[i] : a0;
        a1 = (cv == (uint32_t)i) ? c1[i] : a1;
        const uint32_t w = (mrow >> (3 * i)) & 7u;
        if (NARROW) d32 += (c1[i] - c0[i]) * w;
        else d64 += (uint64_t)((int64_t)c1[i] - (int64_t)c0[i]) * (uint64_t)w;
    }
    A0 = a0; A1 = a1; dB = NARROW ? (uint64_t)d32 : d64;
}
// one probe (primitives)
__device__ __forceinline__ void pgx_dense2_rank(const PgxDevImage &img, uint32_t pos, uint32_t cv, uint32_t mrow, uint64_t &A, uint64_t &B) {
    uint32_t rel;
    const PgxDense2Blk k = pgx_dense2_load(img, pos, rel);
    uint32_t c[6];
    pgx_dense2_counts(img, k, pos, rel, c);
    uint64_t a = 0, bb = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        a = (cv == (uint32_t)i) ? (uint64_t)c[i] : a;
        bb += (uint64_t)c[i] * (uint64_t)((mrow >> (3 * i)) & 7u);
    }
    A = a; B = bb;
}

// ------------------------------------------------------------------------------------------
// WIDE DENSE2 (pgx_image.h): the same blocks, header counts as deltas against the 64-bit bases of the block's superblock; positions
// and counts in 64 bits.  `sb` = the base table (img.sbase2 or its LDS copy): 8 words per superblock {A, C, G, T, N, their sum}.
// (MULHI: the form of pos / 384 this function had until round 3, kept for scripts/anomaly_probe.py only)
template <bool MULHI = false>
__device__ __forceinline__ PgxDense2Blk pgx_dense2w_load(const PgxDevImage &img, uint64_t pos, uint32_t &rel, uint32_t &blk) {
    blk = MULHI ? (uint32_t)(__umul64hi(pos, 0xAAAAAAAAAAAAAAABull) >> 8)
                : (uint32_t)(((pos >> 7) * 0xAAAAAAABull) >> 33); // pos / 384 = (pos / 128) / 3, exact while pos / 128 < 2^32
    rel = (uint32_t)(pos - (uint64_t)blk * PGX_D2_SYMS);
    const uint4 *bp = img.blocks + (size_t)blk * 8;
    PgxDense2Blk b;
    b.h0 = bp[0]; b.h1 = bp[1];
    const uint4 *sp = bp + 2 + 2 * (rel >> 7);
    b.p0 = sp[0]; b.p1 = sp[1];
    return b;
}
__device__ __forceinline__ void pgx_dense2w_counts(const PgxDevImage &img, const uint64_t *__restrict__ sb, const PgxDense2Blk &b, uint64_t pos, uint32_t rel,
                                                   uint32_t blk, uint64_t c[6]) {
    uint32_t d[6];
    pgx_dense2_counts(img, b, rel, rel, d); // with pos = rel: d[0] = -(sum of the five deltas) + e0, the others delta + in-block count
    const uint64_t *base = sb + (size_t)(blk >> img.d2_sb_shift) * 8;
    c[0] = (pos - rel) - base[5] + (uint64_t)(int64_t)(int32_t)d[0]; // (the deltas of a superblock stay below 2^31: d[0] is a small negative number)
    c[1] = base[0] + d[1];
    c[2] = base[1] + d[2];
    c[3] = base[2] + d[3];
    c[4] = base[4] + d[4];
    c[5] = base[3] + d[5];
}
__device__ __forceinline__ void pgx_dense2w_pair(const PgxDevImage &img, const uint64_t *__restrict__ sb, uint64_t p0, uint64_t p1, uint32_t cv, uint32_t mrow,
                                                 uint64_t &A0, uint64_t &A1, uint64_t &dB, bool lower = true) {
    uint32_t r0, r1, b0, b1;
    const PgxDense2Blk k0 = pgx_dense2w_load(img, p0, r0, b0), k1 = pgx_dense2w_load(img, p1, r1, b1);
    if (lower) __builtin_amdgcn_s_setprio(0);
    uint64_t c0[6], c1[6];
    pgx_dense2w_counts(img, sb, k0, p0, r0, b0, c0);
    pgx_dense2w_counts(img, sb, k1, p1, r1, b1, c1);
    uint64_t a0 = 0, a1 = 0, d = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        a0 = (cv == (uint32_t)i) ? c0[i] : a0;
        a1 = (cv == (uint32_t)i) ? c1[i] : a1;
        d += (c1[i] - c0[i]) * (uint64_t)((mrow >> (3 * i)) & 7u);
    }
    A0 = a0; A1 = a1; dB = d;
}
template <bool MULHI = false>
__device__ __forceinline__ void pgx_dense2w_rank(const PgxDevImage &img, uint64_t pos, uint32_t cv, uint32_t mrow, uint64_t &A, uint64_t &B) {
    uint32_t rel, blk;
    const PgxDense2Blk k = pgx_dense2w_load<MULHI>(img, pos, rel, blk);
    uint64_t c[6];
    pgx_dense2w_counts(img, img.sbase2, k, pos, rel, blk, c);
    uint64_t a = 0, bb = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        a = (cv == (uint32_t)i) ? c[i] : a;
        bb += c[i] * (uint64_t)((mrow >> (3 * i)) & 7u);
    }
    A = a; B = bb;
}

// ------------------------------------------------------------------------------------------
// rank probe: A = count of code `cv` in BWT[0,pos), B = sum over codes of mult[code] * count(code)
// (both modulo 2^64; only differences of two probes are ever used).
template <bool LDS_IMAGE>
__device__ __forceinline__ void pgx_rank_ab(const PgxDevImage &img, const uint4 *__restrict__ lds_blocks,
                                            const uint64_t *__restrict__ lds_dir, const uint16_t *__restrict__ lds_blow,
                                            uint64_t pos, uint32_t cv, uint32_t mrow, uint64_t &A, uint64_t &B) {
    if (pos > img.n) pos = img.n; // predecessor(pos >= size) = last block, rel past the end = totals
    if (img.dense == 3) { pgx_dense2w_rank(img, pos, cv, mrow, A, B); return; }
    if (img.dense == 2) { pgx_dense2_rank(img, (uint32_t)pos, cv, mrow, A, B); return; }
    if (img.dense) {
        pgx_dense_rank(pgx_dense_load<LDS_IMAGE>(img, lds_blocks, pos), pos, cv, mrow, A, B);
        return;
    }
    const uint32_t lo = pgx_find_block<LDS_IMAGE>(img, lds_dir, lds_blow, pos);
    const uint4 *bp = (LDS_IMAGE ? lds_blocks : img.blocks) + (size_t)lo * 4;
    const uint4 h0 = bp[0], h1 = bp[1], r0 = bp[2], r1 = bp[3];
    uint64_t c[6];
    c[0] = (uint64_t)h0.x | ((uint64_t)(h1.z & 0xFFu) << 32);
    c[1] = (uint64_t)h0.y | ((uint64_t)((h1.z >> 8) & 0xFFu) << 32);
    c[2] = (uint64_t)h0.z | ((uint64_t)((h1.z >> 16) & 0xFFu) << 32);
    c[3] = (uint64_t)h0.w | ((uint64_t)(h1.z >> 24) << 32);
    c[4] = (uint64_t)h1.x | ((uint64_t)(h1.w & 0xFFu) << 32);
    c[5] = (uint64_t)h1.y | ((uint64_t)((h1.w >> 8) & 0xFFu) << 32);
    uint64_t start = 0, a = 0, b = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        start += ((img.excl_mask >> i) & 1u) ? 0ull : c[i];
        a = (cv == (uint32_t)i) ? c[i] : a;
        b += c[i] * (uint64_t)((mrow >> (3 * i)) & 7u);
    }
    uint32_t rel = (uint32_t)(pos - start); // block extent <= 16 * 4095
    uint32_t ia = 0, ib = 0;
    const uint32_t arow = 1u << (3 * cv);   // one-hot weight row selecting code cv
    const uint32_t rw[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
    for (int e = 0; e < PGX_BLOCK_RUNS; e++) {
        const uint32_t w = rw[e >> 1];
        const uint32_t sh = (e & 1) ? (w >> 28) : __builtin_amdgcn_ubfe(w, 12, 4);          // 3 * code
        const uint32_t len = (e & 1) ? __builtin_amdgcn_ubfe(w, 16, 12) : (w & PGX_RUN_LEN_MAX);
        const uint32_t take = min(len, rel);
        rel -= take;
        ia += take * __builtin_amdgcn_ubfe(arow, sh, 3);
        ib += take * __builtin_amdgcn_ubfe(mrow, sh, 3);
    }
    A = a + ia;
    B = b + ib;
}

// One block decode ("trip") of the rank machinery: decodes the block holding p and returns
//   Ap, Bp  rank sums at p (primary position; p <= n)
//   As, Bs  rank sums at the secondary position p1 when `with_secondary` and this block also serves p1
//           (`covered`): once an interval is narrow (s ~ number of haplotypes) both probes of an extension
//           fall into the same 64-byte block and one decode answers both.
// A = count of code cv, B = sum over codes of mult[code] * count(code), both modulo 2^64.
template <bool LDS_IMAGE>
__device__ __forceinline__ void pgx_probe(const PgxDevImage &img, const uint4 *__restrict__ lds_blocks,
                                          const uint64_t *__restrict__ lds_dir, const uint16_t *__restrict__ lds_blow,
                                          uint64_t p, uint64_t p1, bool with_secondary, uint32_t cv, uint32_t mrow,
                                          uint64_t &Ap, uint64_t &Bp, uint64_t &As, uint64_t &Bs, bool &covered) {
    const uint32_t lo = pgx_find_block<LDS_IMAGE>(img, lds_dir, lds_blow, p);
    const uint4 *bp = (LDS_IMAGE ? lds_blocks : img.blocks) + (size_t)lo * 4;
    const uint4 h0 = bp[0], h1 = bp[1], r0 = bp[2], r1 = bp[3];
    uint64_t c[6];
    c[0] = (uint64_t)h0.x | ((uint64_t)(h1.z & 0xFFu) << 32);
    c[1] = (uint64_t)h0.y | ((uint64_t)((h1.z >> 8) & 0xFFu) << 32);
    c[2] = (uint64_t)h0.z | ((uint64_t)((h1.z >> 16) & 0xFFu) << 32);
    c[3] = (uint64_t)h0.w | ((uint64_t)(h1.z >> 24) << 32);
    c[4] = (uint64_t)h1.x | ((uint64_t)(h1.w & 0xFFu) << 32);
    c[5] = (uint64_t)h1.y | ((uint64_t)((h1.w >> 8) & 0xFFu) << 32);
    uint64_t start = 0, a = 0, b = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        start += ((img.excl_mask >> i) & 1u) ? 0ull : c[i];
        a = (cv == (uint32_t)i) ? c[i] : a;
        b += c[i] * (uint64_t)((mrow >> (3 * i)) & 7u);
    }
    uint32_t relp = (uint32_t)(p - start);   // primary position (inside the block)
    const uint64_t d1 = p1 - start;          // p1 relative to this block; wraps when p1 < start
    uint32_t rels = with_secondary ? (d1 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d1) : 0u;
    uint32_t iap = 0, ibp = 0, ias = 0, ibs = 0, total = 0;
    const uint32_t arow = 1u << (3 * cv); // one-hot weight row selecting code cv
    const uint32_t rw[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
    for (int e = 0; e < PGX_BLOCK_RUNS; e++) {
        // entry = (3 * code) << 12 | len: the stored shift indexes the 3-bit weight rows directly
        const uint32_t w = rw[e >> 1];
        const uint32_t sh = (e & 1) ? (w >> 28) : __builtin_amdgcn_ubfe(w, 12, 4);
        const uint32_t len = (e & 1) ? __builtin_amdgcn_ubfe(w, 16, 12) : (w & PGX_RUN_LEN_MAX);
        const uint32_t tp = min(len, relp), ts = min(len, rels);
        const uint32_t wa = __builtin_amdgcn_ubfe(arow, sh, 3), wm = __builtin_amdgcn_ubfe(mrow, sh, 3);
        total += len;
        relp -= tp;
        rels -= ts;
        iap += tp * wa;
        ias += ts * wa;
        ibp += tp * wm;
        ibs += ts * wm;
    }
    Ap = a + iap;
    Bp = b + ibp;
    As = a + ias;
    Bs = b + ibs;
    // p1 is served by this block when it lies strictly inside it (a probe AT the block end belongs to the
    // next block, whose header may carry a different quirk value), or at the end of the BWT
    covered = with_secondary && (d1 < (uint64_t)total || (rels == 0 && lo + 1 == img.n_blocks));
}

// The two rank probes of one extension, rank(pos0) and rank(pos1) with pos1 = pos0 + s, as at most two
// trips of pgx_probe in a rolled loop (the decode exists once in the instruction stream).
// Outputs A0, A1 and B1 - B0.  (Used by the primitives; the find_mems kernel schedules trips itself.)
template <bool LDS_IMAGE, bool MAYBE_DENSE = true>
__device__ __forceinline__ void pgx_rank_pair(const PgxDevImage &img, const uint4 *__restrict__ lds_blocks,
                                              const uint64_t *__restrict__ lds_dir, const uint16_t *__restrict__ lds_blow,
                                              uint64_t pos0, uint64_t pos1, uint32_t cv, uint32_t mrow, uint64_t &A0,
                                              uint64_t &A1, uint64_t &dB) {
    const uint64_t p0 = pos0 > img.n ? img.n : pos0, p1 = pos1 > img.n ? img.n : pos1;
    uint64_t B0 = 0, B1 = 0;
    if (MAYBE_DENSE && img.dense == 3) { pgx_dense2w_pair(img, img.sbase2, p0, p1, cv, mrow, A0, A1, dB); return; }
    if (MAYBE_DENSE && img.dense == 2) { pgx_dense2_pair<false>(img, (uint32_t)p0, (uint32_t)p1, cv, mrow, A0, A1, dB); return; }
    if (MAYBE_DENSE && img.dense) { // two independent block loads, no directory
        const PgxDenseBlk k0 = pgx_dense_load<LDS_IMAGE>(img, lds_blocks, p0), k1 = pgx_dense_load<LDS_IMAGE>(img, lds_blocks, p1);
        pgx_dense_rank(k0, p0, cv, mrow, A0, B0);
        pgx_dense_rank(k1, p1, cv, mrow, A1, B1);
        dB = B1 - B0;
        return;
    }
    A0 = 0; A1 = 0;
    bool done = false;
#pragma unroll 1
    for (int it = 0; it < 2; ++it) {
        if (!done) {
            uint64_t Ap, Bp, As, Bs;
            bool covered;
            pgx_probe<LDS_IMAGE>(img, lds_blocks, lds_dir, lds_blow, it ? p1 : p0, p1, it == 0, cv, mrow, Ap, Bp, As, Bs, covered);
            if (it == 0) {
                A0 = Ap; B0 = Bp;
                if (covered) { A1 = As; B1 = Bs; done = true; }
            } else {
                A1 = Ap; B1 = Bp;
            }
        }
    }
    dB = B1 - B0;
}

// one FMD extension of (k, kp, s) by `byte` (backward, or forward = backward on the swapped
// interval by the complement, folded into ext_tab[256 + byte]).  Returns the new size (0 = empty).
template <bool LDS_IMAGE>
__device__ __forceinline__ void pgx_extend(const PgxDevImage &img, const uint4 *lds_blocks, const uint64_t *lds_dir,
                                           const uint16_t *lds_blow, const uint32_t *s_ext, const uint64_t *s_C,
                                           uint64_t &k, uint64_t &kp, uint64_t &s, uint32_t byte, bool fwd) {
    const uint32_t e = s_ext[(fwd ? 256u : 0u) + byte];
    const uint32_t cv = PGX_EXT_CV(e), mrow = PGX_EXT_M(e);
    const uint64_t kk = fwd ? kp : k, kq = fwd ? k : kp;
    uint64_t A1, A0, dB;
    pgx_rank_pair<LDS_IMAGE>(img, lds_blocks, lds_dir, lds_blow, kk, kk + s, cv, mrow, A0, A1, dB);
    if (PGX_EXT_KILL(e) || A0 >= A1) { // rank_k >= rank_ks -> bi_interval(0,0,0), src/r-index.cpp:751
        k = 0; kp = 0; s = 0;
        return;
    }
    const uint64_t nk = A0 + s_C[PGX_EXT_V(e)], nq = kq + dB;
    s = A1 - A0;
    k = fwd ? nq : nk;
    kp = fwd ? nk : nq;
}

template <bool LDS_IMAGE>
__device__ __forceinline__ void pgx_stage_tables(const PgxDevImage &img, uint32_t *s_ext, uint64_t *s_C, uint4 *lds_blocks,
                                                 uint64_t *lds_dir, uint16_t *lds_blow) {
    for (uint32_t i = threadIdx.x; i < 512; i += blockDim.x) s_ext[i] = img.consts->ext_tab[i];
    if (threadIdx.x < 8) s_C[threadIdx.x] = img.consts->C[threadIdx.x];
    if (LDS_IMAGE) {
        const uint32_t nb4 = img.n_blocks * 4;
        for (uint32_t i = threadIdx.x; i < nb4; i += blockDim.x) lds_blocks[img.dense ? (i >> 2) * PGX_DENSE_LDS_U4 + (i & 3u) : i] = img.blocks[i];
        if (!img.dense)
            for (uint64_t i = threadIdx.x; i < img.dir_entries; i += blockDim.x) lds_dir[i] = img.dir[i];
        if (!img.dense)
            for (uint32_t i = threadIdx.x; i < img.n_blocks; i += blockDim.x) lds_blow[i] = img.blow[i];
    }
    __syncthreads();
}

// dynamic LDS carve (16-byte aligned base): [blocks | dir | blow]
#define PGX_LDS_CARVE(img)                                                                   \
    extern __shared__ __align__(16) unsigned char pgx_dyn_lds[];                              \
    uint4 *lds_blocks = reinterpret_cast<uint4 *>(pgx_dyn_lds);                               \
    uint64_t *lds_dir = reinterpret_cast<uint64_t *>(pgx_dyn_lds + (size_t)(img).n_blocks * PGX_BLOCK_BYTES);    \
    uint16_t *lds_blow = reinterpret_cast<uint16_t *>(pgx_dyn_lds + (size_t)(img).n_blocks * PGX_BLOCK_BYTES + (img).dir_entries * 8)

// ------------------------------------------------------------------------------------------
// k-mer seeds.  A backward stage of find_mems_function that starts from the full interval (step 1 at j = x + min_len - 1, step 3
// at j = e) performs its first K extensions over the window P[j - K + 1 .. j], last byte first; the table holds the result of
// those K extensions for every ACGT window, computed on the device by the same pgx_extend (so every quirk the tables carry is in
// it), and for windows that leave the index the number of extensions until the interval became empty.  One 16-byte load then
// replaces K extensions = up to 2 K line fetches, the widest ones of the search; the counters advance by K (or by the death
// depth), so MEMs, returned start positions and n_extensions stay those of the stepwise search.
//   index = sum over window bytes b_i (memory order) of code(b_i) << 2 i, code = (byte >> 1) & 3: A 0, C 1, T 2, G 3
__device__ __forceinline__ uint32_t pgx_seed_codes(uint64_t x, uint64_t &bad) {
    const uint64_t c = (x >> 1) & 0x0303030303030303ull;
    const uint64_t b0 = c & 0x0101010101010101ull, b1 = (c >> 1) & 0x0101010101010101ull;
    // the byte each code stands for; anything else in the window (N, lower case, \0, ...) makes it unusable
    const uint64_t recon = 0x4141414141414141ull + 2 * (b0 & ~b1) + 0x13 * (b1 & ~b0) + 6 * (b0 & b1);
    bad = x ^ recon;
    uint64_t t = (c | (c >> 6)) & 0x000F000F000F000Full;
    t = (t | (t >> 12)) & 0x000000FF000000FFull;
    t = (t | (t >> 24)) & 0xFFFFull;
    return (uint32_t)t;
}
__device__ __forceinline__ bool pgx_seed_index(uint64_t lo, uint64_t hi, uint32_t K, uint32_t &idx) {
    uint64_t badlo, badhi;
    const uint32_t ilo = pgx_seed_codes(lo, badlo), ihi = pgx_seed_codes(hi, badhi);
    const uint32_t nlo = K < 8u ? K : 8u, nhi = K > 8u ? K - 8u : 0u;
    const uint64_t mlo = nlo == 8u ? ~0ull : ((1ull << (8u * nlo)) - 1ull), mhi = nhi == 8u ? ~0ull : ((1ull << (8u * nhi)) - 1ull);
    idx = (ilo & ((1u << (2u * nlo)) - 1u)) | ((ihi & ((1u << (2u * nhi)) - 1u)) << 16);
    return ((badlo & mlo) | (badhi & mhi)) == 0ull;
}
