// pgx_query_kernels.hip -- kernels off the find_mems hot path (gfx950): the builders of the seed tables and of first_ext, and the
// per-call rank / extend / count / LF entry points (tests, the compat header, query_tags).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"
#include "pgx_rank_device.h"

// level `level` (4^level entries, src; level 0 = the full interval) -> level + 1: entry (p << 2 | c) = entry p extended by code c
__global__ void __launch_bounds__(256)
pgx_seed_build_kernel(PgxDevImage img, const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t level, uint64_t n_dst, uint64_t limit, int end_table) {
    __shared__ uint32_t s_ext[512];
    __shared__ uint64_t s_C[8];
    pgx_stage_tables<false>(img, s_ext, s_C, nullptr, nullptr, nullptr);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_dst; i += (uint64_t)gridDim.x * blockDim.x) { // (a level can have 2^32 entries)
    uint64_t k = 0, kp = 0, s = img.n;
    uint32_t depth = 0;
    const uint32_t base_depth = end_table ? 1u : 0u; // the end table: level 0 is the full interval extended by 0 (pattern[len]), which counts as an extension
    if (end_table && !level) {
        pgx_extend<false>(img, nullptr, nullptr, nullptr, s_ext, s_C, k, kp, s, 0u, false);
        if (s == 0) { k = 0; kp = 0; depth = 1u; }
    }
    if (level) {
        const uint4 e = src[i >> 2];
        k = (uint64_t)e.x | ((uint64_t)(e.w & 0xFFu) << 32);
        kp = (uint64_t)e.y | ((uint64_t)((e.w >> 8) & 0xFFu) << 32);
        s = (uint64_t)e.z | ((uint64_t)((e.w >> 16) & 0xFFu) << 32);
        depth = e.w >> 24;
    }
    if (s != 0) {
        const uint32_t byte = (0x47544341u >> (8u * (uint32_t)(i & 3))) & 0xFFu; // "ACTG"[code]
        pgx_extend<false>(img, nullptr, nullptr, nullptr, s_ext, s_C, k, kp, s, byte, false);
        if (s == 0) { k = 0; kp = 0; depth = level + 1 + base_depth; }
        else if (k >= limit || kp >= limit || k + s >= limit || kp + s >= limit || k + s < k || kp + s < kp) { k = 0; kp = 0; s = 0; depth = PGX_SEED_UNUSABLE; }
    }
    uint4 o;
    o.x = (uint32_t)k; o.y = (uint32_t)kp; o.z = (uint32_t)s;
    o.w = (uint32_t)(k >> 32) | ((uint32_t)(kp >> 32) << 8) | ((uint32_t)(s >> 32) << 16) | (depth << 24);
    dst[i] = o;
  }
}

// first extension of every backward stage: the full interval extended by each byte value
__global__ void __launch_bounds__(256) pgx_first_ext_kernel(PgxDevImage img, uint4 *__restrict__ out) { // out[512]
    __shared__ uint32_t s_ext[512];
    __shared__ uint64_t s_C[8];
    pgx_stage_tables<false>(img, s_ext, s_C, nullptr, nullptr, nullptr);
    uint64_t k = 0, kp = 0, s = img.n;
    pgx_extend<false>(img, nullptr, nullptr, nullptr, s_ext, s_C, k, kp, s, threadIdx.x, false);
    auto pack = [](uint64_t k_, uint64_t q_, uint64_t s_) { // like a seed entry: low dwords, then the bits 32..39 of each
        return make_uint4((uint32_t)k_, (uint32_t)q_, (uint32_t)s_, (uint32_t)((k_ >> 32) & 0xFFu) | ((uint32_t)((q_ >> 32) & 0xFFu) << 8) | ((uint32_t)((s_ >> 32) & 0xFFu) << 16));
    };
    out[threadIdx.x] = pack(k, kp, s);
    k = 0; kp = 0; s = img.n; // by 0 (what pattern[len] reads as), then by the byte
    pgx_extend<false>(img, nullptr, nullptr, nullptr, s_ext, s_C, k, kp, s, 0u, false);
    if (s) pgx_extend<false>(img, nullptr, nullptr, nullptr, s_ext, s_C, k, kp, s, threadIdx.x, false);
    out[256 + threadIdx.x] = pack(k, kp, s);
}

// ------------------------------------------------------------------------------------------
// primitives for tests (mirror rank_at_cached_encoded / backward_extend_encoded / forward_...)
__global__ void __launch_bounds__(256)
pgx_rank_kernel(PgxDevImage img, const uint64_t *__restrict__ pos, uint64_t n, int true_codes, uint64_t *__restrict__ out) {
    // one (position, slot) per thread
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 6 * n) return;
    const uint64_t i = t / 6;
    const uint32_t sl = (uint32_t)(t - 6 * i);
    const uint32_t sigma = img.consts->sigma;
    uint64_t A = 0, B;
    if (true_codes) pgx_rank_ab<false>(img, nullptr, nullptr, nullptr, pos[i], sl, 0, A, B);
    else if (sl < sigma) pgx_rank_ab<false>(img, nullptr, nullptr, nullptr, pos[i], img.consts->slot_code[sl], 0, A, B);
    out[t] = A;
}
// Probe of the round-3 anomaly (DESIGN.md "stale counts"; scripts/anomaly_probe.py; PGX_RANK_PROBE selects it in pgx_rank_batch): the shape
// pgx_rank_kernel had until commit 66308c2 -- LOOP: one thread walks the six slots of its position -- and the form of pos / 384 it used -- MULHI --,
// each switchable on its own, over a wide dense2 image with true codes.  Test-only.
template <bool LOOP, bool MULHI>
__global__ void __launch_bounds__(256)
pgx_rank_probe_kernel(PgxDevImage img, const uint64_t *__restrict__ pos, uint64_t n, uint64_t *__restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (LOOP) {
        if (t >= n) return;
        for (uint32_t sl = 0; sl < 6; sl++) {
            uint64_t A = 0, B;
            const uint64_t p = pos[t] > img.n ? img.n : pos[t];
            pgx_dense2w_rank<MULHI>(img, p, sl, 0, A, B);
            out[t * 6 + sl] = A;
        }
    } else {
        if (t >= 6 * n) return;
        const uint64_t i = t / 6;
        uint64_t A = 0, B;
        const uint64_t p = pos[i] > img.n ? img.n : pos[i];
        pgx_dense2w_rank<MULHI>(img, p, (uint32_t)(t - 6 * i), 0, A, B);
        out[t] = A;
    }
}
template __global__ void pgx_rank_probe_kernel<true, true>(PgxDevImage, const uint64_t *, uint64_t, uint64_t *);
template __global__ void pgx_rank_probe_kernel<true, false>(PgxDevImage, const uint64_t *, uint64_t, uint64_t *);
template __global__ void pgx_rank_probe_kernel<false, true>(PgxDevImage, const uint64_t *, uint64_t, uint64_t *);

template <bool LDS_IMAGE>
__global__ void __launch_bounds__(256)
pgx_extend_kernel(PgxDevImage img, const pgx_biint *__restrict__ in, const uint8_t *__restrict__ sym,
                  const uint8_t *__restrict__ forward, uint64_t n, pgx_biint *__restrict__ out) {
    __shared__ uint32_t s_ext[512];
    __shared__ uint64_t s_C[8];
    PGX_LDS_CARVE(img);
    pgx_stage_tables<LDS_IMAGE>(img, s_ext, s_C, lds_blocks, lds_dir, lds_blow);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t k = in[i].forward, kp = in[i].reverse, s = (uint64_t)in[i].size;
    pgx_extend<LDS_IMAGE>(img, lds_blocks, lds_dir, lds_blow, s_ext, s_C, k, kp, s, sym[i], forward[i] != 0);
    pgx_biint o;
    o.forward = k; o.reverse = kp; o.size = (int64_t)s;
    out[i] = o;
}
template __global__ void pgx_extend_kernel<false>(PgxDevImage, const pgx_biint *, const uint8_t *, const uint8_t *, uint64_t, pgx_biint *);
template __global__ void pgx_extend_kernel<true>(PgxDevImage, const pgx_biint *, const uint8_t *, const uint8_t *, uint64_t, pgx_biint *);


// ------------------------------------------------------------------------------------------
// query_tags path: FastLocate::count / count_encoded (r-index.hpp:540-556), one lane
// per read: range = {0, n-1}; for each symbol from the end: LF (src/r-index.cpp:650-711).  An empty
// range is {1, 0} and stays empty.
template <bool LDS_IMAGE>
__global__ void __launch_bounds__(256)
pgx_count_kernel(PgxDevImage img, const uint8_t *__restrict__ reads, const uint64_t *__restrict__ offsets, uint64_t n_reads,
                 pgx_range *__restrict__ out) {
    __shared__ uint32_t s_cnt[256];
    __shared__ uint64_t s_C[8];
    PGX_LDS_CARVE(img);
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) s_cnt[i] = img.consts->cnt_tab[i];
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
    const uint64_t rid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (rid >= n_reads) return;
    const uint64_t base = offsets[rid], len = offsets[rid + 1] - base;
    uint64_t lo = 0, hi = img.n - 1;
    if (img.n == 0) { lo = 1; hi = 0; }
    for (uint64_t i = len; i > 0 && lo <= hi; i--) {
        const uint32_t e = s_cnt[reads[base + i - 1]];
        if (PGX_EXT_KILL(e)) { lo = 1; hi = 0; break; }
        uint64_t A0, A1, dB;
        pgx_rank_pair<LDS_IMAGE>(img, lds_blocks, lds_dir, lds_blow, lo, hi + 1, PGX_EXT_CV(e), 0u, A0, A1, dB);
        if (A1 == A0) { lo = 1; hi = 0; break; } // sym_inside == 0 -> {1, 0}
        lo = A0 + s_C[PGX_EXT_V(e)];
        hi = lo + (A1 - A0) - 1;
    }
    pgx_range r;
    r.first = lo; r.second = hi;
    out[rid] = r;
}
template __global__ void pgx_count_kernel<false>(PgxDevImage, const uint8_t *, const uint64_t *, uint64_t, pgx_range *);
template __global__ void pgx_count_kernel<true>(PgxDevImage, const uint8_t *, const uint64_t *, uint64_t, pgx_range *);

// One LF step per query (FastLocate::LF src/r-index.cpp:650-687 / LF_encoded :689-711): the inclusive range [first, second]
// mapped by `sym`; an empty input or result is {1, 0}.  Same tables as pgx_count_kernel.
__global__ void __launch_bounds__(256)
pgx_lf_kernel(PgxDevImage img, const pgx_range *__restrict__ in, const uint8_t *__restrict__ sym, uint64_t n, pgx_range *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = img.consts->cnt_tab[sym[i]];
    pgx_range r;
    r.first = 1; r.second = 0;
    const uint64_t lo = in[i].first, hi = in[i].second;
    if (!PGX_EXT_KILL(e) && lo <= hi) { // positions beyond n rank like n (predecessor -> last block, totals)
        uint64_t A0, A1, dB;
        pgx_rank_pair<false>(img, nullptr, nullptr, nullptr, lo, hi + 1, PGX_EXT_CV(e), 0u, A0, A1, dB);
        if (A1 != A0) {
            r.first = A0 + img.consts->C[PGX_EXT_V(e)];
            r.second = r.first + (A1 - A0) - 1;
        }
    }
    out[i] = r;
}

// ------------------------------------------------------------------------------------------
// FastLocate::rankAt_encoded as the reference executes it on an encoded index without N (quirk 3, pgx_device.h PgxLitImage)
__device__ __forceinline__ uint64_t pgx_lit_rank(const PgxLitImage &lit, uint64_t pos, uint32_t target) {
    // predecessor: last block start <= pos (positions at or beyond the end fall into the last block)
    uint64_t lo = 0, hi = lit.n_blocks; // bstart[0] = 0
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (lit.bstart[mid] <= pos) lo = mid; else hi = mid;
    }
    const uint64_t rel = pos - lit.bstart[lo];
    uint64_t rank = 0, cur = 0;
    for (uint32_t e = lit.roff[lo]; e < lit.roff[lo + 1]; e++) { // EncodedBlock::rank_of_code, src/r-index.cpp:114-131
        const uint64_t u = lit.runs[e], len = u & ((1ull << 56) - 1);
        if ((uint32_t)(u >> 56) == target) {
            if (cur + len > rel) { rank += rel - cur; break; }
            rank += len;
        }
        cur += len;
        if (cur > rel) break;
    }
    return rank + lit.cum[lo * 6 + target];
}
__global__ void __launch_bounds__(256)
pgx_lit_count_kernel(PgxLitImage lit, const uint8_t *__restrict__ reads, const uint64_t *__restrict__ offsets, const pgx_range *__restrict__ in,
                     const uint8_t *__restrict__ sym, uint64_t n, pgx_range *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t lo, hi, len, base = 0;
    if (in) { lo = in[i].first; hi = in[i].second; len = 1; }
    else { lo = 0; hi = lit.n - 1; base = offsets[i]; len = offsets[i + 1] - base; }
    for (uint64_t t = len; t > 0; t--) { // LF_encoded, src/r-index.cpp:689-711: no symbol is rejected, an empty range stays {1, 0}
        const uint32_t byte = in ? sym[i] : reads[base + t - 1];
        if (lo > hi) { lo = 1; hi = 0; continue; }
        const uint32_t target = lit.code_of[byte];
        const uint64_t f = pgx_lit_rank(lit, lo, target), inside = pgx_lit_rank(lit, hi + 1, target) - f;
        if (inside == 0) { lo = 1; hi = 0; continue; }
        lo = f + lit.C[lit.cslot_of[byte]];
        hi = lo + inside - 1;
    }
    pgx_range r;
    r.first = lo; r.second = hi;
    out[i] = r;
}
