// pgx_compact.cpp -- host side of the compact result form (include/pgx.h "compact result"): pgx_compact_expand, pgx_compact_bound.
// No device, no HIP: the encoder is pgx_compact_kernels.hip, its host glue is in pgx_batch_forms.hip.
#include <new>
#include <string>

#include "pgx_host.hpp"

namespace {

// one block's bytes: reads never leave [p, end)
struct Cursor {
    const uint8_t *p, *end;
    uint64_t block;
    [[noreturn]] void fail(const char *what) const {
        throw pgx::Error(PGX_ERR_FORMAT, "pgx_compact_expand: block " + std::to_string(block) + ": " + what);
    }
    uint64_t varint() {
        uint64_t v = 0;
        for (int i = 0; i < 10; i++) {
            if (p == end) fail("truncated (the block ends inside a number or before its last one)");
            const uint8_t c = *p++;
            if (i == 9 && c > 1) fail(c & 0x80 ? "a varint longer than 10 bytes" : "the tenth byte of a varint is above 1");
            v |= (uint64_t)(c & 0x7F) << (7 * i);
            if (!(c & 0x80)) return v;
        }
        fail("a varint longer than 10 bytes"); // (not reached: i == 9 returns or fails)
    }
};

void expand_block(const pgx_compact_result *c, uint64_t k, bool tags, uint64_t *mem_offsets, pgx_mem *mems, uint64_t *run_counts, uint64_t *pos_offsets,
                  uint64_t *positions) {
    Cursor cur{nullptr, nullptr, k};
    const uint64_t o0 = c->block_offsets[k], o1 = c->block_offsets[k + 1];
    if (o0 > o1 || o1 > c->n_bytes) cur.fail("block_offsets decrease or point beyond n_bytes");
    const uint64_t m0 = c->block_first_mem[k], m1 = c->block_first_mem[k + 1];
    if (m0 > m1 || m1 > c->n_mems) cur.fail("block_first_mem decreases or points beyond n_mems");
    const uint64_t p0 = tags ? c->block_first_pos[k] : 0, p1 = tags ? c->block_first_pos[k + 1] : 0;
    if (p0 > p1 || p1 > c->n_positions) cur.fail("block_first_pos decreases or points beyond n_positions");
    cur.p = c->bytes + o0;
    cur.end = c->bytes + o1;
    const uint64_t r0 = k * PGX_COMPACT_BLOCK_READS;
    const uint64_t r1 = c->n_reads - r0 < PGX_COMPACT_BLOCK_READS ? c->n_reads : r0 + PGX_COMPACT_BLOCK_READS;
    uint64_t m = m0;
    for (uint64_t r = r0; r < r1; r++) { // 1. MEMs per read
        const uint64_t cnt = cur.varint();
        if (cnt > m1 - m) cur.fail("the MEM counts of its reads overrun block_first_mem of the next block");
        mem_offsets[r] = m;
        m += cnt;
    }
    if (m != m1) cur.fail("the MEM counts of its reads fall short of block_first_mem of the next block");
    uint64_t p = p0;
    for (m = m0; m < m1; m++) { // 2. the MEM records
        pgx_mem x;
        x.start = cur.varint();
        x.end = x.start + cur.varint();
        x.bwt_start = cur.varint();
        x.size = (int64_t)cur.varint();
        uint64_t runs = 0, np = 0;
        if (tags) {
            runs = cur.varint();
            np = cur.varint();
            if (np > p1 - p) cur.fail("the position counts of its MEMs overrun block_first_pos of the next block");
        }
        mems[m] = x;
        if (tags) {
            run_counts[m] = runs;
            pos_offsets[m] = p;
            p += np;
        }
    }
    if (p != p1) cur.fail("the position counts of its MEMs fall short of block_first_pos of the next block");
    if (tags)
        for (m = m0; m < m1; m++) { // 3. the positions
            const uint64_t a = pos_offsets[m], b = m + 1 < m1 ? pos_offsets[m + 1] : p1;
            uint64_t v = 0;
            for (uint64_t i = a; i < b; i++) {
                v += cur.varint(); // (the first as it is: v starts at 0; mod 2^64)
                positions[i] = v;
            }
        }
    if (cur.end - cur.p >= 8) cur.fail("more than 7 bytes of padding");
    if ((o1 - o0) & 7) cur.fail("not padded to a multiple of 8 bytes");
    for (; cur.p != cur.end; cur.p++)
        if (*cur.p) cur.fail("non-zero padding");
}

} // namespace

extern "C" pgx_status pgx_compact_expand(const pgx_compact_result *c, uint64_t first_block, uint64_t n_blocks, uint64_t *mem_offsets, pgx_mem *mems,
                                         uint64_t *tag_run_counts, uint64_t *pos_offsets, uint64_t *positions) {
    try {
        if (!c || !mem_offsets || !c->block_offsets || !c->block_first_mem || !c->block_first_pos || (c->n_bytes && !c->bytes) || (c->n_mems && !mems))
            throw pgx::Error(PGX_ERR_ARG, "pgx_compact_expand: null argument");
        if (c->flags & ~PGX_COMPACT_TAGS) throw pgx::Error(PGX_ERR_FORMAT, "pgx_compact_expand: unknown flag");
        const bool tags = (c->flags & PGX_COMPACT_TAGS) != 0;
        if (tags && (!pos_offsets || (c->n_mems && !tag_run_counts) || (c->n_positions && !positions)))
            throw pgx::Error(PGX_ERR_ARG, "pgx_compact_expand: PGX_COMPACT_TAGS without the tag arrays");
        if (c->block_reads != PGX_COMPACT_BLOCK_READS) throw pgx::Error(PGX_ERR_FORMAT, "pgx_compact_expand: block_reads is not PGX_COMPACT_BLOCK_READS");
        if (c->n_blocks != c->n_reads / PGX_COMPACT_BLOCK_READS + (c->n_reads % PGX_COMPACT_BLOCK_READS != 0))
            throw pgx::Error(PGX_ERR_FORMAT, "pgx_compact_expand: n_blocks is not ceil(n_reads / 64)");
        if (first_block > c->n_blocks || n_blocks > c->n_blocks - first_block) throw pgx::Error(PGX_ERR_ARG, "pgx_compact_expand: block range beyond n_blocks");
        for (uint64_t k = first_block; k < first_block + n_blocks; k++) expand_block(c, k, tags, mem_offsets, mems, tag_run_counts, pos_offsets, positions);
        if (first_block + n_blocks == c->n_blocks) { // the closing entries
            const uint64_t k = c->n_blocks;
            if (c->block_first_mem[k] != c->n_mems || (tags && c->block_first_pos[k] != c->n_positions) || c->block_offsets[k] != c->n_bytes)
                throw pgx::Error(PGX_ERR_FORMAT, "pgx_compact_expand: block " + std::to_string(k) + ": the closing table entries disagree with n_mems / n_positions / n_bytes");
            mem_offsets[c->n_reads] = c->n_mems;
            if (tags) pos_offsets[c->n_mems] = c->n_positions;
        }
        return PGX_OK;
    } catch (const pgx::Error &e) {
        pgx::set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc &) {
        pgx::set_last_error("out of host memory");
        return PGX_ERR_NOMEM;
    }
}

extern "C" uint64_t pgx_compact_bound(uint64_t n_reads, uint64_t n_mems, uint64_t n_positions, uint32_t flags) {
    const uint64_t n_blocks = n_reads / PGX_COMPACT_BLOCK_READS + (n_reads % PGX_COMPACT_BLOCK_READS != 0);
    const bool tags = (flags & PGX_COMPACT_TAGS) != 0;
    return 10 * (n_reads + n_mems * (tags ? 6 : 4) + (tags ? n_positions : 0)) + 7 * n_blocks;
}
