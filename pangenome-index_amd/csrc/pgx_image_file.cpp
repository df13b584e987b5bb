// pgx_image_file.cpp -- the image file of include/pgx.h ("image file"): the built host images of a handle written once and read back
// without a .ri or a tag file.  Host only, no HIP: the section sum on host threads, the writer (pgx_index_save_image), the reader
// (pgx_index_open_image) and pgx_image_file_info.  The device side of the check is in pgx_images.hip / pgx_image_sum_kernels.hip.
//
// The reader trusts nothing it has not checked: the header's identity, the header sum, then every table entry against the size the
// constants imply (section_rule below: the one place that states how large each array of pgx_image.h is -- the writer refuses to
// write an image that breaks it, so the builders and the reader cannot drift apart unnoticed) and against the file size, in
// arithmetic that cannot wrap.  Only then is anything allocated, by those lengths.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "pgx_host.hpp"

namespace pgx {

// ------------------------------------------------------------------------------------------
// the section sum (include/pgx.h "SECTION SUM")
static inline uint64_t sum_term(uint64_t w, uint64_t i) {
    uint64_t z = w + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 32)) * 0xD6E8FEB86659FD93ull;
    return z ^ (z >> 32);
}

uint64_t image_sum_words(const uint8_t *p, uint64_t first_word, uint64_t n_words, uint64_t n_bytes) {
    uint64_t s = 0;
    const uint64_t whole = n_bytes >> 3, end = first_word + n_words;
    for (uint64_t i = first_word; i < end && i < whole; i++) {
        uint64_t w;
        std::memcpy(&w, p + (i << 3), 8);
        s += sum_term(w, i);
    }
    if (end > whole && (n_bytes & 7) && whole >= first_word) { // the padded last word
        uint64_t w = 0;
        std::memcpy(&w, p + (whole << 3), (size_t)(n_bytes & 7));
        s += sum_term(w, whole);
    }
    return s;
}

uint64_t image_sum_host(const void *bytes, uint64_t n, unsigned threads) {
    const uint8_t *p = static_cast<const uint8_t *>(bytes);
    const uint64_t nw = (n + 7) >> 3;
    if (threads == 0) threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency() / 2));
    threads = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(threads, nw / (1u << 20) + 1));
    if (threads == 1) return image_sum_words(p, 0, nw, n);
    std::vector<uint64_t> part(threads, 0);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < threads; t++)
        th.emplace_back([&, t]() {
            const uint64_t a = nw * t / threads, b = nw * (t + 1) / threads;
            part[t] = image_sum_words(p, a, b - a, n);
        });
    for (auto &x : th) x.join();
    uint64_t s = 0;
    for (uint64_t v : part) s += v;
    return s;
}

// ------------------------------------------------------------------------------------------
// sections
struct SectionKind { uint32_t id, elem; const char *name; };
static const SectionKind kKinds[] = {
    {PGX_IMAGE_SEC_CONSTS, 1, "consts"}, {PGX_IMAGE_SEC_BLOCKS, 1, "blocks"}, {PGX_IMAGE_SEC_DIR, 8, "dir"}, {PGX_IMAGE_SEC_BSTART, 8, "bstart"},
    {PGX_IMAGE_SEC_BLOW, 2, "blow"}, {PGX_IMAGE_SEC_EXC, 4, "exc"}, {PGX_IMAGE_SEC_PAIRS, 1, "pairs"}, {PGX_IMAGE_SEC_SBASE2, 8, "sbase2"},
    {PGX_IMAGE_SEC_PBASE, 8, "pbase"}, {PGX_IMAGE_SEC_TSTART, 8, "tstart"}, {PGX_IMAGE_SEC_TVALS, 8, "tvals"}, {PGX_IMAGE_SEC_TDIR, 4, "tdir"},
    {PGX_IMAGE_SEC_N_RUNS, 8, "n_runs"},
    {PGX_IMAGE_SEC_LOC_CONSTS, 1, "loc_consts"}, {PGX_IMAGE_SEC_RSTART, 8, "rstart"}, {PGX_IMAGE_SEC_RSAMP, 8, "rsamp"}, {PGX_IMAGE_SEC_RDIR, 4, "rdir"},
    {PGX_IMAGE_SEC_LPOS, 8, "lpos"}, {PGX_IMAGE_SEC_LNEXT, 8, "lnext"}, {PGX_IMAGE_SEC_LDIR, 4, "ldir"},
    {PGX_IMAGE_SEC_LIT_BSTART, 8, "lit_bstart"}, {PGX_IMAGE_SEC_LIT_CUM, 8, "lit_cum"}, {PGX_IMAGE_SEC_LIT_RUNS, 8, "lit_runs"},
    {PGX_IMAGE_SEC_LIT_ROFF, 4, "lit_roff"}, {PGX_IMAGE_SEC_LIT_TABS, 4, "lit_tabs"},
};
static const SectionKind *kind_of(uint32_t id) {
    for (const auto &k : kKinds) if (k.id == id) return &k;
    return nullptr;
}
static const uint64_t kLitTabsBytes = 256 * 4 + 256 * 4 + 8 * 8; // LitTabs below

// the ids a file of this shape holds, in file order
static std::vector<uint32_t> expected_ids(uint32_t flags) {
    std::vector<uint32_t> ids;
    for (uint32_t id = PGX_IMAGE_SEC_CONSTS; id <= PGX_IMAGE_SEC_N_RUNS; id++) ids.push_back(id);
    if (flags & PGX_IMAGE_HAS_LOCATE) for (uint32_t id = PGX_IMAGE_SEC_LOC_CONSTS; id <= PGX_IMAGE_SEC_LDIR; id++) ids.push_back(id);
    if (flags & PGX_IMAGE_HAS_LITERAL) for (uint32_t id = PGX_IMAGE_SEC_LIT_BSTART; id <= PGX_IMAGE_SEC_LIT_TABS; id++) ids.push_back(id);
    return ids;
}

static const uint64_t kNoSize = ~(uint64_t)0; // a product that does not fit: equal to no length a file can have
static inline uint64_t mul(uint64_t a, uint64_t b) { return (b && a > (kNoSize - 1) / b) ? kNoSize : a * b; }
static inline uint64_t add(uint64_t a, uint64_t b) { return (a == kNoSize || b == kNoSize || a > kNoSize - 1 - b) ? kNoSize : a + b; }

// The four array lengths that no constant of pgx_image.h states; the meta record carries them (include/pgx.h, offsets 424 .. 455)
struct FreeCounts { uint64_t tag_items = 0, exc = 0, lit_blocks = 0, lit_runs = 0; };

// How many bytes section `id` has for these constants and counts.  The expressions are those of the builders in pgx_index.cpp
// (build_rank_image and the images it chooses among, build_tag_image, build_locate_image, build_literal_image).  Throws PGX_ERR_FORMAT
// naming the section when the constants contradict each other.
static uint64_t section_rule(uint32_t id, const PgxConsts &c, const PgxLocConsts *lc, bool has_rank, bool has_tags, bool lit, const FreeCounts &fc) {
    auto bad = [&](const char *what) -> uint64_t { throw Error(PGX_ERR_FORMAT, std::string("image file: section ") + kind_of(id)->name + ": constants are inconsistent (" + what + ")"); };
    auto exact = [](uint64_t v) { return v; };
    if (id == PGX_IMAGE_SEC_CONSTS) return sizeof(PgxConsts); // (asked before the constants are read)
    if (id == PGX_IMAGE_SEC_LOC_CONSTS) return sizeof(PgxLocConsts);
    const bool rl = c.image_kind == PGX_IMAGE_RL, d1 = c.image_kind == PGX_IMAGE_DENSE, d2 = c.image_kind == PGX_IMAGE_DENSE2;
    if (has_rank) {
        if (!(rl || d1 || d2)) bad("image_kind");
        if (c.n >> PGX_COUNT_BITS) bad("n");
        if (d1 && (uint64_t)c.n_blocks != (c.n >> 6) + 1) bad("n_blocks of the dense image");
        if (d2 && (uint64_t)c.n_blocks != c.n / PGX_D2_SYMS + 1) bad("n_blocks of the dense2 image");
        if (rl && (c.dir_shift > PGX_DIR_MAX_SHIFT || c.dir_entries != (c.n >> c.dir_shift) + 2 || c.n_blocks == 0)) bad("directory of the run-length image");
        if (!rl && c.dir_entries != 1) bad("dir_entries");
        if (c.has_pairs && rl) bad("has_pairs");
        if (c.has_pairs && c.pairs_stride != PGX_PAIRS_SYMS && c.pairs_stride != PGX_PAIRS_STRIDE64) bad("pairs_stride");
        if (c.wide && !d2) bad("wide");
    }
    const uint64_t nbp = (has_rank && c.has_pairs) ? c.n / c.pairs_stride + 1 : 0;
    switch (id) {
    case PGX_IMAGE_SEC_CONSTS: return exact(sizeof(PgxConsts));
    case PGX_IMAGE_SEC_BLOCKS: return exact(!has_rank ? 0 : mul(c.n_blocks, d2 ? PGX_D2_BLOCK_BYTES : PGX_BLOCK_BYTES));
    case PGX_IMAGE_SEC_DIR: return exact(!has_rank ? 0 : mul(c.dir_entries, 8));
    case PGX_IMAGE_SEC_BSTART: return exact(has_rank && rl ? mul(c.n_blocks, 8) : 0);
    case PGX_IMAGE_SEC_BLOW: return exact(has_rank && rl ? mul(c.n_blocks, 2) : 0);
    case PGX_IMAGE_SEC_EXC: // at most 192 alternating runs in the 384 symbols of a block; one unused entry where there is none
        if (!(has_rank && d2)) { if (fc.exc) bad("exception runs without a dense2 image"); return exact(0); }
        if (fc.exc == 0 || fc.exc > add(mul(c.n_blocks, 192), 1)) bad("number of exception runs");
        return exact(mul(fc.exc, 4));
    case PGX_IMAGE_SEC_SBASE2: {
        if (!(has_rank && d2)) return exact(0);
        if (c.n_sb2 == 0 || c.n_sb2 > PGX_SB_MAX) bad("n_sb2");
        if (c.wide ? (c.d2_sb_shift > 31 || (((uint64_t)c.n_blocks - 1) >> c.d2_sb_shift) + 1 != c.n_sb2) : c.n_sb2 != 1) bad("superblocks of the dense2 image");
        return exact((uint64_t)c.n_sb2 * 8 * 8);
    }
    case PGX_IMAGE_SEC_PAIRS: return exact(mul(nbp, PGX_PAIRS_BLOCK_BYTES));
    case PGX_IMAGE_SEC_PBASE: {
        if (!nbp) return exact(0);
        if (c.n_sbp == 0 || c.n_sbp > PGX_SB_MAX) bad("n_sbp");
        if (c.wide ? (c.pairs_sb_shift > 31 || ((nbp - 1) >> c.pairs_sb_shift) + 1 != c.n_sbp) : c.n_sbp != 1) bad("superblocks of the PAIRS image");
        return exact((uint64_t)c.n_sbp * 24 * 8);
    }
    case PGX_IMAGE_SEC_TSTART: return exact(has_tags ? mul(c.n_tag_runs, 8) : 0);
    case PGX_IMAGE_SEC_TVALS: // one value per stored item
        if (!has_tags && fc.tag_items) bad("tag values without tags");
        return exact(mul(fc.tag_items, 8));
    case PGX_IMAGE_SEC_TDIR:
        if (has_tags && (c.tag_dir_shift > 40 || (c.n_tag_runs >> 32))) bad("tag directory");
        return exact(has_tags ? mul(c.tag_dir_entries, 4) : 0);
    case PGX_IMAGE_SEC_N_RUNS: // (the last section every file has: the literal counts belong to sections that may be absent)
        if (!lit && (fc.lit_blocks || fc.lit_runs)) bad("counts of a literal count image the file does not hold");
        return exact(8);
    case PGX_IMAGE_SEC_LOC_CONSTS: return exact(sizeof(PgxLocConsts));
    case PGX_IMAGE_SEC_RSTART: return exact(mul(add(lc->n_runs, 1), 8));
    case PGX_IMAGE_SEC_RSAMP: return exact(mul(lc->n_runs, 8));
    case PGX_IMAGE_SEC_RDIR:
        if (lc->rdir_shift > 48 || lc->rdir_entries != ((lc->n + 1) >> lc->rdir_shift) + 2 || (lc->n_runs >> 32)) bad("run directory of the locate image");
        return exact(mul(lc->rdir_entries, 4));
    case PGX_IMAGE_SEC_LPOS: case PGX_IMAGE_SEC_LNEXT: return exact(mul(lc->n_last, 8));
    case PGX_IMAGE_SEC_LDIR:
        if (lc->ldir_shift > 48 || (lc->n_last >> 32)) bad("tail directory of the locate image");
        return exact(mul(lc->ldir_entries, 4));
    case PGX_IMAGE_SEC_LIT_BSTART: return exact(mul(fc.lit_blocks, 8));
    case PGX_IMAGE_SEC_LIT_CUM: return exact(mul(fc.lit_blocks, 6 * 8));
    case PGX_IMAGE_SEC_LIT_RUNS:
        if (fc.lit_runs == 0 || (fc.lit_runs >> 32)) bad("number of runs");
        return exact(mul(fc.lit_runs, 8));
    case PGX_IMAGE_SEC_LIT_ROFF: return exact(mul(add(fc.lit_blocks, 1), 4));
    case PGX_IMAGE_SEC_LIT_TABS: return exact(kLitTabsBytes);
    default: break;
    }
    throw Error(PGX_ERR_FORMAT, "image file: unknown section id " + std::to_string(id));
}

// ------------------------------------------------------------------------------------------
// header, table and meta record as bytes
template <class T> static void put(std::vector<uint8_t> &b, size_t at, T v) { std::memcpy(b.data() + at, &v, sizeof v); }
template <class T> static T get(const uint8_t *b, size_t at) { T v; std::memcpy(&v, b + at, sizeof v); return v; }

static void meta_to_bytes(const IndexMeta &m, const FreeCounts &fc, uint8_t *o) {
    std::memset(o, 0, PGX_IMAGE_META_BYTES);
    std::memcpy(o, m.sym_map, 256);
    std::memcpy(o + 256, m.C, 64);
    std::memcpy(o + 320, &m.sigma, 4); std::memcpy(o + 324, &m.encoded, 4); std::memcpy(o + 328, &m.hasN, 4); std::memcpy(o + 332, &m.tags_format, 4);
    std::memcpy(o + 336, &m.sequence_size, 8); std::memcpy(o + 344, &m.max_length, 8); std::memcpy(o + 352, &m.n_file_blocks, 8);
    std::memcpy(o + 360, &m.ref_block_mean_bytes, 8); std::memcpy(o + 368, &m.n_samples, 8);
    std::memcpy(o + 376, m.sym_total, 48);
    std::memcpy(o + 424, &fc.tag_items, 8); std::memcpy(o + 432, &fc.exc, 8); std::memcpy(o + 440, &fc.lit_blocks, 8); std::memcpy(o + 448, &fc.lit_runs, 8);
}
static void meta_from_bytes(const uint8_t *o, IndexMeta &m, FreeCounts &fc) {
    fc.tag_items = get<uint64_t>(o, 424); fc.exc = get<uint64_t>(o, 432); fc.lit_blocks = get<uint64_t>(o, 440); fc.lit_runs = get<uint64_t>(o, 448);
    std::memcpy(m.sym_map, o, 256);
    std::memcpy(m.C, o + 256, 64);
    m.sigma = get<uint32_t>(o, 320); m.encoded = get<uint32_t>(o, 324); m.hasN = get<uint32_t>(o, 328); m.tags_format = get<uint32_t>(o, 332);
    m.sequence_size = get<uint64_t>(o, 336); m.max_length = get<uint64_t>(o, 344); m.n_file_blocks = get<uint64_t>(o, 352);
    m.ref_block_mean_bytes = get<double>(o, 360); m.n_samples = get<uint64_t>(o, 368);
    std::memcpy(m.sym_total, o + 376, 48);
}

struct FileHead {
    uint32_t version = 0, layout = 0, consts_bytes = 0, loc_consts_bytes = 0, mode = 0, has_rank = 0, has_tags = 0, n_sections = 0, meta_bytes = 0, flags = 0;
    uint64_t header_sum = 0, file_bytes = 0;
    std::vector<ImageSection> table;
    IndexMeta meta;
    FreeCounts counts;
};

static uint64_t head_sum(std::vector<uint8_t> head) { // (a copy: the sum field reads as zero)
    std::memset(head.data() + 48, 0, 8);
    return image_sum_words(head.data(), 0, (head.size() + 7) >> 3, head.size());
}

struct Fd {
    int fd = -1;
    ~Fd() { if (fd >= 0) ::close(fd); }
};

static void pread_all(int fd, void *dst, uint64_t bytes, uint64_t off, const char *what) {
    uint8_t *p = static_cast<uint8_t *>(dst);
    while (bytes) {
        const ssize_t k = ::pread(fd, p, (size_t)std::min<uint64_t>(bytes, 1u << 30), (off_t)off);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) throw Error(k < 0 ? PGX_ERR_IO : PGX_ERR_FORMAT, std::string("image file: cannot read ") + what + (k < 0 ? std::string(": ") + std::strerror(errno) : std::string(": the file ends early")));
        p += k; off += (uint64_t)k; bytes -= (uint64_t)k;
    }
}

// header checks 1 and 2 of pgx_index_open_image, and the table as it stands (its entries are checked by check_entry)
static void read_head(int fd, const std::string &path, FileHead &h) {
    struct stat st;
    if (::fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) throw Error(PGX_ERR_IO, "image file: not a regular file: " + path);
    h.file_bytes = (uint64_t)st.st_size;
    uint8_t hd[PGX_IMAGE_HEADER_BYTES];
    if (h.file_bytes < 8) throw Error(PGX_ERR_FORMAT, "not an image file (shorter than the magic): " + path);
    pread_all(fd, hd, 8, 0, "the magic");
    if (std::memcmp(hd, PGX_IMAGE_MAGIC, 8) != 0) throw Error(PGX_ERR_FORMAT, "not an image file (no PGXIMAGE magic): " + path);
    if (h.file_bytes < PGX_IMAGE_HEADER_BYTES) throw Error(PGX_ERR_FORMAT, "image file: truncated inside the header: " + path);
    pread_all(fd, hd, PGX_IMAGE_HEADER_BYTES, 0, "the header");
    h.version = get<uint32_t>(hd, 8); h.layout = get<uint32_t>(hd, 12); h.consts_bytes = get<uint32_t>(hd, 16); h.loc_consts_bytes = get<uint32_t>(hd, 20);
    h.mode = get<uint32_t>(hd, 24); h.has_rank = get<uint32_t>(hd, 28); h.has_tags = get<uint32_t>(hd, 32); h.n_sections = get<uint32_t>(hd, 36);
    h.meta_bytes = get<uint32_t>(hd, 40); h.flags = get<uint32_t>(hd, 44); h.header_sum = get<uint64_t>(hd, 48);
    auto other_build = [&](const std::string &what) {
        throw Error(PGX_ERR_UNSUPPORTED, "image file written by another build (" + what + "), make it again: " + path);
    };
    if (h.version != PGX_IMAGE_FILE_VERSION) other_build("file version " + std::to_string(h.version) + ", this build reads " + std::to_string(PGX_IMAGE_FILE_VERSION));
    if (h.layout != PGX_IMAGE_LAYOUT) other_build("image layout " + std::to_string(h.layout) + ", this build has " + std::to_string(PGX_IMAGE_LAYOUT));
    if (h.consts_bytes != sizeof(PgxConsts)) other_build("PgxConsts of " + std::to_string(h.consts_bytes) + " bytes, this build has " + std::to_string(sizeof(PgxConsts)));
    if (h.loc_consts_bytes != sizeof(PgxLocConsts)) other_build("PgxLocConsts of " + std::to_string(h.loc_consts_bytes) + " bytes, this build has " + std::to_string(sizeof(PgxLocConsts)));
    if (h.meta_bytes != PGX_IMAGE_META_BYTES) other_build("meta record of " + std::to_string(h.meta_bytes) + " bytes");
    if (h.n_sections == 0 || h.n_sections > PGX_IMAGE_MAX_SECTIONS)
        throw Error(PGX_ERR_FORMAT, "image file: section count " + std::to_string(h.n_sections) + " outside 1.." + std::to_string(PGX_IMAGE_MAX_SECTIONS) + ": " + path);
    const uint64_t head_bytes = PGX_IMAGE_HEADER_BYTES + (uint64_t)PGX_IMAGE_ENTRY_BYTES * h.n_sections + PGX_IMAGE_META_BYTES; // (at most 64 entries: cannot wrap)
    if (h.file_bytes < head_bytes) throw Error(PGX_ERR_FORMAT, "image file: truncated inside the section table: " + path);
    std::vector<uint8_t> head((size_t)head_bytes);
    pread_all(fd, head.data(), head_bytes, 0, "the section table");
    if (head_sum(head) != h.header_sum) throw Error(PGX_ERR_FORMAT, "image file: the header sum does not match (header, section table or meta record damaged): " + path);
    h.table.resize(h.n_sections);
    for (uint32_t i = 0; i < h.n_sections; i++) {
        const uint8_t *e = head.data() + PGX_IMAGE_HEADER_BYTES + (size_t)PGX_IMAGE_ENTRY_BYTES * i;
        h.table[i].id = get<uint32_t>(e, 0); h.table[i].elem_size = get<uint32_t>(e, 4);
        h.table[i].bytes = get<uint64_t>(e, 8); h.table[i].offset = get<uint64_t>(e, 16); h.table[i].sum = get<uint64_t>(e, 24);
    }
    meta_from_bytes(head.data() + PGX_IMAGE_HEADER_BYTES + (size_t)PGX_IMAGE_ENTRY_BYTES * h.n_sections, h.meta, h.counts);
}

static std::string sec_name(uint32_t id) {
    const SectionKind *k = kind_of(id);
    return k ? std::string(k->name) : "id " + std::to_string(id);
}

// one table entry against its kind, its size rule, its predecessor and the file size; nothing here can wrap
static void check_entry(const FileHead &h, size_t i, uint32_t want_id, uint64_t want_bytes, uint64_t want_offset) {
    const ImageSection &s = h.table[i];
    const std::string name = sec_name(want_id);
    auto bad = [&](const std::string &what) { throw Error(PGX_ERR_FORMAT, "image file: section " + name + ": " + what); };
    if (s.id != want_id) bad("the table holds id " + std::to_string(s.id) + " in its place");
    const SectionKind *k = kind_of(want_id);
    if (s.elem_size != k->elem) bad("element size " + std::to_string(s.elem_size) + ", expected " + std::to_string(k->elem));
    if (s.bytes % k->elem) bad("length " + std::to_string(s.bytes) + " is no multiple of the element size");
    if (s.bytes != want_bytes) bad("length " + std::to_string(s.bytes) + ", the constants imply " + (want_bytes == kNoSize ? std::string("more than any file holds") : std::to_string(want_bytes)));
    if (s.offset % PGX_IMAGE_ALIGN) bad("offset " + std::to_string(s.offset) + " is no multiple of " + std::to_string(PGX_IMAGE_ALIGN));
    if (s.offset != want_offset) bad("offset " + std::to_string(s.offset) + ", the sections before it end at " + std::to_string(want_offset));
    if (s.offset > h.file_bytes || s.bytes > h.file_bytes - s.offset)
        bad("offset " + std::to_string(s.offset) + " + length " + std::to_string(s.bytes) + " exceeds the file (" + std::to_string(h.file_bytes) + " bytes: truncated?)");
}

// a large section is read by a few threads side by side (the page cache, or several queues of the disk)
static void read_section(int fd, void *dst, const ImageSection &s) {
    const uint64_t piece = 64ull << 20;
    const unsigned nt = (unsigned)std::min<uint64_t>(std::max(1u, std::min(8u, std::thread::hardware_concurrency() / 2)), s.bytes / piece + 1);
    const std::string name = "section " + sec_name(s.id);
    if (nt <= 1) { pread_all(fd, dst, s.bytes, s.offset, name.c_str()); return; }
    std::vector<std::thread> th;
    std::vector<std::string> err(nt);
    std::vector<int> code(nt, 0);
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&, t]() {
            const uint64_t a = s.bytes * t / nt, b = s.bytes * (t + 1) / nt;
            try { pread_all(fd, static_cast<uint8_t *>(dst) + a, b - a, s.offset + a, name.c_str()); }
            catch (const Error &e) { err[t] = e.what(); code[t] = (int)e.code; }
        });
    for (auto &x : th) x.join();
    for (unsigned t = 0; t < nt; t++) if (code[t]) throw Error((pgx_status)code[t], err[t]);
}

// where section `id` of a handle lives: its address and, for the writer, its length
struct SecMem { void *p; uint64_t bytes; };
template <class T> static SecMem vec_mem(std::vector<T> &v, uint64_t resize_to) {
    if (resize_to != kNoSize) v.resize((size_t)(resize_to / sizeof(T)));
    return SecMem{v.data(), (uint64_t)v.size() * sizeof(T)};
}
struct LitTabs { uint32_t code_of[256], cslot_of[256]; uint64_t C[8]; };
static_assert(sizeof(LitTabs) == 2112, "literal tables section");

// resize_to: kNoSize = leave the buffer as it is (writer), else the checked length of the section (reader)
static SecMem section_mem(pgx_index *h, uint32_t id, uint64_t resize_to, LitTabs &tabs) {
    HostImage &m = h->img; LocHostImage &l = h->loc; LitHostImage &q = h->lit;
    switch (id) {
    case PGX_IMAGE_SEC_CONSTS: return SecMem{&m.consts, sizeof(PgxConsts)};
    case PGX_IMAGE_SEC_BLOCKS: return vec_mem(m.blocks, resize_to);
    case PGX_IMAGE_SEC_DIR: return vec_mem(m.dir, resize_to);
    case PGX_IMAGE_SEC_BSTART: return vec_mem(m.bstart, resize_to);
    case PGX_IMAGE_SEC_BLOW: return vec_mem(m.blow, resize_to);
    case PGX_IMAGE_SEC_EXC: return vec_mem(m.exc, resize_to);
    case PGX_IMAGE_SEC_PAIRS: return vec_mem(m.pairs, resize_to);
    case PGX_IMAGE_SEC_SBASE2: return vec_mem(m.sbase2, resize_to);
    case PGX_IMAGE_SEC_PBASE: return vec_mem(m.pbase, resize_to);
    case PGX_IMAGE_SEC_TSTART: return vec_mem(m.tstart, resize_to);
    case PGX_IMAGE_SEC_TVALS: return vec_mem(m.tvals, resize_to);
    case PGX_IMAGE_SEC_TDIR: return vec_mem(m.tdir, resize_to);
    case PGX_IMAGE_SEC_N_RUNS: return SecMem{&m.n_runs, 8};
    case PGX_IMAGE_SEC_LOC_CONSTS: return SecMem{&l.consts, sizeof(PgxLocConsts)};
    case PGX_IMAGE_SEC_RSTART: return vec_mem(l.rstart, resize_to);
    case PGX_IMAGE_SEC_RSAMP: return vec_mem(l.rsamp, resize_to);
    case PGX_IMAGE_SEC_RDIR: return vec_mem(l.rdir, resize_to);
    case PGX_IMAGE_SEC_LPOS: return vec_mem(l.lpos, resize_to);
    case PGX_IMAGE_SEC_LNEXT: return vec_mem(l.lnext, resize_to);
    case PGX_IMAGE_SEC_LDIR: return vec_mem(l.ldir, resize_to);
    case PGX_IMAGE_SEC_LIT_BSTART: return vec_mem(q.bstart, resize_to);
    case PGX_IMAGE_SEC_LIT_CUM: return vec_mem(q.cum, resize_to);
    case PGX_IMAGE_SEC_LIT_RUNS: return vec_mem(q.runs, resize_to);
    case PGX_IMAGE_SEC_LIT_ROFF: return vec_mem(q.roff, resize_to);
    case PGX_IMAGE_SEC_LIT_TABS: return SecMem{&tabs, sizeof(LitTabs)};
    default: break;
    }
    throw Error(PGX_ERR_FORMAT, "image file: unknown section id " + std::to_string(id));
}

// the whole table against the constants (read on the way: consts and loc_consts are sections themselves)
static void check_and_load(int fd, FileHead &fh, pgx_index *h, bool verify) {
    if (fh.mode > PGX_MODE_STRICT || fh.has_rank > 1 || fh.has_tags > 1 || (fh.flags & ~(PGX_IMAGE_HAS_LOCATE | PGX_IMAGE_HAS_LITERAL)) || (!fh.has_rank && (!fh.has_tags || fh.flags)))
        throw Error(PGX_ERR_FORMAT, "image file: header fields out of range (mode, has_rank, has_tags or flags)");
    const IndexMeta &mt = fh.meta;
    if (mt.sigma > 6 || mt.encoded > 1 || mt.hasN > 1 || (fh.has_rank && mt.sigma < 2)) throw Error(PGX_ERR_FORMAT, "image file: meta record out of range");
    const bool lit_expected = fh.has_rank && fh.mode == PGX_MODE_COMPAT && mt.encoded && !mt.hasN;
    if (lit_expected != ((fh.flags & PGX_IMAGE_HAS_LITERAL) != 0)) throw Error(PGX_ERR_FORMAT, "image file: the literal count image is stored exactly for COMPAT handles of encoded indexes without N");
    const std::vector<uint32_t> ids = expected_ids(fh.flags);
    if (ids.size() != fh.n_sections)
        throw Error(PGX_ERR_FORMAT, "image file: " + std::to_string(fh.n_sections) + " sections, a file of this shape has " + std::to_string(ids.size()));
    const uint64_t head_bytes = PGX_IMAGE_HEADER_BYTES + (uint64_t)PGX_IMAGE_ENTRY_BYTES * fh.n_sections + PGX_IMAGE_META_BYTES;
    LitTabs tabs;
    const bool has_rank = fh.has_rank != 0, has_tags = fh.has_tags != 0;
    // one pass in file order: an entry is checked against the length its constants imply and against the offset at which the
    // sections before it end; the two constant records are read as soon as their own entries have passed
    PgxConsts &c = h->img.consts;
    PgxLocConsts &lc = h->loc.consts;
    uint64_t want_offset = head_bytes;
    for (size_t i = 0; i < ids.size(); i++) {
        want_offset = (want_offset + PGX_IMAGE_ALIGN - 1) / PGX_IMAGE_ALIGN * PGX_IMAGE_ALIGN; // (below the file size, checked: cannot wrap)
        check_entry(fh, i, ids[i], section_rule(ids[i], c, &lc, has_rank, has_tags, (fh.flags & PGX_IMAGE_HAS_LITERAL) != 0, fh.counts), want_offset);
        if (ids[i] == PGX_IMAGE_SEC_CONSTS) {
            pread_all(fd, &c, sizeof(PgxConsts), fh.table[i].offset, "section consts");
            if (has_rank && (c.n != mt.sequence_size || c.mode != fh.mode || c.sigma != mt.sigma)) throw Error(PGX_ERR_FORMAT, "image file: section consts: disagrees with the header and the meta record");
            if ((c.has_tags != 0) != has_tags) throw Error(PGX_ERR_FORMAT, "image file: section consts: has_tags disagrees with the header");
        } else if (ids[i] == PGX_IMAGE_SEC_LOC_CONSTS) {
            pread_all(fd, &lc, sizeof(PgxLocConsts), fh.table[i].offset, "section loc_consts");
            if (lc.n != c.n || lc.n_runs != mt.n_samples) throw Error(PGX_ERR_FORMAT, "image file: section loc_consts: disagrees with the constants and the meta record");
        }
        want_offset = fh.table[i].offset + fh.table[i].bytes;
    }
    // every entry has passed: allocate by the checked lengths and read each section into its final buffer
    for (size_t i = 0; i < ids.size(); i++) {
        const ImageSection &s = fh.table[i];
        SecMem mem = section_mem(h, s.id, s.bytes, tabs);
        if (s.bytes) read_section(fd, mem.p, s);
        if (verify) {
            const uint64_t got = image_sum_host(mem.p, s.bytes);
            if (got != s.sum) throw Error(PGX_ERR_FORMAT, "image file: section " + sec_name(s.id) + ": the sum of its bytes does not match the table (damaged file)");
        }
    }
    if (fh.flags & PGX_IMAGE_HAS_LOCATE) h->loc.built = true;
    if (fh.flags & PGX_IMAGE_HAS_LITERAL) {
        std::memcpy(h->lit.code_of, tabs.code_of, 1024); std::memcpy(h->lit.cslot_of, tabs.cslot_of, 1024); std::memcpy(h->lit.C, tabs.C, 64);
        h->lit.built = true;
    }
}

} // namespace pgx

// ------------------------------------------------------------------------------------------
using namespace pgx;

#define PGX_GUARD_BEGIN try {
#define PGX_GUARD_END                                                    \
    }                                                                    \
    catch (const pgx::Error &e) { pgx::set_last_error(e.what()); return e.code; } \
    catch (const std::bad_alloc &) { pgx::set_last_error("out of host memory"); return PGX_ERR_NOMEM; } \
    catch (const std::exception &e) { pgx::set_last_error(e.what()); return PGX_ERR_FORMAT; }

extern "C" const char *pgx_image_section_name(uint32_t id) {
    const SectionKind *k = kind_of(id);
    return k ? k->name : "?";
}

extern "C" pgx_status pgx_index_save_image(pgx_index *h, const char *path, uint32_t flags) {
    PGX_GUARD_BEGIN
    if (!h || !path) throw Error(PGX_ERR_ARG, "pgx_index_save_image: null argument");
    if (flags & ~PGX_IMAGE_NO_LOCATE) throw Error(PGX_ERR_ARG, "pgx_index_save_image: unknown flag");
    uint32_t fflags = 0;
    if (h->has_rank && !(flags & PGX_IMAGE_NO_LOCATE)) { ensure_locate_host(h); fflags |= PGX_IMAGE_HAS_LOCATE; }
    if (h->has_rank && literal_count(h)) { ensure_literal_host(h); fflags |= PGX_IMAGE_HAS_LITERAL; }
    LitTabs tabs;
    std::memset(&tabs, 0, sizeof tabs);
    if (fflags & PGX_IMAGE_HAS_LITERAL) { std::memcpy(tabs.code_of, h->lit.code_of, 1024); std::memcpy(tabs.cslot_of, h->lit.cslot_of, 1024); std::memcpy(tabs.C, h->lit.C, 64); }
    FreeCounts fc;
    fc.tag_items = h->img.tvals.size(); fc.exc = h->img.exc.size();
    if (fflags & PGX_IMAGE_HAS_LITERAL) { fc.lit_blocks = h->lit.bstart.size(); fc.lit_runs = h->lit.runs.size(); }
    const std::vector<uint32_t> ids = expected_ids(fflags);
    const uint64_t head_bytes = PGX_IMAGE_HEADER_BYTES + (uint64_t)PGX_IMAGE_ENTRY_BYTES * ids.size() + PGX_IMAGE_META_BYTES;
    std::vector<ImageSection> table(ids.size());
    std::vector<SecMem> mems(ids.size());
    uint64_t at = head_bytes, end = head_bytes;
    for (size_t i = 0; i < ids.size(); i++) {
        mems[i] = section_mem(h, ids[i], kNoSize, tabs);
        // what is written must be what the reader will accept (section_rule is the one statement of the sizes)
        const uint64_t want = section_rule(ids[i], h->img.consts, &h->loc.consts, h->has_rank, h->has_tags, (fflags & PGX_IMAGE_HAS_LITERAL) != 0, fc);
        if (mems[i].bytes != want)
            throw Error(PGX_ERR_UNSUPPORTED, "pgx_index_save_image: section " + sec_name(ids[i]) + " holds " + std::to_string(mems[i].bytes) + " bytes, its constants imply " + std::to_string(want));
        at = (at + PGX_IMAGE_ALIGN - 1) / PGX_IMAGE_ALIGN * PGX_IMAGE_ALIGN;
        table[i].id = ids[i]; table[i].elem_size = kind_of(ids[i])->elem; table[i].bytes = mems[i].bytes; table[i].offset = at;
        table[i].sum = image_sum_host(mems[i].p, mems[i].bytes);
        at += mems[i].bytes;
        end = at;
    }
    std::vector<uint8_t> head((size_t)head_bytes, 0);
    std::memcpy(head.data(), PGX_IMAGE_MAGIC, 8);
    put<uint32_t>(head, 8, PGX_IMAGE_FILE_VERSION); put<uint32_t>(head, 12, PGX_IMAGE_LAYOUT);
    put<uint32_t>(head, 16, (uint32_t)sizeof(PgxConsts)); put<uint32_t>(head, 20, (uint32_t)sizeof(PgxLocConsts));
    put<uint32_t>(head, 24, h->mode & PGX_MODE_MASK); put<uint32_t>(head, 28, h->has_rank ? 1u : 0u); put<uint32_t>(head, 32, h->has_tags ? 1u : 0u);
    put<uint32_t>(head, 36, (uint32_t)ids.size()); put<uint32_t>(head, 40, PGX_IMAGE_META_BYTES); put<uint32_t>(head, 44, fflags);
    for (size_t i = 0; i < ids.size(); i++) {
        const size_t e = PGX_IMAGE_HEADER_BYTES + (size_t)PGX_IMAGE_ENTRY_BYTES * i;
        put<uint32_t>(head, e, table[i].id); put<uint32_t>(head, e + 4, table[i].elem_size);
        put<uint64_t>(head, e + 8, table[i].bytes); put<uint64_t>(head, e + 16, table[i].offset); put<uint64_t>(head, e + 24, table[i].sum);
    }
    meta_to_bytes(h->meta, fc, head.data() + PGX_IMAGE_HEADER_BYTES + (size_t)PGX_IMAGE_ENTRY_BYTES * ids.size());
    put<uint64_t>(head, 48, head_sum(head));
    // a temporary name next to the target, unique per call; renamed when complete
    static std::atomic<unsigned> save_serial{0};
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long)::getpid()) + "." + std::to_string(save_serial.fetch_add(1));
    Fd f;
    f.fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (f.fd < 0) throw Error(PGX_ERR_IO, "pgx_index_save_image: cannot create " + tmp + ": " + std::strerror(errno));
    auto pwrite_all = [&](const void *src, uint64_t bytes, uint64_t off) {
        const uint8_t *p = static_cast<const uint8_t *>(src);
        while (bytes) {
            const ssize_t k = ::pwrite(f.fd, p, (size_t)std::min<uint64_t>(bytes, 1u << 30), (off_t)off);
            if (k < 0 && errno == EINTR) continue;
            if (k <= 0) throw Error(PGX_ERR_IO, "pgx_index_save_image: write to " + tmp + " failed: " + std::strerror(errno));
            p += k; off += (uint64_t)k; bytes -= (uint64_t)k;
        }
    };
    try {
        if (::ftruncate(f.fd, (off_t)end) != 0) throw Error(PGX_ERR_IO, "pgx_index_save_image: cannot size " + tmp + ": " + std::strerror(errno)); // (the gaps read as zeros)
        pwrite_all(head.data(), head_bytes, 0);
        for (size_t i = 0; i < ids.size(); i++) pwrite_all(mems[i].p, mems[i].bytes, table[i].offset);
        if (::close(f.fd) != 0) { f.fd = -1; throw Error(PGX_ERR_IO, "pgx_index_save_image: closing " + tmp + " failed: " + std::strerror(errno)); }
        f.fd = -1;
        if (::rename(tmp.c_str(), path) != 0) throw Error(PGX_ERR_IO, std::string("pgx_index_save_image: cannot rename to ") + path + ": " + std::strerror(errno));
    } catch (...) { (void)::unlink(tmp.c_str()); throw; }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_index_open_image(const char *path, uint32_t flags, pgx_index **out) {
    PGX_GUARD_BEGIN
    if (!path || !out) throw Error(PGX_ERR_ARG, "pgx_index_open_image: null argument");
    *out = nullptr;
    if (flags & ~PGX_IMAGE_VERIFY) throw Error(PGX_ERR_ARG, "pgx_index_open_image: unknown flag");
    Fd f;
    f.fd = ::open(path, O_RDONLY);
    if (f.fd < 0) throw Error(PGX_ERR_IO, std::string("Cannot open image file: ") + path);
    FileHead fh;
    read_head(f.fd, path, fh);
    std::unique_ptr<pgx_index> h(new pgx_index());
    std::memset(&h->img.consts, 0, sizeof h->img.consts);
    std::memset(&h->loc.consts, 0, sizeof h->loc.consts);
    h->from_image = true;
    h->mode = fh.mode;
    h->has_rank = fh.has_rank != 0;
    h->has_tags = fh.has_tags != 0;
    h->meta = fh.meta;
    check_and_load(f.fd, fh, h.get(), (flags & PGX_IMAGE_VERIFY) != 0);
    h->sections = fh.table;
    *out = h.release();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_image_file_info(const char *path, pgx_image_info *out) {
    PGX_GUARD_BEGIN
    if (!path || !out) throw Error(PGX_ERR_ARG, "pgx_image_file_info: null argument");
    std::memset(out, 0, sizeof *out);
    Fd f;
    f.fd = ::open(path, O_RDONLY);
    if (f.fd < 0) throw Error(PGX_ERR_IO, std::string("Cannot open image file: ") + path);
    FileHead fh;
    read_head(f.fd, path, fh);
    out->version = fh.version; out->layout = fh.layout; out->consts_bytes = fh.consts_bytes; out->loc_consts_bytes = fh.loc_consts_bytes;
    out->mode = fh.mode; out->has_rank = fh.has_rank; out->has_tags = fh.has_tags; out->n_sections = fh.n_sections; out->meta_bytes = fh.meta_bytes;
    out->flags = fh.flags; out->header_sum = fh.header_sum; out->file_bytes = fh.file_bytes;
    for (uint32_t i = 0; i < fh.n_sections; i++) {
        pgx_image_section_info &s = out->sections[i];
        s.id = fh.table[i].id; s.elem_size = fh.table[i].elem_size; s.bytes = fh.table[i].bytes; s.offset = fh.table[i].offset; s.sum = fh.table[i].sum;
        std::snprintf(s.name, sizeof s.name, "%s", pgx_image_section_name(s.id));
    }
    return PGX_OK;
    PGX_GUARD_END
}
