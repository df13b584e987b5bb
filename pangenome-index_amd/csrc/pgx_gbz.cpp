// pgx_gbz.cpp -- the parts of a GBZ file that merge_tags (src/merge_tags.cpp:443-512) and build_tags need: the GBWT's node
// records and, for build_tags, the GBWTGraph's node sequences.
//
// The reference loads the whole GBZ (gbwtgraph::GBZ, simple-sds serialization) and asks it two things:
//   * gbz.index.extract(i)[0]                     the first node of path i            (merge_tags.cpp:508-515)
//   * gbwtgraph::weakly_connected_components       node id -> component               (algorithm.hpp:600-619)
// Both come out of the GBWT's compressed records alone (jltsiren/gbwt, not present under /root/reference; restated from its
// published file format, anchored on the reference's fixtures test_data/**/*.gbz: every path walked through the records
// ends at the endmarker after exactly header.size steps and the reverse paths mirror the forward ones, tests/test_gbz.py):
//   GBZ    = header {u32 tag "GBZ ", u32 version, u64 flags}, tags (StringArray), GBWT, GBWTGraph
//   GBWT   = header {u32 tag 0x6B376B37, u32 version, u64 sequences, size, offset, alphabet_size, flags}, tags (StringArray),
//            RecordArray {SparseVector of record starts, byte vector}, document array samples (option: bit vector, two sparse
//            vectors, int vector), metadata (option, body opens with u32 tag 0x6B375E7A)
//   GBWTGraph = header {u32 tag 0x6B3764AF, u32 version 3, u64 nodes, u64 flags}, node sequences (StringArray indexed by
//            id - first_id, first_id = (GBWT offset + 1) / 2; empty for ids that do not occur), ... (not read)
//   record = ByteCode outdegree; outdegree x (ByteCode node delta, ByteCode offset); runs of (edge rank, length) in
//            gbwt::Run coding: sigma >= 255: two ByteCodes (rank, length - 1); otherwise one byte = rank + sigma * (length - 1),
//            continued by a ByteCode when the basic length reaches 256 / sigma
//   simple-sds: every field padded to 8 bytes; vector = u64 count + items; bit vector = u64 ones, u64 bit length, word vector,
//            three optional supports (u64 size in words + body); int vector = u64 count, u64 width, u64 bit length, word vector;
//            sparse vector = u64 universe, high bit vector, low int vector; string array = sparse vector of starts, byte
//            vector alphabet, int vector of character codes; option = u64 size in words + body
// Host only.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <numeric>
#include <thread>

#include "pgx_host.hpp"

using namespace pgx;

#define PGX_GUARD_BEGIN try {
#define PGX_GUARD_END                                                                               \
    }                                                                                               \
    catch (const pgx::Error &e) { pgx::set_last_error(e.what()); return e.code; }                   \
    catch (const std::bad_alloc &) { pgx::set_last_error("out of host memory"); return PGX_ERR_NOMEM; } \
    catch (const std::exception &e) { pgx::set_last_error(e.what()); return PGX_ERR_FORMAT; }

namespace {
struct Sds {
    const uint8_t *p;
    uint64_t n, o = 0;
    uint64_t u64(const char *what) {
        if (o + 8 > n) throw Error(PGX_ERR_FORMAT, std::string("GBZ: truncated file while reading ") + what);
        uint64_t v;
        std::memcpy(&v, p + o, 8);
        o += 8;
        return v;
    }
    void skip_words(uint64_t w, const char *what) {
        if (w > (n - o) / 8) throw Error(PGX_ERR_FORMAT, std::string("GBZ: truncated file while skipping ") + what);
        o += 8 * w;
    }
    std::vector<uint64_t> words(const char *what) {
        const uint64_t k = u64(what);
        if (k > (n - o) / 8) throw Error(PGX_ERR_FORMAT, std::string("GBZ: word vector longer than the file in ") + what);
        std::vector<uint64_t> v(k);
        if (k) std::memcpy(v.data(), p + o, 8 * k);
        o += 8 * k;
        return v;
    }
    // byte vector: returns the span, advances over the padding
    std::pair<const uint8_t *, uint64_t> bytes(const char *what) {
        const uint64_t k = u64(what);
        const uint64_t padded = (k + 7) / 8 * 8;
        if (padded > n - o) throw Error(PGX_ERR_FORMAT, std::string("GBZ: byte vector longer than the file in ") + what);
        const uint8_t *b = p + o;
        o += padded;
        return {b, k};
    }
    // sparse vector -> ascending positions of its ones
    std::vector<uint64_t> sparse(uint64_t &universe, const char *what) {
        universe = u64(what);
        const uint64_t ones = u64(what), hbits = u64(what);
        const std::vector<uint64_t> high = words(what);
        if (hbits > high.size() * 64) throw Error(PGX_ERR_FORMAT, std::string("GBZ: bad high part in ") + what);
        for (int i = 0; i < 3; i++) skip_words(u64(what), what); // rank / select / select_zero supports
        const uint64_t ln = u64(what), lw = u64(what), lbits = u64(what);
        const std::vector<uint64_t> low = words(what);
        if (ln != ones || lw > 64 || lbits != ln * lw || lbits > low.size() * 64) throw Error(PGX_ERR_FORMAT, std::string("GBZ: bad low part in ") + what);
        std::vector<uint64_t> out;
        out.reserve(ones);
        uint64_t zeros = 0;
        for (uint64_t pos = 0; pos < hbits; pos++) {
            if ((high[pos >> 6] >> (pos & 63)) & 1) {
                const uint64_t k = out.size();
                if (k >= ones) throw Error(PGX_ERR_FORMAT, std::string("GBZ: more ones than declared in ") + what);
                uint64_t lv = 0;
                if (lw) {
                    const uint64_t bit = k * lw, wd = bit >> 6, sh = bit & 63;
                    lv = low[wd] >> sh;
                    if (sh + lw > 64) lv |= low[wd + 1] << (64 - sh);
                    if (lw < 64) lv &= (1ull << lw) - 1;
                }
                out.push_back((zeros << lw) | lv);
            } else zeros++;
        }
        if (out.size() != ones) throw Error(PGX_ERR_FORMAT, std::string("GBZ: fewer ones than declared in ") + what);
        return out;
    }
    void skip_string_array(const char *what) {
        uint64_t uni;
        (void)sparse(uni, what);
        (void)bytes(what);                                  // alphabet
        (void)u64(what); (void)u64(what); (void)u64(what);  // int vector: count, width, bit length
        (void)words(what);
    }
};

inline uint64_t bc(const uint8_t *d, uint64_t end, uint64_t &o) { // gbwt::ByteCode
    uint64_t v = 0, sh = 0;
    for (;;) {
        if (o >= end || sh > 63) throw Error(PGX_ERR_FORMAT, "GBZ: bad ByteCode value in a GBWT record");
        const uint8_t b = d[o++];
        v |= (uint64_t)(b & 0x7F) << sh;
        if (!(b & 0x80)) return v;
        sh += 7;
    }
}

// the GBZ header and the GBWT up to and including its record array
struct GbwtHead {
    uint64_t n_seq = 0, size = 0, offset = 0, sigma = 0, flags = 0;
    std::vector<uint64_t> starts;                // record r starts at byte starts[r] of the record bytes
    std::pair<const uint8_t *, uint64_t> data;   // record bytes
};
void read_gbwt_head(Sds &s, GbwtHead &h) {
    const uint64_t tagver = s.u64("GBZ header");
    if ((uint32_t)tagver != 0x205A4247u) throw Error(PGX_ERR_FORMAT, "GBZ: invalid tag (not a GBZ file)");
    (void)s.u64("GBZ flags");
    s.skip_string_array("GBZ tags");
    const uint64_t gtag = s.u64("GBWT header");
    if ((uint32_t)gtag != 0x6B376B37u) throw Error(PGX_ERR_FORMAT, "GBZ: GBWT tag not found where the simple-sds layout puts it");
    h.n_seq = s.u64("GBWT sequences");
    h.size = s.u64("GBWT size");
    h.offset = s.u64("GBWT offset");
    h.sigma = s.u64("GBWT alphabet size");
    h.flags = s.u64("GBWT flags");
    s.skip_string_array("GBWT tags");
    uint64_t universe = 0;
    h.starts = s.sparse(universe, "GBWT record index");
    h.data = s.bytes("GBWT records");
    if (universe != h.data.second || h.sigma < h.offset || h.starts.size() != h.sigma - h.offset || h.starts.empty())
        throw Error(PGX_ERR_FORMAT, "GBZ: GBWT record index does not match its header");
}
} // namespace

namespace pgx {
void parse_gbz_paths(const std::string &path, GbzPaths &g) {
    const std::vector<uint8_t> file = read_whole_file(path);
    Sds s{file.data(), file.size()};
    GbwtHead h;
    read_gbwt_head(s, h);
    const uint64_t n_seq = h.n_seq, offset = h.offset, sigma = h.sigma;
    const std::vector<uint64_t> &starts = h.starts;
    const auto &data = h.data;
    const uint8_t *d = data.first;
    const uint64_t n_rec = starts.size();
    const uint64_t max_node_id = (sigma - 1) / 2; // GBWT node = 2 * id + orientation
    // union-find over graph node ids; edges = the outgoing edges of every record (what GBWTGraph::follow_edges follows)
    std::vector<uint64_t> parent(max_node_id + 1);
    std::iota(parent.begin(), parent.end(), 0);
    std::vector<uint8_t> present(max_node_id + 1, 0);
    auto find = [&](uint64_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    g.first_node.assign(n_seq, 0);
    for (uint64_t r = 0; r < n_rec; r++) {
        uint64_t o = starts[r];
        const uint64_t end = r + 1 < n_rec ? starts[r + 1] : data.second;
        if (o > end || end > data.second) throw Error(PGX_ERR_FORMAT, "GBZ: GBWT record offsets not monotone");
        if (o == end) continue; // node without a record
        const uint64_t node = r == 0 ? 0 : r + offset; // record 0 is the endmarker
        const uint64_t outdeg = bc(d, end, o);
        std::vector<uint64_t> succ(outdeg);
        uint64_t prev = 0;
        for (uint64_t e = 0; e < outdeg; e++) {
            prev += bc(d, end, o);
            (void)bc(d, end, o); // offset in the successor's record
            succ[e] = prev;
            if (prev > 2 * max_node_id + 1) throw Error(PGX_ERR_FORMAT, "GBZ: edge to a node beyond the alphabet");
        }
        if (node) {
            if (outdeg == 0 && o >= end) continue; // a record without edges or visits: no path uses the node, GBWTGraph does not have it
            present[node / 2] = 1;
            for (uint64_t t : succ)
                if (t) { present[t / 2] = 1; const uint64_t a = find(node / 2), b = find(t / 2); if (a != b) parent[std::max(a, b)] = std::min(a, b); }
            continue;
        }
        // endmarker record: position i of its body = the first node of sequence i
        const uint64_t rc = (outdeg && outdeg < 255) ? 256 / outdeg : 0;
        uint64_t seq = 0;
        while (o < end && seq < n_seq) {
            uint64_t rank, len;
            if (rc == 0) { rank = bc(d, end, o); len = bc(d, end, o) + 1; }
            else {
                const uint8_t code = d[o++];
                rank = code % outdeg; len = code / outdeg + 1;
                if (len >= rc) len += bc(d, end, o);
            }
            if (rank >= outdeg) throw Error(PGX_ERR_FORMAT, "GBZ: run of an edge the endmarker does not have");
            for (uint64_t k = 0; k < len && seq < n_seq; k++) g.first_node[seq++] = succ[rank] / 2; // 0 for an empty path
        }
        if (seq != n_seq) throw Error(PGX_ERR_FORMAT, "GBZ: the endmarker record is shorter than the number of sequences");
    }
    // components numbered by their smallest node id (gbwtgraph::weakly_connected_components order)
    g.component_of_node.assign(max_node_id + 1, ~0u);
    uint32_t n_comp = 0;
    for (uint64_t v = 1; v <= max_node_id; v++) {
        if (!present[v]) continue;
        const uint64_t root = find(v);
        if (g.component_of_node[root] == ~0u) g.component_of_node[root] = n_comp++; // root = smallest id of its component: met first
        g.component_of_node[v] = g.component_of_node[root];
    }
    g.n_components = n_comp;
    g.max_node_id = 0;
    for (uint64_t v = max_node_id; v >= 1; v--) if (present[v]) { g.max_node_id = v; break; }
}
} // namespace pgx

extern "C" pgx_status pgx_gbz_paths(const char *gbz_path, uint64_t *n_sequences, uint64_t *first_node, uint32_t *component, uint64_t cap,
                                    uint64_t *max_node_id, uint32_t *n_components) {
    PGX_GUARD_BEGIN
    if (!gbz_path || !n_sequences) throw Error(PGX_ERR_ARG, "pgx_gbz_paths: null argument");
    GbzPaths g;
    parse_gbz_paths(gbz_path, g);
    *n_sequences = g.first_node.size();
    if (max_node_id) *max_node_id = g.max_node_id;
    if (n_components) *n_components = g.n_components;
    for (uint64_t i = 0; i < g.first_node.size() && i < cap; i++) {
        if (first_node) first_node[i] = g.first_node[i];
        if (component) component[i] = g.first_node[i] ? g.component_of_node[g.first_node[i]] : ~0u;
    }
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// build_tags: the graph's node sequences and every path as its node list
namespace {
// host threads for the path walks: at most 16, PGX_BUILD_THREADS overrides (1..16)
unsigned graph_threads(uint64_t work) {
    unsigned T = std::max(1u, std::min<unsigned>(std::thread::hardware_concurrency(), 16u));
    if (const char *e = std::getenv("PGX_BUILD_THREADS")) T = (unsigned)std::max<long>(1, std::min<long>(std::atol(e), 16));
    return (unsigned)std::min<uint64_t>(T, std::max<uint64_t>(work, 1));
}

// runs t in [0, T) on T threads; the first exception is rethrown after all have joined
template <class F> void run_threads(unsigned T, F &&fn) {
    std::vector<std::thread> th;
    std::exception_ptr err;
    std::mutex mu;
    auto body = [&](unsigned t) {
        try { fn(t); }
        catch (...) { std::lock_guard<std::mutex> g(mu); if (!err) err = std::current_exception(); }
    };
    try {
        for (unsigned t = 1; t < T; t++) th.emplace_back(body, t);
    } catch (...) {
        for (auto &x : th) x.join();
        throw;
    }
    body(0);
    for (auto &x : th) x.join();
    if (err) std::rethrow_exception(err);
}

// the records decoded once for LF: run k of record r covers record positions [run_start[k], run_start[k + 1]) (within the
// record) and maps them to (run_node[k], run_base[k] + position - run_start[k])
struct LfRecords {
    uint64_t offset = 0;
    std::vector<uint64_t> run_off, rec_size, run_start, run_node, run_base;
    void decode(const GbwtHead &h) {
        const uint8_t *d = h.data.first;
        const uint64_t n_rec = h.starts.size();
        offset = h.offset;
        run_off.assign(n_rec + 1, 0);
        rec_size.assign(n_rec, 0);
        std::vector<uint64_t> node, cnt;
        for (uint64_t r = 0; r < n_rec; r++) {
            uint64_t o = h.starts[r];
            const uint64_t end = r + 1 < n_rec ? h.starts[r + 1] : h.data.second;
            if (o > end || end > h.data.second) throw Error(PGX_ERR_FORMAT, "GBZ: GBWT record offsets not monotone");
            run_off[r] = run_start.size();
            if (o == end) continue;
            const uint64_t outdeg = bc(d, end, o);
            if (outdeg > end - o) throw Error(PGX_ERR_FORMAT, "GBZ: GBWT record with more edges than bytes");
            node.assign(outdeg, 0); cnt.assign(outdeg, 0);
            uint64_t prev = 0;
            for (uint64_t e = 0; e < outdeg; e++) {
                prev += bc(d, end, o);
                node[e] = prev;
                cnt[e] = bc(d, end, o);
                if (prev >= h.sigma) throw Error(PGX_ERR_FORMAT, "GBZ: edge to a node beyond the alphabet");
            }
            const uint64_t rc = (outdeg && outdeg < 255) ? 256 / outdeg : 0;
            uint64_t pos = 0;
            while (o < end) {
                uint64_t rank, len;
                if (rc == 0) { rank = bc(d, end, o); len = bc(d, end, o) + 1; }
                else {
                    const uint8_t code = d[o++];
                    rank = code % outdeg; len = code / outdeg + 1;
                    if (len >= rc) len += bc(d, end, o);
                }
                if (rank >= outdeg) throw Error(PGX_ERR_FORMAT, "GBZ: run of an edge the record does not have");
                run_start.push_back(pos); run_node.push_back(node[rank]); run_base.push_back(cnt[rank]);
                cnt[rank] += len; pos += len;
            }
            rec_size[r] = pos;
        }
        run_off[n_rec] = run_start.size();
    }
    // gbwt::GBWT::LF(node, i)
    void lf(uint64_t &node, uint64_t &i) const {
        if (node != 0 && (node <= offset || node - offset >= rec_size.size())) throw Error(PGX_ERR_FORMAT, "GBZ: path through a node without a record");
        const uint64_t r = node == 0 ? 0 : node - offset;
        if (i >= rec_size[r]) throw Error(PGX_ERR_FORMAT, "GBZ: path position beyond its record");
        uint64_t lo = run_off[r], hi = run_off[r + 1] - 1; // last run with run_start <= i
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (run_start[mid] <= i) lo = mid; else hi = mid - 1;
        }
        node = run_node[lo];
        i = run_base[lo] + (i - run_start[lo]);
    }
};
} // namespace

namespace pgx {
void parse_gbz_graph(const std::string &path, bool forward_only, bool with_sequences, GbzGraph &g) {
    const std::vector<uint8_t> file = read_whole_file(path);
    Sds s{file.data(), file.size()};
    GbwtHead h;
    read_gbwt_head(s, h);
    // document array samples: an option whose body is read through to check the layout
    {
        const uint64_t words = s.u64("GBWT document array samples");
        if (words > (s.n - s.o) / 8) throw Error(PGX_ERR_FORMAT, "GBZ: document array samples longer than the file");
        const uint64_t end = s.o + 8 * words;
        if (words) {
            Sds b{s.p, end, s.o};
            (void)b.u64("DA sampled records"); (void)b.u64("DA sampled records"); (void)b.words("DA sampled records");
            for (int i = 0; i < 3; i++) b.skip_words(b.u64("DA sampled records"), "DA sampled records");
            uint64_t uni;
            (void)b.sparse(uni, "DA BWT ranges");
            (void)b.sparse(uni, "DA sampled offsets");
            (void)b.u64("DA samples"); (void)b.u64("DA samples"); (void)b.u64("DA samples"); (void)b.words("DA samples");
            if (b.o != end) throw Error(PGX_ERR_FORMAT, "GBZ: document array samples do not fill their option");
        }
        s.o = end;
    }
    // metadata: an option
    {
        const uint64_t words = s.u64("GBWT metadata");
        if (words > (s.n - s.o) / 8) throw Error(PGX_ERR_FORMAT, "GBZ: metadata longer than the file");
        if (words && (uint32_t)Sds{s.p, s.n, s.o}.u64("GBWT metadata") != 0x6B375E7Au)
            throw Error(PGX_ERR_FORMAT, "GBZ: metadata tag not found where the simple-sds layout puts it");
        s.o += 8 * words;
    }
    const uint64_t gtag = s.u64("GBWTGraph header");
    if ((uint32_t)gtag != 0x6B3764AFu || (gtag >> 32) != 3)
        throw Error(PGX_ERR_FORMAT, "GBZ: GBWTGraph header (tag 0x6B3764AF, version 3) not found after the GBWT");
    (void)s.u64("GBWTGraph nodes"); (void)s.u64("GBWTGraph flags");
    uint64_t universe = 0;
    std::vector<uint64_t> starts = s.sparse(universe, "node sequences");
    const auto alpha = s.bytes("node sequence alphabet");
    const uint64_t n_chars = s.u64("node sequences"), width = s.u64("node sequences"), bits = s.u64("node sequences");
    const std::vector<uint64_t> codes = s.words("node sequences");
    if (width > 8 || bits != n_chars * width || bits > codes.size() * 64)
        throw Error(PGX_ERR_FORMAT, "GBZ: bad character codes in the node sequences");
    const uint64_t n_ids = starts.size();
    g.n_gbwt_seq = h.n_seq;
    g.first_node_id = (h.offset + 1) / 2;
    g.node_length.assign(n_ids, 0);
    for (uint64_t k = 0; k < n_ids; k++) {
        const uint64_t a = starts[k], b = k + 1 < n_ids ? starts[k + 1] : n_chars;
        if (b < a || b > n_chars) throw Error(PGX_ERR_FORMAT, "GBZ: node sequence offsets not monotone");
        if (b - a > 0xFFFFFFFFull) throw Error(PGX_ERR_FORMAT, "GBZ: node sequence longer than 2^32 bp");
        g.node_length[k] = (uint32_t)(b - a);
    }
    g.seq_start.clear(); g.chars.clear();
    if (with_sequences) {
        g.seq_start = starts;
        g.seq_start.push_back(n_chars);
        g.chars.resize(n_chars);
        for (uint64_t i = 0; i < n_chars; i++) {
            uint64_t c = 0;
            if (width) {
                const uint64_t bit = i * width, wd = bit >> 6, sh = bit & 63;
                c = codes[wd] >> sh;
                if (sh + width > 64) c |= codes[wd + 1] << (64 - sh);
                c &= (1ull << width) - 1;
            }
            if (c >= alpha.second) throw Error(PGX_ERR_FORMAT, "GBZ: node sequence character outside its alphabet");
            g.chars[i] = alpha.first[c];
        }
    }
    // paths: the sequences used are all of them, or the even ones (forward orientation); with a bidirectional GBWT
    // (header flag 0x1) sequence 2k + 1 is sequence 2k reversed with flipped orientations, so only even ones are walked
    LfRecords rec;
    rec.decode(h);
    const bool bidir = (h.flags & 1) && h.n_seq % 2 == 0;
    const uint64_t step = forward_only ? 2 : 1, n_used = (h.n_seq + step - 1) / step;
    std::vector<std::vector<uint64_t>> walks(n_used);
    const unsigned T = graph_threads(n_used);
    run_threads(T, [&](unsigned t) {
        for (uint64_t u = t; u < n_used; u += T) {
            const uint64_t sq = u * step;
            if (bidir && (sq & 1)) continue; // derived below
            std::vector<uint64_t> &w = walks[u];
            uint64_t node = 0, i = sq;
            rec.lf(node, i);
            while (node != 0) {
                if (w.size() >= h.size) throw Error(PGX_ERR_FORMAT, "GBZ: path " + std::to_string(sq) + " does not reach the endmarker");
                w.push_back(node);
                rec.lf(node, i);
            }
        }
    });
    if (bidir && step == 1)
        for (uint64_t sq = 1; sq < n_used; sq += 2) {
            const std::vector<uint64_t> &f = walks[sq - 1];
            walks[sq].assign(f.rbegin(), f.rend());
            for (uint64_t &v : walks[sq]) v ^= 1;
        }
    g.path_offsets.assign(n_used + 1, 0);
    for (uint64_t u = 0; u < n_used; u++) g.path_offsets[u + 1] = g.path_offsets[u] + walks[u].size();
    g.path_nodes.resize(g.path_offsets[n_used]);
    for (uint64_t u = 0; u < n_used; u++) {
        std::copy(walks[u].begin(), walks[u].end(), g.path_nodes.begin() + g.path_offsets[u]);
        for (uint64_t v : walks[u]) {
            const uint64_t id = v >> 1;
            if (id < g.first_node_id || id - g.first_node_id >= n_ids || g.node_length[id - g.first_node_id] == 0)
                throw Error(PGX_ERR_FORMAT, "GBZ: path " + std::to_string(u * step) + " visits node " + std::to_string(id) +
                                                ", which has no sequence in the graph");
        }
        std::vector<uint64_t>().swap(walks[u]);
    }
}
} // namespace pgx

extern "C" pgx_status pgx_gbz_extract(const char *gbz_path, const char *out_text_path, uint32_t flags) {
    PGX_GUARD_BEGIN
    if (!gbz_path || !out_text_path) throw Error(PGX_ERR_ARG, "pgx_gbz_extract: null argument");
    if (flags & ~PGX_BUILD_TAGS_FORWARD_ONLY) throw Error(PGX_ERR_ARG, "pgx_gbz_extract: unknown flag");
    GbzGraph g;
    parse_gbz_graph(gbz_path, (flags & PGX_BUILD_TAGS_FORWARD_ONLY) != 0, true, g);
    const uint64_t n_paths = g.path_offsets.size() - 1;
    // spelled in slices of paths by the host threads, written in order
    std::vector<std::string> text(n_paths);
    const unsigned T = graph_threads(n_paths);
    run_threads(T, [&](unsigned t) {
        for (uint64_t u = t; u < n_paths; u += T) {
            std::string &o = text[u];
            for (uint64_t k = g.path_offsets[u]; k < g.path_offsets[u + 1]; k++) {
                const uint64_t v = g.path_nodes[k], x = (v >> 1) - g.first_node_id;
                const uint8_t *a = g.chars.data() + g.seq_start[x], *b = g.chars.data() + g.seq_start[x + 1];
                if (!(v & 1)) { o.append(a, b); continue; }
                for (const uint8_t *c = b; c != a;) {
                    const uint8_t ch = *--c;
                    o.push_back(ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : (char)ch);
                }
            }
            o.push_back('\n');
        }
    });
    FILE *f = std::fopen(out_text_path, "wb");
    if (!f) throw Error(PGX_ERR_IO, std::string("Cannot create file: ") + out_text_path);
    for (const std::string &t : text)
        if (std::fwrite(t.data(), 1, t.size(), f) != t.size()) {
            std::fclose(f);
            throw Error(PGX_ERR_IO, std::string("Short write: ") + out_text_path);
        }
    if (std::fclose(f) != 0) throw Error(PGX_ERR_IO, std::string("Short write: ") + out_text_path);
    return PGX_OK;
    PGX_GUARD_END
}
