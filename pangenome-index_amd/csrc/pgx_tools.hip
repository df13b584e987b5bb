// pgx_tools.hip -- the offline tools behind the C ABI: merge_tags (per-chromosome tag streams -> one compact tag array) and build_tags
// (tag array from a graph's paths and the BWT).  Both need only the locate side of an index (locate_image, locate_core).
#include <chrono>
#include <memory>
#include <string>
#include <thread>

#include "pgx_runtime_internal.hpp"

// ------------------------------------------------------------------------------------------
// merge_tags (pgx_merge_kernels.hip)
// where the ByteCodes of a build_tags file start: 8 behind the int_vector<8> header of sdsl::int_vector_buffer<8> (u64 bit
// count of the body; the body is zero-padded to whole words, and a zero byte decodes as a run of length 0), else 0 (a bare stream)
static uint64_t algorithm_tags_start(const std::vector<uint8_t> &raw) {
    if (raw.size() < 8) return 0;
    uint64_t bits = 0;
    std::memcpy(&bits, raw.data(), 8);
    const uint64_t body = raw.size() - 8;
    if (bits == body * 8) return 8;
    return (bits % 8 == 0 && bits / 8 < body && (bits / 8 + 7) / 8 * 8 == body) ? 8 : 0; // padded
}

static void merge_tags_core(const char *ri_path, const char *const *tag_paths, uint32_t n_files, const uint32_t *seq_to_file, uint64_t n_seq,
                            int device, const char *out_path, uint64_t max_node_floor, uint32_t opts) {
    if (!ri_path || !tag_paths || !seq_to_file || !out_path) throw Error(PGX_ERR_ARG, "pgx_merge_tags: null argument");
    if (opts & ~(PGX_MERGE_REFERENCE_RUNS | PGX_MERGE_DEVICE_ENCODE)) throw Error(PGX_ERR_ARG, "pgx_merge_tags: unknown flag");
    if (n_files == 0 || n_files > 250) throw Error(PGX_ERR_ARG, "pgx_merge_tags: between 1 and 250 tag files");
    // only the locate side of the index is needed: parse the file, no rank image
    std::unique_ptr<pgx_index, void (*)(pgx_index *)> guard(new pgx_index(), pgx_index_close);
    pgx_index *h = guard.get();
    {
        std::vector<uint8_t> f;
        try { f = read_whole_file(ri_path); }
        catch (const Error &) { throw Error(PGX_ERR_IO, std::string("Cannot open r-index: ") + ri_path); }
        h->ri.parse(f.data(), f.size());
        std::memset(&h->img.consts, 0, sizeof h->img.consts);
        h->mode = PGX_MODE_STRICT;
        h->has_rank = true;
    }
    // the tag streams are parsed by host threads (one per file) while the device computes the document array
    struct Stream { std::vector<uint64_t> st, vl; std::string err; };
    std::vector<Stream> streams(n_files);
    std::vector<std::thread> parsers;
    for (uint32_t f = 0; f < n_files; f++)
        if (!tag_paths[f]) throw Error(PGX_ERR_ARG, "pgx_merge_tags: null tag path"); // before any thread exists
    // joins whatever was started, also when starting a later thread throws (a joinable std::thread must not be destroyed)
    struct Joiner { std::vector<std::thread> &t; ~Joiner() { for (auto &x : t) if (x.joinable()) x.join(); } } joiner{parsers};
    parsers.reserve(n_files);
    for (uint32_t f = 0; f < n_files; f++) {
        parsers.emplace_back([&streams, tag_paths, f]() {
            Stream &o = streams[f];
            try {
                std::vector<uint8_t> raw = read_whole_file(tag_paths[f]);
                uint64_t loc = algorithm_tags_start(raw); // merge_tags.cpp:207
                o.st.assign(1, 0);
                while (loc < raw.size()) {
                    const uint64_t v = bytecode_read(raw.data(), raw.size(), loc, "tag run");
                    const uint64_t len = (v >> 11) & 0x1FF; // decode_run, length_bits = 9 (src/tag_arrays.cpp:59-70)
                    if (!len) continue;
                    o.vl.push_back((v & 0x7FF) | ((v >> 20) << 11)); // offset | rev << 10 | node << 11
                    o.st.push_back(o.st.back() + len);
                }
            } catch (const std::exception &e) { o.err = e.what(); }
        });
    }
    const uint64_t n = h->ri.sequence_size, tot = h->ri.C.size() > 1 ? h->ri.C[1] - h->ri.C[0] : 0;
    if (n_seq != tot) throw Error(PGX_ERR_ARG, "pgx_merge_tags: seq_to_file has " + std::to_string(n_seq) + " entries, the index holds " +
                                                   std::to_string(tot) + " sequences");
    // every entry, also that of an empty sequence, which has no row behind the endmarker block for pgx_mt_file_of_kernel to see
    for (uint64_t sq = 0; sq < n_seq; sq++)
        if (seq_to_file[sq] >= n_files) throw Error(PGX_ERR_ARG, "pgx_merge_tags: seq_to_file names a file index >= n_files");
    pgx_device_image *d = locate_image(h, device);
    DevBuf da, file_of, tags, rank, scan_tmp, s2f, ctr, rstart, rval, expanded, flags, out_val, out_start;
    DevBuf *all[] = {&da, &file_of, &tags, &rank, &scan_tmp, &s2f, &ctr, &rstart, &rval, &expanded, &flags, &out_val, &out_start};
    std::vector<uint64_t> h_val, h_start;
    try {
        hipStream_t s = nullptr;
        // 1. document array of the whole BWT
        {
            const uint64_t first = 0, last = n ? n - 1 : 0;
            std::vector<uint64_t> off;
            uint64_t nv = 0;
            if (n) locate_core(h, d, &first, &last, 1, PGX_LOCATE_SEQ_IDS, off, da, nv);
        }
        // 2. file of every position
        file_of.ensure(n ? n : 1); tags.ensure((n ? n : 1) * 8); rank.ensure((n + 1) * 8); s2f.ensure((n_seq ? n_seq : 1) * 4); ctr.ensure(64);
        HIPCHECK(hipMemsetAsync(ctr.p, 0, 64, s));
        HIPCHECK(hipMemsetAsync(tags.p, 0, (n ? n : 1) * 8, s));
        if (n_seq) HIPCHECK(hipMemcpyAsync(s2f.p, seq_to_file, n_seq * 4, hipMemcpyHostToDevice, s));
        if (n) {
            hipLaunchKernelGGL(pgx_mt_file_of_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, da.as<uint64_t>(), n, n_seq, s2f.as<uint32_t>(), n_files,
                               file_of.as<uint8_t>(), ctr.as<unsigned long long>());
            HIPCHECK(hipGetLastError());
        }
        if (read_u64(ctr.as<uint64_t>(), s)) throw Error(PGX_ERR_ARG, "pgx_merge_tags: seq_to_file names a file index >= n_files");
        da.release();
        // 3. per file: expanded stream, rank of its positions, gather
        for (uint32_t f = 0; f < n_files; f++) {
            parsers[f].join();
            if (!streams[f].err.empty()) throw Error(PGX_ERR_FORMAT, std::string(tag_paths[f]) + ": " + streams[f].err);
            const std::vector<uint64_t> &st = streams[f].st, &vl = streams[f].vl;
            const uint64_t nr = vl.size(), total = st.back();
            scan_excl(3, file_of.p, n, f, rank.as<uint64_t>(), scan_tmp, s);
            const uint64_t have = read_u64(rank.as<uint64_t>() + n, s);
            if (have != total)
                throw Error(PGX_ERR_FORMAT, std::string("pgx_merge_tags: ") + tag_paths[f] + " holds " + std::to_string(total) + " tags, the BWT has " +
                                                std::to_string(have) + " positions of its sequences");
            if (!total) continue;
            rstart.ensure((nr + 1) * 8); rval.ensure(nr * 8); expanded.ensure(total * 8);
            HIPCHECK(hipMemcpyAsync(rstart.p, st.data(), (nr + 1) * 8, hipMemcpyHostToDevice, s));
            HIPCHECK(hipMemcpyAsync(rval.p, vl.data(), nr * 8, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(pgx_mt_expand_kernel, dim3(grid_for(nr, 256)), dim3(256), 0, s, rstart.as<uint64_t>(), rval.as<uint64_t>(), nr,
                               expanded.as<uint64_t>());
            hipLaunchKernelGGL(pgx_mt_gather_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, file_of.as<uint8_t>(), f, rank.as<uint64_t>(),
                               expanded.as<uint64_t>(), total, n, tags.as<uint64_t>());
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipStreamSynchronize(s)); // st / vl are host vectors read by the async copies
        }
        // 4. run-length encode
        uint64_t n_out = 0;
        if (n) {
            flags.ensure(n);
            hipLaunchKernelGGL(pgx_mt_flags_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, tags.as<uint64_t>(), n, n_seq, flags.as<uint8_t>());
            scan_excl(4, flags.p, n, 0, rank.as<uint64_t>(), scan_tmp, s);
            n_out = read_u64(rank.as<uint64_t>() + n, s);
            out_val.ensure(n_out * 8); out_start.ensure(n_out * 8);
            hipLaunchKernelGGL(pgx_mt_compact_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, tags.as<uint64_t>(), flags.as<uint8_t>(), rank.as<uint64_t>(),
                               n, n_seq, out_val.as<uint64_t>(), out_start.as<uint64_t>());
            HIPCHECK(hipGetLastError());
        }
        if (opts & PGX_MERGE_DEVICE_ENCODE) {
            // the file from (out_val, out_start) where they lie: lengths (next start - start, the last run ends at n; mod 65 536 in
            // reference mode, 0 = nothing written) come from the encoder's first kernel
            HIPCHECK(hipStreamSynchronize(s));
            DevBuf *done[] = {&file_of, &tags, &rank, &scan_tmp, &s2f, &ctr, &rstart, &rval, &expanded, &flags};
            for (DevBuf *b : done) b->release();
            const PgxTeRuns runs{out_val.as<uint64_t>(), out_start.as<uint64_t>(), n_out, n, 1u, (opts & PGX_MERGE_REFERENCE_RUNS) ? 1u : 0u};
            tags_encode_device(runs, false, max_node_floor, PGX_TAGS_COMPACT, out_path, s);
            for (DevBuf *b : all) b->release();
            return;
        }
        if (n) {
            h_val.resize(n_out); h_start.resize(n_out + 1);
            HIPCHECK(hipMemcpy(h_val.data(), out_val.p, n_out * 8, hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(h_start.data(), out_start.p, n_out * 8, hipMemcpyDeviceToHost));
            h_start[n_out] = n;
        }
        for (uint64_t i = 0; i < n_out; i++) h_start[i] = h_start[i + 1] - h_start[i]; // lengths
        if (opts & PGX_MERGE_REFERENCE_RUNS) {
            // the reference counts a merged run in a uint16_t (std::pair<pos_t, uint16_t>, src/merge_tags.cpp:282,346,394-398,625) and
            // adds the pieces of a run that crosses a 500-run job in the same type (:776-777): what reaches
            // append_compact_run_streamed is the maximal run's length mod 65 536, and a length of 0 writes nothing (tag_arrays.cpp:959)
            uint64_t w = 0;
            for (uint64_t i = 0; i < n_out; i++) {
                const uint64_t l16 = h_start[i] & 0xFFFFull;
                if (!l16) continue;
                h_val[w] = h_val[i]; h_start[w++] = l16;
            }
            h_val.resize(w); h_start.resize(w + 1);
        }
    } catch (...) {
        for (DevBuf *b : all) b->release();
        throw;
    }
    for (DevBuf *b : all) b->release();
    write_compact_tags(out_path, h_val.data(), h_start.data(), h_val.size(), max_node_floor);
}

extern "C" pgx_status pgx_merge_tags(const char *ri_path, const char *const *tag_paths, uint32_t n_files, const uint32_t *seq_to_file,
                                     uint64_t n_seq, int device, const char *out_path) {
    PGX_GUARD_BEGIN
    merge_tags_core(ri_path, tag_paths, n_files, seq_to_file, n_seq, device, out_path, 0, 0);
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_merge_tags_ex(const char *ri_path, const char *const *tag_paths, uint32_t n_files, const uint32_t *seq_to_file,
                                        uint64_t n_seq, int device, const char *out_path, uint32_t flags) {
    PGX_GUARD_BEGIN
    merge_tags_core(ri_path, tag_paths, n_files, seq_to_file, n_seq, device, out_path, 0, flags);
    return PGX_OK;
    PGX_GUARD_END
}

// first tag of a per-chromosome stream (FileReader::get_first_tag, src/merge_tags.cpp:205-232): its node id
static uint64_t first_tag_node(const char *path) {
    std::vector<uint8_t> raw = read_whole_file(path);
    uint64_t loc = algorithm_tags_start(raw);
    if (loc >= raw.size()) throw Error(PGX_ERR_FORMAT, std::string(path) + ": empty tag file");
    const uint64_t v = bytecode_read(raw.data(), raw.size(), loc, "tag run");
    return v >> 20; // offset:10 | rev:1 | len:9 | node << 20 (encode_run_length, src/tag_arrays.cpp:28-36)
}

static void merge_tags_gbz_core(const char *gbz_path, const char *ri_path, const char *const *tag_paths, uint32_t n_files, int device,
                                const char *out_path, uint32_t flags) {
    if (!gbz_path || !ri_path || !tag_paths || !out_path || !n_files) throw Error(PGX_ERR_ARG, "pgx_merge_tags_gbz: null argument");
    GbzPaths g;
    try { parse_gbz_paths(gbz_path, g); }
    catch (const Error &e) { if (e.code == PGX_ERR_IO) throw Error(PGX_ERR_IO, std::string("Cannot open graph: ") + gbz_path); throw; }
    // component -> file: the component of the first tag's node of every file (merge_tags.cpp:481-490)
    std::vector<uint32_t> comp_to_file(g.n_components, ~0u);
    for (uint32_t f = 0; f < n_files; f++) {
        if (!tag_paths[f]) throw Error(PGX_ERR_ARG, "pgx_merge_tags_gbz: null tag path");
        const uint64_t node = first_tag_node(tag_paths[f]);
        // a node the graph does not have (0: a stream that opens with a gap run) lands in component 0 like the reference's
        // node_to_comp_map[...] (std::unordered_map::operator[] default-inserts 0, merge_tags.cpp:489)
        const uint32_t c = (node < g.component_of_node.size() && g.component_of_node[node] != ~0u) ? g.component_of_node[node] : 0u;
        if (c >= g.n_components) throw Error(PGX_ERR_FORMAT, "pgx_merge_tags_gbz: the graph has no component");
        if (comp_to_file[c] != ~0u) throw Error(PGX_ERR_FORMAT, std::string(tag_paths[f]) + ": a second tag file for the same graph component");
        comp_to_file[c] = f;
    }
    std::vector<uint32_t> s2f(g.first_node.size());
    for (uint64_t sq = 0; sq < s2f.size(); sq++) {
        const uint64_t node = g.first_node[sq];
        const uint32_t c = node ? g.component_of_node[node] : ~0u;
        if (c == ~0u || comp_to_file[c] == ~0u)
            throw Error(PGX_ERR_FORMAT, "path " + std::to_string(sq) + " of the graph starts in a component without a tag file");
        s2f[sq] = comp_to_file[c];
    }
    merge_tags_core(ri_path, tag_paths, n_files, s2f.data(), s2f.size(), device, out_path, g.max_node_id, flags);
}

extern "C" pgx_status pgx_merge_tags_gbz(const char *gbz_path, const char *ri_path, const char *const *tag_paths, uint32_t n_files, int device,
                                         const char *out_path) {
    PGX_GUARD_BEGIN
    merge_tags_gbz_core(gbz_path, ri_path, tag_paths, n_files, device, out_path, 0);
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_merge_tags_gbz_ex(const char *gbz_path, const char *ri_path, const char *const *tag_paths, uint32_t n_files, int device,
                                            const char *out_path, uint32_t flags) {
    PGX_GUARD_BEGIN
    merge_tags_gbz_core(gbz_path, ri_path, tag_paths, n_files, device, out_path, flags);
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// build_tags (pgx_build_tags_kernels.hip)
static thread_local double g_build_tags_ms[6] = {0, 0, 0, 0, 0, 0};

struct StageClock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap() {
        const auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};

// host tables of the paths: length of every sequence, start of every path node within its sequence, and the directory
// (per sequence: the path node covering text position 1024 b for every bucket b, then the sequence's last node)
struct PathTables {
    std::vector<uint64_t> seq_len, node_start, dir_off, dir;
};
static void path_tables(uint64_t n_seq, const uint64_t *path_offsets, const uint64_t *path_nodes, const uint32_t *node_length,
                        uint64_t first_node_id, uint64_t n_node_ids, PathTables &t) {
    if (path_offsets[0] != 0) throw Error(PGX_ERR_ARG, "pgx_build_tags_paths: path_offsets[0] must be 0");
    const uint64_t P = path_offsets[n_seq];
    t.seq_len.assign(n_seq, 0); t.node_start.assign(P, 0); t.dir_off.assign(n_seq, 0); t.dir.clear();
    t.dir.reserve(P / 32 + 2 * n_seq + 2);
    auto length_of = [&](uint64_t s, uint64_t v) -> uint64_t {
        const uint64_t id = v >> 1;
        if (id < first_node_id || id - first_node_id >= n_node_ids || node_length[id - first_node_id] == 0)
            throw Error(PGX_ERR_FORMAT, "build_tags: sequence " + std::to_string(s) + " visits node " + std::to_string(id) + ", which has no sequence");
        const uint64_t len = node_length[id - first_node_id];
        if (len > 1024)
            throw Error(PGX_ERR_FORMAT, "build_tags: sequence " + std::to_string(s) + " visits node " + std::to_string(id) + " of " + std::to_string(len) +
                                            " bp; tags hold offsets of 10 bits (nodes of at most 1024 bp)");
        if (id >> 44) throw Error(PGX_ERR_FORMAT, "build_tags: node id " + std::to_string(id) + " does not fit the 44 bits of a tag run");
        return len;
    };
    for (uint64_t s = 0; s < n_seq; s++) {
        const uint64_t a = path_offsets[s], e = path_offsets[s + 1];
        if (e < a || e > P) throw Error(PGX_ERR_ARG, "pgx_build_tags_paths: path_offsets not ascending");
        uint64_t pos = 0;
        for (uint64_t k = a; k < e; k++) { t.node_start[k] = pos; pos += length_of(s, path_nodes[k]); }
        t.seq_len[s] = pos;
        t.dir_off[s] = t.dir.size();
        uint64_t k = a;
        for (uint64_t b = 0; b * 1024 < pos; b++) {
            while (t.node_start[k] + node_length[(path_nodes[k] >> 1) - first_node_id] <= b * 1024) k++;
            t.dir.push_back(k);
        }
        t.dir.push_back(e > a ? e - 1 : a);
    }
}

static void build_tags_check_flags(uint32_t flags, const char *who) {
    if (flags & ~(PGX_BUILD_TAGS_REFERENCE_RUNS | PGX_BUILD_TAGS_FORWARD_ONLY | PGX_BUILD_TAGS_INPUT_RLBWT | PGX_BUILD_TAGS_OUT_COMPACT | PGX_BUILD_TAGS_OUT_BYTECODE))
        throw Error(PGX_ERR_ARG, std::string(who) + ": unknown flag");
    if ((flags & PGX_BUILD_TAGS_OUT_COMPACT) && (flags & PGX_BUILD_TAGS_OUT_BYTECODE))
        throw Error(PGX_ERR_ARG, std::string(who) + ": one output format at most");
}

static void build_tags_core(const char *ri_path, uint32_t flags, uint64_t n_paths, const uint64_t *path_offsets, const uint64_t *path_nodes,
                            const uint32_t *node_length, uint64_t first_node_id, uint64_t n_node_ids, int device, const char *out_path, double *ms) {
    StageClock clk;
    const uint32_t out_format = (flags & PGX_BUILD_TAGS_OUT_COMPACT) ? PGX_TAGS_COMPACT : (flags & PGX_BUILD_TAGS_OUT_BYTECODE) ? PGX_TAGS_BYTECODE : 0u;
    // 1. the index: only its locate side (as merge_tags)
    std::unique_ptr<pgx_index, void (*)(pgx_index *)> guard(new pgx_index(), pgx_index_close);
    pgx_index *h = guard.get();
    {
        std::vector<uint8_t> f;
        if (flags & PGX_BUILD_TAGS_INPUT_RLBWT) {
            try { f = build_rindex_bytes(ri_path, 0); }
            catch (const Error &e) { if (e.code == PGX_ERR_IO) throw Error(PGX_ERR_IO, std::string("Cannot open BWT: ") + ri_path); throw; }
        } else {
            try { f = read_whole_file(ri_path); }
            catch (const Error &) { throw Error(PGX_ERR_IO, std::string("Cannot open r-index: ") + ri_path); }
        }
        h->ri.parse(f.data(), f.size());
        std::memset(&h->img.consts, 0, sizeof h->img.consts);
        h->mode = PGX_MODE_STRICT;
        h->has_rank = true;
    }
    const uint64_t n = h->ri.sequence_size, n_seq = h->ri.C.size() > 1 ? h->ri.C[1] - h->ri.C[0] : 0;
    if (n_seq != n_paths)
        throw Error(PGX_ERR_FORMAT, "build_tags: sequence " + std::to_string(std::min(n_seq, n_paths)) + ": the index holds " + std::to_string(n_seq) +
                                        " sequences, the graph gives " + std::to_string(n_paths) + " paths" +
                                        ((flags & PGX_BUILD_TAGS_FORWARD_ONLY) ? "" : " (a text of one orientation per path needs the forward-only option)"));
    PathTables t;
    path_tables(n_seq, path_offsets, path_nodes, node_length, first_node_id, n_node_ids, t);
    pgx_device_image *d = locate_image(h, device);
    const uint64_t max_length = d->loc.max_length ? d->loc.max_length : 1;
    HIPCHECK(hipDeviceSynchronize());
    ms[1] = clk.lap();
    DevBuf sa, seq_len, dir_off, dir, node_start, nodes, idx_len, bad, head, scan, scan_tmp, run_val, run_aux, body;
    DevBuf *all[] = {&sa, &seq_len, &dir_off, &dir, &node_start, &nodes, &idx_len, &bad, &head, &scan, &scan_tmp, &run_val, &run_aux, &body};
    std::vector<uint8_t> out;
    try {
        hipStream_t s = nullptr;
        // 2. suffix array of the whole BWT
        if (n) {
            const uint64_t first = 0, last = n - 1;
            std::vector<uint64_t> off;
            uint64_t nv = 0;
            locate_core(h, d, &first, &last, 1, 0, off, sa, nv);
        }
        ms[2] = clk.lap();
        // 3. lengths from the endmarker rows, tag of every other row
        const uint64_t P = path_offsets[n_seq], D = t.dir.size();
        seq_len.ensure((n_seq ? n_seq : 1) * 8); dir_off.ensure((n_seq ? n_seq : 1) * 8); dir.ensure((D ? D : 1) * 8);
        node_start.ensure((P ? P : 1) * 8); nodes.ensure((P ? P : 1) * 8); idx_len.ensure((n_seq ? n_seq : 1) * 8); bad.ensure(8);
        if (n_seq) {
            HIPCHECK(hipMemcpyAsync(seq_len.p, t.seq_len.data(), n_seq * 8, hipMemcpyHostToDevice, s));
            HIPCHECK(hipMemcpyAsync(dir_off.p, t.dir_off.data(), n_seq * 8, hipMemcpyHostToDevice, s));
            HIPCHECK(hipMemsetAsync(idx_len.p, 0xFF, n_seq * 8, s));
        }
        if (D) HIPCHECK(hipMemcpyAsync(dir.p, t.dir.data(), D * 8, hipMemcpyHostToDevice, s));
        if (P) {
            HIPCHECK(hipMemcpyAsync(node_start.p, t.node_start.data(), P * 8, hipMemcpyHostToDevice, s));
            HIPCHECK(hipMemcpyAsync(nodes.p, path_nodes, P * 8, hipMemcpyHostToDevice, s));
        }
        HIPCHECK(hipMemsetAsync(bad.p, 0xFF, 8, s));
        if (n_seq) hipLaunchKernelGGL(pgx_bt_endmarker_kernel, dim3(grid_for(n_seq, 256)), dim3(256), 0, s, sa.as<uint64_t>(), n_seq, max_length,
                                      idx_len.as<uint64_t>());
        if (n > n_seq)
            hipLaunchKernelGGL(pgx_bt_tag_kernel, dim3(grid_for(n - n_seq, 256)), dim3(256), 0, s, sa.as<uint64_t>(), n, n_seq, max_length,
                               seq_len.as<uint64_t>(), dir_off.as<uint64_t>(), dir.as<uint64_t>(), node_start.as<uint64_t>(), nodes.as<uint64_t>(),
                               bad.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
        std::vector<uint64_t> il(n_seq);
        if (n_seq) HIPCHECK(hipMemcpy(il.data(), idx_len.p, n_seq * 8, hipMemcpyDeviceToHost));
        const uint64_t first_bad = read_u64(bad.as<uint64_t>(), s);
        for (uint64_t q = 0; q < n_seq; q++) {
            if (il[q] == ~0ull) throw Error(PGX_ERR_FORMAT, "build_tags: sequence " + std::to_string(q) + " has no endmarker row in the index");
            if (il[q] != t.seq_len[q])
                throw Error(PGX_ERR_FORMAT, "build_tags: sequence " + std::to_string(q) + ": its path spells " + std::to_string(t.seq_len[q]) +
                                                " bp, the index holds " + std::to_string(il[q]));
        }
        if (first_bad != ~0ull)
            throw Error(PGX_ERR_FORMAT, "build_tags: sequence " + std::to_string(first_bad) + ": a suffix-array row lies beyond its path");
        DevBuf *tables[] = {&seq_len, &dir_off, &dir, &node_start, &nodes, &idx_len};
        for (DevBuf *b : tables) b->release();
        ms[3] = clk.lap();
        // 4. runs: heads, scan, compaction (value, start), lengths (over the tags, now free), ByteCode bytes (over the starts), scan, write
        uint64_t R = 0, B = 0;
        head.ensure(n ? n : 1); scan.ensure((n + 1) * 8);
        if (n) hipLaunchKernelGGL(pgx_bt_heads_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, sa.as<uint64_t>(), n, n_seq, head.as<uint8_t>());
        HIPCHECK(hipGetLastError());
        scan_excl(4, head.p, n, 0, scan.as<uint64_t>(), scan_tmp, s);
        R = read_u64(scan.as<uint64_t>() + n, s);
        if (out_format) {
            // a query format: the encoder takes (value, start) as they lie; the algorithm-format body is never made, only its size.
            // That size matters: convert_tags, like the reference's, decodes the file from its first byte, so the int_vector<8> header
            // (the body's bit count) is read as ByteCodes too -- up to 8 runs in front of the real ones, the zero-length ones of which
            // still widen the compact item.  They take the PRE slots in front of the compacted runs.
            const uint64_t PRE = 8;
            run_val.ensure((R + PRE) * 8); run_aux.ensure((R + PRE) * 8);
            uint64_t *rv = run_val.as<uint64_t>() + PRE, *rs = run_aux.as<uint64_t>() + PRE;
            if (R) {
                body.ensure(R * 8);
                hipLaunchKernelGGL(pgx_bt_compact_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, sa.as<uint64_t>(), head.as<uint8_t>(), scan.as<uint64_t>(), n, rv, rs);
                hipLaunchKernelGGL(pgx_bt_length_kernel, dim3(grid_for(R, 256)), dim3(256), 0, s, rs, R, n,
                                   (uint32_t)((flags & PGX_BUILD_TAGS_REFERENCE_RUNS) ? 1 : 0), sa.as<uint64_t>());
                hipLaunchKernelGGL(pgx_bt_size_kernel, dim3(grid_for(R, 256)), dim3(256), 0, s, rv, sa.as<uint64_t>(), R, body.as<uint64_t>());
                HIPCHECK(hipGetLastError());
                scan_excl(1, body.p, R, 0, scan.as<uint64_t>(), scan_tmp, s);
                B = read_u64(scan.as<uint64_t>() + R, s);
            }
            uint64_t pre_val[PRE], pre_start[PRE], floor = 0;
            const uint64_t k = algorithm_header_runs(B, pre_val, pre_start, &floor); // (lengths for now; B = 0 gives none)
            uint64_t next = n_seq; // start of the first real run; the starts of the header's runs count down from it (only differences are read)
            for (uint64_t j = k; j-- > 0;) { next -= pre_start[j]; pre_start[j] = next; }
            if (k) {
                HIPCHECK(hipMemcpy(rv - k, pre_val, k * 8, hipMemcpyHostToDevice));
                HIPCHECK(hipMemcpy(rs - k, pre_start, k * 8, hipMemcpyHostToDevice));
            }
            HIPCHECK(hipDeviceSynchronize());
            sa.release(); head.release(); scan.release(); scan_tmp.release(); body.release();
            ms[4] = clk.lap();
            const PgxTeRuns runs{rv - k, rs - k, R + k, n, 1u, (flags & PGX_BUILD_TAGS_REFERENCE_RUNS) ? 1u : 0u};
            tags_encode_device(runs, false, floor, out_format, out_path, s);
            for (DevBuf *b : all) b->release();
            ms[5] = clk.lap();
            return;
        }
        if (R) {
            run_val.ensure(R * 8); run_aux.ensure(R * 8);
            hipLaunchKernelGGL(pgx_bt_compact_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, sa.as<uint64_t>(), head.as<uint8_t>(), scan.as<uint64_t>(), n,
                               run_val.as<uint64_t>(), run_aux.as<uint64_t>());
            hipLaunchKernelGGL(pgx_bt_length_kernel, dim3(grid_for(R, 256)), dim3(256), 0, s, run_aux.as<uint64_t>(), R, n,
                               (uint32_t)((flags & PGX_BUILD_TAGS_REFERENCE_RUNS) ? 1 : 0), sa.as<uint64_t>());
            hipLaunchKernelGGL(pgx_bt_size_kernel, dim3(grid_for(R, 256)), dim3(256), 0, s, run_val.as<uint64_t>(), sa.as<uint64_t>(), R,
                               run_aux.as<uint64_t>());
            HIPCHECK(hipGetLastError());
            scan_excl(1, run_aux.p, R, 0, scan.as<uint64_t>(), scan_tmp, s);
            B = read_u64(scan.as<uint64_t>() + R, s);
        }
        head.release();
        const uint64_t padded = (B + 7) / 8 * 8;
        out.assign(8 + padded, 0);
        const uint64_t bits = B * 8;
        std::memcpy(out.data(), &bits, 8); // int_vector<8> header of sdsl::int_vector_buffer<8>
        if (B) {
            body.ensure(B);
            hipLaunchKernelGGL(pgx_bt_write_kernel, dim3(grid_for(R, 256)), dim3(256), 0, s, run_val.as<uint64_t>(), sa.as<uint64_t>(), scan.as<uint64_t>(), R,
                               body.as<uint8_t>());
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipMemcpy(out.data() + 8, body.p, B, hipMemcpyDeviceToHost));
        }
        HIPCHECK(hipDeviceSynchronize());
        ms[4] = clk.lap();
    } catch (...) {
        for (DevBuf *b : all) b->release();
        throw;
    }
    for (DevBuf *b : all) b->release();
    // 5. the file, written only now: an error above leaves none behind
    try { write_whole_file(out_path, out); }
    catch (...) { std::remove(out_path); throw; }
    ms[5] = clk.lap();
}

extern "C" pgx_status pgx_build_tags_paths(const char *ri_path, uint64_t n_seq, const uint64_t *path_offsets, const uint64_t *path_nodes,
                                           const uint32_t *node_length, uint64_t first_node_id, uint64_t n_node_ids, int device,
                                           const char *out_path, uint32_t flags) {
    PGX_GUARD_BEGIN
    double *ms = g_build_tags_ms;
    std::fill(ms, ms + 6, 0.0);
    if (!ri_path || !out_path || !path_offsets || (path_offsets[n_seq] && !path_nodes) || (n_node_ids && !node_length))
        throw Error(PGX_ERR_ARG, "pgx_build_tags_paths: null argument");
    build_tags_check_flags(flags, "pgx_build_tags_paths");
    build_tags_core(ri_path, flags, n_seq, path_offsets, path_nodes, node_length, first_node_id, n_node_ids, device, out_path, ms);
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_build_tags(const char *gbz_path, const char *ri_path, int device, const char *out_path, uint32_t flags) {
    PGX_GUARD_BEGIN
    double *ms = g_build_tags_ms;
    std::fill(ms, ms + 6, 0.0);
    if (!gbz_path || !ri_path || !out_path) throw Error(PGX_ERR_ARG, "pgx_build_tags: null argument");
    build_tags_check_flags(flags, "pgx_build_tags");
    StageClock clk;
    GbzGraph g;
    try { parse_gbz_graph(gbz_path, (flags & PGX_BUILD_TAGS_FORWARD_ONLY) != 0, false, g); }
    catch (const Error &e) { if (e.code == PGX_ERR_IO) throw Error(PGX_ERR_IO, std::string("Cannot open graph: ") + gbz_path); throw; }
    ms[0] = clk.lap();
    build_tags_core(ri_path, flags, g.path_offsets.size() - 1, g.path_offsets.data(), g.path_nodes.data(), g.node_length.data(), g.first_node_id,
                    g.node_length.size(), device, out_path, ms);
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_build_tags_timing(double *ms, uint32_t n) {
    PGX_GUARD_BEGIN
    if (!ms && n) throw Error(PGX_ERR_ARG, "pgx_build_tags_timing: null argument");
    for (uint32_t i = 0; i < n && i < 6; i++) ms[i] = g_build_tags_ms[i];
    return PGX_OK;
    PGX_GUARD_END
}
