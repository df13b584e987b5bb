// pgx_tags_encode.hip -- host side of the device encoder of tag query files (kernels and method: pgx_tags_encode_kernels.hip).
// Two phases: everything whose size is variable is sized first (pieces, ByteCode bytes, select superblocks: count -> scan_excl),
// then the file is laid out on the host, allocated once on the device, filled by one thread per output word, downloaded once into
// pinned memory and written once.
#include <chrono>

#include "pgx_runtime_internal.hpp"

static thread_local double g_tags_encode_ms[7] = {0, 0, 0, 0, 0, 0, 0};

namespace {

inline unsigned hi_bit(uint64_t x) { return x ? 63u - (unsigned)__builtin_clzll(x) : 0u; } // sdsl::bits::hi

struct Clock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap(hipStream_t s) {
        HIPCHECK(hipStreamSynchronize(s));
        const auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};

struct SelPlan { // select_support_mcl<b> over the high bit vector (pgx_sdsl.cpp write_select_support)
    uint32_t b = 0, any_long = 0;
    uint64_t cnt = 0, n_sb = 0, logn = 0, logn4 = 0, body = 0;
    uint64_t at_super = 0, at_kind = 0, at_body = 0; // file offsets of the words
    DevBuf first, meta, sizes, off;
    uint64_t super_words() const { return (n_sb * logn + 63) / 64; }
    uint64_t kind_words() const { return (n_sb + 63) / 64; }
};

struct SdPlan { // SdVector::write
    PgxTeSd dev{};
    uint64_t size = 0, low_words = 0, high_bits = 0, high_words = 0, at_low = 0, at_high = 0;
    SelPlan sel[2]; // [0] select_1, [1] select_0: the order of the file
    void plan(const uint64_t *ones, uint64_t m, uint64_t size_) {
        size = size_;
        uint64_t logm = hi_bit(m) + 1;
        const uint64_t logn = hi_bit(size) + 1;
        if (logm == logn) logm--;
        if (logm > logn) throw Error(PGX_ERR_ARG, "pgx_tags_encode: more ones than positions"); // (cannot happen: m <= size by construction)
        dev.ones = ones; dev.m = m; dev.wl = (uint32_t)(logn - logm);
        low_words = (m * dev.wl + 63) / 64;
        high_bits = m + ((size + (1ull << dev.wl) - 1) >> dev.wl);
        high_words = (high_bits + 63) / 64;
        const uint64_t capacity = ((high_bits + 63) >> 6) << 6, l = hi_bit(capacity) + 1;
        for (int k = 0; k < 2; k++) {
            SelPlan &p = sel[k];
            p.b = k == 0 ? 1 : 0;
            p.cnt = p.b ? m : high_bits - m;
            p.n_sb = (p.cnt + 4095) / 4096;
            p.logn = l; p.logn4 = l * l * l * l;
        }
    }
};

struct Encoder {
    hipStream_t s;
    DevBuf tmp_np, tmp_len, tmp_nb, piece_off, pos_off, byte_off, scan_tmp, ctr, pos, items, sstart, file, fields;
    HostBuf pin;
    SdPlan sd[2]; // starts, intervals
    std::vector<PgxTeField> h_fields;
    uint64_t peak = 0;

    std::vector<DevBuf *> all;
    Encoder() : all{&tmp_np, &tmp_len, &tmp_nb, &piece_off, &pos_off, &byte_off, &scan_tmp, &ctr, &pos, &items, &sstart, &file, &fields} {
        for (SdPlan &v : sd)
            for (SelPlan &p : v.sel) { all.push_back(&p.first); all.push_back(&p.meta); all.push_back(&p.sizes); all.push_back(&p.off); }
    }
    Encoder(const Encoder &) = delete;
    Encoder &operator=(const Encoder &) = delete;
    void note_peak() {
        uint64_t sum = 0;
        for (DevBuf *b : all) sum += b->cap;
        peak = std::max(peak, sum);
    }
    void release_device() { for (DevBuf *b : all) b->release(); }
    void release() { release_device(); pin.release(); }
    void field(uint64_t offset, uint64_t value, uint32_t bytes) { h_fields.push_back(PgxTeField{offset, value, bytes, 0}); }

    // phase 1 of a select support: kind, width and bytes of every superblock, their offsets
    void size_select(SdPlan &v) {
        for (SelPlan &p : v.sel) {
            if (!p.cnt) continue;
            p.first.ensure(p.n_sb * 8); p.meta.ensure(p.n_sb); p.sizes.ensure(p.n_sb * 8); p.off.ensure((p.n_sb + 1) * 8);
            unsigned int *flag = ctr.as<unsigned int>() + 4 + (&v - sd) * 2 + (&p - v.sel);
            hipLaunchKernelGGL(pgx_te_sel_size_kernel, dim3(grid_for(p.n_sb, 256)), dim3(256), 0, s, v.dev, p.b, p.cnt, p.n_sb, p.logn4, p.first.as<uint64_t>(),
                               p.meta.as<uint8_t>(), p.sizes.as<uint64_t>(), flag);
            HIPCHECK(hipGetLastError());
            scan_excl(1, p.sizes.p, p.n_sb, 0, p.off.as<uint64_t>(), scan_tmp, s);
            p.body = read_u64(p.off.as<uint64_t>() + p.n_sb, s);
            uint64_t two = 0; // (the flags are 4-byte words; read the aligned pair)
            read_scalars(&two, ctr.as<unsigned int>() + 4 + (&v - sd) * 2, 8, s);
            p.any_long = (uint32_t)(two >> (32 * (&p - v.sel))) & 1u;
        }
    }
    // the layout of one sd_vector from file offset o on: scalar fields now, word offsets for the fill; returns the offset behind it
    uint64_t lay_out(SdPlan &v, uint64_t o) {
        field(o, v.size, 8); field(o + 8, v.dev.wl, 1); o += 9;
        field(o, v.dev.m * v.dev.wl, 8); field(o + 8, v.dev.wl, 1); o += 9;
        v.at_low = o; o += v.low_words * 8;
        field(o, v.high_bits, 8); o += 8;
        v.at_high = o; o += v.high_words * 8;
        for (SelPlan &p : v.sel) {
            field(o, p.cnt, 8); o += 8;
            if (!p.cnt) continue;
            field(o, p.n_sb * p.logn, 8); field(o + 8, p.logn, 1); o += 9;
            p.at_super = o; o += p.super_words() * 8;
            field(o, p.any_long ? p.n_sb : 0, 8); o += 8;
            if (p.any_long) { p.at_kind = o; o += p.kind_words() * 8; }
            p.at_body = o; o += p.body;
        }
        return o;
    }
    void fill_sd(SdPlan &v) {
        uint8_t *f = file.as<uint8_t>();
        if (v.low_words) hipLaunchKernelGGL(pgx_te_sd_low_kernel, dim3(grid_for(v.low_words, 256)), dim3(256), 0, s, v.dev, f + v.at_low, v.low_words);
        hipLaunchKernelGGL(pgx_te_sd_high_kernel, dim3(grid_for(v.high_words, 256)), dim3(256), 0, s, v.dev, f + v.at_high, v.high_words);
        HIPCHECK(hipGetLastError());
    }
    void fill_select(SdPlan &v) {
        uint8_t *f = file.as<uint8_t>();
        for (SelPlan &p : v.sel) {
            if (!p.cnt) continue;
            hipLaunchKernelGGL(pgx_te_sel_super_kernel, dim3(grid_for(p.super_words(), 256)), dim3(256), 0, s, p.first.as<uint64_t>(), p.n_sb, (uint32_t)p.logn,
                               f + p.at_super, p.super_words());
            if (p.any_long)
                hipLaunchKernelGGL(pgx_te_sel_kind_kernel, dim3(grid_for(p.kind_words(), 256)), dim3(256), 0, s, p.meta.as<uint8_t>(), p.n_sb, f + p.at_kind,
                                   p.kind_words());
            hipLaunchKernelGGL(pgx_te_sel_body_kernel, dim3(grid_for(p.n_sb, 1)), dim3(64), 0, s, v.dev, p.b, p.cnt, p.first.as<uint64_t>(), p.meta.as<uint8_t>(),
                               p.off.as<uint64_t>(), f + p.at_body);
            HIPCHECK(hipGetLastError());
        }
    }

    void run(const PgxTeRuns &runs, bool zero_len_counts, uint64_t max_node_floor, uint32_t format, const char *out_path, double *ms) {
        const bool bytecode = format == PGX_TAGS_BYTECODE;
        const uint64_t R = runs.n_runs;
        Clock clk;
        // 1. pieces, lengths, ByteCode bytes per run and their prefix sums; the largest node
        ctr.ensure(64);
        HIPCHECK(hipMemsetAsync(ctr.p, 0, 64, s));
        piece_off.ensure((R + 1) * 8); pos_off.ensure((R + 1) * 8);
        if (bytecode) byte_off.ensure((R + 1) * 8);
        uint64_t M = 0, T = 0, B = 0;
        if (R) {
            tmp_np.ensure(R * 8); tmp_len.ensure(R * 8);
            if (bytecode) tmp_nb.ensure(R * 8);
            hipLaunchKernelGGL(pgx_te_count_kernel, dim3(grid_for(R, 256)), dim3(256), 0, s, runs, (uint32_t)(zero_len_counts ? 1 : 0), tmp_np.as<uint64_t>(),
                               tmp_len.as<uint64_t>(), bytecode ? tmp_nb.as<uint64_t>() : (uint64_t *)nullptr, ctr.as<unsigned long long>());
            HIPCHECK(hipGetLastError());
        }
        scan_excl(1, tmp_np.p, R, 0, piece_off.as<uint64_t>(), scan_tmp, s);
        scan_excl(1, tmp_len.p, R, 0, pos_off.as<uint64_t>(), scan_tmp, s);
        if (bytecode) scan_excl(1, tmp_nb.p, R, 0, byte_off.as<uint64_t>(), scan_tmp, s);
        M = read_u64(piece_off.as<uint64_t>() + R, s);
        T = read_u64(pos_off.as<uint64_t>() + R, s);
        if (bytecode) B = read_u64(byte_off.as<uint64_t>() + R, s);
        const uint64_t max_node = std::max(read_u64(ctr.as<uint64_t>(), s), bytecode ? 0 : max_node_floor);
        note_peak();
        tmp_np.release(); tmp_len.release(); tmp_nb.release();
        const unsigned width = 11 + hi_bit(max_node) + 1; // merge_tags.cpp:636-637
        if (!bytecode && width > 64) throw Error(PGX_ERR_FORMAT, "pgx_tags_encode: node id " + std::to_string(max_node) + " does not fit a 64-bit item");
        if (bytecode && (max_node >> 44)) throw Error(PGX_ERR_FORMAT, "pgx_tags_encode: node id " + std::to_string(max_node) + " does not fit the 44 bits of a tag run");
        // 2. per piece: BWT start; item (compact) or the byte offset of every 10th piece (ByteCode)
        const uint64_t m_starts = (M + 9) / 10;
        pos.ensure((M ? M : 1) * 8);
        if (bytecode) sstart.ensure((m_starts ? m_starts : 1) * 8);
        else items.ensure((M ? M : 1) * 8);
        if (M) {
            hipLaunchKernelGGL(pgx_te_expand_kernel, dim3(grid_for(R, 256)), dim3(256), 0, s, runs, piece_off.as<uint64_t>(), pos_off.as<uint64_t>(),
                               bytecode ? byte_off.as<uint64_t>() : (const uint64_t *)nullptr, PGX_TE_EXPAND_PIECES, pos.as<uint64_t>(),
                               bytecode ? (uint64_t *)nullptr : items.as<uint64_t>(), bytecode ? sstart.as<uint64_t>() : (uint64_t *)nullptr, (uint8_t *)nullptr);
            HIPCHECK(hipGetLastError());
        }
        uint64_t starts_size = 1; // builder(start_pos + 1, ones): tag_arrays.cpp:626 (compact, item index), :565 (ByteCode, byte offset)
        if (m_starts) starts_size = (bytecode ? read_u64(sstart.as<uint64_t>() + (m_starts - 1), s) : 10 * (m_starts - 1)) + 1;
        sd[0].plan(bytecode ? sstart.as<uint64_t>() : nullptr, m_starts, starts_size);
        sd[1].plan(pos.as<uint64_t>(), M, T + 1);
        ms[0] = clk.lap(s);
        // 3. select supports, phase 1
        for (SdPlan &v : sd) size_select(v);
        ms[2] = clk.lap(s);
        // 4. the layout
        uint64_t o = 0, at_body = 0, item_words = 0;
        if (bytecode) {
            field(0, B, 8);
            at_body = 8; o = 8 + B;
        } else {
            item_words = (M * width + 63) / 64;
            field(0, M * width, 8); field(8, width, 1);
            at_body = 9; o = 9 + item_words * 8;
        }
        o = lay_out(sd[0], o);
        const uint64_t total = lay_out(sd[1], o);
        file.ensure(total + 8);
        fields.ensure(h_fields.size() * sizeof(PgxTeField));
        note_peak();
        uint8_t *f = file.as<uint8_t>();
        HIPCHECK(hipMemcpyAsync(fields.p, h_fields.data(), h_fields.size() * sizeof(PgxTeField), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(pgx_te_fields_kernel, dim3(grid_for(h_fields.size(), 64)), dim3(64), 0, s, fields.as<PgxTeField>(), (uint32_t)h_fields.size(), f);
        // 5. items / ByteCodes
        if (bytecode && M)
            hipLaunchKernelGGL(pgx_te_expand_kernel, dim3(grid_for(R, 256)), dim3(256), 0, s, runs, piece_off.as<uint64_t>(), pos_off.as<uint64_t>(),
                               byte_off.as<uint64_t>(), PGX_TE_EXPAND_STREAM, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, f + at_body);
        if (!bytecode && item_words)
            hipLaunchKernelGGL(pgx_te_pack_items_kernel, dim3(grid_for(item_words, 256)), dim3(256), 0, s, items.as<uint64_t>(), M, width, f + at_body, item_words);
        HIPCHECK(hipGetLastError());
        ms[0] += clk.lap(s);
        // 6. the two sd_vector bodies, then their select supports
        for (SdPlan &v : sd) fill_sd(v);
        ms[1] = clk.lap(s);
        for (SdPlan &v : sd) fill_select(v);
        ms[2] += clk.lap(s);
        // 7. one download, one write: an error above leaves no file
        pin.ensure(total ? total : 1);
        HIPCHECK(hipMemcpyAsync(pin.p, file.p, total, hipMemcpyDeviceToHost, s));
        ms[3] = clk.lap(s);
        ms[5] = (double)total; ms[6] = (double)peak;
        release_device();
        FILE *fp = std::fopen(out_path, "wb");
        if (!fp) throw Error(PGX_ERR_IO, std::string("Cannot create file: ") + out_path);
        const bool ok = std::fwrite(pin.p, 1, total, fp) == total;
        if (std::fclose(fp) != 0 || !ok) {
            std::remove(out_path);
            throw Error(PGX_ERR_IO, std::string("Short write: ") + out_path);
        }
        ms[4] = clk.lap(s);
    }
};

} // namespace

void tags_encode_device(const PgxTeRuns &runs, bool zero_len_counts, uint64_t max_node_floor, uint32_t format, const char *out_path, hipStream_t s) {
    double *ms = g_tags_encode_ms;
    std::fill(ms, ms + 7, 0.0);
    if (format != PGX_TAGS_COMPACT && format != PGX_TAGS_BYTECODE) throw Error(PGX_ERR_ARG, "pgx_tags_encode: the format is PGX_TAGS_COMPACT or PGX_TAGS_BYTECODE");
    Encoder e;
    e.s = s;
    try { e.run(runs, zero_len_counts, max_node_floor, format, out_path, ms); }
    catch (...) { e.release(); throw; }
    e.release();
}

extern "C" pgx_status pgx_tags_encode(int device, const uint64_t *values, const uint64_t *lengths, uint64_t n_runs, uint64_t max_node_floor, uint32_t format,
                                      const char *out_path) {
    PGX_GUARD_BEGIN
    std::fill(g_tags_encode_ms, g_tags_encode_ms + 7, 0.0);
    if (!out_path || (n_runs && (!values || !lengths))) throw Error(PGX_ERR_ARG, "pgx_tags_encode: null argument");
    if (format != PGX_TAGS_COMPACT && format != PGX_TAGS_BYTECODE) throw Error(PGX_ERR_ARG, "pgx_tags_encode: the format is PGX_TAGS_COMPACT or PGX_TAGS_BYTECODE");
    use_device(device);
    DevBuf val, len, bytes, off, scan_tmp;
    DevBuf *all[] = {&val, &len, &bytes, &off, &scan_tmp};
    try {
        // the runs behind 8 free slots.  ByteCode: pgx_convert_tags' input is a build_tags file, whose header it reads as up to 8 more
        // runs in front (algorithm_header_runs); they depend on the size of the body those runs make, counted by build_tags' own kernel
        const uint64_t PRE = 8;
        hipStream_t s = nullptr;
        val.ensure((n_runs + PRE) * 8); len.ensure((n_runs + PRE) * 8);
        uint64_t *dv = val.as<uint64_t>() + PRE, *dl = len.as<uint64_t>() + PRE, k = 0;
        if (n_runs) {
            HIPCHECK(hipMemcpy(dv, values, n_runs * 8, hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(dl, lengths, n_runs * 8, hipMemcpyHostToDevice));
        }
        if (format == PGX_TAGS_BYTECODE && n_runs) {
            bytes.ensure(n_runs * 8); off.ensure((n_runs + 1) * 8);
            hipLaunchKernelGGL(pgx_bt_size_kernel, dim3(grid_for(n_runs, 256)), dim3(256), 0, s, dv, dl, n_runs, bytes.as<uint64_t>());
            HIPCHECK(hipGetLastError());
            scan_excl(1, bytes.p, n_runs, 0, off.as<uint64_t>(), scan_tmp, s);
            uint64_t pre_val[PRE], pre_len[PRE], node = 0;
            k = algorithm_header_runs(read_u64(off.as<uint64_t>() + n_runs, s), pre_val, pre_len, &node);
            if (k) {
                HIPCHECK(hipMemcpy(dv - k, pre_val, k * 8, hipMemcpyHostToDevice));
                HIPCHECK(hipMemcpy(dl - k, pre_len, k * 8, hipMemcpyHostToDevice));
            }
            bytes.release(); off.release(); scan_tmp.release();
        }
        const PgxTeRuns runs{dv - k, dl - k, n_runs + k, 0, 0, 0};
        tags_encode_device(runs, true, max_node_floor, format, out_path, s);
    } catch (...) {
        for (DevBuf *b : all) b->release();
        throw;
    }
    for (DevBuf *b : all) b->release();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_tags_encode_timing(double *ms, uint32_t n) {
    PGX_GUARD_BEGIN
    if (!ms && n) throw Error(PGX_ERR_ARG, "pgx_tags_encode_timing: null argument");
    for (uint32_t i = 0; i < n && i < 7; i++) ms[i] = g_tags_encode_ms[i];
    return PGX_OK;
    PGX_GUARD_END
}
