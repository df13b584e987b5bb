// pgx_batch_forms.hip -- the result of a run in its other two forms, each made on the device from the batch (pgx_batch_result_compact,
// pgx_batch_format) or from host arrays (pgx_compact_encode, pgx_format_result): the compact form and the text form.
#include <string>

#include "pgx_batch_internal.hpp"

// ------------------------------------------------------------------------------------------
// compact result form (pgx_compact_kernels.hip; the format: include/pgx.h "compact result"; the host decoder: pgx_compact.cpp)
// Sizes every block, scans the sizes into block_offsets and brings the three tables to w.h_tab: the host waits for them here, their last entry
// sizes the byte buffer.  Returns the size of the stream.
static uint64_t compact_tables(CompactWork &w, const uint64_t *d_mem_off, const pgx_mem *d_mems, const uint64_t *d_run_nums, const uint64_t *d_pos_off,
                               const uint64_t *d_positions, uint64_t n_reads, bool tags, bool timed, hipStream_t s) {
    const uint64_t nb = (n_reads + PGX_COMPACT_BLOCK_READS - 1) / PGX_COMPACT_BLOCK_READS;
    w.sizes.ensure((nb ? nb : 1) * 8);
    w.tab.ensure(3 * (nb + 1) * 8);
    w.h_tab.ensure(3 * (nb + 1) * 8);
    uint64_t *bo = w.tab.as<uint64_t>(), *fm = bo + (nb + 1), *fp = fm + (nb + 1);
    if (timed) {
        for (auto &e : w.ev)
            if (!e) HIPCHECK(hipEventCreate(&e));
        HIPCHECK(hipEventRecord(w.ev[0], s));
    }
    hipLaunchKernelGGL(pgx_compact_size_kernel, dim3(grid_for(nb + 1, 4)), dim3(256), 0, s, d_mem_off, d_mems, d_run_nums, d_pos_off, d_positions, n_reads, nb,
                       tags ? 1 : 0, w.sizes.as<uint64_t>(), fm, fp);
    HIPCHECK(hipGetLastError());
    scan_excl(1, w.sizes.p, nb, 0, bo, w.scan_tmp, s);
    if (timed) HIPCHECK(hipEventRecord(w.ev[1], s));
    HIPCHECK(hipMemcpyAsync(w.h_tab.p, w.tab.p, 3 * (nb + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return w.h_tab.as<uint64_t>()[nb];
}

// the stream itself into w.bytes (grown to `total` first); async on s
static void compact_fill(CompactWork &w, const uint64_t *d_mem_off, const pgx_mem *d_mems, const uint64_t *d_run_nums, const uint64_t *d_pos_off,
                         const uint64_t *d_positions, uint64_t n_reads, bool tags, bool timed, uint64_t total, hipStream_t s) {
    const uint64_t nb = (n_reads + PGX_COMPACT_BLOCK_READS - 1) / PGX_COMPACT_BLOCK_READS;
    w.bytes.ensure(total ? total : 8);
    if (timed) HIPCHECK(hipEventRecord(w.ev[2], s));
    if (nb) {
        // PGX_COMPACT_STAGE=1 (read per call): the fill kernel that stages its bytes in LDS and stores 8-byte words; the same stream either way
        const char *e = std::getenv("PGX_COMPACT_STAGE");
        const bool staged = e && e[0] == '1' && e[1] == 0;
        hipLaunchKernelGGL(staged ? pgx_compact_fill_staged_kernel : pgx_compact_fill_kernel, dim3(grid_for(nb, 4)), dim3(256), 0, s, d_mem_off, d_mems, d_run_nums, d_pos_off, d_positions, n_reads, nb,
                           tags ? 1 : 0, (const uint64_t *)w.tab.as<uint64_t>(), w.bytes.as<uint8_t>());
        HIPCHECK(hipGetLastError());
    }
    if (timed) HIPCHECK(hipEventRecord(w.ev[3], s));
}

static float compact_ms(CompactWork &w) { // (behind the synchronisation that follows compact_fill)
    float a = 0, c = 0;
    HIPCHECK(hipEventElapsedTime(&a, w.ev[0], w.ev[1]));
    HIPCHECK(hipEventElapsedTime(&c, w.ev[2], w.ev[3]));
    return a + c;
}

extern "C" pgx_status pgx_batch_result_compact(pgx_batch *b, pgx_compact_result *out) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_result_compact");
    checked_device_count();
    if (!b || !out || !b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_result_compact: batch has not been run");
    use_device(b->device);
    CompactWork &w = b->cw;
    hipStream_t s = b->own; // (the run itself completed inside pgx_batch_run, on whatever stream it used)
    const bool tags = b->ran_tags, timed = b->timed;
    const uint64_t n = b->n_reads, nb = (n + PGX_COMPACT_BLOCK_READS - 1) / PGX_COMPACT_BLOCK_READS;
    const uint64_t *run_nums = tags ? b->tw.run_nums.as<uint64_t>() : nullptr, *pos_off = tags ? b->tw.pos_off.as<uint64_t>() : nullptr;
    const uint64_t *positions = tags ? b->tw.positions.as<uint64_t>() : nullptr;
    const uint64_t total = compact_tables(w, b->mem_off.as<uint64_t>(), b->mems.as<pgx_mem>(), run_nums, pos_off, positions, n, tags, timed, s);
    compact_fill(w, b->mem_off.as<uint64_t>(), b->mems.as<pgx_mem>(), run_nums, pos_off, positions, n, tags, timed, total, s);
    w.h_bytes.ensure(total ? total : 8);
    if (total) HIPCHECK(hipMemcpyAsync(w.h_bytes.p, w.bytes.p, total, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    std::memset(out, 0, sizeof *out);
    out->n_reads = n;
    out->n_mems = b->n_mems;
    out->n_extensions = b->n_ext;
    if (tags) {
        out->n_positions = b->n_positions;
        out->n_tag_overflow = b->n_tag_overflow;
        out->flags = PGX_COMPACT_TAGS;
    }
    out->block_reads = PGX_COMPACT_BLOCK_READS;
    out->n_blocks = nb;
    out->n_bytes = total;
    out->block_offsets = w.h_tab.as<uint64_t>();
    out->block_first_mem = out->block_offsets + (nb + 1);
    out->block_first_pos = out->block_first_mem + (nb + 1);
    out->bytes = w.h_bytes.as<uint8_t>();
    out->ms_encode = timed ? compact_ms(w) : 0;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_compact_encode(int device, const pgx_result *in, uint8_t *bytes, uint64_t bytes_cap, uint64_t *block_offsets,
                                         uint64_t *block_first_mem, uint64_t *block_first_pos, uint64_t *n_bytes) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_compact_encode");
    use_device(device);
    if (!in || !in->mem_offsets || (in->n_mems && !in->mems) || (bytes_cap && !bytes) || !block_offsets || !block_first_mem || !block_first_pos || !n_bytes)
        throw Error(PGX_ERR_ARG, "pgx_compact_encode: null argument");
    const bool tags = in->pos_offsets != nullptr;
    const uint64_t n = in->n_reads, m = in->n_mems, np = tags ? in->n_positions : 0;
    if (tags && ((m && !in->tag_run_counts) || (np && !in->positions))) throw Error(PGX_ERR_ARG, "pgx_compact_encode: pos_offsets without tag_run_counts / positions");
    auto check_csr = [](const uint64_t *off, uint64_t cnt, uint64_t last, const char *name) { // the kernels index the arrays by these
        bool ok = off[0] == 0 && off[cnt] == last;
        for (uint64_t i = 0; ok && i < cnt; i++) ok = off[i] <= off[i + 1];
        if (!ok) throw Error(PGX_ERR_ARG, std::string("pgx_compact_encode: ") + name + " must start at 0, never decrease and end at the count of what it indexes");
    };
    check_csr(in->mem_offsets, n, m, "mem_offsets");
    if (tags) check_csr(in->pos_offsets, m, np, "pos_offsets");
    struct EncodeInput { // device copies of the input + the encoder's buffers, released on every way out
        DevBuf mem_off, mems, run_nums, pos_off, positions;
        CompactWork w;
        ~EncodeInput() { release_all({&mem_off, &mems, &run_nums, &pos_off, &positions}); w.release(); }
    } k;
    upload(k.mem_off, in->mem_offsets, (n + 1) * 8);
    upload(k.mems, in->mems, m * sizeof(pgx_mem));
    if (tags) {
        upload(k.run_nums, in->tag_run_counts, m * 8);
        upload(k.pos_off, in->pos_offsets, (m + 1) * 8);
        upload(k.positions, in->positions, np * 8);
    }
    hipStream_t s = nullptr;
    const uint64_t nb = (n + PGX_COMPACT_BLOCK_READS - 1) / PGX_COMPACT_BLOCK_READS;
    const uint64_t total = compact_tables(k.w, k.mem_off.as<uint64_t>(), k.mems.as<pgx_mem>(), k.run_nums.as<uint64_t>(), k.pos_off.as<uint64_t>(),
                                          k.positions.as<uint64_t>(), n, tags, false, s);
    *n_bytes = total;
    const uint64_t *t = k.w.h_tab.as<uint64_t>();
    std::memcpy(block_offsets, t, (nb + 1) * 8);
    std::memcpy(block_first_mem, t + (nb + 1), (nb + 1) * 8);
    std::memcpy(block_first_pos, t + 2 * (nb + 1), (nb + 1) * 8);
    if (total > bytes_cap)
        throw Error(PGX_ERR_NOMEM, "pgx_compact_encode: the stream takes " + std::to_string(total) + " bytes, bytes_cap is " + std::to_string(bytes_cap));
    compact_fill(k.w, k.mem_off.as<uint64_t>(), k.mems.as<pgx_mem>(), k.run_nums.as<uint64_t>(), k.pos_off.as<uint64_t>(), k.positions.as<uint64_t>(), n, tags,
                 false, total, s);
    if (total) HIPCHECK(hipMemcpyAsync(bytes, k.w.bytes.p, total, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// text output (pgx_format_kernels.hip; the grammar: include/pgx.h "text output")
struct FormatIn { // a result on the device, and what pgx_format_params adds
    const uint64_t *mem_off, *pos_off, *positions, *loc_off, *values;
    const pgx_mem *mems;
    uint64_t n_reads, n_mems, n_positions, n_values, first_seq, max_length;
    uint32_t flags;
    bool locate() const { return (flags & (PGX_FORMAT_LOCATE_POSITIONS | PGX_FORMAT_LOCATE_SEQS)) != 0; }
    PgxFormatArgs args() const { return PgxFormatArgs{mem_off, mems, pos_off, loc_off, n_reads, n_mems, first_seq, flags}; }
    uint64_t value_divisor() const { return (flags & PGX_FORMAT_LOCATE_POSITIONS) ? max_length : 0; } // (0: the values print as they are)
};

// what both entry points refuse in a pgx_format_params, said with or without a device
static void format_check_params(const pgx_format_params *p, const char *who) {
    if (!p) throw Error(PGX_ERR_ARG, std::string(who) + ": null argument");
    if (p->flags & ~(PGX_FORMAT_STDERR | PGX_FORMAT_LOCATE_POSITIONS | PGX_FORMAT_LOCATE_SEQS)) throw Error(PGX_ERR_ARG, std::string(who) + ": unknown flag");
    if (p->reserved) throw Error(PGX_ERR_ARG, std::string(who) + ": reserved must be 0");
    if ((p->flags & PGX_FORMAT_LOCATE_POSITIONS) && (p->flags & PGX_FORMAT_LOCATE_SEQS))
        throw Error(PGX_ERR_ARG, std::string(who) + ": PGX_FORMAT_LOCATE_POSITIONS and PGX_FORMAT_LOCATE_SEQS exclude each other");
}

// The length pass: every level's lengths and scans, then read_offsets (and the total of the stderr lines behind them) to w.h_roff.  The host waits
// here: the totals size the text buffers.
static void format_lengths(FormatWork &w, const FormatIn &in, bool timed, hipStream_t s, uint64_t &n_bytes, uint64_t &n_err_bytes) {
    const uint64_t n = in.n_reads, m = in.n_mems, np = in.n_positions, nv = in.locate() ? in.n_values : 0;
    const bool err = (in.flags & PGX_FORMAT_STDERR) != 0;
    w.plen.ensure(np ? np : 1); w.pcum.ensure((np + 1) * 8);
    if (in.locate()) { w.vlen.ensure(nv ? nv : 1); w.vcum.ensure((nv + 1) * 8); }
    w.mlen.ensure((m ? m : 1) * 8); w.mcum.ensure((m + 1) * 8);
    w.rlen.ensure((n ? n : 1) * 8); w.roff.ensure((n + 1) * 8);
    if (err) { w.elen.ensure(n ? n : 1); w.eoff.ensure((n + 1) * 8); }
    HostBuf &h_roff = w.h_roff[w.cur];
    h_roff.ensure((n + 2) * 8);
    if (timed) {
        for (auto &e : w.ev)
            if (!e) HIPCHECK(hipEventCreate(&e));
        HIPCHECK(hipEventRecord(w.ev[0], s));
    }
    if (np) hipLaunchKernelGGL(pgx_format_item_len_kernel, dim3(grid_for(np, 256)), dim3(256), 0, s, in.positions, np, (uint64_t)0, w.plen.as<uint8_t>());
    scan_excl(4, w.plen.p, np, 0, w.pcum.as<uint64_t>(), w.scan_tmp, s);
    if (in.locate()) {
        if (nv) hipLaunchKernelGGL(pgx_format_item_len_kernel, dim3(grid_for(nv, 256)), dim3(256), 0, s, in.values, nv, in.value_divisor(), w.vlen.as<uint8_t>());
        scan_excl(4, w.vlen.p, nv, 0, w.vcum.as<uint64_t>(), w.scan_tmp, s);
    }
    const uint64_t *vcum = in.locate() ? w.vcum.as<uint64_t>() : nullptr;
    if (m) hipLaunchKernelGGL(pgx_format_mem_len_kernel, dim3(grid_for(m, 256)), dim3(256), 0, s, in.args(), (const uint64_t *)w.pcum.as<uint64_t>(), vcum, w.mlen.as<uint64_t>());
    scan_excl(1, w.mlen.p, m, 0, w.mcum.as<uint64_t>(), w.scan_tmp, s);
    if (n) hipLaunchKernelGGL(pgx_format_read_len_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, in.args(), (const uint64_t *)w.mcum.as<uint64_t>(), w.rlen.as<uint64_t>(),
                              err ? w.elen.as<uint8_t>() : nullptr);
    HIPCHECK(hipGetLastError());
    scan_excl(1, w.rlen.p, n, 0, w.roff.as<uint64_t>(), w.scan_tmp, s);
    if (err) scan_excl(4, w.elen.p, n, 0, w.eoff.as<uint64_t>(), w.scan_tmp, s);
    if (timed) HIPCHECK(hipEventRecord(w.ev[1], s));
    uint64_t *h = h_roff.as<uint64_t>();
    h[n + 1] = 0;
    HIPCHECK(hipMemcpyAsync(h, w.roff.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (err) HIPCHECK(hipMemcpyAsync(h + n + 1, w.eoff.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    n_bytes = h[n];
    n_err_bytes = h[n + 1];
}

// The fill pass into w.text / w.etext (grown to the totals first); async on s.  Every byte of text[0 .. n_bytes) is written by exactly one lane.
static void format_fill(FormatWork &w, const FormatIn &in, bool timed, hipStream_t s, uint64_t n_bytes, uint64_t n_err_bytes) {
    const uint64_t n = in.n_reads, m = in.n_mems, np = in.n_positions, nv = in.locate() ? in.n_values : 0;
    const bool err = (in.flags & PGX_FORMAT_STDERR) != 0;
    w.text.ensure(n_bytes ? n_bytes : 8);
    if (err) w.etext.ensure(n_err_bytes ? n_err_bytes : 8);
    w.pbase.ensure((m ? m : 1) * 8);
    if (in.locate()) w.vbase.ensure((m ? m : 1) * 8);
    char *text = w.text.as<char>();
    const uint64_t *roff = w.roff.as<uint64_t>(), *pcum = w.pcum.as<uint64_t>(), *vcum = in.locate() ? w.vcum.as<uint64_t>() : nullptr;
    if (timed) HIPCHECK(hipEventRecord(w.ev[2], s));
    if (n) hipLaunchKernelGGL(pgx_format_fill_reads_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, in.args(), roff, err ? (const uint64_t *)w.eoff.as<uint64_t>() : nullptr, text,
                              err ? w.etext.as<char>() : nullptr);
    if (m) hipLaunchKernelGGL(pgx_format_fill_mems_kernel, dim3(grid_for(m, 256)), dim3(256), 0, s, in.args(), roff, (const uint64_t *)w.mcum.as<uint64_t>(), pcum, vcum, text,
                              w.pbase.as<uint64_t>(), in.locate() ? w.vbase.as<uint64_t>() : nullptr);
    if (np) hipLaunchKernelGGL(pgx_format_fill_items_kernel, dim3(grid_for(np, 256)), dim3(256), 0, s, in.positions, np, in.pos_off, m, pcum, (const uint64_t *)w.pbase.as<uint64_t>(),
                               (uint64_t)0, text);
    if (nv) hipLaunchKernelGGL(pgx_format_fill_items_kernel, dim3(grid_for(nv, 256)), dim3(256), 0, s, in.values, nv, in.loc_off, m, vcum, (const uint64_t *)w.vbase.as<uint64_t>(),
                               in.value_divisor(), text);
    HIPCHECK(hipGetLastError());
    if (timed) HIPCHECK(hipEventRecord(w.ev[3], s));
}

static float format_ms(FormatWork &w) { // (behind the synchronisation that follows format_fill)
    float a = 0, c = 0;
    HIPCHECK(hipEventElapsedTime(&a, w.ev[0], w.ev[1]));
    HIPCHECK(hipEventElapsedTime(&c, w.ev[2], w.ev[3]));
    return a + c;
}

extern "C" pgx_status pgx_batch_format(pgx_batch *b, const pgx_format_params *p, pgx_text *out) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_format");
    checked_device_count();
    if (!b || !out) throw Error(PGX_ERR_ARG, "pgx_batch_format: null argument");
    format_check_params(p, "pgx_batch_format");
    if (!b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_format: batch has not been run");
    if (!b->ran_tags) throw Error(PGX_ERR_ARG, "pgx_batch_format: the run had no PGX_RUN_TAGS (the text holds the positions of every MEM)");
    FormatIn in{};
    in.flags = p->flags;
    if (in.locate()) { // the last locate must be of the form the flag prints
        const LocWork &lw = b->lw;
        const uint32_t want = (p->flags & PGX_FORMAT_LOCATE_SEQS) ? (PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE) : 0u;
        if (!lw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_format: a locate flag without a completed pgx_batch_locate");
        if (lw.flags != want || lw.n_mems != b->n_mems)
            throw Error(PGX_ERR_ARG, "pgx_batch_format: the last pgx_batch_locate ran with flags " + std::to_string(lw.flags) + ", the locate flag given prints the result of flags " +
                                         std::to_string(want));
        in.loc_off = lw.d_off;
        in.values = lw.vals.as<uint64_t>();
        in.n_values = lw.n_values;
    }
    use_device(b->device);
    FormatWork &w = b->fw;
    hipStream_t s = b->own; // (the run and the locate completed inside their calls, on whatever stream they used)
    const bool timed = b->timed, err = (p->flags & PGX_FORMAT_STDERR) != 0;
    in.mem_off = b->mem_off.as<uint64_t>();
    in.mems = b->mems.as<pgx_mem>();
    in.pos_off = b->tw.pos_off.as<uint64_t>();
    in.positions = b->tw.positions.as<uint64_t>();
    in.n_reads = b->n_reads; in.n_mems = b->n_mems; in.n_positions = b->n_positions;
    in.first_seq = p->first_seq;
    in.max_length = p->max_length ? p->max_length : b->h->meta.max_length ? b->h->meta.max_length : 1;
    uint64_t n_bytes = 0, n_err = 0;
    w.cur ^= 1; // (the set of the call before stays as it is)
    HostBuf &h_text = w.h_text[w.cur], &h_etext = w.h_etext[w.cur];
    format_lengths(w, in, timed, s, n_bytes, n_err);
    format_fill(w, in, timed, s, n_bytes, n_err);
    h_text.ensure(n_bytes ? n_bytes : 8);
    if (n_bytes) HIPCHECK(hipMemcpyAsync(h_text.p, w.text.p, n_bytes, hipMemcpyDeviceToHost, s));
    if (err) {
        h_etext.ensure(n_err ? n_err : 8);
        if (n_err) HIPCHECK(hipMemcpyAsync(h_etext.p, w.etext.p, n_err, hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    std::memset(out, 0, sizeof *out);
    out->n_reads = in.n_reads;
    out->n_bytes = n_bytes;
    out->n_err_bytes = n_err;
    out->read_offsets = w.h_roff[w.cur].as<uint64_t>();
    out->text = h_text.as<char>();
    out->err_text = err ? h_etext.as<char>() : nullptr;
    out->ms_format = timed ? format_ms(w) : 0;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_format_result(int device, const pgx_result *in_, const pgx_locations *loc, const pgx_format_params *p, char *text, uint64_t text_cap,
                                        uint64_t *read_offsets, uint64_t *n_bytes, char *err_text, uint64_t err_cap, uint64_t *n_err_bytes) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_format_result");
    // everything the arguments alone decide comes first: said with or without a device
    format_check_params(p, "pgx_format_result");
    const bool err = (p->flags & PGX_FORMAT_STDERR) != 0, locate = (p->flags & (PGX_FORMAT_LOCATE_POSITIONS | PGX_FORMAT_LOCATE_SEQS)) != 0;
    if (!in_ || !in_->mem_offsets || (in_->n_mems && !in_->mems) || !in_->pos_offsets || (in_->n_positions && !in_->positions) || (text_cap && !text) || !read_offsets ||
        !n_bytes || !n_err_bytes || (err && err_cap && !err_text))
        throw Error(PGX_ERR_ARG, "pgx_format_result: null argument (pos_offsets included: the text holds the positions of every MEM)");
    const uint64_t n = in_->n_reads, m = in_->n_mems, np = in_->n_positions;
    if (locate && (!loc || !loc->loc_offsets || (loc->n_values && !loc->values))) throw Error(PGX_ERR_ARG, "pgx_format_result: a locate flag without loc");
    if (locate && loc->n_mems != m) throw Error(PGX_ERR_ARG, "pgx_format_result: loc->n_mems differs from in->n_mems");
    if ((p->flags & PGX_FORMAT_LOCATE_POSITIONS) && !p->max_length) throw Error(PGX_ERR_ARG, "pgx_format_result: PGX_FORMAT_LOCATE_POSITIONS needs max_length");
    auto check_csr = [](const uint64_t *off, uint64_t cnt, uint64_t last, const char *name) { // the kernels index the arrays by these
        bool ok = off[0] == 0 && off[cnt] == last;
        for (uint64_t i = 0; ok && i < cnt; i++) ok = off[i] <= off[i + 1];
        if (!ok) throw Error(PGX_ERR_ARG, std::string("pgx_format_result: ") + name + " must start at 0, never decrease and end at the count of what it indexes");
    };
    check_csr(in_->mem_offsets, n, m, "mem_offsets");
    check_csr(in_->pos_offsets, m, np, "pos_offsets");
    if (locate) check_csr(loc->loc_offsets, m, loc->n_values, "loc_offsets");
    *n_bytes = *n_err_bytes = 0;
    use_device(device);
    struct FormatInput { // device copies of the input + the formatter's buffers, released on every way out
        DevBuf mem_off, mems, pos_off, positions, loc_off, values;
        FormatWork w;
        ~FormatInput() { release_all({&mem_off, &mems, &pos_off, &positions, &loc_off, &values}); w.release(); }
    } k;
    upload(k.mem_off, in_->mem_offsets, (n + 1) * 8);
    upload(k.mems, in_->mems, m * sizeof(pgx_mem));
    upload(k.pos_off, in_->pos_offsets, (m + 1) * 8);
    upload(k.positions, in_->positions, np * 8);
    FormatIn in{};
    in.flags = p->flags;
    if (locate) {
        upload(k.loc_off, loc->loc_offsets, (m + 1) * 8);
        upload(k.values, loc->values, loc->n_values * 8);
        in.loc_off = k.loc_off.as<uint64_t>();
        in.values = k.values.as<uint64_t>();
        in.n_values = loc->n_values;
    }
    in.mem_off = k.mem_off.as<uint64_t>();
    in.mems = k.mems.as<pgx_mem>();
    in.pos_off = k.pos_off.as<uint64_t>();
    in.positions = k.positions.as<uint64_t>();
    in.n_reads = n; in.n_mems = m; in.n_positions = np;
    in.first_seq = p->first_seq;
    in.max_length = p->max_length;
    hipStream_t s = nullptr;
    uint64_t total = 0, total_err = 0;
    format_lengths(k.w, in, false, s, total, total_err);
    *n_bytes = total;
    *n_err_bytes = total_err;
    std::memcpy(read_offsets, k.w.h_roff[k.w.cur].as<uint64_t>(), (n + 1) * 8);
    if (total > text_cap) throw Error(PGX_ERR_NOMEM, "pgx_format_result: the text takes " + std::to_string(total) + " bytes, text_cap is " + std::to_string(text_cap));
    if (err && total_err > err_cap)
        throw Error(PGX_ERR_NOMEM, "pgx_format_result: the stderr lines take " + std::to_string(total_err) + " bytes, err_cap is " + std::to_string(err_cap));
    format_fill(k.w, in, false, s, total, total_err);
    if (total) HIPCHECK(hipMemcpyAsync(text, k.w.text.p, total, hipMemcpyDeviceToHost, s));
    if (err && total_err) HIPCHECK(hipMemcpyAsync(err_text, k.w.etext.p, total_err, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

