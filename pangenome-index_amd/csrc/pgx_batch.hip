// pgx_batch.hip -- the pgx_batch object: uploads, pgx_batch_run, results, pgx_batch_locate, pgx_batch_read_hits, pgx_batch_read_place,
// pgx_batch_read_verify, pgx_batch_read_align, pgx_batch_read_walk.
//
// Pipeline of pgx_batch_run (one HIP stream, results stay on the device):
//   scan(cap)      -> slot offsets (worst-case MEMs per read: min(len, len - min_len + 1)); the slot buffer
//                     is bounded, larger batches run in chunks of consecutive reads
//   find_mems      -> MEM slots + per-read counts                      [dominant kernel, persistent grid]
//   scan(count)    -> CSR offsets ; compact slots -> dense MEM array in read order
//   tag_locate     -> per MEM run_nums + first item + size-class lists ; scans -> segment offsets
//   tag_small      -> <= 16 runs: gather + sort + unique in registers
//   tag_gather / tag_sort_unique / tag_sort_large -> listed bigger queries (identical large ones once)
//   scan ; tag_compact -> positions CSR
// The only host synchronisations are the scalar read-backs that size the next buffer.
#include <memory>
#include <string>
#include <thread>

#include "pgx_runtime_internal.hpp"

// ------------------------------------------------------------------------------------------
struct pgx_chunk { uint64_t r0, r1, slot_base, slots; }; // consecutive reads sharing one pass over the slot buffer

// the compact result form (pgx_batch_result_compact; pgx_compact_encode uses one of its own): grow-only like the other result buffers
struct CompactWork {
    DevBuf sizes, tab, bytes, scan_tmp; // padded bytes per block; block_offsets | block_first_mem | block_first_pos; the stream
    HostBuf h_tab, h_bytes;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // around the sizing kernel + scan, around the fill kernel
    void release() {
        DevBuf *all[] = {&sizes, &tab, &bytes, &scan_tmp};
        for (DevBuf *d : all) d->release();
        h_tab.release(); h_bytes.release();
        for (auto &e : ev)
            if (e) { (void)hipEventDestroy(e); e = nullptr; }
    }
};

// the text output (pgx_batch_format; pgx_format_result uses one of its own): grow-only like the other result buffers
struct FormatWork {
    // lengths and their scans per level: positions (plen -> pcum), located values (vlen -> vcum), MEMs (mlen -> mcum), reads (rlen -> roff = read_offsets;
    // elen -> eoff for the stderr lines); pbase / vbase: where a MEM's lists start (pgx_format_fill_mems_kernel); the text and the stderr lines
    DevBuf plen, pcum, vlen, vcum, mlen, mcum, rlen, roff, elen, eoff, pbase, vbase, text, etext, scan_tmp;
    // the host side, twice: pgx_batch_format alternates between the two sets, so the text of one call outlives the next call (a writer thread may
    // still be writing it); h_roff: read_offsets, and behind them the total of the stderr lines
    HostBuf h_roff[2], h_text[2], h_etext[2];
    int cur = 0; // the set the last call filled
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // around the length pass, around the fill pass
    void release() {
        DevBuf *all[] = {&plen, &pcum, &vlen, &vcum, &mlen, &mcum, &rlen, &roff, &elen, &eoff, &pbase, &vbase, &text, &etext, &scan_tmp};
        for (DevBuf *d : all) d->release();
        for (int i = 0; i < 2; i++) { h_roff[i].release(); h_text[i].release(); h_etext[i].release(); }
        for (auto &e : ev)
            if (e) { (void)hipEventDestroy(e); e = nullptr; }
    }
};

struct pgx_batch {
    pgx_index *h = nullptr;
    pgx_device_image *dimg = nullptr;
    int device = 0;
    hipStream_t own = nullptr; // non-blocking stream of this batch: its copies, and its kernels when the caller names no stream
    // second stream: the dense2 kernel over the reads with a byte outside A C G T, while the two-step kernel runs (pgx_classify_reads_kernel)
    hipStream_t side = nullptr;
    hipEvent_t ev_side[2] = {nullptr, nullptr};
    bool class_valid = false, class_ok = false; // read_flags / side_list / side_count describe the uploaded reads (ok: few enough such reads to list)
    uint64_t side_reads_est = 0;                 // about how many reads the second-stream launch serves (sizes its grid)
    uint64_t n_reads = 0, read_bytes = 0;
    HostBuf h_off[2];                // rebased host copy of the offsets (chunk planning; pinned: its upload runs at link speed), and the one being filled
    int h_off_cur = 0;
    const uint64_t *h_offsets() const { return h_off[h_off_cur].as<uint64_t>(); }
    std::vector<pgx_chunk> chunks;   // plan of the last run (reused while min_len / budget are unchanged)
    bool plan_valid = false, slot_off_valid = false;
    uint64_t slot_off_min_len = 0;
    uint64_t plan_min_len = 0, plan_budget = 0;
    DevBuf reads, offsets;
    // run state
    DevBuf slot_off, slots, mem_count, mem_off, mems, scan_tmp, counters, heavy_list, heavy_scratch, read_flags, side_list, side_count, packed, ovf_base;
    DevBuf up_side_ids, up_side_off, up_side_bytes; // pgx_batch_upload_packed: the listed reads as they arrive
    DevBuf fx_text, fx_tiles, fx_tile_base, fx_lines, fx_contrib, fx_rec, fx_out_off, fx_rec_idx, fx_offs, fx_scal, fx_scan_tmp; // pgx_batch_upload_text
    std::vector<uint64_t> h_side_off;
    hipEvent_t ev_up[2] = {nullptr, nullptr};        // around the device passes of an upload
    float ms_upload_passes = 0;                      // device time of the passes this upload needed before its first find_mems launch (pgx_timing.ms_per_upload adds the run's own)
    uint64_t last_ovf_used = 0; // arena slots the last run handed out (sizes the next arena)
    uint64_t max_read_len = 0; // longest read of the upload (sizes the LDS columns of the packed pairs kernel)
    TagWork tw;
    LocWork lw; // pgx_batch_locate
    CompactWork cw; // pgx_batch_result_compact
    FormatWork fw;  // pgx_batch_format
    HitsWork hw;    // pgx_batch_read_hits
    PlaceWork pw;   // pgx_batch_read_place
    VerifyWork vw;  // pgx_batch_read_verify
    AlignWork aw;   // pgx_batch_read_align
    WalkWork ww;    // pgx_batch_read_walk
    uint64_t n_mems = 0, n_positions = 0, n_ext = 0, n_tag_overflow = 0;
    bool ran = false, ran_tags = false;
    // speculative sizing (pgx_batch_run): what the last run with these parameters produced
    bool shape_valid = false;
    uint64_t shape_reads = 0, shape_min_len = 0, shape_min_occ = 0, last_mems = 0;
    bool shape_tags = false;
    uint32_t spec_runs = 0, spec_fallbacks = 0;
    // host copies
    HostBuf h_mem_off, h_mems, h_run_nums, h_pos_off, h_positions;
    // timing
    hipEvent_t ev[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // [8]: behind the first find_mems launch; [9]: before it, behind the passes a fresh upload needs
    bool timed = false;
    pgx_timing timing{};
};

static void batch_release(pgx_batch *b) {
    if (!b) return;
    if (hipSetDevice(b->device) == hipSuccess) {
        DevBuf *all[] = {&b->reads, &b->offsets, &b->slot_off, &b->slots, &b->mem_count, &b->mem_off, &b->mems, &b->scan_tmp,
                         &b->counters, &b->heavy_list, &b->heavy_scratch, &b->read_flags, &b->side_list, &b->side_count, &b->packed, &b->ovf_base,
                         &b->up_side_ids, &b->up_side_off, &b->up_side_bytes, &b->fx_text, &b->fx_tiles, &b->fx_tile_base, &b->fx_lines,
                         &b->fx_contrib, &b->fx_rec, &b->fx_out_off, &b->fx_rec_idx, &b->fx_offs, &b->fx_scal, &b->fx_scan_tmp};
        for (DevBuf *d : all) d->release();
        b->tw.release();
        b->lw.release();
        b->cw.release();
        b->fw.release();
        b->hw.release();
        b->pw.release();
        b->vw.release();
        b->aw.release();
        b->ww.release();
        HostBuf *hb[] = {&b->h_mem_off, &b->h_mems, &b->h_run_nums, &b->h_pos_off, &b->h_positions, &b->h_off[0], &b->h_off[1]};
        for (HostBuf *x : hb) x->release();
        for (auto &e : b->ev)
            if (e) { (void)hipEventDestroy(e); e = nullptr; }
        if (b->own) { (void)hipStreamDestroy(b->own); b->own = nullptr; }
        if (b->side) { (void)hipStreamDestroy(b->side); b->side = nullptr; }
        for (auto &e : b->ev_side)
            if (e) { (void)hipEventDestroy(e); e = nullptr; }
        for (auto &e : b->ev_up)
            if (e) { (void)hipEventDestroy(e); e = nullptr; }
    }
    delete b;
}

extern "C" void pgx_batch_free(pgx_batch *b) { batch_release(b); }

// the new reads have proved valid and their offsets lie in the spare host buffer: swap it in and forget what belonged to the reads before
// (both uploads call this only behind their last check: a refused upload leaves the batch as it was)
static void batch_reset_for_upload(pgx_batch *b, uint64_t n_reads, uint64_t max_read_len, uint64_t read_bytes) {
    b->h_off_cur ^= 1;
    b->n_reads = n_reads;
    b->ran = b->ran_tags = false;
    b->lw.valid = false;
    b->hw.valid = false;
    b->pw.valid = false;
    b->vw.valid = false;
    b->aw.valid = false;
    b->ww.valid = false;
    b->plan_valid = false;
    b->slot_off_valid = false;
    b->class_valid = false;
    b->ms_upload_passes = 0;
    b->max_read_len = max_read_len;
    b->read_bytes = read_bytes;
}

// (re)fill a batch: device buffers only ever grow, so a long-lived batch costs no allocation per call
// offsets: validated, rebased to 0 (host copy for the chunk planner, device copy for the kernels), longest read -- one pass over them
static void batch_take_offsets(pgx_batch *b, const uint64_t *offsets, uint64_t n_reads, const char *who) {
    const uint64_t lo = offsets[0];
    HostBuf &hb = b->h_off[b->h_off_cur ^ 1]; // (swapped in once the offsets have proved valid: a refused upload leaves the batch as it was)
    hb.ensure((n_reads + 1) * 8);
    uint64_t *ho = hb.as<uint64_t>();
    ho[0] = 0;
    // ten million offsets are ~15 ms of one core: slices on a few host threads (a fresh batch per step is bound by what its host thread does
    // between the device's work: bench.py fresh_batch)
    const unsigned nt = n_reads >= (1u << 20) ? 4u : 1u;
    uint64_t longest[4] = {0, 0, 0, 0};
    bool bad[4] = {false, false, false, false};
    auto slice = [&](unsigned t) {
        const uint64_t i0 = 1 + n_reads * t / nt, i1 = 1 + n_reads * (t + 1) / nt;
        uint64_t prev = offsets[i0 - 1], mx = 0;
        bool b_ = false;
        for (uint64_t i = i0; i < i1; i++) {
            const uint64_t o = offsets[i];
            b_ |= o < prev;
            mx = std::max(mx, o - prev);
            ho[i] = o - lo;
            prev = o;
        }
        longest[t] = mx; bad[t] = b_;
    };
    if (nt == 1) slice(0);
    else {
        std::thread th[3];
        for (unsigned t = 1; t < nt; t++) th[t - 1] = std::thread(slice, t);
        slice(0);
        for (unsigned t = 1; t < nt; t++) th[t - 1].join();
    }
    uint64_t mx = 0;
    for (unsigned t = 0; t < nt; t++) {
        if (bad[t]) throw Error(PGX_ERR_ARG, std::string(who) + ": offsets must be non-decreasing");
        mx = std::max(mx, longest[t]);
    }
    if (mx >= (1ull << 31)) throw Error(PGX_ERR_UNSUPPORTED, "read longer than 2^31 bytes");
    batch_reset_for_upload(b, n_reads, mx, offsets[n_reads] - lo);
    b->offsets.ensure((n_reads + 1) * 8);
    HIPCHECK(hipMemcpyAsync(b->offsets.p, ho, (n_reads + 1) * 8, hipMemcpyHostToDevice, b->own));
}

static void batch_upload(pgx_batch *b, const uint8_t *reads, const uint64_t *offsets, uint64_t n_reads) {
    batch_take_offsets(b, offsets, n_reads, "pgx_batch_upload");
    // device offsets are rebased to 0; 32 bytes of zero padding after the last read
    // copies go through the batch's own non-blocking stream: batches of other host threads (other streams of the same device)
    // are not serialised behind them the way copies on the legacy default stream would be
    b->reads.ensure(b->read_bytes + 32);
    HIPCHECK(hipMemsetAsync((uint8_t *)b->reads.p + b->read_bytes, 0, 32, b->own));
    if (b->read_bytes) HIPCHECK(hipMemcpyAsync(b->reads.p, reads + offsets[0], b->read_bytes, hipMemcpyHostToDevice, b->own));
    HIPCHECK(hipStreamSynchronize(b->own));
}

// the reads as the host packed them (pgx_pack_reads): a quarter of the bytes over the link, and neither pgx_bad_chunks_kernel nor
// pgx_classify_reads_kernel nor their read-back on the device -- the packed words, the flags and the side list the two-step kernel wants arrive
// ready; the bytes the other kernels read are rebuilt on the device (pgx_unpack_reads_kernel + the listed reads' own bytes over them)
static void batch_upload_packed(pgx_batch *b, const uint32_t *packed, const uint64_t *offsets, uint64_t n_reads, const uint64_t *side_ids,
                                const uint8_t *side_bytes, uint64_t n_side) {
    if (offsets[0] != 0) throw Error(PGX_ERR_ARG, "pgx_batch_upload_packed: offsets[0] must be 0 (word w of the packed stream holds symbols 16 w .. 16 w + 15)");
    if (n_side > n_reads) throw Error(PGX_ERR_ARG, "pgx_batch_upload_packed: more listed reads than reads");
    for (uint64_t k = 0; k < n_side; k++) // (before anything of the batch changes: a refused upload leaves it as it was)
        if (side_ids[k] >= n_reads || (k && side_ids[k] <= side_ids[k - 1])) throw Error(PGX_ERR_ARG, "pgx_batch_upload_packed: listed read ids must ascend and lie inside the batch");
    batch_take_offsets(b, offsets, n_reads, "pgx_batch_upload_packed");
    b->h_side_off.resize(n_side + 1);
    b->h_side_off[0] = 0;
    for (uint64_t k = 0; k < n_side; k++) b->h_side_off[k + 1] = b->h_side_off[k] + (offsets[side_ids[k] + 1] - offsets[side_ids[k]]);
    const uint64_t n_chunks = (b->read_bytes + 15) >> 4, side_total = b->h_side_off[n_side];
    hipStream_t s = b->own;
    b->packed.ensure((n_chunks + 64) * 4);
    b->reads.ensure(n_chunks * 16 + 32);
    b->read_flags.ensure(((n_reads + 3) & ~3ull) + 4);
    b->side_list.ensure((n_reads ? n_reads : 1) * sizeof(pgx_heavy_item));
    b->side_count.ensure(16);
    if (n_chunks) HIPCHECK(hipMemcpyAsync(b->packed.p, packed, n_chunks * 4, hipMemcpyHostToDevice, s));
    if (n_side) {
        b->up_side_ids.ensure(n_side * 8);
        b->up_side_off.ensure((n_side + 1) * 8);
        b->up_side_bytes.ensure(side_total ? side_total : 1);
        HIPCHECK(hipMemcpyAsync(b->up_side_ids.p, side_ids, n_side * 8, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(b->up_side_off.p, b->h_side_off.data(), (n_side + 1) * 8, hipMemcpyHostToDevice, s));
        if (side_total) HIPCHECK(hipMemcpyAsync(b->up_side_bytes.p, side_bytes, side_total, hipMemcpyHostToDevice, s));
    }
    for (auto &e : b->ev_up)
        if (!e) HIPCHECK(hipEventCreate(&e));
    HIPCHECK(hipEventRecord(b->ev_up[0], s));
    HIPCHECK(hipMemsetAsync(b->side_count.p, 0, 16, s));
    HIPCHECK(hipMemsetAsync(b->read_flags.p, 0, ((n_reads + 3) & ~3ull) + 4, s));
    if (n_chunks) {
        int cus = 0;
        HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        hipLaunchKernelGGL(pgx_unpack_reads_kernel, dim3(std::min<unsigned>(grid_for(n_chunks, 256), (unsigned)cus * 16u)), dim3(256), 0, s, b->packed.as<uint32_t>(), n_chunks,
                           b->reads.as<uint8_t>());
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipMemsetAsync((uint8_t *)b->reads.p + b->read_bytes, 0, 32, s)); // (the tail of the last word unpacks to 'A's)
    if (n_side) {
        hipLaunchKernelGGL(pgx_side_reads_kernel, dim3(grid_for(n_side * 64, 256)), dim3(256), 0, s, b->reads.as<uint8_t>(), b->offsets.as<uint64_t>(), b->up_side_ids.as<uint64_t>(),
                           b->up_side_off.as<uint64_t>(), b->up_side_bytes.as<uint8_t>(), n_side, b->read_flags.as<uint8_t>(), b->side_list.as<pgx_heavy_item>(),
                           b->side_count.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipEventRecord(b->ev_up[1], s));
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipEventElapsedTime(&b->ms_upload_passes, b->ev_up[0], b->ev_up[1]));
    b->class_valid = true; // what pgx_batch_run would otherwise find out with two passes over the bytes and a read-back
    b->class_ok = true;
    b->side_reads_est = n_side;
}

// reads as text (pgx.h, PGX_READS_*), parsed by the passes of pgx_fastx_kernels.hip on the batch's own stream.  Everything up to the
// validation goes into buffers of its own (text, line table, scans, the new offsets): a refused upload leaves the batch as it was.
// Two small read-backs: the newline count (sizes the line arrays), then error word / reads / bytes / longest read in one copy.
static void batch_upload_text(pgx_batch *b, const uint8_t *text, uint64_t n_bytes, uint32_t format, uint64_t *n_reads_out) {
    static const char *const fmt_name[3] = {"LINES", "FASTA", "FASTQ"};
    if (n_bytes >= (1ull << 40)) throw Error(PGX_ERR_UNSUPPORTED, "pgx_batch_upload_text: text of 2^40 bytes or more");
    if (n_bytes == 0) {
        static const uint64_t none[1] = {0};
        batch_upload(b, nullptr, none, 0);
        *n_reads_out = 0;
        return;
    }
    hipStream_t s = b->own;
    const uint64_t n_tiles = (n_bytes + PGX_FASTX_TILE - 1) / PGX_FASTX_TILE;
    b->fx_text.ensure(n_bytes + 64); // (a 16-byte load that starts before n_bytes stays inside)
    b->fx_tiles.ensure(n_tiles * 4);
    b->fx_tile_base.ensure((n_tiles + 1) * 8);
    b->fx_scal.ensure(64);
    unsigned long long *scal = b->fx_scal.as<unsigned long long>(); // [0] first error (line << 8 | code), [1] reads, [2] sequence bytes, [3] longest read
    HIPCHECK(hipMemcpyAsync(b->fx_text.p, text, n_bytes, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(scal, 0, 64, s));
    HIPCHECK(hipMemsetAsync(scal, 0xFF, 8, s));
    const uint8_t *dt = b->fx_text.as<uint8_t>();
    hipLaunchKernelGGL(pgx_fastx_count_kernel, dim3(grid_for(n_tiles, 1)), dim3(256), 0, s, dt, n_bytes, b->fx_tiles.as<uint32_t>());
    HIPCHECK(hipGetLastError());
    scan_excl(0, b->fx_tiles.p, n_tiles, 0, b->fx_tile_base.as<uint64_t>(), b->fx_scan_tmp, s);
    const uint64_t n_nl = read_u64(b->fx_tile_base.as<uint64_t>() + n_tiles, s);
    const uint32_t tail = text[n_bytes - 1] != '\n';
    const uint64_t n_lines = n_nl + tail;
    b->fx_lines.ensure((n_lines + 1) * 8);
    b->fx_contrib.ensure(n_lines * 4);
    b->fx_rec.ensure(n_lines);
    b->fx_out_off.ensure((n_lines + 1) * 8);
    b->fx_rec_idx.ensure((n_lines + 1) * 8);
    b->fx_offs.ensure((n_lines + 1) * 8); // (reads <= lines)
    uint64_t *ls = b->fx_lines.as<uint64_t>(), *out_off = b->fx_out_off.as<uint64_t>(), *rec_idx = b->fx_rec_idx.as<uint64_t>(), *offs = b->fx_offs.as<uint64_t>();
    hipLaunchKernelGGL(pgx_fastx_lines_kernel, dim3(grid_for(n_tiles, 1)), dim3(256), 0, s, dt, n_bytes, b->fx_tile_base.as<uint64_t>(), ls, n_lines, tail);
    hipLaunchKernelGGL(pgx_fastx_role_kernel, dim3(grid_for(n_lines, 256)), dim3(256), 0, s, dt, (const uint64_t *)ls, n_lines, format, b->fx_contrib.as<uint32_t>(),
                       b->fx_rec.as<uint8_t>(), scal);
    HIPCHECK(hipGetLastError());
    scan_excl(0, b->fx_contrib.p, n_lines, 0, out_off, b->fx_scan_tmp, s, reinterpret_cast<uint64_t *>(scal + 2));
    scan_excl(4, b->fx_rec.p, n_lines, 0, rec_idx, b->fx_scan_tmp, s, reinterpret_cast<uint64_t *>(scal + 1));
    hipLaunchKernelGGL(pgx_fastx_records_kernel, dim3(grid_for(n_lines, 256)), dim3(256), 0, s, n_lines, format, (const uint32_t *)b->fx_contrib.as<uint32_t>(),
                       (const uint8_t *)b->fx_rec.as<uint8_t>(), (const uint64_t *)out_off, (const uint64_t *)rec_idx, offs, scal);
    hipLaunchKernelGGL(pgx_fastx_longest_kernel, dim3(std::min<unsigned>(grid_for(n_lines, 256), 2048u)), dim3(256), 0, s, (const uint64_t *)offs, (const uint64_t *)(rec_idx + n_lines), scal + 3);
    HIPCHECK(hipGetLastError());
    uint64_t sc[4];
    read_scalars(sc, scal, 32, s);
    if (sc[0] != ~0ull) { // the first bad line: its start (and the neighbours the message needs) from the line table
        const uint64_t line = sc[0] >> 8, code = sc[0] & 0xFF, w0 = line >= 2 ? line - 2 : 0;
        uint64_t win[4] = {0, 0, 0, 0}, ri = 0;
        read_scalars(win, ls + w0, (line + 2 - w0) * 8, s);
        ri = read_u64(rec_idx + line, s);
        const uint64_t at = win[line - w0], len = win[line - w0 + 1] - 1 - at;
        const unsigned long long rec = format == PGX_READS_FASTQ ? line / 4 + 1 : format == PGX_READS_FASTA ? std::max<uint64_t>(ri, 1) : ri + 1;
        char msg[256];
        const char *f = fmt_name[format];
        auto stripped = [&](uint64_t a, uint64_t l) { return l - ((l && text[a + l - 1] == '\r') ? 1 : 0); };
        switch (code) {
        case PGX_FASTX_ERR_NO_AT: std::snprintf(msg, sizeof msg, "%s record %llu (byte %llu): header line does not start with '@'", f, rec, (unsigned long long)at); break;
        case PGX_FASTX_ERR_NO_PLUS: std::snprintf(msg, sizeof msg, "%s record %llu (byte %llu): third line does not start with '+'", f, rec, (unsigned long long)at); break;
        case PGX_FASTX_ERR_QUAL_LEN: {
            const uint64_t sa = win[line - 2 - w0], sl = win[line - 1 - w0] - 1 - sa;
            std::snprintf(msg, sizeof msg, "%s record %llu (byte %llu): quality length %llu != sequence length %llu", f, rec, (unsigned long long)at,
                          (unsigned long long)stripped(at, len), (unsigned long long)stripped(sa, sl));
            break;
        }
        case PGX_FASTX_ERR_TRUNCATED:
            std::snprintf(msg, sizeof msg, "%s record %llu (byte %llu): truncated record (%llu of 4 lines)", f, rec, (unsigned long long)at, (unsigned long long)(n_lines - line));
            break;
        case PGX_FASTX_ERR_BEFORE_FIRST: std::snprintf(msg, sizeof msg, "%s record 1 (byte %llu): text before the first '>'", f, (unsigned long long)at); break;
        default: std::snprintf(msg, sizeof msg, "%s record %llu (byte %llu): line of 2^31 bytes or more", f, rec, (unsigned long long)at); break;
        }
        throw Error(code == PGX_FASTX_ERR_LONG_LINE ? PGX_ERR_UNSUPPORTED : PGX_ERR_FORMAT, std::string("pgx_batch_upload_text: ") + msg);
    }
    const uint64_t n_reads = sc[1], total = sc[2], longest = sc[3];
    if (longest >= (1ull << 31)) throw Error(PGX_ERR_UNSUPPORTED, "read longer than 2^31 bytes");
    // valid: from here on the batch changes
    HostBuf &hb = b->h_off[b->h_off_cur ^ 1];
    hb.ensure((n_reads + 1) * 8);
    b->reads.ensure(total + 32);
    if (total) {
        hipLaunchKernelGGL(pgx_fastx_copy_kernel, dim3(grid_for(total, 4096)), dim3(256), 0, s, dt, (const uint64_t *)ls, (const uint64_t *)out_off, n_lines, total,
                           b->reads.as<uint8_t>());
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipMemsetAsync((uint8_t *)b->reads.p + total, 0, 32, s));
    std::swap(b->offsets, b->fx_offs);
    HIPCHECK(hipMemcpyAsync(hb.p, b->offsets.p, (n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    batch_reset_for_upload(b, n_reads, longest, total);
    *n_reads_out = n_reads;
}

extern "C" pgx_status pgx_batch_create(pgx_index *h, int device, const uint8_t *reads, const uint64_t *offsets,
                                       uint64_t n_reads, pgx_batch **out) {
    PGX_GUARD_BEGIN
    if (!h || !out || !offsets || (!reads && n_reads && offsets[n_reads] != offsets[0]))
        throw Error(PGX_ERR_ARG, "pgx_batch_create: null argument");
    if (!h->has_rank) throw Error(PGX_ERR_ARG, "pgx_batch_create: index opened without an r-index");
    *out = nullptr;
    pgx_device_image *dimg = device_image(h, device);
    ensure_lce(h, dimg);
    std::unique_ptr<pgx_batch, void (*)(pgx_batch *)> b(new pgx_batch(), batch_release);
    b->h = h;
    b->dimg = dimg;
    b->device = device;
    HIPCHECK(hipStreamCreateWithFlags(&b->own, hipStreamNonBlocking));
    batch_upload(b.get(), reads, offsets, n_reads);
    *out = b.release();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_upload(pgx_batch *b, const uint8_t *reads, const uint64_t *offsets, uint64_t n_reads) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_upload");
    if (!b || !offsets || (!reads && n_reads && offsets[n_reads] != offsets[0])) throw Error(PGX_ERR_ARG, "pgx_batch_upload: null argument");
    use_device(b->device);
    batch_upload(b, reads, offsets, n_reads);
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_upload_packed(pgx_batch *b, const uint32_t *packed, const uint64_t *offsets, uint64_t n_reads, const uint64_t *side_ids,
                                              const uint8_t *side_bytes, uint64_t n_side) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_upload_packed");
    if (!b || !offsets || (!packed && n_reads && offsets[n_reads] != offsets[0]) || (n_side && (!side_ids || !side_bytes)))
        throw Error(PGX_ERR_ARG, "pgx_batch_upload_packed: null argument");
    use_device(b->device);
    batch_upload_packed(b, packed, offsets, n_reads, side_ids, side_bytes, n_side);
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_upload_text(pgx_batch *b, const uint8_t *text, uint64_t n_bytes, uint32_t format, uint64_t *n_reads) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_upload_text");
    if (!b || !n_reads || (!text && n_bytes)) throw Error(PGX_ERR_ARG, "pgx_batch_upload_text: null argument");
    if (format > PGX_READS_FASTQ) throw Error(PGX_ERR_ARG, "pgx_batch_upload_text: unknown format " + std::to_string(format));
    use_device(b->device);
    batch_upload_text(b, text, n_bytes, format, n_reads);
    return PGX_OK;
    PGX_GUARD_END
}

// the reads as they lie on the device, whichever upload put them there (tests)
extern "C" pgx_status pgx_batch_reads(pgx_batch *b, pgx_reads_info *info, uint64_t *offsets, uint64_t offsets_cap, uint8_t *bytes, uint64_t bytes_cap) {
    PGX_GUARD_BEGIN
    if (!b || !info) throw Error(PGX_ERR_ARG, "pgx_batch_reads: null argument");
    info->n_reads = b->n_reads;
    info->n_bytes = b->read_bytes;
    info->longest = b->max_read_len;
    if ((offsets && offsets_cap < b->n_reads + 1) || (bytes && bytes_cap < b->read_bytes)) throw Error(PGX_ERR_ARG, "pgx_batch_reads: capacity too small");
    use_device(b->device);
    if (offsets) HIPCHECK(hipMemcpyAsync(offsets, b->offsets.p, (b->n_reads + 1) * 8, hipMemcpyDeviceToHost, b->own));
    if (bytes && b->read_bytes) HIPCHECK(hipMemcpyAsync(bytes, b->reads.p, b->read_bytes, hipMemcpyDeviceToHost, b->own));
    HIPCHECK(hipStreamSynchronize(b->own));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// pgx_batch_run

// Every environment variable a run consults, read once at the top of each pgx_batch_run call (per call, not per process: the tests change
// them between the runs of one process).  Each keeps the parse rule it always had.  The image-build knobs are read where the image is
// built (pgx_images.hip ImageKnobs), PGX_LOCATE_BUDGET_MB by pgx_batch_locate, PGX_ROCTX and PGX_SCAN_THREE once per process.
struct RunKnobs {
    bool spec;               // PGX_SPEC=0 clears it: no speculative sizing, every run reads its intermediate totals back
    bool arena;              // PGX_SLOT_ARENA=0 clears it: MEM slots in the worst-case layout, no arena for the fifth and later MEMs
    bool has_arena_cap;      // PGX_SLOT_ARENA_CAP is set, and
    uint64_t arena_cap;      //   its value (strtoull): arena capacity in slots before rounding (tests: an arena that overflows)
    uint64_t budget_slots;   // PGX_SLOT_BUDGET_MB (strtoull, at least 1), in slots: bound of the slot buffer; 0 = not set
    bool narrow;             // PGX_FM_NARROW=0 clears it: 64-bit interval state even where the 32-bit kernels would do
    bool force_redo;         // PGX_FM_NARROW_FORCE_REDO is set at all (tests): the first attempt of every chunk in 32 bits is repeated in 64, no speculation
    bool pairs;              // PGX_FM_PAIRS=0 clears it: the dense2 kernel alone, even where the index has a PAIRS image
    bool side;               // PGX_FM_NO_SIDE set at all clears it: no launch on the second stream, the pairs kernel serves every read
    bool packed;             // PGX_FM_PACKED=0 clears it: the pairs kernel reads byte windows, not two bits per symbol from LDS
    int coop;                // PGX_FM_COOP: 1 if it starts with '1', 0 if set to anything else, -1 if not set (then the size of the PAIRS image decides)
    bool lce;                // PGX_FM_LCE=0 clears it: no forward stages through the LCE image even where it exists
    bool has_wg_per_cu;      // PGX_FM_WG_PER_CU is set at all (switches the reads-per-lane rule off), and
    int wg_per_cu;           //   its value (atoi): resident workgroups per CU, applied where it lies in [1, occupancy)
    uint32_t heavy_ext;      // PGX_FM_HEAVY_EXT (strtoul; default PGX_FM_HEAVY_EXT): extensions on one read before its rest goes to the heavy-read kernel, 0 = never
    bool has_side_heavy_ext; // PGX_FM_SIDE_HEAVY_EXT is set, and
    uint32_t side_heavy_ext; //   its value (strtoul): the same threshold for the second-stream launch alone
    bool debug_counters;     // PGX_DEBUG_COUNTERS set at all: the run's device counters on stderr
    bool fm_stats;           // PGX_FM_STATS set at all: the lane statistics of a -DPGX_FM_STATS build on stderr
};

static RunKnobs read_run_knobs() {
    auto is_set = [](const char *name) { return std::getenv(name) != nullptr; };
    auto not_zero = [](const char *name) { const char *e = std::getenv(name); return !(e && e[0] == '0'); };
    RunKnobs k{};
    k.spec = not_zero("PGX_SPEC");
    k.arena = not_zero("PGX_SLOT_ARENA");
    if (const char *e = std::getenv("PGX_SLOT_ARENA_CAP")) { k.has_arena_cap = true; k.arena_cap = std::strtoull(e, nullptr, 10); }
    if (const char *e = std::getenv("PGX_SLOT_BUDGET_MB")) k.budget_slots = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10)) * (1ull << 20) / sizeof(pgx_mem);
    k.narrow = not_zero("PGX_FM_NARROW");
    k.force_redo = is_set("PGX_FM_NARROW_FORCE_REDO");
    k.pairs = not_zero("PGX_FM_PAIRS");
    k.side = !is_set("PGX_FM_NO_SIDE");
    k.packed = not_zero("PGX_FM_PACKED");
    k.coop = -1;
    if (const char *e = std::getenv("PGX_FM_COOP")) k.coop = e[0] == '1';
    k.lce = not_zero("PGX_FM_LCE");
    if (const char *e = std::getenv("PGX_FM_WG_PER_CU")) { k.has_wg_per_cu = true; k.wg_per_cu = std::atoi(e); }
    k.heavy_ext = PGX_FM_HEAVY_EXT;
    if (const char *e = std::getenv("PGX_FM_HEAVY_EXT")) k.heavy_ext = (uint32_t)std::strtoul(e, nullptr, 10);
    if (const char *e = std::getenv("PGX_FM_SIDE_HEAVY_EXT")) { k.has_side_heavy_ext = true; k.side_heavy_ext = (uint32_t)std::strtoul(e, nullptr, 10); }
    k.debug_counters = is_set("PGX_DEBUG_COUNTERS");
    k.fm_stats = is_set("PGX_FM_STATS");
    return k;
}

// The variants of pgx_find_mems_kernel the runtime launches, each named here and in the instantiation list of pgx_fm_kernels.hip (for the pairs kernel below:
// of pgx_pairs_kernels.hip), and nowhere else.
// Only images of up to 48 KiB are staged in LDS, and only the run-length and the 64-byte dense image are (pgx_images.hip device_image); the run-length image has
// neither a 32-bit form nor seeds, the wide dense2 image (kind 3) no 32-bit form.
// (nullptr: no such instance)
static const void *find_mems_entry(bool in_lds, uint32_t kind, bool narrow, bool seeded) {
    using K = const void *;
    static const K tab[2][4][2][2] = { // [image in LDS][image kind][32-bit state][seeded]
        {{{(K)pgx_find_mems_kernel<false, 0, false, false>, nullptr}, {nullptr, nullptr}},
         {{(K)pgx_find_mems_kernel<false, 1, false, false>, (K)pgx_find_mems_kernel<false, 1, false, true>},
          {(K)pgx_find_mems_kernel<false, 1, true, false>, (K)pgx_find_mems_kernel<false, 1, true, true>}},
         {{(K)pgx_find_mems_kernel<false, 2, false, false>, (K)pgx_find_mems_kernel<false, 2, false, true>},
          {(K)pgx_find_mems_kernel<false, 2, true, false>, (K)pgx_find_mems_kernel<false, 2, true, true>}},
         {{(K)pgx_find_mems_kernel<false, 3, false, false>, (K)pgx_find_mems_kernel<false, 3, false, true>}, {nullptr, nullptr}}},
        {{{(K)pgx_find_mems_kernel<true, 0, false, false>, nullptr}, {nullptr, nullptr}},
         {{(K)pgx_find_mems_kernel<true, 1, false, false>, (K)pgx_find_mems_kernel<true, 1, false, true>},
          {(K)pgx_find_mems_kernel<true, 1, true, false>, (K)pgx_find_mems_kernel<true, 1, true, true>}},
         {{nullptr, nullptr}, {nullptr, nullptr}},
         {{nullptr, nullptr}, {nullptr, nullptr}}}};
    return kind < 4 ? tab[in_lds][kind][narrow][seeded] : nullptr;
}

// pgx_timing.kernels: the coordinates of an instance in the table above
static uint32_t find_mems_bits(bool in_lds, uint32_t kind, bool narrow, bool seeded) {
    return PGX_KERNELS_FM | (seeded ? PGX_KERNELS_FM_SEEDED : 0u) | (narrow ? PGX_KERNELS_FM_NARROW : 0u) | (kind << PGX_KERNELS_FM_KIND_SHIFT) | (in_lds ? PGX_KERNELS_FM_LDS : 0u);
}

static const void *find_mems_variant(bool in_lds, uint32_t kind, bool narrow, bool seeded, uint32_t &bits) {
    if (kind == 0) seeded = false; // (no stage of the run-length kernel looks at a seed table)
    const void *f = find_mems_entry(in_lds, kind, narrow, seeded);
    if (!f) throw Error(PGX_ERR_UNSUPPORTED, "pgx_batch_run: no find_mems kernel for this image");
    bits = find_mems_bits(in_lds, kind, narrow, seeded);
    return f;
}

// The same for pgx_find_mems_pairs_kernel (always seeded).  The cooperative line fetches and the LCE path exist only with the packed reads,
// the LCE path only for narrow images without the cooperative fetches.
// (nullptr: no such instance)
static const void *find_mems_pairs_entry(bool wide, bool packed, bool coop, bool s64, bool lce) {
    using K = const void *;
    static const K plain[2][2] = { // [wide][stride 64]
        {(K)pgx_find_mems_pairs_kernel<false, false, false, false, false>, (K)pgx_find_mems_pairs_kernel<false, false, false, true, false>},
        {(K)pgx_find_mems_pairs_kernel<true, false, false, false, false>, (K)pgx_find_mems_pairs_kernel<true, false, false, true, false>}};
    static const K pack[2][2][2] = { // [wide][cooperative][stride 64]
        {{(K)pgx_find_mems_pairs_kernel<false, true, false, false, false>, (K)pgx_find_mems_pairs_kernel<false, true, false, true, false>},
         {(K)pgx_find_mems_pairs_kernel<false, true, true, false, false>, (K)pgx_find_mems_pairs_kernel<false, true, true, true, false>}},
        {{(K)pgx_find_mems_pairs_kernel<true, true, false, false, false>, (K)pgx_find_mems_pairs_kernel<true, true, false, true, false>},
         {(K)pgx_find_mems_pairs_kernel<true, true, true, false, false>, (K)pgx_find_mems_pairs_kernel<true, true, true, true, false>}}};
    static const K with_lce[2] = {(K)pgx_find_mems_pairs_kernel<false, true, false, false, true>, (K)pgx_find_mems_pairs_kernel<false, true, false, true, true>}; // [stride 64]
    if (lce) return (wide || !packed || coop) ? nullptr : with_lce[s64];
    if (!packed) return coop ? nullptr : plain[wide][s64];
    return pack[wide][coop][s64];
}

static uint32_t find_mems_pairs_bits(bool wide, bool packed, bool coop, bool s64, bool lce) {
    return PGX_KERNELS_PAIRS | (s64 ? PGX_KERNELS_PAIRS_S64 : 0u) | (coop ? PGX_KERNELS_PAIRS_COOP : 0u) | (packed ? PGX_KERNELS_PAIRS_PACKED : 0u) |
           (wide ? PGX_KERNELS_PAIRS_WIDE : 0u) | (lce ? PGX_KERNELS_PAIRS_LCE : 0u);
}

static const void *find_mems_pairs_variant(bool wide, bool packed, bool coop, bool s64, bool lce, uint32_t &bits) {
    const void *f = find_mems_pairs_entry(wide, packed, coop, s64, lce);
    if (!f && lce) throw Error(PGX_ERR_UNSUPPORTED, "pgx_batch_run: no LCE pairs kernel for this image");
    if (!f) throw Error(PGX_ERR_UNSUPPORTED, "pgx_batch_run: no cooperative pairs kernel without the packed reads");
    bits = find_mems_pairs_bits(wide, packed, coop, s64, lce);
    return f;
}

// every instance of the two tables, as pgx_timing.kernels names it (tests: what "all variants" means comes from here)
extern "C" uint32_t pgx_kernel_variants(uint32_t *out, uint32_t cap) {
    uint32_t n = 0;
    auto put = [&](uint32_t bits) { if (out && n < cap) out[n] = bits; n++; };
    for (int c = 0; c < 32; c++) {
        const bool in_lds = c & 16, narrow = c & 2, seeded = c & 1;
        const uint32_t kind = (c >> 2) & 3;
        if (find_mems_entry(in_lds, kind, narrow, seeded)) put(find_mems_bits(in_lds, kind, narrow, seeded));
    }
    for (int c = 0; c < 32; c++) {
        const bool wide = c & 16, packed = c & 8, coop = c & 4, s64 = c & 2, lce = c & 1;
        if (find_mems_pairs_entry(wide, packed, coop, s64, lce)) put(find_mems_pairs_bits(wide, packed, coop, s64, lce));
    }
    return n;
}

// what a run carries from stage to stage
struct RunCtx {
    pgx_batch *b;
    hipStream_t s;
    RunKnobs k;
    PgxDevImage img; // (a copy: the seed table is chosen per run)
    uint64_t n, min_len, min_occ;
    bool want_tags;
    unsigned long long *ctr = nullptr; // the device counters (PgxCounterSlot, pgx_device.h)
    // chosen once per pass
    bool spec = false, arena_on = false;
    uint64_t cm_cap = 0; // capacity of the MEM array of a speculative pass
    const void *kfn = nullptr, *kfn_wide = nullptr, *kfn_pairs = nullptr; // the kernel of the first attempt, its 64-bit form, the pairs kernel (or none)
    uint32_t kfn_bits = 0, kfn_pairs_bits = 0; // their instances, as pgx_timing.kernels names them
    size_t pairs_lds = 0;
    int cus = 0;
    // gathered over the pass
    bool fresh_work = false, fresh_mark = false; // the pass performs work only the first run after an upload needs (pgx_timing.ms_per_upload); event 9 recorded behind it
    uint64_t n_ext = 0;
    float ms_fm = 0, ms_cp = 0, ms_main = 0;     // per-chunk times of a timed run with several chunks
};

// the arguments the find_mems kernels of one attempt share (hipLaunchKernel takes their addresses)
struct FmArgs {
    PgxDevImage img;
    const uint8_t *reads;
    const uint64_t *off, *slot_off;
    uint64_t n, min_len, min_occ, base, first;
    pgx_mem *slots;
    uint32_t *cnt;
    unsigned long long *next, *cur;
    uint32_t hext, hcap;
    pgx_heavy_item *hlist;
    unsigned long long *hcount;
    uint32_t *ovf; // (indexed by read id; the buffer holds this chunk's reads)
    uint64_t ovf_cap;
};

static void record(pgx_batch *b, int i, hipStream_t s) {
    static const char *const stage[10] = {"pgx: run begins (classify, sizing)", "pgx: find_mems launches follow", "pgx: find_mems enqueued", "pgx: compaction enqueued",
                                          "pgx: tag locate enqueued", "pgx: tag gather enqueued", "pgx: tag sort/unique enqueued", "pgx: run enqueued", "pgx: main find_mems kernel enqueued",
                                          "pgx: per-upload passes enqueued"};
    if (roctx().on) roctx().mark(stage[i]);
    if (!b->timed) return;
    if (!b->ev[i]) HIPCHECK(hipEventCreate(&b->ev[i]));
    HIPCHECK(hipEventRecord(b->ev[i], s));
}

// Persistent grid of a find_mems launch over cn reads: as many workgroups as the device keeps resident (no inter-workgroup dependency exists, so
// any grid size is correct; this one avoids a tail of late blocks), at most PGX_FM_WG_PER_CU per CU where that is set.  Without it, kernels for which
// `few_suffice` (the dense and the packed ones) need little occupancy, and every resident lane ends the launch inside a read (the tail): they aim at
// >= 5 reads per lane, at least 2 workgroups per CU (1 M reads: 3 workgroups per CU measured best, 493 vs 477 (x) and 179 vs 160 (synth) Mreads/s).
static unsigned find_mems_grid(const RunCtx &r, const void *kfn, size_t lds, bool few_suffice, uint64_t cn) {
    int wg = 0;
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg, kfn, PGX_FM_THREADS, lds));
    if (wg < 1) wg = 1;
    if (r.k.has_wg_per_cu) {
        if (r.k.wg_per_cu >= 1 && r.k.wg_per_cu < wg) wg = r.k.wg_per_cu;
    } else if (few_suffice)
        wg = (int)std::min<uint64_t>((uint64_t)wg, std::max<uint64_t>(2, cn / (5ull * (uint64_t)r.cus * PGX_FM_THREADS)));
    return std::min(grid_for(cn, 64), (unsigned)(wg * r.cus));
}

// 1. worst-case MEM slots per read: cap = min(len, len - min_len + 1).  The slot buffer is bounded by a budget; batches whose worst case
//    exceeds it are processed in chunks of consecutive reads.  Offsets and plan are kept across runs.
static void plan_slots(RunCtx &r) {
    pgx_batch *b = r.b;
    const uint64_t n = r.n, min_len = r.min_len;
    b->slot_off.ensure((n + 1) * 8);
    if (!b->slot_off_valid || b->slot_off_min_len != min_len) { // depends on the reads and min_len only: kept across runs
        r.fresh_work = true;
        scan_excl(2, b->offsets.p, n, min_len, b->slot_off.as<uint64_t>(), b->scan_tmp, r.s);
        b->slot_off_valid = true;
        b->slot_off_min_len = min_len;
    }
    b->mem_count.ensure((n ? n : 1) * 4);
    b->mem_off.ensure((n + 1) * 8);
    // a quarter of the device's memory (72 GB of the MI355X's 288 GB: ten million 150-bp reads are one chunk), 16 GiB at least
    uint64_t budget_slots = (16ull << 30) / sizeof(pgx_mem);
    {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess) budget_slots = std::max<uint64_t>(budget_slots, (uint64_t)(mem_total / 4) / sizeof(pgx_mem));
        else (void)hipGetLastError();
    }
    if (r.k.budget_slots) budget_slots = r.k.budget_slots;
    if (!b->plan_valid || b->plan_min_len != min_len || b->plan_budget != budget_slots) { // cached across runs
        b->chunks.clear();
        uint64_t r0 = 0, base = 0, acc = 0;
        // the slots of a read never exceed its length: a batch whose bytes fit the budget is one chunk, no per-read loop
        if (n && b->read_bytes <= budget_slots) b->chunks.push_back({0, n, 0, std::max<uint64_t>(b->read_bytes, 1)});
        else {
            for (uint64_t i = 0; i < n; i++) {
                const uint64_t len = b->h_offsets()[i + 1] - b->h_offsets()[i];
                const uint64_t cap = len < min_len ? 0 : std::min<uint64_t>(len, len - min_len + 1);
                if (acc && acc + cap > budget_slots) { b->chunks.push_back({r0, i, base, acc}); r0 = i; base += acc; acc = 0; }
                acc += cap;
            }
            if (n) b->chunks.push_back({r0, n, base, acc});
        }
        b->plan_valid = true; b->plan_min_len = min_len; b->plan_budget = budget_slots;
    }
    uint64_t max_chunk_reads = 1;
    for (auto &c : b->chunks) max_chunk_reads = std::max(max_chunk_reads, c.r1 - c.r0);
    b->ovf_base.ensure(max_chunk_reads * 4);
}

// the kernels of the pass: kfn for the first attempt of a chunk, kfn_wide for its repeat in 64 bits, kfn_pairs where the pairs kernel runs
// (kfn then serves the reads it skips, on the second stream)
static void choose_kernels(RunCtx &r) {
    pgx_batch *b = r.b;
    const PgxDevImage &img = r.img;
    const bool in_lds = b->dimg->lds_bytes != 0;
    const bool seeded = img.seed_k != 0 && r.min_len >= img.seed_k; // (no stage of a shorter search has room for a seed)
    r.kfn = r.kfn_wide = find_mems_variant(in_lds, img.dense, false, seeded, r.kfn_bits);
    // 32-bit interval state for dense images of BWTs shorter than 2^30 (PGX_FM_NARROW=0 switches it off)
    bool c_fits = true; // C[] comes straight from the file: a (corrupt) value beyond 2^32 must not be truncated by the 32-bit state
    for (int i = 0; i < 8; i++) c_fits = c_fits && !(b->h->img.consts.C[i] >> 32);
    if (img.dense && img.dense != 3 && img.n < (1ull << 30) && c_fits && r.k.narrow) r.kfn = find_mems_variant(in_lds, img.dense, true, seeded, r.kfn_bits);
    // two extensions per cache line where the index has a PAIRS image (PGX_FM_PAIRS=0: the dense2 kernel alone)
    // (only behind the seed table: the wide intervals at the start of an unseeded stage always have special positions between their ends)
    r.kfn_pairs = nullptr;
    if (img.pairs && seeded && !(r.n >> 32) && b->read_bytes < (1ull << 35) && r.k.pairs)
        r.kfn_pairs = find_mems_pairs_variant(img.wide != 0, false, false, img.pairs_stride == PGX_PAIRS_STRIDE64, false, r.kfn_pairs_bits);
    r.pairs_lds = img.wide ? (size_t)img.n_sbp * 192 : 0; // (superblock bases of the wide form, behind the other dynamic LDS)
    HIPCHECK(hipDeviceGetAttribute(&r.cus, hipDeviceAttributeMultiprocessorCount, b->device));
}

// once per upload: which reads hold a byte outside A C G T (two small passes and one scalar read back), and the reads at two bits per symbol
static void classify_reads(RunCtx &r, uint64_t cn) {
    pgx_batch *b = r.b;
    hipStream_t s = r.s;
    r.fresh_work = true;
    const uint64_t cap = std::max<uint64_t>(cn, 1024); // chunks with such a byte; beyond that (lower-case reads, say) no side launch
    b->read_flags.ensure(((cn + 3) & ~3ull) + 4);
    b->side_list.ensure((cn ? cn : 1) * sizeof(pgx_heavy_item));
    b->side_count.ensure(16);
    b->scan_tmp.ensure(cap * 8);
    b->scan_tmp.scan_epoch = 0; // (the list overwrites the scans' tile words: the next scan clears the buffer)
    b->packed.ensure(((b->read_bytes + 15) / 16 + 64) * 4); // the reads as two bits per symbol (written by the same pass)
    HIPCHECK(hipMemsetAsync(b->side_count.p, 0, 16, s));
    HIPCHECK(hipMemsetAsync(b->read_flags.p, 0, ((cn + 3) & ~3ull) + 4, s));
    unsigned long long *d_bad = b->side_count.as<unsigned long long>() + 1;
    hipLaunchKernelGGL(pgx_bad_chunks_kernel, dim3(std::min<unsigned>(grid_for((b->read_bytes + 15) / 16, 256), (unsigned)r.cus * 16u)), dim3(256), 0, s,
                       (const uint8_t *)b->reads.as<uint8_t>(), b->read_bytes, b->scan_tmp.as<uint64_t>(), d_bad, cap, b->packed.as<uint32_t>());
    HIPCHECK(hipGetLastError());
    unsigned long long n_bad = 0;
    read_scalars(&n_bad, d_bad, sizeof n_bad, s);
    b->class_ok = n_bad <= cap;
    b->side_reads_est = n_bad / 4; // (a read that overlaps an N run holds a handful of such 16-byte chunks)
    if (b->class_ok && n_bad) {
        hipLaunchKernelGGL(pgx_classify_reads_kernel, dim3(grid_for(n_bad, 256)), dim3(256), 0, s, (const uint8_t *)b->reads.as<uint8_t>(),
                           (const uint64_t *)b->offsets.as<uint64_t>(), cn, (const uint64_t *)b->scan_tmp.as<uint64_t>(), (const unsigned long long *)d_bad, cap,
                           b->read_flags.as<uint32_t>(), b->side_list.as<pgx_heavy_item>(), b->side_count.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
    }
    b->class_valid = true;
}

// Reads with a byte outside A C G T cannot be seeded: they go to the other kernel (kf) at once, on a second stream next to the pairs kernel, which
// skips them (a read cut from an N run is a chain of thousands of extensions: behind the pairs kernel it was 1.5 ms of tail).
static void launch_side(RunCtx &r, FmArgs &a, const void *kf, unsigned grid) {
    pgx_batch *b = r.b;
    HIPCHECK(hipEventRecord(b->ev_side[0], r.s));
    HIPCHECK(hipStreamWaitEvent(b->side, b->ev_side[0], 0));
    const pgx_heavy_item *s_list = b->side_list.as<pgx_heavy_item>();
    const unsigned long long *s_count = b->side_count.as<unsigned long long>();
    unsigned long long *s_cur = r.ctr + PGX_CTR_SIDE_CURSOR;
    // (a lane of this launch walks its read alone, one dependent extension after the other next to the pairs kernel: the launch lasts as long
    //  as its longest chain, so its reads go to the heavy-read kernel -- every start position at once -- earlier than the main launch's)
    uint32_t s_hext = r.k.heavy_ext ? std::min<uint32_t>(r.k.heavy_ext, PGX_FM_SIDE_HEAVY_EXT) : 0u;
    if (r.k.has_side_heavy_ext) s_hext = r.k.side_heavy_ext;
    void *sargs[] = {&a.img, &a.reads, &a.off, &a.n, &a.min_len, &a.min_occ, &a.slot_off, &a.slots, &a.cnt, &a.next, &s_cur, &a.first, &a.base,
                     &s_hext, &a.hcap, &a.hlist, &a.hcount, &s_list, &s_count, &a.ovf, &a.ovf_cap};
    // one workgroup per CU next to the pairs kernel while these reads are few (0.4 % of the chr22 workload: 43 k reads, less than one per lane);
    // with many of them the launch was the longest thing in the step (5 % = 500 k reads, 7.6 per lane one after the other: 21.8 ms next
    // to a 17 ms pairs kernel): up to four per CU, two reads per lane (profiles/r04_n_read_share.txt)
    const uint64_t cus = (uint64_t)r.cus;
    const unsigned side_wgs = (unsigned)std::min<uint64_t>(4 * cus, std::max<uint64_t>(cus, b->side_reads_est / (2ull * PGX_FM_THREADS) + 1));
    HIPCHECK(hipLaunchKernel(kf, dim3(std::min<unsigned>(grid, side_wgs)), dim3(PGX_FM_THREADS), sargs, b->dimg->lds_bytes, b->side));
    b->timing.kernels |= r.kfn_bits | PGX_KERNELS_SIDE | (kf != r.kfn ? PGX_KERNELS_FM_REDO : 0u);
    HIPCHECK(hipEventRecord(b->ev_side[1], b->side));
}

// The pairs kernel over the chunk.  It takes the reads from LDS, two bits per symbol, when every read the launch serves is pure A C G T (skip: the
// others are skipped) and a thread's column stays small enough for four workgroups per CU (reads up to ~350 bp); PGX_FM_PACKED=0 switches that off.
static void launch_pairs(RunCtx &r, FmArgs &a, const uint8_t *skip, uint64_t cn, unsigned grid) {
    pgx_batch *b = r.b;
    const PgxDevImage &img = r.img;
    const void *kp = r.kfn_pairs;
    uint32_t kp_bits = r.kfn_pairs_bits;
    size_t plds = r.pairs_lds;
    const uint32_t *a_packed = nullptr;
    uint32_t a_pkw = 0;
    const uint32_t pkw = (uint32_t)((15 + b->max_read_len + 15) >> 4) + 1u; // words of the longest read at the worst phase + one of padding
    if (skip && pkw <= 24 && r.k.packed) {
        // cooperative line fetches (one address translation per line instead of five) for PAIRS images beyond the reach of the
        // translation caches, ~3 GB (profiles/r03_ubench_gather_loads_per_line.txt); PGX_FM_COOP=0 / 1 overrides
        const bool coop = r.k.coop >= 0 ? r.k.coop != 0 : b->h->img.pairs.size() > (3ull << 30);
        // forward stages over narrow intervals through the suffix array and the text (pgx_image.h "LCE image"; min_occ <= 1: the longest match decides)
        const bool lce = img.lce_sa && !coop && !img.wide && r.min_occ <= 1 && r.k.lce;
        kp = find_mems_pairs_variant(img.wide != 0, true, coop, img.pairs_stride == PGX_PAIRS_STRIDE64, lce, kp_bits);
        // per thread of the LCE kernel: a seed entry, a suffix array entry, sixteen common prefixes from any byte on (five dwords)
        const size_t lce_lds = lce ? (size_t)PGX_FM_THREADS * (16 + 4 + 20) : 0;
        a_packed = b->packed.as<uint32_t>();
        a_pkw = pkw;
        plds = (size_t)pkw * PGX_FM_THREADS * 4 + (coop ? (size_t)(PGX_FM_THREADS / 64) * 8192 : 0) + (img.wide ? (size_t)img.n_sbp * 192 : 0) + lce_lds;
        b->timing.pairs_reads = lce ? 4u : coop ? 3u : 2u;
        grid = find_mems_grid(r, kp, plds, true, cn);
    }
    // the kernel's one argument: what it reads of the image, and the launch (pgx_device.h)
    PgxPairsArgs p = {};
    p.pairs = img.pairs; p.seed = img.seed; p.seed_end = img.seed_end;
    p.lce_sa = img.lce_sa; p.lce_text = img.lce_text; p.lce_flags = img.lce_flags; p.lce_lcp = img.lce_lcp;
    p.reads = a.reads; p.slots = a.slots; p.mem_count = a.cnt;
    p.n = img.n; p.min_len = a.min_len; p.min_occ = a.min_occ;
    p.first_read = a.first; p.n_reads = a.n;
    p.seed_k = img.seed_k; p.seed_end_k = img.seed_end_k; p.lce_max = img.lce_max; p.refill_min = img.refill_min;
    p.pk_words = a_pkw; p.heavy_ext = a.hext; p.pairs_sb_shift = img.pairs_sb_shift; p.dense = img.dense;
    p.consts = img.consts; p.first_ext = img.first_ext; p.pbase = img.pbase; p.n_sbp = img.n_sbp;
    p.offsets = a.off; p.skip = skip; p.packed = a_packed;
    p.cursor = a.cur; p.ctr = a.next;
    p.slot_off = a.slot_off; p.slot_base = a.base; p.ovf_base = a.ovf; p.ovf_cap = a.ovf_cap;
    p.heavy_list = a.hlist; p.heavy_count = a.hcount; p.heavy_cap = a.hcap; p.d2_sb_shift = img.d2_sb_shift;
    p.blocks = img.blocks; p.exc = img.exc; p.sbase2 = img.sbase2;
    void *pargs[] = {&p};
    HIPCHECK(hipLaunchKernel(kp, dim3(grid), dim3(PGX_FM_THREADS), pargs, plds, r.s)); // (PGX_FM_THREADS: the kernel takes its LDS strides from it)
    b->timing.kernels |= kp_bits;
}

// arena for the fifth and later MEMs of a chunk's reads, in slots (0 = worst-case layout): sized from the last run of this batch, or eight slots per read
static uint64_t arena_slots(const RunCtx &r, const pgx_chunk &c) {
    const pgx_batch *b = r.b;
    if (!r.arena_on) return 0;
    const uint64_t cn = c.r1 - c.r0;
    uint64_t want = b->shape_valid && b->shape_reads == r.n && b->shape_min_len == r.min_len && b->chunks.size() == 1 ? with_slack(b->last_ovf_used) + 4096 : 8 * cn + 4096; // (first run of a shape: eight slots per read; chr22 scale asks for 2.6, the x fixture for 6.7)
    if (r.k.has_arena_cap) want = r.k.arena_cap; // tests: an arena that overflows
    want = std::max<uint64_t>(want, b->max_read_len + 1); // (an overflowing extent is parked at the start of the arena: it must fit)
    want = std::max<uint64_t>(want, (uint64_t)PGX_ARENA_SUBS * (b->max_read_len + 1)); // (every sub-arena must hold a parked extent)
    want = (want + PGX_ARENA_SUBS - 1) / PGX_ARENA_SUBS * PGX_ARENA_SUBS;
    return want < c.slots && want < (1ull << 32) ? want : 0; // otherwise the worst case is no bigger
}

// 2. the hot kernel over one chunk, repeated where it has to be: in the worst-case slot layout after the arena proved too small, in 64 bits after a
//    coordinate left 32.  Returns the chunk's MEM total (a speculative pass: the capacity; the total stays on the device), and in ovf_cap the arena
//    the last attempt used.
static uint64_t find_mems_chunk(RunCtx &r, size_t ci, uint64_t &ovf_cap) {
    pgx_batch *b = r.b;
    hipStream_t s = r.s;
    const pgx_chunk &c = b->chunks[ci];
    const uint64_t cn = c.r1 - c.r0;
    const bool one_chunk = b->chunks.size() == 1;
    const uint32_t heavy_ext = r.k.heavy_ext;
    const unsigned grid = find_mems_grid(r, r.kfn_pairs ? r.kfn_pairs : r.kfn, r.kfn_pairs ? r.pairs_lds : b->dimg->lds_bytes, r.img.dense != 0, cn);
    uint64_t *local = b->mem_off.as<uint64_t>() + c.r0; // local CSR offsets of this chunk (scratch until the global scan)
    const void *kf = r.kfn;
    ovf_cap = arena_slots(r, c);
    for (int attempt = 0;; attempt++) {
        b->slots.ensure(((ovf_cap ? ovf_cap : c.slots) + 4 * cn) * sizeof(pgx_mem));
        // per-chunk counters (slots below PGX_CTR_TAG0): extensions, cursors, heavy reads, 32-bit overflow flag, MEMs of the chunk
        if (ci || attempt) {
            HIPCHECK(hipMemsetAsync(r.ctr, 0, PGX_CTR_TAG0 * 8, s));
            HIPCHECK(hipMemsetAsync(r.ctr + PGX_CTR_ARENA0, 0, (PGX_CTR_ALL - PGX_CTR_ARENA0) * 8, s));
        }
        FmArgs a;
        a.img = r.img;
        a.reads = b->reads.as<uint8_t>();
        a.off = b->offsets.as<uint64_t>(); a.slot_off = b->slot_off.as<uint64_t>();
        a.n = c.r1; a.min_len = r.min_len; a.min_occ = r.min_occ; a.base = c.slot_base; a.first = c.r0;
        a.slots = b->slots.as<pgx_mem>();
        a.cnt = b->mem_count.as<uint32_t>();
        a.next = r.ctr; a.cur = r.ctr + PGX_CTR_CURSOR;
        a.hext = heavy_ext; a.hcap = PGX_FM_HEAVY_CAP;
        a.hlist = b->heavy_list.as<pgx_heavy_item>();
        a.hcount = r.ctr + PGX_CTR_HEAVY;
        a.ovf = b->ovf_base.as<uint32_t>() - c.r0;
        a.ovf_cap = ovf_cap;
        bool side_running = false;
        if (r.kfn_pairs) { // the pairs kernel; the kernel chosen for the first attempt (or its 64-bit form) serves the reads it skips
            const uint8_t *skip = nullptr;
            if (one_chunk && r.k.side) {
                if (!b->side) {
                    HIPCHECK(hipStreamCreateWithFlags(&b->side, hipStreamNonBlocking));
                    for (auto &e : b->ev_side) HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                }
                if (!b->class_valid) classify_reads(r, cn);
                record(b, 9, s); r.fresh_mark = true;
                if (b->class_ok) {
                    skip = b->read_flags.as<uint8_t>();
                    launch_side(r, a, kf, grid);
                    side_running = true;
                }
            }
            launch_pairs(r, a, skip, cn, grid);
        } else { // (without it the one kernel serves every read of the launch itself)
            const pgx_heavy_item *a_rlist = nullptr;
            const unsigned long long *a_rcount = nullptr;
            void *args[] = {&a.img, &a.reads, &a.off, &a.n, &a.min_len, &a.min_occ, &a.slot_off, &a.slots, &a.cnt, &a.next, &a.cur, &a.first, &a.base,
                            &a.hext, &a.hcap, &a.hlist, &a.hcount, &a_rlist, &a_rcount, &a.ovf, &a.ovf_cap};
            if (ci == 0 && attempt == 0) { record(b, 9, s); r.fresh_mark = true; }
            HIPCHECK(hipLaunchKernel(kf, dim3(grid), dim3(PGX_FM_THREADS), args, b->dimg->lds_bytes, s)); // one of the variants
            b->timing.kernels |= r.kfn_bits | (kf != r.kfn ? PGX_KERNELS_FM_REDO : 0u);
        }
        record(b, 8, s);
        if (side_running) HIPCHECK(hipStreamWaitEvent(s, b->ev_side[1], 0)); // the other stream's reads are done (they may have queued heavy reads)
        if (heavy_ext) { // the rest of reads that spent heavy_ext extensions (usually none: the launch then costs a few microseconds)
            b->timing.kernels |= PGX_KERNELS_HEAVY;
            if (b->dimg->lds_bytes)
                hipLaunchKernelGGL(pgx_find_mems_heavy_kernel<true>, dim3(PGX_FM_HEAVY_GRID), dim3(256), b->dimg->lds_bytes, s, r.img, a.reads, a.off,
                                   r.min_len, r.min_occ, a.slot_off, c.slot_base, a.slots, a.cnt, r.ctr, (const pgx_heavy_item *)a.hlist,
                                   (const unsigned long long *)a.hcount, (uint32_t)PGX_FM_HEAVY_CAP, b->heavy_scratch.as<PgxHeavyResult>(), c.r0, cn, a.ovf, a.ovf_cap);
            else
                hipLaunchKernelGGL(pgx_find_mems_heavy_kernel<false>, dim3(PGX_FM_HEAVY_GRID), dim3(256), 0, s, r.img, a.reads, a.off, r.min_len, r.min_occ,
                                   a.slot_off, c.slot_base, a.slots, a.cnt, r.ctr, (const pgx_heavy_item *)a.hlist,
                                   (const unsigned long long *)a.hcount, (uint32_t)PGX_FM_HEAVY_CAP, b->heavy_scratch.as<PgxHeavyResult>(), c.r0, cn, a.ovf, a.ovf_cap);
        }
        if (ovf_cap) hipLaunchKernelGGL(pgx_arena_demand_kernel, dim3(1), dim3(PGX_ARENA_SUBS), 0, s, r.ctr);
        HIPCHECK(hipGetLastError());
        b->timing.find_mems_launches++;
        record(b, 2, s);
        scan_excl(0, b->mem_count.as<uint32_t>() + c.r0, cn, 0, local, b->scan_tmp, s, reinterpret_cast<uint64_t *>(r.ctr + PGX_CTR_MEMS));
        if (r.spec) return r.cm_cap; // nothing is read back: the MEM total stays on the device
        unsigned long long cc[16];
        read_scalars(cc, r.ctr, sizeof cc, s);
        if (ovf_cap) b->last_ovf_used = cc[PGX_CTR_OVF_TOP]; // (what the reads asked for, whether or not it fitted: sizes the next arena)
        if (ovf_cap && cc[PGX_CTR_OVF_ABORT]) { ovf_cap = 0; continue; } // the arena was too small: once more in the worst-case layout
        const bool forced = attempt == 0 && kf != r.kfn_wide && r.k.force_redo; // tests
        if ((cc[PGX_CTR_OVF32] || forced) && kf != r.kfn_wide) { kf = r.kfn_wide; continue; } // a coordinate left 32 bits: repeat the chunk in 64 bits
        r.n_ext += cc[PGX_CTR_EXT];
        b->timing.heavy_reads += (uint32_t)std::min<unsigned long long>(cc[PGX_CTR_HEAVY], PGX_FM_HEAVY_CAP);
        b->timing.pairs_other_steps += (uint32_t)cc[PGX_CTR_REDO];
        return cc[PGX_CTR_MEMS];
    }
}

// 3. the chunk's slots -> the dense MEM array in read order, behind the mem_base MEMs of the chunks before
static void compact_chunk(RunCtx &r, const pgx_chunk &c, uint64_t cm, uint64_t mem_base, uint64_t ovf_cap) {
    pgx_batch *b = r.b;
    hipStream_t s = r.s;
    const uint64_t cn = c.r1 - c.r0;
    b->mems.ensure_keep((mem_base + cm ? mem_base + cm : 1) * sizeof(pgx_mem), mem_base * sizeof(pgx_mem));
    hipLaunchKernelGGL(pgx_compact_mems_kernel, dim3(grid_for(cn, 256)), dim3(256), 0, s, c.r0, cn, b->slot_off.as<uint64_t>(),
                       c.slot_base, b->slots.as<pgx_mem>(), b->mem_count.as<uint32_t>(), (const uint64_t *)(b->mem_off.as<uint64_t>() + c.r0), mem_base,
                       b->mems.as<pgx_mem>(), r.spec ? r.cm_cap : ~0ull, reinterpret_cast<uint64_t *>(r.ctr + PGX_CTR_ABORT),
                       (const uint32_t *)(b->ovf_base.as<uint32_t>() - c.r0), ovf_cap);
    HIPCHECK(hipGetLastError());
    record(b, 3, s);
    if (b->timed && b->chunks.size() > 1) { // events are reused per chunk: accumulate now
        HIPCHECK(hipStreamSynchronize(s));
        float t1 = 0, t2 = 0, t3 = 0;
        HIPCHECK(hipEventElapsedTime(&t1, b->ev[1], b->ev[2]));
        HIPCHECK(hipEventElapsedTime(&t2, b->ev[2], b->ev[3]));
        HIPCHECK(hipEventElapsedTime(&t3, b->ev[1], b->ev[8]));
        r.ms_fm += t1; r.ms_cp += t2; r.ms_main += t3;
    }
}

// 5. the one read-back of all counters behind the pass: the totals of a speculative pass (false: one of its capacities was too small, the pass
//    counts for nothing), the kernels' traffic counters, the shape the next run may assume, the stderr statistics and the times
static bool read_back(RunCtx &r, bool &force_worst) {
    pgx_batch *b = r.b;
    const size_t n_chunks = b->chunks.size();
    unsigned long long cnt[PGX_CTR_SLOTS];
    read_scalars(cnt, b->counters.p, sizeof cnt, r.s);
    if (r.spec) {
        b->spec_runs++;
        if (cnt[PGX_CTR_OVF_ABORT]) { force_worst = true; b->last_ovf_used = cnt[PGX_CTR_OVF_TOP]; } // (the arena sized from the last run overflowed: the next one is sized from this demand)
        if (r.k.debug_counters)
            std::fprintf(stderr, "[pgx] speculative run: abort flags %llu, 32-bit overflow %llu, arena overflow %llu (top %llu), MEMs %llu of capacity %llu\n", cnt[PGX_CTR_ABORT], cnt[PGX_CTR_OVF32],
                         cnt[PGX_CTR_OVF_ABORT], cnt[PGX_CTR_OVF_TOP], cnt[PGX_CTR_MEMS], (unsigned long long)r.cm_cap);
        if (cnt[PGX_CTR_ABORT] || cnt[PGX_CTR_OVF32] || cnt[PGX_CTR_OVF_ABORT] || cnt[PGX_CTR_MEMS] > r.cm_cap) { b->spec_fallbacks++; b->ran_tags = false; return false; } // a capacity was too small: once more, exactly
        b->last_ovf_used = cnt[PGX_CTR_OVF_TOP];
        b->n_mems = cnt[PGX_CTR_MEMS];
        r.n_ext = cnt[PGX_CTR_EXT];
        b->timing.heavy_reads = (uint32_t)std::min<unsigned long long>(cnt[PGX_CTR_HEAVY], PGX_FM_HEAVY_CAP);
        b->timing.pairs_other_steps = (uint32_t)cnt[PGX_CTR_REDO];
        if (r.want_tags) {
            TagWork &w = b->tw;
            const unsigned long long *tc = cnt + PGX_CTR_TAG0; // (scalars of tag_pipeline)
            w.last_big = tc[0]; w.last_large = tc[1]; w.last_largest = tc[2]; w.last_G = tc[3]; w.last_small = tc[5];
            w.last_rep = tc[6]; w.last_dup = tc[7]; w.last_P = tc[8];
            w.n_positions = tc[8];
            b->n_positions = tc[8];
        }
    }
    // the kernels' own traffic counters (accumulated over the chunks of the run)
    if (r.kfn_pairs) {
        b->timing.main_lines = cnt[PGX_CTR_PAIRS_LINES]; b->timing.main_seed_loads = cnt[PGX_CTR_PAIRS_SEEDS];
        b->timing.other_lines = cnt[PGX_CTR_FM_LINES]; b->timing.other_seed_loads = cnt[PGX_CTR_FM_SEEDS];
        b->timing.two_step_trips = cnt[PGX_CTR_PAIRS_TWO];
    } else { b->timing.main_lines = cnt[PGX_CTR_FM_LINES]; b->timing.main_seed_loads = cnt[PGX_CTR_FM_SEEDS]; }
    b->last_mems = b->n_mems;
    b->shape_valid = true; b->shape_reads = r.n; b->shape_min_len = r.min_len; b->shape_min_occ = r.min_occ; b->shape_tags = r.want_tags;
    if (cnt[PGX_CTR_ST_TRIPS] && r.k.fm_stats) // only a -DPGX_FM_STATS build of the kernels fills these (scripts/fm_stats.sh)
        std::fprintf(stderr, "[pgx] find_mems wave trips %llu, live lane-trips %llu (%.1f%% of lanes), longest wave %llu trips, extensions %llu\n", cnt[PGX_CTR_ST_TRIPS],
                     cnt[PGX_CTR_ST_LIVE], 100.0 * (double)cnt[PGX_CTR_ST_LIVE] / (64.0 * (double)cnt[PGX_CTR_ST_TRIPS]), cnt[PGX_CTR_ST_LONGEST], cnt[PGX_CTR_EXT]);
    if (cnt[PGX_CTR_ST_PAIR_TRIPS] && r.k.fm_stats)
        std::fprintf(stderr, "[pgx] pairs kernel wave trips %llu, live lane-trips %llu (%.1f%%), with two extensions %llu, waiting for a second block %llu, fresh %llu, extensions through the other image %llu\n",
                     cnt[PGX_CTR_ST_PAIR_TRIPS], cnt[PGX_CTR_ST_PAIR_LIVE], 100.0 * (double)cnt[PGX_CTR_ST_PAIR_LIVE] / (64.0 * (double)cnt[PGX_CTR_ST_PAIR_TRIPS]),
                     cnt[PGX_CTR_PAIRS_TWO], cnt[PGX_CTR_ST_PAIR_WAIT], cnt[PGX_CTR_ST_PAIR_FRESH], cnt[PGX_CTR_REDO]);
    if (cnt[PGX_CTR_ST_PAIR_T_TOTAL] && r.k.fm_stats)
        std::fprintf(stderr, "[pgx] pairs kernel clock ticks: %.1f%% of the waves' time in the refill loop (%llu of %llu), %llu trips with a refill round; waiting for the seed entry %.1f%%, then for the block line %.1f%%\n",
                     100.0 * (double)cnt[PGX_CTR_ST_PAIR_T_REFILL] / (double)cnt[PGX_CTR_ST_PAIR_T_TOTAL], cnt[PGX_CTR_ST_PAIR_T_REFILL], cnt[PGX_CTR_ST_PAIR_T_TOTAL], cnt[PGX_CTR_ST_PAIR_REFILLS],
                     100.0 * (double)cnt[PGX_CTR_ST_PAIR_T_SEED] / (double)cnt[PGX_CTR_ST_PAIR_T_TOTAL], 100.0 * (double)cnt[PGX_CTR_ST_PAIR_T_LINE] / (double)cnt[PGX_CTR_ST_PAIR_T_TOTAL]);
    if (r.k.debug_counters)
        std::fprintf(stderr, "[pgx] counters: extensions %llu tag overflows %llu heavy %llu other-image steps %llu lines %llu + %llu seeds %llu + %llu\n", cnt[PGX_CTR_EXT], cnt[PGX_CTR_TAG_OVERFLOW],
                     cnt[PGX_CTR_HEAVY], cnt[PGX_CTR_REDO], cnt[PGX_CTR_PAIRS_LINES], cnt[PGX_CTR_FM_LINES], cnt[PGX_CTR_PAIRS_SEEDS], cnt[PGX_CTR_FM_SEEDS]);
    b->n_ext = r.n_ext;
    b->n_tag_overflow = cnt[PGX_CTR_TAG_OVERFLOW];
    if (b->timed) {
        auto el = [&](int a, int c) { float ms = 0; HIPCHECK(hipEventElapsedTime(&ms, b->ev[a], b->ev[c])); return ms; };
        b->timing.ms_find_mems = n_chunks > 1 ? r.ms_fm : el(1, 2);
        b->timing.ms_find_mems_main = n_chunks > 1 ? r.ms_main : (r.n ? el(1, 8) : 0.0f);
        b->timing.ms_compact = n_chunks > 1 ? r.ms_cp : el(2, 3);
        if (r.want_tags) {
            b->timing.ms_tag_locate = el(3, 4); // locate + scans
            b->timing.ms_tag_gather = el(4, 5); // 16-lane small path (gather + sort + unique)
            b->timing.ms_tag_sort = el(5, 6);   // big path + final scan + compaction
        }
        b->timing.ms_total = el(0, 7);
        // what a fresh batch pays before its first find_mems launch (one chunk on the side-stream path: where the passes are)
        if (r.fresh_work) b->timing.ms_per_upload = b->ms_upload_passes + (r.fresh_mark ? el(0, 9) : 0.0f);
    }
    if (r.fresh_work) b->ms_upload_passes = 0; // (reported once)
    return true;
}

// One pass over the batch: scan(cap) -> find_mems -> scan(count) + compact, per chunk -> tag stage -> read-back.
// Speculative sizing: a run normally reads a few scalars back in mid-flight (MEM total, tag-stage totals) because they size
// the next buffers -- each a host synchronisation with the device idle meanwhile.  When the previous run of this batch had the
// same shape (reads, min_len, min_occ, tags), the buffers and grids are sized from ITS totals (+ 25 %), all counts stay on the
// device, capacity checks raise an abort flag there, and the host reads everything once at the end; if the flag came up (or the
// 32-bit state overflowed) the pass returns false and the run is repeated in exact mode.  PGX_SPEC=0 switches it off.
// force_worst: the arena of the speculative pass overflowed, the exact pass uses the worst-case slot layout.
static bool run_pass(RunCtx &r, bool may_speculate, bool &force_worst) {
    pgx_batch *b = r.b;
    hipStream_t s = r.s;
    b->n_mems = b->n_positions = b->n_ext = b->n_tag_overflow = 0;
    std::memset(&b->timing, 0, sizeof b->timing);
    r.fresh_work = r.fresh_mark = false;
    r.n_ext = 0;
    r.ms_fm = r.ms_cp = r.ms_main = 0;
    b->counters.ensure(PGX_CTR_ALL * 8); // layout: PgxCounterSlot (pgx_device.h)
    HIPCHECK(hipMemsetAsync(b->counters.p, 0, PGX_CTR_ALL * 8, s));
    r.ctr = b->counters.as<unsigned long long>();

    record(b, 0, s);
    plan_slots(r);
    const std::vector<pgx_chunk> &chunks = b->chunks;
    // The slot buffer: a dense array of the first four MEMs of every read (PGX_FAST_SLOTS, pgx_slots_device.h pgx_slot_index) + either an ARENA for the
    // fifth and later MEMs (arena_slots), or -- PGX_SLOT_ARENA=0, tiny batches, and the repeat of a chunk whose arena proved too small -- the
    // worst-case region.  Sized per chunk.
    r.arena_on = r.k.arena && !force_worst;
    r.kfn = r.kfn_wide = r.kfn_pairs = nullptr;
    r.cus = 0;
    if (r.n) choose_kernels(r);
    if (r.k.heavy_ext) {
        b->heavy_list.ensure((size_t)PGX_FM_HEAVY_CAP * sizeof(pgx_heavy_item));
        b->heavy_scratch.ensure((size_t)PGX_FM_HEAVY_GRID * PGX_FM_HEAVY_MAXLEN * sizeof(PgxHeavyResult));
    }
    r.spec = may_speculate && chunks.size() == 1 && b->shape_valid && b->shape_reads == r.n && b->shape_min_len == r.min_len && b->shape_min_occ == r.min_occ &&
             b->shape_tags == r.want_tags && (!r.want_tags || (b->tw.have_last && b->tw.last_largest <= PGX_SORT_WG_LDS_CAP)) && r.k.spec && !r.k.force_redo;
    r.cm_cap = with_slack(b->last_mems);
    uint64_t mem_base = 0;
    for (size_t ci = 0; ci < chunks.size(); ci++) {
        record(b, 1, s);
        uint64_t ovf_cap = 0;
        const uint64_t cm = find_mems_chunk(r, ci, ovf_cap);
        compact_chunk(r, chunks[ci], cm, mem_base, ovf_cap);
        mem_base += cm;
    }
    b->n_mems = mem_base;
    if (!r.kfn_pairs) b->timing.pairs_reads = 0u;
    else if (!b->timing.pairs_reads) b->timing.pairs_reads = 1u; // (2 / 3 / 4 when the launch used the packed reads / the cooperative fetches / the LCE image too)
    b->timing.seed_depth = (r.img.seed_k != 0 && r.min_len >= r.img.seed_k && r.img.dense) ? r.img.seed_k : 0u;
    if (chunks.size() != 1) { // global CSR offsets (a single chunk's local offsets already are global)
        if (chunks.empty()) { record(b, 1, s); record(b, 2, s); }
        scan_excl(0, b->mem_count.p, r.n, 0, b->mem_off.as<uint64_t>(), b->scan_tmp, s);
        b->mems.ensure_keep((b->n_mems ? b->n_mems : 1) * sizeof(pgx_mem), b->n_mems * sizeof(pgx_mem));
        record(b, 3, s);
    }
    record(b, 3, s);
    // 4. tag queries (find_mems.cpp:129)
    if (r.want_tags) {
        tag_pipeline(r.img, b->mems.as<pgx_mem>(), nullptr, nullptr, b->n_mems, b->tw, r.ctr + PGX_CTR_TAG_OVERFLOW, r.ctr + PGX_CTR_TAG0, s,
                     [&](int stage) { record(b, 4 + stage, s); }, r.spec, reinterpret_cast<const uint64_t *>(r.ctr + PGX_CTR_MEMS),
                     reinterpret_cast<uint64_t *>(r.ctr + PGX_CTR_ABORT));
        b->n_positions = b->tw.n_positions;
        b->ran_tags = true;
    }
    record(b, 7, s);
    return read_back(r, force_worst);
}

extern "C" pgx_status pgx_batch_run(pgx_batch *b, uint64_t min_len, uint64_t min_occ, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_run");
    if (!b) throw Error(PGX_ERR_ARG, "pgx_batch_run: null batch");
    use_device(b->device);
    RunCtx r{b, stream ? (hipStream_t)stream : b->own, read_run_knobs(), b->dimg->img, b->n_reads, min_len, min_occ, (flags & PGX_RUN_TAGS) != 0};
    // seeds need min_len >= their depth (no stage of a shorter search has room for one): the shallower table serves searches below the depth of the first
    PgxDevImage &img = r.img;
    if (img.seed_k_main && min_len < img.seed_k_main && img.seed_k_small && min_len >= img.seed_k_small) { img.seed = img.seed_small; img.seed_k = img.seed_k_small; }
    if (r.want_tags && !b->h->has_tags) throw Error(PGX_ERR_ARG, "pgx_batch_run: PGX_RUN_TAGS without a tag array");
    b->timed = (flags & PGX_RUN_TIMING) != 0;
    b->ran = false;
    b->ran_tags = false;
    b->lw.valid = false; // (the locate result belongs to the run before)
    b->hw.valid = false; // (and so do the hits)
    b->pw.valid = false; // (and the places)
    b->vw.valid = false; // (and what was verified at them)
    b->aw.valid = false; // (and aligned there)
    b->ww.valid = false; // (and walked through the graph)
    b->n_mems = b->n_positions = b->n_ext = b->n_tag_overflow = 0;
    std::memset(&b->timing, 0, sizeof b->timing);
    bool force_worst = false;
    if (!run_pass(r, true, force_worst)) run_pass(r, false, force_worst); // (a speculative pass, then at most one exact pass)
    b->ran = true;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_device_result(pgx_batch *b, pgx_device_result *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_device_result: batch has not been run");
    std::memset(out, 0, sizeof *out);
    out->n_reads = b->n_reads;
    out->n_mems = b->n_mems;
    out->mem_offsets = b->mem_off.as<uint64_t>();
    out->mems = b->mems.as<pgx_mem>();
    if (b->ran_tags) {
        out->n_positions = b->n_positions;
        out->tag_run_counts = b->tw.run_nums.as<uint64_t>();
        out->pos_offsets = b->tw.pos_off.as<uint64_t>();
        out->positions = b->tw.positions.as<uint64_t>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_counts(pgx_batch *b, uint64_t *n_mems, uint64_t *n_positions, uint64_t *n_extensions) {
    PGX_GUARD_BEGIN
    if (!b || !b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_counts: batch has not been run");
    if (n_mems) *n_mems = b->n_mems;
    if (n_positions) *n_positions = b->n_positions;
    if (n_extensions) *n_extensions = b->n_ext;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_spec_stats(pgx_batch *b, uint32_t *speculative_runs, uint32_t *fallbacks) {
    PGX_GUARD_BEGIN
    if (!b) throw Error(PGX_ERR_ARG, "pgx_batch_spec_stats: null batch");
    if (speculative_runs) *speculative_runs = b->spec_runs;
    if (fallbacks) *fallbacks = b->spec_fallbacks;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_timing(pgx_batch *b, pgx_timing *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_timing: batch has not been run");
    if (!b->timed) throw Error(PGX_ERR_ARG, "pgx_batch_timing: run without PGX_RUN_TIMING");
    *out = b->timing;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_result(pgx_batch *b, pgx_result *out) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_result");
    if (!b || !out || !b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_result: batch has not been run");
    use_device(b->device);
    const uint64_t n = b->n_reads, m = b->n_mems;
    b->h_mem_off.ensure((n + 1) * 8);
    HIPCHECK(hipMemcpyAsync(b->h_mem_off.p, b->mem_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, b->own));
    b->h_mems.ensure((m ? m : 1) * sizeof(pgx_mem));
    if (m) HIPCHECK(hipMemcpyAsync(b->h_mems.p, b->mems.p, m * sizeof(pgx_mem), hipMemcpyDeviceToHost, b->own));
    std::memset(out, 0, sizeof *out);
    out->n_reads = n;
    out->n_mems = m;
    out->mem_offsets = b->h_mem_off.as<uint64_t>();
    out->mems = b->h_mems.as<pgx_mem>();
    out->n_extensions = b->n_ext;
    if (b->ran_tags) {
        b->h_run_nums.ensure((m ? m : 1) * 8);
        b->h_pos_off.ensure((m + 1) * 8);
        b->h_positions.ensure((b->n_positions ? b->n_positions : 1) * 8);
        if (m) HIPCHECK(hipMemcpyAsync(b->h_run_nums.p, b->tw.run_nums.p, m * 8, hipMemcpyDeviceToHost, b->own));
        HIPCHECK(hipMemcpyAsync(b->h_pos_off.p, b->tw.pos_off.p, (m + 1) * 8, hipMemcpyDeviceToHost, b->own));
        if (b->n_positions) HIPCHECK(hipMemcpyAsync(b->h_positions.p, b->tw.positions.p, b->n_positions * 8, hipMemcpyDeviceToHost, b->own));
        out->tag_run_counts = b->h_run_nums.as<uint64_t>();
        out->pos_offsets = b->h_pos_off.as<uint64_t>();
        out->positions = b->h_positions.as<uint64_t>();
        out->n_positions = b->n_positions;
        out->n_tag_overflow = b->n_tag_overflow;
    }
    HIPCHECK(hipStreamSynchronize(b->own)); // (the run itself completed inside pgx_batch_run, on whatever stream it used)
    return PGX_OK;
    PGX_GUARD_END
}

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
    struct Work { // device copies of the input + the encoder's buffers, released on every way out
        DevBuf mem_off, mems, run_nums, pos_off, positions;
        CompactWork w;
        ~Work() {
            DevBuf *all[] = {&mem_off, &mems, &run_nums, &pos_off, &positions};
            for (DevBuf *d : all) d->release();
            w.release();
        }
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
    struct Work { // device copies of the input + the formatter's buffers, released on every way out
        DevBuf mem_off, mems, pos_off, positions, loc_off, values;
        FormatWork w;
        ~Work() {
            DevBuf *all[] = {&mem_off, &mems, &pos_off, &positions, &loc_off, &values};
            for (DevBuf *d : all) d->release();
            w.release();
        }
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

// ------------------------------------------------------------------------------------------
// pgx_batch_locate (pgx_mem_locate_kernels.hip): the occurrences of the last run's MEMs, on the device
// values one pass of the intermediate buffer may hold: PGX_LOCATE_BUDGET_MB (fractions allowed), default a quarter of free device memory
static uint64_t locate_budget_values() {
    uint64_t bytes = 0;
    if (const char *e = std::getenv("PGX_LOCATE_BUDGET_MB")) {
        const double mb = std::strtod(e, nullptr);
        if (mb > 0) bytes = (uint64_t)(mb * 1048576.0);
    }
    if (!bytes) {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); mem_free = 1ull << 30; }
        bytes = mem_free / 4;
    }
    return std::max<uint64_t>(bytes / 8, 1);
}

// PGX_LOCATE_SETS=0 (read per call): PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE by the segmented sort even where the sequence sets would serve it
static bool locate_sets_enabled() {
    const char *e = std::getenv("PGX_LOCATE_SETS");
    return !(e && e[0] == '0' && e[1] == 0);
}

extern "C" pgx_status pgx_batch_locate(pgx_batch *b, uint32_t flags, uint64_t max_occ, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_locate");
    if ((flags & PGX_LOCATE_SEQ_SETS) && (flags & (PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE))) // (a contradiction in the call itself: said with or without a device)
        throw Error(PGX_ERR_ARG, "pgx_batch_locate: PGX_LOCATE_SEQ_SETS goes with PGX_LOCATE_CHAINS alone");
    checked_device_count();
    if (!b) throw Error(PGX_ERR_ARG, "pgx_batch_locate: null batch");
    if (flags & ~(PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE | PGX_LOCATE_CHAINS | PGX_LOCATE_SEQ_SETS)) throw Error(PGX_ERR_ARG, "pgx_batch_locate: unknown flag");
    if (!b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_locate: batch has not been run");
    LocWork &w = b->lw;
    w.valid = false;
    locate_check_supported(b->h, "pgx_batch_locate");
    use_device(b->device);
    pgx_device_image *d = locate_image(b->h, b->device);
    hipStream_t s = stream ? (hipStream_t)stream : b->own;
    const uint64_t n = b->n_mems, bwt_n = d->loc.n;
    const bool sets_form = (flags & PGX_LOCATE_SEQ_SETS) != 0;
    const bool seq_ids = sets_form || (flags & PGX_LOCATE_SEQ_IDS) != 0, uniq = (flags & PGX_LOCATE_UNIQUE) != 0;
    // sequence sets: the result itself (PGX_LOCATE_SEQ_SETS), or what the sorted unique sequence ids are expanded from (routed) in place of the sort
    const uint64_t n_seq = b->h->meta.n_sequences();
    const uint64_t W = (n_seq + 63) / 64;
    const bool sets_fit = W >= 1 && W <= PGX_ML_SET_WORDS_MAX;
    if (sets_form && !sets_fit)
        throw Error(PGX_ERR_UNSUPPORTED, "pgx_batch_locate: PGX_LOCATE_SEQ_SETS serves at most " + std::to_string(64 * PGX_ML_SET_WORDS_MAX) + " sequences, the index has " +
                                             std::to_string(n_seq));
    const bool routed = !sets_form && seq_ids && uniq && sets_fit && locate_sets_enabled();
    const bool build_sets = sets_form || routed, sort_uniq = uniq && !routed;
    // the resident suffix array: the LCE image in text coordinates and its sequence starts (built from this very locate image's chains)
    const bool resident = !(flags & PGX_LOCATE_CHAINS) && d->lce_state == 1 && d->img.lce_sa && d->lce_seq_start.p && d->lce_n_seq && d->img.n == bwt_n;
    const bool timed = b->timed;
    if (timed) {
        for (auto &e : w.ev)
            if (!e) HIPCHECK(hipEventCreate(&e));
        HIPCHECK(hipEventRecord(w.ev[0], s));
    }
    // 1. plan: counts (cap, range checks), ranges, not-located total; value offsets
    //    ctr: [0] wave list [1] workgroup list [2] scratch total [3] unique values of a pass [4] not located [5] values [6..7] cut
    w.cnt.ensure((n ? n : 1) * 8); w.qs.ensure((n ? n : 1) * 8); w.qe.ensure((n ? n : 1) * 8); w.voff.ensure((n + 1) * 8); w.ctr.ensure(64);
    unsigned long long *ctr = w.ctr.as<unsigned long long>();
    HIPCHECK(hipMemsetAsync(w.ctr.p, 0, 64, s));
    if (n) {
        hipLaunchKernelGGL(pgx_ml_plan_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const pgx_mem *)b->mems.as<pgx_mem>(), n, bwt_n, max_occ,
                           w.cnt.as<uint64_t>(), w.qs.as<uint64_t>(), w.qe.as<uint64_t>(), ctr + 4);
        HIPCHECK(hipGetLastError());
    }
    scan_excl(1, w.cnt.p, n, 0, w.voff.as<uint64_t>(), w.scan_tmp, s, reinterpret_cast<uint64_t *>(ctr + 5));
    uint64_t tot[2];
    read_scalars(tot, ctr + 4, 16, s);
    const uint64_t n_not = tot[0], V = tot[1];
    const uint64_t *voff = w.voff.as<uint64_t>();
    // 2. passes over consecutive MEMs whose values fit the budget (one pass unless the batch exceeds it)
    const uint64_t budget = locate_budget_values();
    if (sets_form) { // the result: n x W words, cleared once; loc_offsets[m] = m * W
        w.vals.ensure((n ? n * W : 1) * 8); w.uoff.ensure((n + 1) * 8);
        if (n) HIPCHECK(hipMemsetAsync(w.vals.p, 0, n * W * 8, s));
        hipLaunchKernelGGL(pgx_ml_stride_kernel, dim3(grid_for(n + 1, 256)), dim3(256), 0, s, w.uoff.as<uint64_t>(), n + 1, W);
        HIPCHECK(hipGetLastError());
    } else if (!uniq) w.vals.ensure((V ? V : 1) * 8); // (the values are written in place: no intermediate buffer)
    else { w.ucount.ensure((n ? n : 1) * 8); w.uoff.ensure((n + 1) * 8); }
    // the values of a pass need a buffer unless they are written in place or go straight from the resident suffix array into the sets
    const bool value_buffer = sort_uniq || (build_sets && !resident);
    const uint64_t set_mems = std::max<uint64_t>(budget / (W ? W : 1), 1); // MEMs whose sets fit the budget (routed: the set array is intermediate too)
    uint64_t U = 0; // unique values of the passes so far
    for (uint64_t m0 = 0, o0 = 0; m0 < n;) {
        uint64_t m1 = n, o1 = V;
        const bool by_values = !(build_sets && resident) && V - o0 > budget;
        const uint64_t m_lim = routed && n - m0 > set_mems ? m0 + set_mems : n;
        if (by_values || m_lim < n) {
            hipLaunchKernelGGL(pgx_ml_cut_kernel, dim3(1), dim3(64), 0, s, voff, m_lim, m0, by_values ? budget : V, reinterpret_cast<uint64_t *>(ctr + 6));
            HIPCHECK(hipGetLastError());
            uint64_t c[2];
            read_scalars(c, ctr + 6, 16, s);
            m1 = c[0]; o1 = c[1];
        }
        const uint64_t np = m1 - m0, nv = o1 - o0;
        if (value_buffer) w.gbuf.ensure((nv ? nv : 1) * 8);
        uint64_t *dst = value_buffer ? w.gbuf.as<uint64_t>() : w.vals.as<uint64_t>() + o0; // value o of the batch goes to dst[o - o0]
        unsigned long long *sets = nullptr; // the pass's sets: MEM m at sets[(m - m0) * W ..)
        if (sets_form) sets = w.vals.as<unsigned long long>() + m0 * W;
        else if (routed) {
            w.sets.ensure(np * W * 8);
            sets = w.sets.as<unsigned long long>();
            HIPCHECK(hipMemsetAsync(sets, 0, np * W * 8, s));
        }
        if (nv && resident && build_sets) {
            hipLaunchKernelGGL(pgx_ml_sets_kernel, dim3(grid_for(nv, PGX_ML_SPAN)), dim3(256), 0, s, (const pgx_mem *)b->mems.as<pgx_mem>(), voff, m0, m1, o0, nv,
                               (const uint32_t *)d->img.lce_sa, bwt_n, (const uint64_t *)d->lce_seq_start.as<uint64_t>(), d->lce_n_seq, (uint32_t)W, sets);
            HIPCHECK(hipGetLastError());
        } else if (nv && resident) {
            hipLaunchKernelGGL(pgx_ml_gather_kernel, dim3(grid_for(nv, PGX_ML_SPAN)), dim3(256), 0, s, (const pgx_mem *)b->mems.as<pgx_mem>(), voff, m0, m1, o0, nv,
                               (const uint32_t *)d->img.lce_sa, bwt_n, (const uint64_t *)d->lce_seq_start.as<uint64_t>(), d->lce_n_seq, d->loc.max_length,
                               seq_ids ? 1 : 0, dst);
            HIPCHECK(hipGetLastError());
        } else if (nv) { // the sample chains of pgx_locate_batch, from the device ranges
            w.run0.ensure(np * 8); w.npieces.ensure(np * 8); w.poff.ensure((np + 1) * 8);
            const uint64_t *qs = w.qs.as<uint64_t>() + m0, *qe = w.qe.as<uint64_t>() + m0;
            hipLaunchKernelGGL(pgx_locate_plan_kernel, dim3(grid_for(np, 256)), dim3(256), 0, s, d->loc, qs, qe, np, w.run0.as<uint64_t>(), w.npieces.as<uint64_t>());
            HIPCHECK(hipGetLastError());
            scan_excl(1, w.npieces.p, np, 0, w.poff.as<uint64_t>(), w.scan_tmp, s);
            const uint64_t n_pieces = read_u64(w.poff.as<uint64_t>() + np, s);
            if (n_pieces) {
                hipLaunchKernelGGL(pgx_locate_walk_kernel, dim3(grid_for(n_pieces, 256)), dim3(256), 0, s, d->loc, qs, qe, np, (const uint64_t *)w.run0.as<uint64_t>(),
                                   (const uint64_t *)w.poff.as<uint64_t>(), n_pieces, voff + m0, o0, seq_ids ? 1 : 0, dst);
                HIPCHECK(hipGetLastError());
                if (build_sets) { // the pass's sequence ids -> bits
                    hipLaunchKernelGGL(pgx_ml_sets_ids_kernel, dim3(grid_for(nv, PGX_ML_SPAN)), dim3(256), 0, s, voff, m0, m1, o0, nv, (const uint64_t *)dst, (uint32_t)W,
                                       sets);
                    HIPCHECK(hipGetLastError());
                }
            }
        }
        if (routed) { // the sets as ascending ids behind the passes before: sorted and unique by construction
            uint32_t Wp = 1;
            while (Wp < W) Wp <<= 1;
            uint64_t *ucount = w.ucount.as<uint64_t>() + m0;
            w.uloc.ensure((np + 1) * 8);
            hipLaunchKernelGGL(pgx_ml_set_count_kernel, dim3(grid_for(np * Wp, 256)), dim3(256), 0, s, (const unsigned long long *)sets, np, (uint32_t)W, Wp, ucount);
            HIPCHECK(hipGetLastError());
            scan_excl(1, ucount, np, 0, w.uloc.as<uint64_t>(), w.scan_tmp, s, reinterpret_cast<uint64_t *>(ctr + 3));
            const uint64_t Up = read_u64(reinterpret_cast<const uint64_t *>(ctr + 3), s);
            w.vals.ensure_keep((U + Up ? U + Up : 1) * 8, U * 8); // (the stream is idle here: the read-back above synchronised it)
            if (Up) {
                hipLaunchKernelGGL(pgx_ml_set_expand_kernel, dim3(grid_for(np, 4)), dim3(256), 0, s, (const unsigned long long *)sets, np, (uint32_t)W,
                                   (const uint64_t *)w.uloc.as<uint64_t>(), w.vals.as<uint64_t>() + U);
                HIPCHECK(hipGetLastError());
            }
            U += Up;
        }
        if (sort_uniq) { // segmented sort-unique with the tag stage's kernels, size-class lists built on the device, then compaction behind the passes before
            w.seg.ensure((np + 1) * 8); w.lists.ensure(2 * np * 8); w.need.ensure(np * 8); w.soff.ensure((np + 1) * 8); w.uloc.ensure((np + 1) * 8);
            uint64_t *seg = w.seg.as<uint64_t>(), *wave_list = w.lists.as<uint64_t>(), *wg_list = wave_list + np, *ucount = w.ucount.as<uint64_t>() + m0;
            const uint64_t *cnt = w.cnt.as<uint64_t>() + m0;
            HIPCHECK(hipMemsetAsync(w.ctr.p, 0, 32, s));
            hipLaunchKernelGGL(pgx_ml_classify_kernel, dim3(grid_for(np + 1, 256)), dim3(256), 0, s, cnt, voff + m0, np, seg, wave_list, wg_list,
                               w.need.as<uint64_t>(), ucount, ctr);
            HIPCHECK(hipGetLastError());
            scan_excl(1, w.need.p, np, 0, w.soff.as<uint64_t>(), w.scan_tmp, s, reinterpret_cast<uint64_t *>(ctr + 2));
            uint64_t c[3];
            read_scalars(c, ctr, 24, s);
            const uint64_t n_wave = c[0], n_wg = c[1], S = c[2];
            if (n_wave)
                hipLaunchKernelGGL(pgx_tag_sort_unique_kernel<PgxTagDense>, dim3(grid_for(n_wave, 4)), dim3(256), 0, s, PgxTagDense{wave_list, cnt, seg}, n_wave,
                                   (const uint64_t *)nullptr, (const uint64_t *)nullptr, w.gbuf.as<uint64_t>(), ucount);
            if (n_wg) {
                w.scratch.ensure((S ? S : 1) * 8);
                HIPCHECK(hipFuncSetAttribute((const void *)pgx_tag_sort_large_kernel<PgxTagDense>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(PGX_SORT_WG_LDS_CAP * 8)));
                hipLaunchKernelGGL(pgx_tag_sort_large_kernel<PgxTagDense>, dim3(grid_for(n_wg, 1)), dim3(1024), (size_t)PGX_SORT_WG_LDS_CAP * 8, s, PgxTagDense{wg_list, cnt, seg},
                                   n_wg, (const uint64_t *)nullptr, (const uint64_t *)nullptr, w.gbuf.as<uint64_t>(), w.scratch.as<uint64_t>(),
                                   (const uint64_t *)w.soff.as<uint64_t>(), ucount);
            }
            HIPCHECK(hipGetLastError());
            scan_excl(1, ucount, np, 0, w.uloc.as<uint64_t>(), w.scan_tmp, s, reinterpret_cast<uint64_t *>(ctr + 3));
            const uint64_t Up = read_u64(reinterpret_cast<const uint64_t *>(ctr + 3), s);
            w.vals.ensure_keep((U + Up ? U + Up : 1) * 8, U * 8); // (the stream is idle here: the read-back above synchronised it)
            if (Up) {
                hipLaunchKernelGGL(pgx_tag_compact_kernel<PgxTagDense>, dim3(grid_for(np, 16)), dim3(256), 0, s, PgxTagDense{nullptr, nullptr, seg}, np,
                                   (const uint64_t *)nullptr, (const uint64_t *)nullptr, (const uint64_t *)ucount, (const uint64_t *)w.gbuf.as<uint64_t>(),
                                   (const uint64_t *)w.uloc.as<uint64_t>(), w.vals.as<uint64_t>() + U, ~0ull);
                HIPCHECK(hipGetLastError());
            }
            U += Up;
        }
        m0 = m1; o0 = o1;
    }
    if (uniq) scan_excl(1, w.ucount.p, n, 0, w.uoff.as<uint64_t>(), w.scan_tmp, s);
    w.vals.ensure(8);
    if (timed) HIPCHECK(hipEventRecord(w.ev[1], s));
    HIPCHECK(hipStreamSynchronize(s));
    w.ms = 0;
    if (timed) HIPCHECK(hipEventElapsedTime(&w.ms, w.ev[0], w.ev[1]));
    w.d_off = uniq || sets_form ? w.uoff.as<uint64_t>() : voff;
    w.n_mems = n;
    w.n_values = sets_form ? n * W : uniq ? U : V;
    w.n_not_located = n_not;
    w.flags = flags & (PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE | PGX_LOCATE_SEQ_SETS);
    w.set_words = build_sets ? (uint32_t)W : 0;
    w.resident = resident;
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void locations_header(const pgx_batch *b, pgx_locations *out) {
    const LocWork &w = b->lw;
    std::memset(out, 0, sizeof *out);
    out->n_mems = w.n_mems;
    out->n_values = w.n_values;
    out->n_not_located = w.n_not_located;
    out->flags = w.flags;
    out->resident = w.resident ? 1u : 0u;
    out->ms_locate = w.ms;
    out->set_words = w.set_words;
}

extern "C" pgx_status pgx_batch_device_locations(pgx_batch *b, pgx_locations *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->lw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_locations: batch has no locate result");
    locations_header(b, out);
    out->loc_offsets = b->lw.d_off;
    out->values = b->lw.vals.as<uint64_t>();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_locations(pgx_batch *b, pgx_locations *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->lw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_locations: batch has no locate result");
    use_device(b->device);
    LocWork &w = b->lw;
    w.h_off.ensure((w.n_mems + 1) * 8);
    w.h_vals.ensure((w.n_values ? w.n_values : 1) * 8);
    HIPCHECK(hipMemcpyAsync(w.h_off.p, w.d_off, (w.n_mems + 1) * 8, hipMemcpyDeviceToHost, b->own));
    if (w.n_values) HIPCHECK(hipMemcpyAsync(w.h_vals.p, w.vals.p, w.n_values * 8, hipMemcpyDeviceToHost, b->own));
    HIPCHECK(hipStreamSynchronize(b->own)); // (the locate itself completed inside pgx_batch_locate, on whatever stream it used)
    locations_header(b, out);
    out->loc_offsets = w.h_off.as<uint64_t>();
    out->values = w.h_vals.as<uint64_t>();
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// read hits (pgx_hits_kernels.hip; the definitions: include/pgx.h "read hits")
static const uint32_t HITS_FLAGS = PGX_HITS_BEST_SETS | PGX_HITS_SCORES;

// log2 of the lanes a read takes (Sp: the power of two >= n_seq, 64 with more than one word column); refuses what one launch cannot hold
static uint32_t hits_lane_shift(uint64_t n_reads, uint64_t n_seq, uint32_t W, const char *who) {
    uint32_t sp_shift = 0;
    while (W == 1 && (1ull << sp_shift) < n_seq) sp_shift++;
    if (W > 1) sp_shift = 6;
    // (a grid holds fewer than 2^32 threads: a larger launch would lose reads without an error)
    if (n_reads > (((1ull << 32) - PGX_HITS_THREADS) >> sp_shift))
        throw Error(PGX_ERR_UNSUPPORTED, std::string(who) + ": " + std::to_string(n_reads) + " reads at " + std::to_string(1u << sp_shift) +
                                             " lanes a read exceed the 2^32 threads of one launch: score the reads in smaller batches");
    return sp_shift;
}

// the one launch: sizes the outputs the flags ask for and enqueues the kernel on s (sets: n_mems x W words on the device)
static void hits_launch(HitsWork &w, const uint64_t *mem_off, const pgx_mem *mems, const uint64_t *sets, uint64_t n_reads, uint64_t n_mems, uint64_t n_seq, uint32_t W,
                        uint32_t flags, hipStream_t s) {
    const uint32_t sp_shift = hits_lane_shift(n_reads, n_seq, W, "read hits");
    w.hits.ensure((n_reads ? n_reads : 1) * sizeof(pgx_read_hit));
    if (flags & PGX_HITS_BEST_SETS) w.best_sets.ensure((n_reads ? n_reads * W : 1) * 8);
    if (flags & PGX_HITS_SCORES) w.scores.ensure((n_reads ? n_reads * n_seq : 1) * 4);
    if (!n_reads) return;
    unsigned long long *best = (flags & PGX_HITS_BEST_SETS) ? w.best_sets.as<unsigned long long>() : nullptr;
    uint32_t *scores = (flags & PGX_HITS_SCORES) ? w.scores.as<uint32_t>() : nullptr;
    const unsigned long long *dsets = reinterpret_cast<const unsigned long long *>(sets);
    if (W == 1) { // Sp lanes a read
        hipLaunchKernelGGL(pgx_read_hits_kernel, dim3(grid_for(n_reads, PGX_HITS_THREADS >> sp_shift)), dim3(PGX_HITS_THREADS), 0, s, mem_off, mems, dsets, n_reads, n_mems,
                           n_seq, sp_shift, flags, w.hits.as<pgx_read_hit>(), best, scores);
    } else // a wave a read
        hipLaunchKernelGGL(pgx_read_hits_wide_kernel, dim3(grid_for(n_reads, PGX_HITS_THREADS / 64)), dim3(PGX_HITS_THREADS), 0, s, mem_off, mems, dsets, n_reads, n_mems,
                           n_seq, W, flags, w.hits.as<pgx_read_hit>(), best, scores);
    HIPCHECK(hipGetLastError());
}

extern "C" pgx_status pgx_batch_read_hits(pgx_batch *b, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_read_hits");
    checked_device_count();
    if (!b) throw Error(PGX_ERR_ARG, "pgx_batch_read_hits: null batch");
    HitsWork &w = b->hw;
    w.valid = false;
    if (flags & ~HITS_FLAGS) throw Error(PGX_ERR_ARG, "pgx_batch_read_hits: unknown flag");
    if (!b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_read_hits: batch has not been run");
    const LocWork &lw = b->lw;
    if (!lw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_read_hits: needs a completed pgx_batch_locate(PGX_LOCATE_SEQ_SETS), the batch has no locate result");
    if (lw.flags != PGX_LOCATE_SEQ_SETS || lw.n_mems != b->n_mems || !lw.set_words)
        throw Error(PGX_ERR_ARG, "pgx_batch_read_hits: needs a completed pgx_batch_locate(PGX_LOCATE_SEQ_SETS), the last pgx_batch_locate ran with flags " +
                                     std::to_string(lw.flags));
    use_device(b->device);
    hipStream_t s = stream ? (hipStream_t)stream : b->own;
    const uint64_t n = b->n_reads, n_seq = b->h->meta.n_sequences();
    const uint32_t W = lw.set_words;
    (void)hits_lane_shift(n, n_seq, W, "pgx_batch_read_hits");
    if (flags & PGX_HITS_SCORES) {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); mem_free = 1ull << 30; }
        const uint64_t need = n * n_seq * 4;
        if (need > mem_free / 4)
            throw Error(PGX_ERR_NOMEM, "pgx_batch_read_hits: PGX_HITS_SCORES takes " + std::to_string(need) + " bytes, a quarter of the free device memory is " +
                                           std::to_string(mem_free / 4));
    }
    const bool timed = b->timed;
    if (timed) {
        for (auto &e : w.ev)
            if (!e) HIPCHECK(hipEventCreate(&e));
        HIPCHECK(hipEventRecord(w.ev[0], s));
    }
    hits_launch(w, b->mem_off.as<uint64_t>(), b->mems.as<pgx_mem>(), lw.vals.as<uint64_t>(), n, b->n_mems, n_seq, W, flags, s);
    if (timed) HIPCHECK(hipEventRecord(w.ev[1], s));
    HIPCHECK(hipStreamSynchronize(s));
    w.ms = 0;
    if (timed) HIPCHECK(hipEventElapsedTime(&w.ms, w.ev[0], w.ev[1]));
    w.flags = flags;
    w.set_words = W;
    w.n_reads = n;
    w.n_seq = n_seq;
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void hits_header(const pgx_batch *b, pgx_read_hits *out) {
    const HitsWork &w = b->hw;
    std::memset(out, 0, sizeof *out);
    out->n_reads = w.n_reads;
    out->n_seq = w.n_seq;
    out->set_words = w.set_words;
    out->flags = w.flags;
    out->ms_hits = w.ms;
}

extern "C" pgx_status pgx_batch_device_hits(pgx_batch *b, pgx_read_hits *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->hw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_hits: batch has no hits result");
    const HitsWork &w = b->hw;
    hits_header(b, out);
    out->hits = w.hits.as<pgx_read_hit>();
    out->best_sets = (w.flags & PGX_HITS_BEST_SETS) ? w.best_sets.as<uint64_t>() : nullptr;
    out->scores = (w.flags & PGX_HITS_SCORES) ? w.scores.as<uint32_t>() : nullptr;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_hits(pgx_batch *b, pgx_read_hits *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->hw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_hits: batch has no hits result");
    use_device(b->device);
    HitsWork &w = b->hw;
    const uint64_t n = w.n_reads;
    const bool best = (w.flags & PGX_HITS_BEST_SETS) != 0, scores = (w.flags & PGX_HITS_SCORES) != 0;
    w.h_hits.ensure((n ? n : 1) * sizeof(pgx_read_hit));
    if (n) HIPCHECK(hipMemcpyAsync(w.h_hits.p, w.hits.p, n * sizeof(pgx_read_hit), hipMemcpyDeviceToHost, b->own));
    if (best) {
        w.h_best_sets.ensure((n ? n * w.set_words : 1) * 8);
        if (n) HIPCHECK(hipMemcpyAsync(w.h_best_sets.p, w.best_sets.p, n * w.set_words * 8, hipMemcpyDeviceToHost, b->own));
    }
    if (scores) {
        w.h_scores.ensure((n ? n * w.n_seq : 1) * 4);
        if (n) HIPCHECK(hipMemcpyAsync(w.h_scores.p, w.scores.p, n * w.n_seq * 4, hipMemcpyDeviceToHost, b->own));
    }
    HIPCHECK(hipStreamSynchronize(b->own)); // (the kernel completed inside pgx_batch_read_hits, on whatever stream it used)
    hits_header(b, out);
    out->hits = w.h_hits.as<pgx_read_hit>();
    out->best_sets = best ? w.h_best_sets.as<uint64_t>() : nullptr;
    out->scores = scores ? w.h_scores.as<uint32_t>() : nullptr;
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_read_hits_arrays(int device, const uint64_t *mem_offsets, uint64_t n_reads, const pgx_mem *mems, const uint64_t *sets, uint32_t set_words,
                                           uint64_t n_seq, uint32_t flags, pgx_read_hit *hits, uint64_t *best_sets, uint32_t *scores) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_hits_arrays");
    checked_device_count();
    if (flags & ~HITS_FLAGS) throw Error(PGX_ERR_ARG, "pgx_read_hits_arrays: unknown flag");
    if (set_words < 1 || set_words > PGX_ML_SET_WORDS_MAX || n_seq == 0 || (n_seq + 63) / 64 != set_words)
        throw Error(PGX_ERR_ARG, "pgx_read_hits_arrays: set_words must be ceil(n_seq / 64) and 1 .. " + std::to_string(PGX_ML_SET_WORDS_MAX) + ", got set_words " +
                                     std::to_string(set_words) + " for n_seq " + std::to_string(n_seq));
    if (!mem_offsets || (n_reads && !hits) || ((flags & PGX_HITS_BEST_SETS) && n_reads && !best_sets) || ((flags & PGX_HITS_SCORES) && n_reads && !scores))
        throw Error(PGX_ERR_ARG, "pgx_read_hits_arrays: null argument");
    (void)hits_lane_shift(n_reads, n_seq, set_words, "pgx_read_hits_arrays"); // (before the arrays are read)
    bool ok = mem_offsets[0] == 0;
    for (uint64_t i = 0; ok && i < n_reads; i++) ok = mem_offsets[i] <= mem_offsets[i + 1];
    if (!ok) throw Error(PGX_ERR_ARG, "pgx_read_hits_arrays: mem_offsets must start at 0 and never decrease");
    const uint64_t m = mem_offsets[n_reads];
    if (m && (!mems || !sets)) throw Error(PGX_ERR_ARG, "pgx_read_hits_arrays: null argument");
    use_device(device);
    struct Work { // device copies of the input + the stage's buffers, released on every way out
        DevBuf mem_off, mems, sets;
        HitsWork w;
        ~Work() {
            DevBuf *all[] = {&mem_off, &mems, &sets};
            for (DevBuf *d : all) d->release();
            w.release();
        }
    } k;
    upload(k.mem_off, mem_offsets, (n_reads + 1) * 8);
    upload(k.mems, mems, m * sizeof(pgx_mem));
    upload(k.sets, sets, m * set_words * 8);
    hipStream_t s = nullptr;
    if (n_reads) { // the precondition, before anything is written
        k.w.bad.ensure(8);
        HIPCHECK(hipMemsetAsync(k.w.bad.p, 0xFF, 8, s));
        hipLaunchKernelGGL(pgx_read_hits_check_kernel, dim3(grid_for(n_reads, 256)), dim3(256), 0, s, (const uint64_t *)k.mem_off.as<uint64_t>(),
                           (const pgx_mem *)k.mems.as<pgx_mem>(), n_reads, m, k.w.bad.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
        const uint64_t bad = read_u64(k.w.bad.as<uint64_t>(), s);
        if (bad != ~0ull) throw Error(PGX_ERR_ARG, "pgx_read_hits_arrays: the MEM starts of read " + std::to_string(bad) + " do not ascend strictly");
    }
    hits_launch(k.w, k.mem_off.as<uint64_t>(), k.mems.as<pgx_mem>(), k.sets.as<uint64_t>(), n_reads, m, n_seq, set_words, flags, s);
    if (n_reads) {
        HIPCHECK(hipMemcpyAsync(hits, k.w.hits.p, n_reads * sizeof(pgx_read_hit), hipMemcpyDeviceToHost, s));
        if (flags & PGX_HITS_BEST_SETS) HIPCHECK(hipMemcpyAsync(best_sets, k.w.best_sets.p, n_reads * set_words * 8, hipMemcpyDeviceToHost, s));
        if (flags & PGX_HITS_SCORES) HIPCHECK(hipMemcpyAsync(scores, k.w.scores.p, n_reads * n_seq * 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// read placement (pgx_place_kernels.hip; the definitions: include/pgx.h "read placement")
static const uint32_t PLACE_FLAGS = PGX_PLACE_LIST;
// reads, MEMs or keys one launch takes at a thread an item or fewer: a grid holds fewer than 2^32 threads, and a larger one would lose items without an error
static const uint64_t PLACE_LAUNCH_ITEMS = 1ull << 31;

// keys one pass may hold: PGX_PLACE_BUDGET_MB (read per call, fractions allowed), default a quarter of the free device memory
static uint64_t place_budget_keys(size_t mem_free) {
    uint64_t bytes = 0;
    if (const char *e = std::getenv("PGX_PLACE_BUDGET_MB")) {
        const double mb = std::strtod(e, nullptr);
        if (mb > 0) bytes = (uint64_t)(mb * 1048576.0);
    }
    if (!bytes) bytes = mem_free / 4;
    return std::min<uint64_t>(std::max<uint64_t>(bytes / 8, 1), PLACE_LAUNCH_ITEMS);
}

static uint32_t place_bits(unsigned __int128 v) {
    uint32_t b = 0;
    while (v) { b++; v >>= 1; }
    return b;
}

// log2 of the lanes a read of the sweep takes: the power of two >= twice the mean anchors a read of the pass, 4 .. 64 (a longer read takes more
// steps).  PGX_PLACE_LANES (tests; 1 .. 64, rounded up to a power of two) fixes it.  Results never depend on it.
static uint32_t place_lane_shift(uint64_t keys, uint64_t reads) {
    uint64_t want = reads ? 2 * ((keys + reads - 1) / reads) : 4;
    want = std::min<uint64_t>(std::max<uint64_t>(want, 4), 64);
    if (const char *e = std::getenv("PGX_PLACE_LANES")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= 64) want = (uint64_t)v;
    }
    uint32_t sh = 0;
    while ((1ull << sh) < want) sh++;
    return sh;
}

static size_t free_device_memory() {
    size_t mem_free = 0, mem_total = 0;
    if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); mem_free = 1ull << 30; }
    return mem_free;
}

// The stage on device arrays, enqueued on s (synchronised where a size is read back): w.recs, and with PGX_PLACE_LIST w.place_off / w.places.
// loc_off: n_mems + 1 value offsets, values: n_values.  Refuses before a result buffer is written.
static void place_core(PlaceWork &w, const uint64_t *mem_off, const pgx_mem *mems, const uint64_t *loc_off, const uint64_t *values, uint64_t n, uint64_t n_mems,
                       uint64_t n_values, uint64_t n_seq, uint64_t L, uint32_t flags, size_t mem_free, hipStream_t s, const std::string &who) {
    if (n >= PLACE_LAUNCH_ITEMS || n_mems >= PLACE_LAUNCH_ITEMS)
        throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n) + " reads with " + std::to_string(n_mems) + " MEMs exceed the " + std::to_string(PLACE_LAUNCH_ITEMS) +
                                             " one launch holds: place the reads in smaller batches");
    const bool list = (flags & PGX_PLACE_LIST) != 0;
    // 1. plan: the anchors of every read, the first MEM of every MEM's read, the maxima of the key layout
    //    ctr: [0] most MEMs of a read [1] largest MEM start [2] aoff[n] [3] aoff[0]; later [0] wave list [1] workgroup list [2] scratch total [3] placements of a pass [6..7] cut
    w.aoff.ensure((n + 1) * 8); w.acnt.ensure((n ? n : 1) * 8); w.mfirst.ensure((n_mems ? n_mems : 1) * 8); w.ctr.ensure(64);
    unsigned long long *ctr = w.ctr.as<unsigned long long>();
    HIPCHECK(hipMemsetAsync(w.ctr.p, 0, 64, s));
    hipLaunchKernelGGL(pgx_place_plan_kernel, dim3(grid_for(n + 1, 256)), dim3(256), 0, s, mem_off, loc_off, mems, n, n_mems, n_values, w.aoff.as<uint64_t>(),
                       w.acnt.as<uint64_t>(), ctr);
    if (n_mems) hipLaunchKernelGGL(pgx_place_first_kernel, dim3(grid_for(n_mems, 256)), dim3(256), 0, s, mem_off, n, n_mems, w.mfirst.as<uint64_t>());
    HIPCHECK(hipGetLastError());
    uint64_t c[4];
    read_scalars(c, ctr, 32, s);
    const uint64_t most_mems = c[0], bias = c[1], a_end = c[2], a_begin = std::min(c[3], c[2]);
    const uint32_t ordinal_bits = place_bits(most_mems ? most_mems - 1 : 0);
    const uint64_t span = L + bias;
    const uint32_t group_bits = span < L ? 65u : place_bits((unsigned __int128)n_seq * span);
    if (group_bits + ordinal_bits > 64)
        throw Error(PGX_ERR_UNSUPPORTED, who + ": a key needs " + std::to_string(group_bits) + " bits for sequence and diagonal (" + std::to_string(n_seq) + " sequences x (max_length " +
                                             std::to_string(L) + " + largest MEM start " + std::to_string(bias) + ")) and " + std::to_string(ordinal_bits) +
                                             " bits for the MEM of a read (most MEMs of a read: " + std::to_string(most_mems) + "), 64 are available");
    const uint64_t budget = place_budget_keys(mem_free);
    const uint64_t *aoff = w.aoff.as<uint64_t>(), *acnt = w.acnt.as<uint64_t>();
    w.recs.ensure((n ? n : 1) * sizeof(pgx_read_place)); w.pcount.ensure((n ? n : 1) * 8);
    // 2. passes over consecutive whole reads whose keys fit the budget (one pass unless the batch exceeds it)
    uint64_t U = 0; // placements listed by the passes so far
    uint32_t passes = 0;
    for (uint64_t r0 = 0, o0 = a_begin; r0 < n;) {
        uint64_t r1 = n, o1 = a_end;
        if (a_end - o0 > budget) {
            hipLaunchKernelGGL(pgx_ml_cut_kernel, dim3(1), dim3(64), 0, s, aoff, n, r0, budget, reinterpret_cast<uint64_t *>(ctr + 6));
            HIPCHECK(hipGetLastError());
            uint64_t cut[2];
            read_scalars(cut, ctr + 6, 16, s);
            r1 = cut[0]; o1 = cut[1];
            if (o1 - o0 > budget) // (the cut is a read at least)
                throw Error(PGX_ERR_NOMEM, who + ": read " + std::to_string(r0) + " has " + std::to_string(o1 - o0) + " anchors, the keys of a pass hold " + std::to_string(budget) +
                                               " (PGX_PLACE_BUDGET_MB)");
        }
        const uint64_t np = r1 - r0, nk = o1 - o0;
        passes++;
        // keys, then the segmented sort of the tag stage: a read is a segment, the size-class lists are built on the device
        w.keys.ensure((nk ? nk : 1) * 8);
        w.seg.ensure((np + 1) * 8); w.lists.ensure(2 * np * 8); w.need.ensure(np * 8); w.soff.ensure((np + 1) * 8); w.ucount.ensure(np * 8);
        uint64_t *keys = w.keys.as<uint64_t>(), *seg = w.seg.as<uint64_t>(), *wave_list = w.lists.as<uint64_t>(), *wg_list = wave_list + np, *ucount = w.ucount.as<uint64_t>();
        if (nk) {
            hipLaunchKernelGGL(pgx_place_keys_kernel, dim3(grid_for(nk, PGX_ML_SPAN)), dim3(256), 0, s, mems, loc_off, (const uint64_t *)w.mfirst.as<uint64_t>(), values,
                               (uint64_t)0, n_mems, o0, nk, L, span, bias, ordinal_bits, keys);
            HIPCHECK(hipGetLastError());
        }
        HIPCHECK(hipMemsetAsync(w.ctr.p, 0, 32, s));
        hipLaunchKernelGGL(pgx_ml_classify_kernel, dim3(grid_for(np + 1, 256)), dim3(256), 0, s, acnt + r0, aoff + r0, np, seg, wave_list, wg_list, w.need.as<uint64_t>(),
                           ucount, ctr);
        HIPCHECK(hipGetLastError());
        scan_excl(1, w.need.p, np, 0, w.soff.as<uint64_t>(), w.scan_tmp, s, reinterpret_cast<uint64_t *>(ctr + 2));
        uint64_t lc[3];
        read_scalars(lc, ctr, 24, s);
        const uint64_t n_wave = lc[0], n_wg = lc[1], S = lc[2];
        if (n_wave)
            hipLaunchKernelGGL(pgx_tag_sort_unique_kernel<PgxTagDense>, dim3(grid_for(n_wave, 4)), dim3(256), 0, s, PgxTagDense{wave_list, acnt + r0, seg}, n_wave,
                               (const uint64_t *)nullptr, (const uint64_t *)nullptr, keys, ucount);
        if (n_wg) {
            w.scratch.ensure((S ? S : 1) * 8);
            HIPCHECK(hipFuncSetAttribute((const void *)pgx_tag_sort_large_kernel<PgxTagDense>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(PGX_SORT_WG_LDS_CAP * 8)));
            hipLaunchKernelGGL(pgx_tag_sort_large_kernel<PgxTagDense>, dim3(grid_for(n_wg, 1)), dim3(1024), (size_t)PGX_SORT_WG_LDS_CAP * 8, s,
                               PgxTagDense{wg_list, acnt + r0, seg}, n_wg, (const uint64_t *)nullptr, (const uint64_t *)nullptr, keys, w.scratch.as<uint64_t>(),
                               (const uint64_t *)w.soff.as<uint64_t>(), ucount);
        }
        HIPCHECK(hipGetLastError());
        // the sweep, in launches of fewer than 2^32 threads
        const uint32_t g_shift = place_lane_shift(nk, np);
        const uint64_t per_launch = PLACE_LAUNCH_ITEMS >> g_shift;
        auto sweep = [&](bool fill, const uint64_t *list_off, pgx_placement *places) {
            for (uint64_t q0 = 0; q0 < np; q0 += per_launch) {
                const uint64_t nr = std::min(per_launch, np - q0);
                const dim3 grid(grid_for(nr, PGX_PLACE_THREADS >> g_shift)), block(PGX_PLACE_THREADS);
                if (fill)
                    hipLaunchKernelGGL(pgx_place_sweep_kernel<true>, grid, block, 0, s, mem_off, mems, loc_off, acnt, (const uint64_t *)keys, (const uint64_t *)seg,
                                       (const uint64_t *)ucount, r0, r0 + q0, nr, n_mems, span, bias, ordinal_bits, g_shift, w.recs.as<pgx_read_place>(),
                                       w.pcount.as<uint64_t>(), list_off, places);
                else
                    hipLaunchKernelGGL(pgx_place_sweep_kernel<false>, grid, block, 0, s, mem_off, mems, loc_off, acnt, (const uint64_t *)keys, (const uint64_t *)seg,
                                       (const uint64_t *)ucount, r0, r0 + q0, nr, n_mems, span, bias, ordinal_bits, g_shift, w.recs.as<pgx_read_place>(),
                                       w.pcount.as<uint64_t>(), list_off, places);
                HIPCHECK(hipGetLastError());
            }
        };
        sweep(false, nullptr, nullptr);
        if (list) { // the pass's counts -> offsets behind the passes before, then the same walk writes the placements
            w.loff.ensure((np + 1) * 8);
            scan_excl(1, w.pcount.as<uint64_t>() + r0, np, 0, w.loff.as<uint64_t>(), w.scan_tmp, s, reinterpret_cast<uint64_t *>(ctr + 3));
            const uint64_t Up = read_u64(reinterpret_cast<const uint64_t *>(ctr + 3), s);
            if ((U + Up) > (mem_free / 4) / sizeof(pgx_placement))
                throw Error(PGX_ERR_NOMEM, who + ": PGX_PLACE_LIST takes at least " + std::to_string((U + Up) * sizeof(pgx_placement)) +
                                               " bytes, a quarter of the free device memory is " + std::to_string(mem_free / 4));
            w.places.ensure_keep((U + Up ? U + Up : 1) * sizeof(pgx_placement), U * sizeof(pgx_placement)); // (the stream is idle here: the read-back above synchronised it)
            if (Up) sweep(true, w.loff.as<uint64_t>(), w.places.as<pgx_placement>() + U);
            U += Up;
        }
        r0 = r1; o0 = o1;
    }
    if (list) {
        w.place_off.ensure((n + 1) * 8);
        w.places.ensure(sizeof(pgx_placement));
        scan_excl(1, w.pcount.p, n, 0, w.place_off.as<uint64_t>(), w.scan_tmp, s);
    }
    w.flags = flags;
    w.n_reads = n;
    w.n_anchors = a_end - a_begin;
    w.n_places = U;
    w.n_passes = passes;
}

extern "C" pgx_status pgx_batch_read_place(pgx_batch *b, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_read_place");
    checked_device_count();
    if (!b) throw Error(PGX_ERR_ARG, "pgx_batch_read_place: null batch");
    // (what is refused here leaves an earlier place result as it was)
    if (flags & ~PLACE_FLAGS) throw Error(PGX_ERR_ARG, "pgx_batch_read_place: unknown flag");
    if (!b->ran) throw Error(PGX_ERR_ARG, "pgx_batch_read_place: batch has not been run");
    const LocWork &lw = b->lw;
    if (!lw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_read_place: needs a completed pgx_batch_locate(flags = 0), the batch has no locate result");
    if (lw.flags != 0 || lw.n_mems != b->n_mems)
        throw Error(PGX_ERR_ARG, "pgx_batch_read_place: needs a completed pgx_batch_locate(flags = 0), the last pgx_batch_locate ran with flags " + std::to_string(lw.flags));
    use_device(b->device);
    pgx_device_image *d = locate_image(b->h, b->device);
    hipStream_t s = stream ? (hipStream_t)stream : b->own;
    PlaceWork &w = b->pw;
    w.valid = false;
    const size_t mem_free = free_device_memory();
    const bool timed = b->timed;
    if (timed) {
        for (auto &e : w.ev)
            if (!e) HIPCHECK(hipEventCreate(&e));
        HIPCHECK(hipEventRecord(w.ev[0], s));
    }
    place_core(w, b->mem_off.as<uint64_t>(), b->mems.as<pgx_mem>(), lw.d_off, lw.vals.as<uint64_t>(), b->n_reads, b->n_mems, lw.n_values, b->h->meta.n_sequences(),
               d->loc.max_length, flags, mem_free, s, "pgx_batch_read_place");
    if (timed) HIPCHECK(hipEventRecord(w.ev[1], s));
    HIPCHECK(hipStreamSynchronize(s));
    w.ms = 0;
    if (timed) HIPCHECK(hipEventElapsedTime(&w.ms, w.ev[0], w.ev[1]));
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void places_header(const pgx_batch *b, pgx_read_places *out) {
    const PlaceWork &w = b->pw;
    std::memset(out, 0, sizeof *out);
    out->n_reads = w.n_reads;
    out->n_anchors = w.n_anchors;
    out->n_places = w.n_places;
    out->flags = w.flags;
    out->n_passes = w.n_passes;
    out->ms_place = w.ms;
}

extern "C" pgx_status pgx_batch_device_places(pgx_batch *b, pgx_read_places *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->pw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_places: batch has no place result");
    const PlaceWork &w = b->pw;
    places_header(b, out);
    out->reads = w.recs.as<pgx_read_place>();
    if (w.flags & PGX_PLACE_LIST) {
        out->place_offsets = w.place_off.as<uint64_t>();
        out->places = w.places.as<pgx_placement>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_places(pgx_batch *b, pgx_read_places *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->pw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_places: batch has no place result");
    use_device(b->device);
    PlaceWork &w = b->pw;
    const uint64_t n = w.n_reads;
    const bool list = (w.flags & PGX_PLACE_LIST) != 0;
    w.h_recs.ensure((n ? n : 1) * sizeof(pgx_read_place));
    if (n) HIPCHECK(hipMemcpyAsync(w.h_recs.p, w.recs.p, n * sizeof(pgx_read_place), hipMemcpyDeviceToHost, b->own));
    if (list) {
        w.h_place_off.ensure((n + 1) * 8);
        w.h_places.ensure((w.n_places ? w.n_places : 1) * sizeof(pgx_placement));
        HIPCHECK(hipMemcpyAsync(w.h_place_off.p, w.place_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, b->own));
        if (w.n_places) HIPCHECK(hipMemcpyAsync(w.h_places.p, w.places.p, w.n_places * sizeof(pgx_placement), hipMemcpyDeviceToHost, b->own));
    }
    HIPCHECK(hipStreamSynchronize(b->own)); // (the stage completed inside pgx_batch_read_place, on whatever stream it used)
    places_header(b, out);
    out->reads = w.h_recs.as<pgx_read_place>();
    if (list) {
        out->place_offsets = w.h_place_off.as<uint64_t>();
        out->places = w.h_places.as<pgx_placement>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_read_place_arrays(int device, const uint64_t *mem_offsets, uint64_t n_reads, const pgx_mem *mems, const uint64_t *loc_offsets,
                                            const uint64_t *values, uint64_t n_seq, uint64_t max_length, uint32_t flags, pgx_read_place *out,
                                            uint64_t *place_offsets, pgx_placement *places, uint64_t places_cap) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_place_arrays");
    checked_device_count();
    if (flags & ~PLACE_FLAGS) throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: unknown flag");
    if (n_seq == 0 || max_length == 0) throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: n_seq and max_length must be positive");
    const bool list = (flags & PGX_PLACE_LIST) != 0;
    if (!mem_offsets || !loc_offsets || (n_reads && !out) || (list && (!place_offsets || (places_cap && !places))))
        throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: null argument");
    if (mem_offsets[0] != 0) throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: mem_offsets must start at 0");
    for (uint64_t i = 0; i < n_reads; i++)
        if (mem_offsets[i] > mem_offsets[i + 1])
            throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: mem_offsets decrease at read " + std::to_string(i));
    const uint64_t m = mem_offsets[n_reads];
    if (loc_offsets[0] != 0) throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: loc_offsets must start at 0");
    for (uint64_t r = 0; r < n_reads; r++)
        for (uint64_t i = mem_offsets[r]; i < mem_offsets[r + 1]; i++)
            if (loc_offsets[i] > loc_offsets[i + 1])
                throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: loc_offsets decrease at MEM " + std::to_string(i) + " of read " + std::to_string(r));
    const uint64_t nv = loc_offsets[m];
    if ((m && !mems) || (nv && !values)) throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: null argument");
    use_device(device);
    struct Work { // device copies of the input + the stage's buffers, released on every way out
        DevBuf mem_off, mems, loc_off, values;
        PlaceWork w;
        ~Work() {
            DevBuf *all[] = {&mem_off, &mems, &loc_off, &values};
            for (DevBuf *d : all) d->release();
            w.release();
        }
    } k;
    const size_t mem_free = free_device_memory();
    upload(k.mem_off, mem_offsets, (n_reads + 1) * 8);
    upload(k.mems, mems, m * sizeof(pgx_mem));
    upload(k.loc_off, loc_offsets, (m + 1) * 8);
    upload(k.values, values, nv * 8);
    hipStream_t s = nullptr;
    if (n_reads) { // the preconditions, before anything is written
        if (n_reads >= PLACE_LAUNCH_ITEMS || nv >= (1ull << 32) - 256)
            throw Error(PGX_ERR_UNSUPPORTED, "pgx_read_place_arrays: " + std::to_string(n_reads) + " reads with " + std::to_string(nv) + " values exceed one checking launch");
        k.w.bad.ensure(8);
        HIPCHECK(hipMemsetAsync(k.w.bad.p, 0xFF, 8, s));
        hipLaunchKernelGGL(pgx_read_hits_check_kernel, dim3(grid_for(n_reads, 256)), dim3(256), 0, s, (const uint64_t *)k.mem_off.as<uint64_t>(),
                           (const pgx_mem *)k.mems.as<pgx_mem>(), n_reads, m, k.w.bad.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
        uint64_t bad = read_u64(k.w.bad.as<uint64_t>(), s);
        if (bad != ~0ull) throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: the MEM starts of read " + std::to_string(bad) + " do not ascend strictly");
        if (nv) { // (a read's anchors: loc_offsets at its first MEM, what the plan kernel computes too)
            std::vector<uint64_t> h_aoff(n_reads + 1);
            for (uint64_t r = 0; r <= n_reads; r++) h_aoff[r] = loc_offsets[mem_offsets[r]];
            upload(k.w.aoff, h_aoff.data(), (n_reads + 1) * 8);
            hipLaunchKernelGGL(pgx_place_check_values_kernel, dim3(grid_for(nv, 256)), dim3(256), 0, s, (const uint64_t *)k.values.as<uint64_t>(), nv, max_length, n_seq,
                               (const uint64_t *)k.w.aoff.as<uint64_t>(), n_reads, k.w.bad.as<unsigned long long>());
            HIPCHECK(hipGetLastError());
            bad = read_u64(k.w.bad.as<uint64_t>(), s);
            if (bad != ~0ull)
                throw Error(PGX_ERR_ARG, "pgx_read_place_arrays: read " + std::to_string(bad) + " has a value whose sequence is not below n_seq " + std::to_string(n_seq));
        }
    }
    place_core(k.w, k.mem_off.as<uint64_t>(), k.mems.as<pgx_mem>(), k.loc_off.as<uint64_t>(), k.values.as<uint64_t>(), n_reads, m, nv, n_seq, max_length, flags, mem_free, s,
               "pgx_read_place_arrays");
    if (list && k.w.n_places > places_cap)
        throw Error(PGX_ERR_NOMEM, "pgx_read_place_arrays: the list holds " + std::to_string(k.w.n_places) + " placements, places_cap is " + std::to_string(places_cap));
    if (n_reads) HIPCHECK(hipMemcpyAsync(out, k.w.recs.p, n_reads * sizeof(pgx_read_place), hipMemcpyDeviceToHost, s));
    if (list) {
        HIPCHECK(hipMemcpyAsync(place_offsets, k.w.place_off.p, (n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
        if (k.w.n_places) HIPCHECK(hipMemcpyAsync(places, k.w.places.p, k.w.n_places * sizeof(pgx_placement), hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// read verify (pgx_verify_kernels.hip; the definitions: include/pgx.h "read verify")
static const uint32_t VERIFY_FLAGS = PGX_VERIFY_LIST;

static void verify_check_args(const std::string &who, uint32_t penalty, uint32_t flags) {
    if (flags & ~VERIFY_FLAGS) throw Error(PGX_ERR_ARG, who + ": unknown flag");
    if (penalty == 0 || penalty > PGX_VERIFY_MAX_PENALTY)
        throw Error(PGX_ERR_ARG, who + ": mismatch_penalty " + std::to_string(penalty) + " is outside 1 .. " + std::to_string(PGX_VERIFY_MAX_PENALTY));
}

// The stage on device arrays, enqueued on s: the candidates w.cand_off / cand_seq / cand_diag / cand_read (n_cands of them) -> w.cands, w.recs.
// reads: read_bytes bytes, read_off: n + 1 offsets into them.  Every buffer was sized by the caller's checks; nothing is read back.
static void verify_core(VerifyWork &w, const uint32_t *text4, const uint64_t *seq_start, uint32_t endmark, const uint8_t *reads, uint64_t read_bytes, const uint64_t *read_off,
                        uint64_t n, uint64_t n_cands, uint32_t penalty, hipStream_t s) {
    const uint64_t n_rw = (read_bytes + 7) / 8 + 1;
    w.rcode.ensure(n_rw * 4);
    w.cands.ensure((n_cands ? n_cands : 1) * sizeof(pgx_read_verify));
    w.recs.ensure((n ? n : 1) * sizeof(pgx_read_verify));
    // the reads at the text's symbol width, once per read whatever the number of its candidates
    hipLaunchKernelGGL(pgx_verify_code_kernel, dim3((unsigned)std::min<uint64_t>((n_rw + 255) / 256, 1u << 20)), dim3(256), 0, s, reads, read_bytes, n_rw, w.rcode.as<uint32_t>());
    if (n_cands)
        hipLaunchKernelGGL(pgx_verify_kernel, dim3(grid_for(n_cands, PGX_VERIFY_THREADS)), dim3(PGX_VERIFY_THREADS), 0, s, text4, seq_start, endmark,
                           (const uint32_t *)w.rcode.as<uint32_t>(), read_off, (const uint64_t *)w.cand_off.as<uint64_t>(), (const uint64_t *)w.cand_read.as<uint64_t>(),
                           (const uint32_t *)w.cand_seq.as<uint32_t>(), (const int64_t *)w.cand_diag.as<int64_t>(), n_cands, penalty, w.cands.as<pgx_read_verify>());
    if (n)
        hipLaunchKernelGGL(pgx_verify_reduce_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const pgx_read_verify *)w.cands.as<pgx_read_verify>(),
                           (const uint64_t *)w.cand_off.as<uint64_t>(), n, w.recs.as<pgx_read_verify>());
    HIPCHECK(hipGetLastError());
}

extern "C" pgx_status pgx_batch_read_verify(pgx_batch *b, uint32_t max_cand, uint32_t mismatch_penalty, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_read_verify");
    checked_device_count();
    const std::string who = "pgx_batch_read_verify";
    if (!b) throw Error(PGX_ERR_ARG, who + ": null batch");
    // (what is refused here leaves an earlier verify result as it was)
    verify_check_args(who, mismatch_penalty, flags);
    if (max_cand < 1 || max_cand > PGX_VERIFY_MAX_CAND) throw Error(PGX_ERR_ARG, who + ": max_cand " + std::to_string(max_cand) + " is outside 1 .. " + std::to_string(PGX_VERIFY_MAX_CAND));
    if (!b->ran) throw Error(PGX_ERR_ARG, who + ": batch has not been run");
    PlaceWork &pw = b->pw;
    if (!pw.valid || pw.n_reads != b->n_reads) throw Error(PGX_ERR_ARG, who + ": needs a completed pgx_batch_read_place, the batch has no place result");
    if (max_cand > 1 && !(pw.flags & PGX_PLACE_LIST))
        throw Error(PGX_ERR_ARG, who + ": max_cand " + std::to_string(max_cand) + " needs a place result made with PGX_PLACE_LIST, the last pgx_batch_read_place ran without it");
    if (b->max_read_len >= (1ull << 31)) throw Error(PGX_ERR_UNSUPPORTED, who + ": a read of " + std::to_string(b->max_read_len) + " bytes; the records hold read positions below 2^31");
    const uint64_t n = b->n_reads;
    if (n >= PLACE_LAUNCH_ITEMS) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n) + " reads exceed one launch");
    use_device(b->device);
    pgx_device_image *d = device_image(b->h, b->device);
    ensure_text(b->h, d); // (throws where the index has no text image, before anything of the batch changes)
    hipStream_t s = stream ? (hipStream_t)stream : b->own;
    VerifyWork &w = b->vw;
    w.valid = false;
    const bool timed = b->timed;
    if (timed) {
        for (auto &e : w.ev)
            if (!e) HIPCHECK(hipEventCreate(&e));
        HIPCHECK(hipEventRecord(w.ev[0], s));
    }
    // the candidates: counted, scanned, filled
    const bool from_list = max_cand > 1;
    const pgx_read_place *recs = pw.recs.as<pgx_read_place>();
    const uint64_t *place_off = from_list ? pw.place_off.as<uint64_t>() : nullptr;
    const pgx_placement *places = from_list ? pw.places.as<pgx_placement>() : nullptr;
    w.count.ensure((n ? n : 1) * 8);
    w.cand_off.ensure((n + 1) * 8);
    uint64_t n_cands = 0;
    if (n) {
        hipLaunchKernelGGL(pgx_verify_choose_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, recs, place_off, places, n, max_cand, w.count.as<uint64_t>(),
                           (const uint64_t *)nullptr, (uint32_t *)nullptr, (int64_t *)nullptr);
        HIPCHECK(hipGetLastError());
        scan_excl(1, w.count.p, n, 0, w.cand_off.as<uint64_t>(), w.scan_tmp, s);
        n_cands = read_u64(w.cand_off.as<uint64_t>() + n, s);
    } else HIPCHECK(hipMemsetAsync(w.cand_off.p, 0, 8, s));
    if (n_cands >= PLACE_LAUNCH_ITEMS) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_cands) + " candidates exceed one launch; lower max_cand");
    {
        const uint64_t need = n_cands * (sizeof(pgx_read_verify) + 20) + n * sizeof(pgx_read_verify) + b->read_bytes / 2;
        const size_t mem_free = free_device_memory();
        if (need > w.cands.cap + w.recs.cap + w.rcode.cap && need - (w.cands.cap + w.recs.cap + w.rcode.cap) > mem_free)
            throw Error(PGX_ERR_NOMEM, who + ": " + std::to_string(n_cands) + " candidates take " + std::to_string(need) + " bytes of device memory, " + std::to_string(mem_free) + " are free");
    }
    w.cand_seq.ensure((n_cands ? n_cands : 1) * 4);
    w.cand_diag.ensure((n_cands ? n_cands : 1) * 8);
    w.cand_read.ensure((n_cands ? n_cands : 1) * 8);
    if (n_cands) {
        hipLaunchKernelGGL(pgx_verify_choose_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, recs, place_off, places, n, max_cand, w.count.as<uint64_t>(),
                           (const uint64_t *)w.cand_off.as<uint64_t>(), w.cand_seq.as<uint32_t>(), w.cand_diag.as<int64_t>());
        hipLaunchKernelGGL(pgx_verify_owner_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const uint64_t *)w.cand_off.as<uint64_t>(), n, n_cands, w.cand_read.as<uint64_t>());
        HIPCHECK(hipGetLastError());
    }
    verify_core(w, d->text4.as<uint32_t>(), d->text_seq_start.as<uint64_t>(), 1u, b->reads.as<uint8_t>(), b->read_bytes, b->offsets.as<uint64_t>(), n, n_cands, mismatch_penalty, s);
    if (timed) HIPCHECK(hipEventRecord(w.ev[1], s));
    HIPCHECK(hipStreamSynchronize(s));
    w.ms = 0;
    if (timed) HIPCHECK(hipEventElapsedTime(&w.ms, w.ev[0], w.ev[1]));
    w.n_reads = n; w.n_cands = n_cands; w.flags = flags; w.max_cand = max_cand; w.penalty = mismatch_penalty;
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void verified_header(const pgx_batch *b, pgx_read_verifies *out) {
    const VerifyWork &w = b->vw;
    std::memset(out, 0, sizeof *out);
    out->n_reads = w.n_reads;
    out->n_cands = w.n_cands;
    out->flags = w.flags;
    out->max_cand = w.max_cand;
    out->mismatch_penalty = w.penalty;
    out->ms_verify = w.ms;
}

extern "C" pgx_status pgx_batch_device_verified(pgx_batch *b, pgx_read_verifies *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->vw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_verified: batch has no verify result");
    const VerifyWork &w = b->vw;
    verified_header(b, out);
    out->reads = w.recs.as<pgx_read_verify>();
    if (w.flags & PGX_VERIFY_LIST) {
        out->cand_offsets = w.cand_off.as<uint64_t>();
        out->cands = w.cands.as<pgx_read_verify>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_verified(pgx_batch *b, pgx_read_verifies *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->vw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_verified: batch has no verify result");
    use_device(b->device);
    VerifyWork &w = b->vw;
    const uint64_t n = w.n_reads;
    const bool list = (w.flags & PGX_VERIFY_LIST) != 0;
    w.h_recs.ensure((n ? n : 1) * sizeof(pgx_read_verify));
    if (n) HIPCHECK(hipMemcpyAsync(w.h_recs.p, w.recs.p, n * sizeof(pgx_read_verify), hipMemcpyDeviceToHost, b->own));
    if (list) {
        w.h_cand_off.ensure((n + 1) * 8);
        w.h_cands.ensure((w.n_cands ? w.n_cands : 1) * sizeof(pgx_read_verify));
        HIPCHECK(hipMemcpyAsync(w.h_cand_off.p, w.cand_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, b->own));
        if (w.n_cands) HIPCHECK(hipMemcpyAsync(w.h_cands.p, w.cands.p, w.n_cands * sizeof(pgx_read_verify), hipMemcpyDeviceToHost, b->own));
    }
    HIPCHECK(hipStreamSynchronize(b->own)); // (the stage completed inside pgx_batch_read_verify, on whatever stream it used)
    verified_header(b, out);
    out->reads = w.h_recs.as<pgx_read_verify>();
    if (list) {
        out->cand_offsets = w.h_cand_off.as<uint64_t>();
        out->cands = w.h_cands.as<pgx_read_verify>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_read_verify_arrays(int device, const uint8_t *text, const uint64_t *seq_offsets, uint64_t n_seq, const uint8_t *reads,
                                             const uint64_t *read_offsets, uint64_t n_reads, const uint64_t *cand_offsets, const uint32_t *cand_seq,
                                             const int64_t *cand_diag, uint32_t mismatch_penalty, uint32_t flags, pgx_read_verify *out,
                                             uint64_t *list_offsets, pgx_read_verify *list, uint64_t list_cap) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_verify_arrays");
    checked_device_count();
    const std::string who = "pgx_read_verify_arrays";
    verify_check_args(who, mismatch_penalty, flags);
    const bool want_list = (flags & PGX_VERIFY_LIST) != 0;
    if (!seq_offsets || !read_offsets || !cand_offsets || (n_reads && !out) || (want_list && (!list_offsets || (list_cap && !list))))
        throw Error(PGX_ERR_ARG, who + ": null argument");
    auto check_offsets = [&](const uint64_t *o, uint64_t k, const char *name, const char *item) {
        if (o[0] != 0) throw Error(PGX_ERR_ARG, who + ": " + name + " must start at 0");
        for (uint64_t i = 0; i < k; i++)
            if (o[i] > o[i + 1]) throw Error(PGX_ERR_ARG, who + ": " + name + " decrease at " + item + " " + std::to_string(i));
    };
    check_offsets(seq_offsets, n_seq, "seq_offsets", "sequence");
    check_offsets(read_offsets, n_reads, "read_offsets", "read");
    check_offsets(cand_offsets, n_reads, "cand_offsets", "read");
    const uint64_t n_text = seq_offsets[n_seq], read_bytes = read_offsets[n_reads], n_cands = cand_offsets[n_reads];
    if ((n_text && !text) || (read_bytes && !reads) || (n_cands && (!cand_seq || !cand_diag))) throw Error(PGX_ERR_ARG, who + ": null argument");
    if (n_text >= (1ull << 32) - (1ull << 20)) throw Error(PGX_ERR_UNSUPPORTED, who + ": a text of " + std::to_string(n_text) + " symbols, the image holds fewer than 2^32 - 2^20");
    for (uint64_t i = 0; i < n_text; i++) {
        const uint8_t c = text[i];
        if (c != '\n' && c != 'A' && c != 'C' && c != 'G' && c != 'N' && c != 'T')
            throw Error(PGX_ERR_UNSUPPORTED, who + ": text byte " + std::to_string((unsigned)c) + " at offset " + std::to_string(i) + " is none of \\n A C G N T");
    }
    for (uint64_t r = 0; r < n_reads; r++)
        if (read_offsets[r + 1] - read_offsets[r] >= (1ull << 31))
            throw Error(PGX_ERR_UNSUPPORTED, who + ": read " + std::to_string(r) + " has " + std::to_string(read_offsets[r + 1] - read_offsets[r]) + " bytes; the records hold read positions below 2^31");
    if (n_reads >= PLACE_LAUNCH_ITEMS || n_cands >= PLACE_LAUNCH_ITEMS)
        throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_reads) + " reads with " + std::to_string(n_cands) + " candidates exceed one launch");
    if (want_list && n_cands > list_cap)
        throw Error(PGX_ERR_NOMEM, who + ": the list holds " + std::to_string(n_cands) + " candidates, list_cap is " + std::to_string(list_cap));
    use_device(device);
    struct Work { // device copies of the input + the stage's buffers, released on every way out
        DevBuf text8, text4, seq_off, reads, read_off;
        VerifyWork w;
        ~Work() {
            DevBuf *all[] = {&text8, &text4, &seq_off, &reads, &read_off};
            for (DevBuf *d : all) d->release();
            w.release();
        }
    } k;
    hipStream_t s = nullptr;
    const uint64_t n_words = (n_text + 7) / 8 + PGX_TEXT_PAD_WORDS;
    upload(k.text8, text, n_text);
    upload(k.seq_off, seq_offsets, (n_seq + 1) * 8);
    upload(k.reads, reads, read_bytes);
    upload(k.read_off, read_offsets, (n_reads + 1) * 8);
    upload(k.w.cand_off, cand_offsets, (n_reads + 1) * 8);
    upload(k.w.cand_seq, cand_seq, n_cands * 4);
    upload(k.w.cand_diag, cand_diag, n_cands * 8);
    k.w.cand_read.ensure((n_cands ? n_cands : 1) * 8);
    if (n_cands) { // the preconditions, before anything is written
        hipLaunchKernelGGL(pgx_verify_owner_kernel, dim3(grid_for(n_reads, 256)), dim3(256), 0, s, (const uint64_t *)k.w.cand_off.as<uint64_t>(), n_reads, n_cands,
                           k.w.cand_read.as<uint64_t>());
        k.w.bad.ensure(8);
        HIPCHECK(hipMemsetAsync(k.w.bad.p, 0xFF, 8, s));
        hipLaunchKernelGGL(pgx_verify_check_kernel, dim3(grid_for(n_cands, 256)), dim3(256), 0, s, (const uint64_t *)k.w.cand_read.as<uint64_t>(),
                           (const uint32_t *)k.w.cand_seq.as<uint32_t>(), n_cands, n_seq, k.w.bad.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
        const uint64_t bad = read_u64(k.w.bad.as<uint64_t>(), s);
        if (bad != ~0ull) throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(bad) + " has a candidate whose sequence is not below n_seq " + std::to_string(n_seq));
    }
    k.text4.ensure(n_words * 4);
    hipLaunchKernelGGL(pgx_text_pack_kernel, dim3((unsigned)std::min<uint64_t>((n_words + 255) / 256, 1u << 20)), dim3(256), 0, s, (const uint8_t *)k.text8.as<uint8_t>(), n_text, n_words,
                       1u, k.text4.as<uint32_t>());
    HIPCHECK(hipGetLastError());
    verify_core(k.w, k.text4.as<uint32_t>(), k.seq_off.as<uint64_t>(), 0u, k.reads.as<uint8_t>(), read_bytes, k.read_off.as<uint64_t>(), n_reads, n_cands, mismatch_penalty, s);
    if (n_reads) HIPCHECK(hipMemcpyAsync(out, k.w.recs.p, n_reads * sizeof(pgx_read_verify), hipMemcpyDeviceToHost, s));
    if (want_list) {
        HIPCHECK(hipMemcpyAsync(list_offsets, k.w.cand_off.p, (n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
        if (n_cands) HIPCHECK(hipMemcpyAsync(list, k.w.cands.p, n_cands * sizeof(pgx_read_verify), hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// read align (pgx_align_kernels.hip; the definitions: include/pgx.h "read align")
static const uint32_t ALIGN_FLAGS = PGX_ALIGN_CIGAR;
static const uint64_t ALIGN_MAX_READ = 1ull << 28; // an operation's length has 28 bits

static void align_check_args(const std::string &who, uint32_t band, uint32_t flags) {
    if (flags & ~ALIGN_FLAGS) throw Error(PGX_ERR_ARG, who + ": unknown flag");
    if (band > PGX_ALIGN_MAX_BAND) throw Error(PGX_ERR_ARG, who + ": band " + std::to_string(band) + " is outside 0 .. " + std::to_string(PGX_ALIGN_MAX_BAND));
}

// bytes of direction planes one pass may hold: PGX_ALIGN_BUDGET_MB (read per call, fractions allowed), default a quarter of the free device memory
static uint64_t align_budget_bytes(size_t mem_free) {
    uint64_t bytes = 0;
    if (const char *e = std::getenv("PGX_ALIGN_BUDGET_MB")) {
        const double mb = std::strtod(e, nullptr);
        if (mb > 0) bytes = (uint64_t)(mb * 1048576.0);
    }
    if (!bytes) bytes = mem_free / 4;
    return std::max<uint64_t>(bytes, 16);
}

struct AlignPass { uint64_t r0, r1, bytes; };

// The passes over consecutive whole reads whose planes fit the budget, from the host's read offsets: a read of len bytes takes len rows of
// row_bytes, rounded up to 16 (pgx_align_need_kernel computes the same on the device).  Throws before anything is launched.
static std::vector<AlignPass> align_plan(const uint64_t *h_read_off, uint64_t n, uint32_t row_bytes, uint64_t budget, const std::string &who) {
    std::vector<AlignPass> passes;
    AlignPass cur{0, 0, 0};
    for (uint64_t r = 0; r < n; r++) {
        const uint64_t len = h_read_off[r + 1] - h_read_off[r];
        if (len >= ALIGN_MAX_READ) throw Error(PGX_ERR_UNSUPPORTED, who + ": read " + std::to_string(r) + " has " + std::to_string(len) + " bytes; an operation's length is below 2^28");
        const uint64_t need = (len * row_bytes + 15) & ~15ull;
        if (need > budget)
            throw Error(PGX_ERR_NOMEM, who + ": read " + std::to_string(r) + " needs " + std::to_string(need) + " bytes of direction planes, a pass holds " + std::to_string(budget) +
                                           " (PGX_ALIGN_BUDGET_MB)");
        if (cur.bytes + need > budget) { passes.push_back(cur); cur = AlignPass{r, r, 0}; }
        cur.bytes += need;
        cur.r1 = r + 1;
    }
    if (cur.r1 > cur.r0) passes.push_back(cur);
    return passes;
}

template <int LG>
static void align_launch_forward(const uint32_t *text4, const uint64_t *seq_start, uint32_t endmark, const uint32_t *rcode, const uint64_t *read_off, const AlignWork &w,
                                 const AlignPass &p, uint32_t band, hipStream_t s) {
    hipLaunchKernelGGL(pgx_align_forward_kernel<LG>, dim3(grid_for(p.r1 - p.r0, PGX_ALIGN_THREADS >> LG)), dim3(PGX_ALIGN_THREADS), 0, s, text4, seq_start, endmark, rcode, read_off,
                       (const uint32_t *)w.cand_seq.as<uint32_t>(), (const int64_t *)w.cand_diag.as<int64_t>(), p.r0, p.r1, band, (const uint64_t *)w.plane_off.as<uint64_t>(),
                       w.planes.as<uint8_t>(), w.fwd.as<uint2>());
}

// The stage on device arrays, enqueued on s (synchronised where the number of operations is read back): w.cand_seq / w.cand_diag (n of each) -> w.recs,
// w.op_off and, with PGX_ALIGN_CIGAR, w.ops.  rcode: the reads coded by pgx_verify_code_kernel.  The plan was made by the caller: nothing here refuses.
// With one pass the planes stay in place between the counting walk and the writing walk; with more, the forward kernel runs again before the writing walk.
static void align_core(AlignWork &w, const uint32_t *text4, const uint64_t *seq_start, uint32_t endmark, const uint32_t *rcode, const uint64_t *read_off, uint64_t n,
                       const std::vector<AlignPass> &plan, uint32_t band, uint32_t flags, bool timed, hipStream_t s) {
    uint32_t lg = 0;
    while ((1u << lg) < 2 * band + 1) lg++;
    const uint32_t row_bytes = std::max(1u << lg, 8u) / 4;
    uint64_t scratch = 16;
    for (const AlignPass &p : plan) scratch = std::max(scratch, p.bytes);
    w.recs.ensure((n ? n : 1) * sizeof(pgx_read_align));
    w.need.ensure((n ? n : 1) * 8); w.plane_off.ensure((n + 1) * 8); w.fwd.ensure((n ? n : 1) * sizeof(uint2));
    w.count.ensure((n ? n : 1) * 8); w.op_off.ensure((n + 1) * 8);
    w.planes.ensure(scratch);
    size_t n_ev = 2;
    auto stamp = [&]() { // the next event of the call, recorded on s
        if (!timed) return;
        if (w.ev.size() <= n_ev) w.ev.resize(n_ev + 1, nullptr);
        if (!w.ev[n_ev]) HIPCHECK(hipEventCreate(&w.ev[n_ev]));
        HIPCHECK(hipEventRecord(w.ev[n_ev++], s));
    };
    std::vector<int> kinds; // of every pair of events: 0 forward, 1 trace
    auto forward = [&](const AlignPass &p) {
        stamp();
        switch (lg) {
        case 0: align_launch_forward<0>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        case 1: align_launch_forward<1>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        case 2: align_launch_forward<2>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        case 3: align_launch_forward<3>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        case 4: align_launch_forward<4>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        case 5: align_launch_forward<5>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        default: align_launch_forward<6>(text4, seq_start, endmark, rcode, read_off, w, p, band, s); break;
        }
        stamp();
        kinds.push_back(0);
    };
    auto trace = [&](const AlignPass &p, uint32_t write) {
        stamp();
        hipLaunchKernelGGL(pgx_align_trace_kernel, dim3(grid_for(p.r1 - p.r0, 256)), dim3(256), 0, s, seq_start, endmark, read_off, (const uint32_t *)w.cand_seq.as<uint32_t>(),
                           (const int64_t *)w.cand_diag.as<int64_t>(), p.r0, p.r1, band, row_bytes, (const uint64_t *)w.plane_off.as<uint64_t>(),
                           (const uint8_t *)w.planes.as<uint8_t>(), (const uint2 *)w.fwd.as<uint2>(), write, w.recs.as<pgx_read_align>(), w.count.as<uint64_t>(),
                           (const uint64_t *)w.op_off.as<uint64_t>(), w.ops.as<uint32_t>());
        stamp();
        kinds.push_back(1);
    };
    uint64_t n_ops = 0;
    if (n) {
        hipLaunchKernelGGL(pgx_align_need_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, read_off, n, row_bytes, w.need.as<uint64_t>());
        HIPCHECK(hipGetLastError());
        scan_excl(1, w.need.p, n, 0, w.plane_off.as<uint64_t>(), w.scan_tmp, s);
        for (const AlignPass &p : plan) { forward(p); trace(p, 0); }
        HIPCHECK(hipGetLastError());
        scan_excl(1, w.count.p, n, 0, w.op_off.as<uint64_t>(), w.scan_tmp, s);
        n_ops = read_u64(w.op_off.as<uint64_t>() + n, s);
    } else HIPCHECK(hipMemsetAsync(w.op_off.p, 0, 8, s));
    if ((flags & PGX_ALIGN_CIGAR) && n_ops) {
        w.ops.ensure(n_ops * 4);
        for (const AlignPass &p : plan) {
            if (plan.size() > 1) forward(p);
            trace(p, 1);
        }
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipStreamSynchronize(s));
    w.ms_forward = w.ms_trace = 0;
    for (size_t i = 0; timed && i < kinds.size(); i++) {
        float ms = 0;
        HIPCHECK(hipEventElapsedTime(&ms, w.ev[2 + 2 * i], w.ev[3 + 2 * i]));
        (kinds[i] ? w.ms_trace : w.ms_forward) += ms;
    }
    w.n_reads = n; w.n_ops = n_ops; w.flags = flags; w.band = band; w.passes = (uint32_t)plan.size(); w.scratch_bytes = plan.empty() ? 0 : scratch;
}

extern "C" pgx_status pgx_batch_read_align(pgx_batch *b, uint32_t band, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_read_align");
    checked_device_count();
    const std::string who = "pgx_batch_read_align";
    if (!b) throw Error(PGX_ERR_ARG, who + ": null batch");
    // (what is refused here leaves an earlier align result as it was)
    align_check_args(who, band, flags);
    if (!b->ran) throw Error(PGX_ERR_ARG, who + ": batch has not been run");
    VerifyWork &vw = b->vw;
    if (!vw.valid || vw.n_reads != b->n_reads) throw Error(PGX_ERR_ARG, who + ": needs a completed pgx_batch_read_verify, the batch has no verify result");
    const uint64_t n = b->n_reads;
    if (n >= PLACE_LAUNCH_ITEMS) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n) + " reads exceed one launch");
    use_device(b->device);
    pgx_device_image *d = device_image(b->h, b->device);
    ensure_text(b->h, d); // (built by the verify stage)
    uint32_t lg = 0;
    while ((1u << lg) < 2 * band + 1) lg++;
    const std::vector<AlignPass> plan = align_plan(b->h_offsets(), n, std::max(1u << lg, 8u) / 4, align_budget_bytes(free_device_memory()), who);
    hipStream_t s = stream ? (hipStream_t)stream : b->own;
    AlignWork &w = b->aw;
    w.valid = false;
    const bool timed = b->timed;
    if (timed) {
        if (w.ev.size() < 2) w.ev.resize(2, nullptr);
        for (int i = 0; i < 2; i++)
            if (!w.ev[i]) HIPCHECK(hipEventCreate(&w.ev[i]));
        HIPCHECK(hipEventRecord(w.ev[0], s));
    }
    w.cand_seq.ensure((n ? n : 1) * 4); w.cand_diag.ensure((n ? n : 1) * 8);
    if (n) {
        hipLaunchKernelGGL(pgx_align_cand_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const pgx_read_verify *)vw.recs.as<pgx_read_verify>(), n, w.cand_seq.as<uint32_t>(),
                           w.cand_diag.as<int64_t>());
        HIPCHECK(hipGetLastError());
    }
    // (the reads were coded by the verify call for all of its candidates: vw.rcode describes this run's reads)
    align_core(w, d->text4.as<uint32_t>(), d->text_seq_start.as<uint64_t>(), 1u, (const uint32_t *)vw.rcode.as<uint32_t>(), b->offsets.as<uint64_t>(), n, plan, band, flags, timed, s);
    w.ms = 0;
    if (timed) {
        HIPCHECK(hipEventRecord(w.ev[1], s));
        HIPCHECK(hipStreamSynchronize(s));
        HIPCHECK(hipEventElapsedTime(&w.ms, w.ev[0], w.ev[1]));
    }
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void aligned_header(const pgx_batch *b, pgx_read_aligns *out) {
    const AlignWork &w = b->aw;
    std::memset(out, 0, sizeof *out);
    out->n_reads = w.n_reads;
    out->n_ops = w.n_ops;
    out->flags = w.flags;
    out->band = w.band;
    out->passes = w.passes;
    out->scratch_bytes = w.scratch_bytes;
    out->ms_align = w.ms;
    out->ms_forward = w.ms_forward;
    out->ms_trace = w.ms_trace;
}

extern "C" pgx_status pgx_batch_device_aligned(pgx_batch *b, pgx_read_aligns *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->aw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_aligned: batch has no align result");
    const AlignWork &w = b->aw;
    aligned_header(b, out);
    out->reads = w.recs.as<pgx_read_align>();
    if (w.flags & PGX_ALIGN_CIGAR) {
        out->op_offsets = w.op_off.as<uint64_t>();
        out->ops = w.ops.as<uint32_t>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_aligned(pgx_batch *b, pgx_read_aligns *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->aw.valid) throw Error(PGX_ERR_ARG, "pgx_batch_aligned: batch has no align result");
    use_device(b->device);
    AlignWork &w = b->aw;
    const uint64_t n = w.n_reads;
    const bool list = (w.flags & PGX_ALIGN_CIGAR) != 0;
    w.h_recs.ensure((n ? n : 1) * sizeof(pgx_read_align));
    if (n) HIPCHECK(hipMemcpyAsync(w.h_recs.p, w.recs.p, n * sizeof(pgx_read_align), hipMemcpyDeviceToHost, b->own));
    if (list) {
        w.h_op_off.ensure((n + 1) * 8);
        w.h_ops.ensure((w.n_ops ? w.n_ops : 1) * 4);
        HIPCHECK(hipMemcpyAsync(w.h_op_off.p, w.op_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, b->own));
        if (w.n_ops) HIPCHECK(hipMemcpyAsync(w.h_ops.p, w.ops.p, w.n_ops * 4, hipMemcpyDeviceToHost, b->own));
    }
    HIPCHECK(hipStreamSynchronize(b->own)); // (the stage completed inside pgx_batch_read_align, on whatever stream it used)
    aligned_header(b, out);
    out->reads = w.h_recs.as<pgx_read_align>();
    if (list) {
        out->op_offsets = w.h_op_off.as<uint64_t>();
        out->ops = w.h_ops.as<uint32_t>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_read_align_arrays(int device, const uint8_t *text, const uint64_t *seq_offsets, uint64_t n_seq, const uint8_t *reads,
                                            const uint64_t *read_offsets, uint64_t n_reads, const uint32_t *cand_seq, const int64_t *cand_diag, uint32_t band,
                                            uint32_t flags, pgx_read_align *out, uint64_t *op_offsets, uint32_t *ops, uint64_t ops_cap) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_align_arrays");
    checked_device_count();
    const std::string who = "pgx_read_align_arrays";
    align_check_args(who, band, flags);
    const bool want_ops = (flags & PGX_ALIGN_CIGAR) != 0;
    if (!seq_offsets || !read_offsets || (n_reads && (!out || !cand_seq || !cand_diag)) || (want_ops && (!op_offsets || (ops_cap && !ops))))
        throw Error(PGX_ERR_ARG, who + ": null argument");
    auto check_offsets = [&](const uint64_t *o, uint64_t k, const char *name, const char *item) {
        if (o[0] != 0) throw Error(PGX_ERR_ARG, who + ": " + name + " must start at 0");
        for (uint64_t i = 0; i < k; i++)
            if (o[i] > o[i + 1]) throw Error(PGX_ERR_ARG, who + ": " + name + " decrease at " + item + " " + std::to_string(i));
    };
    check_offsets(seq_offsets, n_seq, "seq_offsets", "sequence");
    check_offsets(read_offsets, n_reads, "read_offsets", "read");
    const uint64_t n_text = seq_offsets[n_seq], read_bytes = read_offsets[n_reads];
    if ((n_text && !text) || (read_bytes && !reads)) throw Error(PGX_ERR_ARG, who + ": null argument");
    if (n_text >= (1ull << 32) - (1ull << 20)) throw Error(PGX_ERR_UNSUPPORTED, who + ": a text of " + std::to_string(n_text) + " symbols, the image holds fewer than 2^32 - 2^20");
    for (uint64_t i = 0; i < n_text; i++) {
        const uint8_t c = text[i];
        if (c != '\n' && c != 'A' && c != 'C' && c != 'G' && c != 'N' && c != 'T')
            throw Error(PGX_ERR_UNSUPPORTED, who + ": text byte " + std::to_string((unsigned)c) + " at offset " + std::to_string(i) + " is none of \\n A C G N T");
    }
    for (uint64_t r = 0; r < n_reads; r++)
        if (cand_seq[r] != PGX_NO_SEQUENCE && cand_seq[r] >= n_seq)
            throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(r) + " has a candidate whose sequence is not below n_seq " + std::to_string(n_seq));
    if (n_reads >= PLACE_LAUNCH_ITEMS) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_reads) + " reads exceed one launch");
    use_device(device);
    uint32_t lg = 0;
    while ((1u << lg) < 2 * band + 1) lg++;
    const std::vector<AlignPass> plan = align_plan(read_offsets, n_reads, std::max(1u << lg, 8u) / 4, align_budget_bytes(free_device_memory()), who);
    struct Work { // device copies of the input + the stage's buffers, released on every way out
        DevBuf text8, text4, seq_off, reads, read_off;
        AlignWork w;
        ~Work() {
            DevBuf *all[] = {&text8, &text4, &seq_off, &reads, &read_off};
            for (DevBuf *d : all) d->release();
            w.release();
        }
    } k;
    hipStream_t s = nullptr;
    const uint64_t n_words = (n_text + 7) / 8 + PGX_TEXT_PAD_WORDS, n_rw = (read_bytes + 7) / 8 + 1;
    upload(k.text8, text, n_text);
    upload(k.seq_off, seq_offsets, (n_seq + 1) * 8);
    upload(k.reads, reads, read_bytes);
    upload(k.read_off, read_offsets, (n_reads + 1) * 8);
    upload(k.w.cand_seq, cand_seq, n_reads * 4);
    upload(k.w.cand_diag, cand_diag, n_reads * 8);
    k.text4.ensure(n_words * 4);
    k.w.rcode.ensure(n_rw * 4);
    hipLaunchKernelGGL(pgx_text_pack_kernel, dim3((unsigned)std::min<uint64_t>((n_words + 255) / 256, 1u << 20)), dim3(256), 0, s, (const uint8_t *)k.text8.as<uint8_t>(), n_text, n_words,
                       1u, k.text4.as<uint32_t>());
    hipLaunchKernelGGL(pgx_verify_code_kernel, dim3((unsigned)std::min<uint64_t>((n_rw + 255) / 256, 1u << 20)), dim3(256), 0, s, (const uint8_t *)k.reads.as<uint8_t>(), read_bytes, n_rw,
                       k.w.rcode.as<uint32_t>());
    HIPCHECK(hipGetLastError());
    align_core(k.w, k.text4.as<uint32_t>(), k.seq_off.as<uint64_t>(), 0u, (const uint32_t *)k.w.rcode.as<uint32_t>(), k.read_off.as<uint64_t>(), n_reads, plan, band, flags, false, s);
    if (want_ops && k.w.n_ops > ops_cap)
        throw Error(PGX_ERR_NOMEM, who + ": the list holds " + std::to_string(k.w.n_ops) + " operations, ops_cap is " + std::to_string(ops_cap));
    if (n_reads) HIPCHECK(hipMemcpyAsync(out, k.w.recs.p, n_reads * sizeof(pgx_read_align), hipMemcpyDeviceToHost, s));
    if (want_ops) {
        HIPCHECK(hipMemcpyAsync(op_offsets, k.w.op_off.p, (n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
        if (k.w.n_ops) HIPCHECK(hipMemcpyAsync(ops, k.w.ops.p, k.w.n_ops * 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

// ------------------------------------------------------------------------------------------
// read walk (pgx_walk_kernels.hip; the definitions: include/pgx.h "read walk")
static const uint32_t WALK_FLAGS = PGX_WALK_STEPS;

// The stage on device arrays, enqueued on s (synchronised where the number of steps is read back): the align records, or seq / text_start / text_end
// (n of each), -> w.recs, w.step_off and, with PGX_WALK_STEPS, w.steps.  Nothing here refuses.
static void walk_core(WalkWork &w, const PgxWalkImage &img, const uint64_t *seq_start, uint32_t endmark, uint64_t n_seq, const pgx_read_align *recs, const uint32_t *seq,
                      const uint64_t *text_start, const uint64_t *text_end, uint64_t n, uint32_t flags, hipStream_t s) {
    w.recs.ensure((n ? n : 1) * sizeof(pgx_read_walk));
    w.count.ensure((n ? n : 1) * 8); w.first.ensure((n ? n : 1) * 8); w.step_off.ensure((n + 1) * 8);
    uint64_t n_steps = 0;
    if (n) {
        hipLaunchKernelGGL(pgx_walk_count_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, img, seq_start, endmark, n_seq, recs, seq, text_start, text_end, n,
                           w.recs.as<pgx_read_walk>(), w.count.as<uint64_t>(), w.first.as<uint64_t>());
        HIPCHECK(hipGetLastError());
        scan_excl(1, w.count.p, n, 0, w.step_off.as<uint64_t>(), w.scan_tmp, s);
        n_steps = read_u64(w.step_off.as<uint64_t>() + n, s); // (the stage's one read-back)
    } else HIPCHECK(hipMemsetAsync(w.step_off.p, 0, 8, s));
    if ((flags & PGX_WALK_STEPS) && n_steps) {
        w.steps.ensure(n_steps * 8);
        hipLaunchKernelGGL(pgx_walk_fill_kernel, dim3(grid_for(n, 256 / PGX_WALK_FILL_LANES)), dim3(256), 0, s, img, (const uint64_t *)w.count.as<uint64_t>(),
                           (const uint64_t *)w.first.as<uint64_t>(), (const uint64_t *)w.step_off.as<uint64_t>(), n, w.steps.as<uint64_t>());
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipStreamSynchronize(s));
    w.n_reads = n; w.n_steps = n_steps; w.flags = flags;
}

extern "C" pgx_status pgx_batch_read_walk(pgx_batch *b, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_batch_read_walk");
    checked_device_count();
    const std::string who = "pgx_batch_read_walk";
    if (!b) throw Error(PGX_ERR_ARG, who + ": null batch");
    // (what is refused here leaves an earlier walk result as it was)
    if (flags & ~WALK_FLAGS) throw Error(PGX_ERR_ARG, who + ": unknown flag");
    if (!b->ran) throw Error(PGX_ERR_ARG, who + ": batch has not been run");
    AlignWork &aw = b->aw;
    if (!aw.valid || aw.n_reads != b->n_reads) throw Error(PGX_ERR_ARG, who + ": needs a completed pgx_batch_read_align, the batch has no align result");
    const uint64_t n = b->n_reads;
    if (n >= PLACE_LAUNCH_ITEMS / PGX_WALK_FILL_LANES) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n) + " reads exceed one launch");
    use_device(b->device);
    pgx_device_image *d = device_image(b->h, b->device);
    ensure_walk(b->h, d); // (throws before anything of the batch changes)
    hipStream_t s = stream ? (hipStream_t)stream : b->own;
    WalkWork &w = b->ww;
    w.valid = false;
    const bool timed = b->timed;
    if (timed) {
        for (auto &e : w.ev)
            if (!e) HIPCHECK(hipEventCreate(&e));
        HIPCHECK(hipEventRecord(w.ev[0], s));
    }
    walk_core(w, d->walk, d->text_seq_start.as<uint64_t>(), 1u, d->text_n_seq, (const pgx_read_align *)aw.recs.as<pgx_read_align>(), nullptr, nullptr, nullptr, n, flags, s);
    w.ms = 0;
    if (timed) {
        HIPCHECK(hipEventRecord(w.ev[1], s));
        HIPCHECK(hipStreamSynchronize(s));
        HIPCHECK(hipEventElapsedTime(&w.ms, w.ev[0], w.ev[1]));
    }
    w.valid = true;
    return PGX_OK;
    PGX_GUARD_END
}

static void walked_header(const pgx_batch *b, pgx_read_walks *out) {
    const WalkWork &w = b->ww;
    std::memset(out, 0, sizeof *out);
    out->n_reads = w.n_reads;
    out->n_steps = w.n_steps;
    out->flags = w.flags;
    out->ms_walk = w.ms;
}

extern "C" pgx_status pgx_batch_device_walked(pgx_batch *b, pgx_read_walks *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->ww.valid) throw Error(PGX_ERR_ARG, "pgx_batch_device_walked: batch has no walk result");
    const WalkWork &w = b->ww;
    walked_header(b, out);
    out->reads = w.recs.as<pgx_read_walk>();
    if (w.flags & PGX_WALK_STEPS) {
        out->step_offsets = w.step_off.as<uint64_t>();
        out->steps = w.steps.as<uint64_t>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_batch_walked(pgx_batch *b, pgx_read_walks *out) {
    PGX_GUARD_BEGIN
    if (!b || !out || !b->ww.valid) throw Error(PGX_ERR_ARG, "pgx_batch_walked: batch has no walk result");
    use_device(b->device);
    WalkWork &w = b->ww;
    const uint64_t n = w.n_reads;
    const bool list = (w.flags & PGX_WALK_STEPS) != 0;
    w.h_recs.ensure((n ? n : 1) * sizeof(pgx_read_walk));
    if (n) HIPCHECK(hipMemcpyAsync(w.h_recs.p, w.recs.p, n * sizeof(pgx_read_walk), hipMemcpyDeviceToHost, b->own));
    if (list) {
        w.h_step_off.ensure((n + 1) * 8);
        w.h_steps.ensure((w.n_steps ? w.n_steps : 1) * 8);
        HIPCHECK(hipMemcpyAsync(w.h_step_off.p, w.step_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, b->own));
        if (w.n_steps) HIPCHECK(hipMemcpyAsync(w.h_steps.p, w.steps.p, w.n_steps * 8, hipMemcpyDeviceToHost, b->own));
    }
    HIPCHECK(hipStreamSynchronize(b->own)); // (the stage completed inside pgx_batch_read_walk, on whatever stream it used)
    walked_header(b, out);
    out->reads = w.h_recs.as<pgx_read_walk>();
    if (list) {
        out->step_offsets = w.h_step_off.as<uint64_t>();
        out->steps = w.h_steps.as<uint64_t>();
    }
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_read_walk_arrays(int device, const uint64_t *seq_offsets, uint64_t n_seq, const uint64_t *visit_offsets, const uint64_t *visit_nodes,
                                           const uint32_t *visit_length, uint64_t n_reads, const uint32_t *seq, const uint64_t *text_start, const uint64_t *text_end,
                                           uint32_t flags, pgx_read_walk *out, uint64_t *step_offsets, uint64_t *steps, uint64_t steps_cap) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_walk_arrays");
    checked_device_count();
    const std::string who = "pgx_read_walk_arrays";
    if (flags & ~WALK_FLAGS) throw Error(PGX_ERR_ARG, who + ": unknown flag");
    const bool want_steps = (flags & PGX_WALK_STEPS) != 0;
    if (!seq_offsets || !visit_offsets || (n_reads && (!out || !seq || !text_start || !text_end)) || (want_steps && (!step_offsets || (steps_cap && !steps))))
        throw Error(PGX_ERR_ARG, who + ": null argument");
    auto check_offsets = [&](const uint64_t *o, uint64_t k, const char *name) {
        if (o[0] != 0) throw Error(PGX_ERR_ARG, who + ": " + name + " must start at 0");
        for (uint64_t i = 0; i < k; i++)
            if (o[i] > o[i + 1]) throw Error(PGX_ERR_ARG, who + ": " + name + " decrease at sequence " + std::to_string(i));
    };
    check_offsets(seq_offsets, n_seq, "seq_offsets");
    check_offsets(visit_offsets, n_seq, "visit_offsets");
    const uint64_t n_text = seq_offsets[n_seq], V = visit_offsets[n_seq];
    if (V && (!visit_nodes || !visit_length)) throw Error(PGX_ERR_ARG, who + ": null argument");
    if (n_text >= (1ull << 32) - (1ull << 20)) throw Error(PGX_ERR_UNSUPPORTED, who + ": a text of " + std::to_string(n_text) + " symbols, the image holds fewer than 2^32 - 2^20");
    std::vector<uint64_t> marks(V);
    for (uint64_t q = 0; q < n_seq; q++) {
        uint64_t p = seq_offsets[q];
        for (uint64_t k = visit_offsets[q]; k < visit_offsets[q + 1]; k++) {
            if (visit_length[k] == 0 || visit_length[k] > PGX_WALK_MAX_VISIT)
                throw Error(PGX_ERR_ARG, who + ": visit " + std::to_string(k) + " of sequence " + std::to_string(q) + " has length " + std::to_string(visit_length[k]) + ", outside 1 .. 1024");
            marks[k] = p;
            p += visit_length[k];
        }
        if (p != seq_offsets[q + 1])
            throw Error(PGX_ERR_ARG, who + ": the visits of sequence " + std::to_string(q) + " sum to " + std::to_string(p - seq_offsets[q]) + " symbols, the sequence has " +
                                         std::to_string(seq_offsets[q + 1] - seq_offsets[q]));
    }
    for (uint64_t r = 0; r < n_reads; r++) {
        if (seq[r] == PGX_NO_SEQUENCE) continue;
        if (seq[r] >= n_seq) throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(r) + " names a sequence that is not below n_seq " + std::to_string(n_seq));
        const uint64_t ls = seq_offsets[(uint64_t)seq[r] + 1] - seq_offsets[seq[r]];
        if (text_start[r] > text_end[r] || text_end[r] > ls)
            throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(r) + " has the stretch [" + std::to_string(text_start[r]) + ", " + std::to_string(text_end[r]) +
                                         "), its sequence has " + std::to_string(ls) + " symbols");
    }
    if (n_reads >= PLACE_LAUNCH_ITEMS / PGX_WALK_FILL_LANES) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_reads) + " reads exceed one launch");
    use_device(device);
    struct Work { // device copies of the input, the image + the stage's buffers, released on every way out
        DevBuf seq_off, marks, bits, dir, nodes, counts, seq, ts, te;
        WalkWork w;
        ~Work() {
            DevBuf *all[] = {&seq_off, &marks, &bits, &dir, &nodes, &counts, &seq, &ts, &te};
            for (DevBuf *d : all) d->release();
            w.release();
        }
    } k;
    hipStream_t s = nullptr;
    const uint64_t n_blocks = n_text / PGX_WALK_BLOCK_BITS + 1, n_words = n_blocks * PGX_WALK_BLOCK_WORDS;
    upload(k.seq_off, seq_offsets, (n_seq + 1) * 8);
    upload(k.marks, marks.data(), V * 8);
    upload(k.nodes, visit_nodes, V * 8);
    upload(k.seq, seq, n_reads * 4);
    upload(k.ts, text_start, n_reads * 8);
    upload(k.te, text_end, n_reads * 8);
    k.bits.ensure(n_words * 8); k.dir.ensure((n_blocks + 1) * 8);
    HIPCHECK(hipMemsetAsync(k.bits.p, 0, n_words * 8, s));
    if (V) {
        hipLaunchKernelGGL(pgx_walk_set_kernel, dim3((unsigned)std::min<uint64_t>((V + 255) / 256, 1u << 20)), dim3(256), 0, s, (const uint64_t *)k.marks.as<uint64_t>(), V, k.bits.as<uint32_t>());
        HIPCHECK(hipGetLastError());
    }
    walk_directory(k.bits.as<uint64_t>(), n_blocks, k.counts, k.dir.as<uint64_t>(), k.w.scan_tmp, s);
    const PgxWalkImage img{k.bits.as<uint64_t>(), k.dir.as<uint64_t>(), k.nodes.as<uint64_t>(), n_text, n_words, n_blocks, V};
    walk_core(k.w, img, k.seq_off.as<uint64_t>(), 0u, n_seq, nullptr, (const uint32_t *)k.seq.as<uint32_t>(), (const uint64_t *)k.ts.as<uint64_t>(),
              (const uint64_t *)k.te.as<uint64_t>(), n_reads, flags, s);
    if (want_steps && k.w.n_steps > steps_cap)
        throw Error(PGX_ERR_NOMEM, who + ": the list holds " + std::to_string(k.w.n_steps) + " steps, steps_cap is " + std::to_string(steps_cap));
    if (n_reads) HIPCHECK(hipMemcpyAsync(out, k.w.recs.p, n_reads * sizeof(pgx_read_walk), hipMemcpyDeviceToHost, s));
    if (want_steps) {
        HIPCHECK(hipMemcpyAsync(step_offsets, k.w.step_off.p, (n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
        if (k.w.n_steps) HIPCHECK(hipMemcpyAsync(steps, k.w.steps.p, k.w.n_steps * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_find_mems_batch(pgx_index *h, int device, const uint8_t *reads, const uint64_t *offsets,
                                          uint64_t n_reads, uint64_t min_len, uint64_t min_occ, uint32_t flags,
                                          pgx_batch **batch_out, pgx_result *result_out) {
    if (!batch_out || !result_out) { pgx::set_last_error("pgx_find_mems_batch: null argument"); return PGX_ERR_ARG; }
    *batch_out = nullptr;
    pgx_batch *b = nullptr;
    pgx_status st = pgx_batch_create(h, device, reads, offsets, n_reads, &b);
    if (st == PGX_OK) st = pgx_batch_run(b, min_len, min_occ, flags, nullptr);
    if (st == PGX_OK) st = pgx_batch_result(b, result_out);
    if (st != PGX_OK) { pgx_batch_free(b); return st; }
    *batch_out = b;
    return PGX_OK;
}

// reads sharded over devices: contiguous slices, one host thread + batch + stream per slice, the index image
// replicated per device, no collective; slice i covers reads [first_read[i], first_read[i + 1])
extern "C" pgx_status pgx_find_mems_sharded(pgx_index *h, const int *devices, uint32_t n_slices, const uint8_t *reads, const uint64_t *offsets,
                                            uint64_t n_reads, uint64_t min_len, uint64_t min_occ, uint32_t flags, pgx_batch **batches_out,
                                            pgx_result *results_out, uint64_t *first_read) {
    PGX_GUARD_BEGIN
    if (!h || !devices || !n_slices || !offsets || !batches_out || !results_out || !first_read)
        throw Error(PGX_ERR_ARG, "pgx_find_mems_sharded: null argument");
    for (uint32_t i = 0; i < n_slices; i++) { batches_out[i] = nullptr; first_read[i] = n_reads * i / n_slices; }
    first_read[n_slices] = n_reads;
    for (uint32_t i = 0; i < n_slices; i++) (void)device_image(h, devices[i]); // images first: one upload per distinct device
    std::vector<pgx_status> st(n_slices, PGX_OK);
    std::vector<std::string> err(n_slices);
    std::vector<std::thread> th;
    for (uint32_t i = 0; i < n_slices; i++)
        th.emplace_back([&, i]() {
            const uint64_t a = first_read[i], b = first_read[i + 1];
            st[i] = pgx_find_mems_batch(h, devices[i], reads, offsets + a, b - a, min_len, min_occ, flags, &batches_out[i], &results_out[i]);
            if (st[i] != PGX_OK) err[i] = pgx_last_error(); // (the message is thread-local)
        });
    for (auto &t : th) t.join();
    for (uint32_t i = 0; i < n_slices; i++)
        if (st[i] != PGX_OK) {
            for (uint32_t k = 0; k < n_slices; k++) { pgx_batch_free(batches_out[k]); batches_out[k] = nullptr; }
            throw Error(st[i], "slice " + std::to_string(i) + " (device " + std::to_string(devices[i]) + "): " + err[i]);
        }
    return PGX_OK;
    PGX_GUARD_END
}
