// pgx_batch_internal.hpp -- what the units of the batch share and nobody else needs (pgx_batch.hip, pgx_batch_forms.hip, pgx_batch_locate.hip,
// pgx_read_stages.hip, pgx_pack.hip): the pgx_batch object, the work buffers of its result forms, of locate and of the read stages, and the glue around a stage call
// (its stream, its timer, the download of its result).  Nothing here is part of the C ABI, and nothing is exported from libpgx.so.
#pragma once

#include <string>

#include "pgx_runtime_internal.hpp"

#pragma GCC visibility push(hidden)

// The events around a stage call and its device time.  end() of a timed call records, waits for s and returns the time; of an untimed call it returns 0
// and leaves s alone: whether an untimed call synchronises, and where, is said by its caller.
struct StageTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool timed = false;
    void begin(bool timed_, hipStream_t s) {
        timed = timed_;
        if (!timed) return;
        for (auto &e : ev)
            if (!e) HIPCHECK(hipEventCreate(&e));
        HIPCHECK(hipEventRecord(ev[0], s));
    }
    float end(hipStream_t s) {
        float ms = 0;
        if (!timed) return ms;
        HIPCHECK(hipEventRecord(ev[1], s));
        HIPCHECK(hipStreamSynchronize(s));
        HIPCHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        return ms;
    }
    void release() { destroy_events(ev); }
};

// where the result of a read stage lies on the device: n records, and with `list` the n + 1 offsets and the n_list items they index
struct StageResult {
    uint64_t n;
    const void *recs;
    size_t rec_bytes;
    bool list;
    const void *off;
    uint64_t n_list;
    const void *items;
    size_t item_bytes;
};

// a stage's result to three host arrays, async on s (off and items are touched with the list alone)
inline void download_result(const StageResult &r, void *recs, void *off, void *items, hipStream_t s) {
    if (r.n) HIPCHECK(hipMemcpyAsync(recs, r.recs, r.n * r.rec_bytes, hipMemcpyDeviceToHost, s));
    if (!r.list) return;
    HIPCHECK(hipMemcpyAsync(off, r.off, (r.n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (r.n_list) HIPCHECK(hipMemcpyAsync(items, r.items, r.n_list * r.item_bytes, hipMemcpyDeviceToHost, s));
}

// pgx_batch_locate's buffers (grow-only, kept with the batch like its other result buffers) and its result
struct LocWork {
    DevBuf cnt, qs, qe, voff, uoff, vals, gbuf, run0, npieces, poff, seg, lists, need, soff, scratch, ucount, uloc, ctr, scan_tmp, sets;
    HostBuf h_off, h_vals;
    StageTimer timer;
    bool valid = false, resident = false;
    uint32_t flags = 0, set_words = 0; // set_words: W when the call built sequence sets (the set form, or the unique ids expanded from them)
    uint64_t n_mems = 0, n_values = 0, n_not_located = 0;
    const uint64_t *d_off = nullptr; // voff, or uoff with PGX_LOCATE_UNIQUE / PGX_LOCATE_SEQ_SETS
    float ms = 0;
    void release() {
        release_all({&cnt, &qs, &qe, &voff, &uoff, &vals, &gbuf, &run0, &npieces, &poff, &seg, &lists, &need, &soff, &scratch, &ucount, &uloc, &ctr, &scan_tmp, &sets});
        release_all({&h_off, &h_vals}); timer.release(); valid = false;
    }
};

// pgx_batch_read_hits' buffers (grow-only) and its result; pgx_read_hits_arrays uses one of its own
struct HitsWork {
    DevBuf hits, best_sets, scores, bad;
    HostBuf h_hits, h_best_sets, h_scores;
    StageTimer timer;
    bool valid = false;
    uint32_t flags = 0, set_words = 0;
    uint64_t n_reads = 0, n_seq = 0;
    float ms = 0;
    void release() {
        release_all({&hits, &best_sets, &scores, &bad});
        release_all({&h_hits, &h_best_sets, &h_scores}); timer.release(); valid = false;
    }
};

// pgx_batch_read_place's buffers (grow-only, its own: a later locate leaves them alone) and its result; pgx_read_place_arrays uses one of its own
struct PlaceWork {
    DevBuf recs, pcount, place_off, places, aoff, acnt, mfirst, keys, seg, lists, need, soff, scratch, ucount, loff, ctr, scan_tmp, bad;
    HostBuf h_recs, h_place_off, h_places;
    StageTimer timer;
    bool valid = false;
    uint32_t flags = 0, n_passes = 0;
    uint64_t n_reads = 0, n_anchors = 0, n_places = 0;
    float ms = 0;
    StageResult result() const { return {n_reads, recs.p, sizeof(pgx_read_place), (flags & PGX_PLACE_LIST) != 0, place_off.p, n_places, places.p, sizeof(pgx_placement)}; }
    void release() {
        release_all({&recs, &pcount, &place_off, &places, &aoff, &acnt, &mfirst, &keys, &seg, &lists, &need, &soff, &scratch, &ucount, &loff, &ctr, &scan_tmp, &bad});
        release_all({&h_recs, &h_place_off, &h_places}); timer.release(); valid = false;
    }
};

// pgx_batch_read_verify's buffers (grow-only, its own: a later locate leaves them alone) and its result; pgx_read_verify_arrays uses one of its own
struct VerifyWork {
    DevBuf recs, count, cand_off, cand_seq, cand_diag, cand_read, cands, rcode, scan_tmp, bad;
    HostBuf h_recs, h_cand_off, h_cands;
    StageTimer timer;
    bool valid = false;
    uint32_t flags = 0, max_cand = 0, penalty = 0;
    uint32_t max_list = 0; // the longest list: max_cand, or max_cand + 1 <= 64 behind a merge of pgx_batch_read_rescue (sizes the lane group of mates)
    bool merged = false;   // a rescue call has appended its candidates: cand_seq / cand_diag / cand_read describe the list before it
    uint64_t gen = 0;      // counts the verify calls and merges of the batch: what was made from the list says which list it was (MatesWork.verify_gen)
    uint64_t n_reads = 0, n_cands = 0;
    float ms = 0;
    StageResult result() const { return {n_reads, recs.p, sizeof(pgx_read_verify), (flags & PGX_VERIFY_LIST) != 0, cand_off.p, n_cands, cands.p, sizeof(pgx_read_verify)}; }
    void release() {
        release_all({&recs, &count, &cand_off, &cand_seq, &cand_diag, &cand_read, &cands, &rcode, &scan_tmp, &bad});
        release_all({&h_recs, &h_cand_off, &h_cands}); timer.release(); valid = false;
    }
};

// pgx_batch_read_mates' buffers (grow-only, its own) and its result; pgx_read_mates_arrays uses one of its own
struct MatesWork {
    DevBuf recs, ctr; // ctr: the four counters
    HostBuf h_recs;
    StageTimer timer;
    bool valid = false;
    uint32_t flags = 0, penalty = 0;
    int64_t frag_min = 0, frag_max = 0;
    uint64_t n_pairs = 0, counters[4] = {0, 0, 0, 0}; // pairs PROPER, COMPATIBLE, with A moved, with B moved
    uint64_t verify_gen = 0; // VerifyWork.gen of the list the pairs were made from (pgx_batch_read_mapq asks)
    float ms = 0;
    void release() {
        release_all({&recs, &ctr});
        release_all({&h_recs}); timer.release(); valid = false;
    }
};

// pgx_batch_read_rescue's buffers (grow-only, its own) and its result; pgx_read_rescue_arrays uses one of its own
struct RescueWork {
    MatesWork mates; // the pair records under this call's frag bounds, without ELECT: n_compatible and the solo winners are read from them
    DevBuf recs, task_count, task_off, tasks, best, ctr, scan_tmp;
    // MERGE: the rescued reads' flags and slots, their candidate arrays and verified records, the new list (swapped with the verify result's)
    DevBuf rescued, res_off, cand_read, cand_seq, cand_diag, fake_off, res_cands, new_count, new_off, new_cands;
    HostBuf h_recs;
    StageTimer timer;
    bool valid = false;
    uint32_t flags = 0, min_score = 0, max_anchors = 0, penalty = 0;
    int64_t frag_min = 0, frag_max = 0;
    uint64_t n_reads = 0, counters[5] = {0, 0, 0, 0, 0}; // targets, rescued, full, tasks, diagonals
    float ms = 0;
    void release() {
        mates.release();
        release_all({&recs, &task_count, &task_off, &tasks, &best, &ctr, &scan_tmp, &rescued, &res_off, &cand_read, &cand_seq, &cand_diag, &fake_off, &res_cands, &new_count,
                     &new_off, &new_cands});
        release_all({&h_recs}); timer.release(); valid = false;
    }
};

// pgx_batch_read_align's buffers (grow-only, its own) and its result; pgx_read_align_arrays uses one of its own
struct AlignWork {
    DevBuf recs, cand_seq, cand_diag, need, plane_off, planes, fwd, count, op_off, ops, rcode, scan_tmp;
    HostBuf h_recs, h_op_off, h_ops;
    StageTimer timer;
    std::vector<hipEvent_t> ev; // a pair a launch of the forward and of the trace kernel
    bool valid = false;
    uint32_t flags = 0, band = 0, passes = 0;
    uint64_t n_reads = 0, n_ops = 0, scratch_bytes = 0;
    float ms = 0, ms_forward = 0, ms_trace = 0;
    StageResult result() const { return {n_reads, recs.p, sizeof(pgx_read_align), (flags & PGX_ALIGN_CIGAR) != 0, op_off.p, n_ops, ops.p, 4}; }
    void release() {
        release_all({&recs, &cand_seq, &cand_diag, &need, &plane_off, &planes, &fwd, &count, &op_off, &ops, &rcode, &scan_tmp});
        release_all({&h_recs, &h_op_off, &h_ops}); timer.release(); destroy_events(ev); ev.clear(); valid = false;
    }
};

// pgx_batch_read_walk's buffers (grow-only, its own) and its result; pgx_read_walk_arrays uses one of its own
struct WalkWork {
    DevBuf recs, count, first, step_off, steps, scan_tmp;
    HostBuf h_recs, h_step_off, h_steps;
    StageTimer timer;
    bool valid = false;
    uint32_t flags = 0;
    uint64_t n_reads = 0, n_steps = 0;
    float ms = 0;
    StageResult result() const { return {n_reads, recs.p, sizeof(pgx_read_walk), (flags & PGX_WALK_STEPS) != 0, step_off.p, n_steps, steps.p, 8}; }
    void release() {
        release_all({&recs, &count, &first, &step_off, &steps, &scan_tmp});
        release_all({&h_recs, &h_step_off, &h_steps}); timer.release(); valid = false;
    }
};

// pgx_batch_read_mapq's buffers (grow-only, its own) and its result; pgx_read_mapq_arrays uses one of its own
struct MapqWork {
    DevBuf recs, ctr; // ctr: the four counters
    // the extras: their counts and offsets, whether a read has more than were taken, the candidate arrays pgx_verify_kernel takes, their verified records
    DevBuf count, extra_off, more, cand_seq, cand_diag, cand_read, extras, scan_tmp;
    HostBuf h_recs;
    StageTimer timer;
    bool valid = false;
    uint32_t scale = 0, slack = 0, max_extra = 0, flags = 0;
    uint64_t n_reads = 0, n_extras = 0, counters[4] = {0, 0, 0, 0}; // reads with HAS, of them with E == 0, reads CAPPED, the sum of mapq
    float ms = 0;
    void release() {
        release_all({&recs, &ctr, &count, &extra_off, &more, &cand_seq, &cand_diag, &cand_read, &extras, &scan_tmp});
        release_all({&h_recs}); timer.release(); valid = false;
    }
};

struct pgx_chunk { uint64_t r0, r1, slot_base, slots; }; // consecutive reads sharing one pass over the slot buffer

// the compact result form (pgx_batch_result_compact; pgx_compact_encode uses one of its own): grow-only like the other result buffers
struct CompactWork {
    DevBuf sizes, tab, bytes, scan_tmp; // padded bytes per block; block_offsets | block_first_mem | block_first_pos; the stream
    HostBuf h_tab, h_bytes;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // around the sizing kernel + scan, around the fill kernel
    void release() {
        release_all({&sizes, &tab, &bytes, &scan_tmp});
        release_all({&h_tab, &h_bytes}); destroy_events(ev);
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
        release_all({&plen, &pcum, &vlen, &vcum, &mlen, &mcum, &rlen, &roff, &elen, &eoff, &pbase, &vbase, &text, &etext, &scan_tmp});
        release_all({&h_roff[0], &h_roff[1], &h_text[0], &h_text[1], &h_etext[0], &h_etext[1]}); destroy_events(ev);
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
    RescueWork rw;  // pgx_batch_read_rescue
    MatesWork mw;   // pgx_batch_read_mates
    AlignWork aw;   // pgx_batch_read_align
    WalkWork ww;    // pgx_batch_read_walk
    MapqWork qw;    // pgx_batch_read_mapq
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

// the stream a stage call of the batch works on: the caller's, or the batch's own
inline hipStream_t batch_stream(const pgx_batch *b, void *stream) { return stream ? (hipStream_t)stream : b->own; }

// A stage's result into the batch's pinned buffers (grown first) on its own stream, and the wait for it: the stage completed inside its call, on whatever
// stream it used.
inline void download_pinned(pgx_batch *b, const StageResult &r, HostBuf &recs, HostBuf &off, HostBuf &items) {
    recs.ensure((r.n ? r.n : 1) * r.rec_bytes);
    if (r.list) {
        off.ensure((r.n + 1) * 8);
        items.ensure((r.n_list ? r.n_list : 1) * r.item_bytes);
    }
    download_result(r, recs.p, off.p, items.p, b->own);
    HIPCHECK(hipStreamSynchronize(b->own));
}

// pgx_read_stages.hip: what the _arrays entry points share with pgx_pack.hip
size_t free_device_memory();
// what they ask of an offsets array of k items (o[k] is read)
void check_offsets(const std::string &who, const uint64_t *o, uint64_t k, const char *name, const char *item);
// what those that take path tables (walk, mapq, pack) ask of them, and the text position of every visit
std::vector<uint64_t> walk_table_marks(const std::string &who, const uint64_t *seq_offsets, uint64_t n_seq, const uint64_t *visit_offsets, const uint64_t *visit_nodes,
                                       const uint32_t *visit_length);

// the WALK image of stated path tables on the device (null stream), released on every way out
struct WalkTables {
    DevBuf seq_off, marks, bits, dir, nodes, counts, scan_tmp;
    ~WalkTables() { release_all({&seq_off, &marks, &bits, &dir, &nodes, &counts, &scan_tmp}); }
    PgxWalkImage build(const uint64_t *seq_offsets, uint64_t n_seq, const std::vector<uint64_t> &m, const uint64_t *visit_nodes, hipStream_t s) {
        const uint64_t n_text = seq_offsets[n_seq], V = m.size();
        const uint64_t n_blocks = n_text / PGX_WALK_BLOCK_BITS + 1, n_words = n_blocks * PGX_WALK_BLOCK_WORDS;
        upload(seq_off, seq_offsets, (n_seq + 1) * 8);
        upload(marks, m.data(), V * 8);
        upload(nodes, visit_nodes, V * 8);
        bits.ensure(n_words * 8); dir.ensure((n_blocks + 1) * 8);
        HIPCHECK(hipMemsetAsync(bits.p, 0, n_words * 8, s));
        if (V) {
            hipLaunchKernelGGL(pgx_walk_set_kernel, dim3((unsigned)std::min<uint64_t>((V + 255) / 256, 1u << 20)), dim3(256), 0, s, (const uint64_t *)marks.as<uint64_t>(), V, bits.as<uint32_t>());
            HIPCHECK(hipGetLastError());
        }
        walk_directory(bits.as<uint64_t>(), n_blocks, counts, dir.as<uint64_t>(), scan_tmp, s);
        return PgxWalkImage{bits.as<uint64_t>(), dir.as<uint64_t>(), nodes.as<uint64_t>(), n_text, n_words, n_blocks, V};
    }
};

#pragma GCC visibility pop
