// pgx_pack.hip -- read pack (include/pgx.h "read pack"; the kernels: pgx_pack_kernels.hip): the pgx_pack object, which accumulates the coverage of every
// graph base over the batches of a run, and pgx_read_pack_arrays, the same kernels on stated tables.  Both stand on PackCore: the node table, the
// difference array in text coordinates, the coverage vector and the fold between them.
#include <memory>
#include <mutex>
#include <string>

#include "pgx_batch_internal.hpp"

namespace {

static const uint32_t PACK_MAX_MAPQ = 60;
static const uint64_t PACK_LAUNCH_READS = 1ull << 31; // a lane a read: a grid holds fewer than 2^32 threads

struct PackCore {
    DevBuf tdiff, cov, node_len, node_base, len_max, tile_sums, tile_off, scan_tmp, ctr, covered, sum, max;
    PgxWalkImage walk{};
    const uint64_t *seq_start = nullptr; // n_seq + 1; sequence q has seq_start[q + 1] - seq_start[q] - endmark symbols
    uint64_t n_seq = 0, n = 0, n_nodes = 0, G = 0, n_tiles = 0;
    uint32_t endmark = 0;
    // ctr: [0] reads counted [1] reads filtered out [2] bases added [3] positions projected [4] max_id [5] the smallest id with two lengths
    //      [6] the smallest id with a visit of more than 1024 symbols
    unsigned long long *counters() const { return ctr.as<unsigned long long>(); }
    PgxPackTable table() const { return PgxPackTable{node_len.as<uint32_t>(), node_base.as<uint64_t>(), n_nodes}; }
    void release() { release_all({&tdiff, &cov, &node_len, &node_base, &len_max, &tile_sums, &tile_off, &scan_tmp, &ctr, &covered, &sum, &max}); }

    // the node table of `walk`, then the zeroed state; on stream s, synchronised where a size is read back
    void build(const std::string &who, hipStream_t s) {
        n = walk.n;
        const uint64_t V = walk.n_visits;
        ctr.ensure(64);
        HIPCHECK(hipMemsetAsync(ctr.p, 0, 40, s));
        HIPCHECK(hipMemsetAsync(ctr.as<uint8_t>() + 40, 0xFF, 16, s));
        uint64_t max_id = 0;
        if (V) {
            hipLaunchKernelGGL(pgx_pack_max_id_kernel, dim3((unsigned)std::min<uint64_t>((V + 255) / 256, 4096)), dim3(256), 0, s, walk.nodes, V, counters() + 4);
            HIPCHECK(hipGetLastError());
            max_id = read_u64(ctr.as<uint64_t>() + 4, s);
            if (max_id + 2 > (1ull << 32))
                throw Error(PGX_ERR_UNSUPPORTED, who + ": the largest node id is " + std::to_string(max_id) + ", the dense node table holds ids below 2^32 - 1");
        }
        n_nodes = V ? max_id + 1 : 0;
        n_tiles = (n + 1 + PGX_SCAN_BLOCK_ITEMS - 1) / PGX_SCAN_BLOCK_ITEMS;
        {   // G is known behind the table only and is at most the text: the check takes n in its place
            const uint64_t need = 4 * (n + 1) + 4 * n + 12 * (n_nodes + 1) + 4 * n_nodes + 16 * n_nodes + 16 * (n_tiles + 1) + (1ull << 16); // (with the summary and len_max)
            const size_t mem_free = free_device_memory();
            if (need > mem_free) throw Error(PGX_ERR_NOMEM, who + ": the pack takes " + std::to_string(need) + " bytes of device memory, " + std::to_string(mem_free) + " are free");
        }
        const uint64_t nn = n_nodes ? n_nodes : 1;
        node_len.ensure(nn * 4); len_max.ensure(nn * 4); node_base.ensure((n_nodes + 1) * 8);
        HIPCHECK(hipMemsetAsync(node_len.p, 0xFF, nn * 4, s));
        HIPCHECK(hipMemsetAsync(len_max.p, 0, nn * 4, s));
        if (V) {
            hipLaunchKernelGGL(pgx_pack_visit_len_kernel, dim3((unsigned)std::min<uint64_t>((walk.n_words + 255) / 256, 1u << 20)), dim3(256), 0, s, walk, seq_start, n_seq, endmark,
                               n_nodes, node_len.as<uint32_t>(), len_max.as<uint32_t>(), counters() + 5, counters() + 6);
            hipLaunchKernelGGL(pgx_pack_node_len_kernel, dim3((unsigned)std::min<uint64_t>((n_nodes + 255) / 256, 1u << 20)), dim3(256), 0, s, node_len.as<uint32_t>(),
                               (const uint32_t *)len_max.as<uint32_t>(), n_nodes, counters() + 5);
            HIPCHECK(hipGetLastError());
            uint64_t found[2];
            read_scalars(found, ctr.as<uint64_t>() + 5, 16, s);
            const uint64_t bad = found[0], too_long = found[1];
            if (too_long != ~0ull && too_long <= bad)
                throw Error(PGX_ERR_FORMAT, who + ": the tags do not describe whole-node paths: node " + std::to_string(too_long) + " has a visit of more than " +
                                                std::to_string(PGX_WALK_MAX_VISIT) + " symbols");
            if (bad != ~0ull) throw Error(PGX_ERR_FORMAT, who + ": the tags do not describe whole-node paths: node " + std::to_string(bad) + " is visited with more than one length");
        }
        scan_excl(0, node_len.p, n_nodes, 0, node_base.as<uint64_t>(), scan_tmp, s);
        G = read_u64(node_base.as<uint64_t>() + n_nodes, s);
        len_max.release();
        cov.ensure((G ? G : 1) * 4); tdiff.ensure((n + 1) * 4);
        covered.ensure(nn * 4); sum.ensure(nn * 8); max.ensure(nn * 4); // (the summary: sized here, so that no finish can run out of memory)
        tile_sums.ensure(n_tiles * 8); tile_off.ensure((n_tiles + 1) * 8);
        HIPCHECK(hipMemsetAsync(cov.p, 0, (G ? G : 1) * 4, s));
        HIPCHECK(hipMemsetAsync(tdiff.p, 0, (n + 1) * 4, s));
        HIPCHECK(hipStreamSynchronize(s));
    }

    void add(const pgx_read_align *recs, const uint32_t *seq, const uint64_t *text_start, const uint64_t *op_off, const uint32_t *ops, const pgx_read_mapq *mapqs,
             const uint8_t *keep, uint32_t min_mapq, uint64_t n_reads, hipStream_t s) const {
        if (!n_reads) return;
        hipLaunchKernelGGL(pgx_pack_add_kernel, dim3(grid_for(n_reads, PGX_PACK_THREADS)), dim3(PGX_PACK_THREADS), 0, s, recs, seq, text_start, op_off, ops, mapqs, keep, min_mapq,
                           n_reads, seq_start, n_seq, n, tdiff.as<int>(), counters());
        HIPCHECK(hipGetLastError());
    }

    // tdiff -> cov (tdiff is all zero behind it), then the summary; enqueued on s
    void fold(hipStream_t s) {
        hipLaunchKernelGGL(pgx_pack_tile_sum_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, (const int *)tdiff.as<int>(), n + 1, tile_sums.as<uint64_t>());
        HIPCHECK(hipGetLastError());
        scan_excl(1, tile_sums.p, n_tiles, 0, tile_off.as<uint64_t>(), scan_tmp, s);
        hipLaunchKernelGGL(pgx_pack_fold_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, tdiff.as<int>(), n + 1, (const uint64_t *)tile_off.as<uint64_t>(), walk, table(),
                           cov.as<uint32_t>(), counters() + 3);
        if (n_nodes)
            hipLaunchKernelGGL(pgx_pack_summary_kernel, dim3(grid_for(n_nodes * PGX_PACK_NODE_LANES, 256)), dim3(256), 0, s, table(), (const uint32_t *)cov.as<uint32_t>(),
                               covered.as<uint32_t>(), sum.as<uint64_t>(), max.as<uint32_t>());
        HIPCHECK(hipGetLastError());
    }
};

} // namespace

struct pgx_pack {
    pgx_index *h = nullptr;
    int device = 0;
    PackCore c;
    hipStream_t own = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    HostBuf h_base, h_len, h_cov, h_covered, h_sum, h_max;
    std::mutex mu; // ms_add_total (several threads add at once)
    double ms_add_total = 0;
    float ms_fold = 0, ms_table = 0;
    uint64_t counters[4] = {0, 0, 0, 0};
    bool finished = false;
};

static void pack_release(pgx_pack *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    p->c.release();
    release_all({&p->h_base, &p->h_len, &p->h_cov, &p->h_covered, &p->h_sum, &p->h_max});
    destroy_events(p->ev);
    if (p->own) (void)hipStreamDestroy(p->own);
    delete p;
}

extern "C" pgx_status pgx_pack_create(pgx_index *h, int device, pgx_pack **out) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_pack_create");
    checked_device_count();
    const std::string who = "pgx_pack_create";
    if (!h || !out) throw Error(PGX_ERR_ARG, who + ": null argument");
    *out = nullptr;
    use_device(device);
    pgx_device_image *d = device_image(h, device);
    ensure_walk(h, d); // (builds the TEXT image too; its refusals are this call's)
    std::unique_ptr<pgx_pack, void (*)(pgx_pack *)> p(new pgx_pack(), pack_release);
    p->h = h;
    p->device = device;
    HIPCHECK(hipStreamCreateWithFlags(&p->own, hipStreamNonBlocking));
    for (auto &e : p->ev) HIPCHECK(hipEventCreate(&e));
    PackCore &c = p->c;
    c.walk = d->walk;
    c.seq_start = d->text_seq_start.as<uint64_t>();
    c.n_seq = d->text_n_seq;
    c.endmark = 1u;
    HIPCHECK(hipDeviceSynchronize()); // (the images were built on the null stream)
    HIPCHECK(hipEventRecord(p->ev[0], p->own));
    c.build(who, p->own);
    HIPCHECK(hipEventRecord(p->ev[1], p->own));
    HIPCHECK(hipStreamSynchronize(p->own));
    HIPCHECK(hipEventElapsedTime(&p->ms_table, p->ev[0], p->ev[1]));
    *out = p.release();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" void pgx_pack_free(pgx_pack *p) { pack_release(p); }

extern "C" pgx_status pgx_pack_add(pgx_pack *p, pgx_batch *b, uint32_t min_mapq, uint32_t flags, void *stream) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_pack_add");
    checked_device_count();
    const std::string who = "pgx_pack_add";
    if (!p) throw Error(PGX_ERR_ARG, who + ": null pack");
    if (!b) throw Error(PGX_ERR_ARG, who + ": null batch");
    if (flags) throw Error(PGX_ERR_ARG, who + ": unknown flag");
    if (min_mapq > PACK_MAX_MAPQ) throw Error(PGX_ERR_ARG, who + ": min_mapq " + std::to_string(min_mapq) + " exceeds " + std::to_string(PACK_MAX_MAPQ));
    if (b->h != p->h) throw Error(PGX_ERR_ARG, who + ": the batch belongs to another index than the pack");
    if (b->device != p->device) throw Error(PGX_ERR_ARG, who + ": the batch lives on device " + std::to_string(b->device) + ", the pack on device " + std::to_string(p->device));
    if (!b->ran) throw Error(PGX_ERR_ARG, who + ": batch has not been run");
    const AlignWork &aw = b->aw;
    const uint64_t n = b->n_reads;
    if (!aw.valid || aw.n_reads != n) throw Error(PGX_ERR_ARG, who + ": needs a completed pgx_batch_read_align(PGX_ALIGN_CIGAR), the batch has no align result");
    if (!(aw.flags & PGX_ALIGN_CIGAR)) throw Error(PGX_ERR_ARG, who + ": needs an align result made with PGX_ALIGN_CIGAR, the last pgx_batch_read_align ran with flags " + std::to_string(aw.flags));
    const MapqWork &qw = b->qw;
    if (min_mapq > 0 && (!qw.valid || qw.n_reads != n))
        throw Error(PGX_ERR_ARG, who + ": min_mapq " + std::to_string(min_mapq) + " needs a completed pgx_batch_read_mapq, the batch has no mapq result");
    if (n >= PACK_LAUNCH_READS) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n) + " reads exceed one launch");
    use_device(p->device);
    hipStream_t s = batch_stream(b, stream);
    StageTimer timer; // (the call's own: several threads add at once)
    try {
        timer.begin(b->timed, s);
        p->c.add(aw.recs.as<pgx_read_align>(), nullptr, nullptr, aw.op_off.as<uint64_t>(), aw.ops.as<uint32_t>(), min_mapq > 0 ? qw.recs.as<pgx_read_mapq>() : nullptr, nullptr,
                 min_mapq, n, s);
        const float ms = timer.end(s);
        if (!b->timed) HIPCHECK(hipStreamSynchronize(s)); // (a timed call has waited in end())
        timer.release();
        std::lock_guard<std::mutex> lock(p->mu);
        p->ms_add_total += ms;
    } catch (...) { timer.release(); throw; }
    return PGX_OK;
    PGX_GUARD_END
}

static void pack_header(const pgx_pack *p, pgx_pack_result *out) {
    std::memset(out, 0, sizeof *out);
    out->n_nodes = p->c.n_nodes;
    out->n_bases = p->c.G;
    out->n_text = p->c.n;
    out->reads_counted = p->counters[0]; out->reads_filtered = p->counters[1]; out->bases_added = p->counters[2]; out->n_projected = p->counters[3];
    out->ms_add_total = p->ms_add_total;
    out->ms_fold = p->ms_fold;
    out->ms_table = p->ms_table;
}

extern "C" pgx_status pgx_pack_finish(pgx_pack *p, pgx_pack_result *out) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_pack_finish");
    if (!p || !out) throw Error(PGX_ERR_ARG, "pgx_pack_finish: null argument");
    use_device(p->device);
    std::lock_guard<std::mutex> lock(p->mu);
    PackCore &c = p->c;
    hipStream_t s = p->own;
    HIPCHECK(hipEventRecord(p->ev[0], s));
    c.fold(s);
    HIPCHECK(hipEventRecord(p->ev[1], s));
    const uint64_t nn = c.n_nodes, G = c.G;
    p->h_base.ensure((nn + 1) * 8); p->h_len.ensure((nn ? nn : 1) * 4); p->h_cov.ensure((G ? G : 1) * 4);
    p->h_covered.ensure((nn ? nn : 1) * 4); p->h_sum.ensure((nn ? nn : 1) * 8); p->h_max.ensure((nn ? nn : 1) * 4);
    HIPCHECK(hipMemcpyAsync(p->h_base.p, c.node_base.p, (nn + 1) * 8, hipMemcpyDeviceToHost, s));
    if (nn) {
        HIPCHECK(hipMemcpyAsync(p->h_len.p, c.node_len.p, nn * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(p->h_covered.p, c.covered.p, nn * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(p->h_sum.p, c.sum.p, nn * 8, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(p->h_max.p, c.max.p, nn * 4, hipMemcpyDeviceToHost, s));
    }
    if (G) HIPCHECK(hipMemcpyAsync(p->h_cov.p, c.cov.p, G * 4, hipMemcpyDeviceToHost, s));
    read_scalars(p->counters, c.ctr.p, 32, s); // (waits for the stream)
    HIPCHECK(hipEventElapsedTime(&p->ms_fold, p->ev[0], p->ev[1]));
    p->finished = true;
    pack_header(p, out);
    out->node_base = p->h_base.as<uint64_t>();
    out->node_length = p->h_len.as<uint32_t>();
    out->cov = p->h_cov.as<uint32_t>();
    out->covered = p->h_covered.as<uint32_t>();
    out->sum = p->h_sum.as<uint64_t>();
    out->max = p->h_max.as<uint32_t>();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_pack_device_result(pgx_pack *p, pgx_pack_result *out) {
    PGX_GUARD_BEGIN
    if (!p || !out || !p->finished) throw Error(PGX_ERR_ARG, "pgx_pack_device_result: the pack has no finished result");
    std::lock_guard<std::mutex> lock(p->mu);
    const PackCore &c = p->c;
    pack_header(p, out);
    out->node_base = c.node_base.as<uint64_t>();
    out->node_length = c.node_len.as<uint32_t>();
    out->cov = c.cov.as<uint32_t>();
    out->covered = c.covered.as<uint32_t>();
    out->sum = c.sum.as<uint64_t>();
    out->max = c.max.as<uint32_t>();
    return PGX_OK;
    PGX_GUARD_END
}

extern "C" pgx_status pgx_read_pack_arrays(int device, const uint64_t *seq_offsets, uint64_t n_seq, const uint64_t *visit_offsets, const uint64_t *visit_nodes,
                                           const uint32_t *visit_length, uint64_t n_reads, const uint32_t *seq, const uint64_t *text_start, const uint64_t *op_offsets,
                                           const uint32_t *ops, const uint8_t *keep, uint64_t *n_nodes, uint64_t *n_bases, uint64_t *node_base, uint32_t *node_length,
                                           uint32_t *covered, uint64_t *sum, uint32_t *max, uint64_t nodes_cap, uint32_t *cov, uint64_t cov_cap, uint64_t *counters) {
    PGX_GUARD_BEGIN
    RoctxRange range("pgx_read_pack_arrays");
    checked_device_count();
    const std::string who = "pgx_read_pack_arrays";
    if (!seq_offsets || !visit_offsets || !n_nodes || !n_bases || !node_base || !counters || (n_reads && (!seq || !text_start || !op_offsets)) ||
        (nodes_cap && (!node_length || !covered || !sum || !max)) || (cov_cap && !cov))
        throw Error(PGX_ERR_ARG, who + ": null argument");
    const std::vector<uint64_t> marks = walk_table_marks(who, seq_offsets, n_seq, visit_offsets, visit_nodes, visit_length);
    uint64_t n_ops = 0;
    if (n_reads) {
        check_offsets(who, op_offsets, n_reads, "op_offsets", "read");
        n_ops = op_offsets[n_reads];
        if (n_ops && !ops) throw Error(PGX_ERR_ARG, who + ": null argument");
    }
    for (uint64_t r = 0; r < n_reads; r++) {
        uint64_t consumed = 0;
        for (uint64_t j = op_offsets[r]; j < op_offsets[r + 1]; j++) {
            const uint32_t op = ops[j] & 15u;
            if (op != PGX_ALIGN_OP_I && op != PGX_ALIGN_OP_D && op != PGX_ALIGN_OP_S && op != PGX_ALIGN_OP_EQ && op != PGX_ALIGN_OP_X)
                throw Error(PGX_ERR_ARG, who + ": operation " + std::to_string(j - op_offsets[r]) + " of read " + std::to_string(r) + " has the code " + std::to_string(op) + ", none of I D S = X");
            if (op == PGX_ALIGN_OP_D || op == PGX_ALIGN_OP_EQ || op == PGX_ALIGN_OP_X) consumed += ops[j] >> 4;
        }
        if (seq[r] == PGX_NO_SEQUENCE) continue;
        if (seq[r] >= n_seq) throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(r) + " names a sequence that is not below n_seq " + std::to_string(n_seq));
        const uint64_t ls = seq_offsets[(uint64_t)seq[r] + 1] - seq_offsets[seq[r]];
        if (text_start[r] > ls) throw Error(PGX_ERR_ARG, who + ": read " + std::to_string(r) + " starts at " + std::to_string(text_start[r]) + ", its sequence has " + std::to_string(ls) + " symbols");
        if (consumed > ls - text_start[r])
            throw Error(PGX_ERR_ARG, who + ": the CIGAR of read " + std::to_string(r) + " consumes " + std::to_string(consumed) + " symbols of text from " + std::to_string(text_start[r]) +
                                         ", its sequence has " + std::to_string(ls));
    }
    if (n_reads >= PACK_LAUNCH_READS) throw Error(PGX_ERR_UNSUPPORTED, who + ": " + std::to_string(n_reads) + " reads exceed one launch");
    use_device(device);
    struct PackInput : WalkTables { // device copies of the input, the image + the pack's buffers, released on every way out
        DevBuf seq, ts, op_off, ops, keep;
        PackCore c;
        ~PackInput() { release_all({&seq, &ts, &op_off, &ops, &keep}); c.release(); }
    } k;
    hipStream_t s = nullptr;
    upload(k.seq, seq, n_reads * 4);
    upload(k.ts, text_start, n_reads * 8);
    upload(k.op_off, op_offsets, n_reads ? (n_reads + 1) * 8 : 0);
    upload(k.ops, ops, n_ops * 4);
    if (keep) upload(k.keep, keep, n_reads);
    PackCore &c = k.c;
    c.walk = k.build(seq_offsets, n_seq, marks, visit_nodes, s);
    c.seq_start = k.seq_off.as<uint64_t>();
    c.n_seq = n_seq;
    c.endmark = 0u;
    c.build(who, s);
    *n_nodes = c.n_nodes;
    *n_bases = c.G;
    if (c.n_nodes > nodes_cap || c.G > cov_cap)
        throw Error(PGX_ERR_NOMEM, who + ": the table holds " + std::to_string(c.n_nodes) + " nodes and " + std::to_string(c.G) + " graph bases, nodes_cap is " + std::to_string(nodes_cap) +
                                       " and cov_cap " + std::to_string(cov_cap));
    c.add(nullptr, k.seq.as<uint32_t>(), k.ts.as<uint64_t>(), k.op_off.as<uint64_t>(), k.ops.as<uint32_t>(), nullptr, keep ? k.keep.as<uint8_t>() : nullptr, 0u, n_reads, s);
    c.fold(s);
    const uint64_t nn = c.n_nodes;
    HIPCHECK(hipMemcpyAsync(node_base, c.node_base.p, (nn + 1) * 8, hipMemcpyDeviceToHost, s));
    if (nn) {
        HIPCHECK(hipMemcpyAsync(node_length, c.node_len.p, nn * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(covered, c.covered.p, nn * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(sum, c.sum.p, nn * 8, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(max, c.max.p, nn * 4, hipMemcpyDeviceToHost, s));
    }
    if (c.G) HIPCHECK(hipMemcpyAsync(cov, c.cov.p, c.G * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(counters, c.ctr.p, 24, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return PGX_OK;
    PGX_GUARD_END
}
