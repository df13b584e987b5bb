"""GPU tier of pgx_pack on the batch route, on the variation graph of tests/walk_cases.py (136 nodes, 3125 graph bases, 8 haplotypes in both
orientations; tags by pgx_build_tags_paths) with its 200 error-free reads of 60 bases: run, locate, read_place, read_verify, read_align(ALIGN_CIGAR),
then Pack.add and Pack.finish.

Against the emulator: the node table, the vector, the summary and the counters equal tests/pack_emu.py fed with Index.paths() and the batch's own
align records, byte for byte; the device form holds the bytes of the host form.  Without the emulator: the reads' truth (sequence, offset) and the
graph's node table give the expected vector directly, whichever haplotype verify chose -- the reads that walk_cases.ambiguous flags are left out
of the batch, at most MAX_LEFT_OUT = 10 (the function flags 0 of the 200) -- and sum(cov) is the sum of n_match + n_mismatch over the counted
reads.  The reads with base 30 deleted leave a hole: 59 a read.  Finishing twice gives the same arrays; one batch of 200 equals four batches of 50
added from two threads; adding after finish accumulates; min_mapq 1 and 60 equal the emulator on the mapq records of mapq_cases' reads; under
MATES_ELECT the repeat mates of mates_cases cover their truth copy and not the other; an index reopened from its .pgi gives the same vector;
the handles it refuses."""
import os
import threading

import numpy as np
import pytest

import mapq_cases as QC
import mates_cases as MC
import oracle_ffi as O
import pack_emu as E
import pgx_ffi as P
import pgx_workload as W
import walk_cases as C
from test_gpu_hits import _device_read
from test_gpu_mem_locate import _run_batch

pytestmark = pytest.mark.gpu
MAX_LEFT_OUT = 10
MIN_LEN = 12


def _index_files(workdir, name, raw, tables, node_length):
    text = os.path.join(workdir, name + ".txt")
    with open(text, "wb") as f:
        f.write(raw)
    ri = W.build_index_from_text(text, workdir, name, with_tags=False)[0]
    tags = os.path.join(workdir, name + ".graph.tags")
    P.build_tags_paths(ri, tables[0], tables[1], node_length, 1, tags, flags=P.BUILD_TAGS_OUT_COMPACT)
    return ri, tags


@pytest.fixture(scope="module")
def world(workdir):
    g = C.graph()
    ri, tags = _index_files(workdir, "pack_graph", b"".join(t + b"\n" for t in g["texts"]), (g["path_offsets"], g["path_nodes"]), g["node_length"])
    truth, reads = C.cut_reads(g)
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    w = dict(g=g, ri=ri, tags=tags, truth=truth, reads=reads, idx=idx, tables=idx.paths())
    yield w
    idx.close()


def _aligned(idx, reads, lists=False, flags=P.RUN_TAGS):
    """(batch, its align result) behind run, locate, place, verify and align with the CIGAR list; lists: place and verify with their lists (what mapq reads)"""
    cat, offs = O.pack_reads(reads)
    b, _ = _run_batch(idx, cat, offs, MIN_LEN, 1, flags)
    b.locate(0)
    b.read_place(P.PLACE_LIST if lists else 0)
    b.read_verify(16 if lists else 1, 4, P.VERIFY_LIST if lists else 0)
    return b, b.read_align(8, P.ALIGN_CIGAR)


def _emu(tables, a, **kw):
    r = a["reads"]
    return E.read_pack(tables[0], tables[1], tables[2], r["seq"], r["text_start"], a["op_offsets"], a["ops"], text_end=r["text_end"], **kw)


def _packed(idx, batches, min_mapq=0):
    p = P.Pack(idx)
    for b in batches:
        p.add(b, min_mapq)
    out = p.finish()
    p.close()
    return out


def test_the_result_equals_the_emulator_on_the_batchs_own_align_records(world):
    w = world
    b, a = _aligned(w["idx"], w["reads"] + [b"ACGT" * 10, b"T", b""])
    exp = _emu(w["tables"], a)
    p = P.Pack(w["idx"])
    before = b.aligned()
    p.add(b)
    got = p.finish()
    E.same(got, exp)
    assert (got["n_nodes"], got["n_bases"]) == (len(w["g"]["node_length"]) + 1, int(w["g"]["node_length"].sum())) == (137, 3125)
    assert got["node_length"][1:].tolist() == w["g"]["node_length"].tolist() and got["reads_counted"] >= 200 and got["reads_filtered"] == 0
    assert got["n_text"] == sum(len(t) + 1 for t in w["g"]["texts"]) and got["ms_add_total"] == 0 and got["ms_fold"] > 0 and got["n_projected"] > 0
    after = b.aligned()  # the batch is untouched
    assert all(after[k].tobytes() == before[k].tobytes() for k in ("reads", "op_offsets", "ops"))
    again = p.finish()  # finishing twice: the same arrays, nothing projected the second time
    E.same(again, exp)
    assert again["n_projected"] == got["n_projected"]
    dev = p.device_result()
    assert dev["device"] and (dev["n_nodes"], dev["n_bases"]) == (got["n_nodes"], got["n_bases"])
    for k, nbytes in (("node_base", 8 * 138), ("node_length", 4 * 137), ("cov", 4 * 3125), ("covered", 4 * 137), ("sum", 8 * 137), ("max", 4 * 137)):
        assert _device_read(dev[k].__cuda_array_interface__["data"][0], nbytes).tobytes() == got[k].tobytes(), k
    p.add(b)  # adding after finish accumulates
    twice = p.finish()
    assert twice["cov"].tolist() == (2 * got["cov"]).tolist() and twice["reads_counted"] == 2 * got["reads_counted"] and twice["bases_added"] == 2 * got["bases_added"]
    assert twice["covered"].tolist() == got["covered"].tolist() and twice["sum"].tolist() == (2 * got["sum"]).tolist() and twice["max"].tolist() == (2 * got["max"]).tolist()
    p.close()
    b.free()


def _truth_vector(g, truth, keep):
    """the expected vector from the reads' truth and the graph's node table alone: node ids from 1, base = the lengths before"""
    base = np.concatenate(([0, 0], np.cumsum(g["node_length"]))).astype(np.int64)  # base[id], id 0 has no bases
    cov = np.zeros(int(g["node_length"].sum()), dtype=np.uint32)
    under = {}
    for r in keep:
        q, o = truth[r]
        if q not in under:
            at = []
            for v in g["paths"][q]:
                ln = int(g["node_length"][(v >> 1) - 1])
                at += [int(base[v >> 1]) + (ln - 1 - d if v & 1 else d) for d in range(ln)]
            under[q] = at
        for p in range(o, o + C.READ_LEN):
            cov[under[q][p]] += 1
    return cov


def test_error_free_reads_cover_their_source_whichever_haplotype_verify_chose(world):
    w = world
    keep = np.flatnonzero(~C.ambiguous(w["g"], w["truth"], w["reads"]))
    assert len(keep) >= C.N_READS - MAX_LEFT_OUT
    b, a = _aligned(w["idx"], [w["reads"][r] for r in keep])
    got = _packed(w["idx"], [b])
    assert got["cov"].tolist() == _truth_vector(w["g"], w["truth"], keep).tolist()
    assert (a["reads"]["seq"] != np.array([w["truth"][r][0] for r in keep])).any()  # (another haplotype that agrees over the read: the same graph bases)
    assert got["reads_counted"] == len(keep) and int(got["cov"].astype(np.uint64).sum()) == int((a["reads"]["n_match"] + a["reads"]["n_mismatch"]).sum()) == 60 * len(keep)
    assert int(got["sum"].sum()) == got["bases_added"] == 60 * len(keep)
    b.free()


def test_a_deleted_base_leaves_a_hole(world):
    w = world
    b, a = _aligned(w["idx"], C.deleted(w["reads"]))
    got = _packed(w["idx"], [b])
    E.same(got, _emu(w["tables"], a))
    one = np.flatnonzero((a["reads"]["n_del"] == 1) & (a["reads"]["edits"] == 1))
    assert len(one) >= C.N_READS // 2
    only = P.Batch(w["idx"], *O.pack_reads([C.deleted(w["reads"])[r] for r in one]))
    only.run(MIN_LEN, 1, P.RUN_TAGS)
    only.locate(0); only.read_place(0); only.read_verify(1, 4); only.read_align(8, P.ALIGN_CIGAR)
    holes = _packed(w["idx"], [only])
    assert holes["reads_counted"] == len(one) and holes["bases_added"] == 59 * len(one) == int(holes["cov"].astype(np.uint64).sum())
    only.free()
    b.free()


def test_one_batch_equals_four_batches_from_two_threads(world):
    w = world
    whole, _ = _aligned(w["idx"], w["reads"])
    want = _packed(w["idx"], [whole])
    parts = [_aligned(w["idx"], w["reads"][k:k + 50])[0] for k in range(0, 200, 50)]
    p = P.Pack(w["idx"])
    errors = []

    def work(mine):
        try:
            for b in mine:
                p.add(b)
        except Exception as e:  # noqa: BLE001 (shown below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(parts[k::2],)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    got = p.finish()
    E.same(got, want)
    p.close()
    for b in parts + [whole]:
        b.free()


def test_min_mapq_equals_the_emulator_on_the_mapq_records(world):
    w = world
    reads = w["reads"][:60] + QC.indel_mid(w["g"])[1] + QC.none_reads()
    b, a = _aligned(w["idx"], reads, lists=True)
    q = b.read_mapq(2, 0, 16)["records"]["mapq"]  # (without slack the second diagonal of an indel competes: qualities below 60)
    assert (q == 60).any() and (q < 60).any()
    plain = _packed(w["idx"], [b])
    E.same(plain, _emu(w["tables"], a))
    for min_mapq in (1, 60):
        got = _packed(w["idx"], [b], min_mapq)
        E.same(got, _emu(w["tables"], a, mapq=q, min_mapq=min_mapq))
    assert 0 < got["reads_filtered"] and got["reads_counted"] + got["reads_filtered"] == plain["reads_counted"]
    b.free()


def test_elected_repeat_mates_cover_their_truth_copy_and_not_the_other(workdir):
    M = MC.CASES
    po, pn, vl, nl = QC.chunk_tables(M.lens)
    ri, tags = _index_files(workdir, "pack_mates", M.raw, (po, pn), nl)
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    second = [k for k, pr in enumerate(M.pairs) if pr["which"] == 1]
    assert len(second) == 24
    reads, seq, start = [], [], []
    for k in second:
        pr = M.pairs[k]
        reads += [pr["a"], pr["b"]]
        seq += [pr["truth_a"][0], pr["truth_b"][0]]
        start += [pr["truth_a"][1], pr["truth_b"][1]]
    n = len(reads)
    want = E.read_pack(po, pn, vl, seq, start, np.arange(n + 1, dtype=np.uint64), np.full(n, (MC.READ_LEN << 4) | E.OP_EQ, np.uint32))
    b, a = _aligned(idx, reads, lists=True)
    solo = _packed(idx, [b])
    assert solo["cov"].tolist() != want["cov"].tolist()  # alone, the mate inside the repeat lies on the first copy
    b.read_mates(MC.FRAG_MIN, MC.FRAG_MAX, 10, P.MATES_ELECT)
    a = b.read_align(8, P.ALIGN_CIGAR)
    assert (a["reads"]["edits"] == 0).all()
    elected = _packed(idx, [b])
    assert elected["cov"].tolist() == want["cov"].tolist() and elected["reads_counted"] == n
    b.free()
    idx.close()


def test_a_reopened_image_gives_the_same_vector(world, workdir):
    w = world
    b, _ = _aligned(w["idx"], w["reads"][:80])
    want = _packed(w["idx"], [b])
    b.free()
    path = os.path.join(workdir, "pack_graph.pgi")
    w["idx"].save_image(path)
    again = P.Index.open_image(path)
    b2, _ = _aligned(again, w["reads"][:80])
    E.same(_packed(again, [b2]), want)
    b2.free()
    again.close()


def test_refused_handles_add_nothing(world):
    w = world
    idx = w["idx"]
    cat, offs = O.pack_reads(w["reads"][:40])
    p = P.Pack(idx)
    empty = p.finish()
    assert not empty["cov"].any() and empty["reads_counted"] == 0

    def refused(call, code=P.ERR_ARG):
        with pytest.raises(P.PgxError) as e:
            call()
        assert e.value.code == code, str(e.value)
        return str(e.value)

    assert "null batch" in refused(lambda: p.add(None))
    b = P.Batch(idx, cat, offs)
    assert "not been run" in refused(lambda: p.add(b))
    b.run(MIN_LEN, 1, P.RUN_TAGS)
    assert "no align result" in refused(lambda: p.add(b))
    b.locate(0); b.read_place(0); b.read_verify(1, 4)
    b.read_align(8, 0)
    assert "ran with flags 0" in refused(lambda: p.add(b))
    b.read_align(8, P.ALIGN_CIGAR)
    assert "unknown flag" in refused(lambda: p.add(b, 0, 1))
    assert "min_mapq 61 exceeds 60" in refused(lambda: p.add(b, 61))
    assert "no mapq result" in refused(lambda: p.add(b, 1))
    other = P.Index(w["ri"], w["tags"], mode=P.MODE_STRICT)
    po = P.Pack(other)
    assert "another index" in refused(lambda: po.add(b))
    po.close()
    other.close()
    L = P.lib()
    assert L.pgx_pack_add(None, b.b, 0, 0, None) == P.ERR_ARG
    after = p.finish()  # nothing was added by any of them
    assert not after["cov"].any() and (after["reads_counted"], after["reads_filtered"], after["bases_added"]) == (0, 0, 0)
    p.add(b)
    assert p.finish()["reads_counted"] == 40
    b.run(MIN_LEN, 1, P.RUN_TAGS)  # a re-run: the align result belonged to the run before
    refused(lambda: p.add(b))
    p.close()
    b.free()
    bare = P.Index(w["ri"], mode=P.MODE_STRICT)  # no tags: the WALK image's refusal is the pack's
    assert "without a tag array" in refused(lambda: P.Pack(bare), P.ERR_UNSUPPORTED)
    bare.close()


def test_a_timed_run_fills_ms_add_total(world):
    w = world
    b, _ = _aligned(w["idx"], w["reads"][:50], flags=P.RUN_TAGS | P.RUN_TIMING)
    p = P.Pack(w["idx"])
    p.add(b)
    p.add(b)
    out = p.finish()
    assert out["ms_add_total"] > 0 and out["ms_table"] > 0 and out["reads_counted"] == 100
    p.close()
    b.free()
