"""GPU tier of pgx_batch_read_mapq: the batch route through built indexes whose tags describe paths (pgx_build_tags_paths) -- the variation graph of
tests/walk_cases.py with the reads of tests/mapq_cases.py, its near_copy collection, and the pairs of mates_cases and rescue_cases on their
collections cut into nodes (mapq_cases.chunk_tables): run(12, 1), locate(0), read_place(PLACE_LIST), read_verify(16, 4, VERIFY_LIST), then
read_rescue(MERGE) and read_mates(ELECT) where pairs are, then read_mapq.

Against the emulator: the records and the four counters equal tests/mapq_emu.py fed with the downloaded place list, verify list, winners, rescue
records and Index.paths(); the device form holds the bytes of the host form; a second call gives the same bytes; the verify, mates and rescue results
are untouched.  Without the emulator: the statements of tests/test_mapq_cpu.py hold on the device's own lists (the walk reads are one place, the
second diagonal of an indel competes only without slack, the near copy is seen through the extras, a repeat mate has mapq 3 alone and 20 with its
mate, the rescued mates carry the rescue terms).  A later read_verify makes mapqs() PGX_ERR_ARG; every refusal leaves everything as it was;
PGX_MAPQ_LANES 1, 16 and 64 give the same bytes; a batch refilled twice equals fresh batches; a timed run fills ms_mapq."""
import os

import numpy as np
import pytest

import mapq_cases as QC
import mapq_emu as Q
import mates_cases as MC
import mates_emu as M
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import rescue_cases as RC
import test_mapq_cpu as T
import walk_cases as WC
from test_gpu_hits import _device_read
from test_gpu_mem_locate import _run_batch

pytestmark = pytest.mark.gpu
MIN_LEN, MAX_CAND, PENALTY, U = T.MIN_LEN, T.MAX_CAND, T.PENALTY, T.U
COUNTERS = ("n_has", "n_unique", "n_capped", "sum_mapq")


def _index(workdir, name, raw, tables, node_length):
    text = os.path.join(workdir, name + ".txt")
    with open(text, "wb") as f:
        f.write(raw)
    ri = W.build_index_from_text(text, workdir, name, with_tags=False)[0]
    tags = os.path.join(workdir, name + ".graph.tags")
    P.build_tags_paths(ri, tables[0], tables[1], node_length, 1, tags, flags=P.BUILD_TAGS_OUT_COMPACT)
    return P.Index(ri, tags, mode=P.MODE_STRICT)


def _verified_batch(idx, reads, flags=P.RUN_TAGS):
    cat, offs = O.pack_reads(reads)
    b, _ = _run_batch(idx, cat, offs, MIN_LEN, 1, flags)
    b.locate(0)
    b.read_place(P.PLACE_LIST)
    b.read_verify(MAX_CAND, PENALTY, P.VERIFY_LIST)
    return b


def _expected(b, tables, seqs, reads, max_extra, rescue=None, paired=None, **kw):
    """the emulator fed with what the batch holds"""
    v = b.verified()
    offs, ent, list_len, more = Q.candidates_with_extras(seqs, reads, b.places() if max_extra else None, v, max_extra, PENALTY)
    return Q.read_mapq(*tables, offs, ent, Q.chosen_of(v["reads"]), list_len=list_len, rescue=rescue, paired=paired, max_cand=MAX_CAND, more=more if max_extra else None, **kw)


def _same(got, exp, what=""):
    bad = np.flatnonzero(got["records"] != exp["records"])
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got["records"][bad[0]], exp["records"][bad[0]])
    assert got["records"].tobytes() == exp["records"].tobytes()
    assert {k: got[k] for k in COUNTERS} == {k: exp[k] for k in COUNTERS}, what


@pytest.fixture(scope="module")
def graph(workdir):
    g = WC.graph()
    truth, reads = WC.cut_reads(g)
    allr = reads + QC.indel_mid(g)[1] + QC.none_reads()
    tables = QC.graph_tables(g)
    idx = _index(workdir, "gpu_mapq_graph", b"".join(t + b"\n" for t in g["texts"]), tables, g["node_length"])
    b = _verified_batch(idx, allr)
    c = dict(g=g, idx=idx, b=b, tables=tables, seqs=g["texts"], reads=allr, walk=range(0, WC.N_READS), indel=range(WC.N_READS, WC.N_READS + QC.N_INDEL),
             none=range(WC.N_READS + QC.N_INDEL, len(allr)))
    yield c
    b.free()
    idx.close()


@pytest.fixture(scope="module")
def pairs(workdir):
    """the pairs of mates_cases and of rescue_cases: verified, rescued with MERGE, elected"""
    out = {}
    for name, C in (("mates", MC.CASES), ("rescue", RC.CASES)):
        po, pn, vl, nl = QC.chunk_tables(C.lens)
        idx = _index(workdir, "gpu_mapq_" + name, C.raw, (po, pn, vl), nl)
        out[name] = dict(C=C, idx=idx, tables=(po, pn, vl))
    yield out
    for c in out.values():
        c["idx"].close()


def test_records_counters_and_forms_equal_the_emulator(graph):
    c, b = graph, graph["b"]
    tables = c["idx"].paths()
    assert all(np.array_equal(x, y) for x, y in zip(tables, c["tables"]))
    before, places = b.verified(), b.places()
    for scale, slack, max_extra in ((2, 8, 0), (2, 8, 16), (2, 0, 16), (16, 1024, 63), (1, 3, 1)):
        exp = _expected(b, tables, c["seqs"], c["reads"], max_extra, scale=scale, slack=slack)
        got = b.read_mapq(scale, slack, max_extra)
        _same(got, exp, (scale, slack, max_extra))
        assert (got["n_reads"], got["scale"], got["slack"], got["max_extra"], got["flags"], got["ms_mapq"]) == (len(c["reads"]), scale, slack, max_extra, 0, 0)
        assert (got["n_extras"] > 0) == (max_extra > 0)
        dev = b.device_mapqs()
        assert dev["device"] and {k: dev[k] for k in got if k != "records"} == {k: got[k] for k in got if k != "records"}
        assert _device_read(dev["records"].__cuda_array_interface__["data"][0], len(c["reads"]) * 32).tobytes() == exp["records"].tobytes()
        assert dev["records"].__cuda_array_interface__["shape"] == (len(c["reads"]), 4)
        assert b.read_mapq(scale, slack, max_extra)["records"].tobytes() == got["records"].tobytes()  # a second call: the same bytes
    after = b.verified()  # the verify and the place results are untouched
    assert all(after[k].tobytes() == before[k].tobytes() for k in ("reads", "cand_offsets", "cands"))
    assert all(b.places()[k].tobytes() == places[k].tobytes() for k in ("reads", "place_offsets", "places"))
    b.locate(P.LOCATE_UNIQUE)  # a later locate leaves the result valid
    assert b.mapqs()["records"].tobytes() == got["records"].tobytes()
    b.locate(0)


def test_the_statements_of_the_cpu_tier_hold_on_the_devices_own_lists(graph, workdir):
    c, b = graph, graph["b"]
    v = b.verified()
    tied = T.check_walk(c, b.read_mapq(2, 8, 0), v)
    assert tied >= 150
    T.check_indel(c, b.read_mapq(2, 0, 16), b.read_mapq(2, 8, 16))
    N = QC.NEAR
    idx = _index(workdir, "gpu_mapq_near", N.raw, N.tables, N.node_length)
    nb = _verified_batch(idx, N.reads)
    for scale in (2, 4, 12):
        T.check_near(nb.read_mapq(scale, 8, 0)["records"], nb.read_mapq(scale, 8, 16)["records"], scale)
    _same(nb.read_mapq(2, 8, 16), _expected(nb, N.tables, N.seqs, N.reads, 16))
    nb.free()
    idx.close()


def _paired_chain(c, reads, rescue=True):
    """verify, rescue with MERGE, mates with ELECT on a fresh batch: (batch, rescue records or None)"""
    b = _verified_batch(c["idx"], reads)
    resc = b.read_rescue(0, 500, MIN_LEN, 2, P.RESCUE_MERGE)["reads"] if rescue else None
    b.read_mates(0, 500, U, P.MATES_ELECT)
    return b, resc


def test_pairs_equal_the_emulator_and_leave_the_other_results_untouched(pairs):
    for name, c in pairs.items():
        C = c["C"]
        b, resc = _paired_chain(c, C.reads)
        v, mated, rescued = b.verified(), b.mated(), b.rescued()
        paired = dict(seq_lengths=C.lens, frag_min=0, frag_max=500, penalty=U)
        for flags, max_extra in ((P.MAPQ_PAIRED, 0), (P.MAPQ_PAIRED, 16), (0, 16)):
            exp = _expected(b, c["tables"], C.seqs, C.reads, max_extra, rescue=resc, paired=paired if flags else None)
            got = b.read_mapq(2, 8, max_extra, flags)
            _same(got, exp, (name, flags, max_extra))
            assert got["flags"] == flags
            if flags and not max_extra:  # the chosen entry has the largest paired score of its list
                assert not (got["records"]["flags"] & Q.OUTSCORED).any()
        assert b.verified()["reads"].tobytes() == v["reads"].tobytes() and b.verified()["cands"].tobytes() == v["cands"].tobytes()
        assert b.mated()["pairs"].tobytes() == mated["pairs"].tobytes() and b.rescued()["reads"].tobytes() == rescued["reads"].tobytes()
        kept = b.read_mapq(2, 8, 0, P.MAPQ_PAIRED)
        with pytest.raises(P.PgxError) as e:  # a merged list takes no further rescue call, with or without MERGE: the rescue records stay those of the merge
            b.read_rescue(0, 500, MIN_LEN, 2, 0)
        assert e.value.code == P.ERR_ARG and "already merged" in str(e.value)
        assert b.rescued()["reads"].tobytes() == rescued["reads"].tobytes() and b.mapqs()["records"].tobytes() == kept["records"].tobytes()
        assert b.read_mapq(2, 8, 0, P.MAPQ_PAIRED)["records"].tobytes() == kept["records"].tobytes()
        if name == "rescue":
            n = T.check_rescued(dict(verified=v, winners=v["reads"]), b.read_mapq(2, 8, 0)["records"], resc)
            assert n >= 44
        b.free()


def test_a_repeat_mate_is_a_tie_alone_and_twenty_with_its_mate(pairs):
    c = pairs["mates"]
    C = c["C"]
    b = _verified_batch(c["idx"], C.reads)
    solo = b.read_mapq(2, 8, 0)["records"]
    b.read_mates(MC.FRAG_MIN, MC.FRAG_MAX, U, P.MATES_ELECT)
    with pytest.raises(P.PgxError):  # the mates call made the result invalid
        b.mapqs()
    elected = b.read_mapq(2, 8, 0, P.MAPQ_PAIRED)["records"]
    T.check_repeat_mates(solo, elected)
    b.free()


def test_lanes_timing_and_a_refilled_batch(graph, pairs, monkeypatch):
    c, b = graph, graph["b"]
    want = b.read_mapq(2, 8, 16)
    for lanes in ("1", "16", "64"):
        monkeypatch.setenv("PGX_MAPQ_LANES", lanes)
        assert b.read_mapq(2, 8, 16)["records"].tobytes() == want["records"].tobytes(), lanes
    p = pairs["mates"]
    pb, _ = _paired_chain(p, p["C"].reads, rescue=False)
    monkeypatch.delenv("PGX_MAPQ_LANES")
    pwant = pb.read_mapq(2, 8, 16, P.MAPQ_PAIRED)
    for lanes in ("1", "32", "64"):
        monkeypatch.setenv("PGX_MAPQ_LANES", lanes)
        got = pb.read_mapq(2, 8, 16, P.MAPQ_PAIRED)
        assert got["records"].tobytes() == pwant["records"].tobytes() and {k: got[k] for k in COUNTERS} == {k: pwant[k] for k in COUNTERS}, lanes
    monkeypatch.delenv("PGX_MAPQ_LANES")
    pb.free()
    # a timed run fills ms_mapq
    tb = _verified_batch(c["idx"], c["reads"], P.RUN_TAGS | P.RUN_TIMING)
    timed = tb.read_mapq(2, 8, 16)
    assert 0 < timed["ms_mapq"] < 1000 and tb.device_mapqs()["ms_mapq"] == timed["ms_mapq"] and timed["records"].tobytes() == want["records"].tobytes()
    tb.free()
    # a batch refilled twice equals fresh batches
    sets = [c["reads"][:50], c["reads"][150:246], c["reads"][40:47]]
    cat, offs = O.pack_reads(sets[0])
    rb = P.Batch(c["idx"], cat, offs)
    for k, reads in enumerate(sets):
        if k:
            cat, offs = O.pack_reads(reads)
            rb.upload(cat, offs)
        rb.run(MIN_LEN, 1, P.RUN_TAGS)
        rb.locate(0)
        rb.read_place(P.PLACE_LIST)
        rb.read_verify(MAX_CAND, PENALTY, P.VERIFY_LIST)
        got = rb.read_mapq(2, 8, 16)
        fresh = _verified_batch(c["idx"], reads)
        fwant = fresh.read_mapq(2, 8, 16)
        assert got["records"].tobytes() == fwant["records"].tobytes() and {x: got[x] for x in got if x != "records"} == {x: fwant[x] for x in fwant if x != "records"}, k
        fresh.free()
    rb.free()


def test_refusals_leave_everything_as_it_was(graph, pairs, workdir):
    c, b = graph, graph["b"]
    first = b.read_mapq(2, 8, 16)
    v = b.verified()

    def refused(call, code=P.ERR_ARG):
        with pytest.raises(P.PgxError) as e:
            call()
        assert e.value.code == code, str(e.value)
        return str(e.value)

    assert "unknown flag" in refused(lambda: b.read_mapq(2, 8, 16, 1))
    assert "scale 0 is outside 1 .. 16" in refused(lambda: b.read_mapq(0, 8, 16))
    assert "scale 17 is outside 1 .. 16" in refused(lambda: b.read_mapq(17, 8, 16))
    assert "slack 1025 exceeds 1024" in refused(lambda: b.read_mapq(2, 1025, 16))
    assert "max_extra 64 exceeds 63" in refused(lambda: b.read_mapq(2, 8, 64))
    assert "no mates result" in refused(lambda: b.read_mapq(2, 8, 16, P.MAPQ_PAIRED))
    assert b.mapqs()["records"].tobytes() == first["records"].tobytes() and b.verified()["reads"].tobytes() == v["reads"].tobytes()
    cat, offs = O.pack_reads(c["reads"][:11])
    nb = P.Batch(c["idx"], cat, offs)
    assert "not been run" in refused(lambda: nb.read_mapq())
    nb.run(MIN_LEN, 1, P.RUN_TAGS)
    assert "no verify result" in refused(lambda: nb.read_mapq())
    refused(nb.mapqs)
    refused(nb.device_mapqs)
    nb.locate(0)
    nb.read_place(0)
    nb.read_verify(1, PENALTY)
    assert "PGX_VERIFY_LIST" in refused(lambda: nb.read_mapq())  # a verify result without the list
    nb.read_verify(1, PENALTY, P.VERIFY_LIST)
    assert "PGX_PLACE_LIST" in refused(lambda: nb.read_mapq(2, 8, 16))  # extras without the place list
    ok = nb.read_mapq(2, 8, 0)
    assert ok["n_has"] == ok["n_capped"] == 11 and (ok["records"]["flags"] & Q.CAPPED).all()  # max_cand 1: every list is full
    nb.read_place(P.PLACE_LIST)
    nb.read_verify(MAX_CAND, PENALTY, P.VERIFY_LIST)
    assert "no mapq result" in refused(nb.mapqs)  # a later read_verify makes the result invalid
    assert nb.read_mapq(2, 8, 16)["records"].tobytes() == first["records"][:11].tobytes()
    nb.run(MIN_LEN, 1, P.RUN_TAGS)  # a stale run
    assert "no verify result" in refused(lambda: nb.read_mapq())
    refused(nb.mapqs)
    nb.free()
    # PAIRED needs a mates result made on the current verify result
    p = pairs["mates"]
    pb, _ = _paired_chain(p, p["C"].reads[:20], rescue=False)
    good = pb.read_mapq(2, 8, 0, P.MAPQ_PAIRED)
    pb.read_verify(MAX_CAND, PENALTY, P.VERIFY_LIST)
    assert "made on the current verify result" in refused(lambda: pb.read_mapq(2, 8, 0, P.MAPQ_PAIRED))
    pb.read_mates(0, 500, U, P.MATES_ELECT)
    assert pb.read_mapq(2, 8, 0, P.MAPQ_PAIRED)["records"].tobytes() == good["records"].tobytes()
    pb.free()
    # an index whose tags describe no graph of this collection, and one without tags
    text = os.path.join(workdir, "gpu_mapq_graph.txt")
    ri = W.build_index_from_text(text, workdir, "gpu_mapq_notags", with_tags=False)[0]
    bare = P.Index(ri, mode=P.MODE_STRICT)
    cat, offs = O.pack_reads(c["reads"][:8])
    bb = P.Batch(bare, cat, offs)
    bb.run(MIN_LEN, 1, 0)
    bb.locate(0)
    bb.read_place(P.PLACE_LIST)
    bb.read_verify(MAX_CAND, PENALTY, P.VERIFY_LIST)
    with pytest.raises(P.PgxError) as e:
        bb.read_mapq()
    assert e.value.code in (P.ERR_ARG, P.ERR_UNSUPPORTED) and "tag" in str(e.value)
    refused(bb.mapqs)
    bb.free()
    bare.close()
