"""GPU tier of pgx_batch_read_place: the placements of a batch equal tests/place_emu.py fed with the batch's MEMs and with the packed
positions of pgx_locate_batch(flags = 0) on every MEM's range -- never from pgx_batch_locate -- on the collections of
tests/test_gpu_hits.py (64, 66 and 130 sequences) and on the golden xy index in both modes; with a cap that leaves MEMs unlocated, on
the resident path and on the sample chains, as host and as device arrays, across a later locate; error-free reads cut from known places
of the text are found there without the emulator; the placements never beat the hits of the same run; and the calls it refuses."""
import os

import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import place_emu as E
from test_gpu_hits import _device_read
from test_gpu_mem_locate import _ranges, _run_batch
from test_gpu_mem_locate_sets import _collection

pytestmark = pytest.mark.gpu

SETS, UNIQ_IDS = P.LOCATE_SEQ_SETS, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE
KEYS = ("reads", "place_offsets", "places")


def _same(a, b):
    assert a["reads"].tobytes() == b["reads"].tobytes()
    for k in KEYS[1:]:
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or a[k].tobytes() == b[k].tobytes()), k


def _check_places(idx, b, res, max_occ=0):
    """locate(0, max_occ) + read_place == the emulator on values from pgx_locate_batch; the chains give the same bytes; the device arrays
    hold the same bytes; the places outlive a locate of every other form.  Returns the emulator's result."""
    info = idx.info()
    first, last, _ = _ranges(res["mems"], info.bwt_size, max_occ)
    off, vals = idx.locate_batch(first, last, 0)
    n = len(res["mem_offsets"]) - 1
    exp = E.read_place(res["mem_offsets"], res["mems"], off, vals, int(info.max_length))
    b.locate(0, max_occ)
    got = b.read_place(P.PLACE_LIST)
    assert (got["n_reads"], got["n_anchors"], got["n_places"], got["flags"]) == (n, len(vals), len(exp["places"]), P.PLACE_LIST)
    bad = np.flatnonzero(got["reads"] != exp["reads"])
    assert len(bad) == 0, (len(bad), int(bad[0]), got["reads"][bad[0]], exp["reads"][bad[0]])
    _same(got, exp)
    plain = b.read_place(0)
    assert plain["reads"].tobytes() == exp["reads"].tobytes() and plain["places"] is None and plain["place_offsets"] is None and plain["flags"] == 0
    b.locate(P.LOCATE_CHAINS, max_occ)
    _same(b.read_place(P.PLACE_LIST), exp)
    dev = b.device_places()
    assert dev["device"] and (dev["n_reads"], dev["n_places"], dev["flags"]) == (n, len(exp["places"]), P.PLACE_LIST)
    for k, nbytes in (("reads", n * 64), ("place_offsets", (n + 1) * 8), ("places", len(exp["places"]) * 24)):
        if nbytes:
            assert _device_read(dev[k].__cuda_array_interface__["data"][0], nbytes).tobytes() == exp[k].tobytes(), k
    assert dev["reads"].__cuda_array_interface__["shape"] == (n, 8) and dev["places"].__cuda_array_interface__["shape"] == (len(exp["places"]), 3)
    for flags in (SETS, UNIQ_IDS, P.LOCATE_SEQ_IDS, P.LOCATE_UNIQUE):  # places first, any other locate afterwards
        b.locate(flags)
        _same(b.places(), exp)
    return exp


@pytest.mark.parametrize("n_hap", [32, 33, 65])
def test_places_on_the_hits_collections(workdir, n_hap):
    ri, tags, seqs, n_seq = _collection(workdir, "hits_border_%d" % n_hap, n_hap, 2000, 100 + n_hap)
    cat, offs = W.sample_reads(seqs, 150, 150, seed=n_hap)
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 12, 1)
    exp = _check_places(idx, b, res)
    h = exp["reads"]
    assert (h["best_score"] > 0).any() and (h["n_placements"] > 1).any() and (h["n_best"] > 1).any()
    # a cap that leaves some MEMs unlocated, chosen as in test_hits_on_word_borders
    sizes = res["mems"]["size"].astype(np.int64)
    distinct = np.unique(sizes[sizes > 0])
    assert len(distinct) >= 2
    cap = int(distinct[(len(distinct) - 1) // 2])  # at least one MEM on either side
    capped = _check_places(idx, b, res, max_occ=cap)["reads"]
    assert (capped["n_located"] < capped["n_mems"]).any() and (capped["n_anchors"] <= h["n_anchors"]).all()
    assert np.array_equal(capped["n_mems"], h["n_mems"])
    b.free()
    idx.close()


def test_places_on_xy_in_both_modes(golden):
    bt = os.path.join(golden, "bidirectional_test")
    reads = [l for l in open(os.path.join(bt, "reads.txt"), "rb").read().split(b"\n") if l]
    cat, offs = O.pack_reads(reads)
    ran = 0
    for mode in (P.MODE_COMPAT, P.MODE_STRICT):
        idx = P.Index(os.path.join(bt, "xy.ri"), os.path.join(bt, "xy_bidirectional_compressed.tags"), mode=mode)
        info = idx.info()
        if mode == P.MODE_COMPAT and info.is_encoded and not info.has_N:
            idx.close()
            continue  # (locate is not supported there, as in tests/test_gpu_hits.py)
        for min_len in (3, 5):
            b, res = _run_batch(idx, cat, offs, min_len, 1)
            exp = _check_places(idx, b, res)
            assert (exp["reads"]["best_score"] > 0).any()
            b.free()
            ran += 1
        idx.close()
    assert ran >= 2


def test_error_free_reads_lie_where_they_were_cut(workdir):
    """a read that is a substring of the text has the first MEM (0, 60) (step 1 of find_mems_function cannot fail on it, step 2 runs to
    the end), so its best placement covers all 60 positions and the place it was cut from is among the placements of score 60"""
    n_hap = 33
    ri, tags, seqs, n_seq = _collection(workdir, "hits_border_%d" % n_hap, n_hap, 2000, 100 + n_hap)
    rng = np.random.default_rng(3)
    truth, reads = [], []
    while len(reads) < 200:
        q = int(rng.integers(0, len(seqs)))
        s = bytes(seqs[q])
        if len(s) < 60:
            continue
        o = int(rng.integers(0, len(s) - 60 + 1))
        if b"N" in s[o:o + 60]:
            continue
        truth.append((q, o))
        reads.append(s[o:o + 60])
    assert len({q for q, _ in truth}) > 20
    cat, offs = O.pack_reads(reads)
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    b, res = _run_batch(idx, cat, offs, 12, 1)
    b.locate(0)
    got = b.read_place(P.PLACE_LIST)
    assert got["n_reads"] == 200
    for r, (q, o) in enumerate(truth):
        m0 = int(res["mem_offsets"][r])
        assert (int(res["mems"]["start"][m0]), int(res["mems"]["end"][m0])) == (0, 60), r
        assert int(got["reads"]["best_score"][r]) == 60, (r, got["reads"][r])
        mine = got["places"][int(got["place_offsets"][r]):int(got["place_offsets"][r + 1])]
        at = np.flatnonzero((mine["seq"] == q) & (mine["diag"] == o))
        assert len(at) == 1 and int(mine["score"][at[0]]) == 60, (r, q, o)
    b.free()
    idx.close()


def test_places_never_beat_the_hits_of_the_same_run(workdir):
    n_hap = 32
    ri, tags, seqs, n_seq = _collection(workdir, "hits_border_%d" % n_hap, n_hap, 2000, 100 + n_hap)
    cat, offs = W.sample_reads(seqs, 300, 150, seed=21)
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 12, 1)
    sizes = res["mems"]["size"].astype(np.int64)
    distinct = np.unique(sizes[sizes > 0])
    for cap in (0, int(distinct[(len(distinct) - 1) // 2])):
        b.locate(SETS, cap)
        hits = b.read_hits(P.HITS_SCORES)
        b.locate(0, cap)
        pl = b.read_place(P.PLACE_LIST)
        assert (pl["reads"]["best_score"] <= hits["hits"]["best_score"]).all()
        assert np.array_equal(pl["reads"]["n_located"], hits["hits"]["n_located"]) and np.array_equal(pl["reads"]["n_mems"], hits["hits"]["n_mems"])
        top = np.zeros((len(offs) - 1, n_seq), np.uint64)  # the maximum list score of every read on every sequence
        read_of = np.repeat(np.arange(len(offs) - 1), np.diff(pl["place_offsets"].astype(np.int64)))
        np.maximum.at(top, (read_of, pl["places"]["seq"].astype(np.int64)), pl["places"]["score"])
        assert (top <= hits["scores"]).all() and (top > 0).any()
        assert np.array_equal(top.max(axis=1), pl["reads"]["best_score"])
    b.free()
    idx.close()


def test_refusals_leave_everything_as_it_was(workdir):
    ri, tags, seqs, n_seq = _collection(workdir, "hits_border_33", 33, 2000, 133)
    cat, offs = W.sample_reads(seqs, 100, 150, seed=2)
    idx = P.Index(ri, tags)
    b = P.Batch(idx, cat, offs)

    def refused(call):
        with pytest.raises(P.PgxError) as e:
            call()
        assert e.value.code == P.ERR_ARG, str(e.value)
        return str(e.value)

    assert "not been run" in refused(lambda: b.read_place(0))
    b.run(12, 1, P.RUN_TAGS)
    before = b.result()
    assert "no locate result" in refused(lambda: b.read_place(0))
    refused(b.places)
    refused(b.device_places)
    b.locate(0)
    first = b.read_place(P.PLACE_LIST)
    assert first["ms_place"] == 0 and first["n_passes"] == 1  # the run had no PGX_RUN_TIMING
    assert "unknown flag" in refused(lambda: b.read_place(2))
    _same(b.places(), first)
    for flags in (SETS, P.LOCATE_SEQ_IDS, UNIQ_IDS):
        b.locate(flags)
        loc = b.locations()
        assert "ran with flags %d" % flags in refused(lambda: b.read_place(0))
        after, loc2 = b.result(), b.locations()
        for k in ("mem_offsets", "mems", "pos_offsets", "positions"):
            assert after[k].tobytes() == before[k].tobytes(), k
        assert loc2["values"].tobytes() == loc["values"].tobytes() and loc2["loc_offsets"].tobytes() == loc["loc_offsets"].tobytes() and loc2["flags"] == loc["flags"]
        _same(b.places(), first)  # the earlier places stay
    # a re-run and an upload invalidate the places
    b.run(12, 1, P.RUN_TAGS | P.RUN_TIMING)
    refused(b.places)
    refused(lambda: b.read_place(0))  # (the locate belonged to the run before)
    b.locate(0)
    timed = b.read_place(P.PLACE_LIST)
    _same(timed, first)
    assert timed["ms_place"] > 0
    b.upload(cat, offs)
    refused(b.places)
    b.free()
    idx.close()


def test_budget_passes_give_the_same_places(workdir, monkeypatch):
    ri, tags, seqs, n_seq = _collection(workdir, "hits_border_32", 32, 2000, 132)
    cat, offs = W.sample_reads(seqs, 200, 150, seed=4)
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 12, 1)
    b.locate(0)
    one = b.read_place(P.PLACE_LIST)
    assert one["n_passes"] == 1
    most = int(one["reads"]["n_anchors"].max())
    monkeypatch.setenv("PGX_PLACE_BUDGET_MB", repr((3 * most + 5) * 8 / 1048576.0))
    many = b.read_place(P.PLACE_LIST)
    assert many["n_passes"] > 3
    _same(many, one)
    b.free()
    idx.close()
