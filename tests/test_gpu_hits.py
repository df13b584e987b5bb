"""GPU tier of pgx_batch_read_hits: the hits of a batch equal tests/hits_emu.py fed with the batch's MEMs and with sequence sets built
from pgx_locate_batch(PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE) on every MEM's range -- never from pgx_batch_locate -- on the collections
of tests/test_gpu_mem_locate_sets.py (64, 66, 130 and 4096 sequences) and on the golden xy index in both modes; with a cap that leaves
MEMs unlocated, on the resident path and on the sample chains, as host and as device arrays, across a later locate, and for the calls
it refuses."""
import ctypes
import os

import numpy as np
import pytest

import hits_emu as E
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
from test_gpu_mem_locate import _run_batch
from test_gpu_mem_locate_sets import _collection, _expected

pytestmark = pytest.mark.gpu

SETS, UNIQ_IDS = P.LOCATE_SEQ_SETS, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE
BOTH = P.HITS_BEST_SETS | P.HITS_SCORES


def _device_read(src, nbytes):
    """nbytes of device memory at src, by hipMemcpy of the HIP runtime libpgx.so runs on (already in the process)"""
    out = np.zeros(nbytes, np.uint8)
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line}, key=lambda p: "/torch/" in p)
    rcs = []
    for path in paths:
        fn = ctypes.CDLL(path).hipMemcpy
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int], ctypes.c_int
        rcs.append(fn(out.ctypes.data, src, nbytes, 2))
        if rcs[-1] == 0:
            return out
    raise AssertionError("hipMemcpy from the batch's hits failed: %r %r" % (paths, rcs))


def _same(a, b):
    assert a["hits"].tobytes() == b["hits"].tobytes()
    for k in ("best_sets", "scores"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or (a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes())), k


def _check_hits(idx, b, res, max_occ=0):
    """locate(SETS, max_occ) + read_hits == the emulator on sets from pgx_locate_batch; the chains give the same bytes; the device arrays
    hold the same bytes; the hits outlive a locate of another form.  Returns the emulator's result."""
    exp_sets, _, _, _, w = _expected(idx, res["mems"], max_occ)
    n_seq, n = int(idx.info().n_sequences), len(res["mem_offsets"]) - 1
    exp = E.read_hits(res["mem_offsets"], res["mems"], exp_sets, n_seq)
    b.locate(SETS, max_occ)
    got = b.read_hits(BOTH)
    assert (got["n_reads"], got["n_seq"], got["set_words"], got["flags"]) == (n, n_seq, w, BOTH)
    bad = np.flatnonzero(got["hits"] != exp["hits"])
    assert len(bad) == 0, (len(bad), int(bad[0]), got["hits"][bad[0]], exp["hits"][bad[0]])
    _same(got, exp)
    plain = b.read_hits(0)
    assert plain["hits"].tobytes() == exp["hits"].tobytes() and plain["best_sets"] is None and plain["scores"] is None and plain["flags"] == 0
    b.locate(SETS | P.LOCATE_CHAINS, max_occ)
    _same(b.read_hits(BOTH), exp)
    dev = b.device_hits()
    assert dev["device"] and (dev["n_reads"], dev["set_words"], dev["flags"]) == (n, w, BOTH)
    for k, nbytes in (("hits", n * 40), ("best_sets", n * w * 8), ("scores", n * n_seq * 4)):
        assert _device_read(dev[k].__cuda_array_interface__["data"][0], nbytes).tobytes() == exp[k].tobytes(), k
    assert dev["scores"].__cuda_array_interface__["typestr"] == "<u4" and dev["scores"].__cuda_array_interface__["shape"] == (n, n_seq)
    for flags in (0, UNIQ_IDS):  # hits first, positions afterwards
        b.locate(flags)
        _same(b.hits(), exp)
    return exp


@pytest.mark.parametrize("n_hap", [32, 33, 65])
def test_hits_on_word_borders(workdir, n_hap):
    ri, tags, seqs, n_seq = _collection(workdir, "hits_border_%d" % n_hap, n_hap, 2000, 100 + n_hap)
    cat, offs = W.sample_reads(seqs, 400, 150, seed=n_hap)
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 12, 1)
    exp = _check_hits(idx, b, res)
    h = exp["hits"]
    assert (h["best_score"] > 0).any() and (exp["scores"][:, n_seq - 2:] > 0).any()  # (the last word column takes part)
    # a cap that leaves some MEMs unlocated: n_located and covered follow
    sizes = res["mems"]["size"].astype(np.int64)
    distinct = np.unique(sizes[sizes > 0])
    assert len(distinct) >= 2
    cap = int(distinct[(len(distinct) - 1) // 2])  # at least one MEM on either side
    capped = _check_hits(idx, b, res, max_occ=cap)["hits"]
    assert (capped["n_located"] < capped["n_mems"]).any() and (capped["covered"] <= h["covered"]).all()
    assert np.array_equal(capped["n_mems"], h["n_mems"])
    b.free()
    idx.close()


def test_hits_at_4096_sequences(workdir):
    ri, tags, seqs, n_seq = _collection(workdir, "hits_cap_4096", 2048, 100, 11)
    assert n_seq == 4096
    cat, offs = W.sample_reads(seqs, 300, 60, seed=9)
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 12, 1)
    exp = _check_hits(idx, b, res)
    assert (exp["scores"][:, 4032:] > 0).any()  # (the last of the 64 word columns takes part)
    b.free()
    idx.close()


def test_hits_on_xy_in_both_modes(golden):
    bt = os.path.join(golden, "bidirectional_test")
    reads = [l for l in open(os.path.join(bt, "reads.txt"), "rb").read().split(b"\n") if l]
    cat, offs = O.pack_reads(reads)
    ran = 0
    for mode in (P.MODE_COMPAT, P.MODE_STRICT):
        idx = P.Index(os.path.join(bt, "xy.ri"), os.path.join(bt, "xy_bidirectional_compressed.tags"), mode=mode)
        info = idx.info()
        if mode == P.MODE_COMPAT and info.is_encoded and not info.has_N:
            idx.close()
            continue  # (locate is not supported there, as in tests/test_gpu_mem_locate_sets.py)
        for min_len in (3, 5):
            b, res = _run_batch(idx, cat, offs, min_len, 1)
            exp = _check_hits(idx, b, res)
            assert (exp["hits"]["best_score"] > 0).any()
            b.free()
            ran += 1
        idx.close()
    assert ran >= 2


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

    assert "not been run" in refused(lambda: b.read_hits(0))
    b.run(12, 1, P.RUN_TAGS)
    before = b.result()
    refused(lambda: b.read_hits(0))  # no locate yet
    refused(b.hits)
    refused(b.device_hits)
    for flags in (0, UNIQ_IDS, P.LOCATE_SEQ_IDS):
        b.locate(flags)
        loc = b.locations()
        assert "PGX_LOCATE_SEQ_SETS" in refused(lambda: b.read_hits(0))
        refused(b.hits)  # no hits result appears
        after, loc2 = b.result(), b.locations()
        for k in ("mem_offsets", "mems", "pos_offsets", "positions"):
            assert after[k].tobytes() == before[k].tobytes(), k
        assert loc2["values"].tobytes() == loc["values"].tobytes() and loc2["loc_offsets"].tobytes() == loc["loc_offsets"].tobytes() and loc2["flags"] == loc["flags"]
    b.locate(SETS)
    assert "unknown flag" in refused(lambda: b.read_hits(4))
    refused(b.hits)
    first = b.read_hits(BOTH)
    assert "unknown flag" in refused(lambda: b.read_hits(BOTH | 8))
    refused(b.hits)  # a refused call leaves no hits, not the ones of the call before
    _same(b.read_hits(BOTH), first)
    assert first["ms_hits"] == 0  # the run had no PGX_RUN_TIMING
    # a re-run and an upload invalidate the hits
    b.run(12, 1, P.RUN_TAGS | P.RUN_TIMING)
    refused(b.hits)
    refused(lambda: b.read_hits(0))  # (the locate belonged to the run before)
    b.locate(SETS)
    timed = b.read_hits(BOTH)
    _same(timed, first)
    assert timed["ms_hits"] > 0
    b.upload(cat, offs)
    refused(b.hits)
    b.free()
    idx.close()
