"""GPU tier of pgx_batch_read_verify: run, locate(0), read_place(PLACE_LIST) and read_verify equal tests/verify_emu.py fed with the text of
pgx_index_text, the reads of pgx_batch_reads and the candidates chosen in Python from the place result -- on the collections of
tests/test_gpu_hits.py (64, 66 and 130 sequences) and on the golden xy index; as host and as device arrays, across a later locate of every
form; the calls it refuses; and, without the emulator, error-free reads cut from known places and the same reads with one substituted
base, which the place stage alone cannot tell from a read whose other half lies elsewhere."""
import os

import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import verify_emu as E
from test_gpu_hits import _device_read
from test_gpu_mem_locate import _run_batch
from test_gpu_mem_locate_sets import _collection

pytestmark = pytest.mark.gpu

SETS, UNIQ_IDS = P.LOCATE_SEQ_SETS, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE
KEYS = ("reads", "cand_offsets", "cands")


def _same(a, b):
    assert a["reads"].tobytes() == b["reads"].tobytes()
    for k in KEYS[1:]:
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or a[k].tobytes() == b[k].tobytes()), k


def _check_verify(idx, b, penalty=4):
    """locate(0) + read_place(PLACE_LIST) + read_verify(max_cand 1 and 16) == the emulator; the device arrays hold the same bytes; the result
    outlives a locate of every form.  Returns the emulator's result at max_cand 16."""
    lens, text = idx.text()
    seqs = text.split(b"\n")[:-1]
    assert [len(s) for s in seqs] == lens.tolist()
    cat, offs, _ = b.reads()
    reads = [cat[int(offs[r]):int(offs[r + 1])].tobytes() for r in range(len(offs) - 1)]
    n = len(reads)
    b.locate(0)
    place = b.read_place(P.PLACE_LIST)
    for max_cand in (1, 16):
        cands = E.candidates_from_places(place, max_cand)
        exp = E.read_verify(seqs, reads, cands, penalty)
        got = b.read_verify(max_cand, penalty, P.VERIFY_LIST)
        assert (got["n_reads"], got["n_cands"], got["flags"], got["max_cand"], got["mismatch_penalty"]) == (n, len(exp["cands"]), P.VERIFY_LIST, max_cand, penalty)
        bad = np.flatnonzero(got["reads"] != exp["reads"])
        assert len(bad) == 0, (max_cand, len(bad), int(bad[0]), got["reads"][bad[0]], exp["reads"][bad[0]])
        _same(got, exp)
        plain = b.read_verify(max_cand, penalty, 0)
        assert plain["reads"].tobytes() == exp["reads"].tobytes() and plain["cands"] is None and plain["cand_offsets"] is None and plain["flags"] == 0
    b.read_verify(16, penalty, P.VERIFY_LIST)
    dev = b.device_verified()
    assert dev["device"] and (dev["n_reads"], dev["n_cands"], dev["flags"]) == (n, len(exp["cands"]), P.VERIFY_LIST)
    for k, nbytes in (("reads", n * 64), ("cand_offsets", (n + 1) * 8), ("cands", len(exp["cands"]) * 64)):
        if nbytes:
            assert _device_read(dev[k].__cuda_array_interface__["data"][0], nbytes).tobytes() == exp[k].tobytes(), k
    assert dev["reads"].__cuda_array_interface__["shape"] == (n, 8) and dev["cands"].__cuda_array_interface__["shape"] == (len(exp["cands"]), 8)
    for flags in (SETS, UNIQ_IDS, P.LOCATE_SEQ_IDS, P.LOCATE_UNIQUE, 0, P.LOCATE_CHAINS):  # verified first, any locate afterwards
        b.locate(flags)
        _same(b.verified(), exp)
    return exp


@pytest.mark.parametrize("n_hap", [32, 33, 65])
def test_verify_on_the_hits_collections(workdir, n_hap):
    ri, tags, seqs, n_seq = _collection(workdir, "hits_border_%d" % n_hap, n_hap, 2000, 100 + n_hap)
    cat, offs = W.sample_reads(seqs, 100, 150, seed=n_hap)
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 12, 1)
    v = _check_verify(idx, b)["reads"]
    assert (v["n_cand"] > 1).any() and (v["mismatches"] > 0).any() and (v["seg_score"] > 100).any()
    b.free()
    idx.close()


def test_verify_on_xy_in_both_modes(golden):
    bt = os.path.join(golden, "bidirectional_test")
    reads = [l for l in open(os.path.join(bt, "reads.txt"), "rb").read().split(b"\n") if l]
    cat, offs = O.pack_reads(reads)
    ran = 0
    for mode in (P.MODE_COMPAT, P.MODE_STRICT):
        idx = P.Index(os.path.join(bt, "xy.ri"), os.path.join(bt, "xy_bidirectional_compressed.tags"), mode=mode)
        info = idx.info()
        if mode == P.MODE_COMPAT and info.is_encoded and not info.has_N:
            idx.close()
            continue  # (locate is not supported there, as in tests/test_gpu_place.py)
        for min_len, penalty in ((3, 4), (5, 1)):
            b, res = _run_batch(idx, cat, offs, min_len, 1)
            exp = _check_verify(idx, b, penalty)
            assert (exp["reads"]["seg_score"] > 0).any()
            b.free()
            ran += 1
        idx.close()
    assert ran >= 2


def _cut_reads(seqs, n_reads, length, seed):
    rng = np.random.default_rng(seed)
    truth, reads = [], []
    while len(reads) < n_reads:
        q = int(rng.integers(0, len(seqs)))
        s = bytes(seqs[q])
        if len(s) < length:
            continue
        o = int(rng.integers(0, len(s) - length + 1))
        if b"N" in s[o:o + length]:
            continue
        truth.append((q, o))
        reads.append(s[o:o + length])
    return truth, reads


def test_error_free_reads_verify_where_they_were_cut(workdir):
    n_hap = 33
    ri, tags, seqs, n_seq = _collection(workdir, "hits_border_%d" % n_hap, n_hap, 2000, 100 + n_hap)
    truth, reads = _cut_reads(seqs, 200, 60, 3)
    cat, offs = O.pack_reads(reads)
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    b, res = _run_batch(idx, cat, offs, 12, 1)
    b.locate(0)
    b.read_place(P.PLACE_LIST)
    got = b.read_verify(64, 4, P.VERIFY_LIST)
    v = got["reads"]
    assert (v["mismatches"] == 0).all() and (v["matches"] == 60).all() and (v["seg_score"] == 60).all() and (v["seg_mismatches"] == 0).all()
    assert (v["span_lo"] == 0).all() and (v["span_hi"] == 60).all() and (v["seg_start"] == 0).all() and (v["seg_end"] == 60).all()
    assert (v["longest_run"] == 60).all() and (v["run_start"] == 0).all() and (v["cand_index"] == 0).all() and (v["n_tied"] == v["n_cand"]).all()
    for r, (q, o) in enumerate(truth):
        mine = got["cands"][int(got["cand_offsets"][r]):int(got["cand_offsets"][r + 1])]
        assert len(mine) == int(v["n_cand"][r]) >= 1
        if len(mine) < 64:  # (all of the read's best placements are candidates)
            assert ((mine["seq"] == q) & (mine["diag"] == o)).sum() == 1, (r, q, o)
    b.free()
    idx.close()


def test_one_substitution_is_one_mismatch(workdir):
    """what the place stage alone cannot show: with base 30 of 60 substituted no MEM covers the read, so best_score < 60 -- and verify says
    that everything else matches"""
    n_hap = 33
    ri, tags, seqs, n_seq = _collection(workdir, "hits_border_%d" % n_hap, n_hap, 2000, 100 + n_hap)
    truth, reads = _cut_reads(seqs, 200, 60, 4)
    sub = bytes.maketrans(b"ACGT", b"CGTA")
    reads = [r[:30] + r[30:31].translate(sub) + r[31:] for r in reads]
    cat, offs = O.pack_reads(reads)
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    b, res = _run_batch(idx, cat, offs, 12, 1)
    b.locate(0)
    place = b.read_place(P.PLACE_LIST)
    assert (place["reads"]["best_score"] < 60).sum() > 150 and (place["reads"]["best_score"] > 0).all()
    got = b.read_verify(64, 4, P.VERIFY_LIST)
    v = got["reads"]
    exact = 0
    for r, (q, o) in enumerate(truth):
        mine = got["cands"][int(got["cand_offsets"][r]):int(got["cand_offsets"][r + 1])]
        at = np.flatnonzero((mine["seq"] == q) & (mine["diag"] == o))
        if len(at) == 0:
            continue  # (a placement elsewhere covers more of the read, a haplotype that carries the substituted base for one)
        assert len(at) == 1, (r, q, o)
        c = mine[at[0]]
        if int(c["mismatches"]) == 0:
            continue  # (the substituted read is itself a substring of this sequence: a variant site)
        assert (int(c["span_lo"]), int(c["span_hi"]), int(c["matches"]), int(c["mismatches"])) == (0, 60, 59, 1), (r, c)
        assert (int(c["longest_run"]), int(c["run_start"])) == (30, 0) and (int(c["seg_start"]), int(c["seg_end"]), int(c["seg_score"]), int(c["seg_mismatches"])) == (0, 60, 55, 1)
        assert int(v["seg_score"][r]) >= 55 and int(v["matches"][r]) >= 59
        exact += 1
    assert exact > 100
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

    assert "not been run" in refused(lambda: b.read_verify())
    b.run(12, 1, P.RUN_TAGS)
    assert "no place result" in refused(lambda: b.read_verify())
    refused(b.verified)
    refused(b.device_verified)
    b.locate(0)
    b.read_place(0)
    assert "PGX_PLACE_LIST" in refused(lambda: b.read_verify(2))
    first = b.read_verify(1, 4, P.VERIFY_LIST)
    assert first["ms_verify"] == 0  # the run had no PGX_RUN_TIMING
    assert "PGX_PLACE_LIST" in refused(lambda: b.read_verify(16))
    assert "max_cand 0" in refused(lambda: b.read_verify(0))
    assert "max_cand 65" in refused(lambda: b.read_verify(65))
    assert "mismatch_penalty 0" in refused(lambda: b.read_verify(1, 0))
    assert "mismatch_penalty" in refused(lambda: b.read_verify(1, (1 << 20) + 1))
    assert "unknown flag" in refused(lambda: b.read_verify(1, 4, 2))
    _same(b.verified(), first)  # the earlier result stays
    at_limit = b.read_verify(1, 1 << 20, 0)
    assert (at_limit["reads"]["seg_mismatches"] == 0).all()
    # a re-run and an upload invalidate it
    b.run(12, 1, P.RUN_TAGS | P.RUN_TIMING)
    refused(b.verified)
    refused(lambda: b.read_verify())  # (the places belonged to the run before)
    b.locate(0)
    b.read_place(P.PLACE_LIST)
    timed = b.read_verify(1, 4, P.VERIFY_LIST)
    _same(timed, first)
    assert timed["ms_verify"] > 0
    b.upload(cat, offs)
    refused(b.verified)
    b.free()
    idx.close()


def test_compat_without_n_is_unsupported(workdir, golden):
    bt = os.path.join(golden, "bidirectional_test")
    text = os.path.join(bt, "contigs_xy")
    ri = W.build_index_from_text(text, workdir, "verify_compat_xy", encoded=True, with_tags=False)[0]
    idx = P.Index(ri, mode=P.MODE_COMPAT)
    assert idx.info().is_encoded and not idx.info().has_N
    with pytest.raises(P.PgxError) as e:
        idx.text()
    assert e.value.code == P.ERR_UNSUPPORTED
    idx.close()
