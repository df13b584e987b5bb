"""GPU tier of pgx_batch_read_align: run, locate(0), read_place, read_verify and read_align equal tests/align_emu.py fed with the text of
pgx_index_text, the reads of pgx_batch_reads and the winners of the verify result -- on the collections of tests/test_gpu_verify.py (64, 66
and 130 sequences) and on the golden xy index; as host and as device arrays, across a later locate of every form; the calls it refuses; and,
without the emulator, error-free reads of 60 bases as they were cut, with base 30 deleted and with a base inserted at 30: what verify reports
as a wall of mismatches is one edit."""
import os
import re

import numpy as np
import pytest

import align_cases as C
import align_emu as E
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
from test_gpu_hits import _device_read
from test_gpu_mem_locate import _run_batch
from test_gpu_mem_locate_sets import _collection

pytestmark = pytest.mark.gpu

SETS, UNIQ_IDS = P.LOCATE_SEQ_SETS, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE
KEYS = ("reads", "op_offsets", "ops")


def _same(a, b):
    assert a["reads"].tobytes() == b["reads"].tobytes()
    for k in KEYS[1:]:
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or a[k].tobytes() == b[k].tobytes()), k


def _check_align(idx, b, bands=(8, 0, 3), max_cand=1, penalty=4):
    """locate(0) + read_place + read_verify + read_align at every band == the emulator at the verify winners; the device arrays hold the same
    bytes; the result outlives a locate of every form.  Returns the emulator's result at the first band."""
    lens, text = idx.text()
    seqs = text.split(b"\n")[:-1]
    cat, offs, _ = b.reads()
    reads = [cat[int(offs[r]):int(offs[r + 1])].tobytes() for r in range(len(offs) - 1)]
    n = len(reads)
    b.locate(0)
    b.read_place(P.PLACE_LIST)
    verified = b.read_verify(max_cand, penalty)
    cands = E.candidates_from_verified(verified["reads"])
    first = None
    for band in reversed(bands):
        exp = E.read_align(seqs, reads, cands, band)
        got = b.read_align(band, P.ALIGN_CIGAR)
        assert (got["n_reads"], got["n_ops"], got["flags"], got["band"], got["passes"]) == (n, len(exp["ops"]), P.ALIGN_CIGAR, band, 1 if n else 0)
        bad = np.flatnonzero(got["reads"] != exp["reads"])
        assert len(bad) == 0, (band, len(bad), int(bad[0]), got["reads"][bad[0]], exp["reads"][bad[0]])
        _same(got, exp)
        plain = b.read_align(band, 0)
        assert plain["reads"].tobytes() == exp["reads"].tobytes() and plain["ops"] is None and plain["op_offsets"] is None and plain["flags"] == 0
        assert plain["n_ops"] == len(exp["ops"])
        if band == 0:
            v = verified["reads"]
            assert (got["reads"]["edits"] == v["mismatches"]).all() and (got["reads"]["n_match"] == v["matches"]).all()
        first = exp
    b.read_align(bands[0], P.ALIGN_CIGAR)
    dev = b.device_aligned()
    assert dev["device"] and (dev["n_reads"], dev["n_ops"], dev["flags"]) == (n, len(first["ops"]), P.ALIGN_CIGAR)
    for k, nbytes in (("reads", n * 64), ("op_offsets", (n + 1) * 8), ("ops", len(first["ops"]) * 4)):
        if nbytes:
            assert _device_read(dev[k].__cuda_array_interface__["data"][0], nbytes).tobytes() == first[k].tobytes(), k
    assert dev["reads"].__cuda_array_interface__["shape"] == (n, 8) and dev["ops"].__cuda_array_interface__["shape"] == (len(first["ops"]),)
    for flags in (SETS, UNIQ_IDS, P.LOCATE_SEQ_IDS, P.LOCATE_UNIQUE, 0, P.LOCATE_CHAINS):  # aligned first, any locate afterwards
        b.locate(flags)
        _same(b.aligned(), first)
    return first


@pytest.mark.parametrize("n_hap", [32, 33, 65])
def test_align_on_the_verify_collections(workdir, n_hap):
    ri, tags, seqs, n_seq = _collection(workdir, "hits_border_%d" % n_hap, n_hap, 2000, 100 + n_hap)
    cat, offs = W.sample_reads(seqs, 100, 150, seed=n_hap)
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 12, 1)
    v = _check_align(idx, b, max_cand=16 if n_hap == 33 else 1)["reads"]
    assert (v["n_match"] > 100).any() and (v["seq"] != E.NO_SEQUENCE).any()
    b.free()
    idx.close()


def test_align_on_xy_in_both_modes(golden):
    bt = os.path.join(golden, "bidirectional_test")
    reads = [l for l in open(os.path.join(bt, "reads.txt"), "rb").read().split(b"\n") if l]
    cat, offs = O.pack_reads(reads)
    ran = 0
    for mode in (P.MODE_COMPAT, P.MODE_STRICT):
        idx = P.Index(os.path.join(bt, "xy.ri"), os.path.join(bt, "xy_bidirectional_compressed.tags"), mode=mode)
        info = idx.info()
        if mode == P.MODE_COMPAT and info.is_encoded and not info.has_N:
            idx.close()
            continue  # (locate is not supported there, as in tests/test_gpu_verify.py)
        for min_len, bands in ((3, (8, 0, 1)), (5, (31, 2))):
            b, res = _run_batch(idx, cat, offs, min_len, 1)
            exp = _check_align(idx, b, bands)
            assert (exp["reads"]["n_match"] > 0).any()
            b.free()
            ran += 1
        idx.close()
    assert ran >= 2


@pytest.fixture(scope="module")
def cut(workdir):
    """the collection of 66 sequences, its index, the reads of tests/align_cases.py and where they were cut"""
    c = C.COLLECTION
    ri, tags, seqs, n_seq = _collection(workdir, c["name"], c["n_hap"], c["base_len"], c["seed"])
    seqs = [bytes(s) for s in seqs]
    truth, reads = C.cut_reads(seqs)
    return ri, tags, seqs, truth, reads


def _aligned_and_verified(ri, tags, reads, band=8):
    cat, offs = O.pack_reads(reads)
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    b, res = _run_batch(idx, cat, offs, 12, 1)
    b.locate(0)
    b.read_place(0)
    verified = b.read_verify(1, 4)["reads"]
    got = b.read_align(band, P.ALIGN_CIGAR)
    b.free()
    idx.close()
    cigars = [P.cigar_text(got["ops"][int(got["op_offsets"][r]):int(got["op_offsets"][r + 1])]) for r in range(len(reads))]
    return got["reads"], cigars, verified


def test_error_free_reads_align_without_an_edit(cut):
    ri, tags, seqs, truth, reads = cut
    a, cigars, verified = _aligned_and_verified(ri, tags, reads)
    assert (a["edits"] == 0).all() and cigars == ["60="] * C.N_READS
    assert (a["text_end"] - a["text_start"] == 60).all() and not a["band_hit"].any() and (a["n_ops"] == 1).all()
    for r, (q, o) in enumerate(truth):
        assert seqs[int(a["seq"][r])][int(a["text_start"][r]):int(a["text_end"][r])] == reads[r]


def _kept(seqs, forms, verified):
    """the reads the expectation "one edit" holds for: not those whose mutated form occurs in the collection as it is (fewer edits than
    one: tests/test_align_cpu.py bounds their number by the emulator alone), and not those whose verify winner lies on a sequence that holds
    the mutated form with no fewer than two edits (a haplotype with a variant of its own next to the cut: the stage aligns the winner only) --
    the latter decided by the emulator on that one sequence.  At most 5 % of the reads are left out in all."""
    out = C.fewer_edits_elsewhere(forms, seqs)
    for r in np.flatnonzero(~out):
        if int(verified["seq"][r]) == E.NO_SEQUENCE or int(E.infix_distances(forms[r], [seqs[int(verified["seq"][r])]])[0]) > 1:
            out[r] = True
    assert out.sum() <= C.MAX_LEFT_OUT, int(out.sum())
    return np.flatnonzero(~out)


def test_a_deleted_base_is_one_deletion(cut):
    ri, tags, seqs, truth, reads = cut
    forms = C.deleted(reads)
    a, cigars, verified = _aligned_and_verified(ri, tags, forms)
    keep = _kept(seqs, forms, verified)
    assert (a["seq"] == verified["seq"]).all() and (a["diag"] == verified["diag"]).all()
    assert (a["edits"][keep] == 1).all() and (a["n_del"][keep] == 1).all() and (a["n_ins"][keep] == 0).all() and (a["n_mismatch"][keep] == 0).all()
    assert (verified["mismatches"][keep] > 1).all()  # what the chain could say before: part of the read matches, then a wall of mismatches
    assert (a["n_match"][keep] + a["clip_lo"][keep] + a["clip_hi"][keep] == 59).all()
    for r in keep:  # (a read cut at the end of its sequence hangs over on the neighbouring diagonal: a soft clip)
        m = re.fullmatch(r"(?:\d+S)?(\d+)=1D(\d+)=(?:\d+S)?", cigars[r])
        assert m and int(m.group(1)) <= C.AT, (r, cigars[r])


def test_an_inserted_base_is_one_insertion(cut):
    ri, tags, seqs, truth, reads = cut
    forms = C.inserted(reads)
    a, cigars, verified = _aligned_and_verified(ri, tags, forms)
    keep = _kept(seqs, forms, verified)
    assert (a["seq"] == verified["seq"]).all() and (a["diag"] == verified["diag"]).all()
    assert (a["edits"][keep] == 1).all() and (a["n_ins"][keep] == 1).all() and (a["n_del"][keep] == 0).all() and (a["n_mismatch"][keep] == 0).all()
    assert (a["n_match"][keep] + a["clip_lo"][keep] + a["clip_hi"][keep] == 60).all()
    for r in keep:  # (behind a run of the inserted base the gap goes leftmost)
        m = re.fullmatch(r"(?:\d+S)?(\d+)=1I(\d+)=(?:\d+S)?", cigars[r])
        assert m and int(m.group(1)) <= C.AT, (r, cigars[r])


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

    assert "not been run" in refused(lambda: b.read_align())
    b.run(12, 1, P.RUN_TAGS)
    assert "no verify result" in refused(lambda: b.read_align())
    refused(b.aligned)
    refused(b.device_aligned)
    b.locate(0)
    b.read_place(0)
    assert "no verify result" in refused(lambda: b.read_align())
    b.read_verify(1, 4)
    first = b.read_align(8, P.ALIGN_CIGAR)
    assert first["ms_align"] == 0 and first["ms_forward"] == 0  # the run had no PGX_RUN_TIMING
    assert "band 32" in refused(lambda: b.read_align(32))
    assert "unknown flag" in refused(lambda: b.read_align(8, 2))
    _same(b.aligned(), first)  # the earlier result stays
    widest = b.read_align(31, 0)
    assert (widest["reads"]["edits"] <= first["reads"]["edits"]).all()
    # a re-run and an upload invalidate it
    b.run(12, 1, P.RUN_TAGS | P.RUN_TIMING)
    refused(b.aligned)
    refused(lambda: b.read_align())  # (the verify result belonged to the run before)
    b.locate(0)
    b.read_place(0)
    b.read_verify(1, 4)
    timed = b.read_align(8, P.ALIGN_CIGAR)
    _same(timed, first)
    assert timed["ms_align"] > 0 and timed["ms_forward"] > 0 and timed["ms_trace"] > 0 and timed["scratch_bytes"] >= 100 * 150 * 8
    b.upload(cat, offs)
    refused(b.aligned)
    b.free()
    idx.close()
