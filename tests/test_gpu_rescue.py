"""GPU tier of pgx_batch_read_rescue: the batch route on the pairs of tests/rescue_cases.py, through a built index -- run(12, 1), locate(0),
read_place(PLACE_LIST), read_verify(16, 4, VERIFY_LIST), read_rescue, read_mates.

Against the emulator: the records equal tests/rescue_emu.py fed with the downloaded verify list, the five counters match, the device form
holds the bytes of the host form, and with MERGE the list, its offsets and the winners equal the emulator's.  Without the emulator: every
planted mate of the classes dense, dense_both_strands, repeat_anchor and edge has no winner before the call and sits on the truth of the table
after rescue and mates, in a PROPER pair; junk mates stay unplaced; a second rescue call on the merged result is refused; without MERGE the
verify bytes stay as they were; align and walk run on the rescued winners; a timed run fills ms_rescue; every refusal leaves the results as
they were; a batch refilled three times equals fresh batches."""
import os

import numpy as np
import pytest

import align_emu as A
import mates_emu as M
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import rescue_cases as RC
import rescue_emu as R
import verify_emu as V
from test_gpu_hits import _device_read
from test_gpu_mem_locate import _run_batch

pytestmark = pytest.mark.gpu

C = RC.CASES
U = 10
ARGS = (RC.FRAG_MIN, RC.FRAG_MAX, RC.MIN_LEN, 2)
COUNTERS = ("n_reads", "n_targets", "n_rescued", "n_full", "n_tasks", "n_diags")
PLANTED = [k for k, p in enumerate(C.pairs) if p["kind"] in ("dense", "dense_both_strands", "repeat_anchor", "edge")]


def _winner(rec):
    return None if int(rec["seq"]) == V.NO_SEQUENCE else (int(rec["seq"]), int(rec["diag"]))


def _mate(k):
    p = C.pairs[k]
    return (2 * k, p["truth_a"]) if p["mate"] == "a" else (2 * k + 1, p["truth_b"])


def _verified_batch(idx, reads, flags=P.RUN_TAGS):
    cat, offs = O.pack_reads(reads)
    b = P.Batch(idx, cat, offs)
    b.run(RC.MIN_LEN, 1, flags)
    b.locate(0)
    b.read_place(P.PLACE_LIST)
    return b, b.read_verify(16, RC.PENALTY, P.VERIFY_LIST)


@pytest.fixture(scope="module")
def index(workdir):
    path = os.path.join(workdir, "gpu_rescue_cases.txt")
    with open(path, "wb") as f:
        f.write(C.raw)
    ri, tags = W.build_index_from_text(path, workdir, "gpu_rescue_cases")[:2]
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def verified(index):
    b, v = _verified_batch(index, C.reads)
    yield b, v
    b.free()


@pytest.fixture(scope="module")
def expected(verified):
    _, v = verified
    return R.read_rescue(C.seqs, C.reads, v["cand_offsets"], v["cands"], *ARGS[:2], RC.PENALTY, *ARGS[2:], R.MERGE)


def test_records_counters_and_forms_equal_the_emulator_and_verify_stays(verified, expected):
    b, v = verified
    before = b.verified()
    mated = b.read_mates(RC.FRAG_MIN, RC.FRAG_MAX, U)
    got = b.read_rescue(*ARGS)
    bad = np.flatnonzero(got["reads"] != expected["reads"])
    assert len(bad) == 0, (len(bad), int(bad[0]), C.kinds[bad[0] // 2], got["reads"][bad[0]], expected["reads"][bad[0]])
    assert got["reads"].tobytes() == expected["reads"].tobytes()
    assert {k: got[k] for k in COUNTERS} == dict(n_reads=len(C.reads), **{k: expected[k] for k in COUNTERS[1:]})
    assert (got["n_targets"], got["n_rescued"], got["n_tasks"]) == (94, 59, 104)
    assert (got["frag_min"], got["frag_max"], got["min_score"], got["max_anchors"], got["flags"], got["mismatch_penalty"], got["ms_rescue"]) == (0, 500, 12, 2, 0, 4, 0)
    dev = b.device_rescued()
    assert dev["device"] and {k: dev[k] for k in got if k != "reads"} == {k: got[k] for k in got if k != "reads"}
    assert _device_read(dev["reads"].__cuda_array_interface__["data"][0], len(C.reads) * 64).tobytes() == expected["reads"].tobytes()
    assert dev["reads"].__cuda_array_interface__["shape"] == (len(C.reads), 8)
    assert b.read_rescue(*ARGS)["reads"].tobytes() == got["reads"].tobytes()  # a second call without MERGE: the same bytes
    one = b.read_rescue(RC.FRAG_MIN, RC.FRAG_MAX, RC.MIN_LEN, 1)  # other parameters
    want = R.read_rescue(C.seqs, C.reads, v["cand_offsets"], v["cands"], RC.FRAG_MIN, RC.FRAG_MAX, RC.PENALTY, RC.MIN_LEN, 1)
    assert one["reads"].tobytes() == want["reads"].tobytes() and one["n_tasks"] == want["n_tasks"] == 94 and one["n_rescued"] == 49
    after = b.verified()  # without MERGE the verify result is untouched, and so is the mates result
    assert all(after[k].tobytes() == before[k].tobytes() for k in ("reads", "cand_offsets", "cands")) and after["n_cands"] == before["n_cands"]
    assert b.mated()["pairs"].tobytes() == mated["pairs"].tobytes()
    b.locate(P.LOCATE_UNIQUE)  # a later locate leaves the result valid
    assert b.rescued()["reads"].tobytes() == one["reads"].tobytes()
    b.locate(0)


def test_every_planted_mate_is_on_its_truth_after_rescue_and_mates(index, expected):
    b, v = _verified_batch(index, C.reads)  # (a batch of its own: the merge rewrites the verify result)
    try:
        _merge(b, v, expected)
    finally:
        b.free()


def _merge(b, v, expected):
    for k in PLANTED:  # before: no winner
        assert _winner(v["reads"][_mate(k)[0]]) is None, k
    b.read_mates(RC.FRAG_MIN, RC.FRAG_MAX, U)
    got = b.read_rescue(*ARGS, P.RESCUE_MERGE)
    assert got["reads"].tobytes() == expected["reads"].tobytes() and got["flags"] == P.RESCUE_MERGE and got["n_rescued"] == 59
    merged = b.verified()
    assert merged["n_cands"] == v["n_cands"] + 59 and merged["max_cand"] == 16
    assert np.array_equal(merged["cand_offsets"], expected["cand_offsets"])
    assert merged["cands"].tobytes() == expected["cands"].tobytes() and merged["reads"].tobytes() == expected["winners"].tobytes()
    with pytest.raises(P.PgxError) as e:  # the mates result of before the merge is gone
        b.mated()
    assert e.value.code == P.ERR_ARG
    for call in (lambda: b.read_rescue(*ARGS, P.RESCUE_MERGE), lambda: b.read_rescue(*ARGS)):  # a merged verify result takes no second rescue
        with pytest.raises(P.PgxError) as e:
            call()
        assert e.value.code == P.ERR_ARG and "already merged" in str(e.value)
    assert b.rescued()["reads"].tobytes() == expected["reads"].tobytes() and b.verified()["cands"].tobytes() == expected["cands"].tobytes()
    want = M.read_mates(C.lens, expected["cand_offsets"], expected["cands"], RC.FRAG_MIN, RC.FRAG_MAX, U, M.ELECT)
    mates = b.read_mates(RC.FRAG_MIN, RC.FRAG_MAX, U, P.MATES_ELECT)
    assert mates["pairs"].tobytes() == want["pairs"].tobytes() and mates["n_proper"] == 69
    elected = b.verified()
    assert elected["reads"].tobytes() == want["winners"].tobytes()
    for k, p in enumerate(C.pairs):  # without the emulator
        r = 2 * k + 1 if p["mate"] in ("b", None) else 2 * k
        if k in PLANTED:
            assert [_winner(elected["reads"][x]) for x in (2 * k, 2 * k + 1)] == [p["truth_a"], p["truth_b"]], (k, p["kind"])
            assert int(mates["pairs"][k]["flags"]) & M.PROPER and int(mates["pairs"][k]["frag"]) == p["frag"]
        elif p["kind"] == "junk":
            assert _winner(elected["reads"][r]) is None and not int(got["reads"][r]["flags"]) & R.RESCUED
        elif p["kind"] == "threshold":
            assert (_winner(elected["reads"][r]) == p["truth_b"]) == (p["score"] == 12) == bool(int(mates["pairs"][k]["flags"]) & M.PROPER)
        elif p["kind"] == "tandem":
            assert _winner(elected["reads"][r]) == (p["truth_a"][0], p["ties"][0]) and int(got["reads"][r]["n_best"]) == 7
    # align and walk on the rescued winners
    want_al = A.read_align(C.seqs, C.reads, A.candidates_from_verified(want["winners"]), 8)
    al = b.read_align(8, P.ALIGN_CIGAR)
    assert al["reads"].tobytes() == want_al["reads"].tobytes() and al["ops"].tobytes() == want_al["ops"].tobytes()
    assert all(int(al["reads"][_mate(k)[0]]["seq"]) == _mate(k)[1][0] for k in PLANTED)
    wk = b.read_walk(P.WALK_STEPS)
    assert wk["n_reads"] == len(C.reads)
    # a new verify call makes the result fresh again: rescue is served once more
    b.read_verify(16, RC.PENALTY, P.VERIFY_LIST)
    assert b.read_rescue(*ARGS, P.RESCUE_MERGE)["reads"].tobytes() == expected["reads"].tobytes()


def test_ms_rescue_is_filled_under_run_timing(index, expected):
    b, _ = _verified_batch(index, C.reads, P.RUN_TAGS | P.RUN_TIMING)
    try:
        timed = b.read_rescue(*ARGS, P.RESCUE_MERGE)
        assert 0 < timed["ms_rescue"] < 1000 and b.device_rescued()["ms_rescue"] == timed["ms_rescue"]
        assert timed["reads"].tobytes() == expected["reads"].tobytes() and b.verified()["cands"].tobytes() == expected["cands"].tobytes()
    finally:
        b.free()


def test_refusals_leave_everything_as_it_was(index, verified, workdir):
    b, v = verified
    first = b.read_rescue(*ARGS)
    mated = b.read_mates(RC.FRAG_MIN, RC.FRAG_MAX, U)

    def refused(call, code=P.ERR_ARG):
        with pytest.raises(P.PgxError) as e:
            call()
        assert e.value.code == code, str(e.value)
        return str(e.value)

    assert "unknown flag" in refused(lambda: b.read_rescue(0, 500, 12, 2, 2))
    assert "frag_min 501 exceeds frag_max 500" in refused(lambda: b.read_rescue(501, 500, 12, 2))
    assert "window" in refused(lambda: b.read_rescue(0, 65536, 12, 2))
    assert "min_score 0" in refused(lambda: b.read_rescue(0, 500, 0, 2))
    assert "max_anchors 0" in refused(lambda: b.read_rescue(0, 500, 12, 0)) and "max_anchors 9" in refused(lambda: b.read_rescue(0, 500, 12, 9, P.RESCUE_MERGE))
    assert b.rescued()["reads"].tobytes() == first["reads"].tobytes() and b.mated()["pairs"].tobytes() == mated["pairs"].tobytes()
    assert all(b.verified()[k].tobytes() == v[k].tobytes() for k in ("reads", "cand_offsets", "cands"))
    assert b.read_rescue(0, 65535, 12, 2)["n_targets"] == 74  # the widest window is served (the ten `both` pairs are compatible under it)
    cat, offs = O.pack_reads(C.reads)
    nb = P.Batch(index, cat, offs)
    assert "not been run" in refused(lambda: nb.read_rescue(*ARGS))
    nb.run(RC.MIN_LEN, 1, P.RUN_TAGS)
    assert "no verify result" in refused(lambda: nb.read_rescue(*ARGS))
    refused(nb.rescued)
    refused(nb.device_rescued)
    nb.locate(0)
    nb.read_place(P.PLACE_LIST)
    nb.read_verify(16, RC.PENALTY)
    assert "PGX_VERIFY_LIST" in refused(lambda: nb.read_rescue(*ARGS))  # a verify result without the list
    nb.read_verify(16, RC.PENALTY, P.VERIFY_LIST)
    assert nb.read_rescue(*ARGS)["reads"].tobytes() == first["reads"].tobytes()
    nb.run(RC.MIN_LEN, 1, P.RUN_TAGS)  # a stale run: the verify result belongs to the run before
    assert "no verify result" in refused(lambda: nb.read_rescue(*ARGS))
    refused(nb.rescued)
    nb.free()
    odd, _ = _verified_batch(index, C.reads[:5])
    assert "5 reads, an odd number" in refused(lambda: odd.read_rescue(*ARGS))
    odd.free()
    # a forward-only index
    path = os.path.join(workdir, "gpu_rescue_forward.txt")
    with open(path, "wb") as f:
        f.write(C.seqs[0] + b"\n" + C.seqs[1] + b"\n" + C.seqs[2] + b"\n" + C.seqs[4] + b"\n")
    ri, tags = W.build_index_from_text(path, workdir, "gpu_rescue_forward")[:2]
    fwd = P.Index(ri, tags, mode=P.MODE_STRICT)
    fb, _ = _verified_batch(fwd, C.reads[:4])
    text = refused(lambda: fb.read_rescue(*ARGS), P.ERR_UNSUPPORTED)
    assert "not twinned" in text and "p = 1" in text
    refused(fb.rescued)
    fb.free()
    fwd.close()


def test_a_refilled_batch_equals_fresh_batches(index):
    sets = [C.reads[:40], C.reads[40:188], C.reads[100:112]]
    cat, offs = O.pack_reads(sets[0])
    b = P.Batch(index, cat, offs)
    for k, reads in enumerate(sets):
        if k:
            cat, offs = O.pack_reads(reads)
            b.upload(cat, offs)
        b.run(RC.MIN_LEN, 1, P.RUN_TAGS)
        b.locate(0)
        b.read_place(P.PLACE_LIST)
        b.read_verify(16, RC.PENALTY, P.VERIFY_LIST)
        got = b.read_rescue(*ARGS, P.RESCUE_MERGE)
        fresh, _ = _verified_batch(index, reads)
        want = fresh.read_rescue(*ARGS, P.RESCUE_MERGE)
        assert got["reads"].tobytes() == want["reads"].tobytes() and {x: got[x] for x in got if x != "reads"} == {x: want[x] for x in want if x != "reads"}, k
        assert all(b.verified()[x].tobytes() == fresh.verified()[x].tobytes() for x in ("reads", "cand_offsets", "cands")), k
        fresh.free()
    b.free()
