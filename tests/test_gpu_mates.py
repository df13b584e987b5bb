"""GPU tier of pgx_batch_read_mates: the batch route on the pairs of tests/mates_cases.py, through a built index -- run(12, 1), locate(0),
read_place(PLACE_LIST), read_verify(16, 4, VERIFY_LIST), read_mates.

Against the emulator: the records equal tests/mates_emu.py fed with the downloaded verify list, the four counters match, the device form
holds the bytes of the host form, and with ELECT the winner records equal the emulator's.  Without the emulator: with ELECT the winner
(seq, diag) of every mate of the classes unique, repeat_*, reverse and hang is the truth of the table, where before the call the half that
lies in the second copy is not; far, cross, same_strand and orphan pairs are not COMPATIBLE and keep their winner records bit for bit;
border pairs flip PROPER exactly at the bounds of a run with frag_min 150; `tie` pairs take (0, 1) of the tied (0, 1) and (1, 0); `below`
pairs are PROPER at U = 10 and not at U = 0; a timed run fills ms_mates.  Align after the election equals align_emu at the elected
candidates and differs from the un-elected run exactly on the moved reads.  A second call gives the same bytes; without ELECT the verify
result stays untouched; every refusal leaves the results as they were; a batch refilled three times equals fresh batches."""
import os

import numpy as np
import pytest

import align_emu as A
import mates_cases as MC
import mates_emu as M
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import verify_emu as V
from test_gpu_hits import _device_read
from test_gpu_mem_locate import _run_batch

pytestmark = pytest.mark.gpu

C = MC.CASES
U = 10  # the unpaired penalty: 2 * (4 + 1), what find_mems --paired takes at --verify-mismatch 4
TRUTHS = [t for p in C.pairs for t in (p["truth_a"], p["truth_b"])]
SECOND_COPY = [k for k, p in enumerate(C.pairs) if p["which"] == 1]
OVERRULED = [k for k, kind in enumerate(C.kinds) if kind in ("tie", "below")]  # the pair moves a mate without a repeat tie to break


def _winner(rec):
    return None if int(rec["seq"]) == V.NO_SEQUENCE else (int(rec["seq"]), int(rec["diag"]))


def _verified_batch(idx, reads):
    cat, offs = O.pack_reads(reads)
    b, _ = _run_batch(idx, cat, offs, MC.MIN_LEN, 1)
    b.locate(0)
    b.read_place(P.PLACE_LIST)
    return b, b.read_verify(16, 4, P.VERIFY_LIST)


@pytest.fixture(scope="module")
def index(workdir):
    path = os.path.join(workdir, "gpu_mates_cases.txt")
    with open(path, "wb") as f:
        f.write(C.raw)
    ri, tags = W.build_index_from_text(path, workdir, "gpu_mates_cases")[:2]
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def verified(index):
    b, v = _verified_batch(index, C.reads)
    yield b, v
    b.free()


def test_the_index_is_twinned_and_the_list_holds_both_copies(index, verified):
    assert index.twinned() is None
    b, v = verified
    for k in SECOND_COPY:
        r = 2 * k + (0 if C.pairs[k]["mate"] == "a" else 1)
        mine = v["cands"][int(v["cand_offsets"][r]):int(v["cand_offsets"][r + 1])]
        assert len(mine) == 2 and (int(mine[1]["seq"]), int(mine[1]["diag"])) == TRUTHS[r] and _winner(v["reads"][r]) == (int(mine[0]["seq"]), int(mine[0]["diag"]))


def test_records_counters_and_forms_equal_the_emulator(verified):
    b, v = verified
    before = b.verified()
    for frag_min in (MC.FRAG_MIN, MC.BORDER_FRAG_MIN):
        exp = M.read_mates(C.lens, v["cand_offsets"], v["cands"], frag_min, MC.FRAG_MAX, U)
        got = b.read_mates(frag_min, MC.FRAG_MAX, U)
        bad = np.flatnonzero(got["pairs"] != exp["pairs"])
        assert len(bad) == 0, (len(bad), int(bad[0]), C.kinds[bad[0]], got["pairs"][bad[0]], exp["pairs"][bad[0]])
        assert got["pairs"].tobytes() == exp["pairs"].tobytes()
        assert {k: got[k] for k in ("n_pairs", "n_proper", "n_compatible", "n_moved_a", "n_moved_b")} == dict(
            n_pairs=len(C.pairs), n_proper=exp["n_proper"], n_compatible=exp["n_compatible"], n_moved_a=exp["n_moved_a"], n_moved_b=exp["n_moved_b"])
        assert (got["frag_min"], got["frag_max"], got["penalty"], got["flags"], got["ms_mates"]) == (frag_min, MC.FRAG_MAX, U, 0, 0)
        dev = b.device_mated()
        assert dev["device"] and {k: dev[k] for k in got if k != "pairs"} == {k: got[k] for k in got if k != "pairs"}
        assert _device_read(dev["pairs"].__cuda_array_interface__["data"][0], len(C.pairs) * 64).tobytes() == exp["pairs"].tobytes()
        assert dev["pairs"].__cuda_array_interface__["shape"] == (len(C.pairs), 8)
        again = b.read_mates(frag_min, MC.FRAG_MAX, U)  # a second call: the same bytes
        assert again["pairs"].tobytes() == got["pairs"].tobytes()
        if frag_min == MC.BORDER_FRAG_MIN:  # without the emulator: PROPER flips exactly at the bounds
            for k, p in enumerate(C.pairs):
                if p["kind"] == "border":
                    assert bool(int(got["pairs"][k]["flags"]) & M.PROPER) == (150 <= p["frag"] <= 500), (k, p["frag"])
    after = b.verified()  # without ELECT the verify result is untouched
    assert all(after[k].tobytes() == before[k].tobytes() for k in ("reads", "cand_offsets", "cands"))
    b.locate(P.LOCATE_UNIQUE)  # a later locate leaves the result valid
    assert b.mated()["pairs"].tobytes() == got["pairs"].tobytes()
    b.locate(0)


def test_the_election_names_the_truth_and_align_follows_it(index):
    b, v = _verified_batch(index, C.reads)  # (a batch of its own: the election rewrites the winners)
    try:
        _election(b, v)
    finally:
        b.free()


def _election(b, v):
    solo_align = b.read_align(8, P.ALIGN_CIGAR)
    for k, p in enumerate(C.pairs):  # before the call: the second-copy half is missed, and nothing else
        if p["kind"] in ("unique", "repeat_a", "repeat_b", "reverse", "hang"):
            assert [_winner(v["reads"][r]) == TRUTHS[r] for r in (2 * k, 2 * k + 1)].count(False) == (1 if k in SECOND_COPY else 0), (k, p["kind"])
    assert len(SECOND_COPY) == 24 and len(OVERRULED) == 20
    exp = M.read_mates(C.lens, v["cand_offsets"], v["cands"], MC.FRAG_MIN, MC.FRAG_MAX, U, M.ELECT)
    got = b.read_mates(MC.FRAG_MIN, MC.FRAG_MAX, U, P.MATES_ELECT)
    assert got["pairs"].tobytes() == exp["pairs"].tobytes() and got["flags"] == P.MATES_ELECT
    elected = b.verified()
    assert elected["reads"].tobytes() == exp["winners"].tobytes()
    assert elected["cands"].tobytes() == v["cands"].tobytes() and elected["cand_offsets"].tobytes() == v["cand_offsets"].tobytes()
    moved = []
    for k, p in enumerate(C.pairs):
        fl = int(got["pairs"][k]["flags"])
        if p["kind"] in ("unique", "repeat_a", "repeat_b", "reverse", "hang", "tie", "below"):
            assert fl & M.PROPER and int(got["pairs"][k]["frag"]) == p["frag"], (k, p["kind"])
            assert [_winner(elected["reads"][r]) for r in (2 * k, 2 * k + 1)] == TRUTHS[2 * k:2 * k + 2], (k, p["kind"])
        if p["kind"] in ("far", "cross", "same_strand", "orphan"):
            assert not fl & M.COMPATIBLE and elected["reads"][2 * k:2 * k + 2].tobytes() == v["reads"][2 * k:2 * k + 2].tobytes(), (k, p["kind"])
        if p["kind"] == "tie":  # (0, 1) and (1, 0) tie in both sums: the smallest i
            assert (int(got["pairs"][k]["cand_a"]), int(got["pairs"][k]["cand_b"]), int(got["pairs"][k]["n_best"])) == (0, 1, 2) and fl & M.MOVED_B
        if p["kind"] == "below":  # the pair scores below the solo winners and within U of them
            assert int(got["pairs"][k]["pair_score"]) < int(got["pairs"][k]["solo_score"]) <= int(got["pairs"][k]["pair_score"]) + U and fl & M.MOVED_A
        moved += [2 * k + m for m, bit in enumerate((M.MOVED_A, M.MOVED_B)) if fl & bit]
    assert sorted(r // 2 for r in moved) == sorted(SECOND_COPY + OVERRULED) and (got["n_moved_a"], got["n_moved_b"]) == (22, 22)
    strict = b.read_mates(MC.FRAG_MIN, MC.FRAG_MAX, 0, P.MATES_ELECT)  # U = 0: the `below` pairs fall back to their solo winners
    for k in OVERRULED:
        assert bool(int(strict["pairs"][k]["flags"]) & M.PROPER) == (C.kinds[k] == "tie"), k
    got = b.read_mates(MC.FRAG_MIN, MC.FRAG_MAX, U, P.MATES_ELECT)
    # a second call on the elected result: the solo winners are recomputed from the list, so the bytes are the same
    again = b.read_mates(MC.FRAG_MIN, MC.FRAG_MAX, U, P.MATES_ELECT)
    assert again["pairs"].tobytes() == got["pairs"].tobytes() == exp["pairs"].tobytes() and b.verified()["reads"].tobytes() == elected["reads"].tobytes()
    # align works on the elected winners
    want = A.read_align(C.seqs, C.reads, A.candidates_from_verified(exp["winners"]), 8)
    al = b.read_align(8, P.ALIGN_CIGAR)
    assert al["reads"].tobytes() == want["reads"].tobytes() and al["ops"].tobytes() == want["ops"].tobytes()
    assert sorted(np.flatnonzero(al["reads"] != solo_align["reads"])) == sorted(moved)


def test_ms_mates_is_filled_under_run_timing(index, verified):
    cat, offs = O.pack_reads(C.reads)
    b = P.Batch(index, cat, offs)
    try:
        b.run(MC.MIN_LEN, 1, P.RUN_TAGS | P.RUN_TIMING)
        b.locate(0)
        b.read_place(P.PLACE_LIST)
        b.read_verify(16, 4, P.VERIFY_LIST)
        timed = b.read_mates(MC.FRAG_MIN, MC.FRAG_MAX, U)
        assert 0 < timed["ms_mates"] < 1000 and b.device_mated()["ms_mates"] == timed["ms_mates"]
        assert timed["pairs"].tobytes() == verified[0].read_mates(MC.FRAG_MIN, MC.FRAG_MAX, U)["pairs"].tobytes()
    finally:
        b.free()


def test_refusals_leave_everything_as_it_was(index, verified, workdir):
    b, v = verified
    first = b.read_mates(MC.FRAG_MIN, MC.FRAG_MAX, U)

    def refused(call, code=P.ERR_ARG):
        with pytest.raises(P.PgxError) as e:
            call()
        assert e.value.code == code, str(e.value)
        return str(e.value)

    assert "unknown flag" in refused(lambda: b.read_mates(0, 500, U, 2))
    assert "frag_min 501 exceeds frag_max 500" in refused(lambda: b.read_mates(501, 500, U))
    assert b.mated()["pairs"].tobytes() == first["pairs"].tobytes() and b.verified()["reads"].tobytes() == v["reads"].tobytes()
    cat, offs = O.pack_reads(C.reads)
    nb = P.Batch(index, cat, offs)
    assert "not been run" in refused(lambda: nb.read_mates(0, 500, U))
    nb.run(MC.MIN_LEN, 1, P.RUN_TAGS)
    assert "no verify result" in refused(lambda: nb.read_mates(0, 500, U))
    refused(nb.mated)
    refused(nb.device_mated)
    nb.locate(0)
    nb.read_place(P.PLACE_LIST)
    nb.read_verify(16, 4)
    assert "PGX_VERIFY_LIST" in refused(lambda: nb.read_mates(0, 500, U))  # a verify result without the list
    nb.read_verify(16, 4, P.VERIFY_LIST)
    ok = nb.read_mates(0, 500, U)
    assert ok["pairs"].tobytes() == first["pairs"].tobytes()
    nb.run(MC.MIN_LEN, 1, P.RUN_TAGS)  # a stale run: the verify result belongs to the run before
    assert "no verify result" in refused(lambda: nb.read_mates(0, 500, U))
    refused(nb.mated)
    nb.free()
    odd, _ = _verified_batch(index, C.reads[:5])
    assert "5 reads, an odd number" in refused(lambda: odd.read_mates(0, 500, U))
    odd.free()
    # a forward-only index
    path = os.path.join(workdir, "gpu_mates_forward.txt")
    with open(path, "wb") as f:
        f.write(C.seqs[0] + b"\n" + C.seqs[1] + b"\n" + C.seqs[2] + b"\n" + C.seqs[4] + b"\n")
    ri, tags = W.build_index_from_text(path, workdir, "gpu_mates_forward")[:2]
    fwd = P.Index(ri, tags, mode=P.MODE_STRICT)
    fb, _ = _verified_batch(fwd, C.reads[:4])
    assert fwd.twinned() == 1
    text = refused(lambda: fb.read_mates(0, 500, U), P.ERR_UNSUPPORTED)
    assert "not twinned" in text and "p = 1" in text
    refused(fb.mated)
    fb.free()
    fwd.close()


def test_a_refilled_batch_equals_fresh_batches(index):
    sets = [C.reads[:40], C.reads[40:200], C.reads[100:112]]
    cat, offs = O.pack_reads(sets[0])
    b = P.Batch(index, cat, offs)
    for k, reads in enumerate(sets):
        if k:
            cat, offs = O.pack_reads(reads)
            b.upload(cat, offs)
        b.run(MC.MIN_LEN, 1, P.RUN_TAGS)
        b.locate(0)
        b.read_place(P.PLACE_LIST)
        b.read_verify(16, 4, P.VERIFY_LIST)
        got = b.read_mates(MC.FRAG_MIN, MC.FRAG_MAX, U, P.MATES_ELECT)
        fresh, _ = _verified_batch(index, reads)
        want = fresh.read_mates(MC.FRAG_MIN, MC.FRAG_MAX, U, P.MATES_ELECT)
        assert got["pairs"].tobytes() == want["pairs"].tobytes() and b.verified()["reads"].tobytes() == fresh.verified()["reads"].tobytes(), k
        assert {x: got[x] for x in got if x != "pairs"} == {x: want[x] for x in want if x != "pairs"}
        fresh.free()
    b.free()
