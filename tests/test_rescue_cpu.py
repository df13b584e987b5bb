"""CPU tier of read rescue (include/pgx.h "read rescue"): the emulator of tests/rescue_emu.py on hand-worked windows and lists; its linear
segment score against verify_emu's quadratic search; the layout of the records, the header's constants, the exported entry points and,
without a GPU, PGX_ERR_NO_DEVICE (these fail on a library without the stage); the case table of tests/rescue_cases.py with its pinned
counts; and the case chain: the oracle's MEMs of every read, located, go through place_emu and verify_emu at max_cand 16, the emulator
rescues every dense mate to exactly its truth, leaves every random mate alone, and mates_emu on the merged list makes every such pair PROPER.

Each mutation of the emulator changes at least one record of the class it targets; the counts are stated."""
import ctypes
import os
import re

import numpy as np
import pytest

import mates_emu as M
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import place_emu as E
import rescue_cases as RC
import rescue_emu as R
import verify_emu as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = RC.CASES
ENTRY_POINTS = ("pgx_batch_read_rescue", "pgx_batch_rescued", "pgx_batch_device_rescued", "pgx_read_rescue_arrays")
RESCUED_KINDS = ("dense", "dense_both_strands", "repeat_anchor", "edge")


def cand(seq, diag, score, matches=None):
    return dict(seq=seq, diag=diag, seg_score=score, matches=score if matches is None else matches)


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulator by hand
def test_windows_by_hand():
    assert R.window(1000, 50, 100, 0, 500) == (400, 900)            # L - diag - frag_max .. L - diag - frag_min
    assert R.window(1000, 50, 100, 150, 150) == (750, 750)          # one diagonal
    assert R.window(1000, 50, 900, 0, 500) == (-49, 100)            # clipped at the start: the read's last base on the first symbol
    assert R.window(1000, 50, -200, 0, 500) == (700, 999)           # clipped at the end: the read's first base on the last symbol
    assert R.window(64, 50, 0, 0, 500) == (-49, 63)                 # on both sides
    assert R.window(64, 1, 0, 0, 500) == (0, 63)
    assert R.window(1000, 50, -1000, 0, 500) == (0, -1)             # beyond the end: empty
    assert R.window(1000, 50, 1050, 0, 500) == (0, -1)              # before the start: empty
    assert R.window(1000, 50, 1049, 0, 500) == (-49, -49)
    assert R.window(1000, 0, 100, 0, 500) == (0, -1)                # an empty read
    assert R.window(0, 50, 0, 0, 500) == (-49, -1)                  # an empty sequence: diagonals without a span
    assert R.window(1, 50, 0, 0, 500) == (-49, 0)
    assert R.window(1000, 50, 2 ** 61, -2 ** 61 + 1, -2 ** 61 + 1000) == (0, 999)  # (exact integers: the kernel clamps the bounds instead)


def test_the_linear_score_is_verifys_segment_score():
    rng = np.random.default_rng(5)
    n = 0
    for trial in range(300):
        seq = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=int(rng.integers(0, 40)), p=[.24, .24, .24, .24, .04]))
        read = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(rng.integers(0, 30))))
        d = int(rng.integers(-len(read) - 2, len(seq) + 3))
        for i in range(len(read)):  # mostly what the text holds there, so that segments form
            if 0 <= d + i < len(seq) and rng.random() < .7:
                read[i] = seq[d + i]
            if rng.random() < .05:
                read[i] = b"Nacgt*"[int(rng.integers(0, 6))]
        for penalty in (1, 4, 1 << 20):
            v = V.verify_one(bytes(read), seq, d, penalty)
            assert R.score_diag(bytes(read), seq, d, penalty) == (v["seg_score"], v["matches"])
            n += v["seg_score"] > 1
    assert n > 300


def test_the_best_diagonal_and_its_tie_rule_by_hand():
    #            0         1         2         3
    #            0123456789012345678901234567890123456789
    fwd = b"TTTTTTTTTTACGTACGTAAGGTTTTTTTTTTACGTACGTAAGGTTTTTTTTTT"
    seqs = [fwd, fwd]  # (not reverse complements: the emulator takes any twin of the same length)
    read = b"ACGTACGTAAGG"
    mate = [cand(0, 0, 40), cand(0, 1, 40), cand(0, 2, 39)]  # anchors 0 and 1 tie; the windows are L - diag - [0, 60]
    rec = R.rescue_read(seqs, read, 0, mate, 0, 0, 60, 4, 12, 8)
    # both windows hold both copies (diagonals 10 and 32): the best is found four times, the smallest anchor and then the smallest d win
    assert (rec["seq"], rec["diag"], rec["anchor"], rec["n_anchors"], rec["seg_score"], rec["matches"], rec["n_best"], rec["flags"]) == (1, 10, 0, 2, 12, 12, 4, R.TARGET | R.RESCUED)
    assert rec["n_diags"] == sum(hi - lo + 1 for lo, hi in (R.window(54, 12, 0, 0, 60), R.window(54, 12, 1, 0, 60))) == 60 + 61  # d in [-6, 53] and in [-7, 53]
    assert rec["next_score"] == 6
    assert R.rescue_read(seqs, read, 0, mate, 0, 0, 60, 4, 12, 1)["n_best"] == 2
    assert R.rescue_read(seqs, read, 0, mate, 0, 0, 60, 4, 13, 8)["flags"] == R.TARGET
    assert R.rescue_read(seqs, read, 0, mate, 0, 0, 60, 4, 12, 8, "tie_large_d")["diag"] == 32
    assert R.rescue_read(seqs, read, 0, mate, 0, 0, 60, 4, 12, 8, "gt_min")["flags"] == R.TARGET
    assert R.rescue_read(seqs, read, 0, mate, 0, 0, 60, 4, 12, 8, "all_anchors")["n_anchors"] == 3
    # a window that holds the second copy alone: L - diag - d in [0, 25] around the anchor at diag 0 is d in [29, 53]
    rec = R.rescue_read(seqs, read, 0, mate, 0, 0, 25, 4, 12, 1)
    assert (rec["diag"], rec["n_diags"], rec["n_best"]) == (32, 25, 1)
    # no candidate of the mate: no target; 64 of the read's own: FULL
    none = R.rescue_read(seqs, read, 0, [], 0, 0, 60, 4, 12, 8)
    assert (none["flags"], none["seq"], none["n_diags"]) == (0, R.NO_SEQUENCE, 0)
    full = R.rescue_read(seqs, read, 64, mate, 0, 0, 60, 4, 12, 8)
    assert (full["flags"], full["seq"], full["n_anchors"]) == (R.FULL, R.NO_SEQUENCE, 0)
    assert R.rescue_read(seqs, read, 63, mate, 0, 0, 60, 4, 12, 8)["flags"] == R.TARGET | R.RESCUED
    # an empty read: a target whose tasks are empty
    empty = R.rescue_read(seqs, b"", 0, mate, 0, 0, 60, 4, 12, 8)
    assert (empty["flags"], empty["seq"], empty["n_diags"], empty["n_anchors"]) == (R.TARGET, R.NO_SEQUENCE, 0, 2)


def test_merge_by_hand():
    fwd = b"TTTTTTTTTTACGTACGTAAGGTTTTTTTTTTCCCCCCCCCCCCCCCCCCCCCC"
    seqs = [fwd, fwd]
    reads = [b"ACGTACGTAAGG", b"CCCCCCCCCCCC"]
    lst = V.read_verify(seqs, reads, [[], [(0, 32), (0, 33)]], 4)
    res = R.read_rescue(seqs, reads, lst["cand_offsets"], lst["cands"], 0, 60, 4, 12, 2, R.MERGE)
    assert (res["n_targets"], res["n_rescued"], res["n_full"], res["n_tasks"]) == (1, 1, 0, 2) and list(res["cand_offsets"]) == [0, 1, 3]
    new = res["cands"][0]
    assert (int(new["seq"]), int(new["diag"]), int(new["n_cand"]), int(new["cand_index"]), int(new["n_tied"]), int(new["seg_score"]), int(new["span_hi"])) == (1, 10, 0, 0, 0, 12, 12)
    assert res["cands"][1:].tobytes() == lst["cands"].tobytes() and res["winners"][1].tobytes() == lst["reads"][1].tobytes()
    w = res["winners"][0]
    assert (int(w["seq"]), int(w["diag"]), int(w["n_cand"]), int(w["cand_index"]), int(w["n_tied"])) == (1, 10, 1, 0, 1)
    plain = R.read_rescue(seqs, reads, lst["cand_offsets"], lst["cands"], 0, 60, 4, 12, 2)
    assert plain["cands"] is None and plain["winners"] is None and plain["reads"].tobytes() == res["reads"].tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# the library's surface
def test_record_layouts_and_constants():
    d = P.RESCUE_DTYPE
    assert d.itemsize == 64 and d == R.RESCUE_DTYPE
    want = dict(diag=0, n_diags=8, seq=16, flags=20, anchor=24, n_anchors=28, seg_score=32, matches=36, n_best=40, next_score=44, reserved=48)
    assert {n: d.fields[n][1] for n in d.names} == want
    assert ctypes.sizeof(P.ReadRescueResult) == 96
    offs = {n: getattr(P.ReadRescueResult, n).offset for n, _ in P.ReadRescueResult._fields_}
    assert offs == dict(n_reads=0, n_targets=8, n_rescued=16, n_full=24, n_tasks=32, n_diags=40, frag_min=48, frag_max=56, min_score=64, max_anchors=68, flags=72,
                        mismatch_penalty=76, reads=80, ms_rescue=88, reserved=92)
    header = open(os.path.join(ROOT, "include", "pgx.h")).read()
    assert re.search(r"int64_t\s+diag;\s*uint64_t\s+n_diags;\s*uint32_t\s+seq,\s*flags,\s*anchor,\s*n_anchors,\s*seg_score,\s*matches,\s*n_best,\s*next_score,"
                     r"\s*reserved\[4\];\s*\}\s*pgx_read_rescue;", header)
    for name, value in (("MERGE", P.RESCUE_MERGE), ("TARGET", R.TARGET), ("RESCUED", R.RESCUED), ("FULL", R.FULL), ("MAX_ANCHORS", R.MAX_ANCHORS),
                        ("MAX_WINDOW", R.MAX_WINDOW)):
        m = re.search(r"^#define\s+PGX_RESCUE_%s\s+(\d+)u?" % name, header, re.M)
        assert m and int(m.group(1)) == value, name
    assert (P.RESCUE_MERGE, P.RESCUE_TARGET, P.RESCUE_RESCUED, P.RESCUE_FULL, P.RESCUE_MAX_ANCHORS, P.RESCUE_MAX_WINDOW) == (1, 1, 2, 4, 8, 65536)
    assert R.MAX_CAND == int(re.search(r"^#define\s+PGX_VERIFY_MAX_CAND\s+(\d+)u", header, re.M).group(1))


def test_symbols_are_exported_and_the_abi_version_stays(built):
    L = P.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    header = open(os.path.join(ROOT, "include", "pgx.h")).read()
    assert L.pgx_abi_version() == int(re.search(r"^#define\s+PGX_ABI_VERSION\s+(\d+)", header, re.M).group(1)) == 7


def test_no_device(built):
    try:
        none = P.device_count() == 0
    except P.PgxError as e:
        none = e.code == P.ERR_NO_DEVICE
    if not none:
        pytest.skip("a GPU is present")
    L = P.lib()
    with pytest.raises(P.PgxError) as e:
        P.read_rescue_arrays(0, np.zeros(0, np.uint8), [0, 0, 0], np.zeros(0, np.uint8), [0, 0, 0], [0, 0, 0], np.zeros(0, P.VERIFY_DTYPE), 0, 500)
    assert e.value.code == P.ERR_NO_DEVICE
    assert L.pgx_batch_read_rescue(None, 0, 500, 12, 2, 0, None) == P.ERR_NO_DEVICE
    out = P.ReadRescueResult()
    assert L.pgx_batch_rescued(None, ctypes.byref(out)) == P.ERR_ARG and L.pgx_batch_device_rescued(None, ctypes.byref(out)) == P.ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table
def test_the_collection_and_the_pinned_counts():
    assert C.lens[0::2] == C.lens[1::2] == [1200, 1500, 900, 2000, 700, 64] and M.is_twinned(C.lens) is None
    assert all(C.seqs[q + 1] == RC.rc(C.seqs[q]) for q in range(0, 12, 2))
    t0, t1 = C.tandem(8)
    assert C.seqs[8][t0:t1] == b"ACGTT" * 16 and C.seqs[9][C.tandem(9)[0]:C.tandem(9)[1]] == RC.rc(b"ACGTT" * 16)
    kinds = {k: C.kinds.count(k) for k in set(C.kinds)}
    assert kinds == RC.KIND_COUNTS and all(v >= 10 for v in kinds.values()) and len(C.pairs) == 94 and len(C.reads) == 188
    assert all(len(r) == 50 for r in C.reads)
    for p in C.pairs:
        if p["mate"] is None:
            continue
        read, (q, d) = (p["a"], p["truth_a"]) if p["mate"] == "a" else (p["b"], p["truth_b"])
        _, _, m = V.match_string(read, C.seqs[q], d)
        assert V.longest_run(m)[0] < RC.MIN_LEN, p["kind"]                                       # no exact run of min_len at the truth ...
        assert all(read[i:i + RC.MIN_LEN] not in C.raw for i in range(len(read) - RC.MIN_LEN + 1))  # ... nor anywhere else
    assert sorted(-min(p["truth_a"][1], p["truth_b"][1]) for p in C.pairs if p["kind"] == "edge") == sorted(RC.HANGS * 4)
    assert sorted(p["frag"] for p in C.pairs if p["kind"] == "dense")[:2] == [150, 150] and sum(p["frag"] == 500 for p in C.pairs if p["kind"] == "dense") == 2
    assert sorted(p["score"] for p in C.pairs if p["kind"] == "threshold") == [11] * 5 + [12] * 5
    assert all(len(p["ties"]) == 7 and p["ties"][2] == p["truth_a"][1] for p in C.pairs if p["kind"] == "tandem")


@pytest.fixture(scope="module")
def chain(workdir):
    """the verify list of every read at max_cand 16, penalty 4, from the oracle's MEMs, located, through place_emu and verify_emu"""
    path = os.path.join(workdir, "rescue_cases.txt")
    with open(path, "wb") as f:
        f.write(C.raw)
    ri = W.build_index_from_text(path, workdir, "rescue_cases", with_tags=False)[0]
    orc = O.RIndex(ri)
    L = int(P.Index(ri, mode=P.MODE_STRICT).info().max_length)
    mems, mem_off, values, loc_off = [], [0], [], [0]
    for read in C.reads:
        for m in orc.find_all_mems(read, RC.MIN_LEN, 1, O.MODE_STRICT):
            mems.append(m)
            values += [int(v) for v in orc.locate_sa(m[2], m[2] + m[3] - 1, O.MODE_STRICT)]
            loc_off.append(len(values))
        mem_off.append(len(mems))
    marr = np.zeros(len(mems), E.MEM_DTYPE)
    for k, m in enumerate(mems):
        marr[k] = m
    place = E.read_place(np.array(mem_off, np.uint64), marr, np.array(loc_off, np.uint64), np.array(values, np.uint64), L)
    return V.read_verify(C.seqs, C.reads, V.candidates_from_places(place, 16), RC.PENALTY)


@pytest.fixture(scope="module")
def rescued(chain):
    return R.read_rescue(C.seqs, C.reads, chain["cand_offsets"], chain["cands"], RC.FRAG_MIN, RC.FRAG_MAX, RC.PENALTY, RC.MIN_LEN, 2, R.MERGE)


def _mate(k):
    """(read number, truth) of the mate to rescue of pair k"""
    p = C.pairs[k]
    return (2 * k, p["truth_a"]) if p["mate"] == "a" else (2 * k + 1, p["truth_b"])


def _at(rec):
    return None if int(rec["seq"]) == R.NO_SEQUENCE else (int(rec["seq"]), int(rec["diag"]))


def test_every_dense_mate_is_rescued_to_its_truth_and_every_random_one_is_left(chain, rescued):
    n_cands = np.diff(chain["cand_offsets"].astype(np.int64))
    recs = rescued["reads"]
    n = 0
    for k, p in enumerate(C.pairs):
        if p["kind"] in RESCUED_KINDS:
            r, truth = _mate(k)
            assert n_cands[r] == 0 and int(chain["reads"][r]["seq"]) == V.NO_SEQUENCE, (k, p["kind"])  # nothing before ...
            assert int(recs[r]["flags"]) == R.TARGET | R.RESCUED and _at(recs[r]) == truth, (k, p["kind"])  # ... and exactly the truth after
            assert int(recs[r]["n_best"]) == 1 and int(recs[r]["next_score"]) < RC.MIN_LEN <= int(recs[r]["seg_score"])
            assert int(recs[r ^ 1]["flags"]) == 0 and n_cands[r ^ 1] == (2 if p["kind"] == "repeat_anchor" else 1)
            if p["kind"] == "repeat_anchor":
                assert (int(recs[r]["anchor"]), int(recs[r]["n_anchors"])) == (1, 2)
            if p["kind"] == "edge":  # the window is clipped: fewer than the 501 diagonals of the bounds
                assert 0 < int(recs[r]["n_diags"]) < 501 and truth[1] < 0
            n += 1
        elif p["kind"] == "junk":
            r = 2 * k + 1
            assert n_cands[r] == 0 and int(recs[r]["flags"]) == R.TARGET and 0 < int(recs[r]["seg_score"]) < RC.MIN_LEN and int(recs[r]["n_diags"]) > 0
        elif p["kind"] == "threshold":
            r, truth = _mate(k)
            assert _at(recs[r]) == truth and int(recs[r]["seg_score"]) == p["score"] and int(recs[r]["n_best"]) == 1
            assert int(recs[r]["flags"]) == R.TARGET | (R.RESCUED if p["score"] >= RC.MIN_LEN else 0)
        elif p["kind"] == "tandem":
            r, truth = _mate(k)
            assert _at(recs[r]) == (truth[0], p["ties"][0]) and int(recs[r]["n_best"]) == 7 and int(recs[r]["flags"]) == R.TARGET | R.RESCUED
        elif p["kind"] == "both":
            assert [int(recs[r]["flags"]) for r in (2 * k, 2 * k + 1)] == [R.TARGET, R.TARGET] and list(n_cands[2 * k:2 * k + 2]) == [1, 1]
        else:
            assert p["kind"] == "proper" and [int(recs[r]["flags"]) for r in (2 * k, 2 * k + 1)] == [0, 0]
    assert n == 44
    assert (rescued["n_targets"], rescued["n_rescued"], rescued["n_full"], rescued["n_tasks"], rescued["n_diags"]) == (94, 59, 0, 104, COUNT_DIAGS)
    # with one anchor the mates behind the second copy are searched for around the first: none of them is found
    one = R.read_rescue(C.seqs, C.reads, chain["cand_offsets"], chain["cands"], RC.FRAG_MIN, RC.FRAG_MAX, RC.PENALTY, RC.MIN_LEN, 1)["reads"]
    assert all(not int(one[_mate(k)[0]]["flags"]) & R.RESCUED for k, p in enumerate(C.pairs) if p["kind"] == "repeat_anchor")


COUNT_DIAGS = 45905


def test_after_merge_and_mates_every_rescued_pair_is_proper(chain, rescued):
    offs, lst = rescued["cand_offsets"], rescued["cands"]
    assert int(offs[-1]) == int(chain["cand_offsets"][-1]) + 59 == len(lst)
    before = M.read_mates(C.lens, chain["cand_offsets"], chain["cands"], RC.FRAG_MIN, RC.FRAG_MAX, 10, M.ELECT)
    after = M.read_mates(C.lens, offs, lst, RC.FRAG_MIN, RC.FRAG_MAX, 10, M.ELECT)
    for k, p in enumerate(C.pairs):
        proper = bool(int(after["pairs"][k]["flags"]) & M.PROPER)
        if p["kind"] in RESCUED_KINDS + ("tandem",) or p.get("score") == 12:
            r, truth = _mate(k)
            want = (truth[0], p["ties"][0]) if p["kind"] == "tandem" else truth
            assert proper and not int(before["pairs"][k]["flags"]) & M.PROPER, (k, p["kind"])
            assert _at(after["winners"][r]) == want and _at(rescued["winners"][r]) == want and _at(before["winners"][r]) is None
            assert _at(after["winners"][r ^ 1]) == (p["truth_b"] if p["mate"] == "a" else p["truth_a"])
            assert int(after["pairs"][k]["frag"]) == p["frag"] + (want[1] - truth[1]) * (-1)
            # the appended record: the last of its list, what verify writes there
            c = lst[int(offs[r + 1]) - 1]
            v = V.verify_one(C.reads[r], C.seqs[want[0]], want[1], RC.PENALTY)
            assert all(int(c[f]) == v[f] for f in v) and (int(c["n_cand"]), int(c["cand_index"]), int(c["n_tied"])) == (0, 0, 0)
        elif p["kind"] == "proper":
            assert proper and after["pairs"][k].tobytes() == before["pairs"][k].tobytes()
        else:
            assert not proper and after["pairs"][k].tobytes() == before["pairs"][k].tobytes(), (k, p["kind"])
    assert after["n_proper"] == before["n_proper"] + 59 == 69


# ---------------------------------------------------------------------------------------------------------------------------------
# mutations of the emulator: each changes records of the class it targets
MUTATION_COUNTS = {  # mutation -> (frag_min, max_anchors, class, reads of the class whose record or merged list changes)
    "win_lo": (150, 2, "dense", 2),            # the window ends one short of frag_max: the two mates at exactly 500 are lost (every n_diags changes: see below)
    "win_hi": (150, 2, "dense", 2),            # ... one short of frag_min: the two mates at exactly 150
    "clip_lo": (0, 2, "edge", 12),             # the clip at the start one diagonal short: every clipped window loses one
    "clip_hi": (0, 2, "edge", 6),              # ... at the end: the windows on the sequences of 64, which reach both ends
    "tie_large_d": (0, 2, "tandem", 10),       # ties to the largest d: the last of the seven diagonals
    "all_anchors": (0, 2, "tandem", 10),       # a weaker candidate of the placed mate becomes an anchor too: its diagonals are counted; see below
    "gt_min": (0, 2, "threshold", 5),          # > at min_score: the mates at exactly min_score
    "merge_first": (0, 2, "tandem", 10),       # the rescued candidate put first: the list of every rescued read with a candidate of its own changes; see below
}


@pytest.mark.parametrize("mutation", list(MUTATION_COUNTS))
def test_each_mutation_changes_its_class(chain, mutation):
    frag_min, anchors, kind, count = MUTATION_COUNTS[mutation]
    offs, lst, reads = chain["cand_offsets"], chain["cands"], list(C.reads)
    if mutation in ("all_anchors", "merge_first"):
        # give the placed mate of every tandem pair a second, weaker candidate 400 diagonals on (all_anchors searches around it too, and finds nothing
        # more but counts its diagonals), and the tandem mate a candidate of its own far away (merge_first puts the rescued one before it)
        new, noffs = [], [0]
        for r in range(len(reads)):
            mine = list(lst[int(offs[r]):int(offs[r + 1])])
            if C.kinds[r // 2] == "tandem":
                extra = (mine[0] if mine else lst[int(offs[r ^ 1])]).copy()
                extra["diag"] = int(extra["diag"]) + 400 if mine else 5000
                extra["seq"] ^= 0 if mine else 1
                extra["seg_score"], extra["matches"], extra["n_cand"], extra["cand_index"] = 13, 13, len(mine), len(mine)
                mine.append(extra)
            new += mine
            noffs.append(len(new))
        lst, offs = np.array(new, dtype=V.VERIFY_DTYPE), np.array(noffs, np.uint64)
    run = lambda m: R.read_rescue(C.seqs, reads, offs, lst, frag_min, RC.FRAG_MAX, RC.PENALTY, RC.MIN_LEN, anchors, R.MERGE, mutation=m)
    good, bad = run(None), run(mutation)
    if mutation in ("win_lo", "win_hi"):  # (n_diags changes wherever the clip does not hide the bound: what is counted here is a mate lost)
        changed = [r for r in range(len(reads)) if (int(good["reads"][r]["flags"]) ^ int(bad["reads"][r]["flags"])) & R.RESCUED and C.kinds[r // 2] == kind]
    else:
        lists = lambda res, r: res["cands"][int(res["cand_offsets"][r]):int(res["cand_offsets"][r + 1])].tobytes()
        changed = [r for r in range(len(reads)) if (good["reads"][r] != bad["reads"][r] or lists(good, r) != lists(bad, r)) and C.kinds[r // 2] == kind]
    print("%s: %d reads of class %s change" % (mutation, len(changed), kind))
    assert len(changed) == count > 0
