"""GPU tier of the read mates kernel on stated lists: pgx_read_mates_arrays against tests/mates_emu.py byte for byte, records and (with
PGX_MATES_ELECT) winner records, on the shapes no index produces: every candidate count from none to 64 a mate, every group width from 1 to
64 lanes, pair counts at the wave and grid borders, frag at both bounds, ties at every level of the order, the PROPER threshold, score sums
near 2^32, the last twin.  Every candidate carries distinct bytes in the fields the stage only copies, so that an election that copies the
wrong record, or the right one to the wrong place, shows.  Every refusal leaves pre-filled outputs untouched."""
import numpy as np
import pytest

import mates_emu as M
import pgx_ffi as P

pytestmark = pytest.mark.gpu

LENS = [1000, 1000, 500, 500, 64, 64]
COPIED = ("span_lo", "span_hi", "mismatches", "seg_start", "seg_end", "seg_mismatches", "longest_run", "run_start")


def lists_to_arrays(lists):
    """per read a list of (seq, diag, seg_score, matches) -> cand_offsets, cands; the other fields hold a running number"""
    offs = np.zeros(len(lists) + 1, np.uint64)
    offs[1:] = np.cumsum([len(x) for x in lists])
    cands = np.zeros(int(offs[-1]), M.VERIFY_DTYPE)
    at = 0
    for mine in lists:
        for k, (q, diag, score, matches) in enumerate(mine):
            c = cands[at]
            c["seq"], c["diag"], c["seg_score"], c["matches"], c["n_cand"], c["cand_index"] = q, diag, score, matches, k, k
            for n, f in enumerate(COPIED):
                c[f] = (at * 8 + n) & 0xFFFFFFFF
            at += 1
    return offs, cands


def check(lists, fmin, fmax, penalty, lens=LENS):
    """both flag values against the emulator; returns the emulator's result with ELECT"""
    offs, cands = lists_to_arrays(lists)
    for flags in (0, P.MATES_ELECT):
        exp = M.read_mates(lens, offs, cands, fmin, fmax, penalty, flags)
        got = P.read_mates_arrays(0, lens, offs, cands, fmin, fmax, penalty, flags)
        bad = np.flatnonzero(got["pairs"] != exp["pairs"])
        assert len(bad) == 0, (flags, len(bad), int(bad[0]), got["pairs"][bad[0]], exp["pairs"][bad[0]])
        assert got["pairs"].tobytes() == exp["pairs"].tobytes()
        if flags:
            bad = np.flatnonzero(got["winners"] != exp["winners"])
            assert len(bad) == 0, (len(bad), int(bad[0]), got["winners"][bad[0]], exp["winners"][bad[0]])
            assert got["winners"].tobytes() == exp["winners"].tobytes()
        else:
            assert got["winners"] is None
    return exp


def random_pair(rng, na, nb, lens=LENS):
    """the two lists of a pair: candidates on both strands of one path mostly, diagonals that put a fair share of the fragments inside [0, 500]"""
    p = int(rng.integers(0, len(lens) // 2))
    out = []
    for n in (na, nb):
        mine = []
        for _ in range(n):
            q = 2 * p + int(rng.integers(0, 2)) if rng.random() < 0.85 else int(rng.integers(0, len(lens)))
            mine.append((q, int(rng.integers(-40, lens[q] // 2 + 40)), int(rng.integers(0, 4)) * 10 + 20, int(rng.integers(0, 3)) + 40))
        out.append(mine)
    return out


def test_every_candidate_count_in_every_combination():
    rng = np.random.default_rng(9101)
    counts = (0, 1, 2, 3, 63, 64)
    lists = []
    for na in counts:
        for nb in counts:
            lists += random_pair(rng, na, nb)
    exp = check(lists, 0, 500, 25)
    fl = exp["pairs"]["flags"]
    assert len(fl) == 36 and ((fl & M.COMPATIBLE) != 0).sum() >= 10 and ((fl & M.MOVED_A) != 0).sum() >= 3 and ((fl & M.MOVED_B) != 0).sum() >= 3
    assert exp["pairs"]["n_best"].max() > 1 and (exp["pairs"]["next_score"] > 0).any()
    for na in (0, 1, 64):  # and each corner in a call of its own: the group width follows the longest list of the call
        for nb in (0, 1, 64):
            check(random_pair(rng, na, nb) + random_pair(rng, nb, na), 0, 500, 25)


@pytest.mark.parametrize("largest", (1, 2, 3, 4, 5, 8, 9, 33, 64))
def test_every_group_width(largest):
    rng = np.random.default_rng(9200 + largest)
    lists = []
    for k in range(80 if largest < 33 else 24):
        na, nb = (largest, largest) if k == 5 else (int(rng.integers(0, largest + 1)), int(rng.integers(0, largest + 1)))
        lists += random_pair(rng, na, nb)
    exp = check(lists, 0, 500, 25)
    assert exp["n_compatible"] >= 5


@pytest.mark.parametrize("width", (1, 4, 64))
def test_pair_counts_at_wave_and_grid_borders(width):
    """a wave holds 64 / width pairs and a workgroup 256 / width: the pair counts around both, and 1, 63, 64, 65 whatever the width"""
    rng = np.random.default_rng(9300 + width)
    period = 211 if width < 64 else 23  # divides no border
    base = []
    for k in range(period):
        base += random_pair(rng, int(rng.integers(0, width + 1)), int(rng.integers(0, width + 1)))
    base[0:2] = random_pair(rng, width, width)
    per_wave, per_group = 64 // width, 256 // width
    counts = sorted({1, 63, 64, 65} | {x + d for x in (per_wave, per_group) for d in (-1, 0, 1) if x + d > 0})
    offs1, cands1 = lists_to_arrays(base)
    exp1 = M.read_mates(LENS, offs1, cands1, 0, 500, 25, M.ELECT)  # the emulator runs on one period
    for n_pairs in counts:
        reps = n_pairs // period + 1
        offs, cands = lists_to_arrays((base * reps)[:2 * n_pairs])
        for n, f in enumerate(COPIED):  # (the copied fields repeat with the period, as the expectation does)
            cands[f] = np.tile(cands1[f], reps)[:len(cands)]
        got = P.read_mates_arrays(0, LENS, offs, cands, 0, 500, 25, P.MATES_ELECT)
        assert got["pairs"].tobytes() == np.tile(exp1["pairs"], reps)[:n_pairs].tobytes(), n_pairs
        assert got["winners"].tobytes() == np.tile(exp1["winners"], reps)[:2 * n_pairs].tobytes(), n_pairs
    if width == 64:
        return
    # 70 001 pairs: the period repeated; the emulator runs on one period
    n_pairs = 70001
    reps = n_pairs // period + 1
    per = int(offs1[-1])
    offs = np.concatenate([[0], (offs1[1:][None, :] + (np.arange(reps, dtype=np.uint64) * np.uint64(per))[:, None]).ravel()]).astype(np.uint64)[:2 * n_pairs + 1]
    cands = np.tile(cands1, reps)[:int(offs[-1])]
    got = P.read_mates_arrays(0, LENS, offs, cands, 0, 500, 25, P.MATES_ELECT)
    assert got["pairs"].tobytes() == np.tile(exp1["pairs"], reps)[:n_pairs].tobytes()
    assert got["winners"].tobytes() == np.tile(exp1["winners"], reps)[:2 * n_pairs].tobytes()


def test_frag_at_both_bounds_and_off_the_sequence():
    # L = 1000, A at diag 100: frag = 900 - diag_b
    lists = []
    for frag in (149, 150, 500, 501):
        lists += [[(0, 100, 50, 50)], [(1, 900 - frag, 50, 50)]]
    exp = check(lists, 150, 500, 8)
    assert [int(f) & M.COMPATIBLE for f in exp["pairs"]["flags"]] == [0, M.COMPATIBLE, M.COMPATIBLE, 0]
    assert [int(x) for x in exp["pairs"]["frag"]] == [0, 150, 500, 0]
    # one value only
    exp = check(lists, 500, 500, 8)
    assert [int(f) & M.COMPATIBLE for f in exp["pairs"]["flags"]] == [0, 0, M.COMPATIBLE, 0]
    # negative diagonals (a read that hangs over the start) and diagonals beyond L; a negative frag with bounds that admit it
    lists = [[(0, -31, 40, 40)], [(1, 700, 40, 40)],      # frag 331
             [(0, 990, 40, 40)], [(1, -7, 40, 40)],       # frag 17
             [(0, 1200, 40, 40)], [(1, 10, 40, 40)],      # frag -210
             [(2, 499, 40, 40)], [(3, 499, 40, 40)],      # frag -498
             [(3, -49, 40, 40)], [(2, -49, 40, 40)]]      # frag 598: both hang over
    exp = check(lists, 0, 500, 8)
    assert [int(f) & M.COMPATIBLE for f in exp["pairs"]["flags"]] == [M.COMPATIBLE, M.COMPATIBLE, 0, 0, 0]
    exp = check(lists, -498, -210, 8)
    assert [int(x) for x in exp["pairs"]["frag"]] == [0, 0, -210, -498, 0]
    exp = check(lists, -(2 ** 62), 2 ** 62, 8)
    assert [int(x) for x in exp["pairs"]["frag"]] == [331, 17, -210, -498, 598]


def test_all_4096_pairs_compatible_and_tied():
    lists = [[(4, 3, 30, 30)] * 64, [(5, 11, 30, 30)] * 64]  # the last twin, L = 64: frag 50
    exp = check(lists, 0, 500, 0)
    rec = exp["pairs"][0]
    assert (int(rec["n_compatible"]), int(rec["n_best"]), int(rec["cand_a"]), int(rec["cand_b"]), int(rec["frag"]), int(rec["next_score"])) == (4096, 4096, 0, 0, 50, 0)
    assert int(rec["flags"]) == M.PROPER | M.COMPATIBLE | M.HAS_A | M.HAS_B
    assert [int(x) for x in exp["winners"]["n_tied"]] == [64, 64]


def test_ties_are_broken_at_each_level_in_turn():
    b_at = lambda s, m: (1, 600, s, m)
    a_at = lambda s, m: (0, 100, s, m)
    cases = [
        ([a_at(40, 45), a_at(41, 40)], [b_at(40, 40), b_at(40, 41)], (1, 1)),  # the score sum decides, whatever the matches
        ([a_at(40, 40), a_at(40, 41)], [b_at(40, 41), b_at(40, 40)], (1, 0)),  # then the matches sum
        ([a_at(40, 40), a_at(40, 40)], [b_at(39, 40), b_at(40, 40), b_at(40, 40)], (0, 1)),  # then the smallest i, then the smallest j
    ]
    lists = []
    for a, b, _ in cases:
        lists += [a, b]
    exp = check(lists, 0, 500, 1000)
    assert [(int(r["cand_a"]), int(r["cand_b"])) for r in exp["pairs"]] == [c[2] for c in cases]
    assert [int(r["n_best"]) for r in exp["pairs"]] == [1, 1, 4]
    # (0, 1) and (1, 0) tie in both sums and are the only compatible pairs (frag 300; (0, 0) has 500, (1, 1) has 100): i decides before j
    exp = check([[(0, 100, 40, 40), (0, 300, 40, 40)], [(1, 400, 40, 40), (1, 600, 40, 40)]], 250, 350, 1000)
    rec = exp["pairs"][0]
    assert (int(rec["cand_a"]), int(rec["cand_b"]), int(rec["n_best"]), int(rec["n_compatible"])) == (0, 1, 2, 2)


def test_the_proper_threshold_and_the_penalty_range():
    # A's solo winner (60) is compatible with nothing, its second (50) pairs with B (40): pair 90, solo 100
    lists = [[(0, 900, 60, 60), (0, 100, 50, 50)], [(1, 600, 40, 40)]]
    for penalty, proper in ((10, True), (9, False), (0, False), (2 ** 32 - 1, True)):
        exp = check(lists, 0, 500, penalty)
        rec = exp["pairs"][0]
        assert (int(rec["pair_score"]), int(rec["solo_score"]), int(rec["n_compatible"])) == (90, 100, 1)
        assert bool(int(rec["flags"]) & M.PROPER) == proper and bool(int(rec["flags"]) & M.MOVED_A) == proper and not int(rec["flags"]) & M.MOVED_B
        assert (int(rec["cand_a"]), int(rec["solo_a"])) == ((1, 0) if proper else (0, 0))
        assert (int(exp["winners"][0]["diag"]), int(exp["winners"][0]["cand_index"]), int(exp["winners"][0]["n_cand"])) == ((100, 1, 2) if proper else (900, 0, 2))
    # U = 0 keeps a pair only when it is the solo winners themselves
    exp = check([[(0, 100, 50, 50)], [(1, 600, 40, 40)]], 0, 500, 0)
    assert int(exp["pairs"][0]["flags"]) == M.PROPER | M.COMPATIBLE | M.HAS_A | M.HAS_B


def test_zero_scores_and_sums_near_two_to_the_32():
    big = 2 ** 31
    lists = [[(0, 100, 0, 0), (0, 101, 0, 0)], [(1, 600, 0, 0)],                   # seg_score 0 everywhere: the pair scores 0, nothing is below it
             [(0, 100, big - 1, 7), (0, 101, big - 2, 7)], [(1, 600, big, 7)],       # 2^32 - 1 and 2^32 - 2: both fit
             [(0, 100, 2 ** 32 - 1, 2 ** 32 - 1), (0, 101, 5, 5)], [(1, 600, 2 ** 32 - 1, 2 ** 32 - 1)],  # 2^33 - 2: held at 2^32 - 1, compared in 64 bits
             [(0, 900, 2 ** 32 - 1, 1), (0, 100, 2 ** 32 - 2, 1)], [(1, 600, 2 ** 32 - 1, 1)]]             # pair 2^33 - 3 + U 1 >= solo 2^33 - 2 in 64 bits
    exp = check(lists, 0, 500, 1)
    p = exp["pairs"]
    assert (int(p[0]["pair_score"]), int(p[0]["n_best"]), int(p[0]["next_score"]), int(p[0]["flags"]) & M.PROPER) == (0, 2, 0, M.PROPER)
    assert (int(p[1]["pair_score"]), int(p[1]["next_score"])) == (2 ** 32 - 1, 2 ** 32 - 2)
    assert (int(p[2]["pair_score"]), int(p[2]["solo_score"]), int(p[2]["pair_matches"]), int(p[2]["next_score"])) == (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1)
    assert int(p[3]["flags"]) & (M.PROPER | M.MOVED_A) == M.PROPER | M.MOVED_A
    exp = check(lists, 0, 500, 0)
    assert not int(exp["pairs"][3]["flags"]) & M.PROPER


def test_the_same_result_under_forced_lanes(monkeypatch):
    rng = np.random.default_rng(9400)
    lists = []
    for k in range(70):
        lists += random_pair(rng, int(rng.integers(0, 4)), int(rng.integers(0, 4)))
    offs, cands = lists_to_arrays(lists)
    monkeypatch.delenv("PGX_MATES_LANES", raising=False)
    first = P.read_mates_arrays(0, LENS, offs, cands, 0, 500, 25, P.MATES_ELECT)
    for lanes in ("1", "2", "7", "8", "64", "65", "junk"):  # (1 and 2 are below what the lists need, 65 and junk are not lane counts: all ignored)
        monkeypatch.setenv("PGX_MATES_LANES", lanes)
        got = P.read_mates_arrays(0, LENS, offs, cands, 0, 500, 25, P.MATES_ELECT)
        assert got["pairs"].tobytes() == first["pairs"].tobytes() and got["winners"].tobytes() == first["winners"].tobytes(), lanes
    monkeypatch.setenv("PGX_MATES_LANES", "64")
    check(lists, 0, 500, 25)


def test_every_refusal_leaves_the_outputs_untouched():
    ok = [[(0, 100, 50, 50)], [(1, 600, 40, 40)], [], [(5, 3, 9, 9)]]
    offs, cands = lists_to_arrays(ok)
    big_offs, big_cands = lists_to_arrays([[(0, 1, 1, 1)] * 65, []])
    bad_seq = cands.copy()
    bad_seq[2]["seq"] = 6
    refusals = [
        (dict(lens=LENS[:5]), "odd"), (dict(lens=[1000, 999] + LENS[2:]), "p = 0"), (dict(lens=LENS[:4] + [64, 65]), "p = 2"),
        (dict(offs=np.array([1, 1, 2, 2, 3], np.uint64)), "start at 0"), (dict(offs=np.array([0, 2, 1, 2, 3], np.uint64)), "decrease at read 1"),
        (dict(offs=big_offs, cands=big_cands), "read 0 has 65 candidates"), (dict(cands=bad_seq), "read 3 has seq 6"),
        (dict(offs=offs[:4], n_reads=3), "odd"), (dict(fmin=501), "frag_min 501 exceeds frag_max 500"), (dict(flags=2), "unknown flag"),
    ]
    for kw, text in refusals:
        out = dict(pairs=np.full(8, 0xA5, np.uint8).repeat(64).view(M.MATES_DTYPE), winners=np.full(16, 0x5A, np.uint8).repeat(64).view(M.VERIFY_DTYPE))
        keep = out["pairs"].tobytes(), out["winners"].tobytes()
        with pytest.raises(P.PgxError) as e:
            P.read_mates_arrays(0, kw.get("lens", LENS), kw.get("offs", offs), kw.get("cands", cands), kw.get("fmin", 0), 500, 25, kw.get("flags", P.MATES_ELECT),
                                n_reads=kw.get("n_reads"), out=out)
        assert e.value.code == P.ERR_ARG and text in str(e.value), (kw.keys(), str(e.value))
        assert (out["pairs"].tobytes(), out["winners"].tobytes()) == keep
    got = P.read_mates_arrays(0, LENS, offs, cands, 0, 500, 25, P.MATES_ELECT)  # and the same arguments unbroken are served
    assert got["pairs"].tobytes() == M.read_mates(LENS, offs, cands, 0, 500, 25, M.ELECT)["pairs"].tobytes()
    empty = P.read_mates_arrays(0, LENS, np.zeros(1, np.uint64), np.zeros(0, M.VERIFY_DTYPE), 0, 500, 25, P.MATES_ELECT)
    assert len(empty["pairs"]) == 0 and len(empty["winners"]) == 0
