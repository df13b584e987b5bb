"""CPU tier of read verify: tests/verify_emu.py (the definitions of include/pgx.h "read verify" in plain Python) against cases worked out by
hand, and its quadratic segment search against a linear scan with the stated tie rule."""
import numpy as np
import pytest

import verify_emu as E


def _m(s):
    return [c == "M" for c in s]


def kadane(m, penalty):
    """the segment of largest score in one pass: a segment that ends at i is extended while its score is >= 0 (an equal score with a smaller
    start wins), and the best is replaced only by a strictly larger score (the start never moves back: the first to reach a score has the
    smallest start, then the smallest end)"""
    best = (0, 0, 0, 0)
    cur, start, mm = -1, 0, 0
    for i, x in enumerate(m):
        if cur < 0:
            cur, start, mm = 0, i, 0
        if x:
            cur += 1
        else:
            cur -= penalty
            mm += 1
        if cur > best[0]:
            best = (cur, start, i + 1, mm)
    return best


def test_segment_by_hand():
    assert E.best_segment_quadratic(_m(""), 4) == (0, 0, 0, 0)
    assert E.best_segment_quadratic(_m("XXX"), 4) == (0, 0, 0, 0)
    assert E.best_segment_quadratic(_m("MMMM"), 4) == (4, 0, 4, 0)  # the whole span
    assert E.best_segment_quadratic(_m("MMXMM"), 4) == (2, 0, 2, 0)  # two equal segments: the first
    assert E.best_segment_quadratic(_m("MMXMMM"), 4) == (3, 3, 6, 0)
    assert E.best_segment_quadratic(_m("MMMMMXMMMMM"), 4) == (6, 0, 11, 1)  # crossing pays
    assert E.best_segment_quadratic(_m("MMMMXMMMM"), 4) == (4, 0, 4, 0)  # crossing ties with stopping: the smallest end
    assert E.best_segment_quadratic(_m("MXM"), 1) == (1, 0, 1, 0)  # P = 1: a mismatch and a match tie with stopping earlier
    assert E.best_segment_quadratic(_m("MXMM"), 1) == (2, 0, 4, 1)  # ... and an equal score from the smaller start wins over [2, 4)
    assert E.best_segment_quadratic(_m("XMX"), 7) == (1, 1, 2, 0)


def test_runs_by_hand():
    assert E.longest_run(_m("")) == (0, 0)
    assert E.longest_run(_m("XX")) == (0, 0)
    assert E.longest_run(_m("MMXMM")) == (2, 0)
    assert E.longest_run(_m("MXMMXMM")) == (2, 2)
    assert E.longest_run(_m("XMMM")) == (3, 1)


def test_candidate_by_hand():
    seq = b"ACGTNACGTA"
    v = E.verify_one(b"ACGTNACG", seq, 0, 4)  # N opposite N is a mismatch
    assert (v["span_lo"], v["span_hi"], v["matches"], v["mismatches"]) == (0, 8, 7, 1)
    assert (v["seg_start"], v["seg_end"], v["seg_score"], v["seg_mismatches"], v["longest_run"], v["run_start"]) == (0, 4, 4, 0, 4, 0)
    v = E.verify_one(b"acgtACGTA", seq, -4, 4)  # overhang at the start; lower case never matches (it is outside the span here)
    assert (v["span_lo"], v["span_hi"], v["matches"], v["mismatches"]) == (4, 9, 4, 1)
    assert (v["seg_start"], v["seg_end"], v["seg_score"], v["run_start"]) == (4, 8, 4, 4)
    v = E.verify_one(b"GTAAAA", seq, 7, 4)  # overhang at the end
    assert (v["span_lo"], v["span_hi"], v["matches"], v["mismatches"]) == (0, 3, 3, 0)
    v = E.verify_one(b"ACGT", seq, 10, 4)  # no overlap
    assert all(v[k] == 0 for k in v if k != "diag") and v["diag"] == 10
    v = E.verify_one(b"ACGT", seq, -4, 4)
    assert all(v[k] == 0 for k in v if k != "diag")
    v = E.verify_one(b"TTTT", b"AAAA", 0, 4)  # nothing matches: the empty segment at lo
    assert (v["matches"], v["mismatches"], v["seg_start"], v["seg_end"], v["seg_score"], v["longest_run"], v["run_start"]) == (0, 4, 0, 0, 0, 0, 0)
    v = E.verify_one(b"xxTTTT", b"AAAA", -2, 4)
    assert (v["span_lo"], v["span_hi"], v["seg_start"], v["seg_end"]) == (2, 6, 2, 2)
    v = E.verify_one(b"AaA", b"AAA", 0, 4)  # lower case in the span
    assert (v["matches"], v["mismatches"]) == (2, 1)


def test_winner_by_hand():
    seqs = [b"ACGTACGTAC", b"ACGTACGAAC", b"ACGTACGTAC"]
    res = E.read_verify(seqs, [b"ACGTACGT", b"", b"GGGG"], [[(1, 0), (0, 0), (2, 0)], [], [(0, 0)]], 4)
    assert res["cand_offsets"].tolist() == [0, 3, 3, 4] and res["reads"].dtype.itemsize == 64
    r0 = res["reads"][0]
    assert (r0["seq"], r0["cand_index"], r0["n_cand"], r0["n_tied"], r0["seg_score"], r0["matches"]) == (0, 1, 3, 2, 8, 8)
    assert res["cands"]["n_cand"].tolist() == [0, 1, 2, 0] and res["cands"]["n_tied"].tolist() == [0, 0, 0, 0]
    r1 = res["reads"][1]
    assert r1["seq"] == E.NO_SEQUENCE and all(int(r1[f]) == 0 for f in E.VERIFY_DTYPE.names if f != "seq")
    r2 = res["reads"][2]
    assert (r2["seq"], r2["n_cand"], r2["n_tied"], r2["matches"], r2["mismatches"], r2["seg_score"]) == (0, 1, 1, 1, 3, 1)
    # the same score with fewer matches loses; equal in both: the first
    res = E.read_verify([b"AAAAAAAACC", b"AAAAAAAACA", b"AAAAAAAACA"], [b"AAAAAAAAAA"], [[(0, 0), (1, 0), (2, 0)]], 4)
    assert res["cands"]["seg_score"].tolist() == [8, 8, 8] and res["cands"]["matches"].tolist() == [8, 9, 9]
    assert (res["reads"][0]["cand_index"], res["reads"][0]["n_tied"], res["reads"][0]["seq"]) == (1, 2, 1)


@pytest.mark.parametrize("penalty", [1, 2, 4, 7])
def test_quadratic_equals_kadane(penalty):
    rng = np.random.default_rng(penalty)
    for length in range(0, 41):
        for trial in range(30):
            p_match = (0.1, 0.5, 0.9)[trial % 3]
            m = (rng.random(length) < p_match).tolist()
            assert E.best_segment_quadratic(m, penalty) == kadane(m, penalty), (m, penalty)
