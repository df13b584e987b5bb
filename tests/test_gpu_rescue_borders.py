"""GPU tier of the read rescue kernels on stated lists: pgx_read_rescue_arrays against tests/rescue_emu.py byte for byte -- the records and, with
PGX_RESCUE_MERGE, the merged list, its offsets and the winners -- on the shapes no index produces: windows around the wave width, windows
clipped at either end of a sequence, on both and to nothing, read lengths around the 8-symbol word, every residue of the read's offset and
of the text position against that word, the first and the last symbol of the text, bytes that never match, empty sequences, anchors at and
beyond max_anchors, ties at every level of the order, min_score at the best score, both ends of the penalty range, every candidate count of
the target up to FULL, the mates kernel on a merged list, read counts at the wave and grid borders.  Every refusal leaves pre-filled outputs
untouched."""
import numpy as np
import pytest

import mates_emu as M
import pgx_ffi as P
import rescue_emu as R

pytestmark = pytest.mark.gpu

_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
rc = lambda s: bytes(s).translate(_COMP)[::-1]
COPIED = ("span_lo", "span_hi", "mismatches", "seg_start", "seg_end", "seg_mismatches", "longest_run", "run_start")


def collection(seed=77):
    """twins of 1500, 200 (a tandem repeat of period 7 inside, and three N), 0, 1 and 64 symbols: the first sequence starts the text, the last ends it"""
    rng = np.random.default_rng(seed)
    seqs = []
    for n in (1500, 200, 0, 1, 64):
        s = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes())
        if n == 200:
            s[20:174] = b"ACCGTGA" * 22
            s[5], s[100], s[190] = ord("N"), ord("N"), ord("N")
        seqs += [bytes(s), rc(s)]
    return seqs


SEQS = collection()
LENS = [len(s) for s in SEQS]
TEXT = np.frombuffer(b"".join(SEQS), np.uint8)
SEQ_OFFS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.uint64)


def arrays(reads, lists):
    """reads: list of bytes; lists: per read a list of (seq, diag, seg_score, matches) -> read bytes, read_offsets, cand_offsets, cands (the fields the stage
    only copies hold a running number)"""
    roffs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    cands = np.zeros(int(offs[-1]), R.VERIFY_DTYPE)
    at = 0
    for mine in lists:
        for k, (q, diag, score, matches) in enumerate(mine):
            c = cands[at]
            c["seq"], c["diag"], c["seg_score"], c["matches"], c["n_cand"], c["cand_index"] = q, diag, score, matches, k, k
            for n, f in enumerate(COPIED):
                c[f] = (at * 8 + n) & 0xFFFFFFFF
            at += 1
    return np.frombuffer(b"".join(reads), np.uint8), roffs, offs, cands


def check(reads, lists, fmin, fmax, penalty=4, min_score=12, anchors=2, seqs=None):
    """both flag values against the emulator; returns the emulator's result with MERGE"""
    seqs = SEQS if seqs is None else seqs
    text = np.frombuffer(b"".join(seqs), np.uint8)
    soffs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    cat, roffs, offs, cands = arrays(reads, lists)
    for flags in (0, P.RESCUE_MERGE):
        exp = R.read_rescue(seqs, reads, offs, cands, fmin, fmax, penalty, min_score, anchors, flags)
        got = P.read_rescue_arrays(0, text, soffs, cat, roffs, offs, cands, fmin, fmax, penalty, min_score, anchors, flags)
        bad = np.flatnonzero(got["reads"] != exp["reads"])
        assert len(bad) == 0, (flags, len(bad), int(bad[0]), got["reads"][bad[0]], exp["reads"][bad[0]])
        assert got["reads"].tobytes() == exp["reads"].tobytes()
        if flags:
            assert np.array_equal(got["cand_offsets"], exp["cand_offsets"])
            bad = np.flatnonzero(got["cands"] != exp["cands"])
            assert len(bad) == 0, (len(bad), int(bad[0]), got["cands"][bad[0]], exp["cands"][bad[0]])
            assert got["cands"].tobytes() == exp["cands"].tobytes() and got["winners"].tobytes() == exp["winners"].tobytes()
        else:
            assert got["cand_offsets"] is None and got["cands"] is None and got["winners"] is None
    return exp


def cut(q, d, n, subs=(), seqs=None):
    """n bases of sequence q from diagonal d on (bases off the sequence are N, an N of the text reads as A), with the bases at `subs` replaced"""
    s = (SEQS if seqs is None else seqs)[q]
    out = bytearray((ord("N") if not 0 <= d + i < len(s) else s[d + i] if s[d + i] in b"ACGT" else ord("A")) for i in range(n))
    for i in subs:
        out[i] = b"ACGT"[(b"ACGT".index(out[i]) + 1) % 4]
    return bytes(out)


MATE = b"A" * 50  # the placed mate's bytes are never read: its candidates are stated


def flagged(exp, bit):
    return [bool(int(f) & bit) for f in exp["reads"]["flags"]]


@pytest.mark.parametrize("width", (1, 2, 63, 64, 65, 128, 129, 1001))
def test_windows_around_the_wave_width(width):
    # the anchor at diag 100 of sequence 0 (L = 1500): d = 1400 - frag; frag in [300, 300 + width): d in (1100 - width, 1100]
    lo, hi = 1100 - width + 1, 1100
    reads = [MATE, cut(1, lo, 50, (9, 29)), MATE, cut(1, hi, 50, (19,)), MATE, cut(1, lo - 1, 50), MATE, cut(1, hi + 1, 50)]
    exp = check(reads, [[(0, 100, 50, 50)], []] * 4, 300, 300 + width - 1)
    recs = exp["reads"]
    assert flagged(exp, R.RESCUED) == [False, True, False, True, False, False, False, False]  # one off the window on either side: not found
    assert [int(recs[r]["diag"]) for r in (1, 3)] == [lo, hi] and [int(recs[r]["n_diags"]) for r in (1, 3, 5, 7)] == [width] * 4
    assert exp["n_tasks"] == 4 and exp["n_diags"] == 4 * width


def test_windows_clipped_at_the_start_the_end_on_both_sides_and_to_nothing():
    reads, lists = [], []
    # (sequence, diag) of the anchor, the truth on the twin, a substituted base that lies on the sequence
    for q, diag, truth, sub in ((1, 1400, -49, 49), (1, 1400, -1, 25), (1, 1400, 0, 25), (1, 1049, 1, 25), (1, -300, 1480, 5), (1, -300, 1451, 25), (1, -300, 1320, 25),
                                (9, 0, -49, 49), (9, 0, 40, 5), (9, 10, 7, 25), (1, 1550, 5, 25), (1, -1000, 5, 25), (1, 2 ** 40, 5, 25), (1, -(2 ** 40), 5, 25)):
        reads += [MATE, cut(q ^ 1, truth, 50, (sub,) if truth != -49 else ())]
        lists += [[(q, diag, 50, 50)], []]
    exp = check(reads, lists, 0, 500, min_score=1)
    nd = [int(x) for x in exp["reads"]["n_diags"][1::2]]
    assert nd[:4] == [150, 150, 150, 501] and nd[4:7] == [200, 200, 200] and nd[7:10] == [113, 113, 104] and nd[10:] == [0, 0, 0, 0]
    # (at -49 one base lies on the sequence: it matches on many diagonals, of which -49 is the smallest)
    assert [int(x) for x in exp["reads"]["diag"][1:20:2]] == [-49, -1, 0, 1, 1480, 1451, 1320, -49, 40, 7]
    assert flagged(exp, R.TARGET)[1::2] == [True] * 14 and flagged(exp, R.RESCUED)[21::2] == [False] * 4
    assert all(int(s) == R.NO_SEQUENCE for s in exp["reads"]["seq"][21::2])


def test_read_lengths_around_the_word():
    reads, lists = [], []
    for n in (0, 1, 7, 8, 9, 16, 17, 50, 150):
        for truth in (700, 703):
            reads += [MATE, cut(1, truth, n, (n // 2,) if n > 8 else ())]
            lists += [[(0, 500, 50, 50)], []]
    exp = check(reads, lists, 250, 349, min_score=1)  # d in [651, 750]
    recs = exp["reads"][1::2]
    assert [int(x) for x in recs["n_diags"]] == [0, 0] + [100] * 16
    assert all(int(r["diag"]) == (700, 703)[k % 2] for k, r in enumerate(recs) if k >= 6)  # (from 8 bases on the truth is the only best)
    assert [int(x) for x in recs["seg_score"][-4:]] == [45, 45, 145, 145]
    check(reads, lists, 250, 349, min_score=8)


def test_every_residue_of_the_reads_offset_and_of_the_text_position():
    reads, lists = [], []
    for i in range(8):
        for j in range(8):
            reads += [b"C" * (41 + i), cut(1, 900 + j, 50 - j, (11,))]
            lists += [[(0, 100, 50, 50)], []]
    cat, roffs, _, _ = arrays(reads, lists)
    assert {int(roffs[r]) % 8 for r in range(1, len(reads), 2)} == set(range(8))
    exp = check(reads, lists, 400, 520)
    assert [int(x) for x in exp["reads"]["diag"][1::2]] == [900 + j for i in range(8) for j in range(8)] and all(flagged(exp, R.RESCUED)[1::2])
    # the same at the start of the text: the window begins before symbol 0 of sequence 0
    reads, lists = [], []
    for j in range(-8, 9):
        reads += [b"G" * (43 + j % 8), cut(0, j, 50, (30,))]
        lists += [[(1, 1400, 50, 50)], []]
    exp = check(reads, lists, 0, 500)
    assert [int(x) for x in exp["reads"]["diag"][1::2]] == list(range(-8, 9)) and all(flagged(exp, R.RESCUED)[1::2])


def test_the_first_and_the_last_symbol_of_the_text():
    last = len(SEQS) - 1
    reads = [MATE, cut(0, -49, 50), MATE, cut(0, 0, 50, (3,)), MATE, cut(last, 63, 50), MATE, cut(last, 14, 50, (44,)), MATE, cut(last, 15, 50)]  # (15: the last base off the text)
    lists = [[(1, 1400, 50, 50)], [], [(1, 1400, 50, 50)], [], [(last ^ 1, 0, 50, 50)], [], [(last ^ 1, 0, 50, 50)], [], [(last ^ 1, 0, 50, 50)], []]
    exp = check(reads, lists, 0, 500, min_score=1)
    got = [(int(r["seq"]), int(r["diag"]), int(r["matches"])) for r in exp["reads"][1::2]]
    # (one base on the sequence matches on many diagonals: the smallest wins, which is -49 at the start and lies before 63 at the end)
    assert got[:2] == [(0, -49, 1), (0, 0, 49)] and got[2][0] == last and got[2][1] <= 63 and got[2][2] == 1 and got[3:] == [(last, 14, 49), (last, 15, 49)]
    assert [int(x) for x in exp["reads"]["n_diags"][1::2]] == [150, 150, 113, 113, 113]


def test_bytes_that_never_match_and_n_in_the_text():
    # sequence 2 holds N at 5, 100 and 190; its window is all of it
    base = cut(2, 80, 50)
    n_at = bytearray(base); n_at[20] = ord("N")       # N opposite the text's N
    a_at = bytearray(base); a_at[20] = ord("A")       # a base opposite the text's N
    low = bytearray(base); low[30:34] = base[30:34].lower()
    star = bytearray(base); star[0], star[49], star[25] = ord("*"), 0xFF, ord("R")
    all_n = b"N" * 50
    reads = [MATE, bytes(n_at), MATE, bytes(a_at), MATE, bytes(low), MATE, bytes(star), MATE, all_n]
    exp = check(reads, [[(3, 0, 50, 50)], []] * 5, 0, 500)
    recs = exp["reads"][1::2]
    # the read lies in the repeat of period 7, where the N at 100 is one mismatch on whichever diagonal: nine tie, the first at 24
    assert [int(x) for x in recs["diag"]] == [24] * 4 + [-49] and [int(x) for x in recs["matches"]] == [49, 49, 45, 46, 0] and recs[0] == recs[1]
    assert [int(x) for x in recs["seg_score"]] == [45, 45, 25, 38, 0] and int(recs[4]["n_best"]) == int(recs[4]["n_diags"]) == 249 and int(recs[0]["n_best"]) == 9
    assert flagged(exp, R.RESCUED)[1::2] == [True, True, True, True, False]


def test_sequences_of_length_0_and_1():
    reads, lists = [], []
    for q in (4, 5, 6, 7):
        for read in (SEQS[6] * 1, b"ACGT" * 5, b""):
            reads += [MATE, read]
            lists += [[(q, 0, 50, 50), (q, -3, 50, 50)], []]
    exp = check(reads, lists, -10, 500, min_score=1)
    recs = exp["reads"][1::2]
    assert [int(x) for x in recs["n_diags"][:6]] == [0, 38, 0, 0, 38, 0]           # L = 0: the diagonals -(len - 1) .. -1, none with a span
    assert [int(x) for x in recs["n_diags"][6:]] == [2, 40, 0, 2, 40, 0] and [int(x) for x in recs["seg_score"][:6]] == [0] * 6
    assert int(recs[6]["seg_score"]) == 0 and int(recs[9]["seg_score"]) == 1       # the one symbol against itself, on sequence 6 alone (7 holds its complement)


@pytest.mark.parametrize("anchors,tied", [(1, 1), (1, 3), (2, 3), (8, 3), (2, 9), (8, 9)])
def test_anchor_counts_at_and_beyond_max_anchors(anchors, tied):
    # the mate's candidates: a weaker one first, then `tied` equal winners 140 diagonals apart on sequence 0 (L = 1500) -- windows of 50 that do not meet
    mate = [(0, 40, 49, 50)] + [(0, 1200 - 140 * k, 50, 50) for k in range(tied)] + [(1, 300, 50, 49)]
    reads, lists = [], []
    for k in range(tied):  # the truth of pair k lies in the window of tied anchor k: d = 1500 - diag - frag, frag in [200, 249]
        reads += [MATE, cut(1, 1500 - (1200 - 140 * k) - 225, 50, (7, 33))]
        lists += [mate, []]
    exp = check(reads, lists, 200, 249, anchors=anchors)
    recs = exp["reads"][1::2]
    assert [int(x) for x in recs["n_anchors"]] == [min(anchors, tied)] * tied and [int(x) for x in recs["n_diags"]] == [50 * min(anchors, tied)] * tied
    assert flagged(exp, R.RESCUED)[1::2] == [k < anchors for k in range(tied)]  # found where the truth's anchor is among the first max_anchors
    assert all(int(recs[k]["anchor"]) == 1 + k for k in range(min(anchors, tied)))


def test_ties_inside_a_wave_across_waves_and_across_anchors():
    # sequence 3 holds the reverse complement of a repeat of period 7: a read of 50 inside ties on every diagonal 7 apart
    t0 = 200 - 174
    read = cut(3, t0 + 14, 50, (10, 30))
    anchor, twice = [(2, 0, 50, 50)], [(2, 0, 50, 50), (2, 20, 50, 50)]
    reads, lists = [MATE, read, MATE, read, MATE, read], [anchor, [], twice, [], twice + [(2, 21, 50, 50)], []]
    exp = check(reads, lists, 0, 500, anchors=8)
    recs = exp["reads"][1::2]
    # 15 diagonals 7 apart hold the read; the N of the text leaves nine of them tied (on the others it faces a base that matched): over three waves of the window
    ties = 9
    assert [int(x) for x in recs["n_best"]] == [ties, 2 * ties, 3 * ties] and [int(x) for x in recs["diag"]] == [t0] * 3 and [int(x) for x in recs["anchor"]] == [0] * 3
    assert [int(x) for x in recs["n_diags"]] == [249, 479, 708] and int(recs[0]["next_score"]) == int(recs[0]["seg_score"]) - 1 == 39
    # windows that start inside the repeat, one wave wide and less and more: the first tie of the window, not of the repeat
    for width, n_best in ((30, 2), (64, 5), (65, 5), (100, 5)):
        exp = check(reads[:2], lists[:2], 200 - (t0 + 50) - width + 1, 200 - (t0 + 50))  # d in [t0 + 50, t0 + 50 + width)
        rec = exp["reads"][1]
        assert (int(rec["diag"]), int(rec["n_best"]), int(rec["n_diags"])) == (t0 + 63, n_best, width)
    # across anchors with different windows: the smaller anchor ordinal wins although the other's window holds smaller diagonals that tie
    exp = check(reads[:2], [[(2, 40, 50, 50), (2, 0, 50, 50)], []], 0, 120, anchors=2)
    rec = exp["reads"][1]
    assert int(rec["anchor"]) == 0 and int(rec["diag"]) > t0 and (int(rec["diag"]) - t0) % 7 == 0 and int(rec["n_best"]) > 2


def test_min_score_at_the_best_score_and_one_above():
    reads, lists = [MATE, cut(1, 700, 50, (10, 30))], [[(0, 500, 50, 50)], []]
    best = int(check(reads, lists, 0, 500)["reads"][1]["seg_score"])
    assert best == 50 - 2 - 2 * 4
    assert flagged(check(reads, lists, 0, 500, min_score=best), R.RESCUED) == [False, True]
    assert flagged(check(reads, lists, 0, 500, min_score=best + 1), R.RESCUED) == [False, False]
    assert flagged(check(reads, lists, 0, 500, min_score=2 ** 32 - 1), R.RESCUED) == [False, False]


@pytest.mark.parametrize("penalty", (1, 1 << 20))
def test_both_ends_of_the_penalty_range(penalty):
    reads = [MATE, cut(1, 700, 50, (10, 30)), MATE, cut(1, 650, 150, range(5, 150, 9))]
    exp = check(reads, [[(0, 500, 50, 50)], []] * 2, 0, 500, penalty=penalty)
    assert [int(x) for x in exp["reads"]["seg_score"][1::2]] == ([46, 117] if penalty == 1 else [19, 8])  # (at 2^20 the longest run)


def test_every_candidate_count_of_the_target_and_mates_on_the_merged_list():
    reads, lists = [], []
    for own in (0, 1, 15, 16, 63, 64):
        reads += [MATE, cut(1, 700, 50, (10, 30))]
        lists += [[(0, 500, 50, 50)], [(8, 3 + k, 20 + k % 3, 20) for k in range(own)]]  # candidates of its own on another path: none compatible
    exp = check(reads, lists, 0, 500)
    fl = [int(f) for f in exp["reads"]["flags"][1::2]]
    assert fl == [R.TARGET | R.RESCUED] * 5 + [R.FULL] and [int(x) for x in np.diff(exp["cand_offsets"].astype(np.int64))[1::2]] == [1, 2, 16, 17, 64, 64]
    assert [int(w["cand_index"]) for w in exp["winners"][1::2]] == [0, 1, 15, 16, 63, 2]  # the appended candidate scores most; FULL keeps its own winner
    assert exp["n_full"] == 1 and exp["n_rescued"] == 5
    # the mates kernel on the merged list: 17 entries need a group of 32 lanes, 64 one of 64
    for pick in ((6, 8), (8, 10), (0, 12)):
        offs = exp["cand_offsets"][pick[0]:pick[1] + 1] - exp["cand_offsets"][pick[0]]
        cands = exp["cands"][int(exp["cand_offsets"][pick[0]]):int(exp["cand_offsets"][pick[1]])]
        want = M.read_mates(LENS, offs, cands, 0, 500, 10, M.ELECT)
        got = P.read_mates_arrays(0, LENS, offs, cands, 0, 500, 10, P.MATES_ELECT)
        assert got["pairs"].tobytes() == want["pairs"].tobytes() and got["winners"].tobytes() == want["winners"].tobytes()
        assert all(int(f) & M.PROPER for f in want["pairs"]["flags"][:5])


def test_merge_without_a_rescued_read_and_a_pair_of_two_targets():
    reads = [cut(0, 100, 50), cut(1, 400, 50, (25,)), cut(0, 100, 50, (5, 40)), cut(1, 900, 50)]
    lists = [[(0, 100, 50, 50)], [(1, 400, 45, 49)], [], []]  # frag 1000: not compatible, each a target around the other; a pair without any candidate
    exp = check(reads, lists, 0, 500)
    assert [int(f) for f in exp["reads"]["flags"]] == [R.TARGET, R.TARGET, 0, 0] and exp["n_rescued"] == 0 and exp["n_targets"] == 2
    assert list(exp["cand_offsets"]) == [0, 1, 2, 2, 2]
    exp = check(reads, lists, 900, 1000)  # compatible at these bounds: no target
    assert exp["n_targets"] == 0


@pytest.mark.parametrize("n_reads", (2, 126, 128, 130, 70002))
def test_read_counts_at_the_wave_and_grid_borders(n_reads):
    rng = np.random.default_rng(4400)
    base_reads, base_lists = [], []
    period = 11  # pairs; divides no border
    for k in range(period):
        d = int(rng.integers(600, 640))
        kind = k % 4
        mate = [(0, 800, 50, 50)] if kind != 3 else []
        own = [] if kind != 2 else [(1, d, 30, 40)]  # kind 2: compatible, no target; kind 3: the mate has no candidate
        pair = [(MATE[:40 + k], mate), (cut(1, d, 50 - k, (20,)) if kind != 1 else cut(8, 3, 50), own)]
        if k % 2:
            pair.reverse()
        base_reads += [pair[0][0], pair[1][0]]
        base_lists += [pair[0][1], pair[1][1]]
    exp1 = R.read_rescue(SEQS, base_reads, *arrays(base_reads, base_lists)[2:], 40, 139, 4, 12, 2, R.MERGE)  # the emulator runs on one period
    reps = n_reads // (2 * period) + 1
    reads, lists = (base_reads * reps)[:n_reads], (base_lists * reps)[:n_reads]
    cat, roffs, offs, cands = arrays(reads, lists)
    per = int(arrays(base_reads, base_lists)[2][-1])
    cands1 = arrays(base_reads, base_lists)[3]
    for f in COPIED:  # (the copied fields repeat with the period, as the expectation does)
        cands[f] = np.tile(cands1[f], reps)[:len(cands)]
    got = P.read_rescue_arrays(0, TEXT, SEQ_OFFS, cat, roffs, offs, cands, 40, 139, 4, 12, 2, P.RESCUE_MERGE)
    assert got["reads"].tobytes() == np.tile(exp1["reads"], reps)[:n_reads].tobytes()
    assert got["winners"].tobytes() == np.tile(exp1["winners"], reps)[:n_reads].tobytes()
    counts = np.tile(np.diff(exp1["cand_offsets"].astype(np.int64)), reps)[:n_reads]
    assert np.array_equal(np.diff(got["cand_offsets"].astype(np.int64)), counts)
    eo = exp1["cand_offsets"].astype(np.int64)
    want = np.concatenate([exp1["cands"][eo[r % (2 * period)]:eo[r % (2 * period) + 1]] for r in range(n_reads)])
    assert got["cands"].tobytes() == want.tobytes()
    assert (exp1["n_rescued"], exp1["n_targets"]) == (3, 6) and per > 0  # of 11 pairs: three found, three random, three compatible, two without a placed mate


def test_every_refusal_leaves_the_outputs_untouched():
    reads, lists = [MATE, cut(1, 700, 50, (10, 30)), MATE, MATE], [[(0, 500, 50, 50)], [], [], [(9, 3, 9, 9)]]
    cat, roffs, offs, cands = arrays(reads, lists)
    big = arrays([MATE, MATE], [[(0, 1, 1, 1)] * 65, []])
    bad_seq = cands.copy()
    bad_seq[1]["seq"] = len(SEQS)
    bad_text = TEXT.copy()
    bad_text[7] = ord("x")
    untwinned = SEQ_OFFS.copy()
    untwinned[3] += 1
    A, U, N = P.ERR_ARG, P.ERR_UNSUPPORTED, P.ERR_NOMEM
    refusals = [
        (dict(flags=2), A, "unknown flag"), (dict(fmin=501), A, "frag_min 501 exceeds frag_max 500"), (dict(fmin=500 - 65536), A, "window"), (dict(min_score=0), A, "min_score 0"),
        (dict(anchors=0), A, "max_anchors 0"), (dict(anchors=9), A, "max_anchors 9"), (dict(penalty=0), A, "mismatch_penalty 0"), (dict(penalty=(1 << 20) + 1), A, "mismatch_penalty"),
        (dict(soffs=SEQ_OFFS[:-1]), A, "odd"), (dict(soffs=untwinned), A, "p = 1"), (dict(text=bad_text), U, "text byte 120 at offset 7"),
        (dict(offs=np.array([1, 1, 2, 2, 3], np.uint64)), A, "start at 0"), (dict(offs=np.array([0, 2, 1, 2, 3], np.uint64)), A, "decrease at read 1"),
        (dict(roffs=np.array([0, 50, 40, 150, 200], np.uint64)), A, "decrease at read 1"),
        (dict(reads=big[0], roffs=big[1], offs=big[2], cands=big[3]), A, "read 0 has 65 candidates"), (dict(cands=bad_seq), A, "read 3 has seq %d" % len(SEQS)),
        (dict(reads=cat[:150], roffs=roffs[:4], offs=offs[:4]), A, "odd"), (dict(list_cap=2), N, "holds 3 candidates, list_cap is 2"),
    ]
    for kw, code, text in refusals:
        out = dict(reads=np.full(4, 0xA5, np.uint8).repeat(64).view(R.RESCUE_DTYPE), winners=np.full(4, 0x5A, np.uint8).repeat(64).view(R.VERIFY_DTYPE),
                   cands=np.full(8, 0x3C, np.uint8).repeat(64).view(R.VERIFY_DTYPE), cand_offsets=np.full(5, 0x77, np.uint64))
        keep = [out[k].tobytes() for k in sorted(out)]
        with pytest.raises(P.PgxError) as e:
            P.read_rescue_arrays(0, kw.get("text", TEXT), kw.get("soffs", SEQ_OFFS), kw.get("reads", cat), kw.get("roffs", roffs), kw.get("offs", offs), kw.get("cands", cands),
                                 kw.get("fmin", 0), 500, kw.get("penalty", 4), kw.get("min_score", 12), kw.get("anchors", 2), kw.get("flags", P.RESCUE_MERGE),
                                 list_cap=kw.get("list_cap", 8), out=out)
        assert e.value.code == code and text in str(e.value), (list(kw), str(e.value))
        assert [out[k].tobytes() for k in sorted(out)] == keep, list(kw)
    exp = check(reads, lists, 0, 500)  # and the same arguments unbroken are served
    assert exp["n_rescued"] == 1 and int(exp["cand_offsets"][-1]) == 3
    got = P.read_rescue_arrays(0, TEXT, SEQ_OFFS, cat, roffs, offs, cands, 0, 500, 4, 12, 2, P.RESCUE_MERGE, list_cap=3)  # exactly enough
    assert got["cands"].tobytes() == exp["cands"].tobytes()
    check(reads, lists, -(2 ** 63), -(2 ** 63) + 65535), check(reads, lists, 2 ** 63 - 65536, 2 ** 63 - 1), check(reads, lists, -100, 65435)  # the widest windows, at the ends of the range
    empty = P.read_rescue_arrays(0, TEXT, SEQ_OFFS, np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(0, R.VERIFY_DTYPE), 0, 500, 4, 12, 2, P.RESCUE_MERGE)
    assert len(empty["reads"]) == 0 and len(empty["winners"]) == 0 and list(empty["cand_offsets"]) == [0] and len(empty["cands"]) == 0
