"""GPU tier of the read-placement kernels at their borders, through pgx_read_place_arrays (the kernels of pgx_batch_read_place on host
arrays): every field of every record and the full PGX_PLACE_LIST equal tests/place_emu.py byte for byte, and a call without the flag
returns the same records.

The anchors of a read are one segment of the tag stage's segmented sort, whose size classes end at 64 (in registers), 2048
(PGX_SORT_LDS_CAP, a wave in LDS) and 16384 (PGX_SORT_WG_LDS_CAP, a workgroup in LDS; beyond: global scratch); the sweep takes 64 / G
anchors a step at G lanes a read (G = 4 .. 64, chosen from the mean of the pass; PGX_PLACE_LANES fixes it), so 15 / 16 / 17, 63 / 64 / 65
and 127 / 128 / 129 are its step borders."""
import numpy as np
import pytest

import pgx_ffi as P
import place_emu as E

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 16384, 16385]
SMALL = [(2, 9, [(0, 5), (0, 30)]), (4, 12, [(0, 7)])]  # two placements on sequence 0: diagonal 3 (both MEMs) and 28


def _check(case, n_seq, L):
    """records and list == the emulator's, with PLACE_LIST and without; returns the emulator's result"""
    mem_offsets, mems, loc_offsets, values = case
    exp = E.read_place(mem_offsets, mems, loc_offsets, values, L)
    got = P.read_place_arrays(0, mem_offsets, mems, loc_offsets, values, n_seq, L, P.PLACE_LIST)
    bad = np.flatnonzero(got["reads"] != exp["reads"])
    assert len(bad) == 0, (len(bad), int(bad[0]), got["reads"][bad[0]], exp["reads"][bad[0]])
    assert got["reads"].tobytes() == exp["reads"].tobytes()
    assert np.array_equal(got["place_offsets"], exp["place_offsets"])
    bad = np.flatnonzero(got["places"] != exp["places"])
    assert len(bad) == 0, (len(bad), int(bad[0]), got["places"][bad[0]], exp["places"][bad[0]])
    assert got["places"].tobytes() == exp["places"].tobytes()
    assert np.array_equal(exp["reads"]["n_placements"], np.diff(exp["place_offsets"]))
    plain = P.read_place_arrays(0, mem_offsets, mems, loc_offsets, values, n_seq, L, 0)
    assert plain["reads"].tobytes() == exp["reads"].tobytes() and plain["places"] is None and plain["place_offsets"] is None
    return exp


def _case(reads, L):
    mem_offsets, mems, loc_offsets, packed = E.build_case(reads)
    return mem_offsets, mems, loc_offsets, packed(L)


def _one_placement(k):
    """k MEMs of length 4 on starts 0, 2, 4, ... (each overlaps the next), all on diagonal 7 of sequence 1"""
    return [(2 * j, 2 * j + 4, [(1, 7 + 2 * j)]) for j in range(k)]


def _many_placements(k, rng):
    """k anchors over two overlapping MEMs: distinct offsets a MEM, many diagonals shared by the two"""
    ka = (k + 1) // 2
    offs_a = rng.permutation(4 * k + 8)[:ka]
    offs_b = np.concatenate([offs_a[: (k - ka) // 2] + 10, 8 * k + 100 + rng.permutation(4 * k + 8)])[: k - ka]  # (shared: off - start equal)
    return [(0, 20, [(0, int(o)) for o in offs_a]), (10, 35, [(0, int(o)) for o in offs_b])]


@pytest.mark.parametrize("k", SIZES)
def test_anchors_per_read_at_the_size_class_borders(k):
    rng = np.random.default_rng(k)
    L = 1 << 20
    exp = _check(_case([SMALL, _one_placement(k), SMALL], L), 2, L)
    assert exp["reads"]["n_anchors"].tolist() == [3, k, 3] and exp["reads"]["n_placements"].tolist() == [2, min(k, 1), 2]
    assert int(exp["reads"]["best_score"][1]) == (2 * k + 2 if k else 0) and int(exp["reads"]["best_mems"][1]) == k
    exp = _check(_case([SMALL, _many_placements(k, rng), SMALL], L), 2, L)
    assert exp["reads"]["n_anchors"].tolist() == [3, k, 3]
    if k >= 15:
        assert k // 2 < int(exp["reads"]["n_placements"][1]) < k and int(exp["reads"]["best_score"][1]) == 35


def test_a_placement_across_four_steps():
    L = 5000
    reads = [SMALL, [(3 * j, 3 * j + 5, [(2, 100 + 3 * j)] + ([(1, 3 * j + (j % 7))] if j % 3 == 0 else [])) for j in range(300)], SMALL]
    exp = _check(_case(reads, L), 3, L)
    assert exp["reads"][1]["best_mems"] == 300 and exp["reads"][1]["best_score"] == 3 * 299 + 5 and exp["reads"][1]["best_diag"] == 100


@pytest.mark.parametrize("n_seq,L", [(1, 100), (2, 64), (64, 1000), (65, 1000), (4096, 300), (5000, 1 << 20)])
def test_random_reads(n_seq, L, monkeypatch):
    rng = np.random.default_rng(7000 + n_seq)
    for n_reads, lanes in ((1, None), (3, "1"), (5, "8"), (257, None), (257, "64"), (257, "2")):  # the last wave and the last block are partial at every packing
        if lanes:
            monkeypatch.setenv("PGX_PLACE_LANES", lanes)
        else:
            monkeypatch.delenv("PGX_PLACE_LANES", raising=False)
        exp = _check(E.random_case(rng, n_reads, n_seq, L, big=n_reads == 5), n_seq, L)
    h = exp["reads"]
    assert (h["n_mems"] == 0).any() and (h["n_located"] < h["n_mems"]).any() and (h["best_score"] > 0).any() and (h["next_score"] > 0).any()


def test_reads_without_mems_and_mems_without_values():
    L = 50
    reads = [[], [(3, 9, [])], [], [(0, 5, []), (2, 8, [(4, 49)]), (4, 6, [])], [], []]
    exp = _check(_case(reads, L), 5, L)
    assert exp["reads"]["n_mems"].tolist() == [0, 1, 0, 3, 0, 0] and exp["reads"]["n_located"].tolist() == [0, 0, 0, 1, 0, 0]
    assert exp["reads"]["best_seq"].tolist() == [P.NO_SEQUENCE] * 3 + [4] + [P.NO_SEQUENCE] * 2 and int(exp["reads"]["best_diag"][3]) == 47
    _check(_case([[], [], []], L), 5, L)  # no MEM at all: the MEM and value arrays are empty
    _check(_case([[(1, 4, [])]], L), 5, L)  # MEMs, no value


@pytest.mark.parametrize("n_seq", [1, 2, 64, 65, 4096, 5000])
def test_diagonals(n_seq):
    L, z = 1000, n_seq - 1
    reads = [
        [(5, 10, [(z, 2)]), (7, 30, [(z, 4)])],                        # negative diagonal: off < start
        [(0, 10, [(z, L - 1)]), (3, 8, [(z, L - 1)])],                 # off == max_length - 1; diagonals L - 1 and L - 4
        [(0, 10, [(0, 50), (z, 50)]), (20, 25, [(z, 70)])],            # the same diagonal on two sequences
        [(0, 10, [(z, 50)]), (20, 40, [(z, 71)])],                     # diagonals 50 and 51: two placements
        [(1, 9, [(z, 11), (0, 3)])],                                   # the next read has the same anchors
        [(1, 9, [(z, 11), (0, 3)])],
        [(4, 9, [(0, 3)]), (6, 11, [(0, 6)])],                         # first best decided by the sign: diagonals -1 and 0 tie
    ]
    exp = _check(_case(reads, L), n_seq, L)
    h = exp["reads"]
    assert int(h["best_diag"][0]) == -3 and int(h["best_score"][0]) == 25 and int(h["best_diag"][6]) == -1 and int(h["n_best"][6]) == 2
    assert int(h["n_placements"][3]) == 2 and int(h["best_diag"][3]) == 51 and h[4].tobytes() == h[5].tobytes()
    assert int(h["n_placements"][2]) == (2 if n_seq > 1 else 1) and int(h["best_seq"][2]) == (z if n_seq > 1 else 0)


def test_intervals_and_scores_beyond_32_bits():
    L = 1 << 36
    d = [(0, 100)]
    reads = [
        [(0, 10, d), (10, 20, [(0, 110)]), (20, 21, [(0, 120)])],                                  # abutting
        [(0, 10, d), (5, 15, [(0, 105)]), (14, 30, [(0, 114)])],                                   # overlapping
        [(0, 100, d), (10, 20, [(0, 110)]), (30, 40, [(0, 130)]), (50, 120, [(0, 150)])],          # nested, then one that reaches further
        [(0, 50, d), (1, 40, [(0, 101)]), (2, 30, [(0, 102)]), (3, 60, [(0, 103)])],               # ends descend while starts ascend
        [(5, 5, [(0, 105)]), (7, 3, [(0, 107)]), (9, 0, [(0, 109)])],                              # end <= start only: a placement, never best
        [(5, 5, [(0, 105)]), (7, 3, [(0, 107)]), (10, 11, [(0, 110), (1, 0)])],
        [(0, 10, d), (20, 30, [(0, 120)])],                                                        # a gap that stays a gap
        [(3, 1 << 33, [(0, 103), (1, 5)]), (7, (1 << 33) + 5, [(0, 107)])],                        # the score exceeds 32 bits
    ]
    exp = _check(_case(reads, L), 2, L)
    h = exp["reads"]
    assert h["best_score"].tolist() == [21, 30, 120, 60, 0, 1, 20, (1 << 33) + 2]
    assert int(h["n_placements"][4]) == 1 and int(h["best_seq"][4]) == P.NO_SEQUENCE and int(h["next_score"][7]) == (1 << 33) - 3


@pytest.mark.parametrize("n_best", [1, 2, 70])
def test_ties_and_runner_up(n_best):
    L = 10000
    # n_best placements of score 12 (two MEMs each) behind one of score 8 that comes first, and one of score 11
    tie = [(0, 8, [(1, 100 * t) for t in range(n_best)] + [(0, 3)]), (10, 14, [(1, 100 * t + 10) for t in range(n_best)]), (20, 31, [(2, 77)])]
    every = [(0, 8, [(1, 100 * t) for t in range(n_best)])]  # every placement ties: no runner-up
    later = [(0, 5, [(0, 50)]), (6, 20, [(0, 9), (3, 400)]), (30, 44, [(3, 424)])]  # the best is not the first placement
    exp = _check(_case([tie, every, later], L), 4, L)
    h = exp["reads"]
    assert h["n_best"].tolist() == [n_best, n_best, 1] and h["best_score"].tolist() == [12, 8, 28] and h["next_score"].tolist() == [11, 0, 14]
    assert h["best_seq"].tolist() == [1, 1, 3] and h["best_diag"].tolist() == [0, 0, 394] and h["best_mems"].tolist() == [2, 1, 2]


def test_order_of_values_and_duplicates():
    rng = np.random.default_rng(5)
    L, n_seq = 4096, 9
    mem_offsets, mems, loc_offsets, values = E.random_case(rng, 40, n_seq, L, max_occ=12)
    base = P.read_place_arrays(0, mem_offsets, mems, loc_offsets, values, n_seq, L, P.PLACE_LIST)
    shuffled = values.copy()
    for m in range(len(mems)):
        a, b = int(loc_offsets[m]), int(loc_offsets[m + 1])
        shuffled[a:b] = rng.permutation(shuffled[a:b])
    assert not np.array_equal(shuffled, values)
    again = P.read_place_arrays(0, mem_offsets, mems, loc_offsets, shuffled, n_seq, L, P.PLACE_LIST)
    for key in ("reads", "place_offsets", "places"):
        assert again[key].tobytes() == base[key].tobytes(), key
    # one value of one MEM twice: only n_anchors changes
    m = int(np.flatnonzero(np.diff(loc_offsets.astype(np.int64)) > 0)[3])
    r = int(np.searchsorted(mem_offsets, m, side="right")) - 1
    at = int(loc_offsets[m])
    dup_values = np.insert(values, at, values[at])
    dup_offsets = loc_offsets.copy()
    dup_offsets[m + 1:] += np.uint64(1)
    dup = P.read_place_arrays(0, mem_offsets, mems, dup_offsets, dup_values, n_seq, L, P.PLACE_LIST)
    want = base["reads"].copy()
    want["n_anchors"][r] += 1
    assert dup["reads"].tobytes() == want.tobytes() and dup["places"].tobytes() == base["places"].tobytes()


def _budget_case():
    rng = np.random.default_rng(11)
    L = 1 << 16
    reads = E.random_reads(rng, 30, 3, L, max_occ=8)
    for at, k in ((5, 150), (6, 150), (7, 1), (12, 299), (13, 2), (20, 300)):  # read borders on both sides of the pass borders
        reads[at] = _one_placement(k)
    return reads, L


def test_budget_does_not_change_the_bytes(monkeypatch):
    reads, L = _budget_case()
    case = _case(reads, L)
    monkeypatch.delenv("PGX_PLACE_BUDGET_MB", raising=False)
    base = P.read_place_arrays(0, *case, 3, L, P.PLACE_LIST)
    monkeypatch.setenv("PGX_PLACE_BUDGET_MB", "0.0023")  # 2411 bytes: 301 keys a pass
    small = P.read_place_arrays(0, *case, 3, L, P.PLACE_LIST)
    for key in ("reads", "place_offsets", "places"):
        assert small[key].tobytes() == base[key].tobytes(), key
    exp = E.read_place(*case, L)
    assert base["reads"].tobytes() == exp["reads"].tobytes() and base["places"].tobytes() == exp["places"].tobytes()
    assert int(exp["reads"]["n_anchors"].sum()) > 3 * 301  # four passes at least


def _filled(n, cap):
    out = dict(reads=np.zeros(n, P.READ_PLACE_DTYPE), place_offsets=np.zeros(n + 1, np.uint64), places=np.zeros(cap, P.PLACEMENT_DTYPE))
    for a in out.values():
        a.view(np.uint8)[:] = 0xA5
    return out


def _refused(code, case, n_seq, L, flags=P.PLACE_LIST, places_cap=None, named=None):
    n = len(case[0]) - 1
    cap = max(len(case[3]), 1) if places_cap is None else places_cap
    out = _filled(n, max(cap, 1))
    with pytest.raises(P.PgxError) as e:
        P.read_place_arrays(0, *case, n_seq, L, flags, places_cap=cap, out=out)
    assert e.value.code == code, str(e.value)
    if named is not None:
        assert ("read %d" % named) in str(e.value), str(e.value)
    for a in out.values():
        assert (a.view(np.uint8) == 0xA5).all()
    return str(e.value)


def test_a_read_beyond_the_budget_is_refused(monkeypatch):
    reads, L = _budget_case()
    reads[17] = _one_placement(2049)
    monkeypatch.setenv("PGX_PLACE_BUDGET_MB", "0.0023")
    msg = _refused(P.ERR_NOMEM, _case(reads, L), 3, L, named=17)
    assert "2049" in msg and "301" in msg


def test_refusals_leave_the_outputs_untouched():
    L, n_seq = 1000, 4
    reads = [SMALL, [(0, 9, [(3, 5)]), (4, 12, [(2, 8), (1, 0)])], SMALL]
    good = _case(reads, L)
    _refused(P.ERR_ARG, good, n_seq, L, flags=2)                                        # unknown flag
    _refused(P.ERR_ARG, good, n_seq, L, flags=P.PLACE_LIST | 4)
    mem_offsets, mems, loc_offsets, values = (a.copy() for a in good)
    mems["start"][3] = mems["start"][2]                                                 # starts that do not ascend strictly
    _refused(P.ERR_ARG, (mem_offsets, mems, loc_offsets, values), n_seq, L, named=1)
    values = good[3].copy()
    values[-2] = n_seq * L                                                              # a value beyond the last sequence (read 2)
    _refused(P.ERR_ARG, (good[0], good[1], good[2], values), n_seq, L, named=2)
    loc_offsets = good[2].copy()
    loc_offsets[3], loc_offsets[4] = loc_offsets[4], loc_offsets[3] - np.uint64(1)      # decreasing value offsets (same total)
    with pytest.raises(P.PgxError) as e:
        out = _filled(3, 16)
        P._check(P.lib().pgx_read_place_arrays(0, good[0].ctypes.data, 3, good[1].ctypes.data, loc_offsets.ctypes.data, good[3].ctypes.data, n_seq, L, P.PLACE_LIST,
                                               out["reads"].ctypes.data, out["place_offsets"].ctypes.data, out["places"].ctypes.data, 16))
    assert e.value.code == P.ERR_ARG and all((a.view(np.uint8) == 0xA5).all() for a in out.values())
    mem_offsets = good[0].copy()
    mem_offsets[1], mem_offsets[2] = mem_offsets[2], mem_offsets[1]                     # decreasing MEM offsets
    with pytest.raises(P.PgxError) as e:
        out = _filled(3, 16)
        P._check(P.lib().pgx_read_place_arrays(0, mem_offsets.ctypes.data, 3, good[1].ctypes.data, good[2].ctypes.data, good[3].ctypes.data, n_seq, L, P.PLACE_LIST,
                                               out["reads"].ctypes.data, out["place_offsets"].ctypes.data, out["places"].ctypes.data, 16))
    assert e.value.code == P.ERR_ARG and "read 1" in str(e.value) and all((a.view(np.uint8) == 0xA5).all() for a in out.values())
    need = len(E.read_place(*good, L)["places"])
    msg = _refused(P.ERR_NOMEM, good, n_seq, L, places_cap=need - 1)                    # places_cap one too small
    assert str(need) in msg
    got = P.read_place_arrays(0, *good, n_seq, L, P.PLACE_LIST, places_cap=need)
    assert got["places"].tobytes() == E.read_place(*good, L)["places"].tobytes()


def test_keys_that_do_not_fit_64_bits_are_refused():
    n_seq, L = 1 << 20, 1 << 40
    reads = [SMALL, [(2 * j, 2 * j + 3, [(n_seq - 1, 7 + 2 * j)]) for j in range(300)], SMALL]
    msg = _refused(P.ERR_UNSUPPORTED, _case(reads, L), n_seq, L)
    assert "61 bits" in msg and "9 bits" in msg
    # the same reads fit where the sequences are fewer
    _check(_case([SMALL, [(2 * j, 2 * j + 3, [(7, 7 + 2 * j)]) for j in range(300)], SMALL], L), 1 << 14, L)
