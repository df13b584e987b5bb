"""CPU tier of read mates (include/pgx.h "read mates"): the emulator of tests/mates_emu.py on hand-worked lists; the frag formula against
fragments cut from a text on both strands; the layout of the records, the exported entry points and, without a GPU, PGX_ERR_NO_DEVICE (these
fail on a library without the stage); the case table of tests/mates_cases.py with its pinned counts; and the case chain: the oracle's MEMs of
every read, located, go through place_emu and verify_emu at max_cand 16, and the emulator with ELECT then places every mate of the
`repeat_*` and `reverse` classes on its truth, where verify's solo winner alone misses exactly the half that lies in the second copy.

Each mutation of the emulator changes at least one record of the class it targets; the counts are stated."""
import ctypes
import os
import re

import numpy as np
import pytest

import mates_cases as MC
import mates_emu as M
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import place_emu as E
import verify_emu as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = MC.CASES
ENTRY_POINTS = ("pgx_batch_read_mates", "pgx_batch_mated", "pgx_batch_device_mated", "pgx_read_mates_arrays", "pgx_index_twinned")


def cand(seq, diag, score, matches=None):
    return dict(seq=seq, diag=diag, seg_score=score, matches=score if matches is None else matches)


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulator on hand-worked lists
def test_a_repeat_is_settled_by_the_mate():
    lens = [1000, 1000]
    a = [cand(0, 100, 50), cand(0, 700, 50)]  # two copies, tied
    b = [cand(1, 1000 - 700 - 300, 50)]       # the fragment [700, 1000) of path 0: frag 300 with copy 2, 900 with copy 1
    rec = M.mate_pair(lens, a, b, 0, 500, 10)
    assert (rec["frag"], rec["pair_score"], rec["solo_score"], rec["cand_a"], rec["cand_b"], rec["solo_a"], rec["solo_b"]) == (300, 100, 100, 1, 0, 0, 0)
    assert (rec["n_compatible"], rec["n_best"], rec["next_score"], rec["pair_matches"], rec["seq_a"], rec["seq_b"]) == (1, 1, 0, 100, 0, 1)
    assert rec["flags"] == M.PROPER | M.COMPATIBLE | M.HAS_A | M.HAS_B | M.MOVED_A
    rec = M.mate_pair(lens, a, b, 0, 299, 10)  # out of range: the solo winners stay
    assert (rec["frag"], rec["pair_score"], rec["cand_a"], rec["n_compatible"], rec["flags"]) == (0, 0, 0, 0, M.HAS_A | M.HAS_B)


def test_the_monoid_fields_and_the_tie_order():
    lens = [1000, 1000]
    a = [cand(0, 100, 40, 44), cand(0, 101, 40, 45), cand(0, 102, 30, 50)]
    b = [cand(1, 600, 40, 40), cand(1, 601, 40, 40), cand(1, 602, 39, 60)]
    rec = M.mate_pair(lens, a, b, 0, 500, 0)
    # score sums: 80 for i in {0, 1} with j in {0, 1}, 79 with j = 2, 70 / 69 for i = 2; the matches sum picks i = 1 (85), then the smallest j
    assert (rec["pair_score"], rec["pair_matches"], rec["cand_a"], rec["cand_b"], rec["n_best"], rec["n_compatible"], rec["next_score"]) == (80, 85, 1, 0, 2, 9, 79)
    assert rec["solo_a"] == 1 and rec["solo_b"] == 0 and rec["solo_score"] == 80 and rec["flags"] == M.PROPER | M.COMPATIBLE | M.HAS_A | M.HAS_B


def test_mates_without_candidates_and_the_penalty():
    lens = [1000, 1000, 64, 64]
    rec = M.mate_pair(lens, [], [cand(3, 5, 20)], 0, 500, 8)
    assert (rec["cand_a"], rec["solo_a"], rec["seq_a"], rec["seq_b"], rec["solo_score"], rec["flags"]) == (0, 0, M.NO_SEQUENCE, 3, 20, M.HAS_B)
    rec = M.mate_pair(lens, [], [], 0, 500, 8)
    assert (rec["seq_a"], rec["seq_b"], rec["flags"], rec["solo_score"]) == (M.NO_SEQUENCE, M.NO_SEQUENCE, 0, 0)
    a, b = [cand(0, 900, 60), cand(0, 100, 50)], [cand(1, 600, 40)]  # the pair scores 90, the solo winners 100
    assert M.mate_pair(lens, a, b, 0, 500, 10)["flags"] & M.PROPER and not M.mate_pair(lens, a, b, 0, 500, 9)["flags"] & M.PROPER
    offs, cands = np.array([0, 2, 3], np.uint64), np.zeros(3, M.VERIFY_DTYPE)
    for k, c in enumerate(a + b):
        for f, v in c.items():
            cands[k][f] = v
        cands[k]["span_hi"] = 50 + k
    res = M.read_mates(lens, offs, cands, 0, 500, 10, M.ELECT)
    w = res["winners"]
    assert (int(w[0]["diag"]), int(w[0]["span_hi"]), int(w[0]["n_cand"]), int(w[0]["cand_index"]), int(w[0]["n_tied"])) == (100, 51, 2, 1, 1)
    assert (int(w[1]["diag"]), int(w[1]["n_cand"]), int(w[1]["cand_index"]), int(w[1]["n_tied"])) == (600, 1, 0, 1)
    assert (res["n_proper"], res["n_compatible"], res["n_moved_a"], res["n_moved_b"]) == (1, 1, 1, 0)
    assert M.read_mates(lens, offs, cands, 0, 500, 10, 0)["winners"] is None
    assert M.is_twinned(lens) is None and M.is_twinned([5, 5, 7, 8]) == 1 and M.is_twinned([5, 5, 7]) == 1 and M.is_twinned([]) is None


def test_the_frag_formula_on_both_strands():
    """fragment [f, f + I) of sequence q of the case table, cut as the module docstring of mates_cases says: frag == I, whichever mate is named A"""
    n = 0
    for p in C.pairs:
        if p["frag"] is None:
            continue
        (qa, da), (qb, db) = p["truth_a"], p["truth_b"]
        assert qa ^ 1 == qb
        assert M.frag_of(C.lens, dict(seq=qa, diag=da), dict(seq=qb, diag=db)) == p["frag"] == M.frag_of(C.lens, dict(seq=qb, diag=db), dict(seq=qa, diag=da))
        if da >= 0 and db >= 0 and p["kind"] != "below":  # the mates are what the text holds there (`below`: A comes from the other copy, with a substitution)
            assert C.seqs[qa][da:da + MC.READ_LEN] == p["a"] and C.seqs[qb][db:db + MC.READ_LEN] == p["b"]
            frag = C.seqs[qa][da:da + p["frag"]]
            assert frag[:MC.READ_LEN] == p["a"] and MC.rc(frag[-MC.READ_LEN:]) == p["b"]
        n += 1
    assert n == sum(MC.KIND_COUNTS[k] for k in ("unique", "repeat_a", "repeat_b", "reverse", "far", "border", "hang", "tie", "below")) == 132


# ---------------------------------------------------------------------------------------------------------------------------------
# the library's surface
def test_record_layouts():
    d = P.MATES_DTYPE
    assert d.itemsize == 64 and d == M.MATES_DTYPE
    want = dict(frag=0, pair_score=8, solo_score=12, cand_a=16, cand_b=20, solo_a=24, solo_b=28, n_compatible=32, n_best=36, next_score=40, pair_matches=44, seq_a=48,
                seq_b=52, flags=56, reserved=60)
    assert {n: d.fields[n][1] for n in d.names} == want
    assert ctypes.sizeof(P.ReadMatesResult) == 80
    offs = {n: getattr(P.ReadMatesResult, n).offset for n, _ in P.ReadMatesResult._fields_}
    assert offs == dict(n_pairs=0, n_proper=8, n_compatible=16, n_moved_a=24, n_moved_b=32, frag_min=40, frag_max=48, flags=56, penalty=60, pairs=64, ms_mates=72, reserved=76)
    header = open(os.path.join(ROOT, "include", "pgx.h")).read()
    assert re.search(r"int64_t\s+frag;\s*uint32_t\s+pair_score,\s*solo_score,\s*cand_a,\s*cand_b,\s*solo_a,\s*solo_b,\s*n_compatible,\s*n_best,\s*next_score,"
                     r"\s*pair_matches,\s*seq_a,\s*seq_b,\s*flags,\s*reserved;\s*\}\s*pgx_read_mates;", header)
    for name, value in (("ELECT", P.MATES_ELECT), ("PROPER", M.PROPER), ("COMPATIBLE", M.COMPATIBLE), ("HAS_A", M.HAS_A), ("HAS_B", M.HAS_B), ("MOVED_A", M.MOVED_A),
                        ("MOVED_B", M.MOVED_B)):
        m = re.search(r"^#define\s+PGX_MATES_%s\s+(\d+)u" % name, header, re.M)
        assert m and int(m.group(1)) == value, name
    assert (P.MATES_PROPER, P.MATES_COMPATIBLE, P.MATES_HAS_A, P.MATES_HAS_B, P.MATES_MOVED_A, P.MATES_MOVED_B) == (1, 2, 4, 8, 16, 32)


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
        P.read_mates_arrays(0, [10, 10], np.zeros(3, np.uint64), np.zeros(0, P.VERIFY_DTYPE), 0, 500, 8)
    assert e.value.code == P.ERR_NO_DEVICE
    assert L.pgx_batch_read_mates(None, 0, 500, 8, 0, None) == P.ERR_NO_DEVICE
    out = P.ReadMatesResult()
    assert L.pgx_batch_mated(None, ctypes.byref(out)) == P.ERR_ARG and L.pgx_batch_device_mated(None, ctypes.byref(out)) == P.ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table
def test_the_collection_and_the_pinned_counts():
    assert C.lens[0::2] == C.lens[1::2] == list(MC.FORWARD_LENGTHS) == [1200, 1500, 900, 2000, 700, 64]
    assert all(C.seqs[q + 1] == MC.rc(C.seqs[q]) for q in range(0, 12, 2)) and M.is_twinned(C.lens) is None
    for p, (c1, c2) in enumerate(MC.COPIES):
        s = C.seqs[2 * p]
        assert c2 - c1 >= 600 and s[c1:c1 + 100] == s[c2:c2 + 100] and C.raw.count(s[c1:c1 + 100]) == 2
        assert C.copies(2 * p) == (c1, c2) and C.seqs[2 * p + 1][C.copies(2 * p + 1)[0]:][:100] == MC.rc(s[c2:c2 + 100])
    kinds = {k: C.kinds.count(k) for k in set(C.kinds)}
    assert kinds == MC.KIND_COUNTS and all(v >= 10 for v in kinds.values()) and len(C.pairs) == 162 and len(C.reads) == 324
    assert all(len(r) == 50 for p in C.pairs for r in (p["a"], p["b"]) if not (p["kind"] == "orphan" and r == b""))
    for kind in ("repeat_a", "repeat_b"):  # the same number at each copy
        assert [sum(p["kind"] == kind and p["which"] == w for p in C.pairs) for w in (0, 1)] == [8, 8]
    rev = [p for p in C.pairs if p["kind"] == "reverse"]
    assert all(p["truth_a"][0] % 2 == 1 for p in rev) and [sum(p["which"] == w for p in rev) for w in (None, 0, 1)] == [6, 8, 8]
    assert sorted({p["frag"] for p in C.pairs if p["kind"] == "border"}) == [149, 150, 500, 501]
    assert all(p["frag"] == 950 for p in C.pairs if p["kind"] == "far")
    assert all(p["truth_a"][0] // 2 != p["truth_b"][0] // 2 for p in C.pairs if p["kind"] == "cross")
    assert all(p["truth_a"][0] == p["truth_b"][0] for p in C.pairs if p["kind"] == "same_strand")
    hang = [p for p in C.pairs if p["kind"] == "hang"]
    assert sorted(-min(p["truth_a"][1], p["truth_b"][1]) for p in hang) == sorted(MC.HANGS * 8) and {p["truth_a"][0] for p in hang} == {0, 9, 10, 11}
    assert sum(p["truth_a"][1] < 0 for p in hang) == sum(p["truth_b"][1] < 0 for p in hang) == 12


@pytest.fixture(scope="module")
def chain(workdir):
    """the verify list of every read at max_cand 16, penalty 4, from the oracle's MEMs, located, through place_emu and verify_emu"""
    path = os.path.join(workdir, "mates_cases.txt")
    with open(path, "wb") as f:
        f.write(C.raw)
    ri = W.build_index_from_text(path, workdir, "mates_cases", with_tags=False)[0]
    orc = O.RIndex(ri)
    L = int(P.Index(ri, mode=P.MODE_STRICT).info().max_length)
    mems, mem_off, values, loc_off = [], [0], [], [0]
    for read in C.reads:
        for m in orc.find_all_mems(read, MC.MIN_LEN, 1, O.MODE_STRICT):
            mems.append(m)
            values += [int(v) for v in orc.locate_sa(m[2], m[2] + m[3] - 1, O.MODE_STRICT)]
            loc_off.append(len(values))
        mem_off.append(len(mems))
    marr = np.zeros(len(mems), E.MEM_DTYPE)
    for k, m in enumerate(mems):
        marr[k] = m
    place = E.read_place(np.array(mem_off, np.uint64), marr, np.array(loc_off, np.uint64), np.array(values, np.uint64), L)
    return V.read_verify(C.seqs, C.reads, V.candidates_from_places(place, 16), 4)


def _winner(rec):
    return None if int(rec["seq"]) == V.NO_SEQUENCE else (int(rec["seq"]), int(rec["diag"]))


def _truths():
    out = []
    for p in C.pairs:
        out += [p["truth_a"], p["truth_b"]]
    return out


def test_both_copies_of_a_repeat_are_candidates(chain):
    """a read wholly inside an exact repeat is one MEM with two occurrences: two candidates that tie in coverage and in verify"""
    n = 0
    for k, p in enumerate(C.pairs):
        if p["which"] is None:
            continue
        inside = 2 * k + (0 if p["mate"] == "a" else 1)
        mine = chain["cands"][int(chain["cand_offsets"][inside]):int(chain["cand_offsets"][inside + 1])]
        q, diag = _truths()[inside]
        c = C.copies(q)
        other = diag + (c[1] - c[0]) * (1 if p["which"] == 0 else -1)
        assert [(int(x["seq"]), int(x["diag"])) for x in mine] == sorted([(q, diag), (q, other)]), (k, p["kind"])
        assert int(mine[0]["seg_score"]) == int(mine[1]["seg_score"]) == int(mine[0]["matches"]) == int(mine[1]["matches"]) == 50
        assert int(chain["reads"][inside]["n_tied"]) == 2 and int(chain["reads"][inside]["cand_index"]) == 0
        n += 1
    assert n == 48
    # and every other read with a truth has that one candidate alone; the orphans' B mates have none
    for r, t in enumerate(_truths()):
        if C.pairs[r // 2]["which"] is None and C.kinds[r // 2] not in ("tie", "below"):
            mine = chain["cands"][int(chain["cand_offsets"][r]):int(chain["cand_offsets"][r + 1])]
            assert [(int(x["seq"]), int(x["diag"])) for x in mine] == ([t] if t else []), (r, C.kinds[r // 2])


def test_the_election_places_every_repeat_mate_where_verify_alone_misses_the_second_copy(chain):
    res = M.read_mates(C.lens, chain["cand_offsets"], chain["cands"], MC.FRAG_MIN, MC.FRAG_MAX, 10, M.ELECT)
    truths = _truths()
    missed_before, second_copy = [], []
    for k, p in enumerate(C.pairs):
        if p["kind"] not in ("repeat_a", "repeat_b", "reverse", "hang", "unique"):
            continue
        for r in (2 * k, 2 * k + 1):
            assert _winner(res["winners"][r]) == truths[r], (k, p["kind"])
            if _winner(chain["reads"][r]) != truths[r]:
                missed_before.append(r)
        if p["which"] == 1:
            second_copy.append(k)
        assert int(res["pairs"][k]["flags"]) & M.PROPER and int(res["pairs"][k]["frag"]) == p["frag"]
    assert sorted(r // 2 for r in missed_before) == second_copy and len(second_copy) == 24
    # the two classes where the pair overrules verify without a repeat tie to break: `tie` moves B to its second candidate, `below` moves A off its solo winner
    tie, below = ([k for k, kind in enumerate(C.kinds) if kind == x] for x in ("tie", "below"))
    for k in tie + below:
        rec, p = res["pairs"][k], C.pairs[k]
        assert [_winner(res["winners"][r]) for r in (2 * k, 2 * k + 1)] == [p["truth_a"], p["truth_b"]] and int(rec["frag"]) == p["frag"], (k, p["kind"])
        if p["kind"] == "tie":
            assert (int(rec["cand_a"]), int(rec["cand_b"]), int(rec["n_best"]), int(rec["n_compatible"])) == (0, 1, 2, 2) and int(rec["pair_score"]) == int(rec["solo_score"]) == 100
            assert int(rec["flags"]) == M.PROPER | M.COMPATIBLE | M.HAS_A | M.HAS_B | M.MOVED_B
        else:
            assert (int(rec["cand_a"]), int(rec["solo_a"]), int(rec["n_compatible"])) == (0, 1, 1) and int(rec["solo_score"]) == 95
            assert 88 <= int(rec["pair_score"]) < 95 and int(rec["flags"]) == M.PROPER | M.COMPATIBLE | M.HAS_A | M.HAS_B | M.MOVED_A
    moved = ((res["pairs"]["flags"] & (M.MOVED_A | M.MOVED_B)) != 0)
    assert sorted(np.flatnonzero(moved)) == sorted(second_copy + tie + below) and (res["n_moved_a"], res["n_moved_b"]) == (22, 22)
    for k, p in enumerate(C.pairs):  # the classes that no pair fits keep their solo winners, bit for bit
        if p["kind"] in ("far", "cross", "same_strand", "orphan"):
            assert not int(res["pairs"][k]["flags"]) & M.COMPATIBLE, (k, p["kind"])
            assert res["winners"][2 * k:2 * k + 2].tobytes() == chain["reads"][2 * k:2 * k + 2].tobytes()
    strict = M.read_mates(C.lens, chain["cand_offsets"], chain["cands"], MC.BORDER_FRAG_MIN, MC.FRAG_MAX, 10)
    for k, p in enumerate(C.pairs):
        if p["kind"] == "border":
            assert bool(int(strict["pairs"][k]["flags"]) & M.PROPER) == (150 <= p["frag"] <= 500), (k, p["frag"])
            assert bool(int(res["pairs"][k]["flags"]) & M.PROPER) == (p["frag"] <= 500)


# ---------------------------------------------------------------------------------------------------------------------------------
# mutations of the emulator: each changes records of the class it targets
MUTATION_COUNTS = {  # mutation -> (frag_min, penalty, class, records of the class that change)
    "no_twin": (0, 10, "same_strand", 6),      # the twin test dropped: two reads on one strand become a pair where L - 2 f - I + 50 falls inside the bounds
    "same_seq": (0, 10, "unique", 12),         # seq ^ 1 replaced by seq: no proper pair is left
    "diag_sign": (0, 10, "unique", 11),        # the sign of B's diag flipped: frag is off by twice that diag (the twelfth pair has B at diag 0)
    "lt_min": (150, 10, "border", 3),          # < at the lower bound: the pairs at exactly frag_min
    "lt_max": (150, 10, "border", 3),          # < at the upper bound: the pairs at exactly frag_max
    "tie_swap": (0, 10, "tie", 10),            # i and j swapped in the tie order: (1, 0) is chosen where (0, 1) ties with it
    "no_penalty": (0, 10, "below", 10),        # U ignored: the one compatible pair scores below the solo winners and is dropped
}


@pytest.mark.parametrize("mutation", list(MUTATION_COUNTS))
def test_each_mutation_changes_its_class(chain, mutation):
    frag_min, penalty, kind, count = MUTATION_COUNTS[mutation]
    good = M.read_mates(C.lens, chain["cand_offsets"], chain["cands"], frag_min, MC.FRAG_MAX, penalty)["pairs"]
    bad = M.read_mates(C.lens, chain["cand_offsets"], chain["cands"], frag_min, MC.FRAG_MAX, penalty, mutation=mutation)["pairs"]
    changed = [k for k in range(len(C.pairs)) if good[k] != bad[k] and C.kinds[k] == kind]
    print("%s: %d records of class %s change" % (mutation, len(changed), kind))
    assert len(changed) == count > 0
