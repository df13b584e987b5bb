"""GPU tier of the read walk at its borders: pgx_read_walk_arrays (the count and fill kernels of pgx_batch_read_walk on an image made from stated
path tables) against tests/walk_emu.py, byte for byte: records and step list with PGX_WALK_STEPS, the same records without.  No index.

The image has one bit per text position in u64 words and a rank directory entry per 512 positions (PGX_WALK_BLOCK_BITS, csrc/pgx_image.h);
the fill kernel gives a read PGX_WALK_FILL_LANES = 8 lanes.  The tables put stretch starts and ends on every bit residue on both sides of
every word and directory border of a 2 kb text; visits of 1, 1023 and 1024 symbols; 1024 one-bp visits behind a 1024-bp one (LAYOUT_A /
LAYOUT_B of tests/build_tags_cases.py, whose starts lie on 1024 k - 1, 1024 k, 1024 k + 1); first and last visits, whole sequences,
sequences of length 1, empty sequences first, between and last, a last visit that ends with the text; empty stretches and
PGX_NO_SEQUENCE; reads of 1, 7, 8, 9 and 2000 steps; empty inputs; 70 028 reads of three symbols (more than one block of every kernel, no
multiple of 256 or of 32); every refusal with untouched outputs and a steps_cap one too small."""
import numpy as np
import pytest

import build_tags_cases as B
import pgx_ffi as P
import walk_emu as E

pytestmark = pytest.mark.gpu
WORD, BLOCK, LANES = 64, 512, 8


def _tables(cuts):
    """(seq_offsets, visit_offsets, visit_nodes, visit_length): a node id per visit, except that every fifth visit repeats the id before it; the
    orientation bit alternates"""
    so, vo, vn, vl = [0], [0], [], []
    for cut in cuts:
        for ln in cut:
            k = len(vn)
            vn.append(vn[-1] ^ 1 if k % 5 == 4 else ((k + 1) << 1) | (k & 1))
            vl.append(ln)
        so.append(so[-1] + sum(cut))
        vo.append(len(vn))
    return np.array(so, np.uint64), np.array(vo, np.uint64), np.array(vn, np.uint64), np.array(vl, np.uint32)


def _check(tab, seq, ts, te):
    so, vo, vn, vl = tab
    want = E.read_walk(vo, vn, vl, seq, ts, te)
    got = P.read_walk_arrays(0, so, vo, vn, vl, seq, ts, te, flags=P.WALK_STEPS)
    assert got["reads"].tobytes() == want["reads"].tobytes()
    assert np.array_equal(got["step_offsets"], want["step_offsets"]) and np.array_equal(got["steps"], want["steps"])
    bare = P.read_walk_arrays(0, so, vo, vn, vl, seq, ts, te)
    assert bare["reads"].tobytes() == want["reads"].tobytes() and bare["step_offsets"] is None and bare["steps"] is None
    return want


def _residue_cuts():
    rng = np.random.default_rng(512)
    cuts, total = [[]], 0
    while total < 4 * BLOCK + 70:  # directory borders at 512, 1024, 1536 and 2048 inside sequences, a few sequence ends between them
        cut = [int(x) for x in rng.integers(1, 71, size=int(rng.integers(3, 12)))]
        cuts.append(cut)
        total += sum(cut)
    return cuts + [[]]


def test_every_residue_on_both_sides_of_every_border():
    tab = _tables(_residue_cuts())
    so = tab[0]
    assert int(so[-1]) > 4 * BLOCK
    seq, ts, te = [], [], []
    for q in range(len(so) - 1):
        ls = int(so[q + 1] - so[q])
        for a in range(ls):
            for ln in (1, 2, 63, 64, 65, 127, 128, 129, ls - a):
                if a + ln <= ls:
                    seq.append(q); ts.append(a); te.append(a + ln)
    g0 = np.array(ts) + so[np.array(seq)].astype(np.int64)
    g1 = np.array(te) + so[np.array(seq)].astype(np.int64)
    for border in range(WORD, int(so[-1]), WORD):  # a start and an end on every residue within a word of every border that is not a sequence end
        inside = [(border - WORD <= g) & (g < border + WORD) for g in (g0, g1)]
        assert all(len(set((g[m] % WORD).tolist())) == WORD for g, m in zip((g0, g1), inside)), border
    assert all(((g0 < b) & (g1 > b)).any() for b in range(BLOCK, int(so[-1]), BLOCK))  # and stretches across every directory border
    want = _check(tab, seq, ts, te)
    assert int(want["reads"]["n_steps"].max()) > LANES and int(want["reads"]["n_steps"].min()) == 1


LONG_CUTS = [[], [1], [1023], [1024], [1024, 1], [], [1, 1024], [1023, 1024], B.LAYOUT_A, B.LAYOUT_B, [1] * 2500, [1], []]
OFFSETS = (0, 1, 2, 1022, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2050, 3071, 3072, 3073, 3500, 4095, 4096, 4097, 5118, 5119, 5120, 5121, 5122, 6144, 6145)


def test_long_visits_and_buckets_of_short_ones():
    tab = _tables(LONG_CUTS)
    so, vo, _, vl = tab
    seq, ts, te = [], [], []
    for q in range(len(so) - 1):
        ls = int(so[q + 1] - so[q])
        offs = sorted({o for o in OFFSETS if o <= ls} | {ls, max(ls - 1, 0)})
        for i, a in enumerate(offs):
            for b in offs[i:]:  # (a == b: an empty stretch, also on an empty sequence and behind a sequence's last symbol)
                seq.append(q); ts.append(a); te.append(b)
        first, last = int(vl[int(vo[q])]) if vo[q] < vo[q + 1] else 0, int(vl[int(vo[q + 1]) - 1]) if vo[q] < vo[q + 1] else 0
        seq += [q, q, q]; ts += [0, ls - last, 0]; te += [first, ls, ls]  # the first visit, the last one, the whole sequence
    ones = LONG_CUTS.index([1] * 2500)
    for steps in (1, LANES - 1, LANES, LANES + 1, 2000):
        seq.append(ones); ts.append(100); te.append(100 + steps)
    seq += [P.NO_SEQUENCE, P.NO_SEQUENCE]; ts += [0, 5]; te += [0, 9]
    want = _check(tab, seq, ts, te)
    steps = want["reads"]["n_steps"]
    assert {1, LANES - 1, LANES, LANES + 1, 2000} <= set(steps.tolist()) and int(steps.max()) == 2500
    assert int(want["reads"]["path_len"].max()) == 6145 and (want["reads"]["seq"] == P.NO_SEQUENCE).sum() == 2
    assert int(so[-1]) == int(so[-2]) and vl[-1] == 1  # the last visit ends with the text, behind it one empty sequence


def test_many_short_reads_and_empty_inputs():
    tab = _tables([[2, 1, 3, 1, 1, 5, 4, 1, 2], [], [3, 3, 1]])
    n = 70028
    r = np.arange(n)
    seq = np.where(r % 3 == 2, 2, 0)
    ls = np.where(seq == 2, 7, 20)
    ts = r % (ls - 2)
    want = _check(tab, seq, ts, ts + 3)
    assert set(want["reads"]["n_steps"].tolist()) == {1, 2, 3}
    for t in (tab, _tables([])):  # no reads; no reads and no sequences
        got = P.read_walk_arrays(0, *t, [], [], [], flags=P.WALK_STEPS)
        assert len(got["reads"]) == 0 and got["step_offsets"].tolist() == [0] and len(got["steps"]) == 0
    got = P.read_walk_arrays(0, *_tables([[], []]), [0, 1], [0, 0], [0, 0], flags=P.WALK_STEPS)  # sequences, but no visit at all
    assert got["reads"].tolist() == [(0, 0, 0, 0, 0), (0, 0, 0, 0, 1)] and got["step_offsets"].tolist() == [0, 0, 0]


def test_refusals_leave_the_outputs_alone():
    so, vo, vn, vl = _tables([[4, 3, 5], [2]])
    good = dict(seq=[0, 1, 0], ts=[1, 0, 4], te=[9, 2, 12])

    def refused(code, words, tab=(so, vo, vn, vl), flags=P.WALK_STEPS, cap=None, **reads):
        k = dict(good, **reads)
        out = dict(reads=np.full(3, 0x55, dtype=np.uint8).repeat(32).view(P.WALK_DTYPE), step_offsets=np.full(4, 77, np.uint64), steps=np.full(16, 99, np.uint64))
        with pytest.raises(P.PgxError) as e:
            P.read_walk_arrays(0, *tab, k["seq"], k["ts"], k["te"], flags=flags, steps_cap=cap, out=out)
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)
        assert (out["reads"].view(np.uint8) == 0x55).all() and (out["step_offsets"] == 77).all() and (out["steps"] == 99).all()

    refused(P.ERR_ARG, ["unknown flag"], flags=2)
    refused(P.ERR_ARG, ["visit 1 of sequence 0", "length 0"], tab=(so, vo, vn, np.array([4, 0, 8, 2], np.uint32)))
    refused(P.ERR_ARG, ["visit 2 of sequence 0", "1025"], tab=(np.array([0, 1032, 1034], np.uint64), vo, vn, np.array([4, 3, 1025, 2], np.uint32)))
    refused(P.ERR_ARG, ["sequence 1", "sum to 2", "has 3"], tab=(np.array([0, 12, 15], np.uint64), vo, vn, vl))
    refused(P.ERR_ARG, ["read 2", "[4, 13)", "12 symbols"], te=[9, 2, 13])
    refused(P.ERR_ARG, ["read 1", "[2, 1)"], ts=[1, 2, 4], te=[9, 1, 12])
    refused(P.ERR_ARG, ["read 1", "not below n_seq 2"], seq=[0, 2, 0])
    refused(P.ERR_ARG, ["seq_offsets must start at 0"], tab=(np.array([1, 12, 14], np.uint64), vo, vn, vl))
    refused(P.ERR_ARG, ["visit_offsets decrease at sequence 1"], tab=(so, np.array([0, 3, 2], np.uint64), vn, vl))
    want = E.read_walk(vo, vn, vl, good["seq"], good["ts"], good["te"])
    need = len(want["steps"])
    assert need == 3 + 1 + 2
    refused(P.ERR_NOMEM, ["%d steps" % need, "steps_cap is %d" % (need - 1)], cap=need - 1)
    got = P.read_walk_arrays(0, so, vo, vn, vl, good["seq"], good["ts"], good["te"], flags=P.WALK_STEPS, steps_cap=need)
    assert np.array_equal(got["steps"], want["steps"]) and got["reads"].tobytes() == want["reads"].tobytes()
