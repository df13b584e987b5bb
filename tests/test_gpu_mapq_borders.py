"""GPU tier of pgx_read_mapq_arrays: the mapq kernel on stated tables, at the smallest shapes that can go wrong, against tests/mapq_emu.py and against
values worked out by hand.  Reads with 0, 1, 2, 63 and 64 entries, all 64 in one class and 64 classes of one; 0, 1, 2 and 65 reads (66 as pairs) at
1, 2 and 64 lanes a read, so that groups straddle a wave and the last group is partial; scale * d of 48, 49 and 50 and a d whose product with scale
needs 64 bits; paired sums beyond 32 bits and a negative paired score; a rescue n_best of 2^32 - 1; nodes of 1 and 1024 symbols with the anchor on
the first and last base of a node and of a sequence; entries whose span excludes the anchor; an entry on the twin strand; a stated chosen that is
not the best; slack 0, 1 and 1024; and every refusal with its message."""
import numpy as np
import pytest

import mapq_emu as Q
import pgx_ffi as P
import rescue_emu as R

pytestmark = pytest.mark.gpu
NO = Q.NO_CHOSEN


def _tables(seq_nodes):
    """seq_nodes: per sequence a list of (node << 1 | rev, length): (seq_offsets, visit_offsets, visit_nodes, visit_length)"""
    so, vo, vn, vl = [0], [0], [], []
    for nodes in seq_nodes:
        vn += [n for n, _ in nodes]
        vl += [ln for _, ln in nodes]
        so.append(so[-1] + sum(ln for _, ln in nodes))
        vo.append(len(vn))
    return np.array(so, np.uint64), np.array(vo, np.uint64), np.array(vn, np.uint64), np.array(vl, np.uint32)


def _entry(seq, diag, score, lo=0, hi=50, seg_start=0):
    return dict(seq=seq, diag=diag, seg_score=score, matches=min(score, 50), span_lo=lo, span_hi=hi, seg_start=seg_start)


def _pack(per_read):
    offs = np.zeros(len(per_read) + 1, np.uint64)
    flat = []
    for r, items in enumerate(per_read):
        flat += items
        offs[r + 1] = len(flat)
    out = np.zeros(len(flat), Q.VERIFY_DTYPE)
    for k, e in enumerate(flat):
        for f, v in e.items():
            out[k][f] = v
    return offs, out


def _both(tables, per_read, chosen, list_len=None, rescue=None, paired=None, scale=2, slack=8):
    """(device records, emulator records), held equal"""
    so, vo, vn, vl = tables
    offs, ent = _pack(per_read)
    chosen = np.array(chosen, np.uint32)
    kw = dict(frag_min=paired["frag_min"], frag_max=paired["frag_max"], penalty=paired["penalty"], flags=P.MAPQ_PAIRED) if paired else {}
    got = P.read_mapq_arrays(0, so, vo, vn, vl, offs, ent, chosen, rescue=rescue, list_len=list_len, scale=scale, slack=slack, **kw)
    pe = dict(paired, seq_lengths=np.diff(so.astype(np.int64))) if paired else None
    exp = Q.read_mapq(vo, vn, vl, offs, ent, chosen, list_len=list_len, rescue=rescue, paired=pe, scale=scale, slack=slack)["records"]
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (len(bad), int(bad[0]), got[bad[0]], exp[bad[0]])
    return got, exp


# two paths, both strands: nodes 1 (1 symbol), 2 (1024), 3 (1), 4 (24) and 1, 5 (1024), 3, 4: sequences of 1050 symbols
TWO = _tables([[(2, 1), (4, 1024), (6, 1), (8, 24)], [(9, 24), (7, 1), (5, 1024), (3, 1)], [(2, 1), (10, 1024), (6, 1), (8, 24)], [(9, 24), (7, 1), (11, 1024), (3, 1)]])


def _random_case(rng, n_reads, sizes=(0, 1, 2, 63, 64), n_seq=4, ls=1050):
    per_read, chosen, list_len = [], [], []
    for r in range(n_reads):
        k = int(sizes[int(rng.integers(0, len(sizes)))])
        items = []
        for _ in range(k):
            diag = int(rng.integers(-40, ls - 10))
            lo, hi = max(0, -diag), min(50, ls - diag)
            items.append(_entry(int(rng.integers(0, n_seq)), diag, int(rng.integers(0, 60)), lo, hi, seg_start=int(rng.integers(lo, hi))))
        nl = int(rng.integers(0, k + 1))
        per_read.append(items)
        list_len.append(nl)
        chosen.append(int(rng.integers(0, nl)) if nl and rng.integers(0, 8) else NO)
    return per_read, chosen, np.array(list_len, np.uint32)


@pytest.mark.parametrize("lanes", ["1", "2", "64"])
def test_group_sizes_read_counts_and_list_lengths(lanes, monkeypatch):
    monkeypatch.setenv("PGX_MAPQ_LANES", lanes)
    rng = np.random.default_rng(511)
    for n_reads in (0, 1, 2, 65):
        for sizes in ((0, 1), (0, 1, 2), (0, 1, 2, 63, 64)):  # (lists of at most 1: G is what the knob says, 1 included; of at most 2: G >= 2)
            per_read, chosen, list_len = _random_case(rng, n_reads, sizes)
            got, _ = _both(TWO, per_read, chosen, list_len, slack=int(rng.integers(0, 12)))
            assert len(got) == n_reads
    for n_reads in (0, 2, 66):  # as pairs
        for sizes in ((0, 1), (0, 1, 2, 3) if lanes != "64" else (0, 1, 2, 63, 64)):
            per_read, chosen, list_len = _random_case(rng, n_reads, sizes)
            _both(TWO, per_read, chosen, list_len, paired=dict(frag_min=-100, frag_max=700, penalty=int(rng.integers(0, 30))))


def test_65_reads_at_one_lane_a_read(monkeypatch):
    """G = 1: no read has more than one entry, so PGX_MAPQ_LANES=1 is what the kernel runs with: 64 reads a wave, the 65th alone in the second wave, every lane
    storing the 8 words of its record in 8 rounds; as pairs 66 reads, 33 groups.  Every read has its entry here, and the records are not all alike"""
    monkeypatch.setenv("PGX_MAPQ_LANES", "1")
    rng = np.random.default_rng(65)
    for n_reads, paired in ((65, None), (66, dict(frag_min=-100, frag_max=700, penalty=7))):
        per_read, chosen, list_len = _random_case(rng, n_reads, (1,))
        assert max(len(x) for x in per_read) == 1
        got, _ = _both(TWO, per_read, chosen, list_len, paired=paired)
        assert len(got) == n_reads and 0 < int((got["flags"] & Q.HAS != 0).sum()) < n_reads and int(got[64]["n_entries"]) == (1 if chosen[64] != NO else 0)


def test_one_class_of_64_and_64_classes_of_one():
    same = [_entry(2 * (k % 2), 1030, 30 + k % 5, 0, 20) for k in range(64)]  # node 4 at offset 4, on either path
    got, _ = _both(TWO, [same], [7])
    assert tuple(got[0]) == (60, Q.HAS | Q.LOCUS, 64, 1, 64, 0, 0, 0)
    apart = [_entry(0, 1 + 15 * k, 50 - (k % 3)) for k in range(64)]  # node 2 at 64 offsets
    got, _ = _both(TWO, [apart], [0], scale=1)
    assert (int(got[0]["n_loci"]), int(got[0]["n_competing"]), int(got[0]["n_with"]), int(got[0]["best_other"])) == (64, 63, 1, 50)
    assert int(got[0]["excess"]) == 21 * Q.T[0] + 21 * Q.T[1] + 21 * Q.T[2] and int(got[0]["mapq"]) == 0
    got, _ = _both(TWO, [apart], [0], slack=15)  # the neighbour at 15 diagonals is adjacent, the others compete
    assert (int(got[0]["n_competing"]), int(got[0]["n_with"])) == (62, 2)
    got, _ = _both(TWO, [apart], [0], slack=150)  # 15 k <= 150: k <= 10
    assert (int(got[0]["n_competing"]), int(got[0]["n_with"])) == (53, 11)


def test_the_weight_table_at_its_end_and_products_beyond_32_bits():
    for d, excess, mapq in ((48, 1, 48), (49, 0, 60), (50, 0, 60)):
        got, _ = _both(TWO, [[_entry(0, 100, 100), _entry(0, 500, 100 - d)]], [0], scale=1)
        assert (int(got[0]["excess"]), int(got[0]["mapq"]), int(got[0]["n_competing"])) == (excess, mapq, 1), d
    got, _ = _both(TWO, [[_entry(0, 100, 24), _entry(0, 500, 0)]], [0], scale=2)
    assert (int(got[0]["excess"]), int(got[0]["mapq"])) == (1, 48)
    got, _ = _both(TWO, [[_entry(0, 100, 1 << 28), _entry(0, 500, 0)]], [0], scale=16)  # 16 * 2^28 = 2^32: 0 in 32 bits
    assert (int(got[0]["excess"]), int(got[0]["mapq"])) == (0, 60)
    got, _ = _both(TWO, [[_entry(0, 100, 0xFFFFFFFF), _entry(0, 500, 0xFFFFFFFE)]], [0], scale=16)
    assert (int(got[0]["excess"]), int(got[0]["best_other"])) == (Q.T[16], 0xFFFFFFFE)
    # paired sums beyond 32 bits: A's two copies, the second with the compatible mate
    big = 0xFFFFFFFF
    reads = [[_entry(0, 100, big), _entry(0, 600, big)], [_entry(1, 1050 - 600 - 300, big)]]
    got, _ = _both(TWO, reads, [1, 0], paired=dict(frag_min=0, frag_max=400, penalty=3))
    assert (int(got[0]["excess"]), int(got[0]["best_other"]), int(got[0]["flags"])) == (Q.T[6], big, Q.HAS | Q.LOCUS | Q.PAIRED)  # 2 big against 2 big - 3, held at 2^32 - 1
    # a negative paired score: no compatible candidate and a large U
    reads = [[_entry(0, 100, 5), _entry(0, 600, 4)], [_entry(1, 900, 7)]]
    got, exp = _both(TWO, reads, [0, 0], paired=dict(frag_min=0, frag_max=40, penalty=1000))
    assert (int(got[0]["best_other"]), int(got[0]["excess"]), int(got[0]["n_competing"])) == (0, Q.T[2], 1)  # 4 + 7 - 1000 < 0: held at 0


def test_the_rescue_terms_and_a_window_of_ties_beyond_32_bits():
    resc = np.zeros(2, R.RESCUE_DTYPE)
    resc[0]["flags"], resc[0]["n_best"], resc[0]["seg_score"], resc[0]["next_score"] = R.TARGET | R.RESCUED, 0xFFFFFFFF, 40, 39
    resc[1]["flags"], resc[1]["n_best"], resc[1]["seg_score"], resc[1]["next_score"] = R.TARGET | R.RESCUED, 1, 40, 16
    reads = [[_entry(0, 100, 40)], [_entry(0, 100, 33), _entry(0, 600, 40)]]
    got, _ = _both(TWO, reads, [0, 1], rescue=resc)
    assert (int(got[0]["excess"]), int(got[0]["mapq"]), int(got[0]["flags"])) == (0xFFFFFFFF, 0, Q.HAS | Q.LOCUS | Q.RESCUED)
    assert (int(got[1]["excess"]), int(got[1]["mapq"]), int(got[1]["flags"])) == (Q.T[14] + Q.T[48], 14, Q.HAS | Q.LOCUS | Q.RESCUED)  # 2609 + 1: 10 log10(68146 / 2610) = 14.2
    got, _ = _both(TWO, reads, [0, 0], rescue=resc)  # the chosen entry of the second read is not its last
    assert int(got[1]["flags"]) == Q.HAS | Q.LOCUS | Q.OUTSCORED and int(got[1]["excess"]) == Q.T[0]


def test_the_anchor_at_the_borders_of_nodes_and_sequences():
    # read position 0 on the first base of a sequence (node 1, 1 symbol), the last base of node 2 / 5, node 3 (1 symbol), and the last base of the sequence
    for diag, n_loci in ((0, 1), (1, 2), (1024, 2), (1025, 1), (1026, 1), (1049, 1)):
        hi = min(50, 1050 - diag)
        got, _ = _both(TWO, [[_entry(0, diag, 30, 0, hi), _entry(2, diag, 30, 0, hi)]], [0])
        assert (int(got[0]["n_loci"]), int(got[0]["flags"])) == (n_loci, Q.HAS | Q.LOCUS), diag
    # a read that hangs over the start: the anchor is the first position inside
    got, _ = _both(TWO, [[_entry(0, -7, 30, 7, 50, seg_start=7), _entry(2, -7, 30, 7, 50, seg_start=9)]], [0])
    assert int(got[0]["n_loci"]) == 1
    got, _ = _both(TWO, [[_entry(0, -7, 30, 7, 50, seg_start=9), _entry(2, -7, 30, 7, 50, seg_start=9)]], [0])  # two bases on: node 2 against node 5
    assert int(got[0]["n_loci"]) == 2
    # spans that exclude the anchor: before it, behind it, empty; each is a class of its own
    items = [_entry(0, 100, 30, 0, 50, seg_start=20), _entry(0, 100, 30, 21, 50), _entry(0, 100, 30, 0, 20), _entry(0, 100, 30, 0, 0), _entry(0, 100, 30, 20, 21)]
    got, _ = _both(TWO, [items], [0])
    assert (int(got[0]["n_loci"]), int(got[0]["n_competing"]), int(got[0]["n_with"])) == (4, 3, 2)
    got, _ = _both(TWO, [items], [3])  # the chosen entry has no locus itself
    assert (int(got[0]["flags"]), int(got[0]["n_loci"]), int(got[0]["n_with"])) == (Q.HAS, 4, 1)
    # the twin strand: the same node in the other orientation is another place
    got, _ = _both(TWO, [[_entry(0, 100, 30), _entry(1, 1050 - 100 - 50, 30)]], [0])
    assert (int(got[0]["n_loci"]), int(got[0]["mapq"])) == (2, 3)
    # a stated chosen that is not the best, and no chosen at all
    got, _ = _both(TWO, [[_entry(0, 100, 30), _entry(0, 600, 31)], [_entry(0, 100, 30)]], [0, NO])
    assert int(got[0]["flags"]) == Q.HAS | Q.LOCUS | Q.OUTSCORED and tuple(got[1]) == (0,) * 8


@pytest.mark.parametrize("slack", [0, 1, 1024])
def test_slack(slack):
    items = [_entry(0, 0, 30), _entry(0, 1, 29), _entry(0, -1, 29, 1, 50), _entry(0, 1024, 29, 0, 20), _entry(0, 1025, 29, 0, 20), _entry(2, 1, 29)]  # six places
    got, _ = _both(TWO, [items], [0], slack=slack)
    assert int(got[0]["n_with"]) == {0: 1, 1: 3, 1024: 4}[slack] and int(got[0]["n_competing"]) == 6 - int(got[0]["n_with"])


def test_every_refusal_names_the_first_offender():
    so, vo, vn, vl = TWO
    offs, ent = _pack([[_entry(0, 100, 30)], [_entry(1, 100, 30)]])
    chosen = np.array([0, 0], np.uint32)
    out = np.full(2, 7, dtype=P.MAPQ_DTYPE)

    def refused(text, code=P.ERR_ARG, **kw):
        args = dict(seq_offsets=so, visit_offsets=vo, visit_nodes=vn, visit_length=vl, entry_offsets=offs, entries=ent, chosen=chosen)
        args.update(kw)
        with pytest.raises(P.PgxError) as e:
            P.read_mapq_arrays(0, out=out, **args)
        assert e.value.code == code and text in str(e.value), str(e.value)
        assert (out["mapq"] == 7).all()  # nothing written

    refused("unknown flag", flags=1)
    refused("scale 0 is outside 1 .. 16", scale=0)
    refused("scale 17 is outside 1 .. 16", scale=17)
    refused("slack 1025 exceeds 1024", slack=1025)
    refused("seq_offsets must start at 0", seq_offsets=so + np.uint64(1))
    refused("visit_offsets decrease at sequence 1", visit_offsets=np.array([0, 4, 3, 12, 16], np.uint64))
    bad = vl.copy(); bad[1] = 1025
    refused("visit 1 of sequence 0 has length 1025, outside 1 .. 1024", visit_length=bad)
    bad = vl.copy(); bad[3] = 23
    refused("the visits of sequence 0 sum to 1049 symbols, the sequence has 1050", visit_length=bad)
    refused("entry_offsets decrease at read 1", entry_offsets=np.array([0, 2, 1], np.uint64))
    e2 = ent.copy(); e2[1]["seq"] = 4
    refused("entry 0 of read 1 has seq 4, not below n_seq 4", entries=e2)
    e2 = ent.copy(); e2[1]["diag"] = 1020
    refused("entry 0 of read 1 has the span [0, 50) at diag 1020, its sequence has 1050 symbols", entries=e2)
    e2 = ent.copy(); e2[0]["diag"] = -1
    refused("entry 0 of read 0 has the span [0, 50) at diag -1", entries=e2)
    many_offs, many = _pack([[_entry(0, 100, 30)] * 65, []])
    refused("read 0 has 65 entries, more than 64", entry_offsets=many_offs, entries=many)
    refused("read 1 has chosen 1, not below its list_len 1", chosen=np.array([0, 1], np.uint32))
    refused("read 0 has chosen 0, not below its list_len 0", list_len=np.array([0, 1], np.uint32))
    refused("read 1 has list_len 2, above its 1 entries", list_len=np.array([1, 2], np.uint32))
    refused("frag_min 5 exceeds frag_max 4", flags=P.MAPQ_PAIRED, frag_min=5, frag_max=4)
    odd_offs, odd_ent = _pack([[_entry(0, 100, 30)]] * 3)
    refused("n_reads 3 is odd", flags=P.MAPQ_PAIRED, entry_offsets=odd_offs, entries=odd_ent, chosen=np.zeros(3, np.uint32))
    t3 = _tables([[(2, 10)], [(3, 10)], [(4, 10)]])
    small_offs, small = _pack([[_entry(0, 0, 5, 0, 5)], []])
    refused("n_seq 3 is odd", flags=P.MAPQ_PAIRED, seq_offsets=t3[0], visit_offsets=t3[1], visit_nodes=t3[2], visit_length=t3[3], entry_offsets=small_offs, entries=small,
            chosen=np.array([0, NO], np.uint32))
    t4 = _tables([[(2, 10)], [(3, 11)]])
    refused("twins have one length", flags=P.MAPQ_PAIRED, seq_offsets=t4[0], visit_offsets=t4[1], visit_nodes=t4[2], visit_length=t4[3], entry_offsets=small_offs, entries=small,
            chosen=np.array([0, NO], np.uint32))
    # and what is refused unpaired only under PAIRED is served without it
    got = P.read_mapq_arrays(0, t3[0], t3[1], t3[2], t3[3], small_offs, small, np.array([0, NO], np.uint32))
    assert tuple(got[0]) == (60, Q.HAS | Q.LOCUS, 1, 1, 1, 0, 0, 0) and tuple(got[1]) == (0,) * 8
