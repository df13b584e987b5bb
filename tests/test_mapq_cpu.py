"""CPU tier of read mapq (include/pgx.h "read mapq"): the tables T and K by exact integers against the header's literals; the emulator of
tests/mapq_emu.py on hand-worked entries; the layout of the records, the exported entry points and, without a GPU, PGX_ERR_NO_DEVICE (these fail
on a library without the stage); and the emulator chain oracle MEMs -> place_emu -> verify_emu -> (rescue_emu ->) mates_emu -> mapq_emu on the
cases of tests/mapq_cases.py:

  walk        all 200 error-free reads have mapq 60, one locus and no competitor, though most of them tie between haplotypes (n_tied > 1)
  indel_mid   with the next coverage level as extras the second diagonal competes at slack 0 and is adjacent at slack 8
  near_copy   (reads with one read error) mapq 60 without extras; with them the other copy is an extra P + 1 = 5 score units down: mapq = min(60, scale * 5)
              at scale 2, 4 and 12
  repeat mates (mates_cases, which == 1)   unpaired two exact copies: mapq 3; after the election at U = 10, scale 2: the other copy is 10 units down, mapq 20
  rescued mates (rescue_cases)             RESCUED, and the excess is the rescue terms
  under PAIRED the chosen entry has the largest score of its list, for every pair of both tables at U = 0, 10 and 1000

Every mutation of the emulator changes what one of these statements reads -- but one: `<` for `<=` in the K comparison is the same function, because
no E makes E K[q] equal (E + 65536) 65536, which the test shows from the table."""
import ctypes
import os
import re

import numpy as np
import pytest

import mapq_cases as QC
import mapq_emu as Q
import mates_cases as MC
import mates_emu as M
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import place_emu as E
import rescue_cases as RC
import rescue_emu as R
import verify_emu as V
import walk_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pgx_batch_read_mapq", "pgx_batch_mapqs", "pgx_batch_device_mapqs", "pgx_read_mapq_arrays")
T_LITERALS = [65536, 52057, 41350, 32845, 26090, 20724, 16461, 13076, 10386, 8250, 6553, 5205, 4135, 3284, 2609, 2072, 1646, 1307, 1038, 825, 655, 520, 413, 328, 260,
              207, 164, 130, 103, 82, 65, 52, 41, 32, 26, 20, 16, 13, 10, 8, 6, 5, 4, 3, 2, 2, 1, 1, 1, 0]
K_HEAD = [65536, 82504, 103867, 130761, 164618, 207243, 260903, 328458, 413504, 520570, 655360, 825049]
MIN_LEN, MAX_CAND, PENALTY, U = 12, 16, 4, 10


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables and the emulator on hand-worked entries
def _header_table(name):
    src = open(os.path.join(ROOT, "include", "pgx.h")).read()
    return [int(x) for x in re.findall(r"\d+", re.search(r"#define %s \{(.*?)\}" % name, src, re.S).group(1))]


def test_the_tables_are_the_floors_of_the_powers_of_ten():
    assert Q.T == T_LITERALS == _header_table("PGX_MAPQ_T") and len(Q.T) == 50
    assert Q.K[:12] == K_HEAD and Q.K[60] == 65536000000 and Q.K == _header_table("PGX_MAPQ_K") and len(Q.K) == 61
    for k, t in enumerate(Q.T):
        assert t ** 10 * 10 ** k <= 65536 ** 10 < (t + 1) ** 10 * 10 ** k
    for q, v in enumerate(Q.K):
        assert v ** 10 <= 65536 ** 10 * 10 ** q < (v + 1) ** 10
    assert [Q.quality(e) for e in (0, 65536, 2 * 65536, 6553, 655, 1)] == [60, 3, 1, 10, 20, 48]
    assert Q.quality(253121) == 1 and Q.quality(253122) == 0 and Q.quality(1 << 26) == Q.quality((1 << 49)) == 0
    # `<` for `<=`: E K[q] == (E + 65536) 65536 needs (K[q] - 65536) E == 2^32, and no K[q] - 65536 divides 2^32
    assert all((1 << 32) % (Q.K[q] - 65536) for q in range(1, 61))
    assert all(Q.quality(e, "k_lt") == Q.quality(e) for e in list(range(0, 70000, 7)) + [1 << k for k in range(50)])
    # the kernel holds E at 2^26 in the comparison: mapq is 0 from 253 122 on with either sign, so the hold changes nothing, and 2^26 itself is no equality
    hold = lambda e: min(e, 1 << 26)
    assert all(Q.quality(hold(e), m) == Q.quality(e, m) == 0 for m in (None, "k_lt") for e in (253122, (1 << 26) - 1, 1 << 26, (1 << 26) + 1, 1 << 32, (1 << 49) - 1))
    assert all((1 << 26) * Q.K[q] != ((1 << 26) + 65536) * 65536 for q in range(61))


def _entry(seq, diag, score, lo=0, hi=60, seg_start=0):
    return dict(seq=seq, diag=diag, seg_score=score, matches=score, span_lo=lo, span_hi=hi, seg_start=seg_start)


def _entries(items):
    out = np.zeros(len(items), Q.VERIFY_DTYPE)
    for k, e in enumerate(items):
        for f, v in e.items():
            out[k][f] = v
    return out


# two paths of two strands: nodes 1 (10), 2 (100), 3 (90) and 1, 4 (100), 3: sequences 0 .. 3 of 200 symbols
TABLES = (np.array([0, 3, 6, 9, 12], np.uint64), np.array([2, 4, 6, 7, 5, 3, 2, 8, 6, 7, 9, 3], np.uint64), np.array([10, 100, 90, 90, 100, 10, 10, 100, 90, 90, 100, 10], np.uint32))


def _one(items, chosen=0, **kw):
    e = _entries(items)
    return Q.read_mapq(*TABLES, np.array([0, len(e)], np.uint64), e, np.array([chosen], np.uint32), **kw)["records"][0]


def hand_places(m=None):
    rec = _one([_entry(0, 120, 60), _entry(2, 120, 60)], mutation=m)  # node 3 at offset 10 on both paths
    assert tuple(rec) == (60, Q.HAS | Q.LOCUS, 2, 1, 2, 0, 0, 0)
    rec = _one([_entry(0, 20, 60), _entry(2, 20, 60)], mutation=m)    # node 2 against node 4: two places, an exact tie
    assert tuple(rec) == (3, Q.HAS | Q.LOCUS, 2, 2, 1, 1, 60, 65536)
    rec = _one([_entry(0, 20, 60), _entry(2, 20, 55), _entry(0, 140, 50)], mutation=m)  # 5 and 10 units down at scale 2: T[10] + T[20]
    assert (int(rec["excess"]), int(rec["n_competing"]), int(rec["best_other"]), int(rec["mapq"])) == (6553 + 655, 2, 55, 10)
    rec = _one([_entry(0, 20, 60), _entry(0, 140, 50), _entry(2, 140, 50)], mutation=m)  # one class of two haplotypes 10 units down weighs T[20] once
    assert (int(rec["excess"]), int(rec["n_competing"]), int(rec["n_loci"]), int(rec["mapq"])) == (655, 1, 2, 20)
    rec = _one([_entry(0, 20, 60), _entry(2, 20, 55), _entry(0, 140, 50)], scale=16, mutation=m)  # 80 and 160: both held at T[49] = 0
    assert (int(rec["excess"]), int(rec["mapq"])) == (0, 60)
    rec = _one([_entry(0, 20, 60), _entry(0, 140, 36)], scale=2, mutation=m)  # 48: T[48] = 1
    assert (int(rec["excess"]), int(rec["mapq"])) == (1, 48)
    rec = _one([_entry(0, 20, 50), _entry(2, 20, 55)], mutation=m)  # a stated chosen that is not the best
    assert int(rec["flags"]) == Q.HAS | Q.LOCUS | Q.OUTSCORED and (int(rec["excess"]), int(rec["mapq"])) == (65536, 3)


def test_haplotypes_that_share_a_node_are_one_place():
    hand_places()


def hand_diagonals(m=None):
    two = [_entry(0, 20, 31, seg_start=0), _entry(0, 21, 30, seg_start=30)]
    rec = _one(two, slack=0, mutation=m)  # one unit down: T[2] = 41350, 10 log10(106886 / 41350) = 4.1
    assert (int(rec["mapq"]), int(rec["n_competing"]), int(rec["excess"])) == (4, 1, 41350)
    rec = _one(two, slack=1, mutation=m)
    assert tuple(rec) == (60, Q.HAS | Q.LOCUS, 2, 2, 2, 0, 0, 0)
    rec = _one([_entry(0, 20, 31), _entry(1, 21, 30)], slack=8, mutation=m)  # another sequence: not adjacent
    assert int(rec["n_competing"]) == 1
    # the anchor is the chosen entry's seg_start: the paths share node 1 under read position 0 and part under position 10, where the segment starts
    rec = _one([_entry(0, 5, 50, seg_start=10), _entry(2, 5, 50, seg_start=10)], mutation=m)
    assert (int(rec["n_loci"]), int(rec["n_competing"]), int(rec["mapq"])) == (2, 1, 3)
    # an entry whose span ends before the anchor has no locus and is a class of its own
    rec = _one([_entry(0, 120, 30, seg_start=30), _entry(2, 120, 30, lo=0, hi=30)], mutation=m)
    assert (int(rec["n_loci"]), int(rec["n_competing"]), int(rec["flags"])) == (2, 1, Q.HAS | Q.LOCUS)
    rec = _one([_entry(0, 20, 0, lo=0, hi=0)], mutation=m)  # an empty span: the chosen entry has no locus itself
    assert tuple(rec) == (60, Q.HAS, 1, 1, 1, 0, 0, 0)
    assert tuple(_one([_entry(0, 20, 60)], chosen=Q.NO_CHOSEN, mutation=m)) == (0,) * 8
    # the rescue terms: n_best - 1 exact ties and the next level of the window
    resc = np.zeros(1, R.RESCUE_DTYPE)
    resc[0]["flags"], resc[0]["n_best"], resc[0]["seg_score"], resc[0]["next_score"] = R.TARGET | R.RESCUED, 3, 40, 35
    rec = _one([_entry(0, 20, 40)], rescue=resc, mutation=m)
    assert (int(rec["excess"]), int(rec["flags"]), int(rec["mapq"])) == (2 * 65536 + 6553, Q.HAS | Q.LOCUS | Q.RESCUED, 1)
    rec = _one([_entry(0, 20, 40), _entry(0, 140, 40)], rescue=resc, mutation=m)  # the chosen entry is not the list's last: no rescue terms
    assert (int(rec["excess"]), int(rec["flags"])) == (65536, Q.HAS | Q.LOCUS)


def test_neighbouring_diagonals_the_anchor_and_the_rescue_terms():
    hand_diagonals()


def hand_paired(m=None):
    lens = [200, 200, 200, 200]
    # A in two copies (20 and 100 on sequence 0), B on sequence 1 at 40: frag = 200 - 100 - 40 = 60 with the second copy, 140 with the first
    a, b = [_entry(0, 20, 50), _entry(0, 100, 50)], [_entry(1, 40, 50)]
    e = _entries(a + b)
    offs, paired = np.array([0, 2, 3], np.uint64), dict(seq_lengths=lens, frag_min=0, frag_max=100, penalty=10)
    for chosen_a, want in ((1, 20), (0, 3)):  # elected: 100 against 50 + (50 - 10): T[20]; not elected: the other copy scores more, OUTSCORED
        recs = Q.read_mapq(*TABLES, offs, e, np.array([chosen_a, 0], np.uint32), paired=paired, mutation=m)["records"]
        assert int(recs[0]["mapq"]) == want and int(recs[1]["mapq"]) == 60 and int(recs[0]["flags"]) & Q.PAIRED and int(recs[1]["flags"]) & Q.PAIRED
        assert bool(int(recs[0]["flags"]) & Q.OUTSCORED) == (chosen_a == 0)
    lone = Q.read_mapq(*TABLES, np.array([0, 2, 2], np.uint64), _entries(a), np.array([0, Q.NO_CHOSEN], np.uint32), paired=paired, mutation=m)["records"]
    assert int(lone[0]["mapq"]) == 3 and not int(lone[0]["flags"]) & Q.PAIRED and tuple(lone[1]) == (0,) * 8  # the mate has no candidate: m = 0
    assert Q.mate_term(lens, a[0], _entries(b), 0, 100, 1000, m) == -950  # no compatible candidate: solo_mate - U, negative


def test_the_paired_score():
    hand_paired()


# ---------------------------------------------------------------------------------------------------------------------------------
# the library's surface
def test_record_layouts():
    d = P.MAPQ_DTYPE
    assert d.itemsize == 32 and d == Q.MAPQ_DTYPE
    assert {n: d.fields[n][1] for n in d.names} == dict(mapq=0, flags=4, n_entries=8, n_loci=12, n_with=16, n_competing=20, best_other=24, excess=28)
    assert ctypes.sizeof(P.ReadMapqs) == 80
    offs = {n: getattr(P.ReadMapqs, n).offset for n, _ in P.ReadMapqs._fields_}
    assert offs == dict(n_reads=0, n_has=8, n_unique=16, n_capped=24, sum_mapq=32, n_extras=40, scale=48, slack=52, max_extra=56, flags=60, records=64, ms_mapq=72, reserved=76)
    header = open(os.path.join(ROOT, "include", "pgx.h")).read()
    assert re.search(r"uint32_t\s+mapq,\s*flags,\s*n_entries,\s*n_loci,\s*n_with,\s*n_competing,\s*best_other,\s*excess;\s*\}\s*pgx_read_mapq;", header)
    for name, value in (("HAS", Q.HAS), ("LOCUS", Q.LOCUS), ("PAIRED", Q.PAIRED), ("RESCUED", Q.RESCUED), ("CAPPED", Q.CAPPED), ("OUTSCORED", Q.OUTSCORED)):
        m = re.search(r"^#define\s+PGX_MAPQ_%s\s+(\d+)u" % name, header, re.M)
        assert m and int(m.group(1)) == value == getattr(P, "MAPQ_" + name), name
    assert (P.MAPQ_MAX_ENTRIES, P.MAPQ_MAX_SCALE, P.MAPQ_MAX_SLACK, P.MAPQ_MAX_EXTRA, P.MAPQ_NO_CHOSEN) == (64, 16, 1024, 63, 0xFFFFFFFF)


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
        P.read_mapq_arrays(0, np.arange(5, dtype=np.uint64) * 200, *TABLES, np.zeros(2, np.uint64), np.zeros(0, P.VERIFY_DTYPE), np.array([P.MAPQ_NO_CHOSEN], np.uint32))
    assert e.value.code == P.ERR_NO_DEVICE
    assert L.pgx_batch_read_mapq(None, 2, 8, 16, 0, None) == P.ERR_NO_DEVICE
    out = P.ReadMapqs()
    assert L.pgx_batch_mapqs(None, ctypes.byref(out)) == P.ERR_ARG and L.pgx_batch_device_mapqs(None, ctypes.byref(out)) == P.ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the chain
def _chain(workdir, name, raw, seqs, reads):
    """(place, verified) of the reads at max_cand 16, penalty 4, from the oracle's MEMs, located, through place_emu and verify_emu"""
    path = os.path.join(workdir, name + ".txt")
    with open(path, "wb") as f:
        f.write(raw)
    ri = W.build_index_from_text(path, workdir, name, with_tags=False)[0]
    orc = O.RIndex(ri)
    L = int(P.Index(ri, mode=P.MODE_STRICT).info().max_length)
    mems, mem_off, values, loc_off = [], [0], [], [0]
    for read in reads:
        for m in orc.find_all_mems(read, MIN_LEN, 1, O.MODE_STRICT):
            mems.append(m)
            values += [int(v) for v in orc.locate_sa(m[2], m[2] + m[3] - 1, O.MODE_STRICT)]
            loc_off.append(len(values))
        mem_off.append(len(mems))
    marr = np.zeros(len(mems), E.MEM_DTYPE)
    for k, m in enumerate(mems):
        marr[k] = m
    place = E.read_place(np.array(mem_off, np.uint64), marr, np.array(loc_off, np.uint64), np.array(values, np.uint64), L)
    return place, V.read_verify(seqs, reads, V.candidates_from_places(place, MAX_CAND), PENALTY)


def _mapq(tables, seqs, reads, place, verified, max_extra, winners=None, mutation=None, **kw):
    offs, ent, list_len, more = Q.candidates_with_extras(seqs, reads, place, verified, max_extra, PENALTY, mutation)
    chosen = Q.chosen_of(verified["reads"] if winners is None else winners)
    return Q.read_mapq(*tables, offs, ent, chosen, list_len=list_len, max_cand=MAX_CAND, more=more if max_extra else None, mutation=mutation, **kw)


@pytest.fixture(scope="module")
def graph_chain(workdir):
    g = WC.graph()
    truth, reads = WC.cut_reads(g)
    itruth, ireads = QC.indel_mid(g)
    allr = reads + ireads + QC.none_reads()
    place, verified = _chain(workdir, "mapq_walk_graph", b"".join(t + b"\n" for t in g["texts"]), g["texts"], allr)
    return dict(g=g, tables=QC.graph_tables(g), reads=allr, place=place, verified=verified, walk=range(0, WC.N_READS), indel=range(WC.N_READS, WC.N_READS + QC.N_INDEL),
                none=range(WC.N_READS + QC.N_INDEL, len(allr)), truth=truth, itruth=itruth)


@pytest.fixture(scope="module")
def near_chain(workdir):
    N = QC.NEAR
    place, verified = _chain(workdir, "mapq_near_copy", N.raw, N.seqs, N.reads)
    return dict(tables=N.tables, reads=N.reads, place=place, verified=verified)


@pytest.fixture(scope="module")
def mates_chain(workdir):
    C = MC.CASES
    place, verified = _chain(workdir, "mapq_mates_cases", C.raw, C.seqs, C.reads)
    return dict(tables=QC.chunk_tables(C.lens)[:3], reads=C.reads, place=place, verified=verified)


@pytest.fixture(scope="module")
def rescue_chain(workdir):
    C = RC.CASES
    place, verified = _chain(workdir, "mapq_rescue_cases", C.raw, C.seqs, C.reads)
    res = R.read_rescue(C.seqs, C.reads, verified["cand_offsets"], verified["cands"], RC.FRAG_MIN, RC.FRAG_MAX, RC.PENALTY, RC.MIN_LEN, 2, R.MERGE)
    merged = dict(reads=res["winners"], cand_offsets=res["cand_offsets"], cands=res["cands"])
    return dict(tables=QC.chunk_tables(C.lens)[:3], reads=C.reads, place=place, verified=merged, rescue=res["reads"])


def check_walk(c, res, verified):
    """all 200: mapq 60, one locus, no competitor; returns how many of them tie between haplotypes"""
    recs = res["records"]
    for r in c["walk"]:
        assert (int(recs[r]["mapq"]), int(recs[r]["n_competing"]), int(recs[r]["n_loci"])) == (60, 0, 1), r
        assert int(recs[r]["flags"]) == Q.HAS | Q.LOCUS and int(recs[r]["n_with"]) == int(recs[r]["n_entries"]) == int(verified["reads"][r]["n_cand"])
    for r in c["none"]:
        assert tuple(recs[r]) == (0,) * 8
    tied_by_text = sum(1 for r in c["walk"] if sum(t.count(c["reads"][r]) for t in c["g"]["texts"]) > 1)
    tied = sum(1 for r in c["walk"] if int(verified["reads"][r]["n_tied"]) > 1)
    assert tied == tied_by_text >= 150
    return tied


def check_indel(c, at0, at8):
    for r in c["indel"]:
        assert int(at0["records"][r]["n_competing"]) >= 1 and int(at0["records"][r]["mapq"]) < 60, r
        assert int(at0["records"][r]["excess"]) <= 65536 * int(at0["records"][r]["n_competing"]), r  # a class weighs at most T[0], however many haplotypes it holds
        assert (int(at8["records"][r]["mapq"]), int(at8["records"][r]["n_competing"])) == (60, 0), r
        assert int(at8["records"][r]["n_with"]) == int(at8["records"][r]["n_entries"]) and int(at8["records"][r]["n_loci"]) >= 2


def test_walk_reads_are_one_place_whatever_n_tied_says(graph_chain):
    c = graph_chain
    res = _mapq(c["tables"], c["g"]["texts"], c["reads"], c["place"], c["verified"], 0)
    tied = check_walk(c, res, c["verified"])
    print("walk: %d of 200 reads have n_tied > 1, all 200 have mapq 60" % tied)
    assert res["n_has"] == WC.N_READS + QC.N_INDEL and res["sum_mapq"] == int(res["records"]["mapq"].sum()) >= 60 * WC.N_READS
    assert not np.asarray(WC.ambiguous(c["g"], c["truth"], c["reads"][:WC.N_READS])).any()


def test_the_second_diagonal_of_an_indel_competes_only_without_slack(graph_chain):
    c = graph_chain
    args = (c["tables"], c["g"]["texts"], c["reads"], c["place"], c["verified"], 16)
    check_indel(c, _mapq(*args, slack=0), _mapq(*args, slack=8))
    both = sum(1 for r in c["indel"] if int(c["verified"]["reads"][r]["n_cand"]) == 16)
    print("indel_mid: %d of %d reads tie between the two diagonals in coverage, the others see the second one as an extra" % (both, QC.N_INDEL))


def check_near(recs0, recs16, scale):
    for r in range(QC.N_NEAR):
        assert (int(recs0[r]["mapq"]), int(recs0[r]["n_entries"]), int(recs0[r]["n_competing"])) == (60, 1, 0), r
        assert (int(recs16[r]["mapq"]), int(recs16[r]["n_entries"]), int(recs16[r]["n_competing"]), int(recs16[r]["best_other"])) == (min(60, scale * 5), 2, 1, 58 - 2 * PENALTY), (r, scale)


def test_a_copy_one_mismatch_down_is_seen_through_the_extras(near_chain):
    c, N = near_chain, QC.NEAR
    for r in range(QC.N_NEAR):  # the list holds the first copy alone; the second is one coverage level below
        assert (int(c["verified"]["reads"][r]["seq"]), int(c["verified"]["reads"][r]["diag"]), int(c["verified"]["reads"][r]["n_cand"])) == N.truth[r] + (1,)
        assert int(c["place"]["reads"][r]["best_score"]) == 59 and 12 <= int(c["place"]["reads"][r]["next_score"]) <= 59 - 12 and int(c["verified"]["reads"][r]["seg_score"]) == 59 - PENALTY
    for scale in (2, 4, 12):
        check_near(_mapq(c["tables"], N.seqs, c["reads"], c["place"], c["verified"], 0, scale=scale)["records"],
                   _mapq(c["tables"], N.seqs, c["reads"], c["place"], c["verified"], 16, scale=scale)["records"], scale)


def _inside(k):
    """the read of pair k of mates_cases that lies inside the repeat"""
    return 2 * k + (0 if MC.CASES.pairs[k]["mate"] == "a" else 1)


SECOND_COPY = [k for k, p in enumerate(MC.CASES.pairs) if p["which"] == 1]
PAIRED = dict(seq_lengths=MC.CASES.lens, frag_min=MC.FRAG_MIN, frag_max=MC.FRAG_MAX, penalty=U)


def check_repeat_mates(solo, elected):
    assert len(SECOND_COPY) == 24
    for k in SECOND_COPY:
        r = _inside(k)
        assert (int(solo[r]["mapq"]), int(solo[r]["n_loci"]), int(solo[r]["excess"])) == (3, 2, 65536), k
        assert (int(elected[r]["mapq"]), int(elected[r]["excess"]), int(elected[r]["best_other"])) == (20, 655, 90), k
        assert int(elected[r]["flags"]) == Q.HAS | Q.LOCUS | Q.PAIRED and int(elected[r ^ 1]["mapq"]) == 60


def test_a_repeat_is_a_tie_alone_and_twenty_with_its_mate(mates_chain):
    c, C = mates_chain, MC.CASES
    solo = _mapq(c["tables"], C.seqs, c["reads"], c["place"], c["verified"], 0)["records"]
    el = M.read_mates(C.lens, c["verified"]["cand_offsets"], c["verified"]["cands"], MC.FRAG_MIN, MC.FRAG_MAX, U, M.ELECT)
    elected = _mapq(c["tables"], C.seqs, c["reads"], c["place"], c["verified"], 0, winners=el["winners"], paired=PAIRED)["records"]
    check_repeat_mates(solo, elected)


def check_rescued(c, recs, rescue, scale=2):
    n = 0
    for r, rr in enumerate(rescue):
        if not int(rr["flags"]) & R.RESCUED:
            assert not int(recs[r]["flags"]) & Q.RESCUED
            continue
        last = int(c["verified"]["cand_offsets"][r + 1]) - int(c["verified"]["cand_offsets"][r]) - 1
        if int(c["winners"][r]["cand_index"]) != last:
            continue
        terms = (int(rr["n_best"]) - 1) * 65536 + (Q.T[min(49, scale * (int(rr["seg_score"]) - int(rr["next_score"])))] if int(rr["next_score"]) else 0)
        assert int(recs[r]["flags"]) & Q.RESCUED and int(recs[r]["excess"]) >= terms, r
        if int(recs[r]["n_competing"]) == 0:
            assert int(recs[r]["excess"]) == terms and int(recs[r]["mapq"]) == Q.quality(terms), r
        n += 1
    return n


def test_rescued_mates_carry_the_rescue_terms(rescue_chain):
    c, C = rescue_chain, RC.CASES
    c = dict(c, winners=c["verified"]["reads"])
    res = _mapq(c["tables"], C.seqs, c["reads"], c["place"], c["verified"], 0, rescue=c["rescue"])
    n = check_rescued(c, res["records"], c["rescue"])
    tandem = [2 * k + (0 if p["mate"] == "a" else 1) for k, p in enumerate(C.pairs) if p["kind"] == "tandem"]
    assert n >= 44 and all(int(res["records"][r]["excess"]) >= 65536 and int(res["records"][r]["mapq"]) <= 3 for r in tandem)  # a tandem repeat: tied diagonals in the window
    print("rescue: %d rescued mates carry the terms" % n)


def check_chosen_is_best(tables, seqs, verified, winners, lens, penalty):
    """under PAIRED no list entry outscores the chosen one: OUTSCORED is never set when there are no extras"""
    offs, ent, list_len, _ = Q.candidates_with_extras(seqs, [None] * (len(verified["cand_offsets"]) - 1), None, verified, 0)
    res = Q.read_mapq(*tables, offs, ent, Q.chosen_of(winners), list_len=list_len, paired=dict(seq_lengths=lens, frag_min=0, frag_max=500, penalty=penalty))
    assert not (res["records"]["flags"] & Q.OUTSCORED).any()
    return res


@pytest.mark.parametrize("penalty", [0, 10, 1000])
def test_the_chosen_entry_has_the_largest_paired_score(mates_chain, rescue_chain, penalty):
    for c, C in ((mates_chain, MC.CASES), (rescue_chain, RC.CASES)):
        v = c["verified"]
        el = M.read_mates(C.lens, v["cand_offsets"], v["cands"], 0, 500, penalty, M.ELECT)
        check_chosen_is_best(c["tables"], C.seqs, v, el["winners"], C.lens, penalty)
        for r in range(len(c["reads"])):  # and directly: the score of the chosen entry is the largest of its list
            lst, mate = (v["cands"][int(v["cand_offsets"][x]):int(v["cand_offsets"][x + 1])] for x in (r, r ^ 1))
            if len(lst):
                scores = [int(e["seg_score"]) + Q.mate_term(C.lens, e, mate, 0, 500, penalty) for e in lst]
                assert scores[int(el["winners"][r]["cand_index"])] == max(scores), (r, penalty)


# ---------------------------------------------------------------------------------------------------------------------------------
# mutations of the emulator: each trips a statement above
MUTATION_TRIPS = {  # mutation -> the statements it trips (k_lt: none, see test_the_tables_are_the_floors_of_the_powers_of_ten)
    "class_seq_diag": ["hand_places", "hand_diagonals", "walk", "indel"],  # classes by (seq, diag): every tied haplotype is a competitor
    "anchor_zero": ["hand_diagonals"],                  # anchor 0: two paths that part behind read position 0 become one place
    "adj_no_seq": ["hand_diagonals"],                   # adjacency without the seq test: a neighbouring diagonal of another sequence stops competing
    "weight_per_entry": ["hand_places", "indel"],       # the second diagonal's class holds every haplotype: it weighs more than T[0]
    "clamp_48": ["hand_places", "near12"],              # scale * d >= 49 weighs T[48] = 1: mapq 48 where it is 60
    "solo_no_u": ["hand_paired", "mates"],              # solo_mate without - U: the other copy of the repeat ties with the chosen one
    "no_rescue": ["hand_diagonals", "rescued"],         # rescue terms dropped
    "extras_best": ["indel", "near", "near12"],         # extras taken from the best level repeat the list: the next level stays unseen
}


def _trips(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def test_each_mutation_trips_a_statement(graph_chain, near_chain, mates_chain, rescue_chain):
    g, nc, mc, rc = graph_chain, near_chain, mates_chain, rescue_chain
    C, N = MC.CASES, QC.NEAR
    el = M.read_mates(C.lens, mc["verified"]["cand_offsets"], mc["verified"]["cands"], MC.FRAG_MIN, MC.FRAG_MAX, U, M.ELECT)
    rcw = dict(rc, winners=rc["verified"]["reads"])

    def walk(m):
        return _trips(lambda: check_walk(g, _mapq(g["tables"], g["g"]["texts"], g["reads"], g["place"], g["verified"], 0, mutation=m), g["verified"]))

    def indel(m):
        args = (g["tables"], g["g"]["texts"], g["reads"], g["place"], g["verified"], 16)
        return _trips(lambda: check_indel(g, _mapq(*args, slack=0, mutation=m), _mapq(*args, slack=8, mutation=m)))

    def near(m, scale=2):
        return _trips(lambda: check_near(_mapq(nc["tables"], N.seqs, nc["reads"], nc["place"], nc["verified"], 0, scale=scale, mutation=m)["records"],
                                         _mapq(nc["tables"], N.seqs, nc["reads"], nc["place"], nc["verified"], 16, scale=scale, mutation=m)["records"], scale))

    def mates(m):
        return _trips(lambda: check_repeat_mates(_mapq(mc["tables"], C.seqs, mc["reads"], mc["place"], mc["verified"], 0, mutation=m)["records"],
                                                 _mapq(mc["tables"], C.seqs, mc["reads"], mc["place"], mc["verified"], 0, winners=el["winners"], paired=PAIRED, mutation=m)["records"]))

    def rescued(m):
        return _trips(lambda: check_rescued(rcw, _mapq(rc["tables"], RC.CASES.seqs, rc["reads"], rc["place"], rc["verified"], 0, rescue=rc["rescue"], mutation=m)["records"], rc["rescue"]))

    checks = dict(hand_places=lambda m: _trips(hand_places, m), hand_diagonals=lambda m: _trips(hand_diagonals, m), hand_paired=lambda m: _trips(hand_paired, m),
                  walk=walk, indel=indel, near=near, near12=lambda m: near(m, 12), mates=mates, rescued=rescued)
    tripped = {m: [name for name, f in checks.items() if f(m)] for m in Q.MUTATIONS if m != "k_lt"}
    for m, names in tripped.items():
        print("%s: trips %s" % (m, ", ".join(names) or "nothing"))
    assert all(tripped.values()), tripped
    assert not any(f(None) for f in checks.values())  # and nothing trips without a mutation
    assert tripped == MUTATION_TRIPS
