"""GPU tier of the align kernels at their borders, through pgx_read_align_arrays against tests/align_emu.py, byte for byte, records and
operations, and the same records without PGX_ALIGN_CIGAR: every word offset of the text window against the read lengths around a word and
a wave, every band on both sides of every group width, reads of mixed lengths and candidates in one wave, indels at the ends of a read,
indel runs at the band's edge, a band cut by the ends of a sequence, the shortest sequences and the end of the text, the symbols that never
match, candidates that do not overlap or do not exist, empty inputs, more reads than one grid, passes over a small scratch budget, and every
call it refuses."""
import numpy as np
import pytest

import align_emu as E
import pgx_ffi as P

pytestmark = pytest.mark.gpu

LENGTHS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 150, 257)
BANDS = (0, 1, 2, 3, 4, 7, 8, 15, 16, 31)  # group widths 1 2 4 8 16 32 64: both sides of every one
NONE = (E.NO_SEQUENCE, 0)


def _arrays(seqs, reads, cands):
    seq_off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.uint64)
    read_off = np.concatenate(([0], np.cumsum([len(r) for r in reads]))).astype(np.uint64)
    cands = [NONE if c is None else c for c in cands]
    return (np.frombuffer(b"".join(seqs), np.uint8), seq_off, np.frombuffer(b"".join(reads), np.uint8), read_off,
            np.array([q for q, _ in cands], np.uint32), np.array([d for _, d in cands], np.int64))


def _check(seqs, reads, cands, band, exp=None):
    """records and operations of the library == the emulator; without PGX_ALIGN_CIGAR the same records.  Returns the emulator's result."""
    seqs, reads = [bytes(s) for s in seqs], [bytes(r) for r in reads]
    if exp is None:
        exp = E.read_align(seqs, reads, cands, band)
    args = _arrays(seqs, reads, cands)
    got = P.read_align_arrays(0, *args, band=band, flags=P.ALIGN_CIGAR)
    assert got["reads"].dtype == E.ALIGN_DTYPE == P.ALIGN_DTYPE
    bad = np.flatnonzero(got["reads"] != exp["reads"])
    assert len(bad) == 0, (band, len(bad), int(bad[0]), reads[bad[0]], cands[bad[0]], got["reads"][bad[0]], exp["reads"][bad[0]])
    assert got["op_offsets"].tobytes() == exp["op_offsets"].tobytes()
    bad = np.flatnonzero(got["ops"] != exp["ops"])
    assert len(bad) == 0, (band, len(bad), int(bad[0]), P.cigar_text(got["ops"][bad[0]:bad[0] + 4]), E.cigar_text(exp["ops"][bad[0]:bad[0] + 4]))
    for k in ("reads", "op_offsets", "ops"):
        assert got[k].tobytes() == exp[k].tobytes(), k
    plain = P.read_align_arrays(0, *args, band=band, flags=0)
    assert plain["reads"].tobytes() == exp["reads"].tobytes() and plain["ops"] is None and plain["op_offsets"] is None
    return exp


def _dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), size=n))


def _edit(rng, s, n_edits):
    """up to n_edits substitutions, insertions and deletions at random places"""
    a = bytearray(s)
    for _ in range(n_edits):
        at, kind = int(rng.integers(0, len(a) + 1)), int(rng.integers(0, 3))
        if kind == 0 and at < len(a):
            a[at] = b"ACGT"[int(rng.integers(0, 4))]
        elif kind == 1:
            a.insert(at, b"ACGT"[int(rng.integers(0, 4))])
        elif len(a) > 1 and at < len(a):
            del a[at]
    return bytes(a)


@pytest.mark.parametrize("band", BANDS)
def test_every_diagonal_residue_and_length(band):
    """a sequence of 263 symbols behind one of 5 (so that sequence offsets and text words do not line up), reads cut from it with a few edits
    and laid on every diagonal 0 .. 15: the lengths of LENGTHS are those of the edited reads, and reads longer than what is left hang over"""
    rng = np.random.default_rng(10 + band)
    seqs = [_dna(rng, 5), _dna(rng, 263, b"ACGTACGTACGTN")]
    reads, cands = [], []
    for length in LENGTHS:
        for diag in range(16):
            src = _edit(rng, seqs[1][diag:diag + length], int(rng.integers(0, 4)))
            src = (src + _dna(rng, length))[:length]
            reads.append(src)
            cands.append((1, diag))
    v = _check(seqs, reads, cands, band)["reads"]
    assert [len(r) for r in reads] == [n for n in LENGTHS for _ in range(16)]
    assert (v["edits"] > 0).any() and (v["edits"] == 0).any() and (v["clip_hi"] > 0).any()
    if band:
        assert (v["n_ins"] > 0).any() and (v["n_del"] > 0).any() and (v["band_hit"] == 0).any()
    else:
        assert not v["n_ins"].any() and not v["n_del"].any() and not v["band_hit"].any() and (v["text_start"] == v["diag"] + v["clip_lo"]).all()


@pytest.mark.parametrize("band", [0, 1, 3, 7, 12])
def test_mixed_lengths_and_candidates_share_a_wave(band):
    rng = np.random.default_rng(20 + band)
    seqs = [_dna(rng, 40), _dna(rng, 200), _dna(rng, 33), _dna(rng, 1)]
    reads, cands = [], []
    for r in range(300):
        q = int(rng.integers(0, 4))
        length = int(rng.integers(0, 71))
        start = int(rng.integers(-5, len(seqs[q])))
        body = seqs[q][max(start, 0):max(start, 0) + length]
        reads.append((_dna(rng, max(-start, 0)) + _edit(rng, body, int(rng.integers(0, 3))) if body else _dna(rng, length)))
        kind = r % 7
        cands.append(None if kind == 0 else (q, 1000 + r) if kind == 1 else (q, -1000 - r) if kind == 2 else (q, start + int(rng.integers(-2, 3))))
    v = _check(seqs, reads, cands, band)["reads"]
    assert (v["seq"] == E.NO_SEQUENCE).sum() >= 40 and (v["n_match"] > 20).any() and ((v["clip_hi"] > 0) & (v["n_match"] == 0) & (v["seq"] != E.NO_SEQUENCE)).any()


@pytest.mark.parametrize("band", [1, 2, 4, 8])
def test_an_indel_at_the_ends_of_a_read(band):
    rng = np.random.default_rng(30 + band)
    seqs = [_dna(rng, 11), _dna(rng, 120)]
    reads, cands = [], []
    for length in (9, 40, 65):
        src = seqs[1][30:30 + length]
        for at in (0, 1, length - 2, length - 1):
            reads.append(src[:at] + src[at + 1:])  # a deletion from the read: the text holds a base more
            reads.append(src[:at] + bytes([b"ACGT"[(b"ACGT".index(src[at]) + 1) % 4]]) + src[at:])  # a base the text does not hold
            cands += [(1, 30), (1, 30)]
    v = _check(seqs, reads, cands, band)["reads"]
    assert (v["edits"] <= 1).all() and (v["n_ins"] + v["n_del"] > 0).any()


@pytest.mark.parametrize("band", [2, 4, 8, 16])
def test_indel_runs_around_the_band(band):
    """a run of W - 1, W and W + 1 bases missing from the read or added to it, in the middle of 120 matching bases.  A run of W - 1 stays inside
    the band and a run of W walks along its edge: band_hit is 0 and 1.  A run of W + 1 does not fit: the banded optimum is worse than the W + 1
    edits of the unbanded one.  Whether its path touches the edge is up to the definitions alone (the cheapest path left inside a wide band
    may wander through the 60 bases behind the run without touching it; at W = 8 and 16 it does), so there the emulator decides."""
    rng = np.random.default_rng(40 + band)
    seqs = [_dna(rng, 7), _dna(rng, 400)]
    reads, cands, runs = [], [], []
    for n in (band - 1, band, band + 1):
        src = seqs[1][100:220 + n]
        reads.append(src[:60] + src[60 + n:])  # n bases of the text skipped
        reads.append(seqs[1][100:160] + _dna(rng, n) + seqs[1][160:220])  # n bases added
        cands += [(1, 100), (1, 100)]
        runs += [n, n]
    v = _check(seqs, reads, cands, band)["reads"]
    for r, n in enumerate(runs):
        if n <= band:
            assert int(v["band_hit"][r]) == (1 if n == band else 0), (r, n, v[r])
            assert (int(v["edits"][r]), int(v["n_del"][r]), int(v["n_ins"][r])) == ((n, n, 0) if r % 2 == 0 else (n, 0, n)), (r, n, v[r])
        else:
            assert int(v["edits"][r]) > n, (r, n, v[r])


@pytest.mark.parametrize("band", [3, 8, 31])
def test_a_band_cut_by_the_ends_of_the_sequence(band):
    rng = np.random.default_rng(50 + band)
    seqs = [_dna(rng, 13), _dna(rng, 90), _dna(rng, 21)]
    whole = seqs[1]
    reads, cands = [], []
    for diag in (0, 1, 2, band - 1, band, band + 1):  # the band's lower edge lies before the sequence, on its first symbol, behind it
        reads.append(_edit(rng, whole[diag:diag + 30], 2))
        cands.append((1, diag))
    for back in (0, 1, 2, band - 1, band, band + 1):  # and the upper edge behind its last symbol
        reads.append(_edit(rng, whole[60 - back:90 - back], 2))
        cands.append((1, 60 - back))
    reads += [whole[1:40], whole[:60] + whole[61:], _dna(rng, 4) + whole + _dna(rng, 4), whole[50:] + _dna(rng, 9)]
    cands += [(1, 0), (1, 1), (1, -4), (1, 50)]
    v = _check(seqs, reads, cands, band)["reads"]
    assert (v["text_start"] == 0).any() and (v["text_end"] == 90).any() and (v["clip_lo"] == 4).any() and (v["clip_hi"] == 9).any()


def test_shortest_sequences_and_the_end_of_the_text():
    rng = np.random.default_rng(6)
    for last in (1, 8, 9, 23):
        seqs = [b"G", _dna(rng, 8), _dna(rng, 9), _dna(rng, last)]
        reads, cands = [], []
        for q, s in enumerate(seqs):
            for pre, post in ((0, 0), (3, 0), (0, 5), (2, 40)):
                reads.append(_dna(rng, pre) + s + _dna(rng, post))
                cands.append((q, -pre))
            reads.append(s[-1:] + b"ACGTACGTACGTACGTACGT")  # the span ends on the last symbol of the sequence (of the text, for the last one)
            cands.append((q, len(s) - 1))
            reads.append(s[:-1])
            cands.append((q, 0))
        for band in (0, 2, 8, 31):
            v = _check(seqs, reads, cands, band)["reads"]
            assert (v["edits"] == 0).all() and (v["n_match"] + v["clip_lo"] + v["clip_hi"] == [len(r) for r in reads]).all()


@pytest.mark.parametrize("band", [0, 3])
def test_symbols_that_never_match(band):
    seqs = [b"ACGTNNACGTACGTAC", b"NNNN"]
    reads = [b"ACGTNNACGTACGTAC", b"acgtnnacgtacgtac", b"ACGTACACGTACGTAC", b"ACGTRYACGTKMSWAC", b"NNNN", b"ACGT", b"\nCGT\x00NAC\xffTACGTAC", b"ACGTnNACGTACGTAC"]
    cands = [(0, 0), (0, 0), (0, 0), (0, 0), (1, 0), (1, 0), (0, 0), (0, 0)]
    v = _check(seqs, reads, cands, band)["reads"]
    if band == 0:
        assert v["edits"].tolist() == [2, 16, 2, 6, 4, 4, 4, 2] and v["n_match"].tolist() == [14, 0, 14, 10, 0, 0, 12, 14]
    assert (v["edits"][[0, 7]] == 2).all() and v["edits"][4] == 4


def test_no_overlap_no_candidate_and_empty_inputs():
    seqs = [b"ACGTACGT", b"TTTTT"]
    reads = [b"ACGT", b"ACGT", b"ACGT", b"ACGT", b"", b"", b"ACGT"]
    cands = [(0, 8), (0, -4), (1, 1 << 40), (1, -(1 << 40)), (0, 0), None, None]
    v = _check(seqs, reads, cands, 4)
    assert v["reads"]["clip_hi"].tolist() == [4, 4, 4, 4, 0, 0, 0] and v["reads"]["n_ops"].tolist() == [1, 1, 1, 1, 0, 0, 0]
    assert v["ops"].tolist() == [(4 << 4) | 4] * 4 and v["reads"]["seq"].tolist() == [0, 0, 1, 1, 0, E.NO_SEQUENCE, E.NO_SEQUENCE]
    for band in (0, 8):
        _check(seqs, [], [], band)
        _check([], [b"ACGT"], [None], band)
        _check([b"", b"A"], [b"ACGT", b"ACGT"], [(0, 0), (1, -1)], band)
        _check(seqs, [b""], [(0, 3)], band)


@pytest.mark.parametrize("band", [0, 2, 8])
def test_more_short_reads_than_one_grid(band):
    rng = np.random.default_rng(7)
    seqs = [_dna(rng, 29), _dna(rng, 64)]
    kinds = [(bytes(seqs[1][d:d + 3]) if k % 3 else _dna(rng, 3), (1, d) if k % 5 else None) for k, d in enumerate(range(61))]
    small = E.read_align(seqs, [r for r, _ in kinds], [c for _, c in kinds], band)
    reps = 70000 // len(kinds) + 1
    assert reps * len(kinds) >= 70000
    per = np.diff(small["op_offsets"].astype(np.int64))
    exp = dict(reads=np.tile(small["reads"], reps), ops=np.tile(small["ops"], reps), op_offsets=np.concatenate(([0], np.cumsum(np.tile(per, reps)))).astype(np.uint64))
    _check(seqs, [r for r, _ in kinds] * reps, [c for _, c in kinds] * reps, band, exp=exp)


def test_passes_over_a_small_budget_give_the_same_bytes(monkeypatch):
    rng = np.random.default_rng(8)
    seqs = [_dna(rng, 9), _dna(rng, 600)]
    reads, cands = [], []
    for r in range(120):
        start = int(rng.integers(0, 440))
        reads.append(_edit(rng, seqs[1][start:start + int(rng.integers(1, 151))], 3))
        cands.append((1, start) if r % 11 else None)
    exp = E.read_align(seqs, reads, cands, 8)
    monkeypatch.delenv("PGX_ALIGN_BUDGET_MB", raising=False)
    _check(seqs, reads, cands, 8, exp=exp)
    for mb in ("0.01", "0.002", "0.0012"):  # 8 bytes a read position at W = 8: about eight reads a pass, two, one
        monkeypatch.setenv("PGX_ALIGN_BUDGET_MB", mb)
        _check(seqs, reads, cands, 8, exp=exp)
    monkeypatch.setenv("PGX_ALIGN_BUDGET_MB", "0.001")  # 1048 bytes: a read of 150 needs 1200
    long_at = next(r for r, x in enumerate(reads) if len(x) * 8 > 1048)
    with pytest.raises(P.PgxError) as e:
        P.read_align_arrays(0, *_arrays(seqs, reads, cands), band=8, flags=P.ALIGN_CIGAR)
    assert e.value.code == P.ERR_NOMEM and "read %d needs" % long_at in str(e.value) and "PGX_ALIGN_BUDGET_MB" in str(e.value)
    _check(seqs, reads, cands, 0, exp=None)  # 2 bytes a position at W = 0: the same budget holds every read


def test_refusals_write_nothing():
    seqs, reads, cands = [b"ACGTACGT", b"TTTT"], [b"ACGT", b"CGTTA", b"GGGG"], [(0, 0), (0, 1), (1, 1)]
    text, seq_off, rd, read_off, cseq, cdiag = _arrays(seqs, reads, cands)
    mark = lambda: dict(reads=np.full(3, 0xA5, np.uint8).repeat(64).view(P.ALIGN_DTYPE), op_offsets=np.full(4, 0xA5A5, np.uint64), ops=np.full(16, 0xA5A5A5A5, np.uint32))

    def refused(code, needle, **kw):
        a = dict(text=text, seq_offsets=seq_off, reads=rd, read_offsets=read_off, cand_seq=cseq, cand_diag=cdiag, band=4, flags=P.ALIGN_CIGAR)
        a.update(kw)
        out = mark()
        with pytest.raises(P.PgxError) as e:
            P.read_align_arrays(0, a["text"], a["seq_offsets"], a["reads"], a["read_offsets"], a["cand_seq"], a["cand_diag"], band=a["band"], flags=a["flags"],
                                ops_cap=a.get("ops_cap", 16), out=out)
        assert e.value.code == code and needle in str(e.value), str(e.value)
        clean = mark()
        for k in clean:
            assert out[k].tobytes() == clean[k].tobytes(), k

    refused(P.ERR_ARG, "unknown flag", flags=2)
    refused(P.ERR_ARG, "band 32", band=32)
    for name, item in (("seq_offsets", "sequence 1"), ("read_offsets", "read 1")):
        o = dict(seq_offsets=seq_off, read_offsets=read_off)[name].copy()
        o[0] = 1
        refused(P.ERR_ARG, name + " must start at 0", **{name: o})
        o[0] = 0
        o[1] = o[2] + 1 if name != "seq_offsets" else o[-1] + 1
        refused(P.ERR_ARG, name + " decrease at " + item, **{name: o})
    bad_seq = cseq.copy()
    bad_seq[1] = 2
    bad_seq[2] = 7
    refused(P.ERR_ARG, "read 1 has a candidate whose sequence is not below n_seq 2", cand_seq=bad_seq)
    bad_text = text.copy()
    bad_text[5] = ord("a")
    refused(P.ERR_UNSUPPORTED, "text byte 97 at offset 5", text=bad_text)
    exp = E.read_align(seqs, reads, cands, 4)
    assert E.cigar_text(exp["ops"]) == "4=2=1I2=3X1S"
    refused(P.ERR_NOMEM, "6 operations, ops_cap is 5", ops_cap=5)
    # and what is not refused: the same call with room
    out = mark()
    got = P.read_align_arrays(0, text, seq_off, rd, read_off, cseq, cdiag, band=4, flags=P.ALIGN_CIGAR, ops_cap=16, out=out)
    assert got["reads"].tobytes() == exp["reads"].tobytes() and got["ops"].tobytes() == exp["ops"].tobytes()
