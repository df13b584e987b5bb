"""GPU tier of the verify kernels at their borders, through pgx_read_verify_arrays against tests/verify_emu.py, byte for byte, records and
list: every word offset of the text window against every read length around a word, overhang and non-overlap, the shortest sequences and the
padding behind the last one, the symbols that never match, segment ties, 64 candidates with tied winners, empty inputs, more reads than one
grid of single-word reads, and every call it refuses."""
import numpy as np
import pytest

import pgx_ffi as P
import verify_emu as E

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 150, 255, 256, 257, 1000)


def _arrays(seqs, reads, cands):
    seq_off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.uint64)
    read_off = np.concatenate(([0], np.cumsum([len(r) for r in reads]))).astype(np.uint64)
    cand_off = np.concatenate(([0], np.cumsum([len(c) for c in cands]))).astype(np.uint64)
    flat = [c for mine in cands for c in mine]
    return (np.frombuffer(b"".join(seqs), np.uint8), seq_off, np.frombuffer(b"".join(reads), np.uint8), read_off, cand_off,
            np.array([q for q, _ in flat], np.uint32), np.array([d for _, d in flat], np.int64))


def _check(seqs, reads, cands, penalty=4, exp=None):
    """records and list of the library == the emulator; without PGX_VERIFY_LIST the same records.  Returns the emulator's result."""
    seqs, reads = [bytes(s) for s in seqs], [bytes(r) for r in reads]
    if exp is None:
        exp = E.read_verify(seqs, reads, cands, penalty)
    args = _arrays(seqs, reads, cands)
    got = P.read_verify_arrays(0, *args, penalty=penalty, flags=P.VERIFY_LIST)
    assert got["reads"].dtype == E.VERIFY_DTYPE == P.VERIFY_DTYPE
    bad = np.flatnonzero(got["cands"] != exp["cands"]) if len(got["cands"]) == len(exp["cands"]) else [-1]
    assert len(bad) == 0, (len(bad), int(bad[0]), got["cands"][bad[0]], exp["cands"][bad[0]])
    bad = np.flatnonzero(got["reads"] != exp["reads"])
    assert len(bad) == 0, (len(bad), int(bad[0]), got["reads"][bad[0]], exp["reads"][bad[0]])
    for k in ("reads", "cand_offsets", "cands"):
        assert got[k].tobytes() == exp[k].tobytes(), k
    plain = P.read_verify_arrays(0, *args, penalty=penalty, flags=0)
    assert plain["reads"].tobytes() == exp["reads"].tobytes() and plain["cands"] is None and plain["cand_offsets"] is None
    return exp


def _dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), size=n))


def _mutate(rng, s, rate):
    a = bytearray(s)
    for i in np.flatnonzero(rng.random(len(a)) < rate):
        a[i] = b"ACGT"[(b"ACGT".index(a[i]) + 1 + int(rng.integers(0, 3))) % 4] if a[i] in b"ACGT" else ord("A")
    return bytes(a)


def test_every_diagonal_residue_and_length():
    """a sequence of 300 symbols behind one of 5 (so that sequence offsets and text words do not line up), reads cut from it with a few
    substitutions and laid on every diagonal 0 .. 31: reads longer than what is left hang over the end"""
    rng = np.random.default_rng(1)
    seqs = [_dna(rng, 5), _dna(rng, 300, b"ACGTACGTACGTN")]
    reads, cands = [], []
    for length in LENGTHS:
        for diag in range(32):
            src = seqs[1][diag:diag + length]
            reads.append(_mutate(rng, src + _dna(rng, length - len(src)), 0.05))
            cands.append([(1, diag)])
    exp = _check(seqs, reads, cands)
    v = exp["reads"]
    assert (v["mismatches"] > 0).any() and (v["seg_mismatches"] > 0).any() and (v["span_hi"] < [len(r) for r in reads]).any()
    assert (v["matches"] == 0).any() and (v["longest_run"] > 20).any()


def test_overhang_and_non_overlap():
    rng = np.random.default_rng(2)
    seqs = [_dna(rng, 40), _dna(rng, 100), _dna(rng, 33)]
    whole = seqs[1]
    reads = [_dna(rng, 13) + whole[:37], whole[80:] + _dna(rng, 25), _dna(rng, 21) + whole + _dna(rng, 30), whole[:50], whole[:50], whole[:50], whole[:50], b"", whole[:9]]
    cands = [[(1, -13)], [(1, 80)], [(1, -21)], [(1, 100)], [(1, -50)], [(1, 1000000)], [(1, -(1 << 40))], [(1, 3)], [(1, 99), (1, -8), (1, 101), (1, -9)]]
    exp = _check(seqs, reads, cands)["reads"]
    assert (exp["span_lo"][0], exp["span_hi"][0], exp["mismatches"][0]) == (13, 50, 0)
    assert (exp["span_lo"][1], exp["span_hi"][1], exp["mismatches"][1]) == (0, 20, 0)
    assert (exp["span_lo"][2], exp["span_hi"][2], exp["matches"][2]) == (21, 121, 100)
    assert not exp["span_hi"][3:8].any() and not exp["matches"][3:8].any()


def test_shortest_sequences_and_the_end_of_the_text():
    rng = np.random.default_rng(3)
    for last in (1, 8, 9, 23):
        seqs = [b"G", _dna(rng, 8), _dna(rng, 9), _dna(rng, last)]
        reads, cands = [], []
        for q, s in enumerate(seqs):
            for pre, post in ((0, 0), (3, 0), (0, 5), (2, 40)):
                reads.append(_dna(rng, pre) + s + _dna(rng, post))
                cands.append([(q, -pre)])
            reads.append(s[-1:] + b"ACGTACGTACGTACGTACGT")  # the span ends on the last symbol of the sequence (of the text, for the last one)
            cands.append([(q, len(s) - 1)])
        exp = _check(seqs, reads, cands)["reads"]
        assert (exp["matches"] == exp["span_hi"] - exp["span_lo"]).all() and (exp["matches"] > 0).all()


def test_symbols_that_never_match():
    seqs = [b"ACGTNNACGTACGTAC", b"NNNN"]
    reads = [b"ACGTNNACGTACGTAC", b"acgtnnacgtacgtac", b"ACGTACACGTACGTAC", b"ACGTRYACGTKMSWAC", b"NNNN", b"ACGT", b"\nCGT\x00NAC\xffTACGTAC"]
    cands = [[(0, 0)], [(0, 0)], [(0, 0)], [(0, 0)], [(1, 0)], [(1, 0)], [(0, 0)]]
    exp = _check(seqs, reads, cands)["reads"]
    assert exp["mismatches"].tolist() == [2, 16, 2, 6, 4, 4, 4] and exp["matches"].tolist() == [14, 0, 14, 10, 0, 0, 12]


@pytest.mark.parametrize("penalty", [1, 2, 4, 7, 1 << 20])
def test_segment_ties(penalty):
    rng = np.random.default_rng(penalty)
    base = _dna(rng, 64)
    other = bytes(b"ACGT"[(b"ACGT".index(c) + 1) % 4] for c in base)
    pick = lambda pattern: bytes(base[i] if x == "M" else other[i] for i, x in enumerate(pattern))
    patterns = ["MMMMXMMMM", "MMXMM", "M" * 40, "X" * 17, "MXM", "MXMM", "MMXMMM", "X" + "M" * 8 + "X" * 3 + "M" * 8, "MM" + "XM" * 20, "M" * 10 + "X" + "M" * (penalty % 50),
                "M" * 9 + "X" + "M" * 9 + "X" + "M" * 9]
    reads = [pick(p) for p in patterns]
    for shift in (0, 3):  # the same patterns at another word offset
        exp = _check([base[:shift], base], reads, [[(1, 0)]] * len(reads), penalty)["reads"]
        assert (exp["seg_start"][0], exp["seg_end"][0]) == ((0, 4) if penalty >= 4 else (0, 9))
        assert (exp["seg_start"][2], exp["seg_end"][2], exp["seg_score"][2]) == (0, 40, 40)
        assert (exp["seg_start"][3], exp["seg_end"][3], exp["seg_score"][3]) == (0, 0, 0)
        if penalty == 1:
            assert (exp["seg_start"][4], exp["seg_end"][4]) == (0, 1) and (exp["seg_start"][5], exp["seg_end"][5], exp["seg_mismatches"][5]) == (0, 4, 1)


def test_sixty_four_candidates_and_tied_winners():
    rng = np.random.default_rng(5)
    unit = _dna(rng, 50)
    variants = [unit, _mutate(rng, unit, 0.04), unit[:25] + b"N" + unit[26:], unit]
    seqs = [variants[k % 4] + _dna(rng, k % 7) for k in range(64)]
    cands = [[(k, 0) for k in range(64)], [(63 - k, (k + 1) % 3) for k in range(64)], [(k % 64, -(k % 5)) for k in range(200)]]
    exp = _check(seqs, [unit, unit, unit[:41]], cands)
    assert exp["reads"]["n_cand"].tolist() == [64, 64, 200] and exp["reads"]["n_tied"][0] == 32 and exp["reads"]["cand_index"][0] == 0
    assert exp["reads"]["cand_index"][1] == 8 and exp["reads"]["seq"][1] == 55  # the first candidate on diagonal 0 of an exact copy


def test_empty_inputs():
    seqs = [b"ACGTACGT"]
    exp = _check(seqs, [b"ACGT", b"ACGT", b""], [[], [(0, 4)], []])["reads"]
    assert exp["seq"].tolist() == [E.NO_SEQUENCE, 0, E.NO_SEQUENCE] and exp["n_cand"].tolist() == [0, 1, 0]
    _check(seqs, [], [])
    _check(seqs, [b"ACGT"], [[]])
    _check([], [b"ACGT"], [[]])
    _check([b"", b"A"], [b"ACGT"], [[(0, 0), (1, 0)]])


def test_more_single_word_reads_than_one_grid():
    rng = np.random.default_rng(6)
    seqs = [_dna(rng, 29), _dna(rng, 64)]
    kinds = [(bytes(seqs[1][d:d + 3]) if k % 3 else _dna(rng, 3), [(1, d)] if k % 5 else [(1, d), (0, d % 27)]) for k, d in enumerate(range(61))]
    small = E.read_verify(seqs, [r for r, _ in kinds], [c for _, c in kinds], 4)
    reps = 70000 // len(kinds) + 1
    n = reps * len(kinds)
    assert n >= 70000
    per = np.diff(small["cand_offsets"].astype(np.int64))
    exp = dict(reads=np.tile(small["reads"], reps), cands=np.tile(small["cands"], reps),
               cand_offsets=np.concatenate(([0], np.cumsum(np.tile(per, reps)))).astype(np.uint64))
    _check(seqs, [r for r, _ in kinds] * reps, [c for _, c in kinds] * reps, 4, exp=exp)


def test_refusals_write_nothing():
    seqs, reads, cands = [b"ACGTACGT", b"TTTT"], [b"ACGT", b"CGTA", b"GGGG"], [[(0, 0)], [(1, 0), (0, 1)], [(1, 1)]]
    text, seq_off, rd, read_off, cand_off, cseq, cdiag = _arrays(seqs, reads, cands)
    mark = lambda: dict(reads=np.full(3, 0xA5, np.uint8).repeat(64).view(P.VERIFY_DTYPE), cand_offsets=np.full(4, 0xA5A5, np.uint64),
                        cands=np.full(4 * 64, 0xA5, np.uint8).view(P.VERIFY_DTYPE))

    def refused(code, needle, **kw):
        a = dict(text=text, seq_offsets=seq_off, reads=rd, read_offsets=read_off, cand_offsets=cand_off, cand_seq=cseq, cand_diag=cdiag, penalty=4, flags=P.VERIFY_LIST)
        a.update(kw)
        out = mark()
        with pytest.raises(P.PgxError) as e:
            P.read_verify_arrays(0, a["text"], a["seq_offsets"], a["reads"], a["read_offsets"], a["cand_offsets"], a["cand_seq"], a["cand_diag"], penalty=a["penalty"],
                                 flags=a["flags"], list_cap=a.get("list_cap"), out=out)
        assert e.value.code == code and needle in str(e.value), str(e.value)
        clean = mark()
        for k in clean:
            assert out[k].tobytes() == clean[k].tobytes(), k

    refused(P.ERR_ARG, "unknown flag", flags=2)
    refused(P.ERR_ARG, "mismatch_penalty 0", penalty=0)
    refused(P.ERR_ARG, "mismatch_penalty %d" % ((1 << 20) + 1), penalty=(1 << 20) + 1)
    for name, item in (("seq_offsets", "sequence 1"), ("read_offsets", "read 1"), ("cand_offsets", "read 1")):
        o = dict(seq_offsets=seq_off, read_offsets=read_off, cand_offsets=cand_off)[name].copy()
        o[0] = 1
        refused(P.ERR_ARG, name + " must start at 0", **{name: o})
        o[0] = 0
        o[1] = o[2] + 1 if name != "seq_offsets" else o[-1] + 1
        refused(P.ERR_ARG, name + " decrease at " + item, **{name: o})
    bad_seq = cseq.copy()
    bad_seq[2] = 2
    bad_seq[3] = 7
    refused(P.ERR_ARG, "read 1 has a candidate whose sequence is not below n_seq 2", cand_seq=bad_seq)
    bad_text = text.copy()
    bad_text[5] = ord("a")
    refused(P.ERR_UNSUPPORTED, "text byte 97 at offset 5", text=bad_text)
    refused(P.ERR_NOMEM, "4 candidates, list_cap is 3", list_cap=3)
    # and what is not refused: the same call with room
    out = mark()
    got = P.read_verify_arrays(0, text, seq_off, rd, read_off, cand_off, cseq, cdiag, flags=P.VERIFY_LIST, out=out)
    assert got["reads"].tobytes() == E.read_verify(seqs, reads, cands)["reads"].tobytes()
