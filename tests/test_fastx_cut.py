"""pgx_fastx_cut (host side of the find_mems CLI's planner for FASTA / FASTQ / device-parsed line files): for every `want` of a
sweep it returns the smallest record start at or after `want`, len(text) when there is none.  CPU tier: record starts from the
Python restatement of the rules (tests/fastx_emu.py); the device parse itself is tests/test_gpu_fastx.py."""
import bisect

import numpy as np
import pytest

import fastx_emu as E
import pgx_ffi as P


def _reads(n, seed, empty_every=0, lower=False):
    rng = np.random.default_rng(seed)
    seqs = []
    for i in range(n):
        ln = 0 if empty_every and i % empty_every == 3 else int(rng.integers(1, 200))
        s = rng.choice(np.frombuffer(b"ACGTN" if not lower else b"acgtN", dtype=np.uint8), size=ln).tobytes()
        seqs.append(s)
    return E.to_batch(seqs)


def _check_sweep(text, fmt, wants=None):
    seqs, starts = E.parse(text, fmt)
    n = len(text)
    if wants is None:
        wants = range(n + 3) if n < 6000 else sorted(set(np.random.default_rng(n).integers(0, n + 2, size=3000).tolist()) | {0, 1, n - 1, n, n + 1})
    for w in wants:
        k = bisect.bisect_left(starts, w)
        exp = starts[k] if k < len(starts) else n
        got = P.fastx_cut(text, fmt, w)
        assert got == exp, (fmt, w, got, exp)
        if n < 6000:
            assert E.cut(text, fmt, w) == exp
    return seqs


@pytest.mark.parametrize("crlf", [False, True])
def test_cut_fastq(built, crlf):
    """quality lines that start with '@' and '+' are no record starts; CRLF"""
    cat, offs = _reads(60, 1, empty_every=17)
    text = E.write_fastq(cat, offs, crlf=crlf, seed=3)
    assert sum(1 for l in text.split(b"\n")[3::4] if l.startswith(b"@")) > 5  # the case the rule is there for
    seqs = _check_sweep(text, P.READS_FASTQ)
    assert len(seqs) == 60


def test_cut_fastq_large(built):
    cat, offs = _reads(3000, 2)
    _check_sweep(E.write_fastq(cat, offs, seed=4), P.READS_FASTQ)


def test_cut_fastq_missing_final_newline_and_short_tail(built):
    cat, offs = _reads(20, 5)
    text = E.write_fastq(cat, offs, seed=6)
    _check_sweep(text[:-1], P.READS_FASTQ)  # the last quality line without its newline
    # a last record of fewer than 4 lines: no record starts there (the parse refuses it; the cut gives len(text))
    short = text + b"@tail\nACGT\n+\n"
    n = len(short)
    for w in range(len(text) - 30, n + 1):
        got = P.fastx_cut(short, P.READS_FASTQ, w)
        assert got == E.cut(short, P.READS_FASTQ, w)
        assert got == n or got < len(text)


@pytest.mark.parametrize("width,crlf", [(0, False), (60, False), (7, True), (80, True)])
def test_cut_fasta(built, width, crlf):
    """wrapped and unwrapped, '>' inside headers, empty records"""
    cat, offs = _reads(50, 7, empty_every=9)
    text = E.write_fasta(cat, offs, width=width, crlf=crlf)
    seqs = _check_sweep(text, P.READS_FASTA)
    assert seqs == [bytes(cat[int(offs[i]):int(offs[i + 1])]) for i in range(50)]
    _check_sweep(text[:-1], P.READS_FASTA)
    _check_sweep(b"\n\n" + text + b"\n\n", P.READS_FASTA)  # blank lines before the first record and after the last


@pytest.mark.parametrize("crlf", [False, True])
def test_cut_lines(built, crlf):
    cat, offs = _reads(80, 8, empty_every=11)
    text = E.write_lines(cat, offs, blank_every=5, crlf=crlf)
    seqs = _check_sweep(text, P.READS_LINES)
    _check_sweep(text[:-1], P.READS_LINES)
    if not crlf:  # empty reads vanish in the line format
        assert seqs == [s for s in (bytes(cat[int(offs[i]):int(offs[i + 1])]) for i in range(80)) if s]


def test_cut_edges(built):
    for fmt in (P.READS_LINES, P.READS_FASTA, P.READS_FASTQ):
        assert P.fastx_cut(b"", fmt, 0) == 0
        assert P.fastx_cut(b"", fmt, 5) == 0
    assert P.fastx_cut(b">a\nAC", P.READS_FASTA, 1) == 5
    assert P.fastx_cut(b"x\n>a\nAC", P.READS_FASTA, 0) == 2
    assert P.fastx_cut(b"\n\nAC\n", P.READS_LINES, 0) == 2
    assert P.fastx_cut(b"@a\nAC\n+\nII", P.READS_FASTQ, 0) == 0


def test_cut_bad_format(built):
    with pytest.raises(P.PgxError) as e:
        P.fastx_cut(b">a\nACGT\n", 3, 0)
    assert e.value.code == P.ERR_ARG


def test_emu_rules():
    """the Python rules on small texts, errors included (the device parse is checked against them on the GPU)"""
    assert E.parse(b"AC\n\nG\r\nT", E.LINES)[0] == [b"AC", b"G\r", b"T"]
    assert E.parse(b"@a\nAC\r\n+\nII\r\n@b\n\n+\n\n", E.FASTQ)[0] == [b"AC", b""]
    assert E.parse(b"\n>a\nAC\r\n\nGT\n>b\n>c\nT", E.FASTA)[0] == [b"ACGT", b"", b"T"]
    for text, fmt, rec in ((b"@a\nACG\n+\nII\n", E.FASTQ, 1), (b"@a\nAC\n+\nII\n@b\nA\n", E.FASTQ, 2), (b"@a\nAC\n-\nII\n", E.FASTQ, 1),
                           (b"x\n>a\nAC\n", E.FASTA, 1), (b"@a\nAC\n+\nII\nb\nAC\n+\nII\n", E.FASTQ, 2)):
        with pytest.raises(E.FastxError) as e:
            E.parse(text, fmt)
        assert e.value.record == rec
