"""CPU tier: the case tables of the device read parser (tests/fastx_cases.py) are what they claim.  The geometry literals are the kernels'
own (parsed from the sources), every text holds the bytes, the line count and the sequence total its case names, the emulator
(tests/fastx_emu.py) accepts or refuses it as the table says, and for LINES the emulator is bytes.split(b"\\n") stated directly.
pgx_batch_reads refuses its NULL arguments before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fastx_cases as FC
import fastx_emu as E
import pgx_ffi as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pangenome-index_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _kernel(src, name):
    """the text of one __global__ function of pgx_fastx_kernels.hip"""
    a = src.index(name + "(")
    b = src.find("\n}\n", a)
    assert b > a
    return src[a:b]


def test_literals_are_the_kernels_own():
    dev, kern, batch = _src("pgx_device.h"), _src("pgx_fastx_kernels.hip"), _src("pgx_batch.hip")
    rounds = int(re.search(r"^#define\s+PGX_FASTX_ROUNDS\s+(\d+)\b", dev, re.M).group(1))
    m = re.search(r"^#define\s+PGX_FASTX_TILE\s+\((\d+) \* (\d+) \* PGX_FASTX_ROUNDS\)", dev, re.M)
    threads, chunk = int(m.group(1)), int(m.group(2))
    assert (threads, chunk, rounds) == (256, FC.CHUNK, FC.TILE // FC.ROUND)
    assert threads * chunk == FC.ROUND and threads * chunk * rounds == FC.TILE
    for name in ("pgx_fastx_count_kernel", "pgx_fastx_lines_kernel"):  # a round is 4096 bytes, a thread's chunk 16
        body = _kernel(kern, name)
        assert "r * %d + threadIdx.x * %d" % (FC.ROUND, FC.CHUNK) in body and "__launch_bounds__(256)\n" + name in kern
    assert int(re.search(r"^#define\s+PGX_SCAN1_TILE_ITEMS\s+(\d+)\b", dev, re.M).group(1)) == FC.SCAN1_TILE_ITEMS
    copy = _kernel(kern, "pgx_fastx_copy_kernel")
    assert "blockIdx.x * %d;" % FC.COPY_BLOCK in copy and "threadIdx.x * 16;" in copy and "k < 16;" in copy
    # the launch shapes of batch_upload_text
    up = batch[batch.index("static void batch_upload_text("):batch.index('extern "C" pgx_status pgx_batch_create(')]
    launches = dict(re.findall(r"hipLaunchKernelGGL\((pgx_fastx_\w+), dim3\((.*?)\), dim3\(256\), 0, s,", up))
    assert set(launches) == {"pgx_fastx_%s_kernel" % k for k in ("count", "lines", "role", "records", "longest", "copy")}
    assert launches["pgx_fastx_count_kernel"] == launches["pgx_fastx_lines_kernel"] == "grid_for(n_tiles, 1)"
    assert launches["pgx_fastx_role_kernel"] == launches["pgx_fastx_records_kernel"] == "grid_for(n_lines, %d)" % FC.LINE_BLOCK
    assert launches["pgx_fastx_longest_kernel"] == "std::min<unsigned>(grid_for(n_lines, 256), 2048u)" and FC.LONGEST_GRID_READS == 2048 * 256
    assert launches["pgx_fastx_copy_kernel"] == "grid_for(total, %d)" % FC.COPY_BLOCK and FC.COPY_THREADS == 256 == FC.COPY_BLOCK // 16
    assert "(n_bytes + PGX_FASTX_TILE - 1) / PGX_FASTX_TILE" in up


def _n_lines(text):
    return text.count(b"\n") + (not text.endswith(b"\n"))


def _check(c):
    for pos, byte in c.at.items():
        assert c.text[pos] == byte, (c.name, pos)
    if c.n_lines is not None:
        assert _n_lines(c.text) == c.n_lines, c.name
    if c.fmt == E.LINES:  # the emulator against the rule stated directly
        parts = c.text.split(b"\n")
        seqs, starts = E.parse(c.text, E.LINES)
        assert seqs == [s for s in parts if s], c.name
        assert [c.text[a:a + len(s)] for a, s in zip(starts, seqs)] == seqs
    if c.ok:
        seqs, _ = E.parse(c.text, c.fmt)
        assert c.total is not None and sum(len(s) for s in seqs) == c.total, c.name
        return seqs
    with pytest.raises(E.FastxError) as e:
        E.parse(c.text, c.fmt)
    line_starts = [0] + [i + 1 for i in np.flatnonzero(np.frombuffer(c.text, np.uint8) == 10).tolist()]
    assert e.value.byte in line_starts and e.value.record >= 1, c.name
    return None


def test_small_cases_hold_their_borders():
    cases = FC.small_cases()
    for c in cases:
        _check(c)
    by = {c.name: c for c in cases}
    # table a: every position, both line ends, every format
    for p in FC.NEWLINE_AT:
        for f in ("lines", "fasta", "fastq"):
            assert by["nl_%d-%s" % (p, f)].text[p] == 10 and by["nl_crlf_%d-%s" % (p, f)].text[p:p + 2] == b"\r\n"
    assert {p % FC.CHUNK for p in FC.NEWLINE_AT} >= {0, 1, 15} and {FC.ROUND - 1, FC.ROUND, FC.TILE - 1, FC.TILE, 2 * FC.TILE - 1, 2 * FC.TILE} <= set(FC.NEWLINE_AT)
    # table b
    for n in FC.TEXT_LENGTHS:
        for f in ("lines", "fasta", "fastq"):
            a, b = by["len_%d-%s" % (n, f)].text, by["len_%d_nl-%s" % (n, f)].text
            assert len(a) == len(b) == n and b.endswith(b"\n") and not a.endswith(b"\n")
    # table c
    assert {FC.LINE_BLOCK + d for d in (-1, 0, 1)} | {FC.SCAN1_TILE_ITEMS + d for d in (-1, 0, 1)} == set(FC.LINE_COUNTS)
    assert by["newline_tile-lines"].text == b"\n" * FC.TILE and E.parse(by["newline_tile_then_read-fasta"].text, E.FASTA)[0] == [b"ACGTA"]
    assert E.parse(by["headers_only-fasta"].text, E.FASTA)[0] == [b"", b"", b""]
    assert not by["lines_255-fastq"].ok and by["lines_256-fastq"].ok and not by["lines_4097-fastq"].ok
    # table d
    t = by["width_1-fasta"].text
    assert max(len(l) for l in t.split(b"\n") if not l.startswith(b">")) == 1
    assert b"\n\n" in by["width_1_blanks-fasta"].text and b"\r\n\r\n" in by["width_1_crlf_blanks-fasta"].text
    offs = np.cumsum([0] + [len(s) for s in E.parse(by["read_over_4096-fastq"].text, E.FASTQ)[0]])
    assert offs[1] < FC.COPY_BLOCK < offs[2]
    assert max(len(l) for l in by["line_10000-lines"].text.split(b"\n")) == 10000
    assert [len(s) for s in E.parse(by["empty_all_over-fasta"].text, E.FASTA)[0]] == [0, 21, 0, 0, 0, 430, 0]
    assert any(c.name.startswith(FC.COPY_CASE_PREFIXES) for c in cases)


def test_error_matrix_messages():
    """what the emulator says of the refused cases, stated here once more for the ones the issue of the parser names"""
    by = {c.name: c for c in FC.small_cases()}

    def err(name):
        with pytest.raises(E.FastxError) as e:
            E.parse(by[name].text, by[name].fmt)
        return e.value.record, e.value.byte, str(e.value)

    assert err("err_truncated_3_no_plus_issue-fastq") == (1, 0, "FASTQ record 1 (byte 0): truncated record (3 of 4 lines)")
    for pos in (1, 65, 100):
        for kind, what in (("no_at", "header line does not start with '@'"), ("no_plus", "third line does not start with '+'"), ("qual_len", "quality length")):
            r, _, msg = err("err_%s_rec%d-fastq" % (kind, pos))
            assert r == pos and what in msg
        for have in (1, 2, 3):
            r, at, msg = err("err_truncated_%d_rec%d-fastq" % (have, pos))
            assert r == pos and "truncated record (%d of 4 lines)" % have in msg
            assert err("err_truncated_%d_rec%d_no_final_nl-fastq" % (have, pos))[:2] == (r, at)
            r2, at2, msg = err("err_truncated_%d_no_at_rec%d-fastq" % (have, pos))
            assert (r2, at2) == (r, at) and "does not start with '@'" in msg
        r, _, msg = err("err_truncated_3_no_plus_rec%d-fastq" % pos)
        assert r == pos and "truncated record (3 of 4 lines)" in msg
    # record 65 is lines 256 .. 259
    t = by["err_no_at_rec65-fastq"].text
    assert t[:err("err_no_at_rec65-fastq")[1]].count(b"\n") == FC.LINE_BLOCK
    for name in by:
        if name.startswith("err_two_late_"):
            assert err(name)[0] == 70
        if name.startswith("err_two_first_block_"):
            assert err(name)[0] == 3
    assert err("err_two_qual_len_truncated-fastq")[0] == 70
    assert err("err_before_first_behind_blanks-fasta")[:2] == (1, 4) and err("err_before_first_line256-fasta")[:2] == (1, FC.LINE_BLOCK)
    assert err("err_before_first_two-fasta")[:2] == (1, 3) and err("err_before_first_last_line-fasta")[:2] == (1, 600)


def test_big_cases_hold_their_borders():
    c = FC.many_reads_case()
    seqs = _check(c)
    assert len(seqs) == FC.MANY_READS + 1 > FC.LONGEST_GRID_READS and len(seqs[-1]) == 300 and max(len(s) for s in seqs[:-1]) == 1
    for fmt in (E.LINES, E.FASTA):
        c = FC.many_tiles_case(fmt)
        assert len(c.text) == FC.MANY_TILES * FC.TILE and FC.MANY_TILES > FC.SCAN1_TILE_ITEMS
        t = np.frombuffer(c.text, np.uint8).reshape(FC.MANY_TILES, FC.TILE)
        assert ((t == 10).sum(axis=1) == 1).all()  # one newline per tile
        phase = (t == 10).argmax(axis=1)
        assert {0, FC.CHUNK - 1, FC.CHUNK, FC.ROUND - 1, FC.ROUND, FC.TILE - 1} <= set(phase.tolist()) and len(set(phase.tolist())) > 4000
        seqs = _check(c)
        assert len(seqs) == (FC.MANY_TILES if fmt == E.LINES else 1)


def test_reads_null_arguments(built):
    L = P.lib()
    info = P.ReadsInfo()
    buf = (C.c_uint64 * 4)()
    assert L.pgx_batch_reads(None, C.byref(info), None, 0, None, 0) == P.ERR_ARG
    assert b"pgx_batch_reads" in L.pgx_last_error()
    assert L.pgx_batch_reads(None, None, None, 0, None, 0) == P.ERR_ARG
    assert L.pgx_batch_reads(None, C.byref(info), C.cast(buf, C.c_void_p), 4, C.cast(buf, C.c_void_p), 32) == P.ERR_ARG
    assert C.sizeof(P.ReadsInfo) == 24
