"""GPU tier: pgx_batch_upload_text parses reads as text on the device (include/pgx.h, PGX_READS_*).  LINES gives what
pgx_batch_upload of the same reads gives; FASTQ and FASTA give the CPU oracle's results on the sequences the Python rules
(tests/fastx_emu.py) find; a malformed text is refused with its record number and leaves the batch as it was."""
import os

import numpy as np
import pytest

import fastx_emu as E
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W

pytestmark = pytest.mark.gpu

ARRAYS = ("mem_offsets", "pos_offsets", "positions", "tag_run_counts")


def _same(a, b):
    assert a["n_extensions"] == b["n_extensions"]
    assert a["mems"].tobytes() == b["mems"].tobytes()
    for k in ARRAYS:
        if k in a or k in b:
            assert np.array_equal(a[k], b[k]), k


def _same_oracle(res, ref):
    assert res["n_extensions"] == ref["n_extensions"]
    assert np.array_equal(res["mem_offsets"], ref["mem_offsets"])
    assert res["mems"].tobytes() == ref["mems"].tobytes()
    assert np.array_equal(res["pos_offsets"], ref["pos_offsets"])
    assert np.array_equal(res["positions"], ref["positions"])


@pytest.fixture(scope="module")
def nidx(workdir):
    """a small sigma = 6 pangenome with N runs (reads over them take the side path)"""
    text = os.path.join(workdir, "fx6.txt")
    W.synth_pangenome_text(text, base_len=120_000, n_hap=2, seed=21, n_runs=3, n_run_len=(100, 2000))
    ri_path, tags_path = W.build_index_from_text(text, workdir, "fx6")[:2]
    return ri_path, tags_path, W.load_sequences(text)


def _mixed_reads(seqs, n, seed):
    """sampled reads (5 % over N runs), some lower case, some cut short, empty ones in between"""
    cat, offs = W.sample_reads(seqs, n, 150, seed=seed, n_frac=0.05)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        r = bytes(cat[int(offs[i]):int(offs[i + 1])])
        if i % 13 == 5:
            r = r.lower()
        if i % 17 == 2:
            r = r[: int(rng.integers(1, 150))]
        out.append(r)
        if i % 29 == 7:
            out.append(b"")
    return out


def test_lines_device_equals_upload(x_index):
    """LINES on the device == the host's line split through pgx_batch_upload: empty lines, '\\r', no final newline"""
    ri, tags = x_index
    idx = P.Index(ri, tags)
    seqs = W.load_sequences(os.path.join(O.GOLDEN, "x.newline_separated"))
    cat, offs = W.sample_reads(seqs, 3000, 150, seed=5)
    rng = np.random.default_rng(5)
    parts = []
    for i in range(3000):
        r = bytes(cat[int(offs[i]):int(offs[i + 1])])
        if i % 7 == 1:
            r += b"\r"
        if i % 11 == 3:
            r = r[: int(rng.integers(0, 40))]
        parts.append(r + b"\n" + (b"\n" if i % 5 == 0 else b""))
    text = b"\n\n" + b"".join(parts)
    for t in (text, text.rstrip(b"\n")):
        got_seqs, _ = E.parse(t, E.LINES)
        c2, o2 = E.to_batch(got_seqs)
        exp = idx.find_mems(c2, o2, 10, 1, tags=True)
        b = idx.batch_empty()
        try:
            assert b.upload_text(t, P.READS_LINES) == len(got_seqs)
            b.run(10, 1, P.RUN_TAGS)
            _same(b.result(), exp)
        finally:
            b.free()


@pytest.mark.parametrize("fmt,width,crlf", [(P.READS_FASTQ, 0, False), (P.READS_FASTQ, 0, True), (P.READS_FASTA, 0, False),
                                            (P.READS_FASTA, 60, False), (P.READS_FASTA, 60, True)])
def test_fastx_equals_oracle(nidx, fmt, width, crlf):
    """FASTQ / FASTA (unwrapped, 60 columns, CRLF) against the CPU oracle on the emu-parsed sequences; empty records are reads;
    one record of 100 kbp+ on a single line"""
    ri_path, tags_path, seqs = nidx
    reads = _mixed_reads(seqs, 4000, 31 + width)
    long = np.array(seqs[0][5000:5000 + 110_000])  # 1 % substitutions, as sample_reads has them (an exact copy of a haplotype is a quadratic read)
    rng = np.random.default_rng(width)
    flip = rng.random(len(long)) < 0.01
    long[flip] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(flip.sum()))]
    reads.insert(1234, long.tobytes())
    reads.append(b"")
    cat, offs = E.to_batch(reads)
    text = E.write_fastq(cat, offs, crlf=crlf) if fmt == P.READS_FASTQ else E.write_fasta(cat, offs, width=width, crlf=crlf)
    got_seqs, _ = E.parse(text, fmt)
    assert got_seqs == reads
    ref = O.find_mems_batch(O.RIndex(ri_path), O.Tags(tags_path, O.TAGS_COMPACT), cat, offs, 20, 1, threads=8)
    idx = P.Index(ri_path, tags_path)
    res = idx.find_mems_text(text, fmt, 20, 1, tags=True)
    assert len(res["mem_offsets"]) == len(reads) + 1
    _same_oracle(res, ref)
    assert len(res["mems"]) > 0 and int(res["mem_offsets"][1235] - res["mem_offsets"][1234]) > 0


def _fastq_fixed(cat, offs, L):
    """FASTQ of reads of one length L, built column-wise (a million records in a moment)"""
    n = len(offs) - 1
    rec = np.empty((n, 2 * L + 7), dtype=np.uint8)
    rec[:, 0:2] = np.frombuffer(b"@r", np.uint8)
    rec[:, 2] = 10
    rec[:, 3:3 + L] = np.asarray(cat, np.uint8).reshape(n, L)
    rec[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 6 + L:6 + 2 * L] = 73
    rec[:, 6 + L] = 64  # quality lines that start with '@'
    rec[:, 6 + 2 * L] = 10
    return rec.reshape(-1)


def test_million_reads_fastq_equals_upload(nidx):
    """one batch of 2^20 reads: upload_text(FASTQ) == upload of the same reads, device against device, over the whole length"""
    ri_path, tags_path, seqs = nidx
    n = 1 << 20
    cat, offs = W.sample_reads(seqs, n, 150, seed=77, n_frac=0.05)
    text = _fastq_fixed(cat, offs, 150)
    idx = P.Index(ri_path, tags_path)
    b1, b2 = idx.batch_empty(), idx.batch_empty()
    try:
        b1.upload(cat, offs)
        b1.run(20, 1, P.RUN_TAGS)
        exp = b1.result()
        assert b2.upload_text(text, P.READS_FASTQ) == n
        b2.run(20, 1, P.RUN_TAGS)
        _same(b2.result(), exp)
        assert len(exp["mems"]) > n
    finally:
        b1.free()
        b2.free()


@pytest.mark.parametrize("fmt,text,record,what", [
    (P.READS_FASTQ, b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\nIII\n", 2, "quality length 3 != sequence length 4"),
    (P.READS_FASTQ, b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\nIIII\n@c\nACGT\nIIII\n@d\nACGT\n+\nIIII\n", 3, "third line does not start with '+'"),
    (P.READS_FASTQ, b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\n", 2, "truncated record (3 of 4 lines)"),
    (P.READS_FASTQ, b"@a\nACGT\n+\nIIII\nb\nACGT\n+\nIIII\n", 2, "header line does not start with '@'"),
    (P.READS_FASTQ, b"@a\nACGT\nIIII", 1, "truncated record (3 of 4 lines)"),  # (the third line has no '+' either: the header line comes first)
    (P.READS_FASTA, b"ACGT\n>a\nACGT\n", 1, "text before the first '>'"),
])
def test_malformed_refused_batch_intact(x_index, fmt, text, record, what):
    ri, tags = x_index
    idx = P.Index(ri, tags)
    seqs = W.load_sequences(os.path.join(O.GOLDEN, "x.newline_separated"))
    cat, offs = W.sample_reads(seqs, 500, 150, seed=3)
    with pytest.raises(E.FastxError) as ee:
        E.parse(text, fmt)
    assert ee.value.record == record
    b = idx.batch_empty()
    try:
        b.upload(cat, offs)
        b.run(10, 1, P.RUN_TAGS)
        before = b.result()
        with pytest.raises(P.PgxError) as e:
            b.upload_text(text, fmt)
        assert e.value.code == P.ERR_FORMAT
        msg = str(e.value)
        assert ("record %d (byte %d): %s" % (record, ee.value.byte, what)) in msg, msg
        assert ("FASTQ" if fmt == P.READS_FASTQ else "FASTA") in msg
        _same(b.result(), before)  # the results of the last run are still there
        b.run(10, 1, P.RUN_TAGS)  # and so are its reads
        _same(b.result(), before)
    finally:
        b.free()
