"""GPU tier: the find_mems CLI on FASTQ and FASTA files (--reads-format fastq|fasta|auto, parsed on the device) prints what the
oracle's results of the same records print, empty records included, over one batch and many; a line file parsed on the device
(--device-parse) prints what the host parse prints; a malformed file ends with the library's message and exit status 1."""
import os
import subprocess

import numpy as np
import pytest

import fastx_emu as E
import oracle_ffi as O
import pgx_workload as W
from cli_format import format_find_mems, strip_timing

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")


def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def reads(x_index, workdir):
    ri, tags = x_index
    seqs = W.load_sequences(os.path.join(O.GOLDEN, "x.newline_separated"))
    cat, offs = W.sample_reads(seqs, 2000, 150, seed=41)
    rs = [bytes(cat[int(offs[i]):int(offs[i + 1])]) for i in range(2000)]
    for k in (0, 777, 1999):
        rs[k] = b""  # empty records: reads without MEMs, numbered all the same
    rs[5] = rs[5].lower()
    cat, offs = E.to_batch(rs)
    ref = O.find_mems_batch(O.RIndex(ri), O.Tags(tags, O.TAGS_COMPACT), cat, offs, 10, 1, threads=4)
    paths = {}
    for name, text in (("r.fq", E.write_fastq(cat, offs, seed=2)), ("r_crlf.fq", E.write_fastq(cat, offs, crlf=True, seed=3)),
                       ("r.fa", E.write_fasta(cat, offs)), ("r60.fa", E.write_fasta(cat, offs, width=60)),
                       ("r.txt", E.write_lines(cat, offs, blank_every=9)[:-1])):
        paths[name] = os.path.join(workdir, name)
        with open(paths[name], "wb") as f:
            f.write(text)
    return paths, format_find_mems(ref), len(rs)


@pytest.mark.parametrize("name,fmt", [("r.fq", "fastq"), ("r_crlf.fq", "fastq"), ("r.fa", "fasta"), ("r60.fa", "fasta"), ("r.fq", "auto"),
                                      ("r60.fa", "auto")])
def test_cli_fastx_equals_oracle(x_index, reads, name, fmt):
    ri, tags = x_index
    paths, exp, n = reads
    for extra in ([], ["--batch", "300", "--devices", "0,0", "--streams", "2"]):
        r = _run(ri, tags, paths[name], 10, 1, "--reads-format", fmt, *extra)
        assert r.returncode == 0, r.stderr
        assert strip_timing(r.stdout) == exp
        assert r.stderr.count("[find_all_mems] total mems=") == n


def test_cli_lines_device_parse(x_index, reads):
    """a line file (blank lines, no final newline) parsed on the device == parsed on the host; also through --reads-format auto"""
    ri, tags = x_index
    paths, _, _ = reads
    base = _run(ri, tags, paths["r.txt"], 10, 1)
    assert base.returncode == 0, base.stderr
    for extra in (["--device-parse"], ["--device-parse", "--batch", "300", "--devices", "0,0", "--streams", "2", "--quiet"],
                  ["--reads-format", "auto", "--device-parse", "--batch", "777"]):
        r = _run(ri, tags, paths["r.txt"], 10, 1, *extra)
        assert r.returncode == 0, r.stderr
        assert strip_timing(r.stdout) == strip_timing(base.stdout)


def test_cli_fastq_format_error(x_index, reads, workdir):
    """a bad record in a later batch: exit 1, the library's message with the record and byte counted from the file's start"""
    ri, tags = x_index
    paths, _, _ = reads
    text = open(paths["r.fq"], "rb").read()
    ls = E.lines(text)
    at = ls[4 * 1500 + 3][0]  # the quality line of record 1501, one byte short
    bad = text[:at] + text[at + 1:]
    path = os.path.join(workdir, "bad.fq")
    with open(path, "wb") as f:
        f.write(bad)
    with pytest.raises(E.FastxError) as ee:
        E.parse(bad, E.FASTQ)
    assert ee.value.record == 1501
    r = _run(ri, tags, path, 10, 1, "--reads-format", "fastq", "--batch", "300", "--quiet")
    assert r.returncode == 1
    assert ("FASTQ record 1501 (byte %d): quality length" % ee.value.byte) in r.stderr, r.stderr
