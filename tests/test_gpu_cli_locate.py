"""GPU tier: `find_mems --locate positions|seqs` prints the committed golden outputs with two more lines per MEM block, computed here
from pgx_locate_batch on the MEMs' ranges (tests/locate_format.py); the same bytes with several device workers and from FASTQ input;
without --locate the output is the golden itself; --locate-max leaves the MEMs above it unlocated."""
import os
import subprocess

import numpy as np
import pytest

import fastx_emu as E
import oracle_ffi as O
import pgx_ffi as P
from cli_format import strip_timing
from locate_format import mem_locate_lines, splice

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")
BT = os.path.join(O.GOLDEN, "bidirectional_test")
RI, TAGS = os.path.join(BT, "xy.ri"), os.path.join(BT, "xy_bidirectional_compressed.tags")


def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def _expected(reads_file, ml, mo, mode, max_occ=0):
    reads = [l for l in open(os.path.join(BT, reads_file), "rb").read().split(b"\n") if l]
    cat, offs = O.pack_reads(reads)
    idx = P.Index(RI, TAGS)
    mems = idx.find_mems(cat, offs, ml, mo)["mems"]  # (the product's MEMs: the golden's, tests/test_gpu_cli.py)
    size = mems["size"].astype(np.int64)
    ok = size > 0 if not max_occ else (size > 0) & (size <= max_occ)
    first = np.where(ok, mems["bwt_start"], 1).astype(np.uint64)
    last = np.where(ok, mems["bwt_start"].astype(np.int64) + size - 1, 0).astype(np.uint64)
    flags = 0 if mode == "positions" else P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE
    off, vals = idx.locate_batch(first, last, flags)
    ml_ = idx.info().max_length
    idx.close()
    golden = open(os.path.join(O.GOLDEN, "expected_find_mems_xy_%s_%d_%d.txt" % (reads_file.split(".")[0], ml, mo))).read()
    return golden, splice(golden, mem_locate_lines(mems, off, vals, mode, ml_)), cat, offs


@pytest.mark.parametrize("reads_file,ml,mo", [("reads.txt", 5, 1), ("test_reads.txt", 3, 1)])
@pytest.mark.parametrize("mode", ["positions", "seqs"])
def test_cli_locate_equals_golden_with_lines(built, workdir, reads_file, ml, mo, mode):
    golden, exp, cat, offs = _expected(reads_file, ml, mo, mode)
    assert exp != golden
    path = os.path.join(BT, reads_file)
    r = _run(RI, TAGS, path, ml, mo)
    assert r.returncode == 0, r.stderr
    assert strip_timing(r.stdout) == golden  # without --locate: the golden, byte for byte
    fq = os.path.join(workdir, "cli_locate_%s.fq" % reads_file)
    with open(fq, "wb") as f:
        f.write(E.write_fastq(cat, offs, seed=4))
    for src, extra in ((path, []), (path, ["--devices", "0,0", "--streams", "2", "--batch", "7"]), (path, ["--gpus", "1", "--quiet"]),
                       (fq, ["--reads-format", "fastq"]), (fq, ["--reads-format", "auto", "--devices", "0,0", "--streams", "2", "--batch", "5"])):
        r = _run(RI, TAGS, src, ml, mo, "--locate", mode, *extra)
        assert r.returncode == 0, r.stderr
        assert strip_timing(r.stdout) == exp, (src, extra)


def test_cli_locate_max(built):
    golden, exp, _, _ = _expected("reads.txt", 5, 1, "positions", max_occ=2)
    r = _run(RI, TAGS, os.path.join(BT, "reads.txt"), 5, 1, "--locate", "positions", "--locate-max", 2)
    assert r.returncode == 0, r.stderr
    assert strip_timing(r.stdout) == exp
    assert "(not located)" in exp or "SIZE: 3" not in golden


def test_cli_locate_compat_unsupported(built, workdir, x_index):
    enc = os.path.join(workdir, "cli_loc_x_enc.ri")
    P.build_rindex(os.path.join(O.GOLDEN, "x.rl_bwt"), enc, encoded=True)
    reads = os.path.join(workdir, "cli_loc_x_reads.txt")
    seqs = open(os.path.join(O.GOLDEN, "x.newline_separated"), "rb").read().split(b"\n")
    with open(reads, "wb") as f:
        f.write(b"\n".join(s[:120] for s in seqs if len(s) >= 120) + b"\n")
    r = _run(enc, x_index[1], reads, 10, 1, "--locate", "seqs")
    assert r.returncode == 1
    assert "PGX_MODE_STRICT" in r.stderr and "--mode strict" in r.stderr, r.stderr
    r = _run(enc, x_index[1], reads, 10, 1, "--locate", "seqs", "--mode", "strict")
    assert r.returncode == 0, r.stderr
