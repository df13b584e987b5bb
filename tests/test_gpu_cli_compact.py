"""GPU tier: `find_mems --result compact` (the result crosses the link as the compact byte stream and the formatter threads expand it)
prints the committed goldens, and the same stdout and stderr as `--result full` with --locate, small batches, --quiet and a batch
large enough for several formatter threads."""
import os
import subprocess

import pytest

import oracle_ffi as O
import pgx_workload as W
from cli_format import strip_timing

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")
BT = os.path.join(O.GOLDEN, "bidirectional_test")
RI, TAGS = os.path.join(BT, "xy.ri"), os.path.join(BT, "xy_bidirectional_compressed.tags")


def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def _stderr(text):
    """stderr without the two lines that state load times"""
    return "\n".join(l for l in text.split("\n") if " took " not in l)


# (the parameter list of tests/test_gpu_cli.py::test_cli_matches_committed_golden)
@pytest.mark.parametrize("reads_file,ml,mo", [("reads.txt", 5, 1), ("reads.txt", 3, 1), ("test_reads.txt", 3, 1)])
def test_cli_compact_matches_committed_golden(built, reads_file, ml, mo):
    r = _run(RI, TAGS, os.path.join(BT, reads_file), ml, mo, "--result", "compact")
    assert r.returncode == 0, r.stderr
    exp = open(os.path.join(O.GOLDEN, "expected_find_mems_xy_%s_%d_%d.txt" % (reads_file.split(".")[0], ml, mo))).read()
    assert strip_timing(r.stdout) == exp
    n_reads = len([l for l in open(os.path.join(BT, reads_file)).read().split("\n") if l])
    assert r.stderr.count("[find_all_mems] total mems=") == n_reads


@pytest.mark.parametrize("extra", [["--locate", "positions"], ["--locate", "seqs"], ["--batch", "100"], ["--quiet"],
                                   ["--locate", "seqs", "--batch", "7", "--devices", "0,0", "--streams", "2"]])
def test_cli_compact_equals_full_xy(built, extra):
    path = os.path.join(BT, "reads.txt")
    full = _run(RI, TAGS, path, 3, 1, "--result", "full", *extra)
    comp = _run(RI, TAGS, path, 3, 1, "--result", "compact", *extra)
    assert full.returncode == 0 and comp.returncode == 0, comp.stderr
    assert strip_timing(comp.stdout) == strip_timing(full.stdout) and len(full.stdout) > 1000
    assert _stderr(comp.stderr) == _stderr(full.stderr)
    assert strip_timing(_run(RI, TAGS, path, 3, 1, *extra).stdout) == strip_timing(full.stdout)  # (full is the default)


def test_cli_compact_equals_full_many_reads(built, x_index, workdir):
    """5000 reads: one batch is cut into several formatter parts (on multiples of 64 reads), --batch 100 into batches that end inside a block"""
    ri, tags = x_index
    seqs = W.load_sequences(os.path.join(O.GOLDEN, "x.newline_separated"))
    cat, offs = W.sample_reads(seqs, 5000, 150, seed=78)
    path = os.path.join(workdir, "compact_reads5000.txt")
    with open(path, "wb") as f:
        for i in range(5000):
            f.write(bytes(cat[offs[i]:offs[i + 1]]) + b"\n")
    for extra in ([], ["--batch", "100"], ["--quiet", "--batch", "4500"], ["--locate", "positions", "--mode", "strict"]):
        full = _run(ri, tags, path, 10, 1, *extra)
        comp = _run(ri, tags, path, 10, 1, "--result", "compact", *extra)
        assert full.returncode == 0 and comp.returncode == 0, comp.stderr
        assert strip_timing(comp.stdout) == strip_timing(full.stdout), extra
        assert _stderr(comp.stderr) == _stderr(full.stderr), extra


def test_cli_result_option_errors(built):
    r = _run(RI, TAGS, os.path.join(BT, "reads.txt"), 5, 1, "--result", "dense")
    assert r.returncode == 1 and "--result: full or compact" in r.stderr
