"""GPU tier: `find_mems --format device` (stdout and the per-read stderr lines are written on the device, pgx_batch_format; the host
only downloads and writes them) prints the committed goldens, and the same stdout and stderr as `--format host` with --locate, small
batches, several workers, --quiet, --result compact, device-parsed FASTQ and a batch of thousands of reads."""
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


def _same(host, dev, what):
    assert host.returncode == 0 and dev.returncode == 0, (what, dev.stderr)
    assert strip_timing(dev.stdout) == strip_timing(host.stdout), what
    assert _stderr(dev.stderr) == _stderr(host.stderr), what


# (the parameter list of tests/test_gpu_cli.py::test_cli_matches_committed_golden)
@pytest.mark.parametrize("reads_file,ml,mo", [("reads.txt", 5, 1), ("reads.txt", 3, 1), ("test_reads.txt", 3, 1)])
def test_cli_format_device_matches_committed_golden(built, reads_file, ml, mo):
    r = _run(RI, TAGS, os.path.join(BT, reads_file), ml, mo, "--format", "device")
    assert r.returncode == 0, r.stderr
    exp = open(os.path.join(O.GOLDEN, "expected_find_mems_xy_%s_%d_%d.txt" % (reads_file.split(".")[0], ml, mo))).read()
    assert strip_timing(r.stdout) == exp
    n_reads = len([l for l in open(os.path.join(BT, reads_file)).read().split("\n") if l])
    assert r.stderr.count("[find_all_mems] total mems=") == n_reads


@pytest.mark.parametrize("extra", [[], ["--locate", "positions"], ["--locate", "seqs"], ["--batch", "100"],
                                   ["--batch", "7", "--devices", "0,0", "--streams", "2"], ["--quiet"], ["--result", "compact"]])
def test_cli_format_device_equals_host_xy(built, extra):
    path = os.path.join(BT, "reads.txt")
    host = _run(RI, TAGS, path, 3, 1, "--format", "host", *extra)
    dev = _run(RI, TAGS, path, 3, 1, "--format", "device", *extra)
    _same(host, dev, extra)
    assert len(host.stdout) > 1000
    assert strip_timing(_run(RI, TAGS, path, 3, 1, *extra).stdout) == strip_timing(host.stdout)  # (host is the default)


def test_cli_format_device_fastq_device_parse(built, workdir):
    """a small FASTQ parsed on the device: a batch formats once every range before it has been counted (its first read's number)"""
    reads = [l for l in open(os.path.join(BT, "reads.txt")).read().split("\n") if l]
    path = os.path.join(workdir, "format_reads.fastq")
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    for extra in ([], ["--batch", "5", "--streams", "3"]):
        args = (RI, TAGS, path, 3, 1, "--reads-format", "fastq", "--device-parse") + tuple(extra)
        _same(_run(*args, "--format", "host"), _run(*args, "--format", "device"), extra)
    assert strip_timing(_run(RI, TAGS, path, 3, 1, "--reads-format", "fastq", "--device-parse", "--format", "device").stdout) == \
        strip_timing(_run(RI, TAGS, os.path.join(BT, "reads.txt"), 3, 1).stdout)


def test_cli_format_device_equals_host_many_reads(built, x_index, workdir):
    """5000 reads: --batch 4500 is one batch of several formatter parts on the host side and a second, short batch"""
    ri, tags = x_index
    seqs = W.load_sequences(os.path.join(O.GOLDEN, "x.newline_separated"))
    cat, offs = W.sample_reads(seqs, 5000, 150, seed=78)
    path = os.path.join(workdir, "format_reads5000.txt")
    with open(path, "wb") as f:
        for i in range(5000):
            f.write(bytes(cat[offs[i]:offs[i + 1]]) + b"\n")
    for extra in (["--batch", "4500"], ["--locate", "positions", "--mode", "strict"]):
        host = _run(ri, tags, path, 10, 1, "--format", "host", *extra)
        dev = _run(ri, tags, path, 10, 1, "--format", "device", *extra)
        _same(host, dev, extra)
        assert host.stdout.count("Seq: ") == 5000


def test_cli_format_option_errors(built):
    r = _run(RI, TAGS, os.path.join(BT, "reads.txt"), 5, 1, "--format", "gpu")
    assert r.returncode == 1 and "--format: host or device" in r.stderr
    r = _run(RI, TAGS, os.path.join(BT, "reads.txt"), 5, 1, "--format", "device", "--result", "dense")
    assert r.returncode == 1 and "--result: full or compact" in r.stderr
