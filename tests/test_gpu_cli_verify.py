"""GPU tier: `find_mems --verify FILE` writes one line per read with the record of Batch.read_verify (itself checked against
tests/verify_emu.py in tests/test_gpu_verify.py), formatted here in Python, and leaves stdout and stderr byte for byte what they are
without it -- with small batches and several workers, --locate, --format device, device-parsed reads and --place next to it;
--verify-only leaves stdout empty and does not go with --locate."""
import os
import subprocess

import pytest

import oracle_ffi as O
import pgx_ffi as P
from cli_format import strip_timing

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")
BT = os.path.join(O.GOLDEN, "bidirectional_test")
RI, TAGS, READS = os.path.join(BT, "xy.ri"), os.path.join(BT, "xy_bidirectional_compressed.tags"), os.path.join(BT, "reads.txt")
MIN_LEN = 3
HEADER = b"#read\tseq\tpos\tspan_lo\tspan_hi\tmatches\tmismatches\tseg_start\tseg_end\tseg_score\tseg_mismatches\trun\trun_start\tcands\ttied\n"
FIELDS = ("span_lo", "span_hi", "matches", "mismatches", "seg_start", "seg_end", "seg_score", "seg_mismatches", "longest_run", "run_start", "n_cand", "n_tied")


def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def _stderr(text):
    """stderr without the two lines that state load times"""
    return "\n".join(l for l in text.split("\n") if " took " not in l)


def _expected_text(max_cand, penalty):
    """the verify file of a run in the CLI's default mode, from the binding"""
    cat, offs = O.pack_reads([l for l in open(READS, "rb").read().split(b"\n") if l])
    idx = P.Index(RI, TAGS)
    b = P.Batch(idx, cat, offs)
    b.run(MIN_LEN, 1, 0)
    b.locate(0)
    b.read_place(P.PLACE_LIST if max_cand > 1 else 0)
    recs = b.read_verify(max_cand, penalty)["reads"]
    b.free()
    idx.close()
    lines = [HEADER]
    for i, x in enumerate(recs):
        where = ["*", "*"] if int(x["seq"]) == 0xFFFFFFFF else [str(int(x["seq"])), str(int(x["diag"]))]
        lines.append(("\t".join([str(i + 1)] + where + [str(int(x[f])) for f in FIELDS]) + "\n").encode())
    return b"".join(lines), recs


@pytest.fixture(scope="module")
def xy_expected(built):
    return _expected_text(1, 4)


@pytest.mark.parametrize("extra", [[], ["--batch", "7", "--streams", "2"], ["--locate", "seqs"], ["--format", "device", "--locate", "positions", "--batch", "5"],
                                   ["--device-parse", "--batch", "7"], ["--quiet"]])
def test_verify_file_and_unchanged_output(built, xy_expected, tmp_path, extra):
    out = str(tmp_path / "verify.tsv")
    plain = _run(RI, TAGS, READS, MIN_LEN, 1, *extra)
    verified = _run(RI, TAGS, READS, MIN_LEN, 1, *extra, "--verify", out)
    assert plain.returncode == 0 and verified.returncode == 0, verified.stderr
    assert strip_timing(verified.stdout) == strip_timing(plain.stdout) and len(plain.stdout) > 1000
    assert _stderr(verified.stderr) == _stderr(plain.stderr)
    text, recs = xy_expected
    assert open(out, "rb").read() == text
    assert (recs["seg_score"] > 0).any() and text.count(b"\n") == len(recs) + 1


def test_verify_max_and_mismatch_next_to_place(built, tmp_path):
    text, recs = _expected_text(16, 1)
    assert (recs["n_cand"] > 1).any()
    out, place, place_alone = str(tmp_path / "verify.tsv"), str(tmp_path / "place.tsv"), str(tmp_path / "place_alone.tsv")
    alone = _run(RI, TAGS, READS, MIN_LEN, 1, "--place", place_alone, "--batch", "7")
    both = _run(RI, TAGS, READS, MIN_LEN, 1, "--place", place, "--verify", out, "--verify-max", 16, "--verify-mismatch", 1, "--batch", "7")
    assert alone.returncode == 0 and both.returncode == 0, both.stderr
    assert open(out, "rb").read() == text and open(place, "rb").read() == open(place_alone, "rb").read()
    assert strip_timing(both.stdout) == strip_timing(alone.stdout)
    for bad in (["--verify-max", "0"], ["--verify-max", "65"], ["--verify-mismatch", "0"], ["--verify-mismatch", "x"]):
        r = _run(RI, TAGS, READS, MIN_LEN, 1, "--verify", out, *bad)
        assert r.returncode == 1 and bad[0] in r.stderr


def test_verify_only_leaves_stdout_empty(built, xy_expected, tmp_path):
    for extra in ([], ["--batch", "7", "--streams", "2"], ["--format", "device"]):
        out = str(tmp_path / "only.tsv")
        r = _run(RI, TAGS, READS, MIN_LEN, 1, "--verify", out, "--verify-only", *extra)
        assert r.returncode == 0, r.stderr
        assert r.stdout == "" and "[find_all_mems]" not in r.stderr
        assert open(out, "rb").read() == xy_expected[0]
    out, place = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")
    r = _run(RI, TAGS, READS, MIN_LEN, 1, "--verify", out, "--place", place, "--place-only")  # either of the two suppresses the text
    assert r.returncode == 0 and r.stdout == "" and open(out, "rb").read() == xy_expected[0]


def test_verify_only_does_not_go_with_locate(built, tmp_path):
    out = str(tmp_path / "refused.tsv")
    for only in ("--verify-only", "--place-only"):
        r = _run(RI, TAGS, READS, MIN_LEN, 1, "--verify", out, "--place", out + ".place", only, "--locate", "positions")
        assert r.returncode == 1 and r.stdout == "" and only in r.stderr and not os.path.exists(out)
    r = _run(RI, TAGS, READS, MIN_LEN, 1, "--verify-only")
    assert r.returncode == 1


def test_an_image_without_locate_is_refused(built, tmp_path):
    img = str(tmp_path / "xy_nolocate.pgi")
    tool = os.path.join(ROOT, "pangenome-index_amd", "pgx_image")
    made = subprocess.run([tool, RI, TAGS, img, "--no-locate"], capture_output=True, text=True, timeout=300)
    assert made.returncode == 0, made.stderr
    out = str(tmp_path / "refused.tsv")
    r = _run(img, "-", READS, MIN_LEN, 1, "--verify", out)
    assert r.returncode == 1 and r.stdout == "", r.stderr
    assert "locate" in r.stderr and not os.path.exists(out)
