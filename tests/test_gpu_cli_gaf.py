"""GPU tier: `find_mems --gaf FILE` writes one GAF line per read, equal to tests/walk_emu.py's gaf_line made from the records of Batch.read_align
and Batch.read_walk (themselves checked against the emulators in tests/test_gpu_align.py and tests/test_gpu_walk.py), and leaves stdout and
stderr byte for byte what they are without it -- with small batches and several workers, --locate, --format device and device-parsed reads;
it composes with --align FILE and takes --align-band and the verify options; --gaf-only leaves stdout empty and does not go with --locate;
a tags argument of - on a .ri ends the run with status 1 and the library's message."""
import os
import subprocess

import pytest

import oracle_ffi as O
import pgx_ffi as P
import walk_emu as E
from cli_format import strip_timing

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")
BT = os.path.join(O.GOLDEN, "bidirectional_test")
RI, TAGS, READS = os.path.join(BT, "xy.ri"), os.path.join(BT, "xy_bidirectional_compressed.tags"), os.path.join(BT, "reads.txt")
MIN_LEN = 3


def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def _stderr(text):
    """stderr without the two lines that state load times"""
    return "\n".join(l for l in text.split("\n") if " took " not in l)


def _expected_text(band=8, max_cand=1, penalty=4):
    """the GAF file of a run in the CLI's default mode, from the bindings and the emulator's line"""
    reads = [l for l in open(READS, "rb").read().split(b"\n") if l]
    cat, offs = O.pack_reads(reads)
    idx = P.Index(RI, TAGS)
    b = P.Batch(idx, cat, offs)
    b.run(MIN_LEN, 1, 0)
    b.locate(0)
    b.read_place(P.PLACE_LIST if max_cand > 1 else 0)
    b.read_verify(max_cand, penalty)
    a = b.read_align(band, P.ALIGN_CIGAR)
    w = b.read_walk(P.WALK_STEPS)
    b.free()
    idx.close()
    lines = []
    for i, read in enumerate(reads):
        ops = a["ops"][int(a["op_offsets"][i]):int(a["op_offsets"][i + 1])]
        steps = w["steps"][int(w["step_offsets"][i]):int(w["step_offsets"][i + 1])]
        lines.append(E.gaf_line(i + 1, len(read), a["reads"][i], w["reads"][i], steps, ops) + "\n")
    return "".join(lines).encode(), w["reads"]


@pytest.fixture(scope="module")
def xy_expected(built):
    return _expected_text()


@pytest.mark.parametrize("extra", [[], ["--batch", "7", "--streams", "2"], ["--locate", "seqs"], ["--format", "device", "--locate", "positions", "--batch", "5"],
                                   ["--device-parse", "--batch", "7"], ["--quiet"]])
def test_gaf_file_and_unchanged_output(built, xy_expected, tmp_path, extra):
    out = str(tmp_path / "reads.gaf")
    plain = _run(RI, TAGS, READS, MIN_LEN, 1, *extra)
    walked = _run(RI, TAGS, READS, MIN_LEN, 1, *extra, "--gaf", out)
    assert plain.returncode == 0 and walked.returncode == 0, walked.stderr
    assert strip_timing(walked.stdout) == strip_timing(plain.stdout) and len(plain.stdout) > 1000
    assert _stderr(walked.stderr) == _stderr(plain.stderr)
    text, recs = xy_expected
    assert open(out, "rb").read() == text
    assert (recs["n_steps"] > 0).any() and text.count(b"\n") == len(recs) and b"\tcg:Z:" in text and (b">" in text or b"<" in text)


def test_gaf_next_to_align_with_the_stage_options(built, tmp_path):
    text, _ = _expected_text(2, 16, 1)
    gaf, align, align_alone = str(tmp_path / "reads.gaf"), str(tmp_path / "align.tsv"), str(tmp_path / "align_alone.tsv")
    opts = ["--verify-max", 16, "--verify-mismatch", 1, "--align-band", 2, "--batch", "7"]
    alone = _run(RI, TAGS, READS, MIN_LEN, 1, "--align", align_alone, *opts)
    both = _run(RI, TAGS, READS, MIN_LEN, 1, "--align", align, "--gaf", gaf, *opts)
    assert alone.returncode == 0 and both.returncode == 0, both.stderr
    assert open(gaf, "rb").read() == text and open(align, "rb").read() == open(align_alone, "rb").read()
    assert strip_timing(both.stdout) == strip_timing(alone.stdout)
    only = _run(RI, TAGS, READS, MIN_LEN, 1, "--gaf", gaf, *opts)  # the stage options without --verify or --align
    assert only.returncode == 0 and open(gaf, "rb").read() == text


def test_gaf_only_leaves_stdout_empty(built, xy_expected, tmp_path):
    for extra in ([], ["--batch", "7", "--streams", "2"], ["--format", "device"]):
        out = str(tmp_path / "only.gaf")
        r = _run(RI, TAGS, READS, MIN_LEN, 1, "--gaf", out, "--gaf-only", *extra)
        assert r.returncode == 0, r.stderr
        assert r.stdout == "" and "[find_all_mems]" not in r.stderr
        assert open(out, "rb").read() == xy_expected[0]


def test_gaf_only_does_not_go_with_locate(built, tmp_path):
    out = str(tmp_path / "refused.gaf")
    r = _run(RI, TAGS, READS, MIN_LEN, 1, "--gaf", out, "--gaf-only", "--locate", "positions")
    assert r.returncode == 1 and r.stdout == "" and "--gaf-only" in r.stderr and not os.path.exists(out)
    r = _run(RI, TAGS, READS, MIN_LEN, 1, "--gaf-only")
    assert r.returncode == 1


def test_an_index_without_tags_is_refused(built, tmp_path):
    out = str(tmp_path / "refused.gaf")
    r = _run(RI, "-", READS, MIN_LEN, 1, "--gaf", out)
    assert r.returncode == 1 and r.stdout == "", r.stderr
    assert "without a tag array" in r.stderr and "--gaf" in r.stderr and not os.path.exists(out)
