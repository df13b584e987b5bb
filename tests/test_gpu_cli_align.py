"""GPU tier: `find_mems --align FILE` writes one line per read with the record and the CIGAR of Batch.read_align (itself checked against
tests/align_emu.py in tests/test_gpu_align.py), formatted here in Python, and leaves stdout and stderr byte for byte what they are without
it -- with small batches and several workers, --locate, --format device, device-parsed reads and --verify / --place next to it;
--align-band outside 0 .. 31 prints the usage; --align-only leaves stdout empty and does not go with --locate."""
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
HEADER = b"#read\tseq\tstart\tend\tclip_lo\tclip_hi\tedits\tmatches\tmismatches\tins\tdel\tband_hit\tcigar\n"
FIELDS = ("clip_lo", "clip_hi", "edits", "n_match", "n_mismatch", "n_ins", "n_del", "band_hit")


def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def _stderr(text):
    """stderr without the two lines that state load times"""
    return "\n".join(l for l in text.split("\n") if " took " not in l)


def _expected_text(band, max_cand=1, penalty=4):
    """the align file of a run in the CLI's default mode, from the binding"""
    cat, offs = O.pack_reads([l for l in open(READS, "rb").read().split(b"\n") if l])
    idx = P.Index(RI, TAGS)
    b = P.Batch(idx, cat, offs)
    b.run(MIN_LEN, 1, 0)
    b.locate(0)
    b.read_place(P.PLACE_LIST if max_cand > 1 else 0)
    b.read_verify(max_cand, penalty)
    got = b.read_align(band, P.ALIGN_CIGAR)
    b.free()
    idx.close()
    lines = [HEADER]
    for i, x in enumerate(got["reads"]):
        ops = got["ops"][int(got["op_offsets"][i]):int(got["op_offsets"][i + 1])]
        none = int(x["seq"]) == 0xFFFFFFFF
        where = ["*", "*", "*"] if none else [str(int(x["seq"])), str(int(x["text_start"])), str(int(x["text_end"]))]
        cigar = "*" if none or len(ops) == 0 else P.cigar_text(ops)
        lines.append(("\t".join([str(i + 1)] + where + [str(int(x[f])) for f in FIELDS] + [cigar]) + "\n").encode())
    return b"".join(lines), got["reads"]


@pytest.fixture(scope="module")
def xy_expected(built):
    return _expected_text(8)


@pytest.mark.parametrize("extra", [[], ["--batch", "7", "--streams", "2"], ["--locate", "seqs"], ["--format", "device", "--locate", "positions", "--batch", "5"],
                                   ["--device-parse", "--batch", "7"], ["--quiet"]])
def test_align_file_and_unchanged_output(built, xy_expected, tmp_path, extra):
    out = str(tmp_path / "align.tsv")
    plain = _run(RI, TAGS, READS, MIN_LEN, 1, *extra)
    aligned = _run(RI, TAGS, READS, MIN_LEN, 1, *extra, "--align", out)
    assert plain.returncode == 0 and aligned.returncode == 0, aligned.stderr
    assert strip_timing(aligned.stdout) == strip_timing(plain.stdout) and len(plain.stdout) > 1000
    assert _stderr(aligned.stderr) == _stderr(plain.stderr)
    text, recs = xy_expected
    assert open(out, "rb").read() == text
    assert (recs["n_match"] > 0).any() and text.count(b"\n") == len(recs) + 1


def test_align_band_and_the_verify_options_next_to_verify_and_place(built, tmp_path):
    text, recs = _expected_text(2, 16, 1)
    out, verify, place, verify_alone = str(tmp_path / "align.tsv"), str(tmp_path / "verify.tsv"), str(tmp_path / "place.tsv"), str(tmp_path / "verify_alone.tsv")
    alone = _run(RI, TAGS, READS, MIN_LEN, 1, "--verify", verify_alone, "--verify-max", 16, "--verify-mismatch", 1, "--batch", "7")
    both = _run(RI, TAGS, READS, MIN_LEN, 1, "--place", place, "--verify", verify, "--verify-max", 16, "--verify-mismatch", 1, "--align", out, "--align-band", 2, "--batch", "7")
    assert alone.returncode == 0 and both.returncode == 0, both.stderr
    assert open(out, "rb").read() == text and open(verify, "rb").read() == open(verify_alone, "rb").read()
    assert strip_timing(both.stdout) == strip_timing(alone.stdout)
    only = _run(RI, TAGS, READS, MIN_LEN, 1, "--verify-max", 16, "--verify-mismatch", 1, "--align", out, "--align-band", 2)  # the verify options without --verify
    assert only.returncode == 0 and open(out, "rb").read() == text
    zero = _run(RI, TAGS, READS, MIN_LEN, 1, "--align", out, "--align-band", 0)
    assert zero.returncode == 0 and open(out, "rb").read() == _expected_text(0)[0]
    for bad in ("32", "-1", "x", ""):
        r = _run(RI, TAGS, READS, MIN_LEN, 1, "--align", out, "--align-band", bad)
        assert r.returncode == 1 and "usage:" in r.stderr and r.stdout == "", (bad, r.stderr)
    r = _run(RI, TAGS, READS, MIN_LEN, 1, "--align-band", 4)  # without --align
    assert r.returncode == 1 and "usage:" in r.stderr


def test_align_only_leaves_stdout_empty(built, xy_expected, tmp_path):
    for extra in ([], ["--batch", "7", "--streams", "2"], ["--format", "device"]):
        out = str(tmp_path / "only.tsv")
        r = _run(RI, TAGS, READS, MIN_LEN, 1, "--align", out, "--align-only", *extra)
        assert r.returncode == 0, r.stderr
        assert r.stdout == "" and "[find_all_mems]" not in r.stderr
        assert open(out, "rb").read() == xy_expected[0]


def test_align_only_does_not_go_with_locate(built, tmp_path):
    out = str(tmp_path / "refused.tsv")
    r = _run(RI, TAGS, READS, MIN_LEN, 1, "--align", out, "--align-only", "--locate", "positions")
    assert r.returncode == 1 and r.stdout == "" and "--align-only" in r.stderr and not os.path.exists(out)
    r = _run(RI, TAGS, READS, MIN_LEN, 1, "--align-only")
    assert r.returncode == 1


def test_an_image_without_locate_is_refused(built, tmp_path):
    img = str(tmp_path / "xy_nolocate.pgi")
    tool = os.path.join(ROOT, "pangenome-index_amd", "pgx_image")
    made = subprocess.run([tool, RI, TAGS, img, "--no-locate"], capture_output=True, text=True, timeout=300)
    assert made.returncode == 0, made.stderr
    out = str(tmp_path / "refused.tsv")
    r = _run(img, "-", READS, MIN_LEN, 1, "--align", out)
    assert r.returncode == 1 and r.stdout == "", r.stderr
    assert "locate" in r.stderr and not os.path.exists(out)
