"""GPU tier: `find_mems --place FILE` writes one line per read with the record tests/place_emu.py derives from the MEMs of the run and from
the packed positions of pgx_locate_batch, and leaves stdout and stderr byte for byte what they are without it -- with small batches and
several workers, --locate, --format device, --result compact, device-parsed reads and --hits next to it; --place-only leaves stdout
empty; --place-max caps the located MEMs."""
import os
import subprocess

import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import place_emu as E
from cli_format import strip_timing
from test_gpu_mem_locate import _ranges

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


def _expected_text(ri, tags, reads_path, min_len, max_occ=0):
    """the place file of a run in the CLI's default mode: MEMs of a batch run, values from pgx_locate_batch, records from the emulator"""
    cat, offs = O.pack_reads([l for l in open(reads_path, "rb").read().split(b"\n") if l])
    idx = P.Index(ri, tags)
    res = idx.find_mems(cat, offs, min_len, 1)
    info = idx.info()
    first, last, _ = _ranges(res["mems"], info.bwt_size, max_occ)
    off, vals = idx.locate_batch(first, last, 0)
    L = int(info.max_length)
    idx.close()
    exp = E.read_place(res["mem_offsets"], res["mems"], off, vals, L)
    return E.place_text(exp["reads"]), exp["reads"]


@pytest.fixture(scope="module")
def xy_expected(built):
    return _expected_text(RI, TAGS, READS, MIN_LEN)


@pytest.mark.parametrize("extra", [[], ["--batch", "7", "--streams", "2"], ["--locate", "seqs"], ["--locate", "positions", "--locate-max", "3"], ["--format", "device"],
                                   ["--result", "compact"], ["--format", "device", "--locate", "seqs", "--batch", "5"], ["--device-parse", "--batch", "7"], ["--quiet"]])
def test_place_file_and_unchanged_output(built, xy_expected, tmp_path, extra):
    out = str(tmp_path / "place.tsv")
    plain = _run(RI, TAGS, READS, MIN_LEN, 1, *extra)
    placed = _run(RI, TAGS, READS, MIN_LEN, 1, *extra, "--place", out)
    assert plain.returncode == 0 and placed.returncode == 0, placed.stderr
    assert strip_timing(placed.stdout) == strip_timing(plain.stdout) and len(plain.stdout) > 1000
    assert _stderr(placed.stderr) == _stderr(plain.stderr)
    text, recs = xy_expected
    assert open(out, "rb").read() == text
    assert (recs["best_score"] > 0).any() and text.count(b"\n") == len(recs) + 1


def test_place_next_to_hits(built, xy_expected, tmp_path):
    out, hits, hits_alone = str(tmp_path / "place.tsv"), str(tmp_path / "hits.tsv"), str(tmp_path / "hits_alone.tsv")
    alone = _run(RI, TAGS, READS, MIN_LEN, 1, "--hits", hits_alone, "--batch", "7")
    both = _run(RI, TAGS, READS, MIN_LEN, 1, "--hits", hits, "--place", out, "--batch", "7")
    assert alone.returncode == 0 and both.returncode == 0, both.stderr
    assert open(out, "rb").read() == xy_expected[0] and open(hits, "rb").read() == open(hits_alone, "rb").read()
    assert strip_timing(both.stdout) == strip_timing(alone.stdout)


def test_place_only_leaves_stdout_empty(built, xy_expected, tmp_path):
    for extra in ([], ["--batch", "7", "--streams", "2"], ["--format", "device", "--result", "compact"]):
        out = str(tmp_path / "only.tsv")
        r = _run(RI, TAGS, READS, MIN_LEN, 1, "--place", out, "--place-only", *extra)
        assert r.returncode == 0, r.stderr
        assert r.stdout == "" and "[find_all_mems]" not in r.stderr
        assert open(out, "rb").read() == xy_expected[0]
    # the text is suppressed when either of the two is given
    out, hits = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")
    r = _run(RI, TAGS, READS, MIN_LEN, 1, "--place", out, "--hits", hits, "--hits-only")
    assert r.returncode == 0 and r.stdout == "" and open(out, "rb").read() == xy_expected[0]


def test_place_max(built, xy_expected, tmp_path):
    cat, offs = O.pack_reads([l for l in open(READS, "rb").read().split(b"\n") if l])
    idx = P.Index(RI, TAGS)
    sizes = np.unique(idx.find_mems(cat, offs, MIN_LEN, 1)["mems"]["size"].astype(np.int64))
    idx.close()
    sizes = sizes[sizes > 0]
    assert len(sizes) >= 2
    cap = int(sizes[(len(sizes) - 1) // 2])
    text, recs = _expected_text(RI, TAGS, READS, MIN_LEN, max_occ=cap)
    assert (recs["n_located"] < xy_expected[1]["n_located"]).any() and text != xy_expected[0]
    out = str(tmp_path / "max.tsv")
    r = _run(RI, TAGS, READS, MIN_LEN, 1, "--place", out, "--place-max", cap)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == text
    r = _run(RI, TAGS, READS, MIN_LEN, 1, "--place", out, "--place-max", "x")
    assert r.returncode == 1 and "--place-max" in r.stderr


def test_an_image_without_locate_is_refused(built, tmp_path):
    img = str(tmp_path / "xy_nolocate.pgi")
    tool = os.path.join(ROOT, "pangenome-index_amd", "pgx_image")
    made = subprocess.run([tool, RI, TAGS, img, "--no-locate"], capture_output=True, text=True, timeout=300)
    assert made.returncode == 0, made.stderr
    out = str(tmp_path / "refused.tsv")
    for extra in ([], ["--place-only"]):
        r = _run(img, "-", READS, MIN_LEN, 1, "--place", out, *extra)
        assert r.returncode == 1 and r.stdout == "", r.stderr
        assert "locate" in r.stderr and not os.path.exists(out)
    assert _run(img, "-", READS, MIN_LEN, 1).returncode == 0  # the image itself is fine
