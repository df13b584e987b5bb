"""GPU tier: `find_mems --hits FILE` writes one line per read with the record tests/hits_emu.py derives from the MEMs of the run and from
sequence sets built with pgx_locate_batch, and leaves stdout and stderr byte for byte what they are without it -- with small batches and
several workers, --locate, --format device, --result compact and device-parsed reads; --hits-only leaves stdout empty; --hits-max caps
the located MEMs; an index of more than 4096 sequences is refused before anything is written."""
import os
import subprocess

import numpy as np
import pytest

import hits_emu as E
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
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
    """the hits file of a run in the CLI's default mode: MEMs of a batch run, sets from pgx_locate_batch, records from the emulator"""
    cat, offs = O.pack_reads([l for l in open(reads_path, "rb").read().split(b"\n") if l])
    idx = P.Index(ri, tags)
    res = idx.find_mems(cat, offs, min_len, 1)
    info = idx.info()
    first, last, _ = _ranges(res["mems"], info.bwt_size, max_occ)
    off, vals = idx.locate_batch(first, last, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE)
    n_seq = int(info.n_sequences)
    idx.close()
    exp = E.read_hits(res["mem_offsets"], res["mems"], E.sets_from_ids(off, vals, len(res["mems"]), n_seq), n_seq)
    return E.hits_text(exp["hits"]), exp["hits"]


@pytest.fixture(scope="module")
def xy_expected(built):
    return _expected_text(RI, TAGS, READS, MIN_LEN)


@pytest.mark.parametrize("extra", [[], ["--batch", "7", "--streams", "2"], ["--locate", "seqs"], ["--locate", "positions", "--locate-max", "3"], ["--format", "device"],
                                   ["--result", "compact"], ["--format", "device", "--locate", "seqs", "--batch", "5"], ["--device-parse", "--batch", "7"], ["--quiet"]])
def test_hits_file_and_unchanged_output(built, xy_expected, tmp_path, extra):
    out = str(tmp_path / "hits.tsv")
    plain = _run(RI, TAGS, READS, MIN_LEN, 1, *extra)
    hits = _run(RI, TAGS, READS, MIN_LEN, 1, *extra, "--hits", out)
    assert plain.returncode == 0 and hits.returncode == 0, hits.stderr
    assert strip_timing(hits.stdout) == strip_timing(plain.stdout) and len(plain.stdout) > 1000
    assert _stderr(hits.stderr) == _stderr(plain.stderr)
    text, recs = xy_expected
    assert open(out, "rb").read() == text
    assert (recs["best_score"] > 0).any() and text.count(b"\n") == len(recs) + 1


def test_hits_only_leaves_stdout_empty(built, xy_expected, tmp_path):
    for extra in ([], ["--batch", "7", "--streams", "2"], ["--format", "device", "--result", "compact"]):
        out = str(tmp_path / "only.tsv")
        r = _run(RI, TAGS, READS, MIN_LEN, 1, "--hits", out, "--hits-only", *extra)
        assert r.returncode == 0, r.stderr
        assert r.stdout == "" and "[find_all_mems]" not in r.stderr
        assert open(out, "rb").read() == xy_expected[0]


def test_hits_max(built, xy_expected, tmp_path):
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
    r = _run(RI, TAGS, READS, MIN_LEN, 1, "--hits", out, "--hits-max", cap)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == text
    r = _run(RI, TAGS, READS, MIN_LEN, 1, "--hits", out, "--hits-max", "x")
    assert r.returncode == 1 and "--hits-max" in r.stderr


def test_more_than_4096_sequences_is_refused(built, workdir, tmp_path):
    text = os.path.join(workdir, "cli_hits_4098.txt")
    assert W.synth_pangenome_text(text, base_len=100, n_hap=2049, seed=12, n_runs=1, n_run_len=(10, 40)) == 4098
    ri, tags = W.build_index_from_text(text, workdir, "cli_hits_4098")[:2]
    cat, offs = W.sample_reads(W.load_sequences(text), 20, 60, seed=9)
    reads = os.path.join(workdir, "cli_hits_4098_reads.txt")
    with open(reads, "wb") as f:
        for r in range(len(offs) - 1):
            f.write(bytes(cat[int(offs[r]):int(offs[r + 1])]) + b"\n")
    out = str(tmp_path / "refused.tsv")
    for extra in ([], ["--hits-only"]):
        r = _run(ri, tags, reads, 12, 1, "--hits", out, *extra)
        assert r.returncode == 1 and r.stdout == "", r.stderr
        assert "4096 sequences" in r.stderr and "4098" in r.stderr
        assert not os.path.exists(out) or os.path.getsize(out) == 0
    assert _run(ri, tags, reads, 12, 1).returncode == 0  # the index itself is fine
