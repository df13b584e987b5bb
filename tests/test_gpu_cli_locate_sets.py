"""GPU tier: `find_mems --locate seqs` is served from the sequence sets by default and prints the same bytes as with the segmented sort
(PGX_LOCATE_SETS=0): on the xy fixture, where both equal the lines tests/locate_format.py renders from the oracle's suffix array, and on a
collection of 66 sequences (two set words a MEM)."""
import os
import subprocess

import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
from cli_format import strip_timing
from locate_format import mem_locate_lines, splice

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")
BT = os.path.join(O.GOLDEN, "bidirectional_test")
RI, TAGS = os.path.join(BT, "xy.ri"), os.path.join(BT, "xy_bidirectional_compressed.tags")


def _run(args, sets):
    env = dict(os.environ)
    env.pop("PGX_LOCATE_SETS", None)
    if not sets:
        env["PGX_LOCATE_SETS"] = "0"
    r = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    return strip_timing(r.stdout)


def test_cli_seqs_on_xy_equals_oracle_both_ways(built):
    reads = os.path.join(BT, "reads.txt")
    by_sets, by_sort = _run([RI, TAGS, reads, 5, 1, "--locate", "seqs"], True), _run([RI, TAGS, reads, 5, 1, "--locate", "seqs"], False)
    assert by_sets == by_sort
    # the oracle: its MEMs, and the distinct sequences of its suffix-array rows
    ori = O.RIndex(RI)
    found = [m for l in open(reads, "rb").read().split(b"\n") if l for m in ori.find_all_mems(l, 5, 1)]
    mems = np.zeros(len(found), P.MEM_DTYPE)
    for f in ("start", "end", "bwt_start", "size"):
        mems[f] = [m[("start", "end", "bwt_start", "size").index(f)] for m in found]
    da = ori.decompress_da()
    per = [np.unique(da[int(m["bwt_start"]):int(m["bwt_start"]) + int(m["size"])]) for m in mems]
    off = np.concatenate(([0], np.cumsum([len(p) for p in per]))).astype(np.uint64)
    vals = np.concatenate(per).astype(np.uint64) if per else np.zeros(0, np.uint64)
    golden = open(os.path.join(O.GOLDEN, "expected_find_mems_xy_reads_5_1.txt")).read()
    exp = splice(golden, mem_locate_lines(mems, off, vals, "seqs", ori.max_length))
    assert exp != golden and by_sets == exp


def test_cli_seqs_on_66_sequences(built, workdir):
    text = os.path.join(workdir, "cli_sets_66.txt")
    assert W.synth_pangenome_text(text, base_len=2000, n_hap=33, seed=133, n_runs=1, n_run_len=(10, 40)) == 66
    ri, tags = W.build_index_from_text(text, workdir, "cli_sets_66")[:2]
    cat, offs = W.sample_reads(W.load_sequences(text), 200, 150, seed=33)
    reads = os.path.join(workdir, "cli_sets_66_reads.txt")
    with open(reads, "wb") as f:
        for r in range(len(offs) - 1):
            f.write(bytes(cat[int(offs[r]):int(offs[r + 1])]) + b"\n")
    args = [ri, tags, reads, 12, 1, "--locate", "seqs"]
    by_sets, by_sort = _run(args, True), _run(args, False)
    assert by_sets == by_sort
    # ids of both set words are printed, as pgx_locate_batch gives them
    idx = P.Index(ri, tags)
    mems = idx.find_mems(cat, offs, 12, 1)["mems"]
    size = mems["size"].astype(np.int64)
    off, vals = idx.locate_batch(mems["bwt_start"].astype(np.uint64), (mems["bwt_start"].astype(np.int64) + size - 1).astype(np.uint64),
                                 P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE)
    assert len(vals) and int(vals.max()) >= 64
    lines = mem_locate_lines(mems, off, vals, "seqs", idx.info().max_length)
    idx.close()
    pos = 0
    for ln in lines:  # in MEM order
        pos = by_sets.find(ln, pos)
        assert pos >= 0, ln
        pos += len(ln)
