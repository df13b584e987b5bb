"""GPU tier: `find_mems --mapq`.  With --gaf FILE, column 12 of every line whose read has steps is the mapq of the record Batch.read_mapq gives
(checked against the emulator in tests/test_gpu_mapq.py), a read without steps keeps 255, and every other column, stdout and stderr are what the
run without --mapq writes at the same --verify-max; --mapq-file FILE holds the records by its header row, whatever the batches; --mapq-scale,
--mapq-slack and --mapq-extra reach the stage; --paired --rescue --mapq runs the stage behind the election with the paired scores; --mapq without
--gaf or --mapq-file, and the mapq options without --mapq, are usage errors; a tags argument of - on a .ri ends the run before any batch."""
import os
import subprocess

import pytest

import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import rescue_cases as RC
from cli_format import strip_timing

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")
BT = os.path.join(O.GOLDEN, "bidirectional_test")
RI, TAGS, READS = os.path.join(BT, "xy.ri"), os.path.join(BT, "xy_bidirectional_compressed.tags"), os.path.join(BT, "reads.txt")
MIN_LEN = 3
HEADER = "#read\tmapq\tentries\tloci\twith\tcompeting\tbest_other\texcess\tflags\n"


def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def _stderr(text):
    return "\n".join(l for l in text.split("\n") if " took " not in l)


def mapq_text(recs):
    """the --mapq-file of these records, by the header row"""
    return HEADER + "".join("\t".join(str(c) for c in [k + 1] + [int(x[f]) for f in ("mapq", "n_entries", "n_loci", "n_with", "n_competing", "best_other", "excess", "flags")]) + "\n"
                            for k, x in enumerate(recs))


@pytest.fixture(scope="module")
def xy_records(built):
    """the records of the golden reads in the CLI's default mode, at the defaults of --mapq and at other knobs"""
    reads = [l for l in open(READS, "rb").read().split(b"\n") if l]
    cat, offs = O.pack_reads(reads)
    idx = P.Index(RI, TAGS)
    b = P.Batch(idx, cat, offs)
    b.run(MIN_LEN, 1, 0)
    b.locate(0)
    b.read_place(P.PLACE_LIST)
    b.read_verify(16, 4, P.VERIFY_LIST)
    out = dict(default=b.read_mapq(2, 8, 16)["records"], other=b.read_mapq(5, 0, 3)["records"])
    b.free()
    idx.close()
    return out


@pytest.mark.parametrize("extra", [[], ["--batch", "7", "--streams", "2"], ["--format", "device", "--locate", "positions", "--batch", "5"], ["--device-parse", "--batch", "7"]])
def test_column_12_is_the_record_and_everything_else_stays(xy_records, tmp_path, extra):
    gaf0, gaf, tsv = (str(tmp_path / n) for n in ("plain.gaf", "mapq.gaf", "mapq.tsv"))
    plain = _run(RI, TAGS, READS, MIN_LEN, 1, "--gaf", gaf0, "--verify-max", 16, *extra)
    with_q = _run(RI, TAGS, READS, MIN_LEN, 1, "--gaf", gaf, "--mapq", "--mapq-file", tsv, *extra)
    assert plain.returncode == 0 and with_q.returncode == 0, with_q.stderr
    assert strip_timing(with_q.stdout) == strip_timing(plain.stdout) and len(plain.stdout) > 1000 and _stderr(with_q.stderr) == _stderr(plain.stderr)
    recs = xy_records["default"]
    a, b = open(gaf0).read().split("\n"), open(gaf).read().split("\n")
    assert len(a) == len(b) == len(recs) + 1
    stepless = 0
    for k, (x, y) in enumerate(zip(a[:-1], b[:-1])):
        cx, cy = x.split("\t"), y.split("\t")
        assert cx[:11] == cy[:11] and cx[12:] == cy[12:] and cx[11] == "255", k
        if cx[5] == "*":
            stepless += 1
            assert cy[11] == "255", k
        else:
            assert cy[11] == str(int(recs[k]["mapq"])), k
    assert open(tsv).read() == mapq_text(recs)
    assert stepless < len(recs)


def test_the_knobs_reach_the_stage_and_the_file_needs_no_gaf(xy_records, tmp_path):
    tsv = str(tmp_path / "other.tsv")
    r = _run(RI, TAGS, READS, MIN_LEN, 1, "--mapq", "--mapq-file", tsv, "--mapq-scale", 5, "--mapq-slack", 0, "--mapq-extra", 3, "--batch", 6)
    assert r.returncode == 0, r.stderr
    assert open(tsv).read() == mapq_text(xy_records["other"]) != mapq_text(xy_records["default"])


def test_paired_rescue_mapq_runs_behind_the_election(built, workdir, tmp_path):
    C = RC.CASES
    text = os.path.join(workdir, "cli_mapq_rescue_cases.txt")
    with open(text, "wb") as f:
        f.write(C.raw)
    ri, tags = W.build_index_from_text(text, workdir, "cli_mapq_rescue_cases")[:2]
    reads = os.path.join(workdir, "cli_mapq_rescue_reads.txt")
    with open(reads, "wb") as f:
        f.write(b"".join(r + b"\n" for r in C.reads))
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    cat, offs = O.pack_reads(C.reads)
    b = P.Batch(idx, cat, offs)
    b.run(RC.MIN_LEN, 1, 0)
    b.locate(0)
    b.read_place(P.PLACE_LIST)
    b.read_verify(16, 4, P.VERIFY_LIST)
    b.read_rescue(RC.FRAG_MIN, RC.FRAG_MAX, RC.MIN_LEN, 2, P.RESCUE_MERGE)
    b.read_mates(RC.FRAG_MIN, RC.FRAG_MAX, 10, P.MATES_ELECT)
    want = b.read_mapq(2, 8, 16, P.MAPQ_PAIRED)
    b.free()
    idx.close()
    assert (want["records"]["flags"] & P.MAPQ_RESCUED).any() and (want["records"]["flags"] & P.MAPQ_PAIRED).any()
    opts = ["--mode", "strict", "--paired", "--frag-max", RC.FRAG_MAX, "--rescue"]
    gaf0, gaf, tsv = (str(tmp_path / n) for n in ("p.gaf", "q.gaf", "q.tsv"))
    plain = _run(ri, tags, reads, RC.MIN_LEN, 1, *opts, "--gaf", gaf0)
    for extra in ([], ["--batch", 6, "--streams", 2]):
        r = _run(ri, tags, reads, RC.MIN_LEN, 1, *opts, "--gaf", gaf, "--mapq", "--mapq-file", tsv, *extra)
        assert plain.returncode == 0 and r.returncode == 0, r.stderr
        assert open(tsv).read() == mapq_text(want["records"])
        assert strip_timing(r.stdout) == strip_timing(plain.stdout) and _stderr(r.stderr) == _stderr(plain.stderr)
        for k, (x, y) in enumerate(zip(open(gaf0).read().split("\n")[:-1], open(gaf).read().split("\n")[:-1])):
            cx, cy = x.split("\t"), y.split("\t")
            assert cx[:11] == cy[:11] and cx[12:] == cy[12:] and cy[11] == ("255" if cx[5] == "*" else str(int(want["records"][k]["mapq"]))), k


def test_usage_errors_and_an_index_without_tags(built, tmp_path):
    out = str(tmp_path / "refused.tsv")
    for args in (["--mapq"], ["--mapq-file", out], ["--gaf", out, "--mapq-scale", 3], ["--gaf", out, "--mapq-slack", 3], ["--gaf", out, "--mapq-extra", 3]):
        r = _run(RI, TAGS, READS, MIN_LEN, 1, *args)
        assert r.returncode == 1 and r.stdout == "" and "--mapq" in r.stderr and not os.path.exists(out), args
    for name, bad, text in (("--mapq-scale", 0, "1 .. 16"), ("--mapq-scale", 17, "1 .. 16"), ("--mapq-slack", 1025, "0 .. 1024"), ("--mapq-extra", 64, "0 .. 63"), ("--mapq-extra", "x", "0 .. 63")):
        r = _run(RI, TAGS, READS, MIN_LEN, 1, "--mapq", "--mapq-file", out, name, bad)
        assert r.returncode == 1 and r.stdout == "" and name + ": a number in " + text in r.stderr and not os.path.exists(out), (name, bad)
    r = _run(RI, "-", READS, MIN_LEN, 1, "--mapq", "--mapq-file", out)
    assert r.returncode == 1 and r.stdout == "", r.stderr
    assert "without a tag array" in r.stderr and "--mapq" in r.stderr and not os.path.exists(out)
