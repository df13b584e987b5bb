"""GPU tier: `find_mems --paired --rescue`.  On the pairs of tests/rescue_cases.py, through an index built from the table's collection:

  --rescued FILE  its lines equal the records of Batch.read_rescue (checked against the emulator in tests/test_gpu_rescue.py), written out here by
                  the format the header row states; the file is the same under --batch 2, 6 and 7 and with --device-parse, and for the same reads
                  given as lines, FASTA and FASTQ; --rescue-min and --rescue-anchors reach the stage
  other outputs   stdout and stderr are what they are without --rescue; --verify, --mates and --gaf show the rescued reads: every planted mate lies
                  on its truth in a proper pair with --rescue and is unplaced without it
  replay          --paired --rescue --gaf on the walk graph of tests/replay_cases.py, on pairs cut here with one mate made dense: the line of every
                  rescued read replays through tests/gaf_replay.py
  refusals        the rescue options without --paired, and --rescue-min / --rescue-anchors / --rescued without --rescue, are usage errors"""
import os
import subprocess

import numpy as np
import pytest

import gaf_replay as G
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import replay_cases as RP
import rescue_cases as RC
from cli_format import strip_timing
from test_gpu_gaf_replay import world  # noqa: F401  (the walk graph's index, a module fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")
C = RC.CASES
READS = C.reads
PLANTED = [k for k, p in enumerate(C.pairs) if p["kind"] in ("dense", "dense_both_strands", "repeat_anchor", "edge")]
HEADER = "#read\ttarget\tanchors\tdiags\tseq\tpos\tseg_score\tmatches\tn_best\tnext\trescued\n"
OPTS = ["--mode", "strict", "--paired", "--frag-max", RC.FRAG_MAX]


def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def _stderr(text):
    return "\n".join(l for l in text.split("\n") if " took " not in l)


def rescued_text(recs):
    """the --rescued file of these records, by the header row"""
    lines = [HEADER]
    for k, x in enumerate(recs):
        fl, none = int(x["flags"]), int(x["seq"]) == 0xFFFFFFFF
        cols = [k + 1, int(bool(fl & P.RESCUE_TARGET)), int(x["n_anchors"]), int(x["n_diags"]), "*" if none else int(x["seq"]), "*" if none else int(x["diag"]),
                int(x["seg_score"]), int(x["matches"]), int(x["n_best"]), int(x["next_score"]), int(bool(fl & P.RESCUE_RESCUED))]
        lines.append("\t".join(str(c) for c in cols) + "\n")
    return "".join(lines)


@pytest.fixture(scope="module")
def files(workdir, built):
    """the index of the table's collection; the reads as lines, FASTA and FASTQ; the expected --rescued texts from the bindings"""
    text = os.path.join(workdir, "cli_rescue_cases.txt")
    with open(text, "wb") as f:
        f.write(C.raw)
    ri, tags = W.build_index_from_text(text, workdir, "cli_rescue_cases")[:2]
    paths = {fmt: os.path.join(workdir, "cli_rescue_reads." + fmt) for fmt in ("lines", "fasta", "fastq")}
    with open(paths["lines"], "wb") as f:
        f.write(b"".join(r + b"\n" for r in READS))
    with open(paths["fasta"], "wb") as f:
        f.write(b"".join(b">r%d\n" % i + r[:30] + b"\n" + r[30:] + b"\n" for i, r in enumerate(READS)))  # (two lines a sequence)
    with open(paths["fastq"], "wb") as f:
        f.write(b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(READS)))
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    cat, offs = O.pack_reads(READS)
    b = P.Batch(idx, cat, offs)
    b.run(RC.MIN_LEN, 1, 0)
    b.locate(0)
    b.read_place(P.PLACE_LIST)
    want = {}
    for key, (min_score, anchors) in dict(default=(RC.MIN_LEN, 2), other=(13, 1)).items():
        b.read_verify(16, 4, P.VERIFY_LIST)  # (what --paired takes; a verify result takes one merge)
        res = b.read_rescue(RC.FRAG_MIN, RC.FRAG_MAX, min_score, anchors, P.RESCUE_MERGE)
        want[key] = rescued_text(res["reads"])
        if key == "default":
            assert (res["n_targets"], res["n_rescued"]) == (94, 59)
        else:
            assert (res["n_targets"], res["n_rescued"]) == (94, 44)  # without the ten behind a second anchor and the five at exactly 12
    b.free()
    idx.close()
    return ri, tags, paths, want


@pytest.mark.parametrize("fmt,extra", [("lines", []), ("lines", ["--batch", 2]), ("lines", ["--batch", 6, "--streams", 2]), ("lines", ["--batch", 7, "--device-parse"]),
                                       ("fasta", ["--batch", 7, "--reads-format", "fasta"]), ("fastq", ["--batch", 2, "--reads-format", "fastq"])])
def test_the_rescued_file_equals_the_bindings_whatever_the_ranges(files, tmp_path, fmt, extra):
    ri, tags, paths, want = files
    out, pairs = str(tmp_path / "rescued.tsv"), str(tmp_path / "pairs.tsv")
    r = _run(ri, tags, paths[fmt], RC.MIN_LEN, 1, *OPTS, "--rescue", "--rescued", out, "--mates", pairs, "--mates-only", *extra)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    got = open(out).read()
    assert got.count("\n") == len(READS) + 1 and got == want["default"]
    if not extra:
        r = _run(ri, tags, paths[fmt], RC.MIN_LEN, 1, *OPTS, "--rescue", "--rescue-min", 13, "--rescue-anchors", 1, "--rescued", out, "--mates", pairs, "--mates-only")
        assert r.returncode == 0 and open(out).read() == want["other"] != want["default"], r.stderr


def test_stdout_and_stderr_stay_and_the_other_files_show_the_rescued_reads(files, tmp_path):
    ri, tags, paths, want = files
    out, ver, gaf, mat, ver0, gaf0, mat0 = (str(tmp_path / n) for n in ("rescued.tsv", "r.verify", "r.gaf", "r.mates", "p.verify", "p.gaf", "p.mates"))
    for extra in ([], ["--batch", 6, "--streams", 2], ["--format", "device", "--batch", 7]):
        plain = _run(ri, tags, paths["lines"], RC.MIN_LEN, 1, *OPTS, "--verify", ver0, "--gaf", gaf0, "--mates", mat0, *extra)
        resc = _run(ri, tags, paths["lines"], RC.MIN_LEN, 1, *OPTS, "--rescue", "--rescued", out, "--verify", ver, "--gaf", gaf, "--mates", mat, *extra)
        assert plain.returncode == 0 and resc.returncode == 0, resc.stderr
        assert strip_timing(resc.stdout) == strip_timing(plain.stdout) and len(plain.stdout) > 1000
        assert _stderr(resc.stderr) == _stderr(plain.stderr)
        assert open(out).read() == want["default"]

    def placed(verify_path, gaf_path, mates_path):
        """(seq, pos) of every read by the verify file, whether its GAF line names a path, and `proper` of every pair by the mates file"""
        v = [l.split("\t") for l in open(verify_path).read().split("\n")[1:-1]]
        g = [l.split("\t")[5] != "*" for l in open(gaf_path).read().split("\n")[:-1]]
        m = [l.split("\t")[3] == "1" for l in open(mates_path).read().split("\n")[1:-1]]
        return [None if x[1] == "*" else (int(x[1]), int(x[2])) for x in v], g, m

    rv, rg, rm = placed(ver, gaf, mat)
    pv, pg, pm = placed(ver0, gaf0, mat0)
    assert len(rv) == len(rg) == len(READS) and len(rm) == len(C.pairs) and len(PLANTED) == 44
    for k in PLANTED:
        p = C.pairs[k]
        r, truth = (2 * k, p["truth_a"]) if p["mate"] == "a" else (2 * k + 1, p["truth_b"])
        assert rv[r] == truth and pv[r] is None and rm[k] and not pm[k], (k, p["kind"])
        other = p["truth_b"] if p["mate"] == "a" else p["truth_a"]
        # (the placed mate of a `repeat_anchor` pair ties between the copies: the rescued mate settles it, verify alone names the first copy)
        assert rv[r ^ 1] == other and (pv[r ^ 1] == other) == (p["kind"] != "repeat_anchor"), (k, p["kind"])
        assert not pg[r]
    for k, p in enumerate(C.pairs):
        if p["kind"] == "junk":
            assert rv[2 * k + 1] is None and pv[2 * k + 1] is None and not rm[k]
        if p["kind"] in ("proper", "both"):
            assert rv[2 * k:2 * k + 2] == pv[2 * k:2 * k + 2] == [p["truth_a"], p["truth_b"]] and rm[k] == pm[k] == (p["kind"] == "proper")
    assert sum(rm) == sum(pm) + 59


def test_the_gaf_line_of_every_rescued_read_replays_on_the_walk_graph(world, tmp_path):  # noqa: F811
    ri, tags, texts = world
    K = RP.CASES
    rng = np.random.default_rng(707)
    assert len(texts) % 2 == 0 and all(len(texts[q]) == len(texts[q + 1]) for q in range(0, len(texts), 2))
    reads = []
    for k in range(40):  # a fragment of 200 .. 400 of a forward haplotype: A its first 60 bases, B the reverse complement of its last 60 with every tenth base replaced
        q = 2 * int(rng.integers(0, len(texts) // 2))
        n = int(rng.integers(200, 401))
        f = int(rng.integers(0, len(texts[q]) - n + 1))
        b = bytearray(RC.rc(texts[q][f + n - 60:f + n]))
        for i in range(int(rng.integers(4, 10)), 60, 10):
            b[i] = b"ACGT"[(b"ACGT".index(b[i]) + 1) % 4]
        reads += [texts[q][f:f + 60], bytes(b)]
    path, gaf, out = str(tmp_path / "rescue_pairs.txt"), str(tmp_path / "rescue_pairs.gaf"), str(tmp_path / "rescue_pairs.tsv")
    with open(path, "wb") as f:
        f.write(b"".join(r + b"\n" for r in reads))
    r = _run(ri, tags, path, RP.MIN_LEN, 1, "--mode", "strict", "--paired", "--frag-max", 500, "--rescue", "--rescued", out, "--align-band", 8, "--gaf", gaf, "--gaf-only")
    assert r.returncode == 0, r.stderr
    lines = open(gaf).read().split("\n")[:-1]
    recs = [l.split("\t") for l in open(out).read().split("\n")[1:-1]]
    assert len(lines) == len(recs) == len(reads)
    rescued = [i for i, x in enumerate(recs) if x[10] == "1"]
    assert len(rescued) >= 30 and all(i % 2 == 1 for i in rescued)
    for i in rescued:
        assert G.replay_gaf_line(lines[i], reads[i], K.node_seq, texts=texts, number=i + 1) is not None, i


def test_usage_errors(files, tmp_path):
    ri, tags, paths, _ = files
    out = str(tmp_path / "refused.tsv")
    for args in (["--rescue"], ["--rescue", "--rescued", out], ["--rescued", out], ["--rescue-min", 12], ["--rescue-anchors", 2],  # without --paired
                 ["--paired", "--rescued", out], ["--paired", "--rescue-min", 12], ["--paired", "--rescue-anchors", 2]):        # without --rescue
        r = _run(ri, tags, paths["lines"], RC.MIN_LEN, 1, "--mode", "strict", *args)
        assert r.returncode == 1 and r.stdout == "" and "usage:" in r.stderr, args
    for args, text in ((["--rescue-anchors", 9], "--rescue-anchors: a number in 1 .. 8"), (["--rescue-anchors", 0], "--rescue-anchors: a number in 1 .. 8"),
                       (["--rescue-min", 0], "--rescue-min: a number in 1 .. 4294967295"), (["--frag-max", 70000], "window of more than 65536")):
        r = _run(ri, tags, paths["lines"], RC.MIN_LEN, 1, "--mode", "strict", "--paired", "--rescue", *args)
        assert r.returncode == 1 and r.stdout == "" and text in r.stderr, args
    assert not os.path.exists(out)
