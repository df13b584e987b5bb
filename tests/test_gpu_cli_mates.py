"""GPU tier: `find_mems --paired`.  On the pairs of tests/mates_cases.py that a line file can hold (every pair but the four whose B is the empty
read), through an index built from the table's collection:

  --mates FILE    its lines equal the records of Batch.read_mates (checked against the emulator in tests/test_gpu_mates.py), written out here by the
                  format the header row states; the file is the same under --batch 2, 6 and 7 and with --device-parse, and for the same reads given
                  as lines, FASTA and FASTQ: the ranges hold whole pairs, or a pair cut in two would pair its halves with their neighbours
  other outputs   stdout and stderr are what they are without --paired; --verify and --gaf report the elected winners: the reads in the second copy
                  of a repeat lie on their truth with --paired and on the first copy without it
  replay          --paired --gaf on the walk graph of tests/replay_cases.py: every line replays through tests/gaf_replay.py
  refusals        an odd record count ends the run with status 1; --mates-only does not go with --locate; --mates without --paired is a usage error"""
import os
import subprocess

import pytest

import gaf_replay as G
import mates_cases as MC
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import replay_cases as RC
from cli_format import strip_timing
from test_gpu_gaf_replay import world  # noqa: F401  (the walk graph's index, a module fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")
C = MC.CASES
PAIRS = [k for k, p in enumerate(C.pairs) if p["a"] and p["b"]]
READS = [r for k in PAIRS for r in (C.pairs[k]["a"], C.pairs[k]["b"])]
TRUTHS = [t for k in PAIRS for t in (C.pairs[k]["truth_a"], C.pairs[k]["truth_b"])]
SECOND = [2 * i + (0 if C.pairs[k]["mate"] == "a" else 1) for i, k in enumerate(PAIRS) if C.pairs[k]["which"] == 1]  # reads in the second copy
HEADER = "#pair\tread_a\tread_b\tproper\tfrag\tpair_score\tsolo_score\tcand_a\tcand_b\tseq_a\tseq_b\tn_compatible\tn_best\tnext\tmoved_a\tmoved_b\n"
OPTS = ["--mode", "strict", "--paired", "--frag-max", MC.FRAG_MAX]


def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def _stderr(text):
    return "\n".join(l for l in text.split("\n") if " took " not in l)


def mates_text(pairs):
    """the --mates file of these records, by the header row"""
    lines = [HEADER]
    for k, x in enumerate(pairs):
        fl = int(x["flags"])
        star = lambda q: "*" if int(q) == 0xFFFFFFFF else str(int(q))
        cols = [k + 1, 2 * k + 1, 2 * k + 2, int(bool(fl & P.MATES_PROPER)), int(x["frag"]) if fl & P.MATES_COMPATIBLE else "*", int(x["pair_score"]), int(x["solo_score"]),
                int(x["cand_a"]), int(x["cand_b"]), star(x["seq_a"]), star(x["seq_b"]), int(x["n_compatible"]), int(x["n_best"]), int(x["next_score"]),
                int(bool(fl & P.MATES_MOVED_A)), int(bool(fl & P.MATES_MOVED_B))]
        lines.append("\t".join(str(c) for c in cols) + "\n")
    return "".join(lines)


@pytest.fixture(scope="module")
def files(workdir, built):
    """the index of the table's collection; the reads as lines, FASTA and FASTQ; the expected --mates text from the bindings"""
    text = os.path.join(workdir, "cli_mates_cases.txt")
    with open(text, "wb") as f:
        f.write(C.raw)
    ri, tags = W.build_index_from_text(text, workdir, "cli_mates_cases")[:2]
    paths = {fmt: os.path.join(workdir, "cli_mates_reads." + fmt) for fmt in ("lines", "fasta", "fastq")}
    with open(paths["lines"], "wb") as f:
        f.write(b"".join(r + b"\n" for r in READS))
    with open(paths["fasta"], "wb") as f:
        f.write(b"".join(b">r%d\n" % i + r[:30] + b"\n" + r[30:] + b"\n" for i, r in enumerate(READS)))  # (two lines a sequence)
    with open(paths["fastq"], "wb") as f:
        f.write(b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(READS)))
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    cat, offs = O.pack_reads(READS)
    b = P.Batch(idx, cat, offs)
    b.run(MC.MIN_LEN, 1, 0)
    b.locate(0)
    b.read_place(P.PLACE_LIST)
    b.read_verify(16, 4, P.VERIFY_LIST)
    mated = b.read_mates(MC.FRAG_MIN, MC.FRAG_MAX, 10, P.MATES_ELECT)  # (what --paired takes: --verify-max 16, U = 2 * (4 + 1))
    b.free()
    idx.close()
    assert mated["n_pairs"] == len(PAIRS) == 158 and mated["n_moved_a"] + mated["n_moved_b"] == 44
    return ri, tags, paths, mates_text(mated["pairs"])


@pytest.mark.parametrize("fmt,extra", [("lines", []), ("lines", ["--batch", 2]), ("lines", ["--batch", 6, "--streams", 2]), ("lines", ["--batch", 7]),
                                       ("lines", ["--batch", 6, "--device-parse"]), ("lines", ["--batch", 7, "--device-parse"]),
                                       ("fasta", ["--batch", 7, "--reads-format", "fasta"]), ("fastq", ["--batch", 2, "--reads-format", "fastq"]),
                                       ("fastq", ["--batch", 7, "--reads-format", "auto"])])
def test_the_mates_file_equals_the_bindings_whatever_the_ranges(files, tmp_path, fmt, extra):
    ri, tags, paths, want = files
    out = str(tmp_path / "pairs.tsv")
    r = _run(ri, tags, paths[fmt], MC.MIN_LEN, 1, *OPTS, "--mates", out, "--mates-only", *extra)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    got = open(out).read()
    assert got.count("\n") == len(PAIRS) + 1 and got == want


def test_stdout_and_stderr_stay_and_the_winners_are_the_elected_ones(files, tmp_path):
    ri, tags, paths, want = files
    out, ver, gaf, ver0, gaf0 = (str(tmp_path / n) for n in ("pairs.tsv", "paired.verify", "paired.gaf", "solo.verify", "solo.gaf"))
    for extra in ([], ["--batch", 6, "--streams", 2], ["--format", "device", "--batch", 7]):
        plain = _run(ri, tags, paths["lines"], MC.MIN_LEN, 1, "--mode", "strict", *extra)
        paired = _run(ri, tags, paths["lines"], MC.MIN_LEN, 1, *OPTS, "--mates", out, "--verify", ver, "--gaf", gaf, *extra)
        assert plain.returncode == 0 and paired.returncode == 0, paired.stderr
        assert strip_timing(paired.stdout) == strip_timing(plain.stdout) and len(plain.stdout) > 1000
        assert _stderr(paired.stderr) == _stderr(plain.stderr)
        assert open(out).read() == want
    solo = _run(ri, tags, paths["lines"], MC.MIN_LEN, 1, "--mode", "strict", "--verify-max", 16, "--verify", ver0, "--gaf", gaf0)
    assert solo.returncode == 0, solo.stderr

    def placed(verify_path, gaf_path):
        """(seq, pos) of every read by the verify file, and by the hs / ho tags of its GAF line"""
        v = [l.split("\t") for l in open(verify_path).read().split("\n")[1:-1]]
        g = [dict(f.split(":", 2)[::2] for f in l.split("\t")[12:]) for l in open(gaf_path).read().split("\n")[:-1]]
        return [None if x[1] == "*" else (int(x[1]), int(x[2])) for x in v], [(int(t["hs"]), int(t["ho"])) if "hs" in t else None for t in g]

    pv, pg = placed(ver, gaf)
    sv, sg = placed(ver0, gaf0)
    assert len(pv) == len(pg) == len(READS) and len(SECOND) == 24
    for r in SECOND:  # wholly inside the sequence: the alignment starts where the read does
        assert pv[r] == pg[r] == TRUTHS[r] and sv[r] == sg[r] != TRUTHS[r] and sv[r][0] == TRUTHS[r][0], r
    kept = [r for r, k in enumerate(k for k in PAIRS for _ in (0, 1)) if C.kinds[k] in ("unique", "far", "cross", "same_strand", "border")]
    assert all(pv[r] == sv[r] == TRUTHS[r] for r in kept) and len(kept) >= 100


def test_paired_gaf_lines_replay_on_the_walk_graph(world, tmp_path):  # noqa: F811
    ri, tags, texts = world
    K = RC.CASES
    reads = [r for r in K.reads if r]
    reads = reads[:len(reads) & ~1]
    path, gaf = str(tmp_path / "replay_pairs.txt"), str(tmp_path / "replay_pairs.gaf")
    with open(path, "wb") as f:
        f.write(b"".join(r + b"\n" for r in reads))
    r = _run(ri, tags, path, RC.MIN_LEN, 1, "--mode", "strict", "--paired", "--align-band", 31, "--gaf", gaf, "--gaf-only", "--batch", 64)
    assert r.returncode == 0, r.stderr
    lines = open(gaf).read().split("\n")[:-1]
    assert len(lines) == len(reads) >= 500
    with_path = sum(G.replay_gaf_line(line, read, K.node_seq, texts=texts, number=i + 1) is not None for i, (line, read) in enumerate(zip(lines, reads)))
    assert with_path >= 400


def test_refusals(files, tmp_path):
    ri, tags, paths, _ = files
    out = str(tmp_path / "refused.tsv")
    odd = str(tmp_path / "odd.txt")
    with open(odd, "wb") as f:
        f.write(b"".join(r + b"\n" for r in READS[:7]))
    r = _run(ri, tags, odd, MC.MIN_LEN, 1, *OPTS, "--mates", out, "--batch", 2)
    assert r.returncode == 1 and "7 records, an odd number" in r.stderr
    r = _run(ri, tags, paths["lines"], MC.MIN_LEN, 1, *OPTS, "--mates", out, "--mates-only", "--locate", "positions")
    assert r.returncode == 1 and r.stdout == "" and "--mates-only" in r.stderr
    for args in (["--mates", out], ["--mates", out, "--mates-only"], ["--frag-max", 400], ["--mates-penalty", 3]):
        r = _run(ri, tags, paths["lines"], MC.MIN_LEN, 1, "--mode", "strict", *args)
        assert r.returncode == 1 and r.stdout == "" and "usage:" in r.stderr, args
    r = _run(ri, tags, paths["lines"], MC.MIN_LEN, 1, *OPTS, "--mates-only")
    assert r.returncode == 1 and "usage:" in r.stderr
    r = _run(ri, tags, paths["lines"], MC.MIN_LEN, 1, "--mode", "strict", "--paired", "--frag-min", 600, "--frag-max", 500)
    assert r.returncode == 1 and "--frag-min 600 exceeds --frag-max 500" in r.stderr
