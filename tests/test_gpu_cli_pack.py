"""GPU tier: `find_mems --pack`.  The two files against coverage recomputed in Python from the --gaf file of the same invocation -- walk column 6,
slice by columns 8 and 9, apply cg:Z: -- which is the host route the option replaces, on the reads of tests/replay_cases.py (mixed edits, clips,
both orientations); the same files under --batch sizes that cut the reads into 1, 3 and 7 batches and under --streams 2; --pack-min-mapq with
--mapq against the qualities of the --mapq-file of the same run; --pack-only leaves stdout empty; without --pack, stdout, stderr and the GAF file
are those of the run with it; an index without tags ends the run before any batch."""
import os
import re
import subprocess

import pytest

import pgx_ffi as P
import pgx_workload as W
import replay_cases as C
from cli_format import strip_timing

pytestmark = pytest.mark.gpu

K = C.CASES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")
_STEP = re.compile(r"([<>])(\d+)")
_CG = re.compile(r"(\d+)([=XIDS])")


@pytest.fixture(scope="module")
def world(workdir):
    g = K.graph
    text = os.path.join(workdir, "cli_pack_graph.txt")
    with open(text, "wb") as f:
        f.write(b"".join(t + b"\n" for t in g["texts"]))
    ri = W.build_index_from_text(text, workdir, "cli_pack_graph", with_tags=False)[0]
    tags = os.path.join(workdir, "cli_pack_graph.graph.tags")
    P.build_tags_paths(ri, g["path_offsets"], g["path_nodes"], g["node_length"], 1, tags, flags=P.BUILD_TAGS_OUT_COMPACT)
    reads = [r for r in K.reads if r]  # (a line file cannot hold the empty read)
    path = os.path.join(workdir, "cli_pack_reads.txt")
    with open(path, "wb") as f:
        f.write(b"".join(r + b"\n" for r in reads))
    return ri, tags, path, len(reads)


def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def _stderr(text):
    return "\n".join(l for l in text.split("\n") if " took " not in l)


def coverage_from_gaf(lines, node_len, min_mapq=0):
    """{(node, offset): reads} from GAF lines: the path of column 6 laid out base by base in the nodes' forward offsets, the stretch of columns 8 and
    9 walked by cg:Z: (= and X add, D skips, I stays).  Lines whose column 12 is below min_mapq are left out."""
    cov = {}
    for line in lines:
        c = line.split("\t")
        if c[5] == "*" or (min_mapq and int(c[11]) < min_mapq):
            continue
        at = []
        for sign, node in _STEP.findall(c[5]):
            ln = node_len[int(node)]
            at += [(int(node), ln - 1 - d if sign == "<" else d) for d in range(ln)]
        assert len(at) == int(c[6])
        t = int(c[7])
        cg = [x for x in c[12:] if x.startswith("cg:Z:")][0][5:]
        for ln, op in _CG.findall(cg):
            ln = int(ln)
            if op in "=X":
                for p in range(t, t + ln):
                    cov[at[p]] = cov.get(at[p], 0) + 1
            if op in "=XD":
                t += ln
        assert t == int(c[8])
    return cov


def files_of(cov, node_len):
    """the --pack and --pack-bases files of a coverage map"""
    nodes = "#node\tlength\tcovered\tsum\tmax\n"
    for node in sorted(node_len):
        vals = [cov[(node, o)] for o in range(node_len[node]) if (node, o) in cov]
        nodes += "%d\t%d\t%d\t%d\t%d\n" % (node, node_len[node], len(vals), sum(vals), max(vals) if vals else 0)
    bases = "#node\toffset\tcoverage\n" + "".join("%d\t%d\t%d\n" % (n, o, cov[(n, o)]) for n, o in sorted(cov))
    return nodes, bases


def _node_len():
    return {k: len(s) for k, s in K.node_seq.items()}


def test_the_files_equal_the_coverage_of_the_gaf_file_whatever_the_batches(world, tmp_path):
    ri, tags, reads, n = world
    base = [ri, tags, reads, C.MIN_LEN, 1, "--mode", "strict", "--align-band", 31]
    gaf0 = str(tmp_path / "plain.gaf")
    plain = _run(*base, "--gaf", gaf0)
    assert plain.returncode == 0, plain.stderr
    want = None
    for k, extra in enumerate(([], ["--batch", (n + 2) // 3], ["--batch", (n + 6) // 7], ["--batch", (n + 6) // 7, "--streams", 2], ["--batch", 64, "--format", "device", "--device-parse"])):
        gaf, pack, bases = (str(tmp_path / ("%d.%s" % (k, e))) for e in ("gaf", "pack", "bases"))
        r = _run(*base, "--gaf", gaf, "--pack", pack, "--pack-bases", bases, *extra)
        assert r.returncode == 0, r.stderr
        lines = open(gaf).read().split("\n")[:-1]
        assert len(lines) == n
        cov = coverage_from_gaf(lines, _node_len())
        nodes_text, bases_text = files_of(cov, _node_len())
        assert open(pack).read() == nodes_text, extra
        assert open(bases).read() == bases_text, extra
        assert len(cov) > 1000 and max(cov.values()) > 5
        if want is None:
            want = (nodes_text, bases_text)
            # without --pack: stdout, stderr and the GAF file are those of the run with it
            assert strip_timing(r.stdout) == strip_timing(plain.stdout) and len(plain.stdout) > 1000 and _stderr(r.stderr) == _stderr(plain.stderr)
            assert open(gaf).read() == open(gaf0).read()
        assert (nodes_text, bases_text) == want, extra
    alone = str(tmp_path / "alone.pack")  # --pack runs the stages itself, without a walk
    r = _run(*base, "--pack", alone)
    assert r.returncode == 0 and open(alone).read() == want[0], r.stderr
    assert strip_timing(r.stdout) == strip_timing(plain.stdout) and _stderr(r.stderr) == _stderr(plain.stderr)


def test_pack_min_mapq_counts_the_reads_the_gaf_file_gives_that_quality(world, tmp_path):
    ri, tags, reads, n = world
    base = [ri, tags, reads, C.MIN_LEN, 1, "--mode", "strict", "--align-band", 31, "--mapq", "--mapq-slack", 0]
    seen = {}
    for q in (1, 30, 60):
        gaf, pack, bases = (str(tmp_path / ("q%d.%s" % (q, e))) for e in ("gaf", "pack", "bases"))
        r = _run(*base, "--gaf", gaf, "--pack", pack, "--pack-bases", bases, "--pack-min-mapq", q, "--batch", 100)
        assert r.returncode == 0, r.stderr
        lines = open(gaf).read().split("\n")[:-1]
        nodes_text, bases_text = files_of(coverage_from_gaf(lines, _node_len(), q), _node_len())
        assert open(pack).read() == nodes_text and open(bases).read() == bases_text, q
        seen[q] = bases_text
    assert len(seen[60]) < len(seen[1])  # (some placed read has a quality below 60)
    only = str(tmp_path / "noq.pack")  # --mapq is satisfied by --pack alone
    r = _run(*base, "--pack", only, "--pack-min-mapq", 60)
    assert r.returncode == 0 and open(only).read() == files_of(coverage_from_gaf(open(str(tmp_path / "q60.gaf")).read().split("\n")[:-1], _node_len(), 60), _node_len())[0], r.stderr


def test_pack_only_and_an_index_without_tags(world, tmp_path):
    ri, tags, reads, n = world
    base = [ri, tags, reads, C.MIN_LEN, 1, "--mode", "strict", "--align-band", 31]
    full, only = str(tmp_path / "full.pack"), str(tmp_path / "only.pack")
    a = _run(*base, "--pack", full)
    b = _run(*base, "--pack", only, "--pack-only")
    assert a.returncode == 0 and b.returncode == 0, b.stderr
    assert b.stdout == "" and len(a.stdout) > 1000 and open(only).read() == open(full).read()
    r = _run(*base, "--pack", only, "--pack-only", "--locate", "positions")
    assert r.returncode == 1 and "does not go with --locate" in r.stderr
    out = str(tmp_path / "refused.pack")
    r = _run(ri, "-", reads, C.MIN_LEN, 1, "--mode", "strict", "--pack", out)
    assert r.returncode == 1 and r.stdout == "", r.stderr
    assert "without a tag array" in r.stderr and "--pack" in r.stderr and not os.path.exists(out)
