"""build_tags on the GPU: pgx_build_tags / pgx_build_tags_paths and the build_tags CLI against the reference's own output
(bidirectional_test/xy_bidirectional.tags), through the rest of the pipeline (convert_tags, find_mems, merge_tags), with
forward-only texts, at a few million rows against numpy truth from the oracle's suffix array, with runs past 511 and 65 536,
and on malformed graphs."""
import os
import subprocess

import numpy as np
import pytest

import gbz_graph_emu as E
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
from cli_format import strip_timing

pytestmark = pytest.mark.gpu

G = O.GOLDEN
BT = os.path.join(G, "bidirectional_test")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pangenome-index_amd")
GOLD = os.path.join(BT, "xy_bidirectional.tags")


def _run(exe, *args):
    return subprocess.run([os.path.join(BIN, exe)] + [str(a) for a in args], capture_output=True, timeout=600)


def _tables(gbz, forward_only=False):
    g, seqs, fid = E.parse_graph(gbz)
    return E.graph_tables(g, seqs, fid, forward_only)


def _truth(ri, po, pn, nl, fid, reference=False):
    """the restatement's file for index ri and the stated graph"""
    r = O.RIndex(ri)
    n_seq = int(r.C_array()[1])
    tags = E.row_tags(r.decompress_sa(), n_seq, r.max_length, po, pn, nl, fid)
    v, l = E.runs(tags, n_seq)
    if reference:
        v, l = E.reference_runs(v, l)
    return E.encode(v, l), v, l


def _compact_runs(path):
    t = O.Tags(path, O.TAGS_COMPACT)
    return [(t.L.orc_tags_interval(t.h, k), t.L.orc_tags_item(t.h, k)) for k in range(t.n_runs)]


def test_golden_file(built, tmp_path):
    out = str(tmp_path / "xy.tags")
    ms = P.build_tags(os.path.join(BT, "xy.gbz"), os.path.join(BT, "xy.ri"), out)
    assert open(out, "rb").read() == open(GOLD, "rb").read()
    assert set(ms) == set(P.BUILD_TAGS_STAGES) and ms["suffix_array"] > 0 and ms["graph"] > 0
    # the reference's argv: graph, .rl_bwt (r-index built in memory), output; nothing on stdout
    cli = str(tmp_path / "cli.tags")
    r = _run("build_tags", os.path.join(BT, "xy.gbz"), os.path.join(BT, "contigs_xy.rl_bwt"), cli)
    assert r.returncode == 0, r.stderr
    assert r.stdout == b"" and b"suffix array" in r.stderr
    assert open(cli, "rb").read() == open(GOLD, "rb").read()
    # the same through the stated tables
    tab = str(tmp_path / "tab.tags")
    po, pn, nl, fid = _tables(os.path.join(BT, "xy.gbz"))
    P.build_tags_paths(os.path.join(BT, "xy.ri"), po, pn, nl, fid, tab)
    assert open(tab, "rb").read() == open(GOLD, "rb").read()


def test_end_to_end_convert_and_find_mems(built, tmp_path):
    built_tags = str(tmp_path / "xy.tags")
    P.build_tags(os.path.join(BT, "xy.gbz"), os.path.join(BT, "xy.ri"), built_tags)
    conv = str(tmp_path / "xy_compressed.tags")
    P.convert_tags(built_tags, conv, compact=False)
    assert open(conv, "rb").read() == open(os.path.join(BT, "xy_bidirectional_compressed.tags"), "rb").read()
    r = subprocess.run([os.path.join(BIN, "find_mems"), os.path.join(BT, "xy.ri"), conv, os.path.join(BT, "reads.txt"), "5", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert strip_timing(r.stdout) == open(os.path.join(G, "expected_find_mems_xy_reads_5_1.txt")).read()


def test_whole_pipeline_from_the_graph(built, tmp_path):
    r = _run("gbz_extract", "-b", os.path.join(BT, "xy.gbz"))
    assert r.returncode == 0, r.stderr
    text = str(tmp_path / "xy.txt")
    open(text, "wb").write(r.stdout)
    rl, ri = str(tmp_path / "xy.rl_bwt"), str(tmp_path / "xy.ri")
    P.build_index_from_text(text, rl, ri, encoded=False)
    assert open(ri, "rb").read() == open(os.path.join(BT, "xy.ri"), "rb").read()
    out = str(tmp_path / "xy.tags")
    r = _run("build_tags", os.path.join(BT, "xy.gbz"), ri, out, "--ri", "--device", "0")
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(GOLD, "rb").read()
    out2 = str(tmp_path / "xy_rl.tags")
    r = _run("build_tags", os.path.join(BT, "xy.gbz"), rl, out2)
    assert r.returncode == 0, r.stderr
    assert open(out2, "rb").read() == open(GOLD, "rb").read()


def test_per_chromosome_then_merge(built, tmp_path):
    """x and y tagged on their own indexes, merged along xy.ri with the graph's component map: the runs of the reference's
    whole-genome tags"""
    paths = []
    for c in ("x", "y"):
        out = str(tmp_path / ("%s.tags" % c))
        r = _run("build_tags", os.path.join(BT, "%s.gbz" % c), os.path.join(BT, "contigs_%s.rl_bwt" % c), out)
        assert r.returncode == 0, r.stderr
        paths.append(out)
    merged = str(tmp_path / "merged.tags")
    P.merge_tags_gbz(os.path.join(BT, "xy.gbz"), os.path.join(BT, "xy.ri"), paths, merged)
    conv = str(tmp_path / "conv.tags")
    P.convert_tags(GOLD, conv, compact=True)
    # merge_tags opens with the endmarker rows (value 0, n_seq = 8 rows); convert_tags, like the reference's, reads the file's
    # int_vector header as one more run in front: past that first run both hold the same runs
    m, c = _compact_runs(merged), _compact_runs(conv)
    assert m[0][1] == 0 and m[1][0] == 8
    mv, cv = [v for _, v in m[1:]], [v for _, v in c[1:]]
    ml, cl = np.diff([s for s, _ in m[1:]]), np.diff([s for s, _ in c[1:]])
    assert mv == cv and np.array_equal(ml, cl) and len(mv) == 6030
    gv, gl = E.decode(open(GOLD, "rb").read())
    assert mv == gv.tolist() and np.array_equal(ml, gl[:-1])


def test_forward_only(built, tmp_path):
    # xy.gbz with the one-orientation text of two_contig_graph
    ri = os.path.join(G, "two_contig_graph", "xy.ri")
    out = str(tmp_path / "fwd.tags")
    P.build_tags(os.path.join(BT, "xy.gbz"), ri, out, flags=P.BUILD_TAGS_FORWARD_ONLY)
    po, pn, nl, fid = _tables(os.path.join(BT, "xy.gbz"), forward_only=True)
    assert open(out, "rb").read() == _truth(ri, po, pn, nl, fid)[0]
    # the reference README's example: x.giraffe.gbz + x.rl_bwt (one orientation per path)
    ri_x = str(tmp_path / "x.ri")
    P.build_rindex(os.path.join(G, "x.rl_bwt"), ri_x)
    gbz = os.path.join(G, "x.giraffe.gbz")
    out = str(tmp_path / "x.tags")
    P.build_tags(gbz, ri_x, out, flags=P.BUILD_TAGS_FORWARD_ONLY)
    po, pn, nl, fid = _tables(gbz, forward_only=True)
    assert open(out, "rb").read() == _truth(ri_x, po, pn, nl, fid)[0]
    bad = str(tmp_path / "x_bad.tags")
    with pytest.raises(P.PgxError) as e:
        P.build_tags(gbz, ri_x, bad)
    assert e.value.code == P.ERR_FORMAT and "sequence" in str(e.value) and not os.path.exists(bad)
    r = _run("build_tags", gbz, os.path.join(G, "x.rl_bwt"), bad)
    assert r.returncode != 0 and b"forward-only" in r.stderr and not os.path.exists(bad)
    r = _run("build_tags", gbz, os.path.join(G, "x.rl_bwt"), bad, "--forward-only")
    assert r.returncode == 0, r.stderr
    assert open(bad, "rb").read() == _truth(ri_x, po, pn, nl, fid)[0]


def test_scale_random_nodes(built, tmp_path):
    """a few million rows: every haplotype chopped at random into nodes of 1..1024 bp (ids not shared, some ids unused, a
    node offset), reverse sequences walk the reversed path; every run against numpy truth from the oracle's SA"""
    text = str(tmp_path / "synth.txt")
    n_seq = W.synth_pangenome_text(text, base_len=400_000, n_hap=4, seed=11)
    ri, _tags, _rl = W.build_index_from_text(text, str(tmp_path), "synth", with_tags=False)
    lens = [len(x) for x in open(text, "rb").read().split(b"\n")[:-1]]
    assert len(lens) == n_seq and sum(lens) + n_seq > 3_000_000
    rng = np.random.default_rng(3)
    fid = 7
    node_len, po, pn = [], [0], []
    for k in range(0, n_seq, 2):
        cut = []
        left = lens[k]
        while left:
            ln = int(min(left, rng.choice([1, 2, int(rng.integers(1, 1025)), 1024])))
            cut.append(ln)
            left -= ln
        if rng.random() < 0.5:
            node_len += [0] * int(rng.integers(1, 4))  # ids without a sequence
        ids = np.arange(len(cut), dtype=np.uint64) + np.uint64(fid + len(node_len))
        node_len += cut
        fwd = ids << np.uint64(1)
        for path in (fwd, (fwd[::-1] | np.uint64(1))):
            pn.append(path)
            po.append(po[-1] + len(path))
    pn = np.concatenate(pn)
    nl = np.array(node_len, dtype=np.uint32)
    assert nl.min() == 0 and (nl == 1).sum() > 100 and nl.max() == 1024
    out = str(tmp_path / "synth.tags")
    ms = P.build_tags_paths(ri, np.array(po, dtype=np.uint64), pn, nl, fid, out)
    raw, v, l = _truth(ri, np.array(po, dtype=np.uint64), pn, nl, fid)
    got = open(out, "rb").read()
    assert len(got) == len(raw) and got == raw
    assert ms["graph"] == 0 and ms["suffix_array"] > 0


def _identical(tmp_path, name, n, seq=b"ACGTTGCA", extra=b""):
    text = str(tmp_path / (name + ".txt"))
    with open(text, "wb") as f:
        f.write((seq + b"\n") * n + extra)
    ri, _t, _rl = W.build_index_from_text(text, str(tmp_path), name, with_tags=False)
    return ri


def _one_node_each(n, ln, node=1):
    po = np.arange(n + 1, dtype=np.uint64)
    pn = np.full(n, node << 1, dtype=np.uint64)
    nl = np.zeros(node + 1, dtype=np.uint32)
    nl[node] = ln
    return po, pn, nl


def test_long_runs(built, tmp_path):
    # 600 identical sequences: every run of 600 rows becomes 511 + 89
    ri = _identical(tmp_path, "six_hundred", 600, seq=b"ACGTTGCAGGATTC")
    po, pn, nl = _one_node_each(600, 14)
    out = str(tmp_path / "600.tags")
    P.build_tags_paths(ri, po, pn, nl, 0, out)
    raw, v, l = _truth(ri, po, pn, nl, 0)
    assert open(out, "rb").read() == raw and set(l.tolist()) == {600}
    dv, dl = E.decode(raw)
    assert sorted(set(dl.tolist())) == [89, 511]
    # 70 000: exact by default, mod 65 536 with REFERENCE_RUNS
    ri = _identical(tmp_path, "seventy_k", 70000)
    po, pn, nl = _one_node_each(70000, 8)
    out, ref = str(tmp_path / "70k.tags"), str(tmp_path / "70k_ref.tags")
    P.build_tags_paths(ri, po, pn, nl, 0, out)
    P.build_tags_paths(ri, po, pn, nl, 0, ref, flags=P.BUILD_TAGS_REFERENCE_RUNS)
    raw, v, l = _truth(ri, po, pn, nl, 0)
    assert open(out, "rb").read() == raw and set(l.tolist()) == {70000}
    raw_ref, v2, l2 = _truth(ri, po, pn, nl, 0, reference=True)
    assert open(ref, "rb").read() == raw_ref and set(l2.tolist()) == {70000 - 65536}
    # exactly 65 536: the runs vanish in reference mode, the other sequence's runs stay
    ri = _identical(tmp_path, "wrap", 65536, extra=b"TTTTGGGGCC\n")
    po = np.arange(65538, dtype=np.uint64)
    pn = np.array([2] * 65536 + [4], dtype=np.uint64)
    nl = np.array([0, 8, 10], dtype=np.uint32)
    out, ref = str(tmp_path / "wrap.tags"), str(tmp_path / "wrap_ref.tags")
    P.build_tags_paths(ri, po, pn, nl, 0, out)
    P.build_tags_paths(ri, po, pn, nl, 0, ref, flags=P.BUILD_TAGS_REFERENCE_RUNS)
    raw, v, l = _truth(ri, po, pn, nl, 0)
    raw_ref, v2, l2 = _truth(ri, po, pn, nl, 0, reference=True)
    assert open(out, "rb").read() == raw and open(ref, "rb").read() == raw_ref
    assert 65536 in set(l.tolist()) and set(l2.tolist()) == {1} and all(int(x) >> 11 == 2 for x in v2)


def test_errors(built, tmp_path):
    ri = os.path.join(BT, "xy.ri")
    po, pn, nl, fid = _tables(os.path.join(BT, "xy.gbz"))
    out = str(tmp_path / "bad.tags")

    def fails(po_, pn_, nl_, *words):
        with pytest.raises(P.PgxError) as e:
            P.build_tags_paths(ri, po_, pn_, nl_, fid, out)
        assert e.value.code == P.ERR_FORMAT, e.value
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        assert not os.path.exists(out)

    # a path's length differs from its sequence's: a node of y (sequences 4..7) one base longer
    nl2 = nl.copy()
    nl2[(int(pn[int(po[4])]) >> 1) - fid] += 1
    fails(po, pn, nl2, "sequence 4", "bp")
    # a node longer than 1024 bp
    nl3 = nl.copy()
    nl3[(int(pn[0]) >> 1) - fid] = 1025
    fails(po, pn, nl3, "sequence 0", "1024")
    # an unknown node id
    pn2 = pn.copy()
    pn2[int(po[2]) + 3] = (len(nl) + fid + 5) << 1
    fails(po, pn2, nl, "sequence 2", "no sequence")
    # sequence counts differ
    fails(po[:-1], pn[:int(po[-2])], nl, "sequence 7", "8 sequences")
    # the graph side of pgx_build_tags
    with pytest.raises(P.PgxError) as e:
        P.build_tags(os.path.join(BT, "xy.ri"), ri, out)
    assert e.value.code == P.ERR_FORMAT and not os.path.exists(out)
