"""build_tags, CPU tier: the GBZ graph reader behind pgx_build_tags / pgx_gbz_extract (GBWTGraph node sequences after the
GBWT's document-array samples and metadata; every path as its node list) on the reference's GBZ fixtures, and the Python
restatement of what the device pipeline computes (tests/gbz_graph_emu.py) against the reference's own build_tags output,
bidirectional_test/xy_bidirectional.tags."""
import os
import subprocess

import numpy as np
import pytest

import gbz_emu
import gbz_graph_emu as E
import oracle_ffi as O
import pgx_ffi as P

G = O.GOLDEN
BT = os.path.join(G, "bidirectional_test")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRACT = os.path.join(ROOT, "pangenome-index_amd", "gbz_extract")

# (graph, text, both orientations): gbz_extract -b gives the contigs_* texts, the forward orientation the one-per-path ones
TEXTS = [("xy.gbz", os.path.join(BT, "contigs_xy"), True), ("x.gbz", os.path.join(BT, "contigs_x"), True),
         ("y.gbz", os.path.join(BT, "contigs_y"), True), ("xy.gbz", os.path.join(G, "two_contig_graph", "contigs_XY.txt"), False),
         ("x.giraffe.gbz", os.path.join(G, "x.newline_separated"), False)]
FIXTURES = [os.path.join(BT, "xy.gbz"), os.path.join(BT, "x.gbz"), os.path.join(BT, "y.gbz"), os.path.join(G, "x.giraffe.gbz")]


def _gbz(name):
    return os.path.join(G if name == "x.giraffe.gbz" else BT, name)


@pytest.mark.parametrize("name,text,both", TEXTS)
def test_gbz_extract_reproduces_the_texts(built, tmp_path, name, text, both):
    out = str(tmp_path / "text")
    P.gbz_extract(_gbz(name), out, both=both)
    assert open(out, "rb").read() == open(text, "rb").read()
    assert E.extract_text(_gbz(name), forward_only=not both) == open(text, "rb").read()  # the restatement agrees


@pytest.mark.parametrize("name,text,both", TEXTS)
def test_gbz_extract_cli(built, name, text, both):
    args = [EXTRACT] + (["-b"] if both else []) + [_gbz(name)]
    r = subprocess.run(args, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == open(text, "rb").read()


def test_gbz_extract_cli_rejects_options(built):
    r = subprocess.run([EXTRACT, _gbz("xy.gbz"), "--both"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "unknown option" in r.stderr and r.stdout == ""
    r = subprocess.run([EXTRACT, os.path.join(BT, "xy.ri")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "GBZ" in r.stderr


@pytest.mark.parametrize("path", FIXTURES)
def test_library_paths_match_the_gbwt_walk(built, tmp_path, path):
    """every sequence spelled by the library (pgx_gbz_extract, one line per GBWT sequence) is the walk of gbz_emu over the
    graph's node sequences: the same node list, hence the same length and bytes"""
    g, seqs, fid = E.parse_graph(path)
    out = str(tmp_path / "all")
    P.gbz_extract(path, out, both=True)
    lines = open(out, "rb").read().split(b"\n")[:-1]
    assert len(lines) == g["nseq"]
    for s in range(g["nseq"]):
        walk = gbz_emu.walk(g, s)
        assert lines[s] == E.spell(seqs, fid, walk)
        assert len(lines[s]) == sum(len(seqs[(v >> 1) - fid]) for v in walk)


def test_graph_layout(built):
    """the GBWTGraph sits where skipping the document-array samples and the metadata puts it; ids that do not occur are empty"""
    g, seqs, fid = E.parse_graph(os.path.join(BT, "x.gbz"))
    assert fid == 1 and len(seqs) == 69 and sum(1 for x in seqs if not x) == 6
    g, seqs, fid = E.parse_graph(os.path.join(BT, "y.gbz"))
    assert fid == 70 and len(seqs) == 69  # GBWT offset 139


def test_gbz_extract_errors(built, tmp_path):
    with pytest.raises(P.PgxError) as e:
        P.gbz_extract(os.path.join(BT, "xy.ri"), str(tmp_path / "t"))
    assert e.value.code == P.ERR_FORMAT
    raw = open(os.path.join(BT, "xy.gbz"), "rb").read()
    for cut in (2100, 2500, 2950, 3300, len(raw) - 300):  # inside the DA samples, metadata, graph header, node sequences
        bad = str(tmp_path / "trunc.gbz")
        open(bad, "wb").write(raw[:cut])
        with pytest.raises(P.PgxError) as e:
            P.gbz_extract(bad, str(tmp_path / "t"))
        assert e.value.code == P.ERR_FORMAT
    with pytest.raises(P.PgxError) as e:
        P.gbz_extract(str(tmp_path / "missing.gbz"), str(tmp_path / "t"))
    assert e.value.code == P.ERR_IO


def test_restatement_reproduces_the_reference_tags(built):
    """oracle SA of xy.ri + graph tables of xy.gbz -> tag per row -> maximal runs -> pieces of <= 511 -> ByteCode file: the
    reference's build_tags output byte for byte"""
    r = O.RIndex(os.path.join(BT, "xy.ri"))
    sa = r.decompress_sa()
    n_seq = int(r.C_array()[1])
    g, seqs, fid = E.parse_graph(os.path.join(BT, "xy.gbz"))
    po, pn, nl, fid = E.graph_tables(g, seqs, fid)
    tags = E.row_tags(sa, n_seq, r.max_length, po, pn, nl, fid)
    v, l = E.runs(tags, n_seq)
    raw = E.encode(v, l)
    gold = open(os.path.join(BT, "xy_bidirectional.tags"), "rb").read()
    assert (len(sa) - n_seq, len(v), len(raw)) == (8014, 6030, 24096)
    assert raw == gold
    dv, dl = E.decode(gold)
    assert np.array_equal(dv, v) and np.array_equal(dl, l)  # no run of the fixture reaches 512


def test_reference_uint16_loop_is_the_mod_65536_rule():
    rng = np.random.default_rng(5)
    n_seq = 3
    pieces = []
    for ln in (1, 65535, 65536, 65537, 70000, 131072, 131073, 2, 511, 512):  # runs around the wrap points
        pieces.append(np.full(ln, int(rng.integers(1, 1 << 30)) << 11, dtype=np.uint64))
    pieces.append(rng.integers(1, 5, size=5000).astype(np.uint64) << np.uint64(11))  # short runs, repeated values
    tags = np.concatenate([np.zeros(n_seq, dtype=np.uint64)] + pieces)
    v, l = E.runs(tags, n_seq)
    rv, rl = E.reference_runs(v, l)
    lv, ll = E.reference_uint16_loop(tags, n_seq)
    assert np.array_equal(rv, lv) and np.array_equal(rl, ll)
    assert 65536 not in set(int(x) for x in l & np.uint64(0xFFFF)) and len(rv) == len(v) - 2  # 65536 and 131072 vanish
    # the ByteCode file splits at 511 either way
    assert E.decode(E.encode(v[:1], np.array([1023], dtype=np.uint64)))[1].tolist() == [511, 511, 1]
