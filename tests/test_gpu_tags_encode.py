"""Tag query files encoded on the GPU (pgx_tags_encode, build_tags with an OUT flag, merge_tags with MERGE_DEVICE_ENCODE) against the
HOST writers, byte for byte: P.write_compact_tags for the compact form, the build_tags file of the runs (gbz_graph_emu.encode)
through P.convert_tags(compact=False) for the ByteCode form.  Nothing expected here comes from the code under test.

Every comparison of the primitive runs twice per call site: no byte of the encoder may depend on the order in which its blocks or
atomics happen to run."""
import os
import pathlib
import struct
import subprocess

import numpy as np
import pytest

import gbz_graph_emu as E
import merge_cases as M
import oracle_ffi as O
import pgx_ffi as P
import test_gpu_build_tags as BT
from cli_format import strip_timing

pytestmark = pytest.mark.gpu

G = O.GOLDEN
BTD = os.path.join(G, "bidirectional_test")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pangenome-index_amd")
COMPACT, BYTECODE = P.TAGS_COMPACT, P.TAGS_BYTECODE
_U = np.uint64


# ---- the host side: expected bytes
def algorithm_file(values, lengths):
    """gbz_graph_emu.encode(values, lengths) with numpy instead of a loop per piece (test_algorithm_file_is_encode holds the two together)"""
    v = np.asarray(values, dtype=_U)
    ln = np.asarray(lengths, dtype=_U)
    keep = ln > 0
    v, ln = v[keep], ln[keep]
    npieces = ((ln + _U(510)) // _U(511)).astype(np.int64)
    pv = np.repeat(v, npieces)
    pl = np.full(len(pv), 511, dtype=_U)
    last = np.cumsum(npieces) - 1
    pl[last] = ln - _U(511) * (npieces.astype(_U) - _U(1))
    codes = (pv & _U(0x7FF)) | (pl << _U(11)) | ((pv >> _U(11)) << _U(20))
    nb = np.ones(len(codes), dtype=np.int64)
    for k in range(1, 10):
        nb += (codes >> _U(7 * k)) != 0
    off = np.cumsum(nb) - nb
    body = np.zeros(int(nb.sum()), dtype=np.uint8)
    for k in range(10):
        m = nb > k
        if not m.any():
            break
        byte = ((codes[m] >> _U(7 * k)) & _U(0x7F)).astype(np.uint8)
        byte[nb[m] > k + 1] |= 0x80
        body[off[m] + k] = byte
    return struct.pack("<Q", 8 * len(body)) + body.tobytes() + b"\0" * (-len(body) % 8)


def host_bytes(d, values, lengths, fmt):
    v = np.asarray(values, dtype=_U)
    ln = np.asarray(lengths, dtype=_U)
    out = os.path.join(str(d), "host.tags")
    if fmt == COMPACT:
        P.write_compact_tags(out, v, ln)
    else:
        assert len(v) == 0 or int(v.max()) >> 11 < 1 << 44
        alg = os.path.join(str(d), "host.algorithm")
        with open(alg, "wb") as f:
            f.write(algorithm_file(v, ln))
        P.convert_tags(alg, out, compact=False)
    return open(out, "rb").read()


def first_difference(got, want):
    if got == want:
        return None
    n = min(len(got), len(want))
    a, b = np.frombuffer(got[:n], dtype=np.uint8), np.frombuffer(want[:n], dtype=np.uint8)
    d = np.flatnonzero(a != b)
    return "sizes %d / %d, first differing byte %s" % (len(got), len(want), int(d[0]) if len(d) else "none")


def check(d, values, lengths, fmts=(COMPACT, BYTECODE)):
    """device file == host file, twice"""
    v = np.asarray(values, dtype=_U)
    ln = np.asarray(lengths, dtype=_U)
    sizes = {}
    for fmt in fmts:
        want = host_bytes(d, v, ln, fmt)
        out = os.path.join(str(d), "device.tags")
        for rep in range(2):
            if os.path.exists(out):
                os.remove(out)
            ms = P.tags_encode(v, ln, out, fmt)
            got = open(out, "rb").read()
            assert first_difference(got, want) is None, (fmt, rep, len(v), first_difference(got, want))
            assert ms["file_bytes"] == len(want) and ms["device_bytes"] > 0
        sizes[fmt] = len(want)
    return sizes


def vals(nodes, n):
    """n run values over the given nodes, neighbours distinct"""
    nodes = np.asarray(nodes, dtype=_U)
    i = np.arange(n, dtype=_U)
    return (nodes[i.astype(np.int64) % len(nodes)] << _U(11)) | ((i & _U(1)) << _U(10)) | (i * _U(7) % _U(1024))


# ---- select_support_mcl of a host file, as far as the tests need it
def _int_vector(raw, o, width_byte=True):
    bits = struct.unpack_from("<Q", raw, o)[0]
    o += 8
    width = 1
    if width_byte:
        width = raw[o]
        o += 1
    return bits, width, o + (bits + 63) // 64 * 8


def _select(raw, o):
    """(arguments, bits of mini_or_long, long superblocks, offset behind)"""
    cnt = struct.unpack_from("<Q", raw, o)[0]
    o += 8
    if not cnt:
        return 0, 0, 0, o
    _, _, o = _int_vector(raw, o)
    kind_bits, _, o = _int_vector(raw, o, width_byte=False)
    n_long = 0
    for _ in range((cnt + 4095) // 4096):
        bits, width, o = _int_vector(raw, o)
        assert bits in (64 * width, 4096 * width)
        n_long += bits == 4096 * width
    return cnt, kind_bits, n_long, o


def _sd_vector(raw, o):
    """(size, ones, [select_1, select_0] as _select gives them, offset behind)"""
    size = struct.unpack_from("<Q", raw, o)[0]
    o += 9
    _, _, o = _int_vector(raw, o)
    _, _, o = _int_vector(raw, o, width_byte=False)
    s1 = _select(raw, o)
    s0 = _select(raw, s1[3])
    return size, s1[0], [s1[:3], s0[:3]], s0[3]


def compact_selects(raw):
    """the four select supports of a compact file: starts (1, 0), intervals (1, 0)"""
    _, _, o = _int_vector(raw, 0)
    a = _sd_vector(raw, o)
    b = _sd_vector(raw, a[3])
    assert b[3] == len(raw)
    return a[2] + b[2]


# ---- 0. the helpers of this file
def test_algorithm_file_is_encode(tmp_path):
    rng = np.random.default_rng(1)
    ln = np.array([0, 1, 510, 511, 512, 1022, 1023, 65535, 65536, 65537, 3, 0, 2000], dtype=_U)
    v = vals([1, 5, (1 << 44) - 1, 300, 1 << 20], len(ln))
    assert algorithm_file(v, ln) == E.encode(v, ln)
    for _ in range(5):
        n = int(rng.integers(1, 300))
        ln = rng.integers(0, 1500, n).astype(_U)
        v = vals(rng.integers(1, 1 << 40, 7), n)
        assert algorithm_file(v, ln) == E.encode(v, ln)
    assert algorithm_file([], []) == E.encode([], [])
    # the parser: the selects of a small host file
    raw = host_bytes(tmp_path, vals([3], 30), np.full(30, 2), COMPACT)
    s = compact_selects(raw)
    assert [x[0] for x in s][::2] == [3, 30] and all(x[1] == 0 and x[2] == 0 for x in s)


# ---- 1. the reference's own file
def _find_mems(tags):
    r = subprocess.run([os.path.join(BIN, "find_mems"), os.path.join(BTD, "xy.ri"), tags, os.path.join(BTD, "reads.txt"), "5", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return strip_timing(r.stdout)


def test_reference_fixture(built, tmp_path):
    gbz, ri = os.path.join(BTD, "xy.gbz"), os.path.join(BTD, "xy.ri")
    plain, bc, cp, conv = (str(tmp_path / n) for n in ("plain.tags", "bytecode.tags", "compact.tags", "conv.tags"))
    P.build_tags(gbz, ri, plain)
    ms = P.build_tags(gbz, ri, bc, flags=P.BUILD_TAGS_OUT_BYTECODE)
    assert set(ms) == set(P.BUILD_TAGS_STAGES) and ms["write"] > 0
    enc = P.tags_encode_timing()
    assert enc["file_bytes"] == os.path.getsize(bc) and enc["pieces"] > 0
    fixture = open(os.path.join(BTD, "xy_bidirectional_compressed.tags"), "rb").read()
    assert first_difference(open(bc, "rb").read(), fixture) is None
    P.build_tags(gbz, ri, cp, flags=P.BUILD_TAGS_OUT_COMPACT)
    P.convert_tags(plain, conv, compact=True)
    assert first_difference(open(cp, "rb").read(), open(conv, "rb").read()) is None
    want = open(os.path.join(G, "expected_find_mems_xy_reads_5_1.txt")).read()
    assert _find_mems(bc) == want and _find_mems(cp) == want
    t = O.Tags(cp, O.TAGS_COMPACT)
    assert t.n_runs == t.n_items and t.n_runs > 6030
    # the CLI: the reference's argv with --format; algorithm is the default and can be named
    for fmt, same in (("bytecode", bc), ("compact", cp), ("algorithm", plain)):
        out = str(tmp_path / ("cli_%s.tags" % fmt))
        r = BT._run("build_tags", gbz, os.path.join(BTD, "contigs_xy.rl_bwt"), out, "--format", fmt)
        assert r.returncode == 0 and r.stdout == b"", r.stderr
        assert open(out, "rb").read() == open(same, "rb").read(), fmt
        assert (b"device encoding" in r.stderr) == (fmt != "algorithm")


# ---- 2. the primitive at its borders
def test_no_runs_and_one_run(tmp_path):
    check(tmp_path, [], [])
    check(tmp_path, [5 << 11], [0])
    for ln in (1, 511, 512):
        check(tmp_path, [(9 << 11) | 1000], [ln])


BORDER_LENGTHS = (0, 1, 510, 511, 512, 1022, 1023, 65535, 65536, 65537)


def test_length_borders(tmp_path):
    ln = np.array(BORDER_LENGTHS, dtype=_U)
    check(tmp_path, vals([1, 2, 77], len(ln)), ln)
    check(tmp_path, vals([4], len(ln)), ln[::-1].copy())
    for one in BORDER_LENGTHS:
        check(tmp_path, vals([6, 3], 3), [2, one, 1])


def test_positions_beyond_32_bits(tmp_path):
    # one run of 2^32 + 5 rows (8 404 997 pieces), short runs on both sides: BWT positions pass 2^32
    sizes = check(tmp_path, vals([3, 9], 5), [7, 600, (1 << 32) + 5, 1, 513])
    assert sizes[COMPACT] > 8_404_997 * 12 // 8


@pytest.mark.parametrize("pieces", [9, 10, 11, 40950, 40951, 40960, 40961, 4095, 4096, 4097, 8192])
def test_piece_count_borders(tmp_path, pieces):
    # 4096 ones of `starts` = 40 960 pieces, 4096 ones of `intervals` = 4096 pieces; every piece a run, then the same count from runs of 2 pieces
    check(tmp_path, vals([1, 2, 3], pieces), np.full(pieces, 3))
    ln = np.full((pieces + 1) // 2, 512 + 511, dtype=_U)
    if pieces % 2:
        ln[-1] = 511
    check(tmp_path, vals([8, 1], len(ln)), ln)


@pytest.mark.parametrize("n", [(1 << 12) - 2, (1 << 12) - 1, 1 << 12])
def test_low_width_borders(tmp_path, n):
    # all lengths 1: `intervals` has m = n ones in n + 1 positions, the logm == logn decrement of the sd_vector builder
    check(tmp_path, vals([1, 2], n), np.ones(n))


@pytest.mark.parametrize("width,node", [(12, 1), (32, (1 << 21) - 1), (33, 1 << 21), (63, (1 << 52) - 1), (64, (1 << 53) - 1)])
def test_item_widths(tmp_path, width, node):
    fmts = (COMPACT, BYTECODE) if node < 1 << 44 else (COMPACT,)
    n = 333  # 333 items: every alignment of an item of `width` bits to a word, straddling ones included
    v = vals([node, 1, max(node >> 1, 1)], n)
    check(tmp_path, v, np.full(n, 2), fmts)
    raw = host_bytes(tmp_path, v, np.full(n, 2), COMPACT)
    assert raw[8] == width
    check(tmp_path, [node << 11], [1], fmts)


def test_random(tmp_path):
    rng = np.random.default_rng(20)
    for case in range(200):
        n = int(rng.integers(1, 5001))
        kind = case % 4
        if kind == 0:
            ln = rng.integers(1, 4, n)
        elif kind == 1:
            ln = rng.integers(0, 1200, n)
        elif kind == 2:
            ln = rng.choice(np.array(BORDER_LENGTHS + (2, 3, 100)), n)
        else:
            ln = np.where(rng.random(n) < 0.01, rng.integers(0, 200000, n), rng.integers(0, 3, n))
        top = int(rng.choice([2, 1 << 9, 1 << 20, 1 << 43]))
        nodes = rng.integers(1, top + 1, int(rng.integers(1, 50)))
        check(tmp_path, vals(nodes, n), ln.astype(_U))


# ---- 3. long select superblocks
def test_long_superblocks_select_1(tmp_path):
    ln = np.array([1] * 2_000_000 + [511] * 4096 + [1] * 10, dtype=_U)
    v = vals([1, 2, 3], len(ln))
    s = compact_selects(host_bytes(tmp_path, v, ln, COMPACT))
    assert s[2][1] > 0 and s[2][2] >= 1  # intervals, select_1: a mini_or_long vector, long superblocks
    check(tmp_path, v, ln)


def test_long_superblocks_select_0(tmp_path):
    ln = np.array([511] * 70_000 + [1] * 300_000 + [511] * 10, dtype=_U)
    v = vals([1, 2, 3], len(ln))
    s = compact_selects(host_bytes(tmp_path, v, ln, COMPACT))
    assert s[3][1] > 0 and s[3][2] >= 1  # intervals, select_0
    check(tmp_path, v, ln)


# ---- 4. build_tags at its existing shapes
_shapes = {}


def _shape(workdir, name):
    if name not in _shapes:
        d = pathlib.Path(workdir) / "tags_encode_shapes"
        d.mkdir(exist_ok=True)
        if name == "six_hundred":
            _shapes[name] = (BT._identical(d, "six_hundred", 600, seq=b"ACGTTGCAGGATTC"),) + BT._one_node_each(600, 14) + (0,)
        elif name == "seventy_k":
            _shapes[name] = (BT._identical(d, "seventy_k", 70000),) + BT._one_node_each(70000, 8) + (0,)
        elif name == "wrap":
            ri = BT._identical(d, "wrap", 65536, extra=b"TTTTGGGGCC\n")
            _shapes[name] = (ri, np.arange(65538, dtype=_U), np.array([2] * 65536 + [4], dtype=_U), np.array([0, 8, 10], dtype=np.uint32), 0)
        elif name == "forward_xy":
            _shapes[name] = (os.path.join(G, "two_contig_graph", "xy.ri"),) + BT._tables(os.path.join(BTD, "xy.gbz"), forward_only=True)
        else:
            ri_x = os.path.join(workdir, "te_x.ri")
            P.build_rindex(os.path.join(G, "x.rl_bwt"), ri_x)
            _shapes[name] = (ri_x,) + BT._tables(os.path.join(G, "x.giraffe.gbz"), forward_only=True)
    return _shapes[name]


@pytest.mark.parametrize("name", ["six_hundred", "seventy_k", "wrap", "forward_xy", "forward_x"])
def test_build_tags_shapes(workdir, tmp_path, name):
    ri, po, pn, nl, fid = _shape(workdir, name)
    base = P.BUILD_TAGS_FORWARD_ONLY if name.startswith("forward") else 0
    for ref in (0, P.BUILD_TAGS_REFERENCE_RUNS):
        plain, conv, out = (str(tmp_path / n) for n in ("plain.tags", "conv.tags", "out.tags"))
        P.build_tags_paths(ri, po, pn, nl, fid, plain, flags=base | ref)
        for flag, compact in ((P.BUILD_TAGS_OUT_COMPACT, True), (P.BUILD_TAGS_OUT_BYTECODE, False)):
            P.convert_tags(plain, conv, compact=compact)
            ms = P.build_tags_paths(ri, po, pn, nl, fid, out, flags=base | ref | flag)
            assert first_difference(open(out, "rb").read(), open(conv, "rb").read()) is None, (name, ref, flag)
            assert set(ms) == set(P.BUILD_TAGS_STAGES)
            os.remove(out)


def test_build_tags_error_leaves_no_file(built, tmp_path):
    ri = os.path.join(BTD, "xy.ri")
    po, pn, nl, fid = BT._tables(os.path.join(BTD, "xy.gbz"))
    nl2 = nl.copy()
    nl2[(int(pn[int(po[4])]) >> 1) - fid] += 1  # a path's length differs from its sequence's (test_errors)
    out = str(tmp_path / "bad.tags")
    for flag in (P.BUILD_TAGS_OUT_COMPACT, P.BUILD_TAGS_OUT_BYTECODE):
        with pytest.raises(P.PgxError) as e:
            P.build_tags_paths(ri, po, pn, nl2, fid, out, flags=flag)
        assert e.value.code == P.ERR_FORMAT and "sequence 4" in str(e.value) and not os.path.exists(out)
    with pytest.raises(P.PgxError) as e:
        P.build_tags_paths(ri, po, pn, nl, fid, out, flags=P.BUILD_TAGS_OUT_COMPACT | P.BUILD_TAGS_OUT_BYTECODE)
    assert e.value.code == P.ERR_ARG and not os.path.exists(out)


# ---- 5. merge_tags
@pytest.mark.parametrize("table,name", [("files", "files_250"), ("long", "long_reference_runs")])
def test_merge_device_encode(workdir, tmp_path, table, name):
    c = M.build_case(workdir, table, name)
    for ref in (0, P.MERGE_REFERENCE_RUNS):
        host, dev = str(tmp_path / "host.tags"), str(tmp_path / "dev.tags")
        P.merge_tags(c.ri, c.tag_paths, c.seq_to_file, host, flags=ref)
        for rep in range(2):
            P.merge_tags(c.ri, c.tag_paths, c.seq_to_file, dev, flags=ref | P.MERGE_DEVICE_ENCODE)
            assert first_difference(open(dev, "rb").read(), open(host, "rb").read()) is None, (name, ref, rep)
            os.remove(dev)
    if table == "long":  # the case is about the mod-65 536 rule: the two modes differ, so both were checked
        a, b = str(tmp_path / "a.tags"), str(tmp_path / "b.tags")
        P.merge_tags(c.ri, c.tag_paths, c.seq_to_file, a, flags=P.MERGE_DEVICE_ENCODE)
        P.merge_tags(c.ri, c.tag_paths, c.seq_to_file, b, flags=P.MERGE_DEVICE_ENCODE | P.MERGE_REFERENCE_RUNS)
        assert open(a, "rb").read() != open(b, "rb").read()


def test_merge_through_the_graph_and_its_floor(built, tmp_path):
    gbz, ri = os.path.join(BTD, "xy.gbz"), os.path.join(BTD, "xy.ri")
    paths = []
    for c in ("x", "y"):
        out = str(tmp_path / ("%s.tags" % c))
        P.build_tags(os.path.join(BTD, "%s.gbz" % c), os.path.join(BTD, "contigs_%s.rl_bwt" % c), out, flags=P.BUILD_TAGS_INPUT_RLBWT)
        paths.append(out)
    # the same streams with every node replaced by the smallest of its component: the graph's largest id (the floor of the item
    # width) then lies above every node of the tags
    first, comp, mx, nc = P.gbz_paths(gbz)
    low = []
    for f, p in enumerate(paths):
        v, ln = E.decode(open(p, "rb").read())
        node = int(first[comp == comp[[1, 5][f]]].min())
        assert node.bit_length() < int(mx).bit_length()
        out = str(tmp_path / ("%s_low.tags" % "xy"[f]))
        with open(out, "wb") as fh:
            fh.write(E.encode((v & _U(0x7FF)) | _U(node << 11), ln))
        low.append(out)
    for files in (paths, low):
        for ref in (0, P.MERGE_REFERENCE_RUNS):
            host, dev = str(tmp_path / "host.tags"), str(tmp_path / "dev.tags")
            P.merge_tags_gbz(gbz, ri, files, host, flags=ref)
            P.merge_tags_gbz(gbz, ri, files, dev, flags=ref | P.MERGE_DEVICE_ENCODE)
            got = open(dev, "rb").read()
            assert first_difference(got, open(host, "rb").read()) is None, (files is low, ref)
            assert got[8] == 11 + int(mx).bit_length()
    # the CLI's switch
    cli = str(tmp_path / "cli.tags")
    d = str(tmp_path / "dir")
    os.makedirs(d)
    for p in paths:
        os.link(p, os.path.join(d, os.path.basename(p)))
    r = BT._run("merge_tags", gbz, ri, d, "--out", cli, "--device-encode")
    assert r.returncode == 0, r.stderr
    P.merge_tags_gbz(gbz, ri, paths, host)
    assert open(cli, "rb").read() == open(host, "rb").read()


def test_merge_flags_still_refused(workdir, tmp_path):
    c = M.build_case(workdir, "files", "idle_file_bare")
    out = str(tmp_path / "refused.tags")
    for flags in (2, 4, 8, 2 | P.MERGE_DEVICE_ENCODE, 0x20, P.MERGE_REFERENCE_RUNS | 4):
        with pytest.raises(P.PgxError) as e:
            P.merge_tags(c.ri, c.tag_paths, c.seq_to_file, out, flags=flags)
        assert e.value.code == P.ERR_ARG and "unknown flag" in str(e.value) and not os.path.exists(out)
