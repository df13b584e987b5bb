"""build_tags on the GPU at its borders (build_tags_cases.py; test_build_tags_cases.py shows on the CPU that the tables hold what they claim):
for every case and both run modes the file pgx_build_tags_paths writes is byte-equal to gbz_graph_emu.encode of the truth from the oracle's
suffix array, and the two query formats encoded on the device are byte-equal to the host's convert_tags of that file.  Then the node id
that no longer fits a piece: refused, no file, and the next call is served."""
import os

import numpy as np
import pytest

import build_tags_cases as B
import gbz_graph_emu as E
import pgx_ffi as P
from test_gpu_tags_encode import first_difference

pytestmark = pytest.mark.gpu

_cases = {}


def _case(workdir, table, name):
    if (table, name) not in _cases:
        _cases[table, name] = B.build_case(workdir, table, name)
    return _cases[table, name]


def _build(c, out, flags):
    if os.path.exists(out):
        os.remove(out)
    P.build_tags_paths(c.ri, c.path_offsets, c.path_nodes, c.node_length, c.first_node_id, out, flags=flags)
    return open(out, "rb").read()


def _check(workdir, c):
    d = os.path.join(workdir, "build_tags_borders")
    os.makedirs(d, exist_ok=True)
    plain, conv, out = (os.path.join(d, "%s.%s.tags" % (c.name, k)) for k in ("plain", "conv", "out"))
    files = {}
    for ref in (0, B.REFERENCE_RUNS):
        want = E.encode(c.ref_values, c.ref_lengths) if ref else E.encode(c.values, c.lengths)
        got = _build(c, plain, ref)
        assert first_difference(got, want) is None, (c.name, ref, first_difference(got, want))
        files[ref] = got
        for flag, compact in ((P.BUILD_TAGS_OUT_COMPACT, True), (P.BUILD_TAGS_OUT_BYTECODE, False)):
            P.convert_tags(plain, conv, compact=compact)
            host = open(conv, "rb").read()
            dev = _build(c, out, ref | flag)
            assert first_difference(dev, host) is None, (c.name, ref, flag, first_difference(dev, host))
    assert (files[0] != files[B.REFERENCE_RUNS]) == bool(c.flags & B.REFERENCE_RUNS)
    for p in (plain, conv, out):
        os.remove(p)
    return files[0]


@pytest.mark.parametrize("name", list(B.DIRECTORY_CASES))
def test_directory_borders(workdir, name):
    _check(workdir, _case(workdir, "directory", name))


@pytest.mark.parametrize("name", list(B.RUN_CASES))
def test_run_length_borders(workdir, name):
    _check(workdir, _case(workdir, "runs", name))


@pytest.mark.parametrize("name", list(B.NODE_ID_CASES))
def test_node_id_borders(workdir, name):
    c = _case(workdir, "node_ids", name)
    raw = _check(workdir, c)
    # 16 pieces of one row, four a node, of the byte counts the table names
    body = int(np.frombuffer(raw[:8], dtype=np.uint64)[0]) // 8
    assert body == sum(B.piece_bytes(int(v), 1) for v in c.values) and 16 * min(c.claims["bytes"]) <= body <= 16 * max(c.claims["bytes"])


@pytest.mark.parametrize("name", list(B.SIZE_CASES))
def test_size_borders(workdir, name):
    _check(workdir, _case(workdir, "sizes", name))


def test_refused_node_id(workdir):
    """node id 2^44 does not fit a piece (node << 20 in 64 bits): PGX_ERR_FORMAT that names the id, no file, and a good call afterwards"""
    good = _case(workdir, "node_ids", "ids_up_to_2_44")
    po, pn, nl = B.node_id_graph(B.REFUSED_FIRST)
    assert int(pn.max()) >> 1 == B.REFUSED_ID and int(pn.min()) >> 1 == B.REFUSED_FIRST
    out = os.path.join(workdir, "build_tags_refused.tags")
    for flags in (0, B.REFERENCE_RUNS, P.BUILD_TAGS_OUT_COMPACT, P.BUILD_TAGS_OUT_BYTECODE):
        with pytest.raises(P.PgxError) as e:
            P.build_tags_paths(good.ri, po, pn, nl, B.REFUSED_FIRST, out, flags=flags)
        assert e.value.code == P.ERR_FORMAT, str(e.value)
        assert str(B.REFUSED_ID) in str(e.value) and "44 bits" in str(e.value), str(e.value)
        assert not os.path.exists(out)
        _check(workdir, good)
