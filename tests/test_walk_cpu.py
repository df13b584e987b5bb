"""CPU tier of the read walk: tests/walk_emu.py (the definitions of include/pgx.h "read walk" as plain loops) against cases worked out by hand,
its marks-from-tags against the path tables of the `directory` table of tests/build_tags_cases.py with the naively stated row tags, the GAF
line against one written out by hand, and the ABI: the record's layout, the exported symbols, the version that stays, no CPU fallback."""
import ctypes
import re

import numpy as np
import pytest

import __graft_entry__ as G
import build_tags_cases as B
import pgx_ffi as P
import walk_emu as E

ENTRY_POINTS = ("pgx_batch_read_walk", "pgx_batch_walked", "pgx_batch_device_walked", "pgx_index_paths", "pgx_read_walk_arrays")
A, Bn, Cn, L = (5 << 1), (6 << 1) | 1, (7 << 1), (9 << 1) | 1  # nodes as id << 1 | rev


def test_stretches_by_hand():
    nodes, lens = [A, Bn, Cn], [4, 3, 5]  # A = [0, 4), B = [4, 7), C = [7, 12)
    assert E.walk(nodes, lens, 5, 6) == (3, 1, 2, [Bn])                # inside one node
    assert E.walk(nodes, lens, 2, 7) == (7, 2, 7, [A, Bn])             # ends on a node's last symbol: the next node is no step
    assert E.walk(nodes, lens, 4, 8) == (8, 0, 4, [Bn, Cn])            # starts on a node's first symbol: the node before is no step
    assert E.walk(nodes, lens, 0, 12) == (12, 0, 12, [A, Bn, Cn])      # the whole sequence
    assert E.walk(nodes, lens, 11, 12) == (5, 4, 5, [Cn])              # the last symbol
    assert E.walk(nodes, lens, 3, 3) == (0, 0, 0, [])                  # an empty stretch
    loop, llen = [A, L, L, L, Cn], [3, 1, 1, 1, 2]                      # a self-loop on a 1-bp node, taken three times
    assert E.walk(loop, llen, 2, 6) == (6, 2, 6, [A, L, L, L])
    assert E.walk(loop, llen, 4, 5) == (1, 0, 1, [L])
    assert E.walk(loop, llen, 3, 7) == (5, 0, 4, [L, L, L, Cn])
    assert E.walk([A, A], [4, 4], 3, 5) == (8, 3, 5, [A, A])           # a node visited twice in a row
    assert E.walk([A, A], [4, 4], 4, 8) == (4, 0, 4, [A])


def test_read_walk_records_and_list():
    po, pn, vl = np.array([0, 3, 3, 5], np.uint64), np.array([A, Bn, Cn, A, A], np.uint64), np.array([4, 3, 5, 4, 4], np.uint32)
    res = E.read_walk(po, pn, vl, [0, E.NO_SEQUENCE, 2, 0, 1], [5, 0, 3, 3, 0], [6, 0, 5, 3, 0])
    assert res["reads"].tolist() == [(3, 1, 2, 1, 0), (0, 0, 0, 0, E.NO_SEQUENCE), (8, 3, 5, 2, 2), (0, 0, 0, 0, 0), (0, 0, 0, 0, 1)]
    assert res["step_offsets"].tolist() == [0, 1, 1, 3, 3, 3] and res["steps"].tolist() == [Bn, A, A]
    bare = E.read_walk(po, pn, vl, [0], [5], [6], flags=0)
    assert bare["step_offsets"] is None and bare["steps"] is None and bare["reads"].tolist() == [(3, 1, 2, 1, 0)]


def test_gaf_line_by_hand():
    align = dict(clip_lo=2, clip_hi=1, n_match=9, n_mismatch=1, n_ins=0, n_del=1, edits=2, seq=3, text_start=40)
    wrec = dict(path_len=15, path_start=4, path_end=15, n_steps=2)
    ops = [(2 << 4) | 4, (5 << 4) | 7, (1 << 4) | 2, (1 << 4) | 8, (4 << 4) | 7, (1 << 4) | 4]
    assert E.gaf_line(7, 13, align, wrec, [A, Bn], ops) == "7\t13\t2\t12\t+\t>5<6\t15\t4\t15\t9\t11\t255\tNM:i:2\ths:i:3\tho:i:40\tcg:Z:5=1D1X4="
    assert E.gaf_line(8, 13, align, dict(wrec, n_steps=0), [], []) == "8\t13\t*\t*\t*\t*\t*\t*\t*\t*\t*\t255"


def test_marks_from_tags_are_the_path_table(workdir):
    """on the collection that holds every border of build_tags' directory: the positions whose naively stated row tag has offset 0, cut into
    visits, are the case's path table with the node lengths -- so Index.paths() has a truth that no bit vector made"""
    c = B.build_case(workdir, "directory", "directory")
    tags = B.naive_row_tags(c)
    seq_len = [ln for _, ln in B.node_starts(c)]
    marks = E.marks_from_row_tags(c.sa, tags, c.n_seq, c.ml)
    po, pn, vl = E.visits_from_marks(marks, seq_len)
    assert np.array_equal(po, c.path_offsets) and np.array_equal(pn, c.path_nodes)
    assert np.array_equal(vl, c.node_length[(c.path_nodes >> np.uint64(1)).astype(np.int64) - c.first_node_id])
    assert [[off for off, _ in m] for m in marks] == [st for st, _ in B.node_starts(c)]
    assert int(vl.max()) == 1024 and int(vl.min()) == 1 and sum(1 for m in marks if not m) == 3


def test_record_layout_and_symbols(built):
    d = P.WALK_DTYPE
    assert d.itemsize == 32 and d == E.WALK_DTYPE and P.WALK_STEPS == E.WALK_STEPS == 1
    assert {n: d.fields[n][1] for n in d.names} == dict(path_len=0, path_start=8, path_end=16, n_steps=24, seq=28)
    with open(G.os.path.join(G.ROOT, "include", "pgx.h")) as f:
        header = f.read()
    assert re.search(r"uint64_t\s+path_len,\s*path_start,\s*path_end;\s*uint32_t\s+n_steps,\s*seq;\s*\}\s*pgx_read_walk;", header)
    assert ctypes.sizeof(P.ReadWalks) == 56
    assert {n: getattr(P.ReadWalks, n).offset for n, _ in P.ReadWalks._fields_} == dict(n_reads=0, n_steps=8, flags=16, reserved=20, reads=24, step_offsets=32, steps=40,
                                                                                       ms_walk=48, reserved2=52)
    lib = P.lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert lib.pgx_abi_version() == 7 == G.header_abi_version()


def test_no_device(built):
    try:
        no_gpu = P.device_count() == 0
    except P.PgxError as e:
        no_gpu = e.code == P.ERR_NO_DEVICE
    if not no_gpu:
        pytest.skip("a GPU is present")
    lib = P.lib()
    assert lib.pgx_batch_read_walk(None, 0, None) == P.ERR_NO_DEVICE
    with pytest.raises(P.PgxError) as e:
        P.read_walk_arrays(0, [0, 4], [0, 1], [A], [4], [0], [1], [3], flags=P.WALK_STEPS)
    assert e.value.code == P.ERR_NO_DEVICE
    out = P.ReadWalks()
    assert lib.pgx_batch_walked(None, ctypes.byref(out)) == P.ERR_ARG
    assert lib.pgx_batch_device_walked(None, ctypes.byref(out)) == P.ERR_ARG
