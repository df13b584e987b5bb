"""GPU tier of pgx_read_pack_arrays at its borders: the pack kernels on the stated tables of tests/pack_cases.py against tests/pack_emu.py, which
counts base by base -- the node table, the coverage vector, the per-node summary and the three counters, byte for byte.

The shapes are the smallest that can go wrong: intervals that start and end on every bit residue around a 64-bit word border and a 512-position
directory border of the WALK image; intervals that end one before, on and one behind a tile border of the fold (PGX_SCAN_BLOCK_ITEMS = 2048) in
collections of 2047, 2048, 2049 and 3 x 2048 + 1 positions; visits of 1, 2, 1023 and 1024 symbols in both orientations; a node visited by several
sequences in both orientations; an interval that ends on its sequence's last position next to one that starts on the next sequence's first;
empty sequences, reads without a candidate, keep = 0; every kind of CIGAR; 70 000 reads on one base; ids with gaps and max_id = 2^20; two
visits of one id with different lengths; an id of 2^32 - 1; every PGX_ERR_ARG, null arguments among them, with the outputs untouched."""
import numpy as np
import pytest

import pack_cases as C
import pack_emu as E
import pgx_ffi as P

pytestmark = pytest.mark.gpu


def _emu(c, **kw):
    return E.read_pack(c["visit_offsets"], c["visit_nodes"], c["visit_length"], c["seq"], c["text_start"], c["op_offsets"], c["ops"], keep=c["keep"], **kw)


def _gpu(c, **kw):
    return P.read_pack_arrays(0, c["seq_offsets"], c["visit_offsets"], c["visit_nodes"], c["visit_length"], c["seq"], c["text_start"], c["op_offsets"], c["ops"], c["keep"], **kw)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_the_stated_tables_equal_the_emulator(name):
    c = C.CASES[name]()
    exp = _emu(c)
    got = _gpu(c)
    E.same(got, exp)
    assert int(got["cov"].astype(np.uint64).sum()) == exp["bases_added"]  # (no base wraps here)
    if name == "deep":
        assert got["max"].max() == 70000 and got["reads_counted"] == 70000
    if name == "gaps":
        assert got["n_nodes"] == (1 << 20) + 1 and got["n_bases"] == 11 and np.count_nonzero(got["node_length"]) == 3
    if name == "sequence_ends":
        assert got["reads_filtered"] == 2 and got["reads_counted"] == 6  # (keep = 0 on a read whose operations consume no text filters nothing)
    if name.startswith("tile_"):
        assert got["cov"].min() >= 1 and got["cov"].max() >= 3  # (one read spans the whole collection)


def test_the_order_of_the_reads_and_an_all_ones_keep_change_nothing():
    c = C.cigars()
    exp = _gpu(c)
    n = len(c["seq"])
    order = np.random.default_rng(5).permutation(n)
    lens = np.diff(c["op_offsets"].astype(np.int64))
    ops = np.concatenate([c["ops"][int(c["op_offsets"][r]):int(c["op_offsets"][r + 1])] for r in order])
    d = dict(c, seq=c["seq"][order], text_start=c["text_start"][order], op_offsets=np.concatenate(([0], np.cumsum(lens[order]))).astype(np.uint64), ops=ops, keep=np.ones(n, np.uint8))
    E.same(_gpu(d), exp)


def test_two_lengths_of_one_node_are_a_format_error_naming_the_smallest():
    c = C.two_lengths()
    with pytest.raises(E.FormatError) as want:
        _emu(c)
    assert want.value.node == 4
    with pytest.raises(P.PgxError) as e:
        _gpu(c)
    assert e.value.code == P.ERR_FORMAT and "do not describe whole-node paths" in str(e.value) and "node 4 " in str(e.value), str(e.value)


def test_an_id_the_dense_table_cannot_hold_is_unsupported():
    c = C.make([[(((1 << 32) - 1) << 1, 3)]], [(0, 0, [(C.EQ, 3)])])
    with pytest.raises(P.PgxError) as e:
        _gpu(c, nodes_cap=0, cov_cap=3)  # (refused behind the max id pass, before any table is sized)
    assert e.value.code == P.ERR_UNSUPPORTED and "the largest node id is 4294967295" in str(e.value), str(e.value)
    fits = C.make([[(5 << 1, 3)]], [(0, 0, [(C.EQ, 3)])])
    E.same(_gpu(fits), _emu(fits))


def test_null_arguments_are_refused():
    import ctypes

    c = C.cigars()
    n, n_seq = len(c["seq"]), len(c["seq_offsets"]) - 1
    nn, nb = ctypes.c_uint64(7), ctypes.c_uint64(7)
    base, counters = np.zeros(64, np.uint64), np.full(3, 9, np.uint64)
    length, covered, most, total, cov = np.zeros(64, np.uint32), np.zeros(64, np.uint32), np.zeros(64, np.uint32), np.zeros(64, np.uint64), np.zeros(256, np.uint32)
    ptr = lambda a: a.ctypes.data
    good = [0, ptr(c["seq_offsets"]), n_seq, ptr(c["visit_offsets"]), ptr(c["visit_nodes"]), ptr(c["visit_length"]), n, ptr(c["seq"]), ptr(c["text_start"]), ptr(c["op_offsets"]),
            ptr(c["ops"]), None, ctypes.addressof(nn), ctypes.addressof(nb), ptr(base), ptr(length), ptr(covered), ptr(total), ptr(most), 63, ptr(cov), 256, ptr(counters)]
    L = P.lib()
    for k in (1, 3, 4, 5, 7, 8, 9, 10, 12, 13, 14, 15, 16, 17, 18, 20, 22):  # every pointer but keep, one at a time
        args = list(good)
        args[k] = None
        assert L.pgx_read_pack_arrays(*args) == P.ERR_ARG, k
        assert "null argument" in L.pgx_last_error().decode(), k
    assert (nn.value, nb.value) == (7, 7) and counters.tolist() == [9, 9, 9]
    assert L.pgx_read_pack_arrays(*good) == P.OK and (nn.value, nb.value) == (27, 100)


def test_capacities_are_checked_with_the_needed_counts():
    c = C.gaps()
    for kw in (dict(nodes_cap=1 << 20), dict(cov_cap=10)):
        with pytest.raises(P.PgxError) as e:
            _gpu(c, **kw)
        assert e.value.code == P.ERR_NOMEM and "1048577 nodes and 11 graph bases" in str(e.value), str(e.value)
    E.same(_gpu(c, nodes_cap=(1 << 20) + 1, cov_cap=11), _emu(c))


def _untouched(c, code=P.ERR_ARG):
    """the call is refused with `code` and writes nothing"""
    fill = dict(node_base=np.full(64, 0xA5A5A5A5A5A5A5A5, np.uint64), node_length=np.full(64, 0xA5A5A5A5, np.uint32), covered=np.full(64, 0xA5A5A5A5, np.uint32),
                sum=np.full(64, 0xA5A5A5A5A5A5A5A5, np.uint64), max=np.full(64, 0xA5A5A5A5, np.uint32), cov=np.full(256, 0xA5A5A5A5, np.uint32),
                counters=np.full(3, 0xA5A5A5A5A5A5A5A5, np.uint64))
    before = {k: v.copy() for k, v in fill.items()}
    with pytest.raises(P.PgxError) as e:
        _gpu(c, nodes_cap=63, cov_cap=256, out=fill)
    assert e.value.code == code, str(e.value)
    for k in fill:
        assert fill[k].tobytes() == before[k].tobytes(), k
    return str(e.value)


def test_every_refused_argument_leaves_the_outputs_untouched():
    base = C.make([[(2, 4), (4, 6)], [(6, 3)]], [(0, 1, [(C.EQ, 5)]), (1, 0, [(C.EQ, 3)])])
    E.same(_gpu(base), _emu(base))
    bad_op = dict(base, ops=np.array([(5 << 4) | 3, (3 << 4) | C.EQ], np.uint32))
    assert "operation 0 of read 0 has the code 3" in _untouched(bad_op)
    assert "read 1 names a sequence" in _untouched(dict(base, seq=np.array([0, 2], np.uint32)))
    assert "read 1 starts at 4" in _untouched(dict(base, text_start=np.array([1, 4], np.uint64)))
    assert "the CIGAR of read 0 consumes 5 symbols of text from 6" in _untouched(dict(base, text_start=np.array([6, 0], np.uint64)))
    long_d = dict(base, ops=np.array([(3 << 4) | C.EQ, (8 << 4) | C.D], np.uint32), op_offsets=np.array([0, 2, 2], np.uint64))
    assert "the CIGAR of read 0 consumes 11" in _untouched(long_d)
    assert "op_offsets decrease at read 1" in _untouched(dict(base, op_offsets=np.array([0, 2, 1], np.uint64)))
    assert "op_offsets must start at 0" in _untouched(dict(base, op_offsets=np.array([1, 1, 2], np.uint64)))
    # the tables: what pgx_read_walk_arrays refuses
    assert "has length 0" in _untouched(dict(base, visit_length=np.array([4, 0, 3], np.uint32)))
    assert "has length 1025" in _untouched(dict(base, visit_length=np.array([4, 1025, 3], np.uint32)))
    assert "the visits of sequence 0 sum to 9" in _untouched(dict(base, visit_length=np.array([4, 5, 3], np.uint32)))
    assert "visit_offsets decrease" in _untouched(dict(base, visit_offsets=np.array([0, 3, 2], np.uint64)))
    assert "seq_offsets must start at 0" in _untouched(dict(base, seq_offsets=np.array([1, 10, 13], np.uint64)))
    # a read without a sequence may carry anything but an unknown code
    free = dict(base, seq=np.array([E.NO_SEQUENCE, 1], np.uint32), text_start=np.array([99, 0], np.uint64))
    E.same(_gpu(free), _emu(free))
