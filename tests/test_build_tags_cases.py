"""CPU tier of the build_tags case tables (build_tags_cases.py; the GPU tier is test_gpu_build_tags_borders.py): every table holds the borders
its line claims, by number, in the truth the GPU tier compares with (the oracle's suffix array of the CPU-built index, then
gbz_graph_emu.row_tags -> runs -> encode).  row_tags is pinned once, on the directory case, to a naive walk of every row's path, and
reference_runs on the 65 535 / 65 536 / 65 537 cases to the reference's uint16_t loop restated."""
import numpy as np
import pytest

import build_tags_cases as B
import gbz_graph_emu as E

_cases = {}


@pytest.fixture
def case(request, workdir):
    """the case of the test's (table, name) parameter, built once a session"""
    key = request.param
    if key not in _cases:
        _cases[key] = B.build_case(workdir, *key)
    return _cases[key]


def _of(table):
    return dict(argnames="case", argvalues=[(table, n) for n in B.TABLES[table][0]], ids=list(B.TABLES[table][0]), indirect=True)


ALL = dict(argnames="case", argvalues=B.ALL_CASES, ids=[n for _, n in B.ALL_CASES], indirect=True)


def test_the_tables_hold_every_case_the_tiers_run():
    assert len(B.ALL_CASES) == len({n for _, n in B.ALL_CASES}) == 1 + 4 + 8 + 20
    assert B.BORDERS == (255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097) and B.SCAN_TILE == 4096
    assert [k["first"] for k in B.NODE_ID_CASES.values()] == [1] + [(1 << k) - 2 for k in (8, 15, 22, 29, 36, 43)] + [(1 << 44) - 4]
    assert B.REFUSED_FIRST + 3 == B.REFUSED_ID == 1 << 44
    assert B.GROUP_LENGTHS == (1, 2, 510, 511, 512, 1021, 1022, 1023, 1533) and B.WRAP_LENGTHS == (65535, 65536, 65537)


@pytest.mark.parametrize(**ALL)
def test_graph_and_truth_fit_together(case):
    c = case
    assert c.n == len(c.sa) == len(c.tags) and c.n_seq == len(c.path_offsets) - 1 and int(c.path_offsets[-1]) == len(c.path_nodes)
    # every path spells its sequence's length, no node is empty or longer than 1024 bp, both orientations occur
    seq_lens = [len(s) for s in c.text.split(b"\n")[:-1]]
    assert [ln for _, ln in B.node_starts(c)] == seq_lens
    used = c.node_length[(c.path_nodes >> np.uint64(1)).astype(np.int64) - c.first_node_id]
    assert used.min() >= 1 and used.max() <= B.BUCKET
    assert set((c.path_nodes & np.uint64(1)).tolist()) == {0, 1}
    assert int(c.path_nodes.min()) >> 1 >= max(c.first_node_id, 1) and int(c.path_nodes.max()) >> 1 < 1 << B.ID_BITS
    # the truth: no tag on the endmarker rows, one on every other row; runs and pieces cover exactly those rows
    assert not c.tags[:c.n_seq].any() and c.tags[c.n_seq:].all()
    assert int(c.lengths.sum()) == c.n - c.n_seq and (c.values[1:] != c.values[:-1]).all()
    p = B.pieces(c.values, c.lengths)
    assert sum(ln for _, ln in p) == c.n - c.n_seq and max(ln for _, ln in p) <= B.MAX_PIECE
    dv, dl = E.decode(E.encode(c.values, c.lengths))
    assert list(zip(dv.tolist(), dl.tolist())) == p
    assert len(E.encode(c.values, c.lengths)) == 8 + -(-sum(B.piece_bytes(v, ln) for v, ln in p) // 8) * 8
    # the two run modes differ exactly where a case says so
    differ = len(c.ref_lengths) != len(c.lengths) or not np.array_equal(c.ref_lengths, c.lengths)
    assert differ == bool(c.flags & B.REFERENCE_RUNS)


# ---- 1. the directory
@pytest.mark.parametrize(**_of("directory"))
def test_row_tags_is_the_naive_walk(case):
    assert np.array_equal(B.naive_row_tags(case), case.tags)


@pytest.mark.parametrize(**_of("directory"))
def test_directory_case(case):
    c = case
    layout = B.node_starts(c)
    seq_lens = [ln for _, ln in layout]
    assert set(B.DIRECTORY_LENGTHS) <= set(seq_lens) and max(seq_lens) == 6145
    assert seq_lens[0] == 0 and seq_lens[-1] == 0 and 0 in seq_lens[1:-1] and c.text.startswith(b"\n") and c.text.endswith(b"\n\n")
    assert c.n == 23555 + len(seq_lens) and c.n_seq == len(seq_lens) == 14
    assert c.node_length[0] == 0 and (c.node_length == 0).sum() == len(B.DIRECTORY_HOLES)  # ids without a sequence, id 1 among them

    def length(s, j):
        return int(c.node_length[(int(c.path_nodes[int(c.path_offsets[s]) + j]) >> 1) - c.first_node_id])

    starts = {(st, length(s, j)) for s, (sts, _) in enumerate(layout) for j, st in enumerate(sts)}
    for k in (1, 2, 3, 5):
        assert any(st == B.BUCKET * k - 1 for st, _ in starts), k
        assert any(st == B.BUCKET * k for st, _ in starts), k
    for k in (1, 2, 5):
        assert any(st == B.BUCKET * k + 1 for st, _ in starts), k
    assert (1, 1024) in starts                                     # a 1024-bp node from offset 1: position 1024 is its offset 1023
    assert (1023, 1024) in starts and (3071, 1024) in starts       # ... and from 1024 k - 1: it covers the whole bucket but one position
    # buckets with 1024 node starts; one of them directly behind a 1024-bp node
    full = [(s, b) for s, (sts, ln) in enumerate(layout) for b in range(-(-ln // B.BUCKET))
            if sum(1 for st in sts if st // B.BUCKET == b) == B.BUCKET]
    assert len(full) == 2
    assert any(b >= 1 and (B.BUCKET * (b - 1), 1024) in {(st, length(s, j)) for j, st in enumerate(layout[s][0])} for s, b in full)
    # a 1024-bp node as the last of its sequence, with and without a one-bp node behind the bucket border
    last = {(seq_lens[s], length(s, len(sts) - 1)) for s, (sts, _) in enumerate(layout) if sts}
    assert {(1024, 1024), (2047, 1024), (2048, 1024), (2049, 1024), (3072, 1024), (6145, 1024), (1025, 1), (4096, 1)} <= last
    # in the truth: in-node offsets 0 and 1023 on both orientations, every row a run of its own
    seen = {(int(t) >> 10 & 1, int(t) & 0x3FF) for t in c.tags[c.n_seq:]}
    assert {(0, 0), (0, 1023), (1, 0), (1, 1023)} <= seen
    assert len(c.values) == c.n - c.n_seq == 23555 and set(c.lengths.tolist()) == {1}
    # position 1024 of the sequence whose 1024-bp node starts at offset 1 is that node's offset 1023
    s = seq_lens.index(6145)
    row = int(np.flatnonzero(c.sa == s * c.ml + 1024)[0])
    assert int(c.tags[row]) & 0x3FF == 1023 and int(c.tags[row]) >> 11 == int(c.path_nodes[int(c.path_offsets[s]) + 1]) >> 1


# ---- 2. run lengths
@pytest.mark.parametrize(**_of("runs"))
def test_run_length_cases(case):
    c = case
    lens = set(c.lengths.tolist())
    last_piece = B.pieces(c.values, c.lengths)[-1][1]
    if c.name == "pieces":
        assert lens == set(B.GROUP_LENGTHS) and c.n == 42946 and c.n_seq == sum(B.GROUP_LENGTHS) + 1 and len(c.values) == 6 * 9
        assert b"\n\n" in c.text
        assert {ln for _, ln in B.pieces(c.values, c.lengths)} == {1, 2, 510, 511, 1021 - 511, 1533 - 2 * 511}
        # the two statements of the piece rule, on every length of the table: (len + 510) / 511 pieces, the last of len - 511 (pieces - 1)
        for ln in B.GROUP_LENGTHS:
            p = [x for _, x in B.pieces(np.array([5 << 11], dtype=np.uint64), np.array([ln], dtype=np.uint64))]
            assert len(p) == (ln + 510) // 511 and p[-1] == ln - 511 * (len(p) - 1) and set(p[:-1]) <= {511}
    elif c.name == "ends_in_long_run":
        assert int(c.lengths[-1]) == 512 and last_piece == 1 and lens == {1, 3, 512, 600}
        assert int(c.values[-1]) == (4 << 11) | (1 << 10)  # offset 0 of the TTTT node
        assert c.n == 3 * 7 + 600 * 5 + 5 + 512 * 5 + 1 and b"\n\n" in c.text
    elif c.name == "wrap":
        assert lens == set(B.WRAP_LENGTHS) and c.n == 983041 and len(c.values) == 12
        assert sorted(c.ref_lengths.tolist()) == [1] * 4 + [65535] * 4 and len(c.ref_values) == 8
        # a run that vanishes between two that stay
        i = np.flatnonzero(c.lengths == 65536)
        assert any(0 < k < len(c.lengths) - 1 and c.lengths[k - 1] != 65536 and c.lengths[k + 1] != 65536 for k in i)
    else:
        assert lens == {1, 65536} and c.n == 4 * 65538 and len(c.values) == 9
        assert len(c.ref_values) == 6 and set(c.ref_lengths.tolist()) == {1}
        same = np.flatnonzero(c.ref_values[1:] == c.ref_values[:-1])
        assert len(same) == 2 and {int(c.ref_values[k]) for k in same} == {1 << 11, (1 << 11) | 1}  # offsets 0 and 1 of the shared node
    if c.flags & B.REFERENCE_RUNS:
        lv, ll = E.reference_uint16_loop(c.tags, c.n_seq)
        assert np.array_equal(lv, c.ref_values) and np.array_equal(ll, c.ref_lengths)


# ---- 3. node ids
@pytest.mark.parametrize(**_of("node_ids"))
def test_node_id_cases(case):
    c = case
    k = B.NODE_ID_CASES[c.name]
    assert c.n == 17 and c.n_seq == 1 and len(c.values) == 16 and set(c.lengths.tolist()) == {1}
    ids = sorted({int(v) >> 11 for v in c.values})
    assert ids == list(range(k["first"], k["first"] + 4)) and c.first_node_id == k["first"]
    by_id = {i: {B.piece_bytes(int(v), 1) for v in c.values if int(v) >> 11 == i} for i in ids}
    assert all(len(b) == 1 for b in by_id.values())
    assert tuple(sorted(set.union(*by_id.values()))) == k["bytes"] == c.claims["bytes"]
    if len(k["bytes"]) == 2:  # the border lies between two neighbouring ids, at a power of two
        border = min(i for i in ids if by_id[i] == {k["bytes"][1]})
        assert by_id[border - 1] == {k["bytes"][0]} and border & (border - 1) == 0 and border in (2, *(1 << b for b in B.ID_BORDERS))
    else:
        assert ids[-1] == (1 << 44) - 1
    # the file's ByteCodes have these byte counts: the body is their sum
    raw = E.encode(c.values, c.lengths)
    assert int(np.frombuffer(raw[:8], dtype=np.uint64)[0]) == 8 * sum(4 * next(iter(by_id[i])) for i in ids)
    assert {(int(v) >> 10) & 1 for v in c.values} == {0, 1}


def test_refused_id_is_one_past_the_largest():
    po, pn, nl = B.node_id_graph(B.REFUSED_FIRST)
    ids = sorted({int(v) >> 1 for v in pn})
    assert ids[-1] == B.REFUSED_ID == 1 << 44 and ids[-2] == (1 << 44) - 1
    assert (ids[-1] << 20) >= 1 << 64 > (ids[-2] << 20) + (511 << 11) + 0x7FF  # node << 20 no longer fits 64 bits


# ---- 4. sizes
@pytest.mark.parametrize(**_of("sizes"))
def test_size_cases(case):
    c = case
    k = B.SIZE_CASES[c.name]
    assert c.n_seq == k["n_seq"] and (c.node_length == 1).all()
    R = len(c.values)
    if k["twice"]:
        assert R == k["m"] and c.n - c.n_seq == 2 * R and set(c.lengths.tolist()) == {2} and int(c.lengths[-1]) == 2
    else:
        assert R == c.n - c.n_seq == k["m"] and set(c.lengths.tolist()) == {1}
    if c.name.startswith(("runs_", "twice_")):
        assert R in B.BORDERS
    if c.name.startswith("seqs_"):
        empty = sum(1 for s in c.text.split(b"\n")[:-1] if not s)
        assert c.n_seq in (255, 256, 257) and c.n == 600 + c.n_seq and empty > 20
    if c.name.startswith("rows_"):
        assert c.n in (2048, 4096) and c.n == int(c.name.split("_")[1])


def test_size_table_covers_every_border():
    runs = {k["m"] for k in B.SIZE_CASES.values() if not k["twice"] and k["n_seq"] == 3}
    assert runs == set(B.BORDERS)
    assert {k["n_seq"] for n, k in B.SIZE_CASES.items() if n.startswith("seqs_")} == {255, 256, 257}
    assert {k["m"] + k["n_seq"] for n, k in B.SIZE_CASES.items() if n.startswith("rows_")} == {2048, 4096}
    assert {k["m"] for k in B.SIZE_CASES.values() if k["twice"]} == {255, 256, 257, 2048, 4096, 4097}
