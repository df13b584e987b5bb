"""CPU tier of the merge_tags case tables (merge_cases.py; the GPU tier is test_gpu_merge_borders.py): every table holds the borders it claims,
the suffix arrays the expectations are built on are the order rule's (a naive sorted() over the suffixes, up to 4097 rows), and the reference's
sequential procedure (test_merge_tags._sequential_merge) over a case's streams and map gives the case's expectation."""
import numpy as np
import pytest

import build_device_cases as BC
import merge_cases as M
from test_merge_tags import _sequential_merge

_cases = {}


@pytest.fixture
def case(request, workdir):
    """the case of the test's (table, name) parameter, built once a session"""
    key = request.param
    if key not in _cases:
        _cases[key] = M.build_case(workdir, *key)
    return _cases[key]


def _of(table):
    return dict(argnames="case", argvalues=[(table, n) for n in M.TABLES[table][0]], ids=list(M.TABLES[table][0]), indirect=True)


ALL = dict(argnames="case", argvalues=M.ALL_CASES, ids=[n for _, n in M.ALL_CASES], indirect=True)


def test_the_tables_hold_every_case_the_tiers_run():
    assert len(M.ALL_CASES) == len({n for _, n in M.ALL_CASES}) == 12 + 12 + 6 + 4 + 3
    assert set(M.CONTAINERS) == {k["container"] for k in M.SIZE_CASES.values()} == {k["container"] for k in M.TOTAL_CASES.values()}
    assert [k["n"] for k in M.SIZE_CASES.values()] == [b + d for b in (256, 4096, 8192, 65536) for d in (-1, 0, 1)]
    assert M.ROW_BLOCK == 256 and M.SCAN_TILE == 4096 and 65536 == 16 * M.SCAN_TILE
    assert sorted({k["tagf"] for k in M.INTERLEAVE_CASES.values()}) == sorted(M.TAGF)


@pytest.mark.parametrize(**ALL)
def test_streams_and_expectation_fit_together(case):
    c = case
    assert c.n == len(c.text) == c.rw.n == len(c.expected) and c.n_seq == c.text.count(b"\n") == len(c.seq_to_file)
    assert len(c.tag_paths) == c.n_files == len(c.file_tags)
    assert not c.expected[:c.n_seq].any()
    # every file holds one tag per non-endmarker row of its sequences
    starts = np.concatenate((c.starts, [c.n]))
    lens = np.diff(starts) - 1
    for f in range(c.n_files):
        assert len(c.file_tags[f]) == int(lens[c.seq_to_file == f].sum())
    assert sum(len(t) for t in c.file_tags) == c.n - c.n_seq
    # the containers: where the ByteCodes start by the library's rule, and that they decode to the file's tags
    for f, p in enumerate(c.tag_paths):
        raw, body = open(p, "rb").read(), c.bodies[f]
        if not len(c.file_tags[f]):
            assert body == b"" and raw == (bytes(8) if c.container == "header" else b"")
        at = M.tags_start(raw)
        assert at == (8 if c.container == "header" or (c.container == "padded" and body) else 0)
        if c.container == "padded" and body:
            assert len(body) % 8 and len(raw) % 8 == 0 and len(raw) == 8 + len(body) + (-len(body) % 8)
            assert int(np.frombuffer(raw[:8], dtype=np.uint64)[0]) == 8 * len(body) and not any(raw[8 + len(body):])
        runs = M.decode_runs(raw, at)
        assert all(ln <= c.piece for _, ln in runs)
        kept = [(v, ln) for v, ln in runs if ln]
        assert kept == M.stream_runs(c.file_tags[f], c.piece)
        assert np.array_equal(np.repeat(np.array([v for v, _ in kept], dtype=np.uint64), [ln for _, ln in kept]), c.file_tags[f])
        if c.container == "zero_runs" and body:
            zero = [i for i, (_, ln) in enumerate(runs) if not ln]
            assert zero == [0, 1 + (len(kept) // 2), len(runs) - 1] and len(runs) == len(kept) + 3
            assert [runs[i][0] for i in zero] == [(77 << 11) | 5, 0, (12345 << 11) | (1 << 10)]
        elif c.container != "padded":
            assert len(runs) == len(kept)
        if c.piece == 1:
            assert len(kept) == len(c.file_tags[f])  # equal neighbours stay apart: as many runs as tags
    if c.piece == 1 and c.table == "long":
        assert any((t[1:] == t[:-1]).any() for t in c.file_tags)


@pytest.mark.parametrize(**ALL)
def test_sequential_merge_gives_the_expectation(case):
    c = case
    got = _sequential_merge(c.rw, c.tag_paths, c.seq_to_file, c.n_seq)
    assert np.array_equal(np.array(got, dtype=np.uint64), c.expected)


SMALL = [(t, n) for t, n in M.ALL_CASES if t == "files" or (t == "size" and M.SIZE_CASES[n]["n"] <= 4097)]  # every case of at most 4097 rows


@pytest.mark.parametrize(argnames="case", argvalues=SMALL, ids=[n for _, n in SMALL], indirect=True)
def test_suffix_arrays_follow_the_order_rule(case):
    """the oracle's suffix array (sequence * max_length + offset) against sorted() over the suffixes; quadratic in memory, so up to 4097 rows"""
    c = case
    assert c.n <= 4097 and len(SMALL) == 12
    order, _ = BC.naive_suffix_order(c.text)
    assert np.array_equal(c.starts[c.sa // c.ml] + c.sa % c.ml, order)


@pytest.mark.parametrize(**_of("size"))
def test_size_cases(case):
    k = M.SIZE_CASES[case.name]
    assert case.n == k["n"] and case.n_seq == M.SIZE_SEQS and case.container == k["container"]
    assert np.array_equal(case.seq_to_file, np.arange(M.SIZE_SEQS) % 2) and all(len(t) for t in case.file_tags)


@pytest.mark.parametrize(**_of("total"))
def test_total_cases(case):
    k = M.TOTAL_CASES[case.name]
    assert len(case.file_tags[0]) == k["total"] and case.n == M.TOTAL_ROWS and case.n % M.ROW_BLOCK and case.n % M.SCAN_TILE
    assert case.piece == k["piece"]
    if k["piece"] == 1:
        at = M.tags_start(open(case.tag_paths[0], "rb").read())
        runs = [r for r in M.decode_runs(open(case.tag_paths[0], "rb").read(), at) if r[1]]
        assert len(runs) == k["total"]
    else:  # (the tag count is on the border; the run count is whatever the tags give, at most that)
        assert len(M.stream_runs(case.file_tags[0], case.piece)) <= k["total"]


@pytest.mark.parametrize(**_of("files"))
def test_file_count_cases(case):
    c, lens = case, np.diff(np.concatenate((case.starts, [case.n]))) - 1
    if c.name == "one_file":
        assert c.n_files == 1 and not c.seq_to_file.any()
    elif c.name == "files_250":
        assert c.n_files == 250 and c.n_seq == 300 and c.n < 1000 and lens.min() == 0 and lens.max() == 3
        assert set(c.seq_to_file.tolist()) == set(range(250)) and {248, 249} <= set(c.seq_to_file.tolist())
        assert lens[c.seq_to_file == 249].max() > 0 and len(c.file_tags[249]) > 0
        d = np.diff(c.seq_to_file.astype(np.int64))
        assert (d < 0).any() and (d > 0).any()  # not ascending
        first_last = [(int(np.flatnonzero(c.seq_to_file == f)[0]), int(np.flatnonzero(c.seq_to_file == f)[-1])) for f in range(250)]
        assert any(b - a + 1 > int((c.seq_to_file == f).sum()) for f, (a, b) in enumerate(first_last))  # not grouped
        assert any(lens[c.seq_to_file == f].sum() == 0 for f in range(250))  # files of empty sequences only occur here too
    elif c.name.startswith("idle_file"):
        assert c.n_files == 3 and set(c.seq_to_file.tolist()) == {0, 2} and len(c.file_tags[1]) == 0
    else:
        assert c.n_files == 3 and (c.seq_to_file == 1).sum() == 3 and lens[c.seq_to_file == 1].sum() == 0 and len(c.file_tags[1]) == 0
        assert len(c.file_tags[0]) and len(c.file_tags[2])


@pytest.mark.parametrize(**_of("interleave"))
def test_interleave_cases(case):
    c = case
    assert c.n_files == 4 and c.n_seq == 16 and np.array_equal(c.seq_to_file, (np.arange(16) * 7) % 4)
    assert sorted(set(c.seq_to_file.tolist())) == [0, 1, 2, 3] and (np.diff(c.seq_to_file.astype(np.int64)) < 0).any()
    vals, lens = M.expected_runs(c.expected)
    if c.name == "interleave_wide":
        assert int(c.expected[c.n_seq:].min()) >= 1 << 44
    if c.name == "interleave_zero_first":
        assert vals[0] == 0 and int(lens[0]) > c.n_seq
        n_a = int((np.frombuffer(c.text, dtype=np.uint8) == ord("A")).sum())
        assert int(lens[0]) == c.n_seq + n_a
    if c.name == "interleave_coarse":  # runs that span files: a maximal run holds rows of all four
        file_of_row = c.seq_to_file[c.sa // c.ml]
        at = int(np.argmax(lens))
        lo = int(lens[:at].sum())
        assert set(file_of_row[lo:lo + int(lens[at])].tolist()) == {0, 1, 2, 3}
    if c.name == "interleave_fine":
        assert len(vals) < c.n - c.n_seq and int(lens[1:].max()) > 1  # haplotype copies share tags: real runs


@pytest.mark.parametrize(**_of("long"))
def test_long_run_cases(case):
    c = case
    vals, lens = M.expected_runs(c.expected)
    at = int(np.argmax(lens))
    lo, ln = int(lens[:at].sum()), int(lens[at])
    assert ln > 65536 and ln % 65536
    file_of_row = c.seq_to_file[c.sa // c.ml]
    assert set(file_of_row[lo:lo + ln].tolist()) == {0, 1}
    if c.flags & M.REFERENCE_RUNS:
        assert int(c.want_lengths.sum()) < c.n and int(c.want_lengths.max()) < 65536 and len(c.want_lengths) == len(lens)
    else:
        assert int(c.want_lengths.sum()) == c.n
