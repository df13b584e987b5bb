"""merge_tags on the GPU at its borders (merge_cases.py; test_merge_cases.py shows on the CPU that the tables hold what they claim): for every
case the output file is byte-equal to the host writer's file of the expected runs, and the oracle's reading of it, expanded item by item, is
the expected array.  Then what stays behind between calls, whether the merged file serves find_mems, and every refusal."""
import os

import numpy as np
import pytest

import merge_cases as M
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W

pytestmark = pytest.mark.gpu

_cases = {}


def _case(workdir, table, name):
    if (table, name) not in _cases:
        _cases[table, name] = M.build_case(workdir, table, name)
    return _cases[table, name]


def _written(workdir, c):
    """the host writer's file of the case's runs (P.write_compact_tags cuts runs of 512 and more itself)"""
    p = os.path.join(workdir, "merge_want_%s.tags" % c.name)
    if not os.path.exists(p):
        P.write_compact_tags(p, c.want_values, c.want_lengths)
    return open(p, "rb").read()


def _merge(c, out):
    if os.path.exists(out):
        os.remove(out)
    P.merge_tags(c.ri, c.tag_paths, c.seq_to_file, out, flags=c.flags)
    return open(out, "rb").read()


def _check(workdir, c, out):
    got = _merge(c, out)
    assert got == _written(workdir, c), c.name
    # the oracle's reading of the file: pieces of 511 for runs of 512 and more, and the expected array row by row
    t = O.Tags(out, O.TAGS_COMPACT)
    k = t.n_runs
    assert k == t.n_items
    starts = np.array([t.L.orc_tags_interval(t.h, i) for i in range(k)], dtype=np.int64)
    items = np.array([t.L.orc_tags_item(t.h, i) for i in range(k)], dtype=np.uint64)
    pieces = M.split511(c.want_values, c.want_lengths)
    total = int(c.want_lengths.sum())
    assert k == len(pieces) and starts[0] == 0 and (np.diff(starts) > 0).all() and starts[-1] < total
    lens = np.diff(np.concatenate((starts, [total])))
    assert list(zip(items.tolist(), lens.tolist())) == pieces, c.name
    rows = np.repeat(items, lens)
    if c.flags & M.REFERENCE_RUNS:  # (a wrapped run lost positions, as in the reference: the rows of the runs as written)
        assert total < c.n and np.array_equal(rows, np.repeat(c.want_values, c.want_lengths.astype(np.int64)))
    else:
        assert total == c.n and len(rows) == c.n and np.array_equal(rows, c.expected), c.name
    return got


# one case a table is merged twice, with a smaller case of another shape in between: the device buffers are per call, nothing may be left over
TWICE = {"size": "n_65537", "total": "total_4097_piece_1", "files": "files_250", "interleave": "interleave_wide", "long": "long_piece_511"}
BETWEEN = ("size", "n_255")


def _run_case(workdir, table, name):
    c = _case(workdir, table, name)
    out = os.path.join(workdir, "merge_out_%s.tags" % name)
    got = _check(workdir, c, out)
    if TWICE[table] == name:
        small = _case(workdir, *BETWEEN)
        assert small.n < c.n
        _check(workdir, small, os.path.join(workdir, "merge_out_between.tags"))
        assert _merge(c, out + ".again") == got
    return c, out


@pytest.mark.parametrize("name", list(M.SIZE_CASES))
def test_size_borders(workdir, name):
    _run_case(workdir, "size", name)


@pytest.mark.parametrize("name", list(M.TOTAL_CASES))
def test_file_total_borders(workdir, name):
    _run_case(workdir, "total", name)


@pytest.mark.parametrize("name", list(M.FILE_CASES))
def test_file_counts(workdir, name):
    _run_case(workdir, "files", name)


@pytest.mark.parametrize("name", list(M.INTERLEAVE_CASES))
def test_interleaved_files(workdir, name):
    c, out = _run_case(workdir, "interleave", name)
    if name == "interleave_fine":  # the merged file serves find_mems like any other tag array
        seqs = [np.frombuffer(s, dtype=np.uint8) for s in c.text.split(b"\n") if len(s)]
        cat, offs = W.sample_reads(seqs, 500, 100, seed=5)
        res = P.Index(c.ri, out).find_mems(cat, offs, 15, 1, tags=True)
        ref = O.find_mems_batch(c.rw, O.Tags(out, O.TAGS_COMPACT), cat, offs, 15, 1, threads=O.lib().orc_max_threads())
        assert len(res["mems"]) > 500 and len(ref["positions"]) > 500
        assert res["mems"].tobytes() == ref["mems"].tobytes() and np.array_equal(res["positions"], ref["positions"])


@pytest.mark.parametrize("name", list(M.LONG_CASES))
def test_long_runs(workdir, name):
    _run_case(workdir, "long", name)


# ---- refusals: the library's error, no file at `out`, and a good call afterwards succeeds
def _refused(workdir, good, code, words, ri, tag_paths, s2f, flags=0, call=None):
    out = os.path.join(workdir, "merge_refused.tags")
    if os.path.exists(out):
        os.remove(out)
    with pytest.raises(P.PgxError) as e:
        if call is None:
            P.merge_tags(ri, tag_paths, s2f, out, flags=flags)
        else:
            call(out)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert not os.path.exists(out)
    assert _merge(good, out) == _written(workdir, good)
    os.remove(out)


def test_refused_sequence_maps(workdir):
    c = _case(workdir, "files", "idle_file_bare")  # three files, seven sequences, none of them empty
    assert c.n_files == 3 and all(np.diff(np.concatenate((c.starts, [c.n]))) > 1)
    for bad in (c.n_files, 254, 255, 0xFFFFFFFF):
        for at in (0, c.n_seq // 2, c.n_seq - 1):
            s2f = c.seq_to_file.copy()
            s2f[at] = bad
            _refused(workdir, c, P.ERR_ARG, ["file index"], c.ri, c.tag_paths, s2f)
    # an empty sequence has no row of its own in the BWT: its entry is checked all the same
    e = _case(workdir, "files", "empty_only_bare")
    for at in np.flatnonzero(e.seq_to_file == 1):
        for bad in (e.n_files, 255):
            s2f = e.seq_to_file.copy()
            s2f[at] = bad
            _refused(workdir, e, P.ERR_ARG, ["file index"], e.ri, e.tag_paths, s2f)
    # one entry short, one long
    _refused(workdir, c, P.ERR_ARG, ["%d entries" % (c.n_seq - 1)], c.ri, c.tag_paths, c.seq_to_file[:-1])
    _refused(workdir, c, P.ERR_ARG, ["%d entries" % (c.n_seq + 1)], c.ri, c.tag_paths, np.append(c.seq_to_file, 0))


def test_refused_file_counts_and_flags(workdir):
    c = _case(workdir, "files", "idle_file_bare")
    _refused(workdir, c, P.ERR_ARG, ["between 1 and 250"], c.ri, [], c.seq_to_file)
    _refused(workdir, c, P.ERR_ARG, ["between 1 and 250"], c.ri, [c.tag_paths[f % 3] for f in range(251)], c.seq_to_file)
    for flags in (2, 8, 0x80000000, M.REFERENCE_RUNS | 4):
        _refused(workdir, c, P.ERR_ARG, ["unknown flag"], c.ri, c.tag_paths, c.seq_to_file, flags=flags)


def test_refused_streams(workdir):
    c = _case(workdir, "files", "idle_file_bare")
    tags, have = c.file_tags[2], len(c.file_tags[2])
    d = os.path.join(workdir, "merge_bad_streams")
    os.makedirs(d, exist_ok=True)

    def stream(name, raw):
        p = os.path.join(d, name)
        with open(p, "wb") as f:
            f.write(raw)
        return c.tag_paths[:2] + [p]

    for container in ("bare", "header"):
        short = stream("short_" + container, M.stream_file(M.stream_body(tags[:-1], container), container))
        _refused(workdir, c, P.ERR_FORMAT, [short[2], "%d tags" % (have - 1), "%d positions" % have], c.ri, short, c.seq_to_file)
        long_ = stream("long_" + container, M.stream_file(M.stream_body(np.append(tags, tags[-1:]), container), container))
        _refused(workdir, c, P.ERR_FORMAT, [long_[2], "%d tags" % (have + 1), "%d positions" % have], c.ri, long_, c.seq_to_file)
    # tags for the file that owns no sequence
    extra = c.tag_paths[:1] + [c.tag_paths[0]] + c.tag_paths[2:]
    _refused(workdir, c, P.ERR_FORMAT, [c.tag_paths[0], "%d tags" % len(c.file_tags[0]), " 0 positions"], c.ri, extra, c.seq_to_file)
    # cut in the middle of a ByteCode (these tags take three bytes and more)
    body = M.stream_body(tags, "bare")
    assert body[-2] & 0x80
    cut = stream("cut", body[:-1])
    _refused(workdir, c, P.ERR_FORMAT, [cut[2], "ByteCode"], c.ri, cut, c.seq_to_file)
    # a missing tag file, as the last of three
    missing = c.tag_paths[:2] + [os.path.join(d, "no_such_file.tags")]
    _refused(workdir, c, P.ERR_FORMAT, [missing[2]], c.ri, missing, c.seq_to_file)


def test_refused_empty_tag_file_of_a_graph(workdir, golden):
    c = _case(workdir, "files", "idle_file_bare")
    bt = os.path.join(golden, "bidirectional_test")
    empty = os.path.join(workdir, "merge_empty.tags")
    open(empty, "wb").close()
    _refused(workdir, c, P.ERR_FORMAT, ["empty tag file", empty], None, None, None,
             call=lambda out: P.merge_tags_gbz(os.path.join(bt, "xy.gbz"), os.path.join(bt, "xy.ri"), [empty], out))
    with open(empty, "wb") as f:
        f.write(bytes(8))  # (a header and no body)
    _refused(workdir, c, P.ERR_FORMAT, ["empty tag file", empty], None, None, None,
             call=lambda out: P.merge_tags_gbz(os.path.join(bt, "xy.gbz"), os.path.join(bt, "xy.ri"), [empty], out))
