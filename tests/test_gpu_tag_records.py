"""The list records of the tag stage: lists appended to from every locate workgroup, segments handed out from the running total of gathered
values, duplicates of large queries in other workgroups' parts of the list, and the scan that stores the one-run queries' values, at its tile
borders and against its capacity.  The case tables are tag_record_cases.py's; test_tag_record_cases.py asserts on the CPU what they hold."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import border_cases as B
import pgx_ffi as P
import tag_record_cases as T
import variant_cases as V

pytestmark = pytest.mark.gpu

FLAGS = P.RUN_TAGS


@pytest.fixture(scope="module")
def tag_index(workdir, x_index):
    arr = B.tag_array(workdir, "random")
    idx = P.Index(x_index[0], arr.path)
    yield arr, idx
    idx.close()


def _thrice_same_as_oracle(arr, idx, key, st, en):
    ern, epo, epos, eover = arr.answers(key, st, en)
    outs = [idx.tag_query_batch(st, en) for _ in range(3)]
    rn, po, pos, nover = outs[0]
    assert np.array_equal(rn, ern)
    assert np.array_equal(po, epo)
    assert np.array_equal(pos, epos)
    assert nover == int(eover.sum())
    for o in outs[1:]:  # where a segment lies differs from run to run (the workgroups take theirs in the order they get there): it must not show
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(o[:3], outs[0][:3])) and o[3] == nover
    return nover


def test_every_list_from_every_workgroup(tag_index):
    arr, idx = tag_index
    st, en = T.mixed_queries(arr)
    assert len(st) == T.N_MIXED
    assert _thrice_same_as_oracle(arr, idx, "records_mixed", st, en) == 0


def test_large_duplicates_across_workgroups(tag_index):
    arr, idx = tag_index
    st, en = T.dup_queries(arr)
    assert _thrice_same_as_oracle(arr, idx, "records_dups", st, en) == T.DUP_GROUPS[1][1]


def _same(res, ref):  # (as test_gpu_spec_borders.py)
    assert np.array_equal(res["mem_offsets"], ref["mem_offsets"])
    assert res["mems"].tobytes() == ref["mems"].tobytes()
    assert res["n_extensions"] == ref["n_extensions"]
    assert np.array_equal(res["tag_run_counts"], ref["tag_run_counts"])
    assert np.array_equal(res["pos_offsets"], ref["pos_offsets"])
    assert np.array_equal(res["positions"], ref["positions"])
    assert res["n_tag_overflow"] == ref["n_tag_overflow"]


def _run(b, ref):
    b.run(B.SPEC_MIN_LEN, B.SPEC_MIN_OCC, FLAGS)
    _same(b.result(), ref)


@pytest.fixture(scope="module")
def full(workdir):
    case = B.spec_case(workdir)
    idx = P.Index(case.ri_path, case.full_tags)
    yield case, idx
    idx.close()


RUN_BATCHES = ("only_single", "no_single", "below_4096", "at_4096", "below_8192", "at_8192")


@pytest.mark.parametrize("name", RUN_BATCHES)
def test_exact_speculative_repeated(full, name):
    case, idx = full
    cat, offs, ref = case.ref("records_" + name, case.full_tags, T.run_batches(case)[name])
    b = idx.batch(cat, offs)
    try:
        _run(b, ref)  # exact: positions sized from the scan, the one-run values stored by a second pass of it
        assert b.spec_stats() == (0, 0)
        _run(b, ref)  # speculative: placed by the scan
        assert b.spec_stats() == (1, 0)
        _run(b, ref)
        assert b.spec_stats() == (2, 0)  # no fallback
    finally:
        b.free()


@pytest.mark.parametrize("name", RUN_BATCHES)
def test_three_launch_scan_gives_the_same(full, workdir, name):
    """PGX_SCAN_THREE is read once per process: a fresh child (started, not exec'ed) runs the batch three times -- exact, speculative, repeated --
    with the three-launch scans, where the one-run values keep their own pass"""
    case, _ = full
    cat, offs, ref = case.ref("records_" + name, case.full_tags, T.run_batches(case)[name])
    reads, out = os.path.join(workdir, "records3_%s.npz" % name), os.path.join(workdir, "records3_%s_out.npz" % name)
    np.savez(reads, cat=cat, offs=offs)
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tag_records_child.py")
    args = [case.ri_path, case.full_tags, reads, out, B.SPEC_MIN_LEN, B.SPEC_MIN_OCC, 3]
    r = subprocess.run([sys.executable, child] + [str(a) for a in args], env=dict(os.environ, PGX_SCAN_THREE="1"), capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    got = np.load(out)
    for k in range(3):
        res = {n: got["%s_%d" % (n, k)] for n in ("mem_offsets", "mems", "tag_run_counts", "pos_offsets", "positions")}
        res["mems"] = res["mems"].view(P.MEM_DTYPE).reshape(-1)
        res["n_extensions"] = int(got["n_extensions_%d" % k])
        res["n_tag_overflow"] = int(got["n_tag_overflow_%d" % k])
        _same(res, ref)
        assert tuple(got["spec_stats_%d" % k]) == (k, 0)  # the second and third run speculative, no fallback


def test_positions_capacity_alone(full, capfd):
    """the scan's own check: B exceeds the positions capacity taken from A and nothing else -- bit 0, raised by the tile with the total, every
    store below the capacity"""
    case, idx = full
    a, bb = T.positions_only_batches(case)
    acat, aoffs, ra = case.ref("records_P_A", case.full_tags, a)
    bcat, boffs, rb = case.ref("records_P_B", case.full_tags, bb)
    assert B.exceeded(ra, rb) == {"P"}
    b = idx.batch(acat, aoffs)
    try:
        _run(b, ra)
        _run(b, ra)
        assert b.spec_stats() == (1, 0)
        b.upload(bcat, boffs)
        capfd.readouterr()
        with V.env({"PGX_DEBUG_COUNTERS": "1"}):
            _run(b, rb)
        assert b.spec_stats() == (2, 1)
        m = re.search(r"speculative run: abort flags (\d+), 32-bit overflow (\d+), arena overflow (\d+)", capfd.readouterr().err)
        assert m, "no counters line of the speculative run"
        assert [int(g) for g in m.groups()] == [1, 0, 0]
        _run(b, rb)
        assert b.spec_stats() == (3, 1)  # speculative again
    finally:
        b.free()
