"""The tag stage through pgx_batch_run where its overflow count is not zero -- one tag array per device site, each in an exact, a
speculative and a repeated run -- and speculative sizing with one capacity exceeded at a time.  The batches are border_cases.py's;
test_border_cases.py asserts on the CPU, from the oracle's answers, which site overflows and which capacities each batch exceeds."""
import re

import numpy as np
import pytest

import border_cases as B
import pgx_ffi as P
import variant_cases as V

pytestmark = pytest.mark.gpu

FLAGS = P.RUN_TAGS


def _same(res, ref):
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


@pytest.mark.parametrize("site", B.OVERFLOW_FILES)
def test_overflow_count_through_mems(workdir, site):
    case = B.spec_case(workdir)
    key, tags_path, reads = B.overflow_file(case, site)
    cat, offs, ref = case.ref(key, tags_path, reads)
    jcat, joffs, jref = case.ref(key + "_junk", tags_path, B.junk_reads(len(reads)))
    assert ref["n_tag_overflow"] > 0
    idx = P.Index(case.ri_path, tags_path)
    b = idx.batch(cat, offs)
    try:
        _run(b, ref)  # exact
        assert b.spec_stats() == (0, 0)
        _run(b, ref)  # speculative
        assert b.spec_stats() == (1, 0)
        b.upload(jcat, joffs)
        _run(b, jref)  # far fewer MEMs: fits
        assert b.spec_stats() == (2, 0)
        b.upload(cat, offs)
        _run(b, ref)  # the capacities of the run before are too small: aborted and repeated exactly -- the count is that of one pass
        assert b.spec_stats() == (3, 1)
    finally:
        b.free()
        idx.close()


@pytest.fixture(scope="module")
def full(workdir):
    case = B.spec_case(workdir)
    idx = P.Index(case.ri_path, case.full_tags)
    yield case, idx
    idx.close()


@pytest.mark.parametrize("name", list(B.CAPACITY_EXCEEDED))
def test_one_capacity_at_a_time(full, name, capfd):
    case, idx = full
    batches = B.capacity_batches(case)
    acat, aoffs, ra = case.ref("cap_A", case.full_tags, batches["A"])
    bcat, boffs, rb = case.ref("cap_" + name, case.full_tags, batches[name])
    assert B.exceeded(ra, rb) == B.CAPACITY_EXCEEDED[name]  # with_slack(v) = v + v / 4 + 64 of A's counts; the power of two for the largest run count
    b = idx.batch(acat, aoffs)
    try:
        _run(b, ra)
        _run(b, ra)
        assert b.spec_stats() == (1, 0)
        b.upload(bcat, boffs)
        capfd.readouterr()
        with V.env({"PGX_DEBUG_COUNTERS": "1"}):
            _run(b, rb)
        assert b.spec_stats() == (2, 1)  # exactly one fallback
        # and it was the capacity check meant that raised it: not the slot arena, not the 32-bit state (either repeats the run as well)
        m = re.search(r"speculative run: abort flags (\d+), 32-bit overflow (\d+), arena overflow (\d+) \(top \d+\), MEMs (\d+) of capacity (\d+)", capfd.readouterr().err)
        assert m, "no counters line of the speculative run"
        flags, ovf32, arena, mems, cap = (int(g) for g in m.groups())
        assert (ovf32, arena) == (0, 0)
        if name == "mems":  # behind the compaction's flag the tag stage's checks read counts of a stage that did not run: only bit 4 is defined
            assert flags & B.CAPACITY_ABORT_FLAGS[name]
        else:
            assert flags == B.CAPACITY_ABORT_FLAGS[name]
        assert cap == B.capacities(ra)["mems"] and (mems > cap) == ("mems" in B.CAPACITY_EXCEEDED[name])
        _run(b, rb)
        assert b.spec_stats() == (3, 1)  # speculative again
        b.upload(acat, aoffs)
        _run(b, ra)
        assert b.spec_stats() == (4, 1)  # A fits what B left behind
    finally:
        b.free()


def test_largest_query_beyond_16384_runs_never_speculates(full):
    case, idx = full
    cat, offs, ref = case.ref("over16384", case.full_tags, B.over_16384_reads(case))
    assert B.demand(ref)["largest"] > B.SORT_WG_LDS_CAP
    b = idx.batch(cat, offs)
    try:
        for _ in range(3):
            _run(b, ref)
        assert b.spec_stats() == (0, 0)  # not a fallback: such a batch is sized exactly every time
    finally:
        b.free()
