"""The case tables of tag_record_cases.py hold what they claim -- asserted with the oracle and numpy alone, so that no test of
test_gpu_tag_records.py can pass by missing its target."""
import numpy as np

import border_cases as B
import tag_record_cases as T


def _classes(rn):
    return np.array([T.record_class(int(c)) for c in rn])


def test_mixed_batch_has_every_class_in_every_window(workdir):
    arr = B.tag_array(workdir, "random")
    fc = T.mixed_batch()
    st, en = T.mixed_queries(arr)
    assert len(st) == T.N_MIXED == 3 * T.LOCATE_WG + 1
    rn, po, pos, over = arr.answers("records_mixed", st, en)
    assert [int(c) for c in rn] == [c for _, c in fc]  # the oracle counts the runs the table names
    cls, win = _classes(rn), T.windows(len(rn))
    for w in range(3):
        assert set(cls[win == w]) == set(T.CLASSES), w
    assert cls[win == 3].tolist() == ["large"]  # the ragged fourth workgroup appends to a list as well
    assert not over.any()
    assert len({f % 10 for f, _ in fc}) == 10
    # a duplicate-free large list: the segments of this batch are all read through their own records
    large = [q for q in fc if q[1] > B.SORT_LDS_CAP]
    assert len(set(large)) == len(large) == 16


def test_duplicates_have_their_representative_candidates_in_other_windows(workdir):
    arr = B.tag_array(workdir, "random")
    fc = T.dup_batch()
    st, en = T.dup_queries(arr)
    rn, po, pos, over = arr.answers("records_dups", st, en)
    assert [int(c) for c in rn] == [c for _, c in fc]
    win = T.windows(len(fc))
    for (f, c), copies in T.DUP_GROUPS:
        at = np.array([i for i, q in enumerate(fc) if q == (f, c)])
        assert T.record_class(c) in ("large", "scratch")
        assert len(at) == (copies if copies else len(at)) and len(at) >= 4
        # whichever copy claims the table slot, copies lie in every other full window (and so in other workgroups' parts of the large list)
        assert set(win[at]) >= {0, 1, 2}
    bulk = sum(q == T.DUP_GROUPS[0][0] for q in fc)
    assert bulk > B.SORT_LDS_CAP
    assert T.record_class(T.DUP_GROUPS[2][0][1]) == "scratch"
    # distinct large queries beside them, nobody's duplicate
    assert all(fc.count(q) == 1 and T.record_class(q[1]) == "large" for q in T.DUP_DISTINCT)
    # the overflow count: exactly the copies of the group that ends in the last run with f % 10 == 0
    (f, c), copies = T.DUP_GROUPS[1]
    assert f % 10 == 0 and f + c - 1 == B.N_TAG_RUNS
    assert int(over.sum()) == copies and all(fc[i] == (f, c) for i in np.flatnonzero(over))
    assert {T.record_class(int(c)) for c in rn} >= {"single", "small", "large", "scratch"}


def test_run_batches_are_what_their_names_say(workdir):
    case = B.spec_case(workdir)
    batches = T.run_batches(case)
    refs = {name: case.ref("records_" + name, case.full_tags, reads)[2] for name, reads in batches.items()}
    rc = refs["only_single"]["tag_run_counts"]
    assert len(rc) > 3000 and np.all(rc == 1)
    assert len(refs["only_single"]["positions"]) == len(rc)
    rc = refs["no_single"]["tag_run_counts"]
    assert len(rc) > 1000 and np.all(rc >= 2)
    assert {T.record_class(int(c)) for c in rc} == {"small", "big", "large"}
    for t in T.TILE_BORDERS:
        below, at = refs["below_%d" % t], refs["at_%d" % t]
        assert len(batches["at_%d" % t]) == len(batches["below_%d" % t]) + 1
        assert len(below["mems"]) < t <= len(at["mems"])  # the last total below the tile border, the first at or above it
        for r in (below, at):
            assert np.any(r["tag_run_counts"] == 1) and np.any(r["tag_run_counts"] > 1)


def test_positions_capacity_alone(workdir):
    """SpecCase allows it: the values of its tag arrays repeat after 3000, so one query of many runs has few unique values for its gathered ones"""
    case = B.spec_case(workdir)
    a, b = T.positions_only_batches(case)
    assert len(a) == len(b)
    ra = case.ref("records_P_A", case.full_tags, a)[2]
    rb = case.ref("records_P_B", case.full_tags, b)[2]
    assert B.exceeded(ra, rb) == {"P"}
    assert B.demand(ra)["largest"] <= B.SORT_WG_LDS_CAP  # A's next run speculates
