"""The tag stage through pgx_tag_query_batch at the border of every size class, with the overflow count compared where it is not
zero and the scans at their tile borders.  The case tables are border_cases.py's; test_border_cases.py asserts on the CPU that they
hit what they claim."""
import numpy as np
import pytest

import border_cases as B
import pgx_ffi as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def indexes(workdir, x_index):
    out = {}
    for pattern in B.TAG_PATTERNS:
        arr = B.tag_array(workdir, pattern)
        out[pattern] = (arr, P.Index(x_index[0], arr.path))
    yield out
    for _, idx in out.values():
        idx.close()


def _same_as_oracle(arr, idx, key, st, en):
    rn, po, pos, nover = idx.tag_query_batch(st, en)
    ern, epo, epos, eover = arr.answers(key, st, en)
    assert np.array_equal(rn, ern), key
    assert np.array_equal(po, epo), key
    assert np.array_equal(pos, epos), key
    assert nover == int(eover.sum()), key
    return nover


@pytest.mark.parametrize("pattern", B.TAG_PATTERNS)
def test_run_counts_at_every_class_border(indexes, pattern):
    """every c of BORDER_C in a batch of its own (the largest run count of the batch sizes the dynamic LDS of the large path and decides
    whether there is global scratch), at three first runs -- f % 10 == 0 among them -- then all of them in one batch"""
    arr, idx = indexes[pattern]
    everything = []
    for c in B.BORDER_C:
        fc = B.border_queries(c)
        st, en = arr.queries(fc)
        rn, po, pos, nover = idx.tag_query_batch(st, en)
        assert nover == 0
        for i, (f, _) in enumerate(fc):
            exp, _ = arr.expected(f, c)  # numpy: the sorted unique values of items f - 1 .. f + c - 2 (f .. f + c - 1 where f % 10 == 0)
            assert int(rn[i]) == c, (c, f)
            assert np.array_equal(pos[int(po[i]):int(po[i + 1])], exp), (c, f)
        _same_as_oracle(arr, idx, ("border", c), st, en)
        everything += fc
    st, en = arr.queries(everything)
    _same_as_oracle(arr, idx, "border_all", st, en)


@pytest.mark.parametrize("sites,count", [(["single"], 1), (["small"], 1), (["big"], 1), (["large"], 1), (["large_scratch"], 1), (["large_dups"], 3),
                                         (list(B.OVERFLOW_SITES), 8)],
                         ids=["single", "small", "big", "large", "large_scratch", "large_dups", "all"])
def test_overflow_count_site_by_site(indexes, sites, count):
    """queries that end in the last run with f % 10 == 0 read one item beyond the array (as 0, counted): one device site per sub-batch, beside
    queries of every class that do not overflow; then all sites together"""
    arr, idx = indexes["random"]
    st, en = arr.queries(B.overflow_batch(sites))
    assert _same_as_oracle(arr, idx, ("over", sites[0] if len(sites) == 1 else "all"), st, en) == count


def test_inverted_queries(indexes):
    arr, idx = indexes["random"]
    st, en = B.inverted_queries(arr)
    rn, po, pos, nover = idx.tag_query_batch(st, en)
    assert not rn.any() and not po.any() and len(pos) == 0 and nover == 0
    _same_as_oracle(arr, idx, "inverted", st, en)
    # and between other queries
    fc = B.border_queries(17) + B.border_queries(1)
    st2, en2 = arr.queries(fc)
    st, en = np.concatenate([st2[:3], st, st2[3:]]), np.concatenate([en2[:3], en, en2[3:]])
    _same_as_oracle(arr, idx, "inverted_mixed", st, en)


@pytest.mark.parametrize("n", B.QUERY_COUNTS)
def test_query_counts_at_scan_tile_borders(indexes, n):
    arr, idx = indexes["random"]
    st, en = arr.queries(B.count_queries())
    ern, epo, epos, eover = arr.answers("counts", st, en)
    rn, po, pos, nover = idx.tag_query_batch(st[:n], en[:n])
    assert np.array_equal(rn, ern[:n])
    assert np.array_equal(po, epo[:n + 1])  # po[n]: written by the tile that holds item n - 1
    assert np.array_equal(pos, epos[:int(epo[n])])
    assert nover == 0 == int(eover[:n].sum())
