"""pgx_locate_batch with ranges of exactly c positions at every border of the sort it shares with the tag stage (locate_core derives the
classes in its own code: one wave up to 2048 values, a workgroup in LDS up to 16384, global scratch beyond), against numpy on the
oracle's suffix array.  test_border_cases.py asserts on the CPU that SEQ_IDS | UNIQUE really removes duplicates from these ranges."""
import numpy as np
import pytest

import border_cases as B
import pgx_ffi as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flags", [0, P.LOCATE_SEQ_IDS, P.LOCATE_UNIQUE, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE])
def test_ranges_of_exactly_c_positions(workdir, flags):
    case = B.locate_case(workdir)
    eoff, evals = B.locate_expected(case, flags)
    idx = P.Index(case["ri_path"], mode=P.MODE_STRICT)
    try:
        off, vals = idx.locate_batch(case["first"], case["last"], flags)
        assert np.array_equal(off, eoff)
        assert np.array_equal(vals, evals)
        # every c in a call of its own: the largest range of a call sizes the dynamic LDS of the workgroup sort
        for k, c in enumerate(B.LOCATE_C):
            off, vals = idx.locate_batch(case["first"][3 * k:3 * k + 3], case["last"][3 * k:3 * k + 3], flags)
            assert np.array_equal(off, eoff[3 * k:3 * k + 4] - eoff[3 * k]), c
            assert np.array_equal(vals, evals[int(eoff[3 * k]):int(eoff[3 * k + 3])]), c
    finally:
        idx.close()
