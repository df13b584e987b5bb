"""pgx_batch_locate on MEMs of exactly 2047, 2048, 2049, 16384 and 16385 occurrences: pgx_ml_classify_kernel derives the classes of the
sort it shares with the tag stage in its own code.  Compared with numpy on the oracle's suffix array, not with pgx_locate_batch (both go
through the same sort).  test_border_cases.py asserts on the CPU that the oracle's MEMs have exactly these sizes."""
import numpy as np
import pytest

import border_cases as B
import pgx_ffi as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def located(workdir):
    case = B.mem_locate_case(workdir)
    idx = P.Index(case["ri_path"])
    b = idx.batch(case["cat"], case["offs"])
    b.run(B.MEM_LOCATE_MIN_LEN, 1, 0)
    yield case, b
    b.free()
    idx.close()


def test_mems_are_the_oracles(located):
    case, b = located
    res = b.result()
    assert np.array_equal(res["mem_offsets"], case["ref"]["mem_offsets"])
    assert res["mems"].tobytes() == case["ref"]["mems"].tobytes()


@pytest.mark.parametrize("chains", [0, P.LOCATE_CHAINS])
@pytest.mark.parametrize("flags", [P.LOCATE_UNIQUE, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE])
def test_sorted_unique_occurrences(located, monkeypatch, flags, chains):
    case, b = located
    monkeypatch.setenv("PGX_LOCATE_SETS", "0")  # SEQ_IDS | UNIQUE through the sort, not the sequence sets
    eoff, evals = B.mem_locate_expected(case, flags)
    b.locate(flags | chains)
    got = b.locations()
    assert got["resident"] == (not chains)
    assert got["set_words"] == 0  # the sort ran, not the sequence sets
    assert got["n_not_located"] == 0 and got["n_values"] == len(evals)
    assert np.array_equal(got["loc_offsets"], eoff)
    assert np.array_equal(got["values"], evals)
