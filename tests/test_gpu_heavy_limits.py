"""The heavy-read kernel at its two limits: more reads offered than PGX_FM_HEAVY_CAP takes (the others continue on their lanes), and
reads of PGX_FM_HEAVY_MAXLEN - 1, PGX_FM_HEAVY_MAXLEN and PGX_FM_HEAVY_MAXLEN + 1 symbols (the last is never handed on; the others index a
scratch row of 4096 entries by start position).  test_border_cases.py asserts on the CPU that the reads pass these limits."""
import numpy as np
import pytest

import border_cases as B
import pgx_ffi as P
import variant_cases as V

pytestmark = pytest.mark.gpu

FORCED = [P.MODE_IMAGE_PAIRS, P.MODE_IMAGE_DENSE2]


def _oracle(mid, key, cat, offs):
    return V.oracle(mid, 20, 1, key=key, cat=cat, offs=offs)


@pytest.mark.parametrize("force", FORCED)
def test_more_heavy_reads_than_the_list_takes(workdir, monkeypatch, force):
    monkeypatch.setenv("PGX_FM_HEAVY_EXT", str(B.HEAVY_EXT))
    mid = V.mid_case(workdir)
    cat, offs = B.heavy_cap_reads(mid)
    ref = _oracle(mid, "heavy_cap", cat, offs)
    idx = P.Index(mid["ri_path"], mid["tags_path"], mode=P.MODE_COMPAT | force)
    try:
        res, tm = V.run(idx, cat, offs, 20, 1)
        V.same(res, ref)  # extension count included
        # heavy_reads is min(offered, PGX_FM_HEAVY_CAP): the list was filled.  That more reads were offered than it takes is asserted from the
        # oracle's extension counts in test_border_cases.py::test_heavy_cases_pass_their_limits (over 8392 of these 9000 qualify)
        assert tm.heavy_reads == B.FM_HEAVY_CAP
    finally:
        idx.close()


@pytest.mark.parametrize("force", FORCED)
def test_reads_around_the_longest_heavy_read(workdir, monkeypatch, force):
    monkeypatch.setenv("PGX_FM_HEAVY_EXT", str(B.HEAVY_EXT))
    mid = V.mid_case(workdir)
    idx = P.Index(mid["ri_path"], mid["tags_path"], mode=P.MODE_COMPAT | force)
    try:
        heavy = {}
        for name, lengths in (("all", B.HEAVY_LENGTHS), ("without_4097", B.HEAVY_LENGTHS[:-1])):
            cat, offs = B.heavy_long_reads(mid, lengths)
            res, tm = V.run(idx, cat, offs, 20, 1)
            V.same(res, _oracle(mid, "heavy_long_" + name, cat, offs))
            heavy[name] = tm.heavy_reads
        assert B.HEAVY_LENGTHS[-1] == B.FM_HEAVY_MAXLEN + 1
        assert heavy["all"] == heavy["without_4097"] >= 3  # the 4097-symbol read was not handed on; the three others were
        # the reads of 1000, 4095 and 4096 symbols alone: each is handed on
        n_long = len(B.HEAVY_LENGTHS) - 1
        cat, offs = B.heavy_long_reads(mid, B.HEAVY_LENGTHS[:-1])
        lo = int(offs[len(offs) - 1 - n_long])
        cat, offs = cat[lo:], offs[len(offs) - 1 - n_long:] - np.uint64(lo)
        res, tm = V.run(idx, cat, offs, 20, 1)
        V.same(res, _oracle(mid, "heavy_long_three", cat, offs))
        assert tm.heavy_reads == n_long
        # and the 4097-symbol read alone is not
        cat, offs = B.heavy_long_reads(mid, B.HEAVY_LENGTHS[-1:])
        lo = int(offs[-2])
        cat, offs = cat[lo:], offs[-2:] - np.uint64(lo)
        res, tm = V.run(idx, cat, offs, 20, 1)
        V.same(res, _oracle(mid, "heavy_long_4097", cat, offs))
        assert tm.heavy_reads == 0
    finally:
        idx.close()
