"""Every instance of pgx_find_mems_kernel and pgx_find_mems_pairs_kernel the runtime can launch (the two tables of pgx_batch.hip, listed
by pgx_kernel_variants), each driven by the index, mode and knobs meant to select it: the run reports the instance it launched
(pgx_timing.kernels) -- it must be the expected one -- and its MEMs, extension count and tag positions equal the oracle's bit for bit.
The last test asserts that the union of the instances seen is the product's own list: a table entry no configuration reaches fails it."""
import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import variant_cases as V

pytestmark = pytest.mark.gpu

PAIRS = [(20, 1), (12, 3)]  # (min_len, min_occ): both behind the seed tables (depth 12 and 10); the LCE path runs at min_occ <= 1 only
FM, PR = V.fm_bits, V.pairs_bits
LCE = "lce"  # in an expected pairs instance: forward stages through the text where min_occ <= 1


def _pairs_runs(s64):
    """the run knobs over a narrow PAIRS image (blocks every 64 / 96 positions); the dense2 kernel serves the reads with a byte outside A C G T"""
    side = FM(0, 2, 1, 1)
    return [({}, side, (0, 1, 0, s64, LCE)),
            ({"PGX_FM_LCE": "0"}, side, (0, 1, 0, s64, 0)),
            ({"PGX_FM_COOP": "1"}, side, (0, 1, 1, s64, 0)),
            ({"PGX_FM_COOP": "0"}, side, (0, 1, 0, s64, LCE)),
            ({"PGX_FM_PACKED": "0"}, side, (0, 0, 0, s64, 0)),
            ({"PGX_FM_NARROW": "0"}, FM(0, 2, 0, 1), (0, 1, 0, s64, LCE)),
            ({"PGX_FM_NARROW_FORCE_REDO": "1"}, side | P.KERNELS_FM_REDO, (0, 1, 0, s64, LCE))]


def _wide_runs(s64):
    side = FM(0, 3, 0, 1)
    return [({}, side, (1, 1, 0, s64, 0)), ({"PGX_FM_COOP": "1"}, side, (1, 1, 1, s64, 0)), ({"PGX_FM_PACKED": "0"}, side, (1, 0, 0, s64, 0))]


def _fm_runs(in_lds, kind, seeded, narrow_form=True):
    """the one kernel over every read: 32-bit interval state where the image has that form, 64-bit with PGX_FM_NARROW=0, and the forced repeat"""
    if not narrow_form:
        return [({}, FM(in_lds, kind, 0, seeded), None)]
    return [({}, FM(in_lds, kind, 1, seeded), None), ({"PGX_FM_NARROW": "0"}, FM(in_lds, kind, 0, seeded), None),
            ({"PGX_FM_NARROW_FORCE_REDO": "1"}, FM(in_lds, kind, 1, seeded) | P.KERNELS_FM_REDO, None)]


# id -> (case, mode bits, oracle mode, image environment (read when the index is opened / its device image built), runs)
# a run: (run environment, expected pgx_find_mems_kernel bits (0: not launched), expected pairs instance or None)
CONFIGS = {
    "mid-pairs-s64": ("mid", P.MODE_COMPAT | P.MODE_IMAGE_PAIRS, O.MODE_COMPAT, {"PGX_PAIRS_STRIDE": "64"}, _pairs_runs(1)),
    "mid-pairs-s96": ("mid", P.MODE_COMPAT | P.MODE_IMAGE_PAIRS, O.MODE_COMPAT, {"PGX_PAIRS_STRIDE": "96"}, _pairs_runs(0)),
    "mid-pairs-s64-strict": ("mid", P.MODE_STRICT | P.MODE_IMAGE_PAIRS, O.MODE_STRICT, {"PGX_PAIRS_STRIDE": "64"}, _pairs_runs(1)[:1]),
    "mid-pairs-wide-s64": ("mid", P.MODE_COMPAT | P.MODE_IMAGE_PAIRS | P.MODE_IMAGE_WIDE, O.MODE_COMPAT, {"PGX_PAIRS_STRIDE": "64", "PGX_SB_SHIFT": "6"}, _wide_runs(1)),
    "mid-pairs-wide-s96": ("mid", P.MODE_COMPAT | P.MODE_IMAGE_PAIRS | P.MODE_IMAGE_WIDE, O.MODE_COMPAT, {"PGX_PAIRS_STRIDE": "96", "PGX_SB_SHIFT": "6"}, _wide_runs(0)),
    "mid-pairs-unseeded": ("mid", P.MODE_COMPAT | P.MODE_IMAGE_PAIRS, O.MODE_COMPAT, {"PGX_SEED_K": "0"}, _fm_runs(0, 2, 0)[:2]),  # (the pairs kernel runs behind a seed table only)
    "mid-dense2": ("mid", P.MODE_COMPAT | P.MODE_IMAGE_DENSE2, O.MODE_COMPAT, {}, _fm_runs(0, 2, 1)),
    "mid-dense2-wide": ("mid", P.MODE_COMPAT | P.MODE_IMAGE_DENSE2 | P.MODE_IMAGE_WIDE, O.MODE_COMPAT, {"PGX_SB_SHIFT": "6"}, _fm_runs(0, 3, 1, False)),
    "mid-dense2-wide-unseeded": ("mid", P.MODE_COMPAT | P.MODE_IMAGE_DENSE2 | P.MODE_IMAGE_WIDE, O.MODE_COMPAT, {"PGX_SB_SHIFT": "6", "PGX_SEED_K": "0"}, _fm_runs(0, 3, 0, False)),
    "mid-dense": ("mid", P.MODE_COMPAT | P.MODE_IMAGE_DENSE, O.MODE_COMPAT, {}, _fm_runs(0, 1, 1)),
    "mid-dense-strict": ("mid", P.MODE_STRICT | P.MODE_IMAGE_DENSE, O.MODE_STRICT, {}, _fm_runs(0, 1, 1)[:1]),
    "mid-dense-unseeded": ("mid", P.MODE_COMPAT | P.MODE_IMAGE_DENSE, O.MODE_COMPAT, {"PGX_SEED_K": "0"}, _fm_runs(0, 1, 0)[:2]),
    "mid-rl": ("mid_small", P.MODE_COMPAT | P.MODE_IMAGE_RL, O.MODE_COMPAT, {}, _fm_runs(0, 0, 0, False)),
    "x-lds-dense": ("x", P.MODE_COMPAT, O.MODE_COMPAT, {}, _fm_runs(1, 1, 1)),
    "x-lds-dense-strict": ("x", P.MODE_STRICT, O.MODE_STRICT, {}, _fm_runs(1, 1, 1)[:1]),
    "x-lds-dense-unseeded": ("x", P.MODE_COMPAT, O.MODE_COMPAT, {"PGX_SEED_K": "0"}, _fm_runs(1, 1, 0)[:2]),
    "x-lds-rl": ("x", P.MODE_COMPAT | P.MODE_IMAGE_RL, O.MODE_COMPAT, {}, _fm_runs(1, 0, 0, False)),
    "xy-compat-rl": ("xy", P.MODE_COMPAT, O.MODE_COMPAT, {}, _fm_runs(1, 0, 0, False)),  # the quirk tables of COMPAT (excl_mask != 0) leave the run-length image only
    "xy-strict-dense": ("xy", P.MODE_STRICT, O.MODE_STRICT, {}, _fm_runs(1, 1, 1)[:1]),
}

_SEEN = {}  # config id -> set of pgx_timing.kernels words its runs reported (each run compared with the oracle before it counts)


@pytest.fixture(scope="module")
def cases(workdir, x_index, xy_paths, golden):
    return {"mid": V.mid_case(workdir), "mid_small": V.mid_small_case(workdir), "x": V.x_case(x_index, golden), "xy": V.xy_case(xy_paths, golden)}


def _drive(cases, cid):
    if cid in _SEEN:
        assert _SEEN[cid] is not None, "configuration %s failed earlier in this session (not run again)" % cid
        return _SEEN[cid]
    _SEEN[cid] = None  # (until it has passed)
    case_name, mode, omode, image_env, runs = CONFIGS[cid]
    case = cases[case_name]
    seen = set()
    with V.env(image_env):
        idx = P.Index(case["ri_path"], case["tags_path"], mode=mode)
        try:
            info = idx.info()
            for run_env, fm, pairs in runs:
                assert bool(info.image_in_lds) == bool(fm & P.KERNELS_FM_LDS), cid
                with V.env(run_env):
                    for min_len, min_occ in PAIRS:
                        ref = V.oracle(case, min_len, min_occ, omode)
                        res, t = V.run(idx, case["cat"], case["offs"], min_len, min_occ)
                        where = (cid, run_env, min_len, min_occ, hex(t.kernels))
                        want = fm | P.KERNELS_HEAVY
                        if pairs:
                            wide, packed, coop, s64, lce = pairs
                            want |= PR(wide, packed, coop, s64, lce == LCE and min_occ <= 1) | P.KERNELS_SIDE
                        assert t.kernels == want, (where, hex(want))
                        V.same(res, ref)
                        seen.add(int(t.kernels))
                        if case_name == "mid" and not run_env and omode == O.MODE_COMPAT:  # (STRICT: an N of a read matches nothing)
                            assert t.heavy_reads > 0, where  # the reads cut from an N run went through the heavy-read kernel
        finally:
            idx.close()
    _SEEN[cid] = seen
    return seen


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_configuration_launches_its_instance_and_equals_the_oracle(cases, cid):
    assert _drive(cases, cid)


def test_every_table_entry_was_launched(cases):
    """the union over all configurations (those not run yet in this session are run now) against pgx_kernel_variants: every instance launched,
    none launched that the product does not list; and the three launches outside the tables -- the 64-bit repeat of a chunk, the launch on the
    second stream, the heavy-read kernel -- all seen"""
    words = set()
    for cid in CONFIGS:
        words |= _drive(cases, cid)
    launched = set()
    for w in words:
        if w & P.KERNELS_FM:
            launched.add(w & P.KERNELS_FM_MASK)
            if w & P.KERNELS_FM_REDO:  # the 64-bit instance of the same kernel ran as well
                launched.add(w & P.KERNELS_FM_MASK & ~P.KERNELS_FM_NARROW)
        if w & P.KERNELS_PAIRS:
            launched.add(w & P.KERNELS_PAIRS_MASK)
    listed = set(P.kernel_variants())
    assert launched == listed, ("never launched", sorted(hex(w) for w in listed - launched), "not listed", sorted(hex(w) for w in launched - listed))
    assert any(w & P.KERNELS_FM_REDO for w in words) and any(w & P.KERNELS_SIDE for w in words) and any(w & P.KERNELS_HEAVY for w in words)
    print("kernel instances launched and equal to the oracle: %d of %d listed (+ 64-bit repeat, second-stream launch, heavy-read kernel)" % (len(launched), len(listed)))
