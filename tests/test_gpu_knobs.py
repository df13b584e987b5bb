"""The environment variables that choose other kernel code or another schedule of a persistent kernel without being meant to change a result
(README "Environment variables"): the same reads on the same mid-size PAIRS + LCE index, against the same oracle answers, under each of them;
the tag locate kernel without its pair / bucket tables on queries of every size class; the three-launch scan in a process of its own; and a
batch kept alive across the wrap of the one-pass scan's epoch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import variant_cases as V

pytestmark = pytest.mark.gpu

PAIRS = [(20, 1), (12, 1), (12, 3)]  # (min_len, min_occ): the LCE kernel at min_occ 1, the packed kernel without it at 3
MODE = P.MODE_COMPAT | P.MODE_IMAGE_PAIRS

# id -> (environment, read when the image is built?)
KNOBS = {
    "default": ({}, False),
    "no-side": ({"PGX_FM_NO_SIDE": "1"}, False),
    "no-side-byte-windows": ({"PGX_FM_NO_SIDE": "1", "PGX_FM_PACKED": "0"}, False),
    "byte-windows": ({"PGX_FM_PACKED": "0"}, False),
    "wg-per-cu-1": ({"PGX_FM_WG_PER_CU": "1"}, False),
    "wg-per-cu-max": ({"PGX_FM_WG_PER_CU": "64"}, False),  # (at or above the occupancy: every workgroup the device keeps resident)
    "wg-per-cu-1-no-side": ({"PGX_FM_WG_PER_CU": "1", "PGX_FM_NO_SIDE": "1"}, False),
    "slot-arena-0": ({"PGX_SLOT_ARENA": "0"}, False),
    "side-heavy-ext-0": ({"PGX_FM_SIDE_HEAVY_EXT": "0"}, False),
    "side-heavy-ext-64": ({"PGX_FM_SIDE_HEAVY_EXT": "64"}, False),
    "refill-min-1": ({"PGX_FM_REFILL_MIN": "1"}, True),
    "refill-min-64": ({"PGX_FM_REFILL_MIN": "64"}, True),
    "lce-max-1": ({"PGX_FM_LCE_MAX": "1"}, True),
    "lce-max-16": ({"PGX_FM_LCE_MAX": "16"}, True),
    "lce-max-128": ({"PGX_FM_LCE_MAX": "128"}, True),
    "lce-max-129": ({"PGX_FM_LCE_MAX": "129"}, True),  # above PGX_LCE_MAX_OCC: held to 128 (pgx_images.hip read_image_knobs), not refused
    "lce-max-1-refill-min-64": ({"PGX_FM_LCE_MAX": "1", "PGX_FM_REFILL_MIN": "64"}, True),
    "seed-end-k-0": ({"PGX_SEED_END_K": "0"}, True),
    "seed-end-k-3": ({"PGX_SEED_END_K": "3"}, True),
    "pairs-ext-0": ({"PGX_PAIRS_EXT": "0"}, True),
    "no-tpair": ({"PGX_NO_TPAIR": "1"}, True),
    "no-tbucket": ({"PGX_NO_TBUCKET": "1"}, True),
    "no-tpair-no-tbucket": ({"PGX_NO_TPAIR": "1", "PGX_NO_TBUCKET": "1"}, True),
}

_SHARED = {}


@pytest.fixture(scope="module")
def mid(workdir):
    return V.mid_case(workdir)


@pytest.fixture(scope="module")
def shared_index(mid):
    """one index for the knobs a run reads; the image knobs open their own"""
    idx = P.Index(mid["ri_path"], mid["tags_path"], mode=MODE)
    yield idx
    idx.close()


@pytest.mark.parametrize("knob", list(KNOBS))
def test_knob_does_not_change_the_result(mid, shared_index, knob):
    settings, image_knob = KNOBS[knob]
    with V.env(settings):
        idx = P.Index(mid["ri_path"], mid["tags_path"], mode=MODE) if image_knob else shared_index
        try:
            for min_len, min_occ in PAIRS:
                res, t = V.run(idx, mid["cat"], mid["offs"], min_len, min_occ)
                V.same(res, V.oracle(mid, min_len, min_occ))
                assert t.kernels & P.KERNELS_PAIRS, (knob, hex(t.kernels))
                # the packed reads need the list of reads the second stream serves: without that launch the kernel reads byte windows
                packed = "PGX_FM_PACKED" not in settings and "PGX_FM_NO_SIDE" not in settings
                assert bool(t.kernels & P.KERNELS_SIDE) == ("PGX_FM_NO_SIDE" not in settings), (knob, hex(t.kernels))
                assert bool(t.kernels & P.KERNELS_PAIRS_PACKED) == packed, (knob, hex(t.kernels))
                # (an LCE_MAX above the limit is accepted, not refused: the path stays on)
                assert bool(t.kernels & P.KERNELS_PAIRS_LCE) == (packed and min_occ <= 1), (knob, min_len, min_occ, hex(t.kernels))
        finally:
            if image_knob:
                idx.close()


@pytest.mark.parametrize("knob", ["default", "no-tpair", "no-tbucket", "no-tpair-no-tbucket"])
def test_tag_locate_without_its_tables_on_every_size_class(workdir, x_index, knob):
    """queries of every size class (<= 16 runs, <= 64, <= 2048, <= 16384, more; tests/test_gpu_tags_large.py) with the locate kernel going through
    tdir / tstart alone"""
    key = "tagq"
    if key not in _SHARED:
        rng = np.random.default_rng(22)
        n_runs = 70000
        vals = (rng.integers(1, 3000, n_runs).astype(np.uint64) << np.uint64(11)) | rng.integers(0, 1024, n_runs).astype(np.uint64)
        lens = rng.integers(1, 4, n_runs).astype(np.uint64)
        path = os.path.join(workdir, "knobs_huge.tags")
        P.write_compact_tags(path, vals, lens)
        total = int(lens.sum())
        st = np.array([0, 0, 5, 100, 1000, 17, 0, 3, 40000, total - 1, total - 50], dtype=np.uint64)
        en = np.array([total - 1, 60000, 5, 130, 9000, 60, 20, 3, 40100, total - 1, total - 1], dtype=np.uint64)
        extra_s = rng.integers(0, total - 1, 200).astype(np.uint64)
        extra_l = np.concatenate([rng.integers(0, 40, 100), rng.integers(40, 5000, 60), rng.integers(5000, total, 40)]).astype(np.uint64)
        st = np.concatenate([st, extra_s])
        en = np.concatenate([en, np.minimum(extra_s + extra_l, np.uint64(total - 1))])
        t = O.Tags(path, O.TAGS_COMPACT)
        want = [t.query(int(a), int(b)) for a, b in zip(st, en)]
        classes = {0 if w[0] <= 16 else 1 if w[0] <= 64 else 2 if w[0] <= 2048 else 3 if w[0] <= 16384 else 4 for w in want}
        assert classes == {0, 1, 2, 3, 4}
        _SHARED[key] = (path, st, en, want)
    path, st, en, want = _SHARED[key]
    with V.env(KNOBS[knob][0]):
        idx = P.Index(x_index[0], path)
        rn, po, pos, _ = idx.tag_query_batch(st, en)
        idx.close()
    for i, (ern, epos, _) in enumerate(want):
        assert int(rn[i]) == ern, (knob, i)
        assert np.array_equal(pos[po[i]:po[i + 1]], np.array(epos, dtype=np.uint64)), (knob, i, ern)


def _child(args, env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "scan_three_child.py")] + [str(a) for a in args],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_three_launch_scan_in_a_fresh_process(workdir, mid):
    """PGX_SCAN_THREE is read once per process: a child process runs the batch with the three-launch scans and writes the result arrays"""
    small = V.mid_small_case(workdir)
    reads, out = os.path.join(workdir, "scan3_reads.npz"), os.path.join(workdir, "scan3_out.npz")
    np.savez(reads, cat=small["cat"], offs=small["offs"])
    _child([small["ri_path"], small["tags_path"], MODE, reads, out, 1, 20, 1, 12, 3], {"PGX_SCAN_THREE": "1"})
    got = np.load(out)
    for k, (min_len, min_occ) in enumerate([(20, 1), (12, 3)]):
        ref = V.oracle(small, min_len, min_occ)
        res = {name: got["%s_%d" % (name, k)] for name in ("mem_offsets", "mems", "tag_run_counts", "pos_offsets", "positions")}
        res["mems"] = res["mems"].view(P.MEM_DTYPE).reshape(-1)
        res["n_extensions"] = int(got["n_extensions_%d" % k])
        V.same(res, ref)


def test_three_launch_scan_over_more_than_four_million_reads(workdir, x_index, golden):
    """more than 2048 blocks of 2048 items: the three-launch scan scans its block totals in a launch of their own (`!raw`).  4.3 M reads of 12
    symbols on the x index, without tags; the one-pass scans of this process against the oracle (a second of CPU time), the child against both"""
    seqs = W.load_sequences(os.path.join(golden, "x.newline_separated"))
    rng = np.random.default_rng(12)
    n, ln = 4_300_000, 12
    s = seqs[0]
    start = rng.integers(0, len(s) - ln, n)
    cat = s[start[:, None] + np.arange(ln)[None, :]].reshape(-1).copy()
    flip = rng.random(len(cat)) < 0.02
    cat[flip] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(flip.sum()))]
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(ln)
    idx = P.Index(x_index[0], x_index[1])
    b = idx.batch(cat, offs)
    b.run(10, 1)
    here = b.result()
    b.free()
    idx.close()
    ref = O.find_mems_batch(O.RIndex(x_index[0]), O.Tags(x_index[1], O.TAGS_COMPACT), cat, offs, 10, 1, threads=O.lib().orc_max_threads())
    assert np.array_equal(here["mem_offsets"], ref["mem_offsets"]) and here["mems"].tobytes() == ref["mems"].tobytes()
    assert here["n_extensions"] == ref["n_extensions"] and len(here["mems"]) > 100_000
    reads, out = os.path.join(workdir, "scan3_big_reads.npz"), os.path.join(workdir, "scan3_big_out.npz")
    np.savez(reads, cat=cat, offs=offs)
    _child([x_index[0], x_index[1], P.MODE_COMPAT, reads, out, 0, 10, 1], {"PGX_SCAN_THREE": "1"})
    got = np.load(out)
    assert np.array_equal(got["mem_offsets_0"], here["mem_offsets"])
    assert got["mems_0"].tobytes() == here["mems"].tobytes()
    assert int(got["n_extensions_0"]) == here["n_extensions"]


def test_scan_epoch_wrap_keeps_results(x_index, golden, monkeypatch):
    """pgx_scan_onepass_kernel tags its tile words with an 18-bit epoch and scan_excl clears them only when the epoch comes round.  A steady-state
    run makes ONE scan_excl call on the batch's own scan buffer (the MEM counts, find_mems_chunk; the slot scan of plan_slots is kept across runs)
    and two or three on the tag stage's, so a real wrap takes ceil(2^18 / 1) + 2^18 = 524 288 runs: at a few hundred microseconds each far
    beyond a minute.  PGX_SCAN_EPOCH0 (tests only) starts a cleared buffer 40 scans below the wrap instead; 300 runs then take every buffer
    round at least seven times.  9 000 reads are three tiles, so tiles do look back at words of the epochs before."""
    case = V.x_case(x_index, golden)
    cat, offs = W.sample_reads(case["seqs"], 9000, 150, seed=23)
    ref = O.find_mems_batch(O.RIndex(case["ri_path"]), O.Tags(case["tags_path"], O.TAGS_COMPACT), cat, offs, 10, 1, threads=O.lib().orc_max_threads())
    monkeypatch.setenv("PGX_SCAN_EPOCH0", str(0x3FFFF - 40))
    idx = P.Index(case["ri_path"], case["tags_path"])
    b = idx.batch(cat, offs)
    b.run(10, 1, P.RUN_TAGS)
    first = b.result()
    V.same(first, ref)
    keys = ("mem_offsets", "mems", "tag_run_counts", "pos_offsets", "positions")
    want = [first[k].tobytes() for k in keys]
    for i in range(300):
        b.run(10, 1, P.RUN_TAGS)
        res = b.result()
        assert [res[k].tobytes() for k in keys] == want, i
    b.free()
    idx.close()
