"""bench.py's plain run and --full, --dump-outputs (the sampled results of the last timed step) and the cache of synthetic indexes.
CPU tier: the option rules and the dump format on a made-up result; GPU tier: two runs of the same arguments dump the same arrays, and
those arrays are what the oracle computes for the sampled reads."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _run(argv, env=None):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=600, env=e)


@pytest.mark.parametrize("flag", ["--overlap", "--batch-sweep", "--pcie"])
def test_extra_legs_need_full(flag):
    r = _run([flag, "--stub-workload"])
    assert r.returncode == 2 and "is a --full measurement" in r.stderr
    assert _run([flag, "--full", "--stub-workload"]).returncode == 0


def test_plain_and_full_parse():
    a = bench.parse(["--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_cache_dir(monkeypatch, tmp_path):
    monkeypatch.delenv("PGX_BENCH_CACHE", raising=False)
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path))
    d = bench.cache_dir()
    assert os.path.dirname(d) == os.path.join(str(tmp_path), "pgx_bench") and d == bench.cache_dir()
    monkeypatch.setenv("PGX_BENCH_CACHE", str(tmp_path / "mine"))
    assert bench.cache_dir() == str(tmp_path / "mine")


def _fake_result(n, seed=3):
    """a pgx_batch_result-shaped dict: n reads, 0..4 MEMs each, 0..3 positions per MEM"""
    import pgx_ffi as P

    rng = np.random.default_rng(seed)
    mc = rng.integers(0, 5, size=n)
    mo = np.concatenate(([0], np.cumsum(mc))).astype(np.uint64)
    m = int(mo[-1])
    mems = np.zeros(m, dtype=P.MEM_DTYPE)
    mems["start"] = rng.integers(0, 150, size=m)
    mems["end"] = mems["start"] + rng.integers(20, 40, size=m).astype(np.uint64)
    mems["bwt_start"] = rng.integers(0, 1 << 40, size=m)
    mems["size"] = rng.integers(1, 9, size=m)
    pc = rng.integers(0, 4, size=m)
    po = np.concatenate(([0], np.cumsum(pc))).astype(np.uint64)
    return dict(n_extensions=12345, n_tag_overflow=0, mem_offsets=mo, mems=mems, tag_run_counts=rng.integers(0, 7, size=m).astype(np.uint64),
                pos_offsets=po, positions=rng.integers(0, 1 << 45, size=int(po[-1])).astype(np.uint64))


def _load(d, prefix=""):
    return {f[len(prefix):-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.startswith(prefix) and f.endswith(".npy")}


def test_dump_outputs_is_a_fixed_sample_of_the_result(tmp_path, built):
    res = _fake_result(200_000)
    bench.dump_outputs(str(tmp_path / "a"), res)
    bench.dump_outputs(str(tmp_path / "b"), res)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == ["mem_counts", "mems", "pos_counts", "positions", "reads", "tag_run_counts", "totals"]
    assert all(v.dtype == np.float64 for v in a.values()) and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a"))) <= bench.DUMP_BYTES
    reads = a["reads"].astype(np.int64)
    assert len(reads) == bench.DUMP_READS and np.all(np.diff(reads) > 0)
    # every array against the result, read by read
    mo, po = res["mem_offsets"].astype(np.int64), res["pos_offsets"].astype(np.int64)
    ids = np.concatenate([np.arange(mo[r], mo[r + 1]) for r in reads])
    assert np.array_equal(a["mem_counts"], mo[reads + 1] - mo[reads])
    m = res["mems"][ids]
    assert np.array_equal(a["mems"], np.stack([m["start"], m["end"], m["bwt_start"], m["size"]], axis=1).astype(np.float64))
    assert np.array_equal(a["tag_run_counts"], res["tag_run_counts"][ids])
    assert np.array_equal(a["pos_counts"], po[ids + 1] - po[ids])
    pos = np.concatenate([res["positions"][po[i]:po[i + 1]] for i in ids])
    assert np.array_equal(a["positions"], pos.astype(np.float64))
    assert list(a["totals"]) == [200_000, float(mo[-1]), float(po[-1]), 12345.0]


def test_dump_outputs_halves_the_sample_to_fit(tmp_path, built, monkeypatch):
    res = _fake_result(50_000)
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    d = bench.dump_outputs(str(tmp_path), res, prefix="p_")
    assert d["reads_sampled"] < min(50_000, bench.DUMP_READS)
    assert sum(os.path.getsize(os.path.join(str(tmp_path), f)) - 128 for f in d["files"]) <= 1 << 20  # (128: the .npy header)
    assert _load(str(tmp_path), "p_")["totals"][0] == 50_000


@pytest.mark.gpu
def test_dump_outputs_of_a_bench_run_equal_the_oracle(tmp_path, built, golden):
    """two plain runs of the same arguments dump the same arrays, and those are the oracle's answer for the sampled reads"""
    import oracle_ffi as O
    import pgx_workload as W

    argv = ["--workload", "x", "--reads", "50000", "--steps", "3", "--warmup", "1", "--workdir", str(tmp_path / "wd")]
    lines = []
    for k in range(2):
        r = _run(argv + ["--dump-outputs", str(tmp_path / ("d%d" % k))])
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    a, b = _load(str(tmp_path / "d0")), _load(str(tmp_path / "d1"))
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert lines[0]["steps"] == 3 and lines[0]["ms_per_step"] > 0 and "parity_sample" not in lines[0] and "cpu_baseline" not in lines[0]
    assert a["totals"][0] == 50000 and a["totals"][1] == lines[0]["mems_per_step"] and a["totals"][2] == lines[0]["positions_per_step"]
    # the same reads as the bench samples them (x: seed 44, rank 0), the sampled ones under the oracle
    cat, offs = W.sample_reads(W.load_sequences(os.path.join(golden, "x.newline_separated")), 50000, 150, seed=44)
    reads = a["reads"].astype(np.int64)
    sub = np.concatenate([cat[int(offs[r]):int(offs[r + 1])] for r in reads])
    soffs = np.arange(len(reads) + 1, dtype=np.uint64) * np.uint64(150)
    wd = str(tmp_path / "wd")
    ref = O.find_mems_batch(O.RIndex(os.path.join(wd, "x.ri")), O.Tags(os.path.join(wd, "x.compact.tags"), O.TAGS_COMPACT), sub, soffs, 10, 1)
    mo = ref["mem_offsets"].astype(np.int64)
    assert np.array_equal(a["mem_counts"], np.diff(mo))
    m = ref["mems"]
    assert np.array_equal(a["mems"], np.stack([m["start"], m["end"], m["bwt_start"], m["size"]], axis=1).astype(np.float64))
    assert np.array_equal(a["tag_run_counts"], ref["tag_run_counts"].astype(np.float64))
    assert np.array_equal(a["pos_counts"], np.diff(ref["pos_offsets"].astype(np.int64)))
    assert np.array_equal(a["positions"], ref["positions"].astype(np.float64))
