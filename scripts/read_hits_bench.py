"""pgx_batch_read_hits on bench.py's workloads: every read scored against every sequence, on the device.

  python3 scripts/read_hits_bench.py [--workload synth|chr22] [--reads N] [--haps H] [--base-len L] [--steps 3] [--no-cli] [--out FILE]

One batch of --reads 150-bp reads of the workload (bench.py's cache directory and reads), min_len 20 / min_occ 1, run with
PGX_RUN_TAGS | PGX_RUN_TIMING, then pgx_batch_locate(PGX_LOCATE_SEQ_SETS) and pgx_batch_read_hits.  One warm-up call, then the median of
--steps, for:
  ms_hits      device events around the one kernel launch, for flags 0, PGX_HITS_BEST_SETS and PGX_HITS_BEST_SETS | PGX_HITS_SCORES
  bytes        what the stage must move with flags 0: 32 + 8 W per MEM and 8 per read in, 40 per read out; over ms_hits as a share of 8 TB/s
  copy floor   a device-to-device copy of that many bytes, timed with events in this invocation
  ms_locate    the SETS locate the stage follows (what it adds to a step), and the find_mems step itself
  sets check   the MEMs with an all-zero set against the locate's own count of MEMs it did not locate: a difference means the locate did not
               cover the batch (one launch of its set kernel takes at most 2^32 x 16 values), and the run ends with status 1 after its rows
  downloads    what a caller has to bring to the host today (the sets, the MEM array and the offsets) against the 40-byte records: copies of
               those sizes from device memory into pinned host memory, timed with events
  CLI          wall time of find_mems --hits F --hits-only against the default text output (stdout to /dev/null, --quiet), alternated; the
               pipeline wall the program reports itself (PGX_CLI_STATS) next to the wall of the whole process, which includes loading the index
Rows are JSON lines; --out also appends them to a file."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import pgx_ffi as P  # noqa: E402

HBM_PEAK = 8.0e12
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")


def median(xs):
    return float(np.median(xs))


_hip = None


def hip():
    """the HIP runtime libpgx.so runs on (already in the process), through ctypes"""
    global _hip
    if _hip is None:
        import ctypes as C

        P.lib()
        P.device_count()
        with open("/proc/self/maps") as f:
            paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line}, key=lambda q: "/torch/" in q)
        _hip = C.CDLL(paths[0])
        vp, sz = C.c_void_p, C.c_size_t
        for name, argtypes in (("hipMalloc", [C.POINTER(vp), sz]), ("hipFree", [vp]), ("hipHostMalloc", [C.POINTER(vp), sz, C.c_uint]), ("hipHostFree", [vp]),
                               ("hipMemset", [vp, C.c_int, sz]), ("hipMemcpyAsync", [vp, vp, sz, C.c_int, vp]), ("hipEventCreate", [C.POINTER(vp)]),
                               ("hipEventRecord", [vp, vp]), ("hipEventSynchronize", [vp]), ("hipEventElapsedTime", [C.POINTER(C.c_float), vp, vp]),
                               ("hipEventDestroy", [vp]), ("hipDeviceSynchronize", [])):
            fn = getattr(_hip, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
    return _hip


def copy_ms(nbytes, to_host, steps):
    """ms of a copy of nbytes out of device memory (to device memory, or to pinned host memory), between two events on the null stream:
    one warm-up, the median of `steps`"""
    import ctypes as C

    H = hip()

    def ok(rc):
        if rc != 0:
            raise SystemExit("HIP call failed in copy_ms: %d" % rc)

    nbytes = max(int(nbytes), 1)
    src, dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(H.hipMalloc(C.byref(src), nbytes))
    ok(H.hipMemset(src, 1, nbytes))
    ok(H.hipHostMalloc(C.byref(dst), nbytes, 0) if to_host else H.hipMalloc(C.byref(dst), nbytes))
    ok(H.hipEventCreate(C.byref(e0)))
    ok(H.hipEventCreate(C.byref(e1)))
    ms = []
    for i in range(steps + 1):
        ok(H.hipEventRecord(e0, None))
        ok(H.hipMemcpyAsync(dst, src, nbytes, 2 if to_host else 3, None))
        ok(H.hipEventRecord(e1, None))
        ok(H.hipEventSynchronize(e1))
        t = C.c_float()
        ok(H.hipEventElapsedTime(C.byref(t), e0, e1))
        if i:
            ms.append(t.value)
    ok(H.hipDeviceSynchronize())
    H.hipEventDestroy(e0)
    H.hipEventDestroy(e1)
    (H.hipHostFree if to_host else H.hipFree)(dst)
    H.hipFree(src)
    return median(ms)


def cli_walls(ri, tags, cat, offs, steps, emit):
    with tempfile.TemporaryDirectory() as td:
        reads = os.path.join(td, "reads.txt")
        nl = np.full(1, 10, np.uint8)
        with open(reads, "wb") as f:
            step = 1 << 16
            for r0 in range(0, len(offs) - 1, step):
                r1 = min(r0 + step, len(offs) - 1)
                lens = np.diff(offs[r0:r1 + 1].astype(np.int64))
                block = np.asarray(cat[int(offs[r0]):int(offs[r1])], dtype=np.uint8)
                if len(lens) and (lens == lens[0]).all():
                    f.write(np.concatenate([block.reshape(len(lens), int(lens[0])), np.full((len(lens), 1), 10, np.uint8)], axis=1).tobytes())
                else:
                    for r in range(r0, r1):
                        f.write(bytes(cat[int(offs[r]):int(offs[r + 1])]) + nl.tobytes())
        hits_file = os.path.join(td, "hits.tsv")
        forms = (("text (default)", ["--quiet"]), ("--hits F --hits-only", ["--quiet", "--hits", hits_file, "--hits-only"]))
        walls = {name: [] for name, _ in forms}
        pipes = {name: [] for name, _ in forms}
        env = dict(os.environ, PGX_CLI_STATS="1")
        for i in range(steps + 1):  # (the first round warms the page cache)
            for name, extra in forms:
                t0 = time.time()
                with open(os.devnull, "wb") as null:
                    r = subprocess.run([CLI, ri, tags, reads, "20", "1"] + extra, stdout=null, stderr=subprocess.PIPE, env=env, timeout=900)
                wall = time.time() - t0
                if r.returncode != 0:
                    raise SystemExit("find_mems failed: " + r.stderr.decode()[-500:])
                pipe = [l for l in r.stderr.decode().split("\n") if l.startswith("[find_mems] pipeline ")]
                if i:
                    walls[name].append(wall)
                    pipes[name].append(float(pipe[0].split()[2]) if pipe else float("nan"))
        hits_bytes = os.path.getsize(hits_file)
        for name, _ in forms:
            emit(dict(cli=name, reads=len(offs) - 1, process_wall_s=round(median(walls[name]), 3), pipeline_wall_s=round(median(pipes[name]), 3),
                      pipeline_all=[round(x, 3) for x in pipes[name]], reads_per_s_pipeline=round((len(offs) - 1) / median(pipes[name]), 1)))
        emit(dict(cli="hits file", bytes=hits_bytes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synth", choices=("chr22", "synth"))
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--haps", type=int, default=None)
    ap.add_argument("--base-len", type=int, default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    argv = ["--workload", a.workload]
    for name, v in (("--reads", a.reads), ("--haps", a.haps), ("--base-len", a.base_len)):
        if v is not None:
            argv += [name, str(v)]
    args = bench.parse(argv)

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    wd = args.workdir or bench.cache_dir()
    os.makedirs(wd, exist_ok=True)
    with bench.DirLock(wd):
        ri, tags, cat, offs, desc, _ = bench.make_workload(args, a.workload, 0, wd, lambda: None, args.reads, args.base_len)
    idx = P.Index(ri, tags)
    info = idx.info()
    b = P.Batch(idx, cat, offs)
    b.run(20, 1, P.RUN_TAGS | P.RUN_TIMING)  # (the first run builds the LCE image where the index has one)
    b.run(20, 1, P.RUN_TAGS | P.RUN_TIMING)
    step_ms = b.timing().ms_total
    n_reads = len(offs) - 1
    n_mems = b.counts()[0]
    ms_loc = []
    for i in range(a.steps + 1):
        b.locate(P.LOCATE_SEQ_SETS)
        if i:
            ms_loc.append(b.device_locations()["ms_locate"])
    w = b.device_locations()["set_words"]
    emit(dict(workload=desc, reads=n_reads, n_mems=int(n_mems), n_sequences=int(info.n_sequences), set_words=w, bwt_size=int(info.bwt_size),
              find_mems_step_ms=round(step_ms, 3), ms_locate_sets=round(median(ms_loc), 3), ms_locate_all=[round(x, 3) for x in ms_loc]))
    # the sets themselves: a MEM the locate counts as located has at least one sequence.  Anything else means that the locate did not finish its
    # work on this batch, and every figure below would describe hits on incomplete sets
    loc = b.locations()
    empty = int((~loc["sets"].any(axis=1)).sum())
    n_not = loc["n_not_located"]
    incomplete = empty != n_not
    emit(dict(check="sets", n_not_located=loc["n_not_located"], mems_with_an_empty_set=empty, complete=not incomplete))
    del loc
    model = (32 + 8 * w) * n_mems + 8 * n_reads + 40 * n_reads
    for flags, name in ((0, "records"), (P.HITS_BEST_SETS, "records + best sets"), (P.HITS_BEST_SETS | P.HITS_SCORES, "records + best sets + scores")):
        ms = []
        for i in range(a.steps + 1):
            P._check(b.L.pgx_batch_read_hits(b.b, flags, None))
            if i:
                ms.append(b.device_hits()["ms_hits"])
        m = median(ms)
        row = dict(form=name, flags=flags, ms_hits=round(m, 4), ms_all=[round(x, 4) for x in ms], reads_per_s=round(n_reads / (m * 1e-3), 1),
                   vs_locate_sets=round(m / median(ms_loc), 4), vs_find_mems_step=round(m / step_ms, 4))
        if flags == 0:
            floor = copy_ms(model, False, a.steps)
            row.update(model_bytes=int(model), hbm_fraction=round(model / (m * 1e-3) / HBM_PEAK, 4), d2d_copy_ms=round(floor, 4), vs_d2d_copy=round(m / floor, 2))
        emit(row)
    today = n_mems * (8 * w + 32) + 8 * (n_reads + 1)
    down_today, down_hits = copy_ms(today, True, a.steps), copy_ms(40 * n_reads, True, a.steps)
    emit(dict(download="sets + MEMs + offsets (today)", bytes=int(today), ms=round(down_today, 3)))
    emit(dict(download="40-byte records", bytes=40 * n_reads, ms=round(down_hits, 3), ratio=round(down_today / down_hits, 2)))
    h = b.hits()["hits"]
    emit(dict(hits="summary", reads_with_a_best=int((h["best_score"] > 0).sum()), unique_best=int((h["n_best"] == 1).sum()),
              mean_best_score=round(float(h["best_score"].mean()), 2), mean_covered=round(float(h["covered"].mean()), 2)))
    b.free()
    idx.close()
    if incomplete:
        raise SystemExit("the set locate left %d sets empty but counts %d MEMs as not located: the figures above are not those of complete sets" % (empty, n_not))
    if not a.no_cli:
        cli_walls(ri, tags, cat, offs, a.steps, emit)


if __name__ == "__main__":
    main()
