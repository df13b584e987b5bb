"""The two download forms of a batch result side by side: pgx_batch_result (six dense uint64 arrays) and pgx_batch_result_compact (the
compact byte stream, encoded on the device; include/pgx.h "compact result").

  python3 scripts/compact_result_bench.py [--reads 10000000] [--workload chr22|synth] [--steps 12] [--warmup 2] [--repeats 3] [--out FILE]

The workload is bench.py's (its cache directory: `bench.py --prepare`), the loop is the shape of bench.py's measure_fresh: --workers device
batches, a host thread and a stream each, every step uploads a packed batch different from the one before (three pinned host batches,
rotating), runs it with tags and downloads the result.  The two forms alternate in one process on one device (--repeats rounds of --steps
steps each, after --warmup steps per worker); reported per form: reads/s (median and every round), host ms inside the result call, bytes
over the link per step.  Then, outside the loop: ms_encode (device time of the encode, HIP events; median of five timed runs), the host
time of pgx_compact_expand over the whole batch on 1, 4 and 16 threads (block ranges, as a caller threads it; median of three) -- stated
separately, the loop does not expand -- and whether the expansion equals pgx_batch_result's arrays."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import pgx_ffi as P  # noqa: E402


def fresh_round(dbs, hbs, form, k0, steps, min_len, min_occ, timed):
    """steps k0 .. k0 + steps of the fresh loop spread over the workers; returns (seconds, host seconds inside [upload, run, result], last)"""
    workers, nb = len(dbs), len(hbs)
    phase = [[0.0, 0.0, 0.0] for _ in range(workers)]
    err, last = [], [None] * workers

    def work(w, n):
        try:
            for k in range(k0, k0 + n):
                hb = hbs[(w + k) % nb]
                t0 = time.perf_counter()
                dbs[w].upload_packed(hb.packed, hb.offs, hb.side_ids, hb.side_bytes, hb.n_side)
                t1 = time.perf_counter()
                dbs[w].run(min_len, min_occ, P.RUN_TAGS, 0)
                t2 = time.perf_counter()
                if form == "compact":
                    c = dbs[w].result_compact(copy=False)
                    last[w] = (c["n_mems"], c["n_positions"], c["n_bytes"] + 24 * (c["n_blocks"] + 1))
                else:
                    nm, npos = dbs[w].result_counts()
                    last[w] = (nm, npos, 8 * (hb.n + 1) + 48 * nm + 8 * (nm + 1) + 8 * npos)
                t3 = time.perf_counter()
                phase[w][0] += t1 - t0; phase[w][1] += t2 - t1; phase[w][2] += t3 - t2
        except Exception as e:  # noqa: BLE001
            err.append(e)

    share = [steps // workers + (1 if w < steps % workers else 0) for w in range(workers)] if timed else [steps] * workers
    th = [threading.Thread(target=work, args=(w, share[w])) for w in range(workers)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt = time.perf_counter() - t0
    if err:
        raise err[0]
    n_steps = sum(share)
    return dt, [1e3 * sum(p[i] for p in phase) / max(n_steps, 1) for i in range(3)], last


def expand_threads(c, out, threads):
    """pgx_compact_expand of the whole result on `threads` host threads, contiguous block ranges; seconds"""
    r, keep = P._compact_struct(c)
    L = P.lib()
    nb = c["n_blocks"]
    ptrs = [out[k].ctypes.data for k in ("mem_offsets", "mems", "tag_run_counts", "pos_offsets", "positions")]
    st = [P.OK] * threads

    def work(t):
        k0, k1 = nb * t // threads, nb * (t + 1) // threads
        st[t] = L.pgx_compact_expand(C.byref(r), k0, k1 - k0, *ptrs)

    th = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt = time.perf_counter() - t0
    assert all(s == P.OK for s in st), st
    del keep
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--workload", default="chr22", choices=("chr22", "synth"))
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    args = bench.parse(["--workload", a.workload, "--reads", str(a.reads)])
    wd = args.workdir or bench.cache_dir()
    os.makedirs(wd, exist_ok=True)
    with bench.DirLock(wd):
        ri, tags, cat, offs, desc, _ = bench.make_workload(args, a.workload, 0, wd, lambda: None, a.reads, args.base_len)
    idx = P.Index(ri, tags)
    hbs = [bench.HostBatch(P, cat, offs, keep_bytes=False)] + [bench.HostBatch(P, *bench.make_workload.resample(k), keep_bytes=False) for k in (1, 2)]
    n = hbs[0].n
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("compact_result_bench: %s" % desc)
    say("device: %s; %d reads of %d bp per batch, min_len %d, min_occ %d, tags; %d workers, packed uploads, %d steps per round after %d warm-up steps per worker, %d rounds per form, alternating"
        % (P.device_name(0), n, args.read_len, args.min_len, args.min_occ, a.workers, a.steps, a.warmup, a.repeats))
    dbs = [idx.batch_empty(device=0) for _ in range(a.workers)]
    forms = ("full", "compact")
    for form in forms:  # warm-up: allocations of both forms, shapes for the speculative sizing
        fresh_round(dbs, hbs, form, 0, a.warmup, args.min_len, args.min_occ, False)
    rate = {f: [] for f in forms}
    res_ms = {f: [] for f in forms}
    run_ms = {f: [] for f in forms}
    up_ms = {f: [] for f in forms}
    link = {}
    for rep in range(a.repeats):
        for form in forms:
            dt, ph, last = fresh_round(dbs, hbs, form, a.warmup + rep * a.steps, a.steps, args.min_len, args.min_occ, True)
            rate[form].append(n * a.steps / dt)
            up_ms[form].append(ph[0]); run_ms[form].append(ph[1]); res_ms[form].append(ph[2])
            link[form] = statistics.median(l[2] for l in last if l)
    say()
    say("form     reads/s (median)   every round (M reads/s)        host ms per step inside: upload   run   result     D2H MB per step")
    for form in forms:
        say("%-8s %8.1f M          %-30s %28.2f %6.2f %7.2f %14.1f" % (
            form, statistics.median(rate[form]) / 1e6, " ".join("%.1f" % (v / 1e6) for v in rate[form]), statistics.median(up_ms[form]),
            statistics.median(run_ms[form]), statistics.median(res_ms[form]), link[form] / 1e6))
    mf, mc = statistics.median(rate["full"]), statistics.median(rate["compact"])
    say("compact / full: %.2fx reads/s, %.1fx fewer bytes over the link (box-to-box spread of this loop: +-4 %%, README.md)" % (mc / mf, link["full"] / link["compact"]))
    say("against the 600 M reads/s floated in VERDICT.md: compact reaches %.0f M reads/s" % (mc / 1e6))
    # ---- outside the loop: the encode's device time, the expansion's host time
    b = dbs[0]
    hb = hbs[0]
    b.upload_packed(hb.packed, hb.offs, hb.side_ids, hb.side_bytes, hb.n_side)
    enc, enc_staged, tot = [], [], []
    for _ in range(5):
        b.run(args.min_len, args.min_occ, P.RUN_TAGS | P.RUN_TIMING, 0)
        c = b.result_compact(copy=False)
        enc.append(c["ms_encode"])
        tot.append(float(b.timing().ms_total))
        os.environ["PGX_COMPACT_STAGE"] = "1"  # the fill kernel that stages its bytes in LDS and stores 8-byte words
        enc_staged.append(b.result_compact(copy=False)["ms_encode"])
        del os.environ["PGX_COMPACT_STAGE"]
    os.environ["PGX_COMPACT_STAGE"] = "1"
    staged_bytes = b.result_compact(copy=True)["bytes"]
    del os.environ["PGX_COMPACT_STAGE"]
    c = b.result_compact(copy=True)
    full = b.result()
    m, npos = c["n_mems"], c["n_positions"]
    say()
    say("one batch: %d MEMs, %d positions; full form %.1f MB, compact %.1f MB (%d blocks; %.2f bytes per read, %.2f per MEM + position)"
        % (m, npos, (8 * (n + 1) + 56 * m + 8 + 8 * npos) / 1e6, (c["n_bytes"] + 24 * (c["n_blocks"] + 1)) / 1e6, c["n_blocks"], c["n_bytes"] / n,
           c["n_bytes"] / max(m + npos, 1)))
    say("ms_encode (sizing kernel + scan + fill kernel, HIP events): median %.3f ms of %s; the run itself: ms_total %.3f ms" % (
        statistics.median(enc), " ".join("%.3f" % v for v in enc), statistics.median(tot)))
    say("ms_encode with PGX_COMPACT_STAGE=1 (LDS stage, 8-byte stores): median %.3f ms of %s; same bytes: %s" % (
        statistics.median(enc_staged), " ".join("%.3f" % v for v in enc_staged), bool(np.array_equal(staged_bytes, c["bytes"]))))
    out = P.compact_expand_arrays(c)
    expand_threads(c, out, 16)  # (first touch of the output arrays)
    same = all(np.asarray(out[k]).tobytes() == np.asarray(full[k]).tobytes() for k in ("mem_offsets", "mems", "tag_run_counts", "pos_offsets", "positions"))
    say("pgx_compact_expand == pgx_batch_result (all five arrays): %s" % same)
    for threads in (1, 4, 16):
        ts = [expand_threads(c, out, threads) for _ in range(3)]
        say("host expansion, %2d threads: median %.1f ms of %s (%.0f M reads/s)" % (threads, 1e3 * statistics.median(ts), " ".join("%.1f" % (1e3 * t) for t in ts),
                                                                                  n / statistics.median(ts) / 1e6))
    say(json.dumps({"reads_per_s": {f: statistics.median(rate[f]) for f in forms}, "result_ms": {f: statistics.median(res_ms[f]) for f in forms},
                    "d2h_bytes": link, "ms_encode": statistics.median(enc), "ms_encode_staged": statistics.median(enc_staged), "expand_equals_full": bool(same)}))
    for d in dbs:
        d.free()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
