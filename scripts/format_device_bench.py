"""The two ways of making the find_mems text side by side: --format host (result arrays or the compact stream over the link, formatter threads
on the host) and --format device (pgx_batch_format: the device writes the text, the host downloads and writes it).

  python3 scripts/format_device_bench.py [--reads 16000000] [--batch-reads 10000000] [--repeats 3] [--out FILE] [--skip cli|batch|api ...] [--base-len N]

The workload is bench.py's default (its cache directory: `bench.py --prepare`; n = 640 M, min_len 20, min_occ 1, tags on), the reads are sampled
once (--reads of 150) and written one per line, as scripts/cli_e2e.py does.  Three comparisons, every pair alternating in one invocation:
  (a) cli    the CLI end to end to /dev/null, default pipeline shape, PGX_CLI_STATS=1: wall of the process, wall of the pipeline (the CLI's own
             figure: without loading the index), the stage seconds of the last run of each form;
  (b) batch  one batch of --batch-reads reads through the CLI with one worker (--streams 1 --batch N): what a single fresh batch pays behind its
             run -- host: compact download + expansion + formatting (the `download` and `format` stages), device: pgx_batch_format, whose text
             the writer takes where it is (`format`) --, and the same batch through the API in this process: pgx_batch_result_compact + pgx_compact_expand on 16
             threads (the formatting itself exists only in the CLI) against pgx_batch_format;
  (c) api    in this process, the same batch: ms_format (HIP events around the length and fill passes), a pinned device-to-host hipMemcpy of
             exactly n_bytes, and a device-to-device copy of the same bytes -- what the kernels are to be compared with.
Every figure is a median with its minimum and maximum."""
import argparse
import ctypes as C
import os
import re
import statistics
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import pgx_ffi as P  # noqa: E402

EXE = os.path.join(ROOT, "pangenome-index_amd", "find_mems")


def mmm(v, fmt="%.3f"):
    return (fmt + " (" + fmt + " - " + fmt + ")") % (statistics.median(v), min(v), max(v))


def write_reads(cat, n, read_len, path):
    lines = np.full((n, read_len + 1), 10, dtype=np.uint8)  # one read per line
    lines[:, :read_len] = cat[:n * read_len].reshape(n, read_len)
    lines.tofile(path)


def run_cli(ri, tags, path, min_len, min_occ, extra):
    """one CLI run to /dev/null: (wall seconds of the process, wall seconds of its pipeline, its stage seconds, its stats lines)"""
    t0 = time.perf_counter()
    with open(os.devnull, "wb") as out:
        r = subprocess.run([EXE, ri, tags, path, str(min_len), str(min_occ), "--quiet"] + extra, stdout=out, stderr=subprocess.PIPE, env=dict(os.environ, PGX_CLI_STATS="1"))
    dt = time.perf_counter() - t0
    err = r.stderr.decode(errors="replace")
    if r.returncode != 0:
        raise SystemExit("find_mems %s failed (%d): %s" % (" ".join(extra), r.returncode, err[-400:]))
    stats = [l for l in err.split("\n") if l.startswith("[find_mems]")]
    g = re.search(r"pipeline ([0-9.]+) s wall", stats[0])
    stages = {k: float(v) for k, v in re.findall(r"(parse|upload|run|download|format|write) ([0-9.]+)", stats[0])}
    return dt, float(g.group(1)), stages, stats


def alternate(say, title, ri, tags, path, n, min_len, min_occ, forms, repeats):
    say()
    say(title)
    wall = {f: [] for f in forms}
    pipe = {f: [] for f in forms}
    stage = {f: {} for f in forms}
    last = {}
    for _ in range(repeats):
        for f, extra in forms.items():
            dt, pw, st, lines = run_cli(ri, tags, path, min_len, min_occ, extra)
            wall[f].append(dt)
            pipe[f].append(pw)
            for k, v in st.items():
                stage[f].setdefault(k, []).append(v)
            last[f] = lines
    say("form      process wall s              pipeline wall s             M reads/s by pipeline wall")
    for f in forms:
        say("%-9s %-27s %-27s %s" % (f, mmm(wall[f]), mmm(pipe[f]), mmm([n / p / 1e6 for p in pipe[f]], "%.1f")))
    for f in forms:
        say("%-9s busy seconds per stage, median (min - max): %s" % (f, "; ".join("%s %s" % (k, mmm(v)) for k, v in stage[f].items())))
    for f in forms:
        for l in last[f]:
            say("    last %s run: %s" % (f, l))
    return pipe, stage


def expand_threads(c, out, threads):
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
    ap.add_argument("--reads", type=int, default=16_000_000)
    ap.add_argument("--batch-reads", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip", nargs="*", default=[], choices=("cli", "batch", "api"))
    ap.add_argument("--base-len", type=int, default=None, help="a smaller index than the default workload's (rehearsals)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.batch_reads = min(a.batch_reads, a.reads)
    args = bench.parse(["--workload", "chr22", "--reads", str(a.reads)] + (["--base-len", str(a.base_len)] if a.base_len else []))
    wd = args.workdir or bench.cache_dir()
    os.makedirs(wd, exist_ok=True)
    with bench.DirLock(wd):
        ri, tags, cat, offs, desc, _ = bench.make_workload(args, "chr22", 0, wd, lambda: None, a.reads, args.base_len)
    rl = args.read_len
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("format_device_bench: %s" % desc)
    say("device: %s; reads of %d bp, min_len %d, min_occ %d, tags; every pair of forms alternates, %d runs each; figures are median (min - max)"
        % (P.device_name(0), rl, args.min_len, args.min_occ, a.repeats))
    with tempfile.TemporaryDirectory(prefix="pgx_format_bench_") as tmp:
        if "cli" not in a.skip:
            path = os.path.join(tmp, "reads.txt")
            write_reads(cat, a.reads, rl, path)
            alternate(say, "(a) CLI end to end, %d reads to /dev/null, default pipeline (three workers, batches of 2^18 reads)" % a.reads, ri, tags, path, a.reads,
                      args.min_len, args.min_occ, {"host": ["--format", "host"], "device": ["--format", "device"]},
                      a.repeats)
            os.unlink(path)
        if "batch" not in a.skip:
            path = os.path.join(tmp, "reads_batch.txt")
            write_reads(cat, a.batch_reads, rl, path)
            one = ["--streams", "1", "--batch", str(a.batch_reads)]
            pipe, stage = alternate(say, "(b) one fresh batch of %d reads through the CLI, one worker (--streams 1 --batch %d)" % (a.batch_reads, a.batch_reads), ri, tags, path,
                                    a.batch_reads, args.min_len, args.min_occ,
                                    {"compact": ["--format", "host", "--result", "compact"] + one, "device": ["--format", "device"] + one}, a.repeats)
            behind = {f: [d + g for d, g in zip(stage[f]["download"], stage[f]["format"])] for f in stage}
            say("behind the run, per batch (download + format stages): compact + host expansion + host formatting %s s; pgx_batch_format %s s (the first call of a batch allocates its pinned text buffers)"
                % (mmm(behind["compact"]), mmm(behind["device"])))
            os.unlink(path)
    if "api" in a.skip:
        return finish(a, lines)
    # ---- in this process: one batch of --batch-reads reads
    n = a.batch_reads
    idx = P.Index(ri, tags)
    b = idx.batch_empty(device=0)
    b.upload(cat[:n * rl], offs[:n + 1])
    b.run(args.min_len, args.min_occ, P.RUN_TAGS | P.RUN_TIMING, 0)
    for _ in range(2):  # (warm-up: code objects, and both sets of pinned text buffers)
        b.format(copy=False)
    c = b.result_compact(copy=False)
    out = P.compact_expand_arrays(c)
    expand_threads(c, out, 16)  # (first touch of the output arrays)
    t_fmt, t_comp, t_exp, ms_fmt, ms_run = [], [], [], [], []
    for _ in range(max(a.repeats, 3)):
        b.run(args.min_len, args.min_occ, P.RUN_TAGS | P.RUN_TIMING, 0)
        ms_run.append(float(b.timing().ms_total))
        t0 = time.perf_counter()
        tx = b.format(copy=False)
        t1 = time.perf_counter()
        c = b.result_compact(copy=False)
        t2 = time.perf_counter()
        t_fmt.append(1e3 * (t1 - t0)); t_comp.append(1e3 * (t2 - t1)); ms_fmt.append(tx["ms_format"])
        t_exp.append(1e3 * expand_threads(c, out, 16))
    nb = tx["n_bytes"]
    say()
    say("(b) the same batch through the API: %d reads, %d MEMs, %d positions; text %.1f MB (%.1f bytes per read), compact stream %.1f MB; the run itself: ms_total %s ms"
        % (n, c["n_mems"], c["n_positions"], nb / 1e6, nb / n, c["n_bytes"] / 1e6, mmm(ms_run)))
    say("    pgx_batch_format, host ms inside the call (kernels + download of the text):                  %s" % mmm(t_fmt, "%.1f"))
    say("    pgx_batch_result_compact, host ms inside the call (encode + download of the stream):         %s" % mmm(t_comp, "%.1f"))
    say("    pgx_compact_expand on 16 threads, host ms (the formatting that follows exists only in the CLI): %s" % mmm(t_exp, "%.1f"))
    # ---- (c) the kernels against plain copies of the same bytes
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    d0, d1 = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d0), nb) == 0 and hip.hipMalloc(C.byref(d1), nb) == 0
    pin = C.c_void_p()
    P._check(P.lib().pgx_host_alloc(nb, C.byref(pin)))
    d2h, d2d = [], []
    for k in range(6):  # (the first round warms both paths up and is dropped)
        t0 = time.perf_counter()
        assert hip.hipMemcpy(pin, d0, nb, 2) == 0 and hip.hipDeviceSynchronize() == 0
        t1 = time.perf_counter()
        assert hip.hipMemcpy(d1, d0, nb, 3) == 0 and hip.hipDeviceSynchronize() == 0
        t2 = time.perf_counter()
        if k:
            d2h.append(1e3 * (t1 - t0)); d2d.append(1e3 * (t2 - t1))
    say()
    say("(c) the same process, the %d bytes of that text:" % nb)
    say("    ms_format (HIP events: length pass + fill pass)   %s ms  = %.0f GB/s of text" % (mmm(ms_fmt), nb / statistics.median(ms_fmt) / 1e6))
    say("    pinned device-to-host hipMemcpy of n_bytes         %s ms  = %.1f GB/s" % (mmm(d2h), nb / statistics.median(d2h) / 1e6))
    say("    device-to-device hipMemcpy of n_bytes              %s ms  = %.0f GB/s" % (mmm(d2d), nb / statistics.median(d2d) / 1e6))
    say("    ms_format / pinned download: %.3f; ms_format / device-to-device copy: %.1f" % (statistics.median(ms_fmt) / statistics.median(d2h),
                                                                                         statistics.median(ms_fmt) / statistics.median(d2d)))
    P.lib().pgx_host_free(pin)
    hip.hipFree(d0); hip.hipFree(d1)
    b.free()
    idx.close()
    finish(a, lines)


def finish(a, lines):
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
