"""Index build on the device against the host builder (GPU box):
    python3 -u scripts/build_index_device_bench.py [--sizes 4000000,40000000] [--haps 8] [--reps 3] [--out profiles/build_index_device_bench.txt]

Texts: the synthetic pangenomes of bench.py (synth_pangenome_text, base_len x haps x 2 strands: 4 M -> n = 64 M, 40 M -> the chr22-scale
640 M), taken from the bench's cache directory when they are there, else written to a temporary directory.  Per size, in one process:
one warm-up of the device call, then the device call (pgx_build_index_from_text_device) and the host call (pgx_workload.build_index_from_text
with its defaults: the text dealt into eight texts above 64 MB, pgx_build_index_from_texts, host threads as they default) alternate `reps`
times.  Recorded: whole-call wall times, the six stage values of the device call, cmp of both output files, and -- from a child process
with PGX_BUILD_TIMING=1, so that the per-pass event synchronisation stays out of the timed calls -- the device bytes allocated against the
formula and the HIP-event time of the radix passes, next to a device-to-device copy of the same bytes in the same run."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))
sys.path.insert(0, ROOT)

import pgx_ffi as P
import pgx_workload as W

PEAK_TBS = 8.0  # MI355X HBM3E


def text_for(base_len, haps, tmp):
    import bench

    name = "synth_%d_%d" % (base_len, haps)
    cached = os.path.join(os.environ.get("PGX_BENCH_CACHE") or bench.cache_dir(), name + ".txt")
    if os.path.exists(cached):
        return cached, "bench cache"
    path = os.path.join(tmp, name + ".txt")
    t0 = time.time()
    W.synth_pangenome_text(path, base_len=base_len, n_hap=haps, seed=45)
    return path, "written in %.1f s" % (time.time() - t0)


def same(a, b):
    return subprocess.run(["cmp", "-s", a, b]).returncode == 0


def dtod_rate(n_bytes):
    """GB/s of hipMemcpy device-to-device that reads and writes n_bytes in all (half of it each way), through the HIP runtime itself"""
    import ctypes as C

    hip = C.CDLL("libamdhip64.so")
    half = max(1, n_bytes // 2)
    a, b = C.c_void_p(), C.c_void_p()

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: hipError %d" % (what, rc))

    ok(hip.hipMalloc(C.byref(a), C.c_size_t(half)), "hipMalloc")
    ok(hip.hipMalloc(C.byref(b), C.c_size_t(half)), "hipMalloc")
    try:
        ok(hip.hipMemset(a, 0, C.c_size_t(half)), "hipMemset")
        ok(hip.hipMemcpy(b, a, C.c_size_t(half), 3), "hipMemcpy")  # hipMemcpyDeviceToDevice; the first one warms up
        ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
        t0 = time.perf_counter()
        for _ in range(3):
            ok(hip.hipMemcpy(b, a, C.c_size_t(half), 3), "hipMemcpy")
        ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
        dt = time.perf_counter() - t0
    finally:
        hip.hipFree(a)
        hip.hipFree(b)
    return 2.0 * half * 3 / dt / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4000000,40000000")
    ap.add_argument("--haps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "build_index_device_bench.txt"))
    ap.add_argument("--pass-timing", default=None, help="(child) one device call on this text with the pass timer on")
    a = ap.parse_args()
    if a.pass_timing:
        with tempfile.TemporaryDirectory() as d:
            P.build_index_from_text_device(a.pass_timing, os.path.join(d, "t.rl_bwt"), os.path.join(d, "t.ri"))
        return
    out = open(a.out, "w")

    def say(s):
        out.write(s + "\n")
        out.flush()
        print(s, flush=True)

    say("# index build: device call against host call; %s; %d repeats after one device warm-up; times in seconds unless marked" % (P.device_name(0), a.reps))
    say("# baseline (host call): pgx_workload.build_index_from_text with its defaults -- above 64 MB the text dealt into eight texts and pgx_build_index_from_texts, host threads as they default")
    with tempfile.TemporaryDirectory() as tmp:
        for base_len in [int(x) for x in a.sizes.split(",")]:
            text, how = text_for(base_len, a.haps, tmp)
            n = os.path.getsize(text)
            say("\n## base_len %d x %d haplotypes x 2 strands: n = %d symbols (text: %s)" % (base_len, a.haps, n, how))
            drl, dri = os.path.join(tmp, "dev.rl_bwt"), os.path.join(tmp, "dev.ri")
            t0 = time.time()
            P.build_index_from_text_device(text, drl, dri)
            say("device warm-up            %8.2f" % (time.time() - t0))
            dev, cpu = [], []
            for r in range(a.reps):
                t0 = time.time()
                ms = P.build_index_from_text_device(text, drl, dri)
                dev.append(time.time() - t0)
                say("device call %d             %8.2f   stages ms: %s" % (r, dev[-1], "  ".join("%s %.1f" % (k, ms[k]) for k in P.BUILD_INDEX_DEVICE_STAGES)))
                t0 = time.time()
                cri, _, crl = W.build_index_from_text(text, os.path.join(tmp, "cpu"), "cpu", with_tags=False)
                cpu.append(time.time() - t0)
                say("host call %d               %8.2f" % (r, cpu[-1]))
            say("cmp .rl_bwt: %s   cmp .ri: %s   (sizes %d, %d bytes)" % ("equal" if same(drl, crl) else "DIFFERENT", "equal" if same(dri, cri) else "DIFFERENT",
                                                                          os.path.getsize(drl), os.path.getsize(dri)))
            say("device %.2f .. %.2f (median %.2f)   host %.2f .. %.2f (median %.2f)   host median / device median = %.1f"
                % (min(dev), max(dev), sorted(dev)[len(dev) // 2], min(cpu), max(cpu), sorted(cpu)[len(cpu) // 2], sorted(cpu)[len(cpu) // 2] / sorted(dev)[len(dev) // 2]))
            env = dict(os.environ, PGX_BUILD_TIMING="1")
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--pass-timing", text], env=env, capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired:
                say("pass timing child did not finish in 300 s")
                continue
            line = next((l for l in r.stderr.splitlines() if "radix passes" in l), None)
            if r.returncode != 0 or not line:
                say("pass timing child failed: rc %d %s" % (r.returncode, r.stderr[-300:]))
                continue
            say(line.strip())
            m = re.search(r"radix passes (\d+) in ([\d.]+) ms", line)
            passes, ms_all = int(m.group(1)), float(m.group(2))
            pass_bytes = 28 * n  # per pass: 4 n of keys read by the histogram, three 4 n columns read and written by the scatter
            rate = pass_bytes * passes / (ms_all * 1e-3) / 1e9
            copy = dtod_rate(pass_bytes)
            say("radix pass: %d bytes (4 n of keys read by the histogram, 12 n read + 12 n written by the scatter) in %.3f ms on average = %.0f GB/s: "
                "%.1f %% of the %.0f TB/s peak, %.1f %% of a device-to-device copy of the same bytes (%.0f GB/s)"
                % (pass_bytes, ms_all / passes, rate, 100 * rate / (PEAK_TBS * 1000), PEAK_TBS, 100 * rate / copy, copy))
    out.close()


if __name__ == "__main__":
    main()
