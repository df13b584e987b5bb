#!/usr/bin/env python3
"""What opening an index costs by the two routes, on the chr22-scale index of bench.py (profiles/open_image_bench.txt):

  (A) pgx_index_open(.ri, tags) + pgx_index_to_device     the parse and the host builds of the images, every start
  (B) pgx_index_open_image(.pgi) + pgx_index_to_device    reading the saved images, their sums on the device
  (C) a plain read of the image file into memory           the floor of any reader

In one process: one warm-up of each route, then three rounds A, B, C in turn.  All three read through a WARM page cache (the files
have just been written or read by the warm-up): the numbers say what the host work costs, not what a disk delivers.  The sum
kernel's rate (bytes over its HIP-event time, from the library's PGX_IMAGE_TIMING line) stands next to a device-to-device copy of
the same number of bytes measured here with HIP events, as the radix passes stand next to one in DESIGN.md 7b.

    python scripts/open_image_bench.py [--out profiles/open_image_bench.txt] [--base-len N --haps H] [--rounds 3]
"""
import argparse
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))

PEAK_BYTES_PER_S = 8.0e12  # HBM3E peak of an MI355X


class Stderr:
    """file descriptor 2 into a temporary file for a block (the library's timing line goes there)"""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        return False


LINE = re.compile(r"uploads(?: \+ sums)? ([0-9.]+) ms wall; sum kernels ([0-9.]+) ms by HIP events over (\d+) bytes; device-side builds ([0-9.]+) ms")


def route(P, open_fn):
    t0 = time.perf_counter()
    idx = open_fn()
    t1 = time.perf_counter()
    with Stderr() as err:
        idx.to_device(0)
    t2 = time.perf_counter()
    idx.close()
    m = LINE.search(err.text)
    up, sums, nbytes, builds = (float(m.group(1)), float(m.group(2)), int(m.group(3)), float(m.group(4))) if m else (0.0, 0.0, 0, 0.0)
    sys.stderr.write("[open_image_bench] open %.2f s, to_device %.2f s\n" % (t1 - t0, t2 - t1))
    return dict(open_s=t1 - t0, to_device_s=t2 - t1, upload_ms=up, sums_ms=sums, sum_bytes=nbytes, builds_ms=builds)


def d2d_copy_ms(nbytes, repeats=5):
    """best HIP-event time of hipMemcpy device-to-device of nbytes, through the HIP runtime libpgx.so is linked against"""
    import ctypes as C

    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p

    def ok(rc):
        if rc != 0:
            raise RuntimeError("HIP call failed with status %d" % rc)

    src, dst, e0, e1 = vp(), vp(), vp(), vp()
    ok(hip.hipMalloc(C.byref(src), C.c_size_t(nbytes)))
    ok(hip.hipMalloc(C.byref(dst), C.c_size_t(nbytes)))
    best = None
    try:
        ok(hip.hipMemset(src, 0, C.c_size_t(nbytes)))
        ok(hip.hipEventCreate(C.byref(e0)))
        ok(hip.hipEventCreate(C.byref(e1)))
        for i in range(repeats + 1):  # (the first one warms up)
            ok(hip.hipEventRecord(e0, None))
            ok(hip.hipMemcpyAsync(dst, src, C.c_size_t(nbytes), 3, None))  # hipMemcpyDeviceToDevice
            ok(hip.hipEventRecord(e1, None))
            ok(hip.hipEventSynchronize(e1))
            ms = C.c_float(0)
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
            if i:
                best = ms.value if best is None else min(best, ms.value)
    finally:
        hip.hipFree(src)
        hip.hipFree(dst)
        if e0:
            hip.hipEventDestroy(e0)
        if e1:
            hip.hipEventDestroy(e1)
    return best


def main():
    import bench
    import pgx_ffi as P
    import pgx_workload as W

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_image_bench.txt"))
    ap.add_argument("--base-len", type=int, default=None)
    ap.add_argument("--haps", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    bargs = bench.parse([])  # the chr22 workload's defaults
    base_len, haps = a.base_len or bargs.base_len, a.haps or bargs.haps
    wd = bench.cache_dir()
    os.makedirs(wd, exist_ok=True)
    with bench.DirLock(wd):
        ri, tags, _, build_s = bench.synth_index(W, wd, base_len, haps, 0, lambda: None)
    image = os.path.join(wd, os.path.splitext(os.path.basename(ri))[0] + ".pgi")
    sys.stderr.write("[open_image_bench] index %s (built here in %.1f s)\n" % (ri, build_s))
    os.environ["PGX_IMAGE_TIMING"] = "1"

    open_a = lambda: P.Index(ri, tags)  # noqa: E731
    open_b = lambda: P.Index.open_image(image)  # noqa: E731
    src = P.Index(ri, tags)
    t0 = time.perf_counter()
    src.save_image(image)
    save_s = time.perf_counter() - t0
    inf = src.info()
    src.close()
    fi = P.image_file_info(image)
    sys.stderr.write("[open_image_bench] image saved in %.2f s: %d bytes\n" % (save_s, fi["file_bytes"]))

    def read_c():
        t0 = time.perf_counter()
        with open(image, "rb") as f:
            n = len(f.read())
        return dict(read_s=time.perf_counter() - t0, bytes=n)

    route(P, open_a); route(P, open_b); read_c()  # warm-up of each route
    A, B, Cc = [], [], []
    for _ in range(a.rounds):
        A.append(route(P, open_a)); B.append(route(P, open_b)); Cc.append(read_c())
    copy_ms = d2d_copy_ms(max(r["sum_bytes"] for r in B))

    def spread(rows, key):
        v = [r[key] for r in rows]
        return "%.3f (min %.3f, max %.3f)" % (sorted(v)[len(v) // 2], min(v), max(v))

    L = []
    L.append("open_image_bench: %s, n = %d, %d runs, image kind %d pairs %d; device %s" % (os.path.basename(ri), inf.bwt_size, inf.n_runs, inf.image_kind, inf.image_pairs, P.device_name(0)))
    L.append("page cache WARM for all three routes (every file was written or read just before); one process, one warm-up of each route, then %d rounds A, B, C in turn; median (min, max)" % a.rounds)
    L.append("image file: %d bytes in %d sections; one pgx_index_save_image: %.2f s" % (fi["file_bytes"], fi["n_sections"], save_s))
    for s in fi["sections"]:
        if s["bytes"] >= 1 << 20:
            L.append("  section %-10s %12d bytes" % (s["name"], s["bytes"]))
    L.append("(A) pgx_index_open(.ri, tags):   host open %s s; to_device %s s [uploads %s ms, device-side builds %s ms]" % (spread(A, "open_s"), spread(A, "to_device_s"), spread(A, "upload_ms"), spread(A, "builds_ms")))
    L.append("(B) pgx_index_open_image(.pgi):  host open %s s; to_device %s s [uploads + sums %s ms, device-side builds %s ms]" % (spread(B, "open_s"), spread(B, "to_device_s"), spread(B, "upload_ms"), spread(B, "builds_ms")))
    L.append("(C) plain read of the .pgi:      %s s" % spread(Cc, "read_s"))
    med = lambda rows, key: sorted(r[key] for r in rows)[len(rows) // 2]  # noqa: E731
    ta, tb, tc = med(A, "open_s") + med(A, "to_device_s"), med(B, "open_s") + med(B, "to_device_s"), med(Cc, "read_s")
    L.append("open + to_device: (A) %.2f s, (B) %.2f s = %.1f x less; host open of (B) = %.2f x the plain read (C)" % (ta, tb, ta / tb if tb else 0.0, med(B, "open_s") / tc if tc else 0.0))
    sb, sm = med(B, "sum_bytes"), med(B, "sums_ms")
    if sm > 0:
        rate = sb / (sm * 1e-3)
        L.append("sum kernels: %d bytes in %s ms by HIP events = %.2f TB/s = %.0f %% of the 8 TB/s peak" % (sb, spread(B, "sums_ms"), rate / 1e12, 100.0 * rate / PEAK_BYTES_PER_S))
        crate = sb / (copy_ms * 1e-3)
        L.append("device-to-device copy of the same %d bytes (HIP events, best of 5): %.3f ms = %.2f TB/s copied (reads + writes: twice that in traffic); the sums take %.2f x the copy's time" % (sb, copy_ms, crate / 1e12, sm / copy_ms))
    if build_s:
        L.append("(the index itself was built for this run: %.1f s)" % build_s)
    text = "\n".join(L) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
