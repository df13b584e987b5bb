"""The last stage of graph -> searchable index, host against device (GPU box):
python3 -u scripts/tags_encode_bench.py [--sizes 4000000,40000000] [--haps 8] [--reps 3] [--host-reps 3] [--out profiles/tags_encode_bench.txt]

On the synthetic pangenomes of scripts/build_tags_bench.py (one node per 32 bp, ids not shared: one run per tagged row, the encoder's
worst case), per size, medians of --reps:
  (a) two steps: build_tags (algorithm format) + pgx_convert_tags(compact = 1) on the host, wall time and stage times
  (b) one step:  build_tags with BUILD_TAGS_OUT_COMPACT, wall time, stage times, the encoder's own stages
  (c) the encoder alone (pgx_tags_encode, upload of the run arrays included in its wall time, not in its stages) against
      pgx_write_compact_tags on the same arrays: R runs of length 1 over the graph's node ids
  (d) the encoder's device time (its stages pieces + sd_vectors + select) against a device-to-device hipMemcpy of its output bytes
and the output size and the encoder's peak device bytes.  (a) and (b) are compared byte for byte.  The steps run one after the other in
this process; the caller gives the whole script its time limit.  Every line goes to stdout and, with --out, to that file."""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)
import numpy as np

import build_tags_bench as B
import pgx_ffi as P

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def med(xs):
    return statistics.median(xs)


def stages(runs, keys):
    return ", ".join("%s %.1f" % (k, med([r[k] for r in runs])) for k in keys)


def d2d_ms(nbytes):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    d0, d1 = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d0), nbytes) == 0 and hip.hipMalloc(C.byref(d1), nbytes) == 0
    ts = []
    for k in range(6):  # (the first round warms the path up and is dropped)
        t0 = time.perf_counter()
        assert hip.hipMemcpy(d1, d0, nbytes, 3) == 0 and hip.hipDeviceSynchronize() == 0
        if k:
            ts.append(1e3 * (time.perf_counter() - t0))
    hip.hipFree(d0)
    hip.hipFree(d1)
    return med(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4000000,40000000")
    ap.add_argument("--haps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=None, help="repetitions of the host legs (default: --reps)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    host_reps = a.host_reps or a.reps
    say("tags_encode_bench on %s; medians of %d (host legs: of %d); times in ms" % (P.device_name(a.device), a.reps, host_reps))
    enc_keys = P.TAGS_ENCODE_STAGES[:5]
    with tempfile.TemporaryDirectory() as td:
        plain, conv, one = (os.path.join(td, n) for n in ("plain.tags", "conv.tags", "one.tags"))
        for base_len in (int(x) for x in a.sizes.split(",")):
            ri, text = B.index_for(base_len, a.haps)
            po, pn, nl, fid = B.graph_of(text)
            inf = P.Index(ri).info()
            n = int(inf.bwt_size)
            say()
            say("== base_len %d x %d haplotypes x 2 strands: n = %d rows, %d node ids" % (base_len, a.haps, n, len(nl)))
            # (a) two steps
            two, bt_ms = [], []
            for _ in range(host_reps):
                t0 = time.perf_counter()
                ms = P.build_tags_paths(ri, po, pn, nl, fid, plain, device=a.device)
                t1 = time.perf_counter()
                P.convert_tags(plain, conv, compact=True)
                t2 = time.perf_counter()
                two.append({"build_tags": 1e3 * (t1 - t0), "convert_tags": 1e3 * (t2 - t1), "total": 1e3 * (t2 - t0)})
                bt_ms.append(ms)
            say("(a) build_tags + convert_tags:   total %.0f  = build_tags %.0f (%s) + convert_tags on the host %.0f; files %d + %d bytes"
                % (med([r["total"] for r in two]), med([r["build_tags"] for r in two]), stages(bt_ms, P.BUILD_TAGS_STAGES),
                   med([r["convert_tags"] for r in two]), os.path.getsize(plain), os.path.getsize(conv)))
            # (b) one step
            wall, ob_ms, oe_ms = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ms = P.build_tags_paths(ri, po, pn, nl, fid, one, device=a.device, flags=P.BUILD_TAGS_OUT_COMPACT)
                wall.append(1e3 * (time.perf_counter() - t0))
                ob_ms.append(ms)
                oe_ms.append(P.tags_encode_timing())
            same = os.path.getsize(one) == os.path.getsize(conv) and open(one, "rb").read() == open(conv, "rb").read()
            say("(b) build_tags --format compact: total %.0f  (%s); its write stage is the encoder: %s; same bytes as (a): %s"
                % (med(wall), stages(ob_ms, P.BUILD_TAGS_STAGES), stages(oe_ms, enc_keys), same))
            say("    (a) / (b) = %.2f; last stage alone, convert_tags / encoder = %.1f"
                % (med([r["total"] for r in two]) / med(wall), med([r["convert_tags"] for r in two]) / med([r["write"] for r in ob_ms])))
            file_bytes, dev_bytes = int(oe_ms[-1]["file_bytes"]), int(oe_ms[-1]["device_bytes"])
            say("    output %d bytes; encoder's peak device bytes %d (%.1f per run)" % (file_bytes, dev_bytes, dev_bytes / max(n, 1)))
            for p in (plain, conv, one):
                os.remove(p)
            # (c) the encoder alone against the host writer, same arrays
            R = n - int(inf.n_sequences)
            i = np.arange(R, dtype=np.uint64)
            values = (((i * np.uint64(2654435761)) % np.uint64(len(nl)) + np.uint64(1)) << np.uint64(11)) | (i & np.uint64(31))
            lengths = np.ones(R, dtype=np.uint64)
            host, dev, dms = [], [], []
            for _ in range(host_reps):
                t0 = time.perf_counter()
                P.write_compact_tags(conv, values, lengths)
                host.append(1e3 * (time.perf_counter() - t0))
            for _ in range(a.reps):
                t0 = time.perf_counter()
                dms.append(P.tags_encode(values, lengths, one, P.TAGS_COMPACT, device=a.device))
                dev.append(1e3 * (time.perf_counter() - t0))
            same = open(one, "rb").read() == open(conv, "rb").read()
            say("(c) %d runs of length 1: pgx_write_compact_tags %.0f; pgx_tags_encode %.0f (%s); ratio %.1f; same bytes: %s"
                % (R, med(host), med(dev), stages(dms, enc_keys), med(host) / med(dev), same))
            # (d) device time against a plain copy of the output
            kern = med([r["pieces"] + r["sd_vectors"] + r["select"] for r in dms])
            nb = int(dms[-1]["file_bytes"])
            cp = d2d_ms(nb)
            say("(d) encoder kernels (pieces + sd_vectors + select, scalar read-backs included) %.1f; device-to-device hipMemcpy of the %d output bytes %.2f"
                " (%.0f GB/s); ratio %.1f" % (kern, nb, cp, nb / cp / 1e6, kern / cp))
            for p in (conv, one):
                os.remove(p)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
