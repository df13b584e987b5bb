"""pgx_batch_read_verify on bench.py's workloads: every read laid on the indexed text at its best placements, on the device.

  python3 scripts/read_verify_bench.py [--workload synth|chr22] [--reads N] [--haps H] [--base-len L] [--steps 3] [--cap 64] [--out FILE]

One batch of --reads 150-bp reads of the workload (bench.py's cache directory and reads), min_len 20 / min_occ 1, run with
PGX_RUN_TAGS | PGX_RUN_TIMING, pgx_batch_locate(0, --cap) and pgx_batch_read_place(PGX_PLACE_LIST), then pgx_batch_read_verify at
max_cand 1 and 16.  One warm-up call, then the median of --steps, for:
  text image   wall time of the first verify call (it builds the image: the whole-range locate or the resident LCE image's suffix array,
               scatter, pack) less a later call, and the bytes the image keeps
  ms_verify    device events around the whole stage (candidates chosen, reads coded, candidates verified, winners), records only
  bytes        what the stage must move by the model: read bytes in and half of them out (the coded reads); per candidate half a byte per
               read position of coded read and of text, 20 B of candidate in, 64 B of record out and in again; 64 B of place record in and
               64 B of verify record out per read; with max_cand > 1 the 24 B of every placement; over ms_verify as a share of 8 TB/s
  copy floor   a device-to-device copy of that many bytes, timed with events in this invocation
  ms_place     the place stage the candidates come from, in the same invocation, and the find_mems step itself
Rows are JSON lines; --out also appends them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench  # noqa: E402
import pgx_ffi as P  # noqa: E402
from read_hits_bench import HBM_PEAK, copy_ms, median  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synth", choices=("chr22", "synth"))
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--haps", type=int, default=None)
    ap.add_argument("--base-len", type=int, default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--cap", type=int, default=64)
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
    n_reads, read_bytes = len(offs) - 1, int(offs[-1] - offs[0])
    n, n_seq = int(info.bwt_size), int(info.n_sequences)
    emit(dict(workload=desc, reads=n_reads, n_mems=int(b.counts()[0]), n_sequences=n_seq, bwt_size=n, find_mems_step_ms=round(step_ms, 3)))
    b.locate(0, a.cap)
    ms_place = []
    for i in range(a.steps + 1):
        P._check(b.L.pgx_batch_read_place(b.b, P.PLACE_LIST, None))
        if i:
            ms_place.append(b.device_places()["ms_place"])
    n_places = int(b.device_places()["n_places"])
    emit(dict(cap=a.cap, anchors=int(b.device_locations()["n_values"]), n_places=n_places, ms_place=round(median(ms_place), 4), ms_place_all=[round(x, 4) for x in ms_place]))
    lce = bool(idx.lce_view(30, 64).any())
    t0 = time.time()
    P._check(b.L.pgx_batch_read_verify(b.b, 1, 4, 0, None))
    first = time.time() - t0
    t0 = time.time()
    P._check(b.L.pgx_batch_read_verify(b.b, 1, 4, 0, None))
    later = time.time() - t0
    emit(dict(text_image="build", route="resident LCE suffix array" if lce else "whole-range locate", wall_ms=round(1e3 * (first - later), 2),
              image_bytes=((n + 7) // 8 + 4) * 4 + (n_seq + 1) * 8, bytes_per_symbol=0.5))
    for max_cand in (1, 16):
        ms = []
        for i in range(a.steps + 1):
            P._check(b.L.pgx_batch_read_verify(b.b, max_cand, 4, 0, None))
            if i:
                ms.append(b.device_verified()["ms_verify"])
        d = b.device_verified()
        c = int(d["n_cands"])
        mean_len = read_bytes / max(n_reads, 1)
        model = int(1.5 * read_bytes + c * (mean_len + 20 + 128) + 128 * n_reads + (24 * n_places if max_cand > 1 else 0))
        m = median(ms)
        floor = copy_ms(model, False, a.steps)
        emit(dict(max_cand=max_cand, n_cands=c, ms_verify=round(m, 4), ms_all=[round(x, 4) for x in ms], reads_per_s=round(n_reads / (m * 1e-3), 1),
                  cands_per_s=round(c / (m * 1e-3), 1), vs_place=round(m / median(ms_place), 4), vs_find_mems_step=round(m / step_ms, 4), model_bytes=model,
                  hbm_fraction=round(model / (m * 1e-3) / HBM_PEAK, 4), d2d_copy_ms=round(floor, 4), vs_d2d_copy=round(m / floor, 2)))
    v = b.read_verify(16, 4)["reads"]
    has = v["seq"] != 0xFFFFFFFF
    emit(dict(verified="summary at max_cand 16", reads_with_a_candidate=int(has.sum()), mean_cands=round(float(v["n_cand"][has].mean()), 3) if has.any() else 0,
              no_mismatch=int((has & (v["mismatches"] == 0)).sum()), one_mismatch=int((v["mismatches"] == 1).sum()),
              winner_not_first=int((v["cand_index"] > 0).sum()), still_tied=int((v["n_tied"] > 1).sum()),
              mean_seg_score=round(float(v["seg_score"][has].mean()), 2) if has.any() else 0))
    b.free()
    idx.close()


if __name__ == "__main__":
    main()
