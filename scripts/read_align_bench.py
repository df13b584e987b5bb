"""pgx_batch_read_align on bench.py's workloads: every read aligned with gaps at its verify winner, on the device.

  python3 scripts/read_align_bench.py [--workload synth|chr22] [--reads N] [--haps H] [--base-len L] [--steps 3] [--cap 64] [--out FILE]

One batch of --reads 150-bp reads of the workload (bench.py's cache directory and reads), min_len 20 / min_occ 1, run with
PGX_RUN_TAGS | PGX_RUN_TIMING, pgx_batch_locate(0, --cap) (the CLI's --place-max), pgx_batch_read_place(0) and pgx_batch_read_verify(1, 4),
then pgx_batch_read_align at W = 4, 8 and 16, with and without PGX_ALIGN_CIGAR.  One warm-up call, then the median of --steps, for:
  ms_align     device events around the whole stage; ms_forward / ms_trace: the sums over the launches of the forward kernel and of the
               traceback walks (the counting walk, and with PGX_ALIGN_CIGAR the writing walk)
  scratch      bytes of direction planes of the largest pass, and the number of passes
  bytes        what the stage must move by the model: per read position half a byte of coded read and (2 W + 1) / 2 bytes of text
               symbols read, a row of planes written and a sixteenth of it read back per walk; per read 64 B of verify record in, 64 B of
               record out, 8 B of end cell out and in, 24 B of offsets and counts; with PGX_ALIGN_CIGAR 4 B an operation; over ms_align as a
               share of 8 TB/s
  copy floor   a device-to-device copy of that many bytes, timed with events in this invocation
  ms_verify, ms_place   the stages before it, in the same invocation, and the find_mems step itself
Rows are JSON lines; --out also appends them to a file."""
import argparse
import json
import os
import sys

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
    emit(dict(workload=desc, reads=n_reads, n_mems=int(b.counts()[0]), n_sequences=int(info.n_sequences), bwt_size=int(info.bwt_size), find_mems_step_ms=round(step_ms, 3)))
    b.locate(0, a.cap)
    ms_place, ms_verify = [], []
    for i in range(a.steps + 1):
        P._check(b.L.pgx_batch_read_place(b.b, 0, None))
        if i:
            ms_place.append(b.device_places()["ms_place"])
    P._check(b.L.pgx_batch_read_verify(b.b, 1, 4, 0, None))  # (builds the text image)
    for i in range(a.steps + 1):
        P._check(b.L.pgx_batch_read_verify(b.b, 1, 4, 0, None))
        if i:
            ms_verify.append(b.device_verified()["ms_verify"])
    emit(dict(cap=a.cap, ms_place=round(median(ms_place), 4), ms_verify=round(median(ms_verify), 4), n_cands=int(b.device_verified()["n_cands"])))
    for band in (4, 8, 16):
        for flags in (0, P.ALIGN_CIGAR):
            rows = []
            for i in range(a.steps + 1):
                P._check(b.L.pgx_batch_read_align(b.b, band, flags, None))
                if i:
                    rows.append(b.device_aligned())
            d = rows[-1]
            m, fwd, trace = (median([r[k] for r in rows]) for k in ("ms_align", "ms_forward", "ms_trace"))
            group = 1
            while group < 2 * band + 1:
                group *= 2
            row_bytes = max(group, 8) // 4
            walks = 2 if flags else 1
            model = int(read_bytes * (0.5 + (2 * band + 1) / 2 + row_bytes + walks * row_bytes / 16) + n_reads * (64 + 64 + 16 + 24) + (4 * d["n_ops"] if flags else 0))
            floor = copy_ms(model, False, a.steps)
            emit(dict(band=band, cigar=bool(flags), ms_align=round(m, 4), ms_forward=round(fwd, 4), ms_trace=round(trace, 4), ms_all=[round(r["ms_align"], 4) for r in rows],
                      n_ops=d["n_ops"], passes=d["passes"], scratch_bytes=d["scratch_bytes"], reads_per_s=round(n_reads / (m * 1e-3), 1),
                      cells_per_s=round(read_bytes * (2 * band + 1) / (m * 1e-3), 1), vs_verify=round(m / median(ms_verify), 3), vs_place=round(m / median(ms_place), 4),
                      vs_find_mems_step=round(m / step_ms, 4), model_bytes=model, hbm_fraction=round(model / (m * 1e-3) / HBM_PEAK, 4), d2d_copy_ms=round(floor, 4),
                      vs_d2d_copy=round(m / floor, 2)))
    v = b.read_align(8, 0)["reads"]
    has = v["seq"] != 0xFFFFFFFF
    emit(dict(aligned="summary at W = 8", reads_with_a_candidate=int(has.sum()), no_edit=int((has & (v["edits"] == 0)).sum()), one_edit=int((v["edits"] == 1).sum()),
              with_a_gap=int(((v["n_ins"] + v["n_del"]) > 0).sum()), band_hit=int(v["band_hit"].sum()), mean_edits=round(float(v["edits"][has].mean()), 3) if has.any() else 0,
              mean_ops=round(float(v["n_ops"][has].mean()), 3) if has.any() else 0))
    b.free()
    idx.close()


if __name__ == "__main__":
    main()
