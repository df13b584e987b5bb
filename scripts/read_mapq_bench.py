"""pgx_batch_read_mapq on bench.py's workloads: a mapping quality for every read, on the device.

  python3 scripts/read_mapq_bench.py [--workload synth|chr22] [--reads N] [--haps H] [--base-len L] [--steps 5] [--cap 64] [--out FILE]

One batch of --reads 150-bp reads of the workload (bench.py's cache directory and reads; an odd count drops its last read), min_len 20 /
min_occ 1, run with PGX_RUN_TAGS | PGX_RUN_TIMING, pgx_batch_locate(0, --cap), pgx_batch_read_place(PGX_PLACE_LIST) and
pgx_batch_read_verify(16, 4, PGX_VERIFY_LIST).  The workloads hold every haplotype next to its reverse complement, so the index is twinned; their
reads are independent samples, and reads 2k and 2k + 1 are taken as mates as they come (bounds [0, 1000], U = 10, with PGX_MATES_ELECT).  Their tags
are one tag per BWT run with offset 0, so every text position is a visit of its own: the stage does its three dependent loads per entry, and the
classes it finds say nothing about a graph.  Then, at max_extra 0 and 16, unpaired and paired, one warm-up call and the median of --steps for:
  ms_mapq      pgx_batch_read_mapq(2, 8, max_extra, flags), device events around the extras' verify and the kernel
  bytes        what the stage must move by the model: 64 B per list record read, 32 B per read written, and per extra what verifying it moves
               (24 B of its placement, 20 B of candidate arrays written and read, 64 B of record written and read)
  copy floor   a device-to-device copy of that many bytes, timed with events in this invocation
against ms_verify at the same max_cand and the find_mems step.  Rows are JSON lines; --out also appends them to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench  # noqa: E402
import pgx_ffi as P  # noqa: E402
from read_hits_bench import HBM_PEAK, copy_ms, median  # noqa: E402

MAX_CAND = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synth", choices=("chr22", "synth"))
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--haps", type=int, default=None)
    ap.add_argument("--base-len", type=int, default=None)
    ap.add_argument("--steps", type=int, default=5)
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
    n_reads = (len(offs) - 1) & ~1  # whole pairs
    offs = offs[: n_reads + 1]
    cat = cat[: int(offs[-1])]
    idx = P.Index(ri, tags)
    info = idx.info()
    b = P.Batch(idx, cat, offs)
    b.run(20, 1, P.RUN_TAGS | P.RUN_TIMING)  # (the first run builds the LCE image where the index has one)
    b.run(20, 1, P.RUN_TAGS | P.RUN_TIMING)
    step_ms = b.timing().ms_total
    b.locate(0, a.cap)
    P._check(b.L.pgx_batch_read_place(b.b, P.PLACE_LIST, None))
    ms_verify = []
    for i in range(a.steps + 1):
        P._check(b.L.pgx_batch_read_verify(b.b, MAX_CAND, 4, P.VERIFY_LIST, None))
        if i:
            ms_verify.append(b.device_verified()["ms_verify"])
    n_cands = b.device_verified()["n_cands"]
    mv = median(ms_verify)
    emit(dict(workload=desc, reads=n_reads, n_sequences=int(info.n_sequences), bwt_size=int(info.bwt_size), find_mems_step_ms=round(step_ms, 3), cap=a.cap,
              max_cand=MAX_CAND, n_cands=n_cands, cands_per_read=round(n_cands / n_reads, 3), ms_verify=round(mv, 4)))
    for paired in (False, True):
        if paired:
            P._check(b.L.pgx_batch_read_mates(b.b, 0, 1000, 10, P.MATES_ELECT, None))
        for max_extra in (0, 16):
            rows = []
            for i in range(a.steps + 1):
                P._check(b.L.pgx_batch_read_mapq(b.b, 2, 8, max_extra, P.MAPQ_PAIRED if paired else 0, None))
                if i:
                    rows.append(b.device_mapqs())
            d = rows[-1]
            m = median([r["ms_mapq"] for r in rows])
            model = 64 * n_cands + 32 * n_reads + (24 + 2 * 20 + 2 * 64) * d["n_extras"]
            floor = copy_ms(model, False, a.steps)
            emit(dict(paired=paired, max_extra=max_extra, ms_mapq=round(m, 4), ms_all=[round(r["ms_mapq"], 4) for r in rows], reads_per_s=round(n_reads / (m * 1e-3), 1),
                      n_extras=d["n_extras"], n_has=d["n_has"], n_unique=d["n_unique"], n_capped=d["n_capped"], mean_mapq=round(d["sum_mapq"] / max(d["n_has"], 1), 2),
                      model_bytes=model, hbm_fraction=round(model / (m * 1e-3) / HBM_PEAK, 4), d2d_copy_ms=round(floor, 4), vs_d2d_copy=round(m / floor, 2),
                      vs_verify=round(m / mv, 4), vs_find_mems_step=round(m / step_ms, 4)))
    b.free()
    idx.close()


if __name__ == "__main__":
    main()
