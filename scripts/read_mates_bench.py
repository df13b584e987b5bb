"""pgx_batch_read_mates on bench.py's workloads: the two reads of a pair choose their placements together, on the device.

  python3 scripts/read_mates_bench.py [--workload synth|chr22] [--reads N] [--haps H] [--base-len L] [--steps 5] [--cap 64] [--out FILE]

One batch of --reads 150-bp reads of the workload (bench.py's cache directory and reads; an odd count drops its last read), min_len 20 /
min_occ 1, run with PGX_RUN_TAGS | PGX_RUN_TIMING, pgx_batch_locate(0, --cap) and pgx_batch_read_place(PGX_PLACE_LIST).  The workloads hold
every haplotype next to its reverse complement, so the index is twinned.  Their reads are independent samples: reads 2k and 2k + 1 are
taken as mates as they come, so with the bounds [0, 1000] next to no pair is compatible and the stage does its loads, its shuffles and its
stores; with the bounds [-2^62, 2^62] every candidate pair on twin sequences is compatible and the monoid is folded for each, which is the
most the kernel can be asked to do on these lists.  Then, at max_cand 1 and 16, one warm-up call and the median of --steps for:
  ms_verify    pgx_batch_read_verify(max_cand, 4, PGX_VERIFY_LIST), device events around the stage
  ms_mates     pgx_batch_read_mates with and without PGX_MATES_ELECT at both bounds, device events around the kernel and its counters
  bytes        what the stage must move by the model: 64 B per candidate read, 64 B per pair written, plus 128 B per pair with ELECT
  copy floor   a device-to-device copy of that many bytes, timed with events in this invocation
Rows are JSON lines; --out also appends them to a file."""
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
    emit(dict(workload=desc, reads=n_reads, pairs=n_reads // 2, n_sequences=int(info.n_sequences), bwt_size=int(info.bwt_size), twinned=idx.twinned() is None,
              find_mems_step_ms=round(step_ms, 3), cap=a.cap))
    for max_cand in (1, 16):
        ms_verify = []
        for i in range(a.steps + 1):
            P._check(b.L.pgx_batch_read_verify(b.b, max_cand, 4, P.VERIFY_LIST, None))
            if i:
                ms_verify.append(b.device_verified()["ms_verify"])
        n_cands = b.device_verified()["n_cands"]
        mv = median(ms_verify)
        emit(dict(max_cand=max_cand, n_cands=n_cands, cands_per_read=round(n_cands / n_reads, 3), ms_verify=round(mv, 4)))
        for bounds, (lo, hi) in (("0..1000", (0, 1000)), ("all", (-2 ** 62, 2 ** 62))):
            for flags in (0, P.MATES_ELECT):
                rows = []
                for i in range(a.steps + 1):
                    P._check(b.L.pgx_batch_read_mates(b.b, lo, hi, 10, flags, None))
                    if i:
                        rows.append(b.device_mated())
                d = rows[-1]
                m = median([r["ms_mates"] for r in rows])
                model = 64 * n_cands + (64 + (128 if flags else 0)) * (n_reads // 2)
                floor = copy_ms(model, False, a.steps)
                emit(dict(max_cand=max_cand, bounds=bounds, elect=bool(flags), ms_mates=round(m, 4), ms_all=[round(r["ms_mates"], 4) for r in rows],
                          pairs_per_s=round(n_reads / 2 / (m * 1e-3), 1), n_compatible=d["n_compatible"], n_proper=d["n_proper"], n_moved=d["n_moved_a"] + d["n_moved_b"],
                          model_bytes=model, hbm_fraction=round(model / (m * 1e-3) / HBM_PEAK, 4), d2d_copy_ms=round(floor, 4), vs_d2d_copy=round(m / floor, 2),
                          vs_verify=round(m / mv, 4), vs_find_mems_step=round(m / step_ms, 4)))
                if flags:  # (the next rows start from verify's own winners again)
                    P._check(b.L.pgx_batch_read_verify(b.b, max_cand, 4, P.VERIFY_LIST, None))
    b.free()
    idx.close()


if __name__ == "__main__":
    main()
