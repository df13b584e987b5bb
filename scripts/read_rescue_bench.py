"""pgx_batch_read_rescue on bench.py's workloads: the unplaced mate of a pair searched for next to the placed one, on the device.

  python3 scripts/read_rescue_bench.py [--workload synth|chr22] [--reads N] [--haps H] [--base-len L] [--steps 3] [--cap 64] [--every K] [--out FILE]

One batch of --reads 150-bp reads of the workload (bench.py's cache directory and reads; an odd count drops its last read), min_len 20 /
min_occ 1, run with PGX_RUN_TAGS | PGX_RUN_TIMING, pgx_batch_locate(0, --cap), pgx_batch_read_place(PGX_PLACE_LIST) and
pgx_batch_read_verify(16, 4, PGX_VERIFY_LIST).  The workloads hold every haplotype next to its reverse complement, so the index is twinned.
Their reads are independent samples: reads 2k and 2k + 1 are taken as mates as they come, so with the bounds [0, 1000] next to no pair is
compatible and nearly every read with a placed mate is a target whose whole window is scored and holds nothing.  THIS IS THE STAGE'S UPPER
END: in a real paired run the targets are the few percent of pairs that place and mates left open.  --every K (default 10) adds a second
batch in which the second read of every pair but each K-th is emptied: its mate then has no placed partner and is no target, and the
emptied read is a target with empty windows, so only every K-th pair costs a scan.  Per batch, one warm-up call and the median of --steps for:
  ms_verify    pgx_batch_read_verify(16, 4, PGX_VERIFY_LIST), device events around the stage
  ms_mates     pgx_batch_read_mates(0, 1000, 10, PGX_MATES_ELECT)
  ms_rescue    pgx_batch_read_rescue(0, 1000, 20, max_anchors, flags) at max_anchors 1 and 2, with and without PGX_RESCUE_MERGE (a verify call
               before every merging call: a verify result takes one merge), device events around the stage, its two read-backs included
  ms_window1   the same call with the bounds [500, 500]: one diagonal a task, so targets, tasks and every pass but the scan stay; scan_share is
               1 - ms_window1 / ms_rescue
  bytes        what the stage must move by the model: 64 B per candidate read, 64 B per read and 64 B per task written and read back; with
               MERGE the list read and written once more and a winner record per read
  copy floor   a device-to-device copy of that many bytes, timed with events in this invocation
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
from read_hits_bench import copy_ms, median  # noqa: E402


def thin(cat, offs, every):
    """the batch with read 2k + 1 emptied in every pair k with k % every != 0"""
    lens = np.diff(offs.astype(np.int64))
    pair = np.arange(len(lens)) // 2
    keep = (np.arange(len(lens)) % 2 == 0) | (pair % every == 0)
    new_lens = np.where(keep, lens, 0)
    mask = np.repeat(keep, lens)
    return np.ascontiguousarray(cat[mask]), np.concatenate([[0], np.cumsum(new_lens)]).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synth", choices=("chr22", "synth"))
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--haps", type=int, default=None)
    ap.add_argument("--base-len", type=int, default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--every", type=int, default=10)
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
    offs = np.asarray(offs[: n_reads + 1], dtype=np.uint64)
    cat = np.asarray(cat[: int(offs[-1])], dtype=np.uint8)
    idx = P.Index(ri, tags)
    info = idx.info()
    for label, (bcat, boffs) in (("every pair open: the stage's upper end", (cat, offs)), ("every %dth pair open" % a.every, thin(cat, offs, a.every))):
        b = P.Batch(idx, bcat, boffs)
        b.run(20, 1, P.RUN_TAGS | P.RUN_TIMING)  # (the first run builds the LCE image where the index has one)
        b.run(20, 1, P.RUN_TAGS | P.RUN_TIMING)
        step_ms = b.timing().ms_total
        b.locate(0, a.cap)
        P._check(b.L.pgx_batch_read_place(b.b, P.PLACE_LIST, None))

        def verify():
            P._check(b.L.pgx_batch_read_verify(b.b, 16, 4, P.VERIFY_LIST, None))
            return b.device_verified()

        ms_verify = [verify()["ms_verify"] for i in range(a.steps + 1)][1:]
        n_cands = b.device_verified()["n_cands"]
        mv = median(ms_verify)
        ms_mates = []
        for i in range(a.steps + 1):
            P._check(b.L.pgx_batch_read_mates(b.b, 0, 1000, 10, P.MATES_ELECT, None))
            ms_mates.append(b.device_mated()["ms_mates"])
            verify()
        mm = median(ms_mates[1:])
        emit(dict(batch=label, workload=desc, reads=n_reads, pairs=n_reads // 2, n_sequences=int(info.n_sequences), bwt_size=int(info.bwt_size), twinned=idx.twinned() is None,
                  find_mems_step_ms=round(step_ms, 3), cap=a.cap, max_cand=16, n_cands=n_cands, ms_verify=round(mv, 4), ms_mates=round(mm, 4)))
        for anchors in (1, 2):
            for flags in (0, P.RESCUE_MERGE):
                def rescue(lo, hi):
                    rows = []
                    for i in range(a.steps + 1):
                        if flags or i == 0:  # (a verify result takes one merge: a fresh one before every merging call, and behind the merging rows)
                            verify()
                        P._check(b.L.pgx_batch_read_rescue(b.b, lo, hi, 20, anchors, flags, None))
                        rows.append(b.device_rescued())
                    return rows[1:]

                rows, one = rescue(0, 1000), rescue(500, 500)
                d = rows[-1]
                m, m1 = median([r["ms_rescue"] for r in rows]), median([r["ms_rescue"] for r in one])
                model = 64 * n_cands + 64 * n_reads + 64 * d["n_tasks"] + ((128 * n_cands + 64 * d["n_rescued"] + 64 * n_reads) if flags else 0)
                floor = copy_ms(model, False, a.steps)
                emit(dict(batch=label, max_anchors=anchors, merge=bool(flags), ms_rescue=round(m, 4), ms_all=[round(r["ms_rescue"], 4) for r in rows], n_targets=d["n_targets"],
                          n_tasks=d["n_tasks"], n_diags=d["n_diags"], n_rescued=d["n_rescued"], n_full=d["n_full"],
                          diag_positions_per_s=round(d["n_diags"] * 150 / (m * 1e-3), 1), ms_window1=round(m1, 4), scan_share=round(1 - m1 / m, 4), model_bytes=model,
                          d2d_copy_ms=round(floor, 4), vs_d2d_copy=round(m / floor, 2), vs_verify=round(m / mv, 3), vs_mates=round(m / mm, 2),
                          vs_find_mems_step=round(m / step_ms, 3)))
        b.free()
    idx.close()


if __name__ == "__main__":
    main()
