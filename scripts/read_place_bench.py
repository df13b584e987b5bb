"""pgx_batch_read_place on bench.py's workloads: every read placed on its best sequence diagonal, on the device.

  python3 scripts/read_place_bench.py [--workload synth|chr22] [--reads N] [--haps H] [--base-len L] [--steps 3] [--caps 64,1024,0]
                                      [--max-read-anchors A] [--no-cli] [--out FILE]

One batch of --reads 150-bp reads of the workload (bench.py's cache directory and reads), min_len 20 / min_occ 1, run with
PGX_RUN_TAGS | PGX_RUN_TIMING, then for every cap of --caps (the max_occ of the locate, what find_mems --place-max sets; 0 = none)
pgx_batch_locate(0, cap) and pgx_batch_read_place.  One warm-up call, then the median of --steps, for:
  anchors      the values of the locate, and the most one read has.  A read's keys are sorted by one wave or one workgroup: a form whose
               largest read exceeds --max-read-anchors (default 2^20) is reported and not timed
  ms_place     device events around the whole stage (plan, keys, sort, sweep), records only and with PGX_PLACE_LIST
  bytes        what the stage must move by the model 16 B per anchor (value read, key written) + 16 B per anchor and sort pass (1: the
               sort reads a read's keys into registers or LDS once and writes them back once) + 32 B per MEM + 8 B in and 64 B out per
               read; over ms_place as a share of 8 TB/s
  copy floor   a device-to-device copy of that many bytes, timed with events in this invocation
  ms_locate    the positions locate the stage follows, and the find_mems step itself
  downloads    what a caller has to bring to the host without the stage (values, offsets and the MEM array) against the 64-byte records:
               copies of those sizes from device memory into pinned host memory, timed with events (the first capped at --max-copy-mb)
  CLI          wall time of find_mems --place F --place-only [--place-max cap] against the default text output (stdout to /dev/null,
               --quiet), alternated, for the first cap of --caps
Rows are JSON lines; --out also appends them to a file."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench  # noqa: E402
import pgx_ffi as P  # noqa: E402
from read_hits_bench import CLI, HBM_PEAK, copy_ms, median  # noqa: E402

SORT_PASSES = 1


def write_reads(path, cat, offs):
    with open(path, "wb") as f:
        step = 1 << 16
        for r0 in range(0, len(offs) - 1, step):
            r1 = min(r0 + step, len(offs) - 1)
            lens = np.diff(offs[r0:r1 + 1].astype(np.int64))
            block = np.asarray(cat[int(offs[r0]):int(offs[r1])], dtype=np.uint8)
            if len(lens) and (lens == lens[0]).all():
                f.write(np.concatenate([block.reshape(len(lens), int(lens[0])), np.full((len(lens), 1), 10, np.uint8)], axis=1).tobytes())
            else:
                for r in range(r0, r1):
                    f.write(bytes(cat[int(offs[r]):int(offs[r + 1])]) + b"\n")


def cli_walls(ri, tags, cat, offs, steps, cap, emit):
    with tempfile.TemporaryDirectory() as td:
        reads = os.path.join(td, "reads.txt")
        write_reads(reads, cat, offs)
        place_file = os.path.join(td, "place.tsv")
        name_place = "--place F --place-only" + (" --place-max %d" % cap if cap else "")
        forms = (("text (default)", ["--quiet"]), (name_place, ["--quiet", "--place", place_file, "--place-only"] + (["--place-max", str(cap)] if cap else [])))
        walls = {name: [] for name, _ in forms}
        pipes = {name: [] for name, _ in forms}
        env = dict(os.environ, PGX_CLI_STATS="1")
        for i in range(steps + 1):  # (the first round warms the page cache)
            for name, extra in forms:
                t0 = time.time()
                with open(os.devnull, "wb") as null:
                    r = subprocess.run([CLI, ri, tags, reads, "20", "1"] + extra, stdout=null, stderr=subprocess.PIPE, env=env, timeout=900)
                wall = time.time() - t0
                if r.returncode != 0:
                    raise SystemExit("find_mems failed: " + r.stderr.decode()[-500:])
                pipe = [l for l in r.stderr.decode().split("\n") if l.startswith("[find_mems] pipeline ")]
                if i:
                    walls[name].append(wall)
                    pipes[name].append(float(pipe[0].split()[2]) if pipe else float("nan"))
        for name, _ in forms:
            emit(dict(cli=name, reads=len(offs) - 1, process_wall_s=round(median(walls[name]), 3), pipeline_wall_s=round(median(pipes[name]), 3),
                      pipeline_all=[round(x, 3) for x in pipes[name]], reads_per_s_pipeline=round((len(offs) - 1) / median(pipes[name]), 1)))
        emit(dict(cli="place file", bytes=os.path.getsize(place_file)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synth", choices=("chr22", "synth"))
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--haps", type=int, default=None)
    ap.add_argument("--base-len", type=int, default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--caps", default="64,1024,0")
    ap.add_argument("--max-read-anchors", type=int, default=1 << 20)
    ap.add_argument("--max-copy-mb", type=int, default=8192)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    argv = ["--workload", a.workload]
    for name, v in (("--reads", a.reads), ("--haps", a.haps), ("--base-len", a.base_len)):
        if v is not None:
            argv += [name, str(v)]
    args = bench.parse(argv)
    caps = [int(c) for c in a.caps.split(",")]

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
    n_reads = len(offs) - 1
    n_mems = int(b.counts()[0])
    res = b.result()
    mem_off = res["mem_offsets"].astype(np.int64)
    emit(dict(workload=desc, reads=n_reads, n_mems=n_mems, n_sequences=int(info.n_sequences), max_length=int(info.max_length), bwt_size=int(info.bwt_size),
              find_mems_step_ms=round(step_ms, 3)))
    for cap in caps:
        ms_loc = []
        for i in range(a.steps + 1):
            b.locate(0, cap)
            if i:
                ms_loc.append(b.device_locations()["ms_locate"])
        loc = b.device_locations()
        anchors = int(loc["n_values"])
        # the most anchors a read has, from the sizes of the MEMs the locate took (what its plan does)
        size = res["mems"]["size"].astype(np.int64)
        took = np.where((size > 0) & ((cap == 0) | (size <= cap)), size, 0)
        per_read = np.add.reduceat(np.concatenate([took, [0]]), np.minimum(mem_off[:-1], len(took))) * (np.diff(mem_off) > 0)
        most = int(per_read.max()) if n_reads else 0
        row = dict(cap=cap, anchors=anchors, anchors_per_read=round(anchors / max(n_reads, 1), 2), most_anchors_of_a_read=most, n_not_located=int(loc["n_not_located"]),
                   resident=bool(loc["resident"]), ms_locate=round(median(ms_loc), 3), ms_locate_all=[round(x, 3) for x in ms_loc])
        emit(row)
        if most > a.max_read_anchors:
            emit(dict(cap=cap, skipped="a read has %d anchors, more than --max-read-anchors %d: one workgroup would sort them" % (most, a.max_read_anchors)))
            continue
        model = 16 * anchors + 16 * SORT_PASSES * anchors + 32 * n_mems + 8 * n_reads + 64 * n_reads
        for flags, name in ((0, "records"), (P.PLACE_LIST, "records + list")):
            ms = []
            for i in range(a.steps + 1):
                P._check(b.L.pgx_batch_read_place(b.b, flags, None))
                if i:
                    ms.append(b.device_places()["ms_place"])
            d = b.device_places()
            m = median(ms)
            row = dict(cap=cap, form=name, flags=flags, ms_place=round(m, 4), ms_all=[round(x, 4) for x in ms], passes=d["n_passes"], n_places=d["n_places"],
                       reads_per_s=round(n_reads / (m * 1e-3), 1), vs_locate=round(m / median(ms_loc), 4), vs_find_mems_step=round(m / step_ms, 4))
            if flags == 0:
                floor = copy_ms(model, False, a.steps)
                row.update(model_bytes=int(model), sort_passes=SORT_PASSES, hbm_fraction=round(model / (m * 1e-3) / HBM_PEAK, 4), d2d_copy_ms=round(floor, 4),
                           vs_d2d_copy=round(m / floor, 2))
            emit(row)
        today = 8 * anchors + 8 * (n_mems + 1) + 32 * n_mems + 8 * (n_reads + 1)
        timed = min(today, a.max_copy_mb << 20)
        down_today, down_recs = copy_ms(timed, True, a.steps) * (today / max(timed, 1)), copy_ms(64 * n_reads, True, a.steps)
        emit(dict(cap=cap, download="values + offsets + MEMs (without the stage)", bytes=int(today), ms=round(down_today, 3), timed_bytes=int(timed)))
        emit(dict(cap=cap, download="64-byte records", bytes=64 * n_reads, ms=round(down_recs, 3), ratio=round(down_today / down_recs, 2)))
        h = b.read_place(0)["reads"]  # (records only: the list of the last timed call is not downloaded)
        emit(dict(cap=cap, places="summary", reads_with_a_best=int((h["best_score"] > 0).sum()), unique_best=int((h["n_best"] == 1).sum()),
                  mean_best_score=round(float(h["best_score"].mean()), 2), mean_placements=round(float(h["n_placements"].mean()), 2),
                  mean_best_mems=round(float(h["best_mems"].mean()), 3)))
    b.free()
    idx.close()
    if not a.no_cli:
        cli_walls(ri, tags, cat, offs, a.steps, caps[0], emit)


if __name__ == "__main__":
    main()
