"""pgx_batch_read_walk on bench.py's workloads: every aligned read as a walk through the graph, on the device.

  python3 scripts/read_walk_bench.py [--workload synth|chr22] [--reads N] [--haps H] [--base-len L] [--steps 3] [--cap 64] [--out FILE]

One batch of --reads 150-bp reads of the workload (bench.py's cache directory and reads), min_len 20 / min_occ 1, run with
PGX_RUN_TAGS | PGX_RUN_TIMING, pgx_batch_locate(0, --cap), pgx_batch_read_place(0), pgx_batch_read_verify(1, 4) and pgx_batch_read_align(8, 0),
then pgx_batch_read_walk with and without PGX_WALK_STEPS.  One warm-up call, then the median of --steps, for:
  ms_walk      device events around the whole stage (count kernel, scan, the read-back of the number of steps, fill kernel)
  bytes        what the stage must move by the model: per read 64 B of align record in, 32 B of record out, 24 B of counts, first visits and
               offsets written and 24 B of them read again, two rank lookups of 8 B of directory and up to 64 B of marks each and two bit scans of
               at least 8 B; with PGX_WALK_STEPS 16 B a step (8 read from the image, 8 written); over ms_walk as a share of 8 TB/s
  copy floor   a device-to-device copy of that many bytes, timed with events in this invocation
  ms_align, ms_verify   the stages before it, in the same invocation, and the find_mems step itself
  image        the WALK image's build on both routes, from the line PGX_IMAGE_TIMING prints: wall time (the TEXT image was built before by the verify
               stage) and bytes.  The workloads' synthetic tags have offset 0 everywhere: every text position is a visit of one symbol, the
               image's worst case (8 bytes of node per position) and the list's (150 steps a read).
Rows are JSON lines; --out also appends them to a file."""
import argparse
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench  # noqa: E402
import pgx_ffi as P  # noqa: E402
from read_hits_bench import HBM_PEAK, copy_ms, median  # noqa: E402


def stderr_of(call):
    """what the library writes to file descriptor 2 during call()"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return f.read().decode(errors="replace")


def image_row(text):
    m = re.search(r"walk image \((\w+) route\): ([0-9.]+) ms wall; (\d+) bytes \((\d+) marks \+ directory, (\d+) visits\)", text)
    return dict(image_route=m.group(1), image_build_ms=float(m.group(2)), image_bytes=int(m.group(3)), marks_and_directory_bytes=int(m.group(4)), visits=int(m.group(5))) if m else \
        dict(image="no timing line", stderr=text[-300:])


def chain(b, cap):
    b.locate(0, cap)
    P._check(b.L.pgx_batch_read_place(b.b, 0, None))
    P._check(b.L.pgx_batch_read_verify(b.b, 1, 4, 0, None))
    P._check(b.L.pgx_batch_read_align(b.b, 8, 0, None))


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
    os.environ["PGX_IMAGE_TIMING"] = "1"
    idx = P.Index(ri, tags)
    info = idx.info()
    b = P.Batch(idx, cat, offs)
    b.run(20, 1, P.RUN_TAGS | P.RUN_TIMING)  # (the first run builds the LCE image where the index has one)
    b.run(20, 1, P.RUN_TAGS | P.RUN_TIMING)
    step_ms = b.timing().ms_total
    n_reads = len(offs) - 1
    emit(dict(workload=desc, reads=n_reads, n_mems=int(b.counts()[0]), n_sequences=int(info.n_sequences), bwt_size=int(info.bwt_size), find_mems_step_ms=round(step_ms, 3)))
    chain(b, a.cap)
    ms_verify, ms_align = [], []
    for i in range(a.steps):
        P._check(b.L.pgx_batch_read_verify(b.b, 1, 4, 0, None))
        ms_verify.append(b.device_verified()["ms_verify"])
    for i in range(a.steps):
        P._check(b.L.pgx_batch_read_align(b.b, 8, 0, None))
        ms_align.append(b.device_aligned()["ms_align"])
    emit(dict(cap=a.cap, ms_verify=round(median(ms_verify), 4), ms_align=round(median(ms_align), 4)))
    emit(image_row(stderr_of(lambda: P._check(b.L.pgx_batch_read_walk(b.b, 0, None)))))  # (the first call builds the image)
    for flags in (0, P.WALK_STEPS):
        rows = []
        for i in range(a.steps + 1):
            P._check(b.L.pgx_batch_read_walk(b.b, flags, None))
            if i:
                rows.append(b.device_walked())
        d = rows[-1]
        m = median([r["ms_walk"] for r in rows])
        model = n_reads * (64 + 32 + 24 + 24 + 2 * (8 + 64) + 2 * 8) + (16 * d["n_steps"] if flags else 0)
        floor = copy_ms(model, False, a.steps)
        emit(dict(steps_list=bool(flags), ms_walk=round(m, 4), ms_all=[round(r["ms_walk"], 4) for r in rows], n_steps=d["n_steps"], reads_per_s=round(n_reads / (m * 1e-3), 1),
                  vs_align=round(m / median(ms_align), 4), vs_verify=round(m / median(ms_verify), 4), vs_find_mems_step=round(m / step_ms, 4), model_bytes=model,
                  hbm_fraction=round(model / (m * 1e-3) / HBM_PEAK, 4), d2d_copy_ms=round(floor, 4), vs_d2d_copy=round(m / floor, 2)))
    w = b.read_walk(0)["reads"]
    has = w["n_steps"] > 0
    emit(dict(walked="summary", reads_with_steps=int(has.sum()), mean_steps=round(float(w["n_steps"][has].mean()), 3) if has.any() else 0,
              mean_path_len=round(float(w["path_len"][has].mean()), 3) if has.any() else 0))
    b.free()
    idx.close()
    # the other route: a second handle without an LCE image, its walk image built by a small batch
    os.environ["PGX_FM_LCE"] = "0"
    idx = P.Index(ri, tags)
    k = min(n_reads, 1000)
    b = P.Batch(idx, cat[: int(offs[k] - offs[0])], offs[: k + 1] - offs[0])
    b.run(20, 1, P.RUN_TAGS)
    chain(b, a.cap)
    emit(image_row(stderr_of(lambda: P._check(b.L.pgx_batch_read_walk(b.b, 0, None)))))
    b.free()
    idx.close()


if __name__ == "__main__":
    main()
