"""pgx_batch_locate on bench.py's workloads: the occurrences of every MEM of a batch, on the device.

  python3 scripts/mem_locate_bench.py [--reads 10000000] [--workload chr22|synth] [--steps 3] [--wide] [--kernels]

One batch of --reads 150-bp reads of the workload (bench.py's cache directory and reads), min_len 20 / min_occ 1, run with
PGX_RUN_TAGS | PGX_RUN_TIMING.  For each flag form (0, PGX_LOCATE_SEQ_IDS, PGX_LOCATE_SEQ_SETS, PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE as routed
through the sequence sets, and the same with PGX_LOCATE_SETS=0 = the segmented sort, side by side in one invocation) and each device path
(the resident suffix array where the index has one, the sample chains with PGX_LOCATE_CHAINS): n_mems, sum of size, n_values, the device
time of pgx_batch_locate (events around the call on the batch's stream; median of --steps), values / s, the time against the run's
device time (ms_total of the find_mems step), and for the resident path the bytes model -- 4 B read + 8 B written per value + 32 B per
MEM; the set forms write 8 W B per MEM in place of the values -- against 8 TB/s.  --forms picks rows by their name (comma-separated).  --wide: the index opened with PGX_MODE_IMAGE_WIDE (no LCE image: the chains alone).  --kernels: one locate per
form and path after the run, nothing else (the run to put under rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import pgx_ffi as P  # noqa: E402

HBM_PEAK = 8.0e12
# (flags, name, PGX_LOCATE_SETS for the calls: None = unset)
FORMS = ((0, "packed positions", None), (P.LOCATE_SEQ_IDS, "sequence ids", None), (P.LOCATE_SEQ_SETS, "sequence sets", None),
         (P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE, "unique sequence ids", None), (P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE, "unique sequence ids (sort)", "0"))


def loc_on_device(flags):
    """the value forms stay on the device (tens of GB at the bench shape); only their header is read"""
    return not (flags & (P.LOCATE_SEQ_SETS | P.LOCATE_UNIQUE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--workload", default="chr22", choices=("chr22", "synth"))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--forms", default="", help="comma-separated row names (default: all)")
    ap.add_argument("--paths", default="resident,chains")
    a = ap.parse_args()
    args = bench.parse(["--workload", a.workload, "--reads", str(a.reads)])
    wd = args.workdir or bench.cache_dir()
    os.makedirs(wd, exist_ok=True)
    with bench.DirLock(wd):
        ri, tags, cat, offs, desc, _ = bench.make_workload(args, a.workload, 0, wd, lambda: None, a.reads, args.base_len)
    idx = P.Index(ri, tags, mode=P.MODE_COMPAT | (P.MODE_IMAGE_WIDE if a.wide else 0))
    b = P.Batch(idx, cat, offs)
    b.run(20, 1, P.RUN_TAGS | P.RUN_TIMING)  # (the first run builds the LCE image where the index has one)
    b.run(20, 1, P.RUN_TAGS | P.RUN_TIMING)
    t = b.timing()
    n_mems, _, _ = b.counts()
    mems = b.result()["mems"]
    sum_size = int(mems["size"].astype(np.int64).sum())
    rows = []
    want = [w.strip() for w in a.forms.split(",") if w.strip()]
    for flags, what, sets_env in FORMS:
        if want and what not in want:
            continue
        for chains in (False, True):
            if ("chains" if chains else "resident") not in a.paths.split(","):
                continue
            f = flags | (P.LOCATE_CHAINS if chains else 0)
            if sets_env is None:
                os.environ.pop("PGX_LOCATE_SETS", None)
            else:
                os.environ["PGX_LOCATE_SETS"] = sets_env  # (read per call)
            ms = []
            if not a.kernels:
                b.locate(f)  # warm-up: buffers of this form
            for _ in range(1 if a.kernels else a.steps):
                b.locate(f)
                loc = b.device_locations() if loc_on_device(f) else b.locations()
                ms.append(loc["ms_locate"])
            os.environ.pop("PGX_LOCATE_SETS", None)
            if not chains and not loc["resident"] and not a.wide:
                print("[mem_locate_bench] no resident suffix array on this index: the chains serve both rows", file=sys.stderr)
            m = float(np.median(ms))
            row = dict(form=what, flags=flags, path="chains" if chains or not loc["resident"] else "resident", n_mems=int(n_mems), sum_size=sum_size,
                       n_values=loc["n_values"], set_words=loc["set_words"], ms_locate=round(m, 3), ms_all=[round(float(x), 3) for x in ms], values_per_s=round(sum_size / (m * 1e-3), 1) if m else None,
                       vs_find_mems_step=round(m / t.ms_total, 3) if t.ms_total else None)
            if row["path"] == "resident":
                byts = (4.0 * sum_size + (32.0 + 8.0 * loc["set_words"]) * n_mems) if loc["set_words"] else 12.0 * sum_size + 32.0 * n_mems
                row["model_bytes"] = int(byts)
                row["hbm_fraction"] = round(byts / (m * 1e-3) / HBM_PEAK, 3) if m else None
            rows.append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps(dict(workload=desc, reads=a.reads, wide=a.wide, find_mems_step_ms=round(t.ms_total, 3), bwt_size=idx.info().bwt_size,
                          n_sequences=idx.info().n_sequences)), flush=True)
    b.free()
    idx.close()


if __name__ == "__main__":
    main()
