"""pgx_pack on bench.py's workloads: the coverage of every graph base, accumulated on the device.

  python3 scripts/read_pack_bench.py [--workload synth|chr22] [--reads N] [--haps H] [--base-len L] [--steps 3] [--cap 64] [--out FILE]

One batch of --reads 150-bp reads of the workload (bench.py's cache directory and reads), min_len 20 / min_occ 1, run with
PGX_RUN_TAGS | PGX_RUN_TIMING, pgx_batch_locate(0, --cap), pgx_batch_read_place(0), pgx_batch_read_verify(1, 4) and
pgx_batch_read_align(8, PGX_ALIGN_CIGAR), as scripts/read_walk_bench.py.  The workloads' synthetic tags have offset 0 everywhere: every text
position is a visit of one symbol, so the fold's projection never reuses a visit -- its worst case.  The 150 M read bases do not spread over the
64 M positions: on the synthetic index the fold projects 27 % of the text (profiles/read_pack_bench.txt).  All comparisons are made in this invocation:
  table        pgx_pack_create's node table (ms_table: max id, visit lengths, the scan), events on the pack's stream; the bytes of the pack
  add          pgx_pack_add, one warm-up call and the median of --steps (the growth of ms_add_total), against
                 a device-to-device copy of the bytes it reads (64 B of align record a read, the operations and their offsets),
                 the walk stage with PGX_WALK_STEPS (ms_walk),
                 the pinned download of the step list, which is what the host route would need instead,
               and as a share of ms_align
  fold         pgx_pack_finish behind each add (ms_fold: tile sums, scan, fold kernel, summary; the download is not in it), the positions it
               projects, against a device-to-device copy of the 4 n bytes of tdiff; and the fold of an all-zero tdiff (a second finish)
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
from read_hits_bench import copy_ms, median  # noqa: E402


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
    n_reads = len(offs) - 1
    b.locate(0, a.cap)
    P._check(b.L.pgx_batch_read_place(b.b, 0, None))
    P._check(b.L.pgx_batch_read_verify(b.b, 1, 4, 0, None))
    ms_align = []
    for i in range(a.steps + 1):
        P._check(b.L.pgx_batch_read_align(b.b, 8, P.ALIGN_CIGAR, None))
        if i:
            ms_align.append(b.device_aligned()["ms_align"])
    n_ops = b.device_aligned()["n_ops"]
    ma = median(ms_align)
    emit(dict(workload=desc, reads=n_reads, n_sequences=int(info.n_sequences), bwt_size=int(info.bwt_size), find_mems_step_ms=round(step_ms, 3), cap=a.cap, n_ops=n_ops,
              ops_per_read=round(n_ops / n_reads, 3), ms_align=round(ma, 4)))
    ms_walk = []
    for i in range(a.steps + 1):  # (the first call builds the WALK image)
        P._check(b.L.pgx_batch_read_walk(b.b, P.WALK_STEPS, None))
        if i:
            ms_walk.append(b.device_walked()["ms_walk"])
    n_steps = b.device_walked()["n_steps"]
    pack = P.Pack(idx)
    first = pack.finish()
    n = first["n_text"]
    emit(dict(table="node table", ms_table=round(first["ms_table"], 4), n_nodes=first["n_nodes"], n_bases=first["n_bases"], n_text=n,
              pack_bytes=4 * (n + 1) + 4 * first["n_bases"] + 12 * (first["n_nodes"] + 1), summary_bytes=16 * first["n_nodes"], ms_fold_of_nothing=round(first["ms_fold"], 4)))
    adds, folds, projected, seen = [], [], [], first["n_projected"]
    for i in range(a.steps + 1):
        t0 = pack.device_result()["ms_add_total"]
        pack.add(b)
        t1 = pack.device_result()["ms_add_total"]
        out = pack.finish()
        if i:
            adds.append(t1 - t0)
            folds.append(out["ms_fold"])
            projected.append(out["n_projected"] - seen)
        seen = out["n_projected"]
    m_add, m_fold, mw = median(adds), median(folds), median(ms_walk)
    read_bytes = 64 * n_reads + 4 * n_ops + 8 * (n_reads + 1)
    c_read = copy_ms(read_bytes, False, a.steps)
    c_steps = copy_ms(8 * n_steps, True, a.steps)
    emit(dict(add="pgx_pack_add", ms_add=round(m_add, 4), ms_all=[round(x, 4) for x in adds], reads_per_s=round(n_reads / (m_add * 1e-3), 1), bytes_read=read_bytes,
              d2d_copy_ms=round(c_read, 4), vs_d2d_copy=round(m_add / c_read, 2), ms_walk_steps=round(mw, 4), vs_walk_steps=round(m_add / mw, 4), n_steps=n_steps,
              step_list_bytes=8 * n_steps, step_list_download_ms=round(c_steps, 4), vs_step_list_download=round(m_add / c_steps, 5), vs_align=round(m_add / ma, 5),
              vs_find_mems_step=round(m_add / step_ms, 4), reads_counted=out["reads_counted"] // (a.steps + 1), bases_added=out["bases_added"] // (a.steps + 1)))
    c_tdiff = copy_ms(4 * n, False, a.steps)
    again = pack.finish()
    emit(dict(fold="pgx_pack_finish", ms_fold=round(m_fold, 4), ms_all=[round(x, 4) for x in folds], positions_projected=int(median(projected)), share_of_text=round(median(projected) / n, 4),
              tdiff_bytes=4 * n, d2d_copy_ms=round(c_tdiff, 4), vs_d2d_copy=round(m_fold / c_tdiff, 2), ms_fold_all_zero=round(again["ms_fold"], 4),
              vs_align=round(m_fold / ma, 5), covered_bases=int((out["cov"] != 0).sum()), max_cov=int(out["cov"].max()) if len(out["cov"]) else 0))
    pack.close()
    b.free()
    idx.close()


if __name__ == "__main__":
    main()
