"""build_tags stage timings (GPU box): python3 -u scripts/build_tags_bench.py [--sizes 4000000,40000000] [--haps 8] [--reps 3]

Device stages (suffix array, tag of every row, run encoding) and the file write of pgx_build_tags_paths on the synthetic
pangenomes of bench.py (base_len x haps x 2 strands: 4 M -> n = 64 M, 40 M -> the chr22-scale 640 M), indexes taken from the
bench's cache directory (built there when missing).  The graph: one node per 32 bp of every haplotype, ids not shared between
haplotypes, the reverse strand walking the reversed path -- every text position has its own tag, so there is one run per
tagged row: the encoder's worst case.  No GBZ of that size exists here, so the host stages of pgx_build_tags (GBZ parse, path
extraction) are timed on the GBZ fixtures only.  One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))
sys.path.insert(0, ROOT)
import numpy as np

import pgx_ffi as P
import pgx_workload as W


def graph_of(text_path, node_bp=32):
    lens = []
    with open(text_path, "rb") as f:
        for line in f:
            lens.append(len(line) - 1)
    po, pn, nl, n_ids = [0], [], [], 0
    for k in range(0, len(lens), 2):  # forward strand, then its reverse complement (synth_pangenome_text)
        L = lens[k]
        cut = np.full(L // node_bp, node_bp, dtype=np.uint32)
        if L % node_bp:
            cut = np.append(cut, np.uint32(L % node_bp))
        ids = np.arange(n_ids + 1, n_ids + 1 + len(cut), dtype=np.uint64)  # ids from 1
        n_ids += len(cut)
        nl.append(cut)
        fwd = ids << np.uint64(1)
        for path in (fwd, fwd[::-1] | np.uint64(1)):
            pn.append(path)
            po.append(po[-1] + len(path))
    return np.array(po, dtype=np.uint64), np.concatenate(pn), np.concatenate(nl), 1


def index_for(base_len, haps):
    import bench

    wd = os.environ.get("PGX_BENCH_CACHE") or bench.cache_dir()
    os.makedirs(wd, exist_ok=True)
    name = "synth_%d_%d" % (base_len, haps)
    text, done = os.path.join(wd, name + ".txt"), os.path.join(wd, name + ".done")
    with bench.DirLock(wd):
        if not os.path.exists(done):
            t0 = time.time()
            W.synth_pangenome_text(text, base_len=base_len, n_hap=haps, seed=45)
            W.build_index_from_text(text, wd, name)
            open(done, "w").write("ok\n")
            sys.stderr.write("[build_tags_bench] index %s built in %.1f s\n" % (name, time.time() - t0))
    return os.path.join(wd, name + ".ri"), text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4000000,40000000")
    ap.add_argument("--haps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    dev = P.device_name(a.device)
    gold = os.path.join(ROOT, "tests", "golden")
    with tempfile.TemporaryDirectory() as td:
        # host stages on the fixtures: GBZ parse + path extraction (pgx_build_tags stage "graph"), gbz_extract
        for gbz, ri, fl in (("bidirectional_test/xy.gbz", "bidirectional_test/xy.ri", 0),
                            ("x.giraffe.gbz", None, P.BUILD_TAGS_FORWARD_ONLY)):
            g = os.path.join(gold, gbz)
            if ri is None:
                ri = os.path.join(td, "x.ri")
                P.build_rindex(os.path.join(gold, "x.rl_bwt"), ri)
            else:
                ri = os.path.join(gold, ri)
            best = None
            for _ in range(a.reps):
                ms = P.build_tags(g, ri, os.path.join(td, "f.tags"), device=a.device, flags=fl)
                best = ms if best is None or ms["graph"] < best["graph"] else best
            t0 = time.perf_counter()
            P.gbz_extract(g, os.path.join(td, "f.txt"), both=not fl)
            ext = (time.perf_counter() - t0) * 1e3
            print(json.dumps({"what": "fixture", "gbz": gbz, "stages_ms": best, "gbz_extract_ms": round(ext, 3), "device": dev}), flush=True)
        for base_len in (int(x) for x in a.sizes.split(",")):
            ri, text = index_for(base_len, a.haps)
            t0 = time.time()
            po, pn, nl, fid = graph_of(text)
            graph_s = time.time() - t0
            out = os.path.join(td, "synth.tags")
            runs = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ms = P.build_tags_paths(ri, po, pn, nl, fid, out, device=a.device)
                ms["call_total"] = (time.perf_counter() - t0) * 1e3
                runs.append(ms)
            size = os.path.getsize(out)
            inf = P.Index(ri).info()
            n, n_seq = int(inf.bwt_size), int(inf.n_sequences)
            med = {k: round(float(np.median([r[k] for r in runs])), 2) for k in runs[0]}
            print(json.dumps({"what": "synthetic", "base_len": base_len, "haps": a.haps, "n": n, "n_seq": n_seq, "path_nodes": int(len(pn)),
                              "node_bp": 32, "file_bytes": size, "reps": a.reps, "median_ms": med,
                              "all_ms": [{k: round(v, 2) for k, v in r.items()} for r in runs],
                              "tables_from_text_s": round(graph_s, 2), "device": dev}), flush=True)
            os.remove(out)


if __name__ == "__main__":
    main()
