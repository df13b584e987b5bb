"""Reads as text, parsed on the device (pgx_batch_upload_text), against the host's line split + pgx_batch_upload.

  python3 scripts/fastx_bench.py [--upload-reads 262144,1048576] [--cli-reads 16000000] [--kernels] [--workdir DIR]

150-bp reads sampled by pgx_workload from the x index (tests/golden/x.rl_bwt), written as lines, FASTQ, FASTA and FASTA wrapped at 60.
1. wall time of one upload per batch (host clock around the call, which ends in a synchronise; pinned text; median of 5), as GB/s of
   input, next to pgx_batch_upload of the same reads (pinned bytes + offsets);
2. the find_mems CLI on --cli-reads reads per format (PGX_CLI_STATS=1 busy seconds), line files host- and device-parsed, outputs
   compared byte for byte;
--kernels: only a few 2^20-read FASTQ uploads (the run to put under rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))
import pgx_ffi as P  # noqa: E402
import pgx_workload as W  # noqa: E402

L = 150


def texts(cat, n):
    """the four formats of n reads of L bytes, built column-wise"""
    s = np.asarray(cat, np.uint8).reshape(n, L)
    out = {}
    t = np.full((n, L + 1), 10, np.uint8)
    t[:, :L] = s
    out["lines"] = t.reshape(-1)
    t = np.empty((n, 2 * L + 7), np.uint8)
    t[:, 0:3] = np.frombuffer(b"@r\n", np.uint8)
    t[:, 3:3 + L] = s
    t[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", np.uint8)
    t[:, 6 + L:6 + 2 * L] = 73
    t[:, 6 + 2 * L] = 10
    out["fastq"] = t.reshape(-1)
    t = np.empty((n, L + 4), np.uint8)
    t[:, 0:3] = np.frombuffer(b">r\n", np.uint8)
    t[:, 3:3 + L] = s
    t[:, 3 + L] = 10
    out["fasta"] = t.reshape(-1)
    t = np.empty((n, L + 6), np.uint8)  # 60 + 60 + 30 columns
    t[:, 0:3] = np.frombuffer(b">r\n", np.uint8)
    t[:, 3:63], t[:, 63] = s[:, 0:60], 10
    t[:, 64:124], t[:, 124] = s[:, 60:120], 10
    t[:, 125:155], t[:, 155] = s[:, 120:150], 10
    out["fasta60"] = t.reshape(-1)
    return out


FMT = {"lines": P.READS_LINES, "fastq": P.READS_FASTQ, "fasta": P.READS_FASTA, "fasta60": P.READS_FASTA}


def pinned(a):
    p = P.pinned_array(len(a), np.uint8)
    p[:] = a
    return p


def timed(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def upload_leg(idx, seqs, n, seed, only_fastq=False):
    cat, offs = W.sample_reads(seqs, n, L, seed=seed)
    rows = []
    b = idx.batch_empty()
    try:
        if not only_fastq:
            pc, po = pinned(cat), P.pinned_array(len(offs), np.uint64)
            po[:] = offs
            t = timed(lambda: b.upload(pc, po))
            rows.append(dict(reads=n, input="bytes+offsets (pgx_batch_upload)", bytes=int(len(cat) + 8 * len(offs)), s=t,
                             gb_s=(len(cat) + 8 * len(offs)) / t / 1e9))
        for name, text in texts(cat, n).items():
            if only_fastq and name != "fastq":
                continue
            pt = pinned(text)
            assert b.upload_text(pt, FMT[name]) == n
            t = timed(lambda: b.upload_text(pt, FMT[name]))
            rows.append(dict(reads=n, input=name + " (pgx_batch_upload_text)", bytes=int(len(text)), s=t, gb_s=len(text) / t / 1e9))
    finally:
        b.free()
    return rows


def _prefix(path):
    """bytes of the output before the timing lines"""
    sz = os.path.getsize(path)
    with open(path, "rb") as f:
        f.seek(max(0, sz - 4096))
        tail = f.read()
    k = tail.rfind(b"\nTotal time for finding all MEMs")
    return sz - len(tail) + k if k >= 0 else sz


def same_text(a, b):
    na, nb = _prefix(a), _prefix(b)
    if na != nb:
        return False
    with open(a, "rb") as fa, open(b, "rb") as fb:
        left = na
        while left:
            k = min(left, 64 << 20)
            if fa.read(k) != fb.read(k):
                return False
            left -= k
    return True


def cli_leg(ri, tags, seqs, n, wd):
    cli = os.path.join(ROOT, "pangenome-index_amd", "find_mems")
    cat, offs = W.sample_reads(seqs, n, L, seed=99)
    rows, first = [], None
    runs = [("lines", []), ("lines", ["--device-parse"]), ("fastq", ["--reads-format", "fastq"]), ("fasta", ["--reads-format", "fasta"]),
            ("fasta60", ["--reads-format", "fasta"])]
    cur = None
    all_texts = None
    for name, extra in runs:
        if cur != name:
            if all_texts is None:
                all_texts = texts(cat, n)
            path = os.path.join(wd, "reads." + name)
            all_texts[name].tofile(path)
            cur = name
        out = os.path.join(wd, "out_%s_%d.txt" % (name, len(extra)))
        t0 = time.perf_counter()
        with open(out, "wb") as fo:
            r = subprocess.run([cli, ri, tags, path, "10", "1", "--quiet"] + extra, stdout=fo, stderr=subprocess.PIPE, text=True,
                               env=dict(os.environ, PGX_CLI_STATS="1"), timeout=900)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise SystemExit("find_mems failed (%s %s): %s" % (name, extra, r.stderr[-2000:]))
        m = re.search(r"\[find_mems\] pipeline .*", r.stderr)
        same = True
        if first is None:
            first = out
        else:
            same = same_text(first, out)
            os.remove(out)
        rows.append(dict(reads=n, input=name, options=" ".join(extra), file_bytes=int(os.path.getsize(path)), wall_s=wall,
                         stats=m.group(0) if m else "", same_output_as_lines_host=same))
        print(json.dumps(rows[-1]), flush=True)
        if name != "lines" or extra:
            os.remove(path)
    os.remove(first)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--upload-reads", default="262144,1048576")
    ap.add_argument("--cli-reads", type=int, default=16_000_000)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--workdir", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "pgx_fastx_bench"))
    args = ap.parse_args()
    os.makedirs(args.workdir, exist_ok=True)
    g = os.path.join(ROOT, "tests", "golden")
    ri, tags = W.build_index_from_rlbwt(os.path.join(g, "x.rl_bwt"), args.workdir, "x")[:2]
    seqs = W.load_sequences(os.path.join(g, "x.newline_separated"))
    idx = P.Index(ri, tags)
    print("# device: %s" % P.device_name(0), flush=True)
    if args.kernels:
        for row in upload_leg(idx, seqs, 1 << 20, 5, only_fastq=True):
            print(json.dumps(row), flush=True)
        return
    for n in [int(x) for x in args.upload_reads.split(",") if x]:
        for row in upload_leg(idx, seqs, n, 5):
            print(json.dumps(row), flush=True)
    if args.cli_reads:
        cli_leg(ri, tags, seqs, args.cli_reads, args.workdir)


if __name__ == "__main__":
    main()
