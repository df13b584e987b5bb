"""Child process of tests/test_gpu_tag_records.py: one batch run RUNS times under the environment it was started with (PGX_SCAN_THREE is
read once per process); the result arrays of every run and the batch's spec_stats() behind it are written for the parent to compare.
usage: tag_records_child.py RI TAGS READS.npz OUT.npz MIN_LEN MIN_OCC RUNS"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))

import pgx_ffi as P  # noqa: E402


def main(argv):
    ri, tags, reads, out = argv[:4]
    min_len, min_occ, runs = (int(a) for a in argv[4:7])
    d = np.load(reads)
    idx = P.Index(ri, tags)
    b = idx.batch(d["cat"], d["offs"])
    arrays = {}
    for k in range(runs):
        b.run(min_len, min_occ, P.RUN_TAGS)
        for name, v in b.result().items():
            arrays["%s_%d" % (name, k)] = np.asarray(v)
        arrays["spec_stats_%d" % k] = np.array(b.spec_stats(), dtype=np.int64)
    b.free()
    idx.close()
    np.savez(out, **arrays)


if __name__ == "__main__":
    main(sys.argv[1:])
