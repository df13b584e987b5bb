"""Child process of tests/test_gpu_knobs.py: one batch under the environment it was started with (PGX_SCAN_THREE is read once per
process), its result arrays written for the parent to compare.
usage: scan_three_child.py RI TAGS MODE READS.npz OUT.npz WITH_TAGS MIN_LEN MIN_OCC [MIN_LEN MIN_OCC ...]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pangenome-index_amd"))

import pgx_ffi as P  # noqa: E402


def main(argv):
    ri, tags, mode, reads, out, with_tags = argv[0], argv[1], int(argv[2]), argv[3], argv[4], int(argv[5])
    params = [int(a) for a in argv[6:]]
    d = np.load(reads)
    idx = P.Index(ri, tags, mode=mode)
    b = idx.batch(d["cat"], d["offs"])
    arrays = {}
    for k in range(len(params) // 2):
        b.run(params[2 * k], params[2 * k + 1], P.RUN_TAGS if with_tags else 0)
        res = b.result()
        for name, v in res.items():
            arrays["%s_%d" % (name, k)] = np.asarray(v)
    b.free()
    idx.close()
    np.savez(out, **arrays)


if __name__ == "__main__":
    main(sys.argv[1:])
