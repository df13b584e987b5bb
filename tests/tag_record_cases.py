"""Case tables for the list records of the tag stage (test_gpu_tag_records.py): batches in which every list is appended to from every locate
workgroup, identical large queries whose copies lie in other workgroups' parts of the list than their representative, and batches whose MEM totals
sit on the tile borders of the scan that places the one-run queries' values.  Built on border_cases.py's tag arrays and SpecCase;
test_tag_record_cases.py asserts on the CPU that the tables hold what they claim."""
import numpy as np

import border_cases as B

LOCATE_WG = 1024       # PGX_TAG_LOCATE_THREADS: queries per workgroup of pgx_tag_locate_kernel (one list atomic per workgroup)
SCAN_TILE = 4096       # PGX_SCAN1_TILE_ITEMS: queries per tile of pgx_scan_tag_tail_kernel
N_MIXED = 3 * LOCATE_WG + 1  # three full workgroups and a ragged fourth

CLASSES = ("inverted", "single", "small", "big", "large", "scratch")


def record_class(c):
    """the six classes a window of the mixed batch has to hold: no run, one run (answered by the locate kernel), the small, big and large lists,
    and the large list's queries beyond the workgroup's LDS"""
    if c == 0:
        return "inverted"
    if c == 1:
        return "single"
    if c <= B.TAG_SMALL:
        return "small"
    if c <= B.SORT_LDS_CAP:
        return "big"
    return "large" if c <= B.SORT_WG_LDS_CAP else "scratch"


def windows(n):
    """the locate workgroup (in a launch of one round per workgroup) of each of n queries"""
    return np.arange(n) // LOCATE_WG


def _queries(arr, fc):
    """(start, end) arrays of (f, c) pairs; c == 0: the inverted query in front of run f - 1 (0-based), [starts[f - 1], starts[f - 1] - 1]"""
    st = np.zeros(len(fc), dtype=np.uint64)
    en = np.zeros(len(fc), dtype=np.uint64)
    for i, (f, c) in enumerate(fc):
        if c == 0:
            st[i], en[i] = arr.starts[f - 1], arr.starts[f - 1] - np.uint64(1)
        else:
            st[i], en[i] = arr.query(f, c)
    return st, en


def mixed_batch():
    """(f, c) of N_MIXED queries.  Every window of 1024: mostly one-run and small queries in random order, 96 big ones (the borders 17, 64, 65,
    2048 among them), four large ones, one beyond 16384 runs and eight inverted ones, at first runs of every residue mod 10; the ragged last
    query is a large one."""
    rng = np.random.default_rng(77)
    fc = []
    for w in range(3):
        cs = [1] * 600 + [int(c) for c in rng.integers(2, B.TAG_SMALL + 1, 315)] + [17, 64, 65, 2048] + [int(c) for c in rng.integers(18, 400, 92)]
        cs += [2049, 4097 + w, 8193, 16384] + [16385 + 100 * w] + [0] * 8
        assert len(cs) == LOCATE_WG
        cs = [cs[i] for i in rng.permutation(LOCATE_WG)]
        for c in cs:
            f = int(rng.integers(2, B.N_TAG_RUNS - max(c, 1) - 20))
            fc.append((f, c))
    fc.append((31000, 3000))
    return fc


def mixed_queries(arr):
    return _queries(arr, mixed_batch())


# identical large queries: (f, c) and how often.  The first is the bulk (more copies than the wave slice of the large path holds values, spread over
# all windows); the second ends in the last run with f % 10 == 0, so every copy reads one item beyond the array and is counted; the third sorts in
# global scratch.
DUP_GROUPS = [((12345, 2500), None), ((65000, B.N_TAG_RUNS - 65000 + 1), 6), ((20000, 16500), 4)]
DUP_DISTINCT = [(1000 + 997 * k, 2049 + 37 * k) for k in range(12)]  # large queries that are nobody's duplicate


def dup_batch():
    """(f, c) of N_MIXED queries: three of every four are copies of DUP_GROUPS[0]; the others are the copies of the two smaller groups (each in
    every full window), the distinct large queries, and one-run / small queries"""
    rng = np.random.default_rng(78)
    fc = [None] * N_MIXED
    free = [i for i in range(N_MIXED) if i % 4 == 0]
    for i in range(N_MIXED):
        if i % 4:
            fc[i] = DUP_GROUPS[0][0]
    per_window = {w: [i for i in free if i // LOCATE_WG == w] for w in range(3)}
    taken = set()
    for (f, c), copies in DUP_GROUPS[1:]:
        for k in range(copies):
            i = per_window[k % 3][5 + 7 * k + (c % 11)]
            assert i not in taken
            taken.add(i)
            fc[i] = (f, c)
    rest = [i for i in free if i not in taken]
    for k, q in enumerate(DUP_DISTINCT):
        i = rest[3 + 61 * k]
        taken.add(i)
        fc[i] = q
    for i in free:
        if i not in taken:
            c = 1 if rng.integers(0, 2) else int(rng.integers(2, B.TAG_SMALL + 1))
            fc[i] = (int(rng.integers(2, 60000)), c)
    return fc


def dup_queries(arr):
    return _queries(arr, dup_batch())


# ---- through pgx_batch_run on border_cases.SpecCase ------------------------------------------------------------------------------------------
TILE_BORDERS = (SCAN_TILE, 2 * SCAN_TILE)


def read_pool(case):
    """sampled reads (a MEM or two each) with the end of a private contig (131 one-run MEMs) or of a haplotype (131 MEMs of a few runs) after every
    fifty of them: more than 8192 MEMs of every small class in any long prefix"""
    tails, hap_tails = case.private_tails(), [bytes(s[-150:]) for s in case.haps]
    pool = []
    for i in range(48):
        pool += list(case.sampled[50 * i:50 * (i + 1)]) + [tails[i // 2] if i % 2 == 0 else hap_tails[(i // 2) % len(hap_tails)]]
    return pool


def _prefix_at(case, total):
    """number k of the pool's reads whose MEMs are the last total below `total`: mem_offsets[k] < total <= mem_offsets[k + 1]"""
    ref = case.ref("records_pool", case.full_tags, read_pool(case))[2]
    mo = ref["mem_offsets"].astype(np.int64)
    k = int(np.searchsorted(mo, total, side="left")) - 1
    assert mo[k] < total <= mo[k + 1]
    return k


def run_batches(case):
    """name -> reads, every batch on the full tag array:
    only_single   the ends of the private contigs: nothing but one-run MEMs (no list, no segment; every position stored by the scan)
    no_single     reads whose MEMs all have two or more runs: the scan stores nothing itself
    below_T / at_T  prefixes of read_pool() whose MEM total is the last below and the first at or above T = 4096, 8192"""
    # (which reads have no one-run MEM is the oracle's word: the ends of the haplotypes and the sampled reads, those with such a MEM left out)
    cand = [bytes(s[-150:]) for s in case.haps] + list(case.sampled[:600])
    ref = case.ref("records_no_single_pool", case.full_tags, cand)[2]
    mo, rc = ref["mem_offsets"].astype(np.int64), ref["tag_run_counts"]
    keep = [r for i, r in enumerate(cand) if mo[i + 1] > mo[i] and np.all(rc[mo[i]:mo[i + 1]] >= 2)]
    out = {"only_single": case.private_tails(), "no_single": keep + [case.n_read_with_size(B.SORT_LDS_CAP, 4096), case.repeat]}
    for t in TILE_BORDERS:
        k = _prefix_at(case, t)
        out["below_%d" % t] = read_pool(case)[:k]
        out["at_%d" % t] = read_pool(case)[:k + 1]
    return out


def positions_only_batches(case):
    """(A, B), the same number of reads: a run of B exceeds the positions capacity taken from a run of A and no other.  A: one query of nearly
    16384 runs, whose values (3000 different ones in the array) are mostly duplicates; B: four distinct queries of a quarter of its runs each -- the
    same number of gathered values, three times the unique ones.  The 64 of with_slack covers the three more MEMs and list entries."""
    big = case.n_read_with_size(8192, B.SORT_WG_LDS_CAP)  # (the shortest such read: the most runs)
    k = len(case.n_read_with_size(B.SORT_LDS_CAP, 4096))
    junk = B.junk_reads(8, seed=9)
    return junk + [big], junk[:5] + [b"N" * (k + 3 * j) for j in range(4)]
