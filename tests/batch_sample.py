"""Compare any subset of the reads of a batch with the oracle (tests of full-size batches).

Results are independent per read: a read's MEMs, tag run counts and positions do not depend on which other reads share its batch.
So the device result of a big batch, cut down to a sample of its reads (`subset`), must equal what the oracle computes on those reads
as a batch of their own (`gather_reads`).  `n_extensions` is a total over the batch and is compared only where both sides ran the same reads.
Everything is vectorised with numpy (gathers through np.repeat / cumsum): 10^6 read ids take seconds."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ARRAYS = ("mem_offsets", "mems", "tag_run_counts", "pos_offsets", "positions")


def _ranges(starts, lens):
    """indices [starts[k], starts[k] + lens[k]) for every k, concatenated -> (indices int64[], new offsets int64[len + 1])"""
    starts = np.asarray(starts, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    new_off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=new_off[1:])
    idx = np.arange(new_off[-1], dtype=np.int64) + np.repeat(starts - new_off[:-1], lens)
    return idx, new_off


def _ids(read_ids):
    ids = np.asarray(read_ids, dtype=np.int64)
    assert ids.ndim == 1 and (len(ids) < 2 or bool(np.all(ids[1:] > ids[:-1]))), "read ids must be sorted and distinct"
    return ids


def subset(res, read_ids):
    """the five result arrays of `res` (a whole batch) for just the reads `read_ids` (sorted), offsets rebased to 0 -- what the oracle
    returns when those reads form a batch of their own; tag arrays only if `res` has them"""
    ids = _ids(read_ids)
    mo = res["mem_offsets"].astype(np.int64)
    mem_idx, new_mo = _ranges(mo[ids], mo[ids + 1] - mo[ids])
    out = {"mem_offsets": new_mo.astype(np.uint64), "mems": res["mems"][mem_idx]}
    if "pos_offsets" in res:
        po = res["pos_offsets"].astype(np.int64)
        pos_idx, new_po = _ranges(po[mem_idx], po[mem_idx + 1] - po[mem_idx])
        out["tag_run_counts"] = res["tag_run_counts"][mem_idx]
        out["pos_offsets"] = new_po.astype(np.uint64)
        out["positions"] = res["positions"][pos_idx]
    return out


def gather_reads(cat, offs, read_ids):
    """the reads `read_ids` (sorted) of the batch (cat, offs) as a batch of their own: (cat, offsets)"""
    ids = _ids(read_ids)
    o = np.asarray(offs).astype(np.int64)
    byte_idx, new_off = _ranges(o[ids], o[ids + 1] - o[ids])
    return np.ascontiguousarray(cat[byte_idx], dtype=np.uint8), new_off.astype(np.uint64)


def non_acgt_reads(cat, offs):
    """ids of the reads with a byte outside A C G T (upper case): the reads the device hands to its other kernel"""
    o = np.asarray(offs).astype(np.int64)
    lut = np.ones(256, dtype=bool)
    lut[ACGT] = False
    at = np.flatnonzero(lut[np.asarray(cat[o[0]:o[-1]], dtype=np.uint8)]) + o[0]  # (few: positions of the bytes outside A C G T)
    return np.unique(np.searchsorted(o, at, side="right") - 1)


def sample_ids(offs, seed, stride=61, tail=20_000, n_random=2_000, random_from=0, extra=()):
    """the read ids a full-size batch is checked on: every `stride`-th read across the whole batch, the last `tail` reads, `n_random`
    reads drawn (with `seed`) from [random_from, n), and `extra` (e.g. the reads with a byte outside A C G T); sorted, distinct"""
    n = len(offs) - 1
    rng = np.random.default_rng(seed)
    parts = [np.arange(0, n, stride, dtype=np.int64), np.arange(max(0, n - tail), n, dtype=np.int64),
             rng.integers(random_from, n, size=n_random if random_from < n else 0).astype(np.int64), np.asarray(extra, dtype=np.int64)]
    return np.unique(np.concatenate(parts))


def _first_diff_rows(a, b):
    """index of the first row where two arrays (same dtype) differ over their common length, or None"""
    k = min(len(a), len(b))
    if k == 0:
        return None
    a, b = np.ascontiguousarray(a[:k]), np.ascontiguousarray(b[:k])
    if a.dtype.fields is not None:  # structured (MEMs): compare the raw bytes row by row
        a, b = a.view(np.uint8).reshape(k, -1), b.view(np.uint8).reshape(k, -1)
        d = np.flatnonzero((a != b).any(axis=1))
    else:
        d = np.flatnonzero(a != b)
    return int(d[0]) if len(d) else None


def first_difference(got, want):
    """(position in the batch of the first read whose results differ, names of the arrays that differ there), or None when all agree.
    Arrays past the first read whose count differs are misaligned and are compared only up to it."""
    if all(np.array_equal(got[k], want[k]) if k != "mems" else got[k].tobytes() == want[k].tobytes() for k in ARRAYS if k in want):
        return None
    n = len(want["mem_offsets"]) - 1
    assert len(got["mem_offsets"]) == n + 1, "the result holds %d reads, expected %d" % (len(got["mem_offsets"]) - 1, n)
    mo_g, mo_w = got["mem_offsets"].astype(np.int64), want["mem_offsets"].astype(np.int64)
    cands = {}  # array name -> first read (position in the batch) where it differs
    d = np.flatnonzero(np.diff(mo_g) != np.diff(mo_w))
    read_mo = int(d[0]) if len(d) else n
    if read_mo < n:
        cands["mem_offsets"] = read_mo
    # MEM rows agree in their read up to read_mo: rows [0, mo_w[read_mo]) are aligned
    aligned_m = int(mo_w[read_mo])
    read_of_mem = lambda j: int(np.searchsorted(mo_w, j, side="right") - 1)  # noqa: E731
    names = ["mems"] + (["tag_run_counts"] if "tag_run_counts" in want else [])
    for k in names:
        j = _first_diff_rows(got[k][:aligned_m], want[k][:aligned_m])
        if j is not None:
            cands[k] = read_of_mem(j)
    if "pos_offsets" in want:
        po_g, po_w = got["pos_offsets"].astype(np.int64), want["pos_offsets"].astype(np.int64)
        d = np.flatnonzero(np.diff(po_g[: aligned_m + 1]) != np.diff(po_w[: aligned_m + 1]))
        mem_po = int(d[0]) if len(d) else aligned_m
        if mem_po < aligned_m:
            cands["pos_offsets"] = read_of_mem(mem_po)
        aligned_p = int(po_w[mem_po])
        j = _first_diff_rows(got["positions"][:aligned_p], want["positions"][:aligned_p])
        if j is not None:
            cands["positions"] = read_of_mem(int(np.searchsorted(po_w, j, side="right") - 1))
    assert cands, "results differ, but no read could be named"
    first = min(cands.values())
    return first, sorted(k for k, v in cands.items() if v == first)


def compare(res_sub, ref, read_ids=None, totals=False, what="result"):
    """assert that `res_sub` equals `ref` read for read: MEM offsets, MEM bytes, and (where `ref` has them) tag run counts, position
    offsets and positions; `read_ids` names the reads of the batch they hold (None: reads 0 .. n - 1).  On a mismatch the AssertionError
    names the first read id that differs, its position in the batch and the arrays that differ.  totals: also n_extensions and n_tag_overflow
    (only where both sides ran the same reads)"""
    n = len(ref["mem_offsets"]) - 1
    ids = np.arange(n, dtype=np.int64) if read_ids is None else np.asarray(read_ids, dtype=np.int64)
    assert len(ids) == n, "%d read ids for a result of %d reads" % (len(ids), n)
    diff = first_difference(res_sub, ref)
    if diff is not None:
        k, arrays = diff
        raise AssertionError("%s: read id %d (position %d of %d in the batch compared) differs in %s" % (what, int(ids[k]), k, n, ", ".join(arrays)))
    if totals:
        for key in ("n_extensions", "n_tag_overflow"):
            assert res_sub[key] == ref[key], "%s: %s %d, expected %d" % (what, key, res_sub[key], ref[key])
