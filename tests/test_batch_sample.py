"""CPU tier: tests/batch_sample.py, the helper the full-size GPU tests check late reads of big batches with.

A subset of a whole-batch oracle result must equal the oracle run on just those reads (results are independent per read), and `compare`
must fail on a single corrupted MEM or position of a late read and name that read -- so the GPU checks built on it cannot pass vacuously."""
import os

import numpy as np
import pytest

import batch_sample as S
import oracle_ffi as O
import pgx_workload as W


@pytest.fixture(scope="module")
def x_batch(x_index, golden):
    """3000 sampled reads of x, some replaced by reads of other lengths, with N, lower case, or empty; the oracle on all of them"""
    ri_path, tags_path = x_index
    seqs = W.load_sequences(os.path.join(golden, "x.newline_separated"))
    cat, offs = W.sample_reads(seqs, 3000, 150, seed=31)
    reads = [bytes(cat[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)]
    for i in range(7, len(reads), 97):
        r = reads[i]
        reads[i] = (r[:40], r[:75] + b"N" + r[76:], r.lower(), b"", r[:19], r + r[:60])[(i // 97) % 6]
    cat, offs = O.pack_reads(reads)
    ri, tags = O.RIndex(ri_path), O.Tags(tags_path, O.TAGS_COMPACT)
    full = O.find_mems_batch(ri, tags, cat, offs, 10, 1, threads=O.lib().orc_max_threads())
    return ri, tags, cat, offs, full


def _ids(n):
    rng = np.random.default_rng(5)
    return {
        "first": np.array([0]),
        "last": np.array([n - 1]),
        "stride": np.arange(3, n, 61),
        "random": np.unique(rng.integers(0, n, size=400)),
        "mixed": S.sample_ids(np.zeros(n + 1), seed=9, stride=61, tail=200, n_random=100, extra=[0, 1, 2]),
    }


def test_subset_equals_the_oracle_on_the_subset(x_batch):
    ri, tags, cat, offs, full = x_batch
    n = len(offs) - 1
    assert len(full["mems"]) > n and len(full["positions"]) > len(full["mems"])
    for name, ids in _ids(n).items():
        scat, soffs = S.gather_reads(cat, offs, ids)
        assert len(soffs) == len(ids) + 1 and all(bytes(scat[int(soffs[k]):int(soffs[k + 1])]) == bytes(cat[int(offs[i]):int(offs[i + 1])])
                                                  for k, i in enumerate(ids))
        ref = O.find_mems_batch(ri, tags, scat, soffs, 10, 1, threads=O.lib().orc_max_threads())
        sub = S.subset(full, ids)
        S.compare(sub, ref, ids, what=name)
        for k in S.ARRAYS:
            assert sub[k].dtype == ref[k].dtype and len(sub[k]) == len(ref[k]), (name, k)
    # the whole batch as its own subset
    S.compare(S.subset(full, np.arange(n)), full)


def test_non_acgt_reads(x_batch):
    _, _, cat, offs, _ = x_batch
    ids = S.non_acgt_reads(cat, offs)
    want = [i for i in range(len(offs) - 1) if set(bytes(cat[int(offs[i]):int(offs[i + 1])])) - set(b"ACGT")]
    assert len(want) >= 8 and ids.tolist() == want


def _late_read(full, n):
    """a read near the end of the batch with at least two MEMs, the second of which has positions"""
    mo, po = full["mem_offsets"], full["pos_offsets"]
    for r in range(n - 5, 0, -1):
        if mo[r + 1] - mo[r] >= 2 and po[mo[r] + 2] > po[mo[r] + 1]:
            return r
    raise AssertionError("no read with two MEMs")


@pytest.mark.parametrize("what", ["position", "mem", "both", "run_count"])
def test_compare_names_a_corrupted_late_read(x_batch, what):
    ri, tags, cat, offs, full = x_batch
    n = len(offs) - 1
    r = _late_read(full, n)
    bad = {k: full[k].copy() for k in S.ARRAYS}
    m = int(full["mem_offsets"][r]) + 1  # the read's second MEM
    if what in ("position", "both"):
        bad["positions"][int(full["pos_offsets"][m])] ^= 1
    if what in ("mem", "both"):
        bad["mems"]["end"][m] += 1
    if what == "run_count":
        bad["tag_run_counts"][m] += 1
    with pytest.raises(AssertionError, match="read id %d \\(position %d of %d" % (r, r, n)):
        S.compare(bad, full)
    # the same read inside a sample of the batch: named by its read id, at its position in the sample
    ids = S.sample_ids(offs, seed=3, stride=61, tail=50, n_random=20, extra=[r])
    k = int(np.searchsorted(ids, r))
    ref = O.find_mems_batch(ri, tags, *S.gather_reads(cat, offs, ids), 10, 1, threads=O.lib().orc_max_threads())
    S.compare(S.subset(full, ids), ref, ids)
    with pytest.raises(AssertionError, match="read id %d \\(position %d of %d" % (r, k, len(ids))):
        S.compare(S.subset(bad, ids), ref, ids)


def test_compare_names_a_read_with_a_missing_mem(x_batch):
    """a read that lost its last MEM: the offsets differ from that read on, and everything after it is misaligned"""
    _, _, cat, offs, full = x_batch
    n = len(offs) - 1
    r = _late_read(full, n)
    mo = full["mem_offsets"].astype(np.int64)
    drop = int(mo[r + 1]) - 1
    bad = dict(full)
    bad["mem_offsets"] = full["mem_offsets"].copy()
    bad["mem_offsets"][r + 1:] -= np.uint64(1)
    po = full["pos_offsets"].astype(np.int64)
    cnt = int(po[drop + 1] - po[drop])
    bad["mems"] = np.delete(full["mems"], drop)
    bad["tag_run_counts"] = np.delete(full["tag_run_counts"], drop)
    bad["pos_offsets"] = np.delete(full["pos_offsets"], drop + 1)
    bad["pos_offsets"][drop + 1:] -= np.uint64(cnt)
    bad["positions"] = np.delete(full["positions"], np.arange(po[drop], po[drop + 1]))
    with pytest.raises(AssertionError, match="read id %d .*mem_offsets" % r):
        S.compare(bad, full)
    # totals: a different extension count alone is caught only where it is compared
    bad2 = dict(full)
    bad2["n_extensions"] = full["n_extensions"] + 1
    S.compare(bad2, full)
    with pytest.raises(AssertionError, match="n_extensions"):
        S.compare(bad2, full, totals=True)
