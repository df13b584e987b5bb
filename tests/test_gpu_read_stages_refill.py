"""GPU tier of the read stages on a batch that is refilled: one pgx_batch on the collection of 66 sequences gets six uploads in a row -- 300
reads of 150, 40 reads of 1 .. 70 bytes, no read at all, 300 other reads of 150, reads that hang over the ends of the collection's sequences,
and the first upload again -- and after each one run, locate(SEQ_SETS), read_hits, locate(0), read_place(PLACE_LIST), read_verify(16, 4,
VERIFY_LIST) and read_align(8, ALIGN_CIGAR).  Every host array of every stage equals, byte for byte, what a fresh batch gives for the same
reads: the stages' buffers grow with the largest upload and keep its tail (counts, candidate offsets, coded reads, forward cells, direction
planes, operation offsets), and nothing of it may show.  The sixth result equals the first; for the short upload the device arrays of
verify and align hold the bytes of the host arrays; once with PGX_RUN_TIMING and once without."""
import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
from test_gpu_hits import BOTH, _device_read
from test_gpu_mem_locate_sets import _collection

pytestmark = pytest.mark.gpu

SETS = P.LOCATE_SEQ_SETS
COUNTERS = dict(hits=("n_reads", "n_seq", "set_words", "flags"), place=("n_reads", "n_anchors", "n_places", "flags"),
                verify=("n_reads", "n_cands", "flags", "max_cand", "mismatch_penalty"), align=("n_reads", "n_ops", "flags", "band", "passes"),
                sets=("n_mems", "n_values", "n_not_located", "flags", "set_words"), positions=("n_mems", "n_values", "n_not_located", "flags", "set_words"))


def _chain(b, timing):
    """the seven calls on the batch's reads -> {stage.array: bytes, stage.counter: int}"""
    out = {}

    def keep(stage, result):
        for k, v in result.items():
            if isinstance(v, np.ndarray):
                out["%s.%s" % (stage, k)] = v.tobytes()
            elif v is None:
                out["%s.%s" % (stage, k)] = None
        for k in COUNTERS.get(stage, ()):
            out["%s.%s" % (stage, k)] = result[k]

    b.run(12, 1, P.RUN_TAGS | (P.RUN_TIMING if timing else 0))
    res = b.result()
    keep("run", res)
    out["run.n_extensions"], out["run.n_tag_overflow"] = res["n_extensions"], res["n_tag_overflow"]
    b.locate(SETS)
    keep("sets", {k: v for k, v in b.locations().items() if k != "sets"})
    keep("hits", b.read_hits(BOTH))
    b.locate(0)
    keep("positions", b.locations())
    keep("place", b.read_place(P.PLACE_LIST))
    keep("verify", b.read_verify(16, 4, P.VERIFY_LIST))
    aligned = b.read_align(8, P.ALIGN_CIGAR)
    keep("align", aligned)
    assert aligned["n_reads"] == 0 or (aligned["ms_align"] > 0) == bool(timing)
    return out


def _overhang_reads(seqs, rng):
    """reads of 30 .. 80 bytes over the starts and the ends of sequences, sequence 0 and the last one among them, with 1, 7, 8 and 9 bases
    that the text does not hold in front or behind, and on both sides of a core"""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    junk = lambda k: bytes(acgt[rng.integers(0, 4, size=k)])
    reads = []
    for q in sorted(set(range(0, len(seqs), 7)) | {len(seqs) - 1}):
        s = bytes(seqs[q])
        for a in (1, 7, 8, 9):
            n_core = int(rng.integers(30, 71))
            reads += [junk(a) + s[:n_core], s[-n_core:] + junk(a), s[-n_core:], s[:n_core], junk(a) + s[100:100 + n_core - 9] + junk(9 - a + 1)]
    assert all(30 <= len(r) <= 80 for r in reads)
    return reads


@pytest.mark.parametrize("timing", [False, True])
def test_a_refilled_batch_gives_what_a_fresh_one_gives(workdir, timing):
    ri, tags, seqs, n_seq = _collection(workdir, "hits_border_33", 33, 2000, 133)
    rng = np.random.default_rng(17)
    first = W.sample_reads(seqs, 300, 150, seed=61)
    mixed = []
    for n in [1, 2, 7, 8, 9, 11, 12, 13, 70] + rng.integers(1, 71, size=31).tolist():
        s = bytes(seqs[int(rng.integers(0, n_seq))])
        at = int(rng.integers(0, len(s) - n))
        mixed.append(s[at:at + n])
    uploads = [first, O.pack_reads(mixed), (np.zeros(0, np.uint8), np.zeros(1, np.uint64)), W.sample_reads(seqs, 300, 150, seed=62),
               O.pack_reads(_overhang_reads(seqs, rng)), first]
    assert [len(o) - 1 for _, o in uploads][:4] == [300, 40, 0, 300] and not np.array_equal(uploads[0][0], uploads[3][0])
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    b = P.Batch(idx, *uploads[0])
    results = []
    for k, (cat, offs) in enumerate(uploads):
        if k:
            b.upload(cat, offs)
        got = _chain(b, timing)
        fresh = P.Batch(idx, cat, offs)
        want = _chain(fresh, timing)
        fresh.free()
        assert got.keys() == want.keys()
        for key in want:
            assert got[key] == want[key], (k, key)
        assert got["align.n_reads"] == got["verify.n_reads"] == got["place.n_reads"] == got["hits.n_reads"] == len(offs) - 1
        if k == 1:  # the device arrays of the short upload, behind the long one's
            n = len(offs) - 1
            dv, da = b.device_verified(), b.device_aligned()
            for dev, stage, sizes in ((dv, "verify", (("reads", n * 64), ("cand_offsets", (n + 1) * 8), ("cands", got["verify.n_cands"] * 64))),
                                      (da, "align", (("reads", n * 64), ("op_offsets", (n + 1) * 8), ("ops", got["align.n_ops"] * 4)))):
                for name, nbytes in sizes:
                    assert nbytes > 0 and _device_read(dev[name].__cuda_array_interface__["data"][0], nbytes).tobytes() == got["%s.%s" % (stage, name)], (stage, name)
        results.append(got)
    assert results[5] == results[0]
    assert results[0]["verify.n_cands"] > 300 and results[1]["verify.n_cands"] > 0 and results[2]["verify.n_cands"] == 0 and results[4]["verify.n_cands"] > 0
    assert results[3]["verify.reads"] != results[0]["verify.reads"] and len(results[1]["align.reads"]) == 40 * 64 and results[2]["align.reads"] == b""
    b.free()
    idx.close()
