"""Shared pieces of the tests that drive pgx_batch_run through its kernel tables and knobs (test_gpu_variants.py, test_gpu_knobs.py,
test_gpu_boundaries.py): the indexes and read sets (built once per session), the oracle's answers (computed once per read set and
parameters: they do not depend on the device configuration under test), the environment of one configuration, and the comparison."""
import contextlib
import os

import numpy as np

import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W

_CASES = {}  # name -> dict(ri_path, tags_path, tags_fmt, seqs, cat, offs, ...)
_REF = {}    # (read set, oracle mode, min_len, min_occ) -> the oracle's answer


def same(res, ref):
    """bit for bit: MEM offsets, MEM bytes, extension count, tag run counts, position offsets, positions"""
    assert np.array_equal(res["mem_offsets"], ref["mem_offsets"])
    assert res["mems"].tobytes() == ref["mems"].tobytes()
    assert res["n_extensions"] == ref["n_extensions"]
    assert np.array_equal(res["tag_run_counts"], ref["tag_run_counts"])
    assert np.array_equal(res["pos_offsets"], ref["pos_offsets"])
    assert np.array_equal(res["positions"], ref["positions"])


@contextlib.contextmanager
def env(settings):
    """the environment variables of one configuration, set for the block and put back behind it (None: unset)"""
    old = {k: os.environ.get(k) for k in settings}
    try:
        for k, v in settings.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def join_reads(cat, offs, extra):
    ecat, eoffs = O.pack_reads(extra)
    return np.concatenate([cat, ecat]), np.concatenate([offs, eoffs[1:] + offs[-1]])


def n_run_read(seqs, read_len=150):
    """a read cut from inside the first N run of the text (N only), and one that straddles its start"""
    for s in seqs:
        pos = np.flatnonzero(s == ord("N"))
        if len(pos) >= read_len:
            a = int(pos[0])
            return [bytes(s[a:a + read_len]), bytes(s[max(0, a - read_len // 2):a + read_len // 2])]
    raise ValueError("no N run of %d symbols" % read_len)


def edge_reads(seqs, rng, n_ragged=300):
    """what the pairs tests use: reads that end or start a sequence, N / lower case / NUL bytes, empty and one-symbol reads, reads cut
    from an N run (work for the heavy-read kernel and the second-stream launch), ragged lengths"""
    extra = []
    for s in seqs[:4]:
        extra.append(bytes(s[-150:]))
        extra.append(bytes(s[:150]))
    extra += n_run_read(seqs) + [b"", b"A", b"N", b"ACGT" * 30, b"N" * 30, b"acgtacgtacgtacgtacgtacgt", b"\0" * 7]
    odd = np.frombuffer(b"Nacgt\x00$", dtype=np.uint8)
    for _ in range(n_ragged):
        s = seqs[int(rng.integers(0, len(seqs)))]
        ln = int(rng.integers(1, 340))
        a = int(rng.integers(0, len(s) - ln))
        r = bytearray(bytes(s[a:a + ln]))
        for _ in range(int(rng.integers(0, 3))):
            r[int(rng.integers(0, ln))] = int(rng.choice(odd))
        extra.append(bytes(r))
    return extra


def mid_case(workdir):
    """the mid-size synthetic pangenome: n = 1.3 M, 8 haplotypes in both strands, N runs -- large enough for the PAIRS and the LCE image
    (n >= 4096), for a seed table of depth 12 with its second table of depth 10, far too large for LDS"""
    if "mid" not in _CASES:
        text = os.path.join(workdir, "variants_mid.txt")
        W.synth_pangenome_text(text, base_len=80_000, n_hap=8, seed=91, n_runs=3, n_run_len=(200, 2500))
        ri_path, tags_path = W.build_index_from_text(text, workdir, "variants_mid")[:2]
        seqs = W.load_sequences(text)
        cat, offs = W.sample_reads(seqs, 20_000, 150, seed=17, n_frac=0.02)
        cat, offs = join_reads(cat, offs, edge_reads(seqs, np.random.default_rng(6)))
        _CASES["mid"] = dict(name="mid", ri_path=ri_path, tags_path=tags_path, tags_fmt=O.TAGS_COMPACT, seqs=seqs, cat=cat, offs=offs)
    return _CASES["mid"]


def mid_small_case(workdir):
    """the same index with a tenth of the reads (the run-length kernel, the child process)"""
    if "mid_small" not in _CASES:
        m = mid_case(workdir)
        cat, offs = W.sample_reads(m["seqs"], 2_000, 150, seed=18, n_frac=0.02)
        cat, offs = join_reads(cat, offs, edge_reads(m["seqs"], np.random.default_rng(7), n_ragged=60))
        _CASES["mid_small"] = dict(m, name="mid_small", cat=cat, offs=offs)
    return _CASES["mid_small"]


def x_case(x_index, golden):
    """the tiny x index (its dense image is staged in LDS)"""
    if "x" not in _CASES:
        seqs = W.load_sequences(os.path.join(golden, "x.newline_separated"))
        cat, offs = W.sample_reads(seqs, 6_000, 150, seed=19)
        extra = [bytes(seqs[0][-150:]), bytes(seqs[0][:150]), b"", b"A", b"N" * 20, b"acgtacgtacgtacgt", b"\0" * 5, b"ACGT" * 30]
        rng = np.random.default_rng(8)
        for _ in range(200):
            s = seqs[int(rng.integers(0, len(seqs)))]
            ln = int(rng.integers(1, min(340, len(s))))
            a = int(rng.integers(0, len(s) - ln))
            extra.append(bytes(s[a:a + ln]))
        cat, offs = join_reads(cat, offs, extra)
        _CASES["x"] = dict(name="x", ri_path=x_index[0], tags_path=x_index[1], tags_fmt=O.TAGS_COMPACT, seqs=seqs, cat=cat, offs=offs)
    return _CASES["x"]


def xy_case(xy_paths, golden):
    """the legacy two-contig index without N: in COMPAT its quirk tables need the run-length image (excl_mask != 0)"""
    if "xy" not in _CASES:
        seqs = W.load_sequences(os.path.join(golden, "bidirectional_test", "contigs_xy"))
        rng = np.random.default_rng(9)
        extra = [b"", b"A", b"N" * 5, b"acgt"] + [bytes(s) for s in seqs] + [bytes(s[:len(s) // 2]) for s in seqs]
        for _ in range(1500):
            s = seqs[int(rng.integers(0, len(seqs)))]
            ln = int(rng.integers(1, len(s)))
            a = int(rng.integers(0, len(s) - ln + 1))
            r = bytearray(bytes(s[a:a + ln]))
            if rng.random() < 0.3:
                r[int(rng.integers(0, ln))] = int(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8)))
            extra.append(bytes(r))
        cat, offs = O.pack_reads(extra)
        _CASES["xy"] = dict(name="xy", ri_path=xy_paths[0], tags_path=xy_paths[1], tags_fmt=O.TAGS_BYTECODE, seqs=seqs, cat=cat, offs=offs)
    return _CASES["xy"]


def oracle(case, min_len, min_occ, omode=O.MODE_COMPAT, key=None, cat=None, offs=None):
    """the oracle's answer for the case's reads (or for cat / offs, named by key), computed once"""
    k = (key or case["name"], omode, min_len, min_occ)
    if k not in _REF:
        if "_ri" not in case:
            case["_ri"], case["_tags"] = O.RIndex(case["ri_path"]), O.Tags(case["tags_path"], case["tags_fmt"])
        _REF[k] = O.find_mems_batch(case["_ri"], case["_tags"], case["cat"] if cat is None else cat, case["offs"] if offs is None else offs,
                                    min_len, min_occ, mode=omode, threads=O.lib().orc_max_threads())
    return _REF[k]


def run(idx, cat, offs, min_len, min_occ):
    """one fresh batch, one run with tags -> (result, timing)"""
    b = idx.batch(cat, offs)
    try:
        b.run(min_len, min_occ, flags=P.RUN_TAGS | P.RUN_TIMING)
        return b.result(), b.timing()
    finally:
        b.free()


def fm_bits(in_lds, kind, narrow, seeded):
    return P.KERNELS_FM | (P.KERNELS_FM_SEEDED if seeded else 0) | (P.KERNELS_FM_NARROW if narrow else 0) | (kind << P.KERNELS_FM_KIND_SHIFT) | (P.KERNELS_FM_LDS if in_lds else 0)


def pairs_bits(wide, packed, coop, s64, lce):
    return (P.KERNELS_PAIRS | (P.KERNELS_PAIRS_S64 if s64 else 0) | (P.KERNELS_PAIRS_COOP if coop else 0) | (P.KERNELS_PAIRS_PACKED if packed else 0) |
            (P.KERNELS_PAIRS_WIDE if wide else 0) | (P.KERNELS_PAIRS_LCE if lce else 0))
