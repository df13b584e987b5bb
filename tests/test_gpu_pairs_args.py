"""pgx_find_mems_pairs_kernel takes one argument structure (PgxPairsArgs) and fetches what its rare paths need from the kernel argument segment
where they run.  Each of those paths is driven here on purpose, over both strides of the PAIRS image, and compared with the oracle bit for bit
(MEM offsets and bytes, extension count, tag run counts and positions): the fifth and later MEMs of a read (arena, arena overflow and its repeat in
the worst-case layout, worst-case layout from the start), several chunks (first_read and slot_base not 0), the heavy hand-over from the pairs
kernel itself, the launch without a second stream (skip == NULL, reads with N handed on inside the kernel), the packed and the byte-window
instance next to the LCE one, the speculative re-runs of a batch, min_len 0 and reads shorter than min_len.

The inputs are chosen on the CPU first (`inputs`): the oracle alone must produce a read with six MEMs or more, a pure A C G T read beyond the
heavy threshold used here, and a slot demand of more than one chunk -- a case that never reaches its path proves nothing."""
import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import variant_cases as V

pytestmark = pytest.mark.gpu

MIN_LEN, MIN_OCC = 10, 1   # behind the second seed table (depth 10) of the mid index; the LCE instance runs at min_occ <= 1
HEAVY_EXT = 300            # PGX_FM_HEAVY_EXT of the hand-over case
BUDGET_MB = 1              # PGX_SLOT_BUDGET_MB of the chunked case: 32768 slots a chunk
N_MUTATED, N_PLAIN, N_WITH_N = 128, 3400, 300  # (the mutated reads first: two in every sub-arena, which is one of 64 by read number)


def _pure(r):
    return all(c in b"ACGT" for c in r)


def make_reads(seqs):
    """at most 4096 reads of at most 150: (pure A C G T reads, reads with other bytes).  Mutated reads (six to nine substitutions: seven MEMs or so at
    min_len 10), plain ones, reads that end a sequence (chains of extensions: heavy), an empty read and reads shorter than min_len"""
    rng = np.random.default_rng(2024)
    pure, odd = [], []
    while len(pure) < N_MUTATED + N_PLAIN:
        s = seqs[int(rng.integers(0, len(seqs)))]
        a = int(rng.integers(0, len(s) - 150))
        r = bytearray(bytes(s[a:a + 150]))
        if not _pure(r):
            continue
        if len(pure) < N_MUTATED:
            for q in rng.choice(150, int(rng.integers(6, 10)), replace=False):
                r[int(q)] = b"ACGT"[(b"ACGT".index(r[int(q)]) + int(rng.integers(1, 4))) & 3]
        pure.append(bytes(r))
    for s in seqs[:8]:
        if _pure(bytes(s[-150:])):
            pure.append(bytes(s[-150:]))
    pure += [b"", b"A", b"ACGTACG", b"ACGTACGTA", b"ACGTACGTAC"]  # empty, shorter than min_len, exactly min_len
    while len(odd) < N_WITH_N:
        s = seqs[int(rng.integers(0, len(seqs)))]
        a = int(rng.integers(0, len(s) - 150))
        r = bytearray(bytes(s[a:a + 150]))
        for _ in range(int(rng.integers(1, 4))):
            r[int(rng.integers(0, 150))] = int(rng.choice(np.frombuffer(b"Nn\x00$", dtype=np.uint8)))
        odd.append(bytes(r))
    odd += V.n_run_read(seqs)
    assert len(pure) + len(odd) <= 4096
    return pure, odd


def check_inputs(case, pure, odd):
    """the oracle's answers (all reads; the pure ones alone) and the proof that the inputs reach the paths; host only"""
    cat, offs = O.pack_reads(pure + odd)
    pcat, poffs = O.pack_reads(pure)
    ref = V.oracle(case, MIN_LEN, MIN_OCC, key="pairs_args_all", cat=cat, offs=offs)
    pref = V.oracle(case, MIN_LEN, MIN_OCC, key="pairs_args_pure", cat=pcat, offs=poffs)
    per_read = np.diff(ref["mem_offsets"].astype(np.int64))
    assert per_read.max() >= 6 and int((per_read >= 6).sum()) >= 64, "no reads with six MEMs"
    # what the reads ask of the arena of fifth and later MEMs (pgx_slots_device.h): a read reserves, with its fifth MEM, as many slots as it has start positions
    # left, in the sub-arena of its number mod 64.  The default arena (eight slots a read and 4096) must hold that, the smallest one (151 slots a sub-arena) must not
    lens = np.diff(offs.astype(np.int64))
    ask = np.zeros(64, dtype=np.int64)
    for r in np.flatnonzero(per_read >= 5):
        x = int(ref["mems"]["start"][int(ref["mem_offsets"][r]) + 4])
        ask[r & 63] += max(int(lens[r]) - MIN_LEN - x + 1, 1)
    n_reads = len(offs) - 1
    assert ask.max() <= (8 * n_reads + 4096) // 64 and ask.max() > 151, (ask.max(), (8 * n_reads + 4096) // 64)
    # a pure read that spends more than HEAVY_EXT extensions: the ones that end a sequence, asked one by one
    tail = [r for r in pure if len(r) == 150][-8:]
    spent = [V.oracle(case, MIN_LEN, MIN_OCC, key="pairs_args_tail%d" % i, cat=O.pack_reads([r])[0], offs=O.pack_reads([r])[1])["n_extensions"] for i, r in enumerate(tail)]
    heavy = max(spent + [0]) > HEAVY_EXT
    if not heavy:  # (otherwise any pure read)
        for i, r in enumerate(pure[:64]):
            c, o = O.pack_reads([r])
            if V.oracle(case, MIN_LEN, MIN_OCC, key="pairs_args_head%d" % i, cat=c, offs=o)["n_extensions"] > HEAVY_EXT:
                heavy = True
                break
    assert heavy, ("no pure read beyond %d extensions" % HEAVY_EXT, spent)
    demand = int(np.where(lens < MIN_LEN, 0, np.minimum(lens, lens - MIN_LEN + 1)).sum())
    assert demand > 2 * (BUDGET_MB << 20) // 32, demand  # worst-case slots of the batch against the slots of one chunk (a pgx_mem is 32 bytes)
    return dict(cat=cat, offs=offs, ref=ref, pcat=pcat, poffs=poffs, pref=pref)


@pytest.fixture(scope="module")
def inputs(workdir):
    case = V.mid_case(workdir)
    pure, odd = make_reads(case["seqs"])
    return case, check_inputs(case, pure, odd)


def _runs(idx, cat, offs, min_len, times=1):
    b = idx.batch(cat, offs)
    try:
        out = []
        for _ in range(times):
            b.run(min_len, MIN_OCC, flags=P.RUN_TAGS | P.RUN_TIMING)
            out.append((b.result(), b.timing()))
        return out
    finally:
        b.free()


# case -> (environment of the run, reads: all / pure, pairs_reads expected: 4 LCE, 2 packed, 1 byte windows)
CASES = {
    "default-arena-side-stream": ({}, "all", 4),
    "arena-overflow-then-worst-case": ({"PGX_SLOT_ARENA_CAP": "1"}, "all", 4),
    "worst-case-layout": ({"PGX_SLOT_ARENA": "0"}, "all", 4),
    "several-chunks": ({"PGX_SLOT_BUDGET_MB": str(BUDGET_MB)}, "all", 1),
    "heavy-hand-over": ({"PGX_FM_HEAVY_EXT": str(HEAVY_EXT)}, "pure", 4),
    "no-side-stream": ({"PGX_FM_NO_SIDE": "1"}, "all", 1),
    "packed-without-lce": ({"PGX_FM_LCE": "0"}, "all", 2),
    "byte-windows": ({"PGX_FM_PACKED": "0"}, "all", 1),
}


@pytest.fixture(scope="module", params=["64", "96"])
def opened(request, inputs):
    case, _ = inputs
    with V.env({"PGX_PAIRS_STRIDE": request.param}):
        idx = P.Index(case["ri_path"], case["tags_path"], mode=P.MODE_COMPAT | P.MODE_IMAGE_PAIRS)
    assert idx.info().pairs_stride == int(request.param)
    yield idx, request.param == "64"
    idx.close()


@pytest.mark.parametrize("name", list(CASES))
def test_rare_path_equals_the_oracle(inputs, opened, name):
    _, data = inputs
    idx, s64 = opened
    env, which, variant = CASES[name]
    cat, offs, ref = (data["cat"], data["offs"], data["ref"]) if which == "all" else (data["pcat"], data["poffs"], data["pref"])
    with V.env(env):
        runs = _runs(idx, cat, offs, MIN_LEN, times=3)  # (the second and third run of a batch are sized speculatively)
    for res, t in runs:
        V.same(res, ref)
        assert t.pairs_reads == variant, (name, t.pairs_reads)
        assert t.kernels & P.KERNELS_PAIRS and bool(t.kernels & P.KERNELS_PAIRS_S64) == s64, hex(t.kernels)
        assert bool(t.kernels & P.KERNELS_PAIRS_LCE) == (variant == 4) and bool(t.kernels & P.KERNELS_PAIRS_PACKED) == (variant != 1), hex(t.kernels)
    t0 = runs[0][1]
    if name == "default-arena-side-stream":
        assert t0.kernels & P.KERNELS_SIDE and t0.find_mems_launches == 1, (hex(t0.kernels), t0.find_mems_launches)
    if name == "arena-overflow-then-worst-case":
        assert t0.find_mems_launches == 2, t0.find_mems_launches  # the chunk once more, in the worst-case layout
    if name == "worst-case-layout":
        assert t0.find_mems_launches == 1, t0.find_mems_launches
    if name == "several-chunks":
        assert t0.find_mems_launches > 2, t0.find_mems_launches
    if name == "heavy-hand-over":
        assert t0.heavy_reads > 0, t0.heavy_reads  # (every read of this batch is pure A C G T: none is served by another kernel first)
    if name == "no-side-stream":
        assert not (t0.kernels & P.KERNELS_SIDE), hex(t0.kernels)


def test_min_len_0_and_reads_shorter_than_min_len(inputs, opened):
    """min_len 0 (no stage has room for a seed: the one-step kernel serves the batch) and, at min_len 10, the empty read and the reads of 1, 7 and 9 symbols
    that are part of every batch above: no MEM, a count of 0 written for each"""
    case, data = inputs
    idx, _ = opened
    ref0 = V.oracle(case, 0, MIN_OCC, key="pairs_args_pure", cat=data["pcat"], offs=data["poffs"])
    (res, t), = _runs(idx, data["pcat"], data["poffs"], 0)
    V.same(res, ref0)
    lens = np.diff(data["poffs"].astype(np.int64))
    short = np.flatnonzero(lens < MIN_LEN)
    assert len(short) >= 4
    (res, t), = _runs(idx, data["pcat"], data["poffs"], MIN_LEN)
    V.same(res, data["pref"])
    assert t.pairs_reads == 4
    assert not np.diff(res["mem_offsets"].astype(np.int64))[short].any()
