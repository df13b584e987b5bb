"""GPU tier of the read-hits kernels at their borders, through pgx_read_hits_arrays (the kernels of pgx_batch_read_hits on host arrays):
every field of every record, the best sets and the score rows equal tests/hits_emu.py, which states the definitions with position masks.
Shapes: every lane packing (1 .. 64 lanes a read), one word column and several, up to the cap of 4096 sequences, a last wave and a
last block that are partial, reads without MEMs, MEMs without sequences, nested and non-monotone ends, long reads, ties and runners-up
across word columns, input bits beyond n_seq, scores beyond 32 bits, and the calls the entry point refuses."""
import numpy as np
import pytest

import hits_emu as E
import pgx_ffi as P

pytestmark = pytest.mark.gpu

BOTH = P.HITS_BEST_SETS | P.HITS_SCORES
N_SEQS = [1, 2, 16, 17, 32, 33, 63, 64, 65, 128, 129, 4096]


def _check(case, n_seq):
    """all outputs == the emulator's, with both optional outputs and without them; returns the emulator's result"""
    mem_offsets, mems, sets = case
    exp = E.read_hits(mem_offsets, mems, sets, n_seq)
    got = P.read_hits_arrays(0, mem_offsets, mems, sets, n_seq, BOTH)
    bad = np.flatnonzero(got["hits"] != exp["hits"])
    assert len(bad) == 0, (n_seq, len(bad), int(bad[0]), got["hits"][bad[0]], exp["hits"][bad[0]])
    assert got["hits"].tobytes() == exp["hits"].tobytes()
    assert np.array_equal(got["scores"], exp["scores"]), n_seq
    assert np.array_equal(got["best_sets"], exp["best_sets"]), n_seq
    if n_seq % 64:  # bits at or beyond n_seq
        assert not (got["best_sets"][:, -1] >> np.uint64(n_seq % 64)).any()
    plain = P.read_hits_arrays(0, mem_offsets, mems, sets, n_seq, 0)
    assert plain["hits"].tobytes() == exp["hits"].tobytes() and plain["best_sets"] is None and plain["scores"] is None
    return exp


@pytest.mark.parametrize("n_seq", N_SEQS)
def test_random_reads_at_every_packing(n_seq):
    rng = np.random.default_rng(1000 + n_seq)
    for n_reads in (1, 3, 5, 257):  # the last wave and the last block are partial at every packing
        exp = _check(E.random_case(rng, n_reads, n_seq), n_seq)
    h = exp["hits"]
    assert (h["n_mems"] == 0).any() and (h["n_located"] < h["n_mems"]).any() and (h["best_score"] > 0).any()
    if n_seq > 1:
        assert (h["n_best"] > 1).any() and (h["next_score"] > 0).any()


@pytest.mark.parametrize("n_seq", [1, 16, 65, 4096])
def test_reads_without_mems_and_mems_without_sequences(n_seq):
    last = n_seq - 1
    reads = [[], [(3, 9, [])], [], [(0, 5, []), (2, 8, [last]), (4, 6, [])], [], []]
    exp = _check(E.build_case(reads, n_seq), n_seq)
    assert exp["hits"]["n_mems"].tolist() == [0, 1, 0, 3, 0, 0] and exp["hits"]["n_located"].tolist() == [0, 0, 0, 1, 0, 0]
    assert exp["hits"]["best_seq"].tolist() == [P.NO_SEQUENCE] * 3 + [last] + [P.NO_SEQUENCE] * 2
    assert exp["hits"]["covered"].tolist() == [0, 0, 0, 6, 0, 0]
    _check(E.build_case([[], [], []], n_seq), n_seq)  # no MEM at all: the MEM and set arrays are empty


@pytest.mark.parametrize("n_seq", [2, 33, 130])
def test_abutting_overlapping_nested_and_empty_intervals(n_seq):
    a, z = 0, n_seq - 1
    reads = [
        [(0, 10, [a]), (10, 20, [a]), (20, 21, [a, z])],                      # abutting
        [(0, 10, [a, z]), (5, 15, [a]), (14, 30, [z])],                       # overlapping
        [(0, 100, [a]), (10, 20, [a, z]), (30, 40, [z]), (50, 120, [a, z])],  # nested, then one that reaches further
        [(0, 50, [a]), (1, 40, [a]), (2, 30, [a]), (3, 60, [z]), (4, 20, [z])],  # ends descend while starts ascend
        [(5, 5, [a]), (7, 3, [a, z]), (9, 0, [z]), (10, 11, [z])],            # end <= start
        [(0, 10, [z]), (20, 30, [z]), (21, 25, [a])],                         # a gap that stays a gap
    ]
    exp = _check(E.build_case(reads, n_seq), n_seq)
    assert exp["scores"][:, a].tolist() == [21, 15, 120, 50, 0, 4] and exp["scores"][:, z].tolist() == [1, 26, 90, 57, 1, 20]
    assert exp["hits"]["covered"].tolist() == [21, 30, 120, 60, 1, 20]


@pytest.mark.parametrize("n_seq", [16, 130])
@pytest.mark.parametrize("n_mems", [70, 300])
def test_long_reads(n_seq, n_mems):
    rng = np.random.default_rng(n_mems + n_seq)
    starts = np.sort(rng.choice(4 * n_mems, n_mems, replace=False))
    long_read = [(int(s), int(s + rng.integers(0, 40)), [int(q) for q in rng.choice(n_seq, rng.integers(0, 4), replace=False)]) for s in starts]
    reads = [[(0, 4, [1])], long_read, [(1, 3, [0])]]
    exp = _check(E.build_case(reads, n_seq), n_seq)
    assert exp["hits"]["n_mems"].tolist() == [1, n_mems, 1] and exp["hits"]["best_score"][1] > 40


@pytest.mark.parametrize("n_seq", [65, 129, 4096])
def test_ties_and_runners_up_across_word_columns(n_seq):
    z = n_seq - 1
    everyone = list(range(n_seq))
    reads = [
        [(0, 10, [0, 5]), (20, 50, [z])],               # the best sequence only in the last word column
        [(0, 10, [0, z]), (3, 5, [1])],                 # a tie that spans the first and the last column
        [(0, 10, everyone), (30, 35, everyone)],        # all sequences tied
        [(0, 10, [z]), (1, 8, [3]), (20, 22, [z - 1])],  # the runner-up in another column than the best
        [(0, 10, [3]), (1, 8, [z]), (20, 22, [1])],     # ... and the other way round
        [(0, 9, [63, 64]), (10, 11, [0])],              # a tie across the border of the first two columns
    ]
    exp = _check(E.build_case(reads, n_seq), n_seq)
    h = exp["hits"]
    assert h["best_seq"].tolist() == [z, 0, 0, z, 3, 63] and h["n_best"].tolist() == [1, 2, n_seq, 1, 1, 2]
    assert h["best_score"].tolist() == [30, 10, 15, 10, 10, 9] and h["next_score"].tolist() == [10, 2, 0, 7, 7, 1]
    assert exp["best_sets"][1, 0] == 1 and exp["best_sets"][1, -1] == np.uint64(1 << (z & 63))


@pytest.mark.parametrize("n_seq", [1, 17, 63, 65, 129])
def test_input_bits_beyond_n_seq_are_ignored(n_seq):
    w = (n_seq + 63) // 64
    mem_offsets, mems, sets = E.build_case([[(0, 10, [0]), (20, 25, [])], [(5, 9, [])]], n_seq)
    beyond = np.uint64((1 << 64) - (1 << (n_seq % 64)))  # every bit of the last word at or beyond n_seq
    sets[:, w - 1] |= beyond
    exp = _check((mem_offsets, mems, sets), n_seq)
    assert exp["hits"]["n_located"].tolist() == [1, 0] and exp["hits"]["covered"].tolist() == [10, 0]
    assert exp["hits"]["best_score"].tolist() == [10, 0] and exp["hits"]["n_best"].tolist() == [1, 0]


@pytest.mark.parametrize("n_seq", [2, 130])
def test_score_beyond_32_bits(n_seq):
    z = n_seq - 1
    exp = _check(E.build_case([[(0, 1 << 33, [z]), (5, 9, [0])], [(1, (1 << 32) + 1, [0]), (2, 1 << 32, [z])]], n_seq), n_seq)
    assert exp["hits"]["best_score"].tolist() == [1 << 33, 1 << 32] and exp["hits"]["next_score"].tolist() == [4, (1 << 32) - 2]
    assert exp["scores"][0, z] == 0xFFFFFFFF and exp["scores"][0, 0] == 4  # saturated in the row, exact in the record
    assert exp["scores"][1, 0] == 0xFFFFFFFF and exp["scores"][1, z] == 0xFFFFFFFE


@pytest.mark.parametrize("n_seq", [16, 130])
def test_starts_that_do_not_ascend_are_refused(n_seq):
    ok = [(0, 5, [0]), (3, 9, [1])]
    for bad_read in ([(4, 9, [0]), (4, 12, [1])], [(4, 9, [0]), (6, 12, [1]), (5, 7, [0])]):  # equal, descending
        mem_offsets, mems, sets = E.build_case([ok, [], ok, bad_read, ok, bad_read], n_seq)
        n, w = len(mem_offsets) - 1, (n_seq + 63) // 64
        out = dict(hits=np.full(n, 0x5A, np.uint8).repeat(40).view(P.READ_HIT_DTYPE), best_sets=np.full((n, w), 0x5A5A, np.uint64),
                   scores=np.full((n, n_seq), 0x5A5A, np.uint32))
        before = {k: v.copy() for k, v in out.items()}
        with pytest.raises(P.PgxError) as e:
            P.read_hits_arrays(0, mem_offsets, mems, sets, n_seq, BOTH, out=out)
        assert e.value.code == P.ERR_ARG and "read 3 " in str(e.value)  # the first such read
        for k in out:
            assert out[k].tobytes() == before[k].tobytes(), k


def test_set_words_must_match_n_seq():
    mem_offsets, mems, sets = E.build_case([[(0, 5, [0])]], 64)
    for n_seq, words in ((64, 2), (65, 1), (128, 3), (4097, 65), (4160, 65), (0, 0), (0, 1), (1, 0)):
        wide = np.zeros((1, max(words, 1)), np.uint64)
        with pytest.raises(P.PgxError) as e:
            P.read_hits_arrays(0, mem_offsets, mems, wide, n_seq, 0, set_words=words, out=dict(hits=np.zeros(1, P.READ_HIT_DTYPE), best_sets=None, scores=None))
        assert e.value.code == P.ERR_ARG, (n_seq, words)
    with pytest.raises(P.PgxError) as e:
        P.read_hits_arrays(0, mem_offsets, mems, sets, 64, 4)  # an unknown flag
    assert e.value.code == P.ERR_ARG
    got = P.read_hits_arrays(0, mem_offsets, mems, sets, 64, 0)
    assert got["hits"]["best_score"][0] == 5


@pytest.mark.parametrize("n_seq", [33, 64, 65])
def test_a_batch_beyond_one_launch_is_refused(n_seq):
    # 64 lanes a read: 2^26 reads would be 2^32 threads, which one launch does not hold; refused before any array is read
    n = 1 << 26
    mem_offsets = np.zeros(n + 1, np.uint64)  # (never touched: no page of it is made)
    small = dict(hits=np.zeros(1, P.READ_HIT_DTYPE), best_sets=None, scores=None)
    with pytest.raises(P.PgxError) as e:
        P.read_hits_arrays(0, mem_offsets, np.zeros(0, P.MEM_DTYPE), np.zeros((0, (n_seq + 63) // 64), np.uint64), n_seq, 0, out=small)
    assert e.value.code == P.ERR_UNSUPPORTED and "2^32 threads" in str(e.value)
    assert not small["hits"].view(np.uint8).any()
