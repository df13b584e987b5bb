"""GPU tier of the device text output: pgx_format_result (synthetic results: every number border in every field, the structure borders of
the one-lane-per-item kernels and their 256-lane workgroups) and pgx_batch_format (real runs) write, byte for byte, the text the Python
statement of the grammar (tests/text_emu.py) derives from the same result.  The text has one spelling, so equality is the whole check."""
import os

import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import text_emu as T

pytestmark = pytest.mark.gpu

BT = os.path.join(O.GOLDEN, "bidirectional_test")
M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
# 0, 9, 10, every 10^k - 1 and 10^k, the switch of the 32-bit conversion path, the largest value
BORDERS = sorted(set([0, 9, 10] + [10 ** k - 1 for k in range(1, 20)] + [10 ** k for k in range(1, 20)] + [(1 << 32) - 1, 1 << 32, M64]))
SIZES = [0, -1, I64_MIN, I64_MAX] + [v for v in BORDERS if v <= I64_MAX] + [-v for v in BORDERS if 0 < v <= I64_MAX]
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _library(built):
    return built


def _result(mem_counts, pos_counts, values=None, rng=None):
    """a result dict: read i has mem_counts[i] MEMs, MEM m has pos_counts[m] positions; fields and positions from `values` in turn (or random)"""
    rng = rng or np.random.default_rng(1)
    m, npos = int(np.sum(mem_counts)), int(np.sum(pos_counts))
    assert len(pos_counts) == m
    mems = np.zeros(m, dtype=P.MEM_DTYPE)
    if values is None:
        for f in ("start", "end", "bwt_start"):
            mems[f] = rng.integers(0, 1 << 40, m, dtype=np.uint64) >> rng.integers(0, 40, m, dtype=np.uint64)
        mems["size"] = rng.integers(1, 100, m)
        pos = rng.integers(0, 1 << 34, npos, dtype=np.uint64) >> rng.integers(0, 34, npos, dtype=np.uint64)
    else:
        k = len(values)
        mems["start"] = np.array([values[i % k] for i in range(m)], dtype=np.uint64)
        mems["end"] = np.array([values[(i + 7) % k] for i in range(m)], dtype=np.uint64)
        mems["bwt_start"] = np.array([values[(i + 13) % k] for i in range(m)], dtype=np.uint64)
        mems["size"] = np.array([SIZES[i % len(SIZES)] for i in range(m)], dtype=np.int64)
        pos = np.array([values[(i + 3) % k] for i in range(npos)], dtype=np.uint64)
    return dict(mem_offsets=np.concatenate([[0], np.cumsum(mem_counts)]).astype(np.uint64), mems=mems,
                pos_offsets=np.concatenate([[0], np.cumsum(pos_counts)]).astype(np.uint64), positions=pos)


def _check(res, first_seq=0, locate=T.LOCATE_NONE, loc=None, max_length=0, stderr=True):
    """pgx_format_result == the emulator: text, stderr lines, read_offsets, exact sizes, guard bytes behind both buffers"""
    flags = (P.FORMAT_STDERR if stderr else 0) | {T.LOCATE_NONE: 0, T.LOCATE_POSITIONS: P.FORMAT_LOCATE_POSITIONS, T.LOCATE_SEQS: P.FORMAT_LOCATE_SEQS}[locate]
    text, err, offs = T.emit(res, first_seq, locate, loc, max_length or 1)
    got = P.format_result(0, res, first_seq=first_seq, flags=flags, max_length=max_length, locations=loc, guard=GUARD)
    assert got["n_bytes"] == len(text) and np.array_equal(got["read_offsets"], offs)
    assert got["text"] == text
    if stderr:
        assert got["n_err_bytes"] == len(err) and got["err_text"] == err
    else:
        assert got["n_err_bytes"] == 0 and got["err_text"] is None
    assert len(got["text_guard"]) == GUARD + 1 and np.all(got["text_guard"] == 0xA5), "pgx_format_result wrote behind text[n_bytes)"
    assert len(got["err_guard"]) >= GUARD + 1 and np.all(got["err_guard"] == 0xA5), "pgx_format_result wrote behind err_text[n_err_bytes)"
    return got


# ---- number borders ---------------------------------------------------------------------------------------------------------------
def test_borders_in_mem_fields_positions_and_sizes():
    """start, end, bwt_start and a position take every border value; size takes 0, -1, INT64_MIN, INT64_MAX and every border of both signs"""
    m = max(len(BORDERS), len(SIZES)) + 20
    res = _result([1] * m, [1 + (i % 3) for i in range(m)], values=BORDERS)
    for f in ("start", "end", "bwt_start"):
        assert set(int(v) for v in res["mems"][f]) == set(BORDERS)
    assert set(int(v) for v in res["positions"]) == set(BORDERS) and set(int(v) for v in res["mems"]["size"]) == set(SIZES)
    got = _check(res)
    assert b" SIZE: -9223372036854775808\n" in got["text"] and b" SIZE: 9223372036854775807\n" in got["text"] and b" SIZE: -1\n" in got["text"]
    assert b"MEM START: 18446744073709551615, " in got["text"] and b"4294967296, " in got["text"]


@pytest.mark.parametrize("border", [10 ** k for k in range(1, 20)] + [1 << 32, M64])
def test_seq_borders(border):
    """seq = first_seq + i + 1 passes border - 1, border (and border + 1): it gains a digit inside the batch at every power of ten"""
    n = 2 if border == M64 else 3
    res = _result([1, 0, 2][:n], [2, 0, 1][:sum([1, 0, 2][:n])])
    got = _check(res, first_seq=border - 2)
    assert got["text"].startswith(b"Seq: %d\n" % (border - 1)) and (b"\nSeq: %d\n" % border) in got["text"]


def test_position_count_borders():
    """the count line at every digit border a batch can hold (10^5 positions in one MEM: 800 KB; 10^19 would not fit any memory): the list of
    such a MEM spans hundreds of workgroups of the item kernel, all owned by one MEM between MEMs without positions"""
    counts = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 0, 99999, 0, 100000, 1]
    res = _result([len(counts)], counts)
    got = _check(res)
    for c in counts:
        assert b"Number of unique positions: %d\n" % c in got["text"]


# ---- structure borders ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_read_counts(n):
    rng = np.random.default_rng(n)
    mc = rng.integers(0, 4, n)
    res = _result(mc, rng.integers(0, 5, int(mc.sum())), rng=rng)
    got = _check(res, first_seq=95)  # (seq gains a digit at read 4 and at read 904 ...)
    assert (got["n_bytes"] == 0) == (n == 0)
    _check(res, stderr=False)


def test_mems_per_read_and_positions_per_mem():
    """reads with 0, 1, 64, 65 MEMs; MEMs with 0, 1, 63, 64, 65 and 5000 positions, in turn"""
    mc = [0, 1, 64, 65, 0, 1, 65, 64]
    pc = [[0, 1, 63, 64, 65, 5000][i % 6] if i % 11 else 5000 for i in range(sum(mc))]
    pc = [c if (c != 5000 or i % 66 == 0) else 2 for i, c in enumerate(pc)]  # (a few lists of 5000, not dozens)
    assert {0, 1, 63, 64, 65, 5000} <= set(pc)
    _check(_result(mc, pc))


def test_all_empty_batch_and_empty_reads_at_workgroup_borders():
    res = _result([0] * 600, [])
    got = _check(res, first_seq=0)
    assert got["text"].startswith(b"Seq: 1\n\nSeq: 2\n\n") and got["err_text"] == b"[find_all_mems] total mems=0\n" * 600
    # 600 reads, one lane each in workgroups of 256: empty reads at the first, the last and both sides of every workgroup border
    mc = np.full(600, 2)
    mc[[0, 255, 256, 257, 511, 512, 599]] = 0
    _check(_result(mc, np.arange(int(mc.sum())) % 4))
    # MEMs without positions on both sides of the MEM kernel's workgroup borders, reads of one MEM each
    pc = np.full(600, 3)
    pc[[0, 255, 256, 511, 512, 599]] = 0
    _check(_result([1] * 600, pc))


def test_one_read_owns_every_mem():
    mc = [0] * 300
    mc[137] = 700  # (the owner search of 700 MEMs ends at one read between empty ones)
    _check(_result(mc, np.arange(700) % 3))
    _check(_result([700], np.arange(700) % 3))


# ---- locate forms -----------------------------------------------------------------------------------------------------------------
def _locations(value_counts, values):
    k = len(values)
    n = int(np.sum(value_counts))
    return dict(loc_offsets=np.concatenate([[0], np.cumsum(value_counts)]).astype(np.uint64),
                values=np.array([values[(5 * i + 1) % k] for i in range(n)], dtype=np.uint64))


@pytest.mark.parametrize("max_length", [1, 1003, 1 << 33])
def test_locate_positions_form(max_length):
    """0 values ("not located"), 1 and 65 values; every border as a packed value (its quotient and remainder by max_length print)"""
    vc = [0, 1, 65, 0, 0, 65, 1, 1, 0, 65]
    res = _result([3, 0, 4, 3], [i % 3 for i in range(10)], values=BORDERS)
    loc = _locations(vc, BORDERS)
    assert set(int(v) for v in loc["values"]) == set(BORDERS)
    got = _check(res, locate=T.LOCATE_POSITIONS, loc=loc, max_length=max_length)
    assert b" (not located)\n\n" in got["text"] and (b"%d:%d, " % (M64 // max_length, M64 % max_length)) in got["text"]


def test_locate_seqs_form():
    vc = [0, 1, 65, 0, 0, 65, 1, 1, 0, 65]
    res = _result([3, 0, 4, 3], [i % 3 for i in range(10)], values=BORDERS)
    loc = _locations(vc, BORDERS)
    got = _check(res, locate=T.LOCATE_SEQS, loc=loc)
    assert b"Sequences: 65\n" in got["text"] and b"Sequences: 1\n" in got["text"] and b" (not located)\n\n" in got["text"]
    # every MEM not located; no MEM at all
    _check(res, locate=T.LOCATE_SEQS, loc=_locations([0] * 10, BORDERS))
    _check(_result([0, 0], []), locate=T.LOCATE_POSITIONS, loc=_locations([], BORDERS), max_length=7)


# ---- layout -----------------------------------------------------------------------------------------------------------------------
def test_capacity_one_byte_short():
    res = _result([2, 0, 3], [1, 2, 0, 4, 1])
    text, err, offs = T.emit(res, 41)
    for caps in ((len(text) - 1, len(err)), (len(text), len(err) - 1)):
        with pytest.raises(P.PgxError) as e:
            P.format_result(0, res, first_seq=41, flags=P.FORMAT_STDERR, text_cap=caps[0], err_cap=caps[1], guard=GUARD)
        assert e.value.code == P.ERR_NOMEM and e.value.n_bytes == len(text) and e.value.n_err_bytes == len(err)
        assert np.array_equal(e.value.read_offsets, offs)  # (read_offsets are written)
        assert np.all(e.value.text_buf == 0xA5) and np.all(e.value.err_buf == 0xA5)  # (text and err_text are not)
    got = P.format_result(0, res, first_seq=41, flags=P.FORMAT_STDERR, text_cap=len(text), err_cap=len(err), guard=GUARD)
    assert got["text"] == text and got["err_text"] == err
    # without PGX_FORMAT_STDERR no stderr buffer is needed at all
    got = P.format_result(0, res, first_seq=41, flags=0, text_cap=len(text), err_cap=0, guard=GUARD)
    assert got["text"] == text and got["n_err_bytes"] == 0 and np.all(got["err_guard"] == 0xA5)


# ---- pgx_batch_format on real runs ------------------------------------------------------------------------------------------------
def _same_result(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("mem_offsets", "mems", "tag_run_counts", "pos_offsets", "positions"))


def _batch_check(b, first_seq=0, locate=T.LOCATE_NONE, max_length=None, stderr=True):
    """format() of the batch's last run == the emulator on result() (and locations()); result() and result_compact() unchanged behind it"""
    res = b.result()
    comp = b.result_compact()
    loc = b.locations() if locate else None
    flags = (P.FORMAT_STDERR if stderr else 0) | {T.LOCATE_NONE: 0, T.LOCATE_POSITIONS: P.FORMAT_LOCATE_POSITIONS, T.LOCATE_SEQS: P.FORMAT_LOCATE_SEQS}[locate]
    got = b.format(first_seq=first_seq, flags=flags)
    text, err, offs = T.emit(res, first_seq, locate, loc, max_length or 1)
    assert got["n_reads"] == len(offs) - 1 and got["n_bytes"] == len(text) and np.array_equal(got["read_offsets"], offs)
    assert got["text"] == text
    assert got["err_text"] == (err if stderr else None) and got["n_err_bytes"] == (len(err) if stderr else 0)
    assert _same_result(b.result(), res)
    comp2 = b.result_compact()
    assert comp2["bytes"].tobytes() == comp["bytes"].tobytes() and np.array_equal(comp2["block_offsets"], comp["block_offsets"])
    if locate:
        loc2 = b.locations()
        assert loc2["values"].tobytes() == loc["values"].tobytes() and np.array_equal(loc2["loc_offsets"], loc["loc_offsets"])
    return res, got


@pytest.fixture(scope="module")
def xreads5000(golden):
    seqs = W.load_sequences(os.path.join(golden, "x.newline_separated"))
    return W.sample_reads(seqs, 5000, 150, seed=31)


def test_batch_format_xy_fixture(built):
    idx = P.Index(os.path.join(BT, "xy.ri"), os.path.join(BT, "xy_bidirectional_compressed.tags"))
    reads = [l for l in open(os.path.join(BT, "reads.txt"), "rb").read().split(b"\n") if l]
    cat, offs = O.pack_reads(reads)
    b = P.Batch(idx, cat, offs)
    for ml in (3, 5):
        b.run(ml, 1, P.RUN_TAGS)
        res, got = _batch_check(b)
        assert len(res["mems"]) > 0 and len(res["positions"]) > 0
        # the text is the committed golden of the CLI
        assert got["text"].decode() == open(os.path.join(O.GOLDEN, "expected_find_mems_xy_reads_%d_1.txt" % ml)).read()
        _batch_check(b, first_seq=998, stderr=False)
    b.free()
    idx.close()


def test_batch_format_x_5000_reads(x_index, xreads5000):
    cat, offs = xreads5000
    idx = P.Index(x_index[0], x_index[1], mode=P.MODE_STRICT)  # (COMPAT cannot locate on an encoded index without N)
    ml = idx.info().max_length
    b = P.Batch(idx, cat, offs)
    b.run(10, 1, P.RUN_TAGS | P.RUN_TIMING)
    res, got = _batch_check(b, first_seq=7777)  # (seq gains a digit inside the batch)
    assert len(res["mems"]) > 5000 and got["ms_format"] > 0
    b.locate(0)
    res, got = _batch_check(b, locate=T.LOCATE_POSITIONS, max_length=ml)
    assert b"Occurrences: " in got["text"] and b":" in got["text"]
    b.locate(P.LOCATE_CHAINS)
    assert b.format(flags=P.FORMAT_LOCATE_POSITIONS)["text"] == got["text"]
    b.locate(0, max_occ=3)  # (some MEMs over the cap: not located)
    res, got = _batch_check(b, locate=T.LOCATE_POSITIONS, max_length=ml)
    assert b" (not located)\n" in got["text"]
    b.locate(P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE)
    res, got = _batch_check(b, locate=T.LOCATE_SEQS)
    assert b"Sequences: " in got["text"]
    # fewer reads into the same batch: the grown buffers leak no stale tail; an untimed run reports no time
    n = 300
    b.upload(cat[:int(offs[n])], offs[:n + 1])
    b.run(10, 1, P.RUN_TAGS)
    res, got = _batch_check(b)
    assert got["n_reads"] == n and got["ms_format"] == 0
    b.free()
    idx.close()


def test_batch_format_errors(x_index, xreads5000):
    cat, offs = xreads5000
    n = 100
    idx = P.Index(x_index[0], x_index[1], mode=P.MODE_STRICT)
    b = P.Batch(idx, cat[:int(offs[n])], offs[:n + 1])

    def code(**kw):
        with pytest.raises(P.PgxError) as e:
            b.format(**kw)
        return e.value.code

    assert code() == P.ERR_ARG  # before any run
    b.run(10, 1, 0)
    assert code() == P.ERR_ARG  # a run without PGX_RUN_TAGS
    b.run(10, 1, P.RUN_TAGS)
    assert len(b.format()["text"]) > 0
    assert code(flags=P.FORMAT_LOCATE_POSITIONS) == P.ERR_ARG and code(flags=P.FORMAT_LOCATE_SEQS) == P.ERR_ARG  # no locate
    assert code(flags=P.FORMAT_LOCATE_POSITIONS | P.FORMAT_LOCATE_SEQS) == P.ERR_ARG
    assert code(flags=8) == P.ERR_ARG and code(reserved=1) == P.ERR_ARG
    b.locate(P.LOCATE_SEQ_SETS)
    assert code(flags=P.FORMAT_LOCATE_POSITIONS) == P.ERR_ARG and code(flags=P.FORMAT_LOCATE_SEQS) == P.ERR_ARG  # a set result never matches
    b.locate(0)
    assert code(flags=P.FORMAT_LOCATE_SEQS) == P.ERR_ARG and len(b.format(flags=P.FORMAT_LOCATE_POSITIONS)["text"]) > 0
    b.locate(P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE)
    assert code(flags=P.FORMAT_LOCATE_POSITIONS) == P.ERR_ARG and len(b.format(flags=P.FORMAT_LOCATE_SEQS)["text"]) > 0
    b.run(10, 1, P.RUN_TAGS)  # a new run: the locate result belongs to the run before
    assert code(flags=P.FORMAT_LOCATE_SEQS) == P.ERR_ARG
    b.upload(cat[:int(offs[n])], offs[:n + 1])
    assert code() == P.ERR_ARG  # an upload invalidates the run
    b.free()
    idx.close()
