"""CPU tier: pgx_compact_expand against the Python statement of the format (tests/compact_emu.py) -- round trips of emulator-encoded
streams, block ranges, and every malformed input the header names, each with the output arrays between guard values."""
import ctypes as C

import numpy as np
import pytest

import compact_emu as E
import pgx_ffi as P

GUARD = 0xA5A5A5A5A5A5A5A5
PAD = 16  # guard words on each side of every output array


def _roundtrip(res):
    c = E.encode(res)
    out = P.compact_expand(c)
    assert E.same_result(out, res)
    mo, mems, runs, po, pos = E.decode(c)  # (the emulator reads its own stream: the two Python halves agree)
    assert np.array_equal(mo, res["mem_offsets"]) and mems.tobytes() == res["mems"].tobytes()
    if po is not None:
        assert np.array_equal(po, res["pos_offsets"]) and np.array_equal(pos, res["positions"]) and np.array_equal(runs, res["tag_run_counts"])
    return c


@pytest.mark.parametrize("tags", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1000])
def test_random_results_round_trip(built, n, tags):
    rng = np.random.default_rng(1000 * n + tags)
    c = _roundtrip(E.random_result(rng, n, tags))
    assert c["n_blocks"] == (n + 63) // 64 and c["n_bytes"] % 8 == 0 and np.all(c["block_offsets"] % 8 == 0)
    _roundtrip(E.random_result(rng, n, tags, big=True))


def test_reads_and_blocks_without_mems(built):
    rng = np.random.default_rng(5)
    res = E.random_result(rng, 300, True)
    # reads 64 .. 191 (blocks 1 and 2) lose their MEMs; then a result without any MEM at all
    mo = res["mem_offsets"].copy()
    cut = int(mo[192] - mo[64])
    keep = np.r_[0:int(mo[64]), int(mo[192]):len(res["mems"])]
    pk = np.concatenate([np.arange(int(res["pos_offsets"][m]), int(res["pos_offsets"][m + 1])) for m in keep] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    cnt = np.diff(res["pos_offsets"])[keep]
    mo[64:192] = mo[64]
    mo[192:] -= np.uint64(cut)
    res2 = dict(mem_offsets=mo, mems=res["mems"][keep], tag_run_counts=res["tag_run_counts"][keep],
                pos_offsets=np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64), positions=res["positions"][pk])
    c = _roundtrip(res2)
    assert c["block_offsets"][2] - c["block_offsets"][1] == 64 and c["block_first_mem"][1] == c["block_first_mem"][3]
    for tags in (False, True):
        empty = dict(mem_offsets=np.zeros(131, dtype=np.uint64), mems=np.zeros(0, dtype=P.MEM_DTYPE))
        if tags:
            empty.update(tag_run_counts=np.zeros(0, dtype=np.uint64), pos_offsets=np.zeros(1, dtype=np.uint64), positions=np.zeros(0, dtype=np.uint64))
        assert _roundtrip(empty)["n_bytes"] == 64 + 64 + 8


def test_mems_without_positions(built):
    rng = np.random.default_rng(6)
    _roundtrip(E.random_result(rng, 200, True, max_pos=0))
    res = E.random_result(rng, 200, True, max_pos=1)  # a mix of MEMs with one position and with none
    assert 0 < len(res["positions"]) < len(res["mems"])
    _roundtrip(res)


def test_varint_borders_in_every_field(built):
    assert [len(E.varint(v)) for v in (0, 127, 128, (1 << 63) - 1, 1 << 63, E.M64)] == [1, 1, 2, 9, 10, 10]
    for tags in (False, True):
        res = E.border_result(tags)
        assert (res["mems"]["size"] < 0).any()
        _roundtrip(res)


def test_descending_positions(built):
    rng = np.random.default_rng(7)
    res = E.random_result(rng, 100, True, max_pos=9)
    po = res["pos_offsets"]
    for m in range(len(res["mems"])):
        seg = res["positions"][int(po[m]):int(po[m + 1])]
        seg[:] = np.sort(seg)[::-1]
    _roundtrip(res)


def test_block_ranges_one_at_a_time(built):
    rng = np.random.default_rng(8)
    res = E.random_result(rng, 1000, True)
    c = E.encode(res)
    whole = P.compact_expand(c)
    out = P.compact_expand_arrays(c)
    for k in reversed(range(c["n_blocks"])):
        P.compact_expand(c, k, 1, out=out)
    assert E.same_result(out, whole) and E.same_result(out, res)
    # a range that stops short of the end leaves the closing entries alone
    part = P.compact_expand(c, 0, c["n_blocks"] - 1)
    assert part["mem_offsets"][-1] == 0 and part["pos_offsets"][-1] == 0 and part["mem_offsets"][64] == res["mem_offsets"][64]
    with pytest.raises(P.PgxError) as e:
        P.compact_expand(c, c["n_blocks"], 1)
    assert e.value.code == P.ERR_ARG


def test_no_reads_no_blocks(built):
    for tags in (False, True):
        res = dict(mem_offsets=np.zeros(1, dtype=np.uint64), mems=np.zeros(0, dtype=P.MEM_DTYPE))
        if tags:
            res.update(tag_run_counts=np.zeros(0, dtype=np.uint64), pos_offsets=np.zeros(1, dtype=np.uint64), positions=np.zeros(0, dtype=np.uint64))
        c = _roundtrip(res)
        assert c["n_blocks"] == 0 and c["n_bytes"] == 0 and len(c["block_offsets"]) == 1
    assert P.compact_bound(0, 0, 0, 0) == 0
    assert P.compact_bound(65, 3, 7, 0) == 10 * (65 + 12) + 14 and P.compact_bound(65, 3, 7, P.COMPACT_TAGS) == 10 * (65 + 18 + 7) + 14


# ---- malformed input ----------------------------------------------------------------------------------------------------------
def _guarded(n, dtype=np.uint64, words=1):
    a = np.full((n * words + 2 * PAD), GUARD, dtype=np.uint64)
    return a


def _expand_guarded(c, first=0, nb=None):
    """pgx_compact_expand into arrays that lie between guard words; returns (status, message); asserts the guards are intact"""
    r, keep = P._compact_struct(c)
    n, m, npos = c["n_reads"], c["n_mems"], c["n_positions"]
    bufs = [_guarded(n + 1), _guarded(m, words=4), _guarded(m), _guarded(m + 1), _guarded(npos)]
    sizes = [n + 1, 4 * m, m, m + 1, npos]
    ptrs = [b.ctypes.data + 8 * PAD for b in bufs]
    st = P.lib().pgx_compact_expand(C.byref(r), first, c["n_blocks"] - first if nb is None else nb, *ptrs)
    for b, k in zip(bufs, sizes):
        assert np.all(b[:PAD] == GUARD) and np.all(b[PAD + k:] == GUARD), "pgx_compact_expand wrote outside its arrays"
    return st, P.lib().pgx_last_error().decode()


def _small():
    """two blocks; the first is small enough to cut at every byte"""
    rng = np.random.default_rng(9)
    res = E.random_result(rng, 70, True, max_mems=2, max_pos=3, p_empty=0.5)
    c = E.encode(res)
    assert _expand_guarded(c)[0] == P.OK
    return res, c


def _with_first_block(c, block):
    """the compact dict with the bytes of block 0 replaced (padded to 8 with zeros; the later blocks move)"""
    block = bytes(block) + bytes(-len(block) % 8)
    old = int(c["block_offsets"][1])
    d = dict(c)
    d["bytes"] = np.frombuffer(block + bytes(c["bytes"][old:]), dtype=np.uint8).copy()
    d["block_offsets"] = c["block_offsets"].copy()
    d["block_offsets"][1:] += np.uint64(len(block)) - np.uint64(old)
    d["n_bytes"] = len(d["bytes"])
    return d


def test_truncated_at_every_byte(built):
    res, c = _small()
    end = int(c["block_offsets"][1])
    body = bytes(c["bytes"][:end]).rstrip(b"\0")  # (without the padding: every cut below takes at least one byte of a number away)
    assert len(body) > 100
    for cut in range(len(body)):
        # the block ends at `cut`, as its table entry then says; the later blocks move up
        d = dict(c)
        d["block_offsets"] = c["block_offsets"].copy()
        d["bytes"] = np.concatenate([c["bytes"][:cut], c["bytes"][end:]])
        d["block_offsets"][1:] -= np.uint64(end - cut)
        d["n_bytes"] = len(d["bytes"])
        st, msg = _expand_guarded(d)
        assert st == P.ERR_FORMAT and "block 0" in msg, (cut, st, msg)
    # the stream itself cut short: n_bytes below the last block offset
    d = dict(c)
    d["n_bytes"] = c["n_bytes"] - 8
    d["bytes"] = c["bytes"][:-8]
    st, msg = _expand_guarded(d)
    assert st == P.ERR_FORMAT and "block 1" in msg
    assert _expand_guarded(d, 0, 1)[0] == P.OK  # (block 0 is whole)


def _one_mem_block(field_bytes):
    """a stream of one read with one MEM whose `start` is spelled by field_bytes"""
    res = dict(mem_offsets=np.array([0, 1], dtype=np.uint64), mems=np.zeros(1, dtype=P.MEM_DTYPE))
    c = E.encode(res)
    return _with_first_block(c, b"\x01" + field_bytes + b"\x00\x00\x00")


def test_bad_varints(built):
    ok = _one_mem_block(b"\xff" * 9 + b"\x01")
    out = P.compact_expand(ok)
    assert out["mems"]["start"][0] == E.M64 and out["mems"]["end"][0] == E.M64
    st, msg = _expand_guarded(_one_mem_block(b"\xff" * 10 + b"\x01"))  # 11 bytes
    assert st == P.ERR_FORMAT and "block 0" in msg and "longer than 10" in msg
    st, msg = _expand_guarded(_one_mem_block(b"\xff" * 9 + b"\x02"))
    assert st == P.ERR_FORMAT and "block 0" in msg and "tenth byte" in msg


def test_bad_padding_and_tables(built):
    res, c = _small()
    end = int(c["block_offsets"][1])
    body = bytes(c["bytes"][:end])
    assert body[-1] == 0, "the first block of this seed has padding"
    d = _with_first_block(c, body[:-1] + b"\x01")
    st, msg = _expand_guarded(d)
    assert st == P.ERR_FORMAT and "block 0" in msg and "padding" in msg
    st, msg = _expand_guarded(_with_first_block(c, body + bytes(8)))  # a whole word of padding
    assert st == P.ERR_FORMAT and "block 0" in msg and "padding" in msg
    for k, v in ((1, 0), (1, c["n_bytes"] + 8), (2, c["n_bytes"] + 8), (1, c["block_offsets"][2] + np.uint64(8))):
        d = dict(c)
        d["block_offsets"] = c["block_offsets"].copy()
        d["block_offsets"][k] = v
        st, msg = _expand_guarded(d)
        assert st == P.ERR_FORMAT and "block" in msg, (k, v)
    # MEM counts against block_first_mem[k + 1]: one too few (the reads' counts overrun it), one too many (they fall short)
    for delta in (-1, 1):
        d = dict(c)
        d["block_first_mem"] = c["block_first_mem"].copy()
        d["block_first_mem"][1:2] += np.uint64(delta & E.M64)
        st, msg = _expand_guarded(d)
        assert st == P.ERR_FORMAT and "block 0" in msg, delta
        d = dict(c)
        d["block_first_pos"] = c["block_first_pos"].copy()
        d["block_first_pos"][1:2] += np.uint64(delta & E.M64)
        st, msg = _expand_guarded(d)
        assert st == P.ERR_FORMAT and "block 0" in msg, delta
    # a read count that alone exceeds everything
    d = _with_first_block(c, E.varint(E.M64) + body)
    st, msg = _expand_guarded(d)
    assert st == P.ERR_FORMAT and "block 0" in msg and "overrun" in msg
    # tables beyond the counters
    d = dict(c)
    d["block_first_mem"] = c["block_first_mem"].copy()
    d["block_first_mem"][2] = c["n_mems"] + 1
    assert _expand_guarded(d)[0] == P.ERR_FORMAT
    d = dict(c)
    d["n_blocks"] = 1
    assert _expand_guarded(d, 0, 1)[0] == P.ERR_FORMAT


def _no_gpu():
    try:
        return P.device_count() == 0
    except P.PgxError as e:
        return e.code == P.ERR_NO_DEVICE


def test_abi_and_no_device(built):
    L = P.lib()
    assert L.pgx_abi_version() == 7
    if not _no_gpu():
        return  # (with a GPU the two entry points are what tests/test_gpu_compact.py runs)
    r = P.CompactResult()
    assert L.pgx_batch_result_compact(None, C.byref(r)) == P.ERR_NO_DEVICE and b"no CPU fallback" in L.pgx_last_error()
    with pytest.raises(P.PgxError) as e:
        P.compact_encode(0, E.random_result(np.random.default_rng(1), 10, True))
    assert e.value.code == P.ERR_NO_DEVICE
