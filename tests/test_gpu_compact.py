"""GPU tier of the compact result form: the device encoder (pgx_batch_result_compact on real runs, pgx_compact_encode on synthetic results)
produces, byte for byte, the stream and tables the Python statement of the format (tests/compact_emu.py) derives from the same result --
the stream is canonical, so equality is the whole check -- and pgx_compact_expand turns it back into what pgx_batch_result delivers."""
import os

import numpy as np
import pytest

import compact_emu as E
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W

pytestmark = pytest.mark.gpu

BT = os.path.join(O.GOLDEN, "bidirectional_test")


def _check(b, tags):
    """result_compact() of the batch's last run == the emulator's encoding of its result(); compact_expand == result(); returns both"""
    res = b.result()
    c = b.result_compact()
    want = E.encode(res)
    assert c["flags"] == (P.COMPACT_TAGS if tags else 0) and ("pos_offsets" in res) == tags
    for k in ("block_offsets", "block_first_mem", "block_first_pos"):
        assert np.array_equal(c[k], want[k]), k
    assert c["bytes"].tobytes() == want["bytes"].tobytes()
    assert E.same_compact(c, want)
    assert c["n_extensions"] == res["n_extensions"] and c["n_tag_overflow"] == res["n_tag_overflow"] and c["block_reads"] == 64
    out = P.compact_expand(c)
    assert E.same_result(out, res) and out["n_extensions"] == res["n_extensions"]
    assert E.same_result(b.result(), res)  # (result() behind result_compact(): unchanged)
    return res, c


def _run_check(idx, cat, offs, min_len, tags=True, b=None, timing=False):
    flags = (P.RUN_TAGS if tags else 0) | (P.RUN_TIMING if timing else 0)
    if b is None:
        b = P.Batch(idx, cat, offs)
    else:
        b.upload(cat, offs)
    b.run(min_len, 1, flags)
    return (b,) + _check(b, tags)


@pytest.fixture(scope="module")
def xidx(x_index):
    idx = P.Index(x_index[0], x_index[1])
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def xreads(golden):
    seqs = W.load_sequences(os.path.join(golden, "x.newline_separated"))
    return W.sample_reads(seqs, 1500, 150, seed=4)


def test_xy_fixture_reads(built):
    idx = P.Index(os.path.join(BT, "xy.ri"), os.path.join(BT, "xy_bidirectional_compressed.tags"))
    reads = [l for l in open(os.path.join(BT, "reads.txt"), "rb").read().split(b"\n") if l]
    cat, offs = O.pack_reads(reads)
    for ml in (5, 3):
        b, res, c = _run_check(idx, cat, offs, ml)
        assert len(res["mems"]) > 0 and len(res["positions"]) > 0
        b.free()
    idx.close()


@pytest.mark.parametrize("tags", [True, False])
def test_x_1500_reads(xidx, xreads, tags):
    b, res, c = _run_check(xidx, xreads[0], xreads[1], 10, tags)
    assert len(res["mems"]) > 0 and c["n_blocks"] == 24
    if tags:
        full = 8 * (1501 + 6 * len(res["mems"]) + 1 + len(res["positions"]))
        assert c["n_bytes"] < full / 3  # (what the form is for)
    b.free()


def test_med_many_mems_per_read(workdir, golden):
    ri, tags = W.build_index_from_rlbwt(os.path.join(golden, "med_test.rl_bwt"), workdir, "compact_med")
    seqs = W.load_sequences(os.path.join(golden, "med_test.txt"))
    idx = P.Index(ri, tags)
    cat, offs = W.sample_reads(seqs, 300, 6, seed=3)
    b, res, c = _run_check(idx, cat, offs, 3)
    per_block = np.diff(c["block_first_mem"].astype(np.int64))
    assert per_block.max() > 64  # more MEMs in a block than one round of the MEM section holds
    b.free()
    idx.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_sizes_at_block_borders(xidx, xreads, n):
    cat, offs = xreads
    b, res, c = _run_check(xidx, cat[:int(offs[n])], offs[:n + 1], 10)
    assert c["n_blocks"] == (n + 63) // 64 and c["n_reads"] == n
    b.free()


def test_block_without_mems_then_mixed(xidx, xreads):
    """70 reads shorter than min_len, then 60 ordinary ones: block 0 holds no MEM, block 1 six empty reads and 58 ordinary ones"""
    cat, offs = xreads
    short = [bytes(cat[int(offs[i]):int(offs[i]) + 5]) for i in range(70)]
    normal = [bytes(cat[int(offs[i]):int(offs[i + 1])]) for i in range(100, 160)]
    c2, o2 = O.pack_reads(short + normal)
    b, res, c = _run_check(xidx, c2, o2, 10)
    assert res["mem_offsets"][70] == 0 and len(res["mems"]) > 0
    assert c["block_offsets"][1] == 64 and c["block_first_mem"][1] == 0 and not c["bytes"][:64].any()
    b.free()


def test_fasta_upload_with_empty_records(xidx, xreads):
    cat, offs = xreads
    text = b""
    for i in range(150):
        text += b">r%d\n" % i
        if i % 5 != 2:  # (every fifth record has no sequence: a read without MEMs)
            text += bytes(cat[int(offs[i]):int(offs[i + 1])]) + b"\n"
    b = xidx.batch_empty()
    assert b.upload_text(text, P.READS_FASTA) == 150
    b.run(10, 1, P.RUN_TAGS)
    res, c = _check(b, True)
    assert res["mem_offsets"][3] == res["mem_offsets"][2] and len(res["mems"]) > 0
    b.free()


def test_lifetime_and_non_mutation(x_index, xreads):
    cat, offs = xreads
    xidx = P.Index(x_index[0], x_index[1], mode=P.MODE_STRICT)  # (COMPAT cannot locate on an encoded index without N)
    b, res, c = _run_check(xidx, cat, offs, 10)
    # the device result is untouched: locate behind result_compact gives what it gives on a fresh batch of the same run
    b.locate(0)
    loc = b.locations()
    b2 = P.Batch(xidx, cat, offs)
    b2.run(10, 1, P.RUN_TAGS)
    b2.locate(0)
    loc2 = b2.locations()
    assert loc["values"].tobytes() == loc2["values"].tobytes() and np.array_equal(loc["loc_offsets"], loc2["loc_offsets"])
    b2.free()
    _check(b, True)  # (and result_compact behind locate)
    # a second run on the same batch, other parameters, without tags
    b.run(25, 1, 0)
    res25, c25 = _check(b, False)
    assert c25["n_bytes"] < c["n_bytes"] and not E.same_result(res25, res)
    # fewer reads into the same batch: the grown buffers leak no stale tail
    n = 200
    b, res_small, c_small = _run_check(xidx, cat[:int(offs[n])], offs[:n + 1], 10, True, b=b)
    assert c_small["n_blocks"] == 4 and c_small["n_bytes"] == int(c_small["block_offsets"][-1]) < c["n_bytes"]
    assert len(c_small["bytes"]) == c_small["n_bytes"] and E.same_compact(c_small, E.encode(res_small))
    # without a completed run: an upload invalidates the result
    b.upload(cat[:int(offs[n])], offs[:n + 1])
    with pytest.raises(P.PgxError) as e:
        b.result_compact()
    assert e.value.code == P.ERR_ARG
    b.free()
    xidx.close()


def test_timed_run_reports_encode_time(xidx, xreads):
    b = P.Batch(xidx, xreads[0], xreads[1])
    b.run(10, 1, P.RUN_TAGS)
    assert b.result_compact()["ms_encode"] == 0
    b.run(10, 1, P.RUN_TAGS | P.RUN_TIMING)
    assert 0 < b.result_compact()["ms_encode"] < 1000
    b.free()


def test_chunked_run(xidx, xreads, monkeypatch):
    monkeypatch.setenv("PGX_SLOT_BUDGET_MB", "1")  # 32768 slots against 141 worst-case MEMs a read: a few hundred reads a chunk
    b, res, c = _run_check(xidx, xreads[0], xreads[1], 10, timing=True)
    chunked_launches = b.timing().find_mems_launches
    monkeypatch.delenv("PGX_SLOT_BUDGET_MB")
    b2, res2, c2 = _run_check(xidx, xreads[0], xreads[1], 10, timing=True)
    assert chunked_launches > b2.timing().find_mems_launches >= 1  # (the first run was chunked)
    assert E.same_compact(c, c2)
    b.free()
    b2.free()


# ---- synthetic results through pgx_compact_encode -------------------------------------------------------------------------------
def _encode_check(res):
    want = E.encode(res)
    got = P.compact_encode(0, res)
    for k in ("block_offsets", "block_first_mem", "block_first_pos"):
        assert np.array_equal(got[k], want[k]), k
    assert got["bytes"].tobytes() == want["bytes"].tobytes() and E.same_compact(got, want)
    assert E.same_result(P.compact_expand(got), res)
    return want


@pytest.mark.parametrize("tags", [True, False])
def test_encode_varint_borders(built, tags):
    _encode_check(E.border_result(tags))
    _encode_check(E.random_result(np.random.default_rng(11), 333, tags, big=True))


def test_encode_one_mem_with_5000_positions(built):
    rng = np.random.default_rng(12)
    res = E.random_result(rng, 200, True)
    m = int(res["mem_offsets"][100])  # a MEM in the middle of block 1
    po = res["pos_offsets"].astype(np.int64)
    at = int(po[m + 1])
    extra = np.sort(rng.integers(0, 1 << 40, 5000, dtype=np.uint64))
    res["positions"] = np.concatenate([res["positions"][:at], extra, res["positions"][at:]])
    po[m + 1:] += 5000
    res["pos_offsets"] = po.astype(np.uint64)
    seg = res["positions"][int(po[m]):int(po[m + 1])]
    seg.sort()
    _encode_check(res)


def test_encode_64_reads_400_positions_each(built):
    rng = np.random.default_rng(13)
    res = E.random_result(rng, 64, True, max_mems=1, max_pos=0, p_empty=0)
    res["mem_offsets"] = np.arange(65, dtype=np.uint64)
    res["mems"] = np.resize(E.random_result(rng, 64, False, max_mems=4, p_empty=0)["mems"], 64)
    res["tag_run_counts"] = rng.integers(1, 40, 64).astype(np.uint64)
    res["pos_offsets"] = (np.arange(65, dtype=np.uint64) * np.uint64(400))
    res["positions"] = np.sort(rng.integers(0, 1 << 34, (64, 400), dtype=np.uint64), axis=1).reshape(-1)
    want = _encode_check(res)
    assert want["n_blocks"] == 1 and want["n_positions"] == 25600


def test_encode_unsorted_positions_and_empty(built):
    rng = np.random.default_rng(14)
    res = E.random_result(rng, 300, True, max_pos=9)
    rng.shuffle(res["positions"])
    _encode_check(res)
    _encode_check(E.random_result(rng, 300, True, max_pos=0))
    _encode_check(dict(mem_offsets=np.zeros(1, dtype=np.uint64), mems=np.zeros(0, dtype=P.MEM_DTYPE)))
    _encode_check(dict(mem_offsets=np.zeros(131, dtype=np.uint64), mems=np.zeros(0, dtype=P.MEM_DTYPE), tag_run_counts=np.zeros(0, dtype=np.uint64),
                       pos_offsets=np.zeros(1, dtype=np.uint64), positions=np.zeros(0, dtype=np.uint64)))
    bad = E.random_result(rng, 10, True)
    bad["pos_offsets"] = bad["pos_offsets"][::-1].copy()
    with pytest.raises(P.PgxError) as e:
        P.compact_encode(0, bad)
    assert e.value.code == P.ERR_ARG


def test_encode_cap_one_byte_short(built):
    res = E.random_result(np.random.default_rng(15), 500, True)
    need = E.encode(res)["n_bytes"]
    assert P.compact_encode(0, res, bytes_cap=need)["n_bytes"] == need
    with pytest.raises(P.PgxError) as e:
        P.compact_encode(0, res, bytes_cap=need - 1)
    assert e.value.code == P.ERR_NOMEM and e.value.n_bytes == need


def test_staged_fill_kernel_same_stream(xidx, xreads, monkeypatch):
    """PGX_COMPACT_STAGE=1: the fill kernel that stages a round's bytes in LDS and stores 8-byte words writes the same stream"""
    monkeypatch.setenv("PGX_COMPACT_STAGE", "1")
    b, res, c = _run_check(xidx, xreads[0], xreads[1], 10)
    b.free()
    for n in (1, 65):
        b, res, c = _run_check(xidx, xreads[0][:int(xreads[1][n])], xreads[1][:n + 1], 10, tags=(n == 1))
        b.free()
    rng = np.random.default_rng(16)
    for res in (E.border_result(True), E.border_result(False), E.random_result(rng, 333, True, big=True), E.random_result(rng, 200, True, max_mems=40, max_pos=1),
                E.random_result(rng, 300, True, max_pos=0), dict(mem_offsets=np.zeros(131, dtype=np.uint64), mems=np.zeros(0, dtype=P.MEM_DTYPE))):
        _encode_check(res)
    res = E.random_result(rng, 64, True, max_mems=1, max_pos=0, p_empty=0)
    res.update(mem_offsets=np.arange(65, dtype=np.uint64), mems=np.resize(E.random_result(rng, 64, False, max_mems=4, p_empty=0)["mems"], 64),
               tag_run_counts=rng.integers(1, 40, 64).astype(np.uint64), pos_offsets=np.arange(65, dtype=np.uint64) * np.uint64(400),
               positions=np.sort(rng.integers(0, 1 << 34, (64, 400), dtype=np.uint64), axis=1).reshape(-1))
    _encode_check(res)
