"""GPU tier of PGX_LOCATE_SEQ_SETS and of the unique sequence ids served from the sets: MEM m's set has bit s iff s is among
pgx_locate_batch(first = bwt_start, last = bwt_start + size - 1, PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE) -- the expected sets are built
here from that call, never from pgx_batch_locate -- on the resident suffix array and on the sample chains, across word borders, with a
MEM wider than a block of the set kernel, in passes, for MEMs that are not located, at the cap of 4096 sequences and beyond it."""
import ctypes
import os

import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
from test_gpu_mem_locate import _cases, _ranges, _run_batch, synth  # noqa: F401  (synth: the module's fixture, _cases needs it)

pytestmark = pytest.mark.gpu

SETS, UNIQ_IDS = P.LOCATE_SEQ_SETS, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE
ML_SPAN = 4096  # PGX_ML_SPAN (pgx_device.h): values per block of the gather and set kernels


def _expected(idx, mems, max_occ=0):
    """(sets uint64[n_mems, W], loc_offsets and values of the sorted unique ids, not-located count, W) from pgx_locate_batch"""
    info = idx.info()
    w = (int(info.n_sequences) + 63) // 64
    first, last, n_not = _ranges(mems, info.bwt_size, max_occ)
    off, vals = idx.locate_batch(first, last, UNIQ_IDS)
    exp = np.zeros((len(mems), w), np.uint64)
    m_of = np.repeat(np.arange(len(mems)), np.diff(off.astype(np.int64)))
    assert len(vals) == 0 or int(vals.max()) < info.n_sequences
    np.bitwise_or.at(exp, (m_of, (vals >> np.uint64(6)).astype(np.int64)), np.uint64(1) << (vals & np.uint64(63)))
    return exp, off, vals, n_not, w


def _locate(b, flags, max_occ=0):
    b.locate(flags, max_occ)
    return b.locations()


def _check_sets(idx, b, mems, max_occ=0, chains_too=True, want_resident=None):
    """the set form == the expected sets with every field of the contract; the chain path gives the same bytes.  Returns the result."""
    exp, _, _, n_not, w = _expected(idx, mems, max_occ)
    n_seq = int(idx.info().n_sequences)
    got = _locate(b, SETS, max_occ)
    assert got["set_words"] == w and got["flags"] == SETS and got["n_mems"] == len(mems) and got["n_values"] == len(mems) * w
    assert got["n_not_located"] == n_not
    assert np.array_equal(got["loc_offsets"], np.arange(len(mems) + 1, dtype=np.uint64) * np.uint64(w))
    assert got["sets"].shape == exp.shape
    bad = np.flatnonzero((got["sets"] != exp).any(axis=1))
    assert len(bad) == 0, (len(bad), int(bad[0]), got["sets"][bad[0]], exp[bad[0]])
    if n_seq % 64:  # bits at or beyond n_seq
        assert not (got["sets"][:, -1] >> np.uint64(n_seq % 64)).any()
    if want_resident is not None:
        assert got["resident"] == want_resident
    if chains_too:
        ch = _locate(b, SETS | P.LOCATE_CHAINS, max_occ)
        assert not ch["resident"] and ch["flags"] == SETS and ch["set_words"] == w and ch["n_not_located"] == n_not
        assert ch["values"].tobytes() == got["values"].tobytes() and ch["loc_offsets"].tobytes() == got["loc_offsets"].tobytes()
    return got


def _collection(workdir, name, n_hap, base_len, seed):
    text = os.path.join(workdir, name + ".txt")
    n_seq = W.synth_pangenome_text(text, base_len=base_len, n_hap=n_hap, seed=seed, n_runs=1, n_run_len=(10, 40))
    ri, tags = W.build_index_from_text(text, workdir, name)[:2]
    return ri, tags, W.load_sequences(text), n_seq


def test_sets_equal_locate_batch_on_existing_cases(workdir, golden, x_index, synth):  # noqa: F811
    for name, ri, tags, seqs, ml, bidir, cat, offs in _cases(workdir, golden, x_index, synth):
        for mode in (P.MODE_COMPAT, P.MODE_STRICT):
            idx = P.Index(ri, tags, mode=mode)
            info = idx.info()
            if mode == P.MODE_COMPAT and info.is_encoded and not info.has_N:
                idx.close()
                continue  # (not supported there: test_compat_unsupported_leaves_results)
            b, res = _run_batch(idx, cat, offs, ml, 1)
            assert len(res["mems"]) > 0, name
            plain = _locate(b, 0)  # `resident` as today: what the flags = 0 form reports
            got = _check_sets(idx, b, res["mems"], want_resident=plain["resident"])
            assert plain["set_words"] == 0
            b.locate(SETS)
            dev = b.device_locations()
            assert dev["sets"].__cuda_array_interface__["shape"] == got["sets"].shape and dev["set_words"] == got["set_words"]
            b.free()
            idx.close()


@pytest.mark.parametrize("n_hap", [32, 33, 65])
def test_word_borders(workdir, n_hap):
    ri, tags, seqs, n_seq = _collection(workdir, "mls_border_%d" % n_hap, n_hap, 2000, 100 + n_hap)
    cat, offs = W.sample_reads(seqs, 400, 150, seed=n_hap)
    idx = P.Index(ri, tags)
    assert idx.info().n_sequences == n_seq == 2 * n_hap
    b, res = _run_batch(idx, cat, offs, 12, 1)
    got = _check_sets(idx, b, res["mems"], want_resident=True)
    per_mem = np.bitwise_count(got["sets"]).sum(axis=1) if hasattr(np, "bitwise_count") else np.unpackbits(got["sets"].view(np.uint8), axis=1).sum(axis=1)
    assert per_mem.max() >= n_seq // 4  # intervals that cover many sequences (a substring lies in one orientation: n_seq / 2 at the most), in every word
    assert (got["sets"] != 0).any(axis=0).all()
    b.free()
    idx.close()


def test_mem_wider_than_a_block_next_to_narrow_ones(workdir):
    ri, tags, seqs, n_seq = _collection(workdir, "mls_wide", 64, 5000, 7)
    long_cat, long_offs = W.sample_reads(seqs, 320, 150, seed=3)
    kmers = [bytes([a, c, g]) for a in b"ACGT" for c in b"ACGT" for g in b"ACGT"]
    reads = []
    for k, kmer in enumerate(kmers):  # interleaved: a 3-mer, then five long reads
        reads.append(kmer)
        reads += [bytes(long_cat[int(long_offs[r]):int(long_offs[r + 1])]) for r in range(5 * k, 5 * k + 5)]
    cat, offs = O.pack_reads(reads)
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 3, 1)
    sizes = res["mems"]["size"].astype(np.int64)
    assert (sizes > ML_SPAN).any() and ((sizes > 0) & (sizes < 64)).any(), (int(sizes.max()), int(sizes.min()))
    _check_sets(idx, b, res["mems"], want_resident=True)
    # the routed unique ids of the same batch
    _, off, vals, _, w = _expected(idx, res["mems"])
    got = _locate(b, UNIQ_IDS)
    assert got["set_words"] == w and got["loc_offsets"].tobytes() == off.tobytes() and got["values"].tobytes() == vals.tobytes()
    b.free()
    idx.close()


def test_passes_give_the_same_bytes(workdir, monkeypatch):
    ri, tags, seqs, n_seq = _collection(workdir, "mls_border_65", 65, 2000, 165)
    cat, offs = W.sample_reads(seqs, 400, 150, seed=65)
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 12, 1)
    exp, off, vals, _, w = _expected(idx, res["mems"])
    one = {f: _locate(b, f) for f in (SETS, SETS | P.LOCATE_CHAINS, UNIQ_IDS, UNIQ_IDS | P.LOCATE_CHAINS)}
    assert np.array_equal(one[SETS]["sets"], exp) and one[UNIQ_IDS]["values"].tobytes() == vals.tobytes()
    monkeypatch.setenv("PGX_LOCATE_BUDGET_MB", "0.002")  # 262 values a pass; 87 MEMs' sets a pass
    assert len(res["mems"]) * w > 4 * 262 and int(res["mems"]["size"].astype(np.int64).sum()) > 4 * 262
    for f, ref in one.items():
        got = _locate(b, f)
        assert got["values"].tobytes() == ref["values"].tobytes() and got["loc_offsets"].tobytes() == ref["loc_offsets"].tobytes(), f
        assert got["set_words"] == w and got["n_values"] == ref["n_values"] and got["n_not_located"] == ref["n_not_located"]
    b.free()
    idx.close()


def _device_write(dst, arr):
    """arr -> device memory at dst, by hipMemcpy of the HIP runtime libpgx.so runs on (already in the process; a second runtime that
    another package brought along does not know the pointer and refuses)"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line}, key=lambda p: "/torch/" in p)
    rcs = []
    for path in paths:
        fn = ctypes.CDLL(path).hipMemcpy
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int], ctypes.c_int
        rcs.append(fn(dst, arr.ctypes.data, arr.nbytes, 1))
        if rcs[-1] == 0:
            return
    raise AssertionError("hipMemcpy to the batch's MEM array failed: %r %r" % (paths, rcs))


def test_not_located(synth):  # noqa: F811
    ri, tags, seqs, cat, offs = synth
    idx = P.Index(ri, tags)
    n = int(idx.info().bwt_size)
    b, res = _run_batch(idx, cat, offs, 20, 1)
    mems = res["mems"]
    sizes = mems["size"].astype(np.int64)
    m = int(np.flatnonzero(sizes == int(np.median(sizes[sizes > 2])))[0])  # the chosen MEM
    s = int(sizes[m])
    for cap, located in ((s - 1, False), (s, True), (s + 1, True)):
        for extra in (0, P.LOCATE_CHAINS):
            got = _locate(b, SETS | extra, cap)
            assert got["n_not_located"] == int((sizes > cap).sum())
            assert got["sets"][m].any() == located
            assert not got["sets"][sizes > cap].any() and got["sets"][sizes <= cap].any(axis=1).all()
    _check_sets(idx, b, mems, max_occ=s)
    # hand-made MEMs, written over the batch's device array: size <= 0, a start beyond the BWT, a range that ends beyond it
    hacked = mems.copy()
    pick = np.flatnonzero(sizes > 0)[:6]
    hacked["size"][pick[0]] = 0
    hacked["size"][pick[1]] = -5
    hacked["bwt_start"][pick[2]] = n + 10
    hacked["bwt_start"][pick[3]], hacked["size"][pick[3]] = n - 1, 2
    hacked["size"][pick[4]] = 1 << 62
    hacked["bwt_start"][pick[5]], hacked["size"][pick[5]] = (1 << 64) - 1, 1
    dev = b.device_result()["mems"].__cuda_array_interface__["data"][0]
    _device_write(dev, hacked)
    assert _ranges(hacked, n)[2] == 6
    got = _check_sets(idx, b, hacked)
    assert got["n_not_located"] == 6 and not got["sets"][pick].any()
    _, off, vals, _, w = _expected(idx, hacked)
    for extra in (0, P.LOCATE_CHAINS):
        u = _locate(b, UNIQ_IDS | extra)
        assert u["set_words"] == w and u["n_not_located"] == 6
        assert u["loc_offsets"].tobytes() == off.tobytes() and u["values"].tobytes() == vals.tobytes()
    _device_write(dev, mems)
    b.free()
    idx.close()


def test_the_cap(workdir):
    # exactly 4096 sequences: W = 64, the sequence starts no longer fit the LDS window of the set kernel
    ri, tags, seqs, n_seq = _collection(workdir, "mls_cap_4096", 2048, 100, 11)
    assert n_seq == 4096
    cat, offs = W.sample_reads(seqs, 300, 60, seed=9)
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 12, 1)
    got = _check_sets(idx, b, res["mems"], want_resident=True)
    assert got["set_words"] == 64 and (got["sets"][:, 63] != 0).any()
    # only the narrow MEMs: more than 32 of them (2048 set words) share a block of values, which then takes several LDS windows
    sizes = res["mems"]["size"].astype(np.int64)
    assert ((sizes > 0) & (sizes <= 100)).sum() > 40
    _check_sets(idx, b, res["mems"], max_occ=100)
    _, off, vals, _, _ = _expected(idx, res["mems"])
    u = _locate(b, UNIQ_IDS)
    assert u["set_words"] == 64 and u["loc_offsets"].tobytes() == off.tobytes() and u["values"].tobytes() == vals.tobytes()
    b.free()
    idx.close()
    # 4098 sequences: no set form, find_mems results untouched, unique ids by the sort as before
    ri, tags, seqs, n_seq = _collection(workdir, "mls_cap_4098", 2049, 100, 12)
    assert n_seq == 4098
    cat, offs = W.sample_reads(seqs, 300, 60, seed=9)
    idx = P.Index(ri, tags)
    b, before = _run_batch(idx, cat, offs, 12, 1)
    for extra in (0, P.LOCATE_CHAINS):
        with pytest.raises(P.PgxError) as e:
            b.locate(SETS | extra)
        assert e.value.code == P.ERR_UNSUPPORTED
    with pytest.raises(P.PgxError) as e:
        b.locations()
    assert e.value.code == P.ERR_ARG
    after = b.result()
    assert after["mems"].tobytes() == before["mems"].tobytes() and np.array_equal(after["mem_offsets"], before["mem_offsets"])
    _, off, vals, n_not, _ = _expected(idx, before["mems"])
    u = _locate(b, UNIQ_IDS)
    assert u["set_words"] == 0 and u["n_not_located"] == n_not
    assert u["loc_offsets"].tobytes() == off.tobytes() and u["values"].tobytes() == vals.tobytes()
    b.free()
    idx.close()


def test_routing(synth, monkeypatch):  # noqa: F811
    ri, tags, seqs, cat, offs = synth
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 20, 1)
    _, off, vals, n_not, w = _expected(idx, res["mems"])
    for extra in (0, P.LOCATE_CHAINS):
        routed = _locate(b, UNIQ_IDS | extra)
        monkeypatch.setenv("PGX_LOCATE_SETS", "0")
        sorted_ = _locate(b, UNIQ_IDS | extra)
        monkeypatch.delenv("PGX_LOCATE_SETS")
        assert routed["set_words"] == w and sorted_["set_words"] == 0
        for got in (routed, sorted_):
            assert got["loc_offsets"].tobytes() == off.tobytes() and got["values"].tobytes() == vals.tobytes()
            assert got["flags"] == UNIQ_IDS and got["n_values"] == len(vals) and got["n_not_located"] == n_not
        assert routed["resident"] == sorted_["resident"] == (extra == 0)
    # unique packed positions and the plain forms build no sets
    for f in (0, P.LOCATE_SEQ_IDS, P.LOCATE_UNIQUE):
        assert _locate(b, f)["set_words"] == 0
    b.free()
    idx.close()


def test_repeat_and_flag_checks(synth):  # noqa: F811
    ri, tags, seqs, cat, offs = synth
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 20, 1)
    old = _locate(b, 0)
    old = (old["loc_offsets"].copy(), old["values"].copy())
    first = _locate(b, SETS)
    first = (first["loc_offsets"].copy(), first["values"].copy())
    again = _locate(b, SETS)  # the clear is per call: nothing is left over from the first
    assert again["loc_offsets"].tobytes() == first[0].tobytes() and again["values"].tobytes() == first[1].tobytes()
    plain = _locate(b, 0)
    assert plain["set_words"] == 0 and plain["flags"] == 0
    assert plain["loc_offsets"].tobytes() == old[0].tobytes() and plain["values"].tobytes() == old[1].tobytes()
    for f in (SETS | P.LOCATE_SEQ_IDS, SETS | P.LOCATE_UNIQUE, SETS | UNIQ_IDS, SETS | P.LOCATE_SEQ_IDS | P.LOCATE_CHAINS):
        with pytest.raises(P.PgxError) as e:
            b.locate(f)
        assert e.value.code == P.ERR_ARG
    # pgx_locate_batch keeps rejecting the flag
    with pytest.raises(P.PgxError) as e:
        idx.locate_batch(np.array([0], np.uint64), np.array([3], np.uint64), SETS)
    assert e.value.code == P.ERR_ARG
    b.free()
    idx.close()
