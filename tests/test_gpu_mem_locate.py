"""GPU tier of pgx_batch_locate: the occurrences of every MEM of a batch, located on the device from the batch's own MEM array, equal
pgx_locate_batch on the MEM's range -- the only definition of correctness (include/pgx.h) -- for every flag form, on both device
paths (the resident suffix array of the LCE image and the sample chains), with the cap, the passes of a small budget, chunked and
speculative runs, and the COMPAT case the locate path does not support."""
import os

import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W

pytestmark = pytest.mark.gpu

FLAGS = (0, P.LOCATE_SEQ_IDS, P.LOCATE_UNIQUE, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE)


def _ranges(mems, n, max_occ=0):
    """the BWT range of every MEM as pgx_batch_locate takes it ({1, 0} = empty where it is not located) and the not-located count"""
    size = mems["size"].astype(np.int64)
    bs = mems["bwt_start"].astype(np.uint64)
    su = np.maximum(size, 0).astype(np.uint64)
    ok = (size > 0) & (bs < np.uint64(n)) & (su <= np.uint64(n) - np.minimum(bs, np.uint64(n)))
    if max_occ:
        ok &= su <= np.uint64(max_occ)
    first = np.where(ok, bs, np.uint64(1)).astype(np.uint64)
    last = np.where(ok, bs + su - np.uint64(1), np.uint64(0)).astype(np.uint64)
    return first, last, int((~ok).sum())


def _locate(b, flags, max_occ=0):
    b.locate(flags, max_occ)
    return b.locations()


def _check_against_locate_batch(idx, b, mems, flags_list=FLAGS, max_occ=0, chains_too=True):
    """every flag form == pgx_locate_batch on the MEMs' ranges; with chains_too the chain path gives the same bytes.  Returns the
    flags = 0 result."""
    n = idx.info().bwt_size
    first, last, n_not = _ranges(mems, n, max_occ)
    out = None
    for flags in flags_list:
        got = _locate(b, flags, max_occ)
        off, vals = idx.locate_batch(first, last, flags)
        assert np.array_equal(got["loc_offsets"], off), flags
        assert got["values"].tobytes() == vals.tobytes(), flags
        assert got["n_values"] == len(vals) and got["n_not_located"] == n_not and got["flags"] == flags
        if chains_too:
            ch = _locate(b, flags | P.LOCATE_CHAINS, max_occ)
            assert not ch["resident"]
            assert np.array_equal(ch["loc_offsets"], off) and ch["values"].tobytes() == vals.tobytes(), flags
        if flags == 0:
            out = (got["loc_offsets"], got["values"], got["resident"])
    return out


def _check_oracle_and_text(ri_path, seqs, mems, off, vals, cat, offs, mem_offsets, strict):
    """the packed values are the oracle's suffix-array rows; on STRICT indexes each one spells its MEM's substring
    read[start:end] in the text"""
    sa = O.RIndex(ri_path).decompress_sa()
    ml = O.RIndex(ri_path).max_length
    read_of = np.repeat(np.arange(len(mem_offsets) - 1), np.diff(mem_offsets.astype(np.int64)))
    for m in range(len(mems)):
        a, c = int(off[m]), int(off[m + 1])
        if a == c:
            continue
        bs = int(mems[m]["bwt_start"])
        assert np.array_equal(vals[a:c], sa[bs:bs + (c - a)]), m
        if strict and m % 3 == 0:
            r = int(read_of[m])
            pat = bytes(cat[int(offs[r]) + int(mems[m]["start"]):int(offs[r]) + int(mems[m]["end"])])  # (a MEM is [start, end), algorithm.hpp:708)
            for v in vals[a:c][:50]:
                q, o = int(v) // ml, int(v) % ml
                assert bytes(seqs[q][o:o + len(pat)]) == pat, (m, q, o)


def _run_batch(idx, cat, offs, min_len, min_occ, flags=P.RUN_TAGS):
    b = P.Batch(idx, cat, offs)
    b.run(min_len, min_occ, flags)
    return b, b.result()


@pytest.fixture(scope="module")
def synth(workdir):
    text = os.path.join(workdir, "mloc_synth.txt")
    W.synth_pangenome_text(text, base_len=30000, n_hap=4, seed=91, n_runs=2, n_run_len=(50, 400))
    ri, tags = W.build_index_from_text(text, workdir, "mloc_synth")[:2]
    seqs = W.load_sequences(text)
    cat, offs = W.sample_reads(seqs, 3000, 150, seed=5)
    return ri, tags, seqs, cat, offs


def _cases(workdir, golden, x_index, synth):
    med_ri, med_tags = W.build_index_from_rlbwt(os.path.join(golden, "med_test.rl_bwt"), workdir, "mloc_med")
    med_seqs = W.load_sequences(os.path.join(golden, "med_test.txt"))
    x_seqs = W.load_sequences(os.path.join(golden, "x.newline_separated"))
    bt = os.path.join(golden, "bidirectional_test")
    xy_seqs = W.load_sequences(os.path.join(bt, "contigs_xy"))
    xy_reads = [l for l in open(os.path.join(bt, "reads.txt"), "rb").read().split(b"\n") if l]
    xy_cat, xy_offs = O.pack_reads(xy_reads)
    out = []
    # (bidir: every sequence next to its reverse complement, where the FMD intervals of a MEM are those of its substring)
    for name, ri, tags, seqs, ml, bidir, (cat, offs) in (
            ("med", med_ri, med_tags, med_seqs, 3, False, W.sample_reads(med_seqs, 300, 6, seed=3)),
            ("x", x_index[0], x_index[1], x_seqs, 10, False, W.sample_reads(x_seqs, 1500, 150, seed=4)),
            ("xy", os.path.join(bt, "xy.ri"), os.path.join(bt, "xy_bidirectional_compressed.tags"), xy_seqs, 3, True, (xy_cat, xy_offs)),
            ("synth", synth[0], synth[1], synth[2], 20, True, (synth[3], synth[4]))):
        out.append((name, ri, tags, seqs, ml, bidir, cat, offs))
    return out


def test_every_mem_equals_locate_batch(workdir, golden, x_index, synth):
    for name, ri, tags, seqs, ml, bidir, cat, offs in _cases(workdir, golden, x_index, synth):
        for mode in (P.MODE_COMPAT, P.MODE_STRICT):
            idx = P.Index(ri, tags, mode=mode)
            info = idx.info()
            if mode == P.MODE_COMPAT and info.is_encoded and not info.has_N:
                idx.close()
                continue  # (test_compat_unsupported)
            b, res = _run_batch(idx, cat, offs, ml, 1)
            assert len(res["mems"]) > 0, name
            off, vals, _ = _check_against_locate_batch(idx, b, res["mems"])
            _check_oracle_and_text(ri, seqs, res["mems"], off, vals, cat, offs, res["mem_offsets"], bidir and mode == P.MODE_STRICT)
            # the result stays where it is: device pointers of the same arrays
            b.locate(0)
            dev = b.device_locations()
            assert dev["n_values"] == len(vals) and dev["loc_offsets"].__cuda_array_interface__["shape"] == (len(res["mems"]) + 1,)
            b.free()
            idx.close()


def test_resident_path_equals_chains(synth):
    ri, tags, seqs, cat, offs = synth
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 20, 1)
    off, vals, resident = _check_against_locate_batch(idx, b, res["mems"])
    assert resident, "the synthetic bidirectional collection keeps its suffix array on the device (LCE image)"
    for flags in FLAGS:
        r = _locate(b, flags)
        c = _locate(b, flags | P.LOCATE_CHAINS)
        assert r["resident"] and not c["resident"]
        assert r["loc_offsets"].tobytes() == c["loc_offsets"].tobytes() and r["values"].tobytes() == c["values"].tobytes()
    b.free()
    idx.close()


def test_wide_image_uses_chains(workdir, monkeypatch):
    text = os.path.join(workdir, "mloc_wide.txt")
    W.synth_pangenome_text(text, base_len=20000, n_hap=3, seed=17, n_runs=1, n_run_len=(50, 200))
    ri, tags = W.build_index_from_text(text, workdir, "mloc_wide")[:2]
    seqs = W.load_sequences(text)
    cat, offs = W.sample_reads(seqs, 1000, 150, seed=2)
    monkeypatch.setenv("PGX_SB_SHIFT", "6")
    idx = P.Index(ri, tags, mode=P.MODE_COMPAT | P.MODE_IMAGE_WIDE)
    assert idx.info().image_wide
    b, res = _run_batch(idx, cat, offs, 20, 1)
    _, _, resident = _check_against_locate_batch(idx, b, res["mems"], chains_too=False)
    assert not resident
    b.free()
    idx.close()


def test_max_occ_boundaries(synth):
    ri, tags, seqs, cat, offs = synth
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 20, 1)
    sizes = res["mems"]["size"].astype(np.int64)
    s = int(np.median(sizes[sizes > 1]))
    for cap in (s, s - 1, 1):
        for flags in (0, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE):
            for extra in (0, P.LOCATE_CHAINS):
                got = _locate(b, flags | extra, cap)
                assert got["n_not_located"] == int((sizes > cap).sum())
                cnt = np.diff(got["loc_offsets"].astype(np.int64))
                assert np.all(cnt[sizes > cap] == 0) and np.all(cnt[sizes <= cap] > 0)
                if flags == 0:
                    assert np.array_equal(cnt[sizes <= cap], sizes[sizes <= cap])
    _check_against_locate_batch(idx, b, res["mems"], max_occ=s)
    b.free()
    idx.close()


def test_edge_cases(synth, monkeypatch):
    ri, tags, seqs, cat, offs = synth
    idx = P.Index(ri, tags)
    # an empty batch, and reads without MEMs
    b = P.Batch(idx, np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    with pytest.raises(P.PgxError) as e:
        b.locate()
    assert e.value.code == P.ERR_ARG  # no run yet
    b.run(20, 1, P.RUN_TAGS)
    for flags in FLAGS:
        got = _locate(b, flags)
        assert list(got["loc_offsets"]) == [0] and got["n_values"] == 0 and got["n_not_located"] == 0
    ecat, eoffs = O.pack_reads([b"ACGT", b"ACGTAC", b"", b"ACGTTGCA" * 2])  # (shorter than min_len)
    b.upload(ecat, eoffs)
    with pytest.raises(P.PgxError):
        b.locations()  # an upload ends the locate result
    b.run(20, 1, P.RUN_TAGS)
    assert len(b.result()["mems"]) == 0
    assert list(_locate(b, 0)["loc_offsets"]) == [0]
    # a speculative re-run of the same batch, then a second locate
    b.upload(cat, offs)
    b.run(20, 1, P.RUN_TAGS)
    first = b.result()
    ref = {f: _locate(b, f) for f in FLAGS}
    b.run(20, 1, P.RUN_TAGS)
    assert b.spec_stats()[0] >= 1
    with pytest.raises(P.PgxError):
        b.locations()  # a run ends it too
    assert b.result()["mems"].tobytes() == first["mems"].tobytes()
    for f in FLAGS:
        got = _locate(b, f)
        assert got["values"].tobytes() == ref[f]["values"].tobytes() and got["loc_offsets"].tobytes() == ref[f]["loc_offsets"].tobytes()
    # a budget of a few hundred values: many passes, the same bytes on both paths
    monkeypatch.setenv("PGX_LOCATE_BUDGET_MB", "0.002")
    for f in FLAGS:
        for extra in (0, P.LOCATE_CHAINS):
            got = _locate(b, f | extra)
            assert got["values"].tobytes() == ref[f]["values"].tobytes() and got["loc_offsets"].tobytes() == ref[f]["loc_offsets"].tobytes(), f
    monkeypatch.delenv("PGX_LOCATE_BUDGET_MB")
    b.free()
    # a chunked run (a small slot budget): the same MEMs, the same occurrences
    monkeypatch.setenv("PGX_SLOT_BUDGET_MB", "1")
    b2 = P.Batch(idx, cat, offs)
    b2.run(20, 1, P.RUN_TAGS)
    assert b2.result()["mems"].tobytes() == first["mems"].tobytes()
    for f in FLAGS:
        assert _locate(b2, f)["values"].tobytes() == ref[f]["values"].tobytes()
    b2.free()
    idx.close()


def test_compat_unsupported_leaves_results(golden, workdir):
    enc = os.path.join(workdir, "mloc_x_enc.ri")
    P.build_rindex(os.path.join(golden, "x.rl_bwt"), enc, encoded=True)
    idx = P.Index(enc, mode=P.MODE_COMPAT)
    assert idx.info().is_encoded and not idx.info().has_N
    seqs = W.load_sequences(os.path.join(golden, "x.newline_separated"))
    cat, offs = W.sample_reads(seqs, 300, 150, seed=8)
    b, before = _run_batch(idx, cat, offs, 10, 1, flags=0)
    for flags in FLAGS:
        with pytest.raises(P.PgxError) as e:
            b.locate(flags)
        assert e.value.code == P.ERR_UNSUPPORTED and "PGX_MODE_STRICT" in str(e.value)
    after = b.result()
    assert after["mems"].tobytes() == before["mems"].tobytes() and np.array_equal(after["mem_offsets"], before["mem_offsets"])
    with pytest.raises(P.PgxError) as e:
        b.locations()
    assert e.value.code == P.ERR_ARG
    b.free()
    idx.close()


def test_scale_sample_every_61st_mem(workdir):
    """1 M reads on the 1/10-scale synthetic pangenome (n = 64 M, tests/test_gpu_fullsize.py): every 61st MEM against pgx_locate_batch"""
    text = os.path.join(workdir, "full_synth.txt")
    if not os.path.exists(text):
        W.synth_pangenome_text(text, base_len=4_000_000)
    ri, tags = W.build_index_from_text(text, workdir, "full_synth")[:2]
    seqs = W.load_sequences(text)
    cat, offs = W.sample_reads(seqs, 1_000_000, 150, seed=11)
    idx = P.Index(ri, tags)
    b, res = _run_batch(idx, cat, offs, 20, 1, flags=P.RUN_TAGS | P.RUN_TIMING)
    mems = res["mems"]
    pick = np.arange(0, len(mems), 61)
    first, last, _ = _ranges(mems[pick], idx.info().bwt_size)
    for flags in (0, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE):
        got = _locate(b, flags)
        assert got["resident"]
        off, vals = idx.locate_batch(first, last, flags)
        lo = got["loc_offsets"]
        for k, m in enumerate(pick):
            assert np.array_equal(got["values"][int(lo[m]):int(lo[m + 1])], vals[int(off[k]):int(off[k + 1])]), (flags, int(m))
        print("\n[mem_locate] %d MEMs, %d values (flags %d): %.3f ms on the device, find_mems step %.3f ms"
              % (len(mems), got["n_values"], flags, got["ms_locate"], b.timing().ms_total))
    b.free()
    idx.close()
