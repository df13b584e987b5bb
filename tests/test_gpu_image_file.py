"""The image file on the GPU tier: a handle opened from an image (no .ri, no tag file) searches, locates and counts as the handle it was
saved from; every section it uploads is summed on the device (pgx_image_sum_kernel) and compared with the file's table before any other
kernel reads it, so a damaged section is an error return naming it -- never a kernel walking damaged tables; pgx_image_sum on the device
agrees with the host form bit for bit, up to byte counts beyond 2^32."""
import os
import subprocess

import numpy as np
import pytest

import image_file_emu as E
import pgx_ffi as P
import pgx_workload as W
import variant_cases as V

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pangenome-index_amd")


@pytest.fixture(scope="module")
def mid(workdir):
    """the mid index as a file handle and as an image handle in one process, and the image's path"""
    case = V.mid_case(workdir)
    src = P.Index(case["ri_path"], case["tags_path"])
    path = os.path.join(workdir, "gpu_mid.pgi")
    src.save_image(path)
    img = P.Index.open_image(path)
    yield case, src, img, path
    src.close(); img.close()


def test_mid_case_both_ways(mid):
    case, src, img, _ = mid
    inf = img.info()
    assert inf.image_pairs == 1 and inf.image_in_lds == 0 and bytes(memoryview(inf)) == bytes(memoryview(src.info()))
    img.to_device()
    for w in (0, 15, 20, 22, 23):  # what the kernels read is what the file held
        assert img.device_view(w).tobytes() == img.image_view(w).tobytes() == src.image_view(w).tobytes(), w
    n = inf.bwt_size
    n_words = (n + 15) // 16 + 64
    for w, nbytes in ((30, n * 4), (31, n_words * 4), (32, (n_words // 1024 + 2) * 4), (33, n)):  # the LCE image: built from the symbol totals and max_length
        a, b = img.lce_view(w, nbytes), src.lce_view(w, nbytes)
        assert a.any() and np.array_equal(a, b), w
    for min_len, min_occ in ((20, 1), (20, 5)):
        ref = V.oracle(case, min_len, min_occ)
        res, t = V.run(img, case["cat"], case["offs"], min_len, min_occ)
        V.same(res, ref)
        _, ts = V.run(src, case["cat"], case["offs"], min_len, min_occ)
        assert t.kernels == ts.kernels and t.pairs_reads == ts.pairs_reads
        if (min_len, min_occ) == (20, 1):
            assert t.pairs_reads == 4


def test_x_and_xy_cases_from_images(workdir, x_index, xy_paths, golden):
    for case, kw in ((V.x_case(x_index, golden), {}), (V.xy_case(xy_paths, golden), dict(tags_format=P.TAGS_BYTECODE))):
        src = P.Index(case["ri_path"], case["tags_path"], **kw)
        path = os.path.join(workdir, "gpu_%s.pgi" % case["name"])
        src.save_image(path)
        src.close()
        img = P.Index.open_image(path)
        assert img.info().image_in_lds == 1 and img.info().image_kind == (P.IMAGE_DENSE if case["name"] == "x" else P.IMAGE_RL)  # both staged in LDS
        for min_len, min_occ in ((10, 1), (20, 2)):
            res, _ = V.run(img, case["cat"], case["offs"], min_len, min_occ)
            V.same(res, V.oracle(case, min_len, min_occ))
        img.close()


def test_small_wide_image(workdir):
    case = V.mid_small_case(workdir)
    with V.env({"PGX_SB_SHIFT": "3"}):
        src = P.Index(case["ri_path"], case["tags_path"], mode=P.MODE_COMPAT | P.MODE_IMAGE_PAIRS | P.MODE_IMAGE_WIDE)
    path = os.path.join(workdir, "gpu_wide.pgi")
    src.save_image(path)
    img = P.Index.open_image(path)
    assert img.info().image_wide == 1 and len(img.image_view(23)) > 24
    for w in (0, 20, 22, 23):
        assert img.device_view(w).tobytes() == src.image_view(w).tobytes()
    for min_len, min_occ in ((20, 1), (12, 2)):
        a, ta = V.run(img, case["cat"], case["offs"], min_len, min_occ)
        b, tb = V.run(src, case["cat"], case["offs"], min_len, min_occ)
        V.same(a, b)
        assert ta.kernels == tb.kernels and (ta.kernels & P.KERNELS_PAIRS_WIDE)
    src.close(); img.close()


def test_locate_from_image(mid, workdir, tmp_path):
    case, src, img, path = mid
    assert np.array_equal(img.decompress_sa(), src.decompress_sa())
    rng = np.random.default_rng(3)
    n = img.info().bwt_size
    first = rng.integers(0, n - 40, 300).astype(np.uint64)
    last = first + rng.integers(0, 40, 300).astype(np.uint64)
    for flags in (0, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE):
        a, b = img.locate_batch(first, last, flags), src.locate_batch(first, last, flags)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    reads = str(tmp_path / "reads.txt")
    with open(reads, "wb") as f:
        for i in range(400):
            f.write(bytes(case["cat"][int(case["offs"][i]):int(case["offs"][i + 1])]).replace(b"\n", b"").replace(b"\0", b"N") + b"\n")
    tail = [reads, "20", "1", "--locate", "positions", "--format", "device"]
    want = subprocess.run([os.path.join(PKG, "find_mems"), case["ri_path"], case["tags_path"]] + tail, capture_output=True)
    got = subprocess.run([os.path.join(PKG, "find_mems"), path, "-"] + tail, capture_output=True)
    assert want.returncode == 0 and got.returncode == 0, (want.stderr[-300:], got.stderr[-300:])
    cut = lambda out: out[:out.rindex(b"\nTotal time for finding all MEMs")]  # (the two closing lines are measured times)
    assert cut(got.stdout) == cut(want.stdout) and b"Occurrences: " in got.stdout


def test_literal_count_from_image(workdir, golden):
    rl = os.path.join(golden, "bidirectional_test", "contigs_xy.rl_bwt")
    enc, _ = W.build_index_from_rlbwt(rl, workdir, "gpu_q3", with_tags=False)
    src = P.Index(enc, None)
    path = os.path.join(workdir, "gpu_q3.pgi")
    src.save_image(path)
    img = P.Index.open_image(path)
    seqs = W.load_sequences(os.path.join(golden, "bidirectional_test", "contigs_xy"))
    cat, offs = W.sample_reads(seqs, 500, 12, seed=2)
    a, b = img.count_batch(cat, offs), src.count_batch(cat, offs)
    assert np.array_equal(a, b) and (a[:, 0] <= a[:, 1]).any()
    src.close(); img.close()


def test_image_without_locate(mid, workdir):
    case, src, _, _ = mid
    path = os.path.join(workdir, "gpu_mid_nl.pgi")
    src.save_image(path, no_locate=True)
    img = P.Index.open_image(path)
    small = V.mid_small_case(workdir)
    res, t = V.run(img, small["cat"], small["offs"], 20, 1)
    V.same(res, V.oracle(small, 20, 1))
    assert t.pairs_reads in (2, 3)  # the PAIRS kernel without the LCE image
    first = np.array([5], dtype=np.uint64)
    for call in (lambda: img.locate_batch(first, first), lambda: img.decompress_sa(), lambda: img.image_view(9)):
        with pytest.raises(P.PgxError) as e:
            call()
        assert e.value.code == P.ERR_UNSUPPORTED and "locate" in str(e.value)
    b = img.batch(small["cat"], small["offs"])
    b.run(20, 1, P.RUN_TAGS)
    with pytest.raises(P.PgxError) as e:
        b.locate()
    assert e.value.code == P.ERR_UNSUPPORTED
    b.free()
    img.close()


def test_corruption_is_caught_before_any_kernel_reads_it(mid, workdir):
    """one flipped byte in a section of a copy of the mid image: the open (without verify) succeeds, the upload's device sum refuses the
    section by name, twice the same; a good file then opens and searches in the same process"""
    case, _, _, path = mid
    data = open(path, "rb").read()
    f = E.ImageFile(data)
    small = V.mid_small_case(workdir)
    bad = os.path.join(workdir, "gpu_mid_bad.pgi")

    def flipped(name, where):
        s = f.by_name(name)
        assert s["bytes"] > 0
        b = bytearray(data)
        b[s["offset"] + {"first": 0, "middle": s["bytes"] // 2, "last": s["bytes"] - 1}[where]] ^= 0x10
        with open(bad, "wb") as fh:
            fh.write(bytes(b))

    for name, where in (("pairs", "middle"), ("blocks", "last"), ("tvals", "first")):
        flipped(name, where)
        img = P.Index.open_image(bad)
        for _ in range(2):
            with pytest.raises(P.PgxError) as e:
                img.to_device()
            assert e.value.code == P.ERR_FORMAT and "section " + name + ":" in str(e.value), str(e.value)
        img.close()
    flipped("rsamp", "middle")
    img = P.Index.open_image(bad)
    img.to_device()  # (the locate image is uploaded, and checked, on its first use)
    first = np.array([7, 100], dtype=np.uint64)
    for _ in range(2):
        with pytest.raises(P.PgxError) as e:
            img.locate_batch(first, first + np.uint64(3))
        assert e.value.code == P.ERR_FORMAT and "section rsamp:" in str(e.value), str(e.value)
    img.close()
    good = P.Index.open_image(path)
    res, _ = V.run(good, small["cat"], small["offs"], 20, 1)
    V.same(res, V.oracle(small, 20, 1))
    assert len(good.locate_batch(first, first + np.uint64(3))[1]) == 8
    good.close()


def test_image_sum_on_the_device():
    rng = np.random.default_rng(5)
    for n in [0, 1, 7, 8, 9, 15, 16, 17, 4095, 4096, 4097, (1 << 20) + 3, (64 << 20) + 5]:
        data = rng.integers(0, 256, n, dtype=np.uint8)
        host = P.image_sum(data, device=-1)
        if n <= (1 << 20) + 3:
            assert host == E.section_sum(data), n  # the host form pinned to numpy; it is the reference beyond
        assert P.image_sum(data, device=0) == host, n
    # the byte count at which a 32-bit index goes wrong (the wide PAIRS section of a 2^32-symbol index lies beyond it)
    n = (4 << 30) + 13
    z = np.zeros(n, dtype=np.uint8)
    z[0], z[(3 << 30) + 5], z[n - 1] = 0x5A, 0xC3, 0x81  # the first, one middle and the last byte
    assert P.image_sum(z, device=0) == P.image_sum(z, device=-1)
