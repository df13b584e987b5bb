"""The image file (include/pgx.h "image file": pgx_index_save_image / pgx_index_open_image / pgx_image_file_info / pgx_image_sum) on the
CPU tier: a handle opened from an image answers as the handle it was saved from, byte for byte; the file is what image_file_emu.py reads
from the header's text alone; damaged, truncated and foreign files are refused with a status and a message, never a crash."""
import os
import struct
import subprocess

import numpy as np
import pytest

import image_file_emu as E
import pgx_ffi as P
import pgx_workload as W
import variant_cases as V

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pangenome-index_amd")
VIEWS = range(24)


def views_of(idx):
    """every host view the handle has: selector -> bytes (a selector that does not exist for the index -> the error code)"""
    out = {}
    for w in VIEWS:
        try:
            out[w] = idx.image_view(w).tobytes()
        except P.PgxError as e:
            out[w] = ("error", e.code)
    return out


def info_bytes(idx):
    inf = idx.info()
    return bytes(memoryview(inf))


def same_handles(a, b):
    va, vb = views_of(a), views_of(b)
    for w in VIEWS:
        assert va[w] == vb[w], "view %d" % w
    assert info_bytes(a) == info_bytes(b)
    if a.info().n_dev_blocks or a.info().sigma:
        ta, tb = a.tables(), b.tables()
        assert all(np.array_equal(x, y) for x, y in zip(ta, tb))
    else:
        for h in (a, b):
            with pytest.raises(P.PgxError) as e:
                h.tables()
            assert e.value.code == P.ERR_ARG


def _open(case):
    kind, args, envs = case
    with V.env(envs):
        if kind == "paths":
            return P.Index(*args[0], **args[1])
        ri_bytes, tags_bytes, mode = args
        h = P.p()
        L = P.lib()
        L.pgx_index_open_memory.argtypes = [P.C.c_char_p, P.u64, P.C.c_char_p, P.u64, P.u32, P.u32, P.C.POINTER(P.p)]
        P._check(L.pgx_index_open_memory(ri_bytes, len(ri_bytes) if ri_bytes else 0, tags_bytes, len(tags_bytes) if tags_bytes else 0, P.TAGS_AUTO, mode, P.C.byref(h)))
        idx = P.Index.__new__(P.Index)
        idx.L, idx.h = L, h
        return idx


@pytest.fixture(scope="module")
def cases(workdir, golden, x_index, xy_paths):
    bt = os.path.join(golden, "bidirectional_test")
    enc_no_n, _ = W.build_index_from_rlbwt(os.path.join(bt, "contigs_xy.rl_bwt"), workdir, "img_xy_enc", with_tags=False)
    mid = V.mid_case(workdir)
    tags_only = open(x_index[1], "rb").read()
    return {
        "xy_legacy_bytecode": ("paths", ((xy_paths[0], xy_paths[1]), dict(tags_format=P.TAGS_BYTECODE)), {}),
        "x_encoded_lds": ("paths", ((x_index[0], x_index[1]), {}), {}),
        "encoded_no_n_compat": ("paths", ((enc_no_n, None), {}), {}),
        "tags_only": ("memory", (None, tags_only, P.MODE_COMPAT), {}),
        "ri_only": ("paths", ((x_index[0], None), {}), {}),
        "mid_pairs": ("paths", ((mid["ri_path"], mid["tags_path"]), dict(mode=P.MODE_COMPAT | P.MODE_IMAGE_PAIRS)), {}),
        "mid_dense2": ("paths", ((mid["ri_path"], mid["tags_path"]), dict(mode=P.MODE_COMPAT | P.MODE_IMAGE_DENSE2)), {}),
        "mid_wide": ("paths", ((mid["ri_path"], mid["tags_path"]), dict(mode=P.MODE_COMPAT | P.MODE_IMAGE_PAIRS | P.MODE_IMAGE_WIDE)), {"PGX_SB_SHIFT": "3"}),
    }


CASE_NAMES = ["xy_legacy_bytecode", "x_encoded_lds", "encoded_no_n_compat", "tags_only", "ri_only", "mid_pairs", "mid_dense2", "mid_wide"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_round_trip(cases, tmp_path, name):
    src = _open(cases[name])
    p1, p2, p3 = (str(tmp_path / ("%s_%d.pgi" % (name, k))) for k in range(3))
    src.save_image(p1)
    src.save_image(p2)
    b1 = open(p1, "rb").read()
    assert b1 == open(p2, "rb").read()  # the same index saved twice: the same bytes
    img = P.Index.open_image(p1)
    same_handles(src, img)
    if name == "mid_wide":
        assert img.info().image_wide == 1 and len(img.image_view(23)) > 24
    if name == "encoded_no_n_compat":
        assert len(img.image_view(18)) > 0
    img.save_image(p3)
    assert open(p3, "rb").read() == b1  # save(open_image(save(h)))
    ver = P.Index.open_image(p1, verify=True)
    same_handles(src, ver)
    # the file, read without the library
    f = E.ImageFile(b1)
    assert f.version == E.FILE_VERSION and f.header_sum == f.computed_header_sum() and f.reserved == 0
    inf = src.info()
    assert (f.mode, f.has_rank, f.has_tags) == (inf.mode, 1 if name != "tags_only" else 0, inf.has_tags)
    assert f.sequence_size == inf.bwt_size and f.max_length == inf.max_length and f.n_samples == inf.n_samples and f.n_file_blocks == inf.n_ref_blocks
    assert (f.encoded, f.hasN, f.tags_format, f.sigma) == (inf.is_encoded, inf.has_N, inf.tag_format, inf.sigma)
    if f.has_rank:
        assert sum(f.sym_total) == inf.bwt_size and f.sym_total[0] == inf.n_sequences
    end = f.head_bytes
    sv = views_of(src)
    assert [s["id"] for s in f.sections] == sorted(s["id"] for s in f.sections)
    for s in f.sections:
        assert s["offset"] % E.ALIGN == 0 and s["offset"] >= end and s["offset"] + s["bytes"] <= len(b1), s
        assert s["offset"] - end < E.ALIGN and not any(b1[end:s["offset"]])  # zero bytes between sections, each where the last one ends
        end = s["offset"] + s["bytes"]
        assert E.section_sum(f.section_bytes(s)) == s["sum"], s["name"]
        if s["id"] in E.SECTION_VIEW:
            assert f.section_bytes(s) == sv[E.SECTION_VIEW[s["id"]]], s["name"]
    assert end == len(b1)
    assert struct.unpack("<Q", f.section_bytes(f.by_name("n_runs")))[0] == inf.n_runs
    has_loc = any(s["name"] == "rsamp" for s in f.sections)
    assert has_loc == bool(f.has_rank) and bool(f.flags & E.HAS_LOCATE) == has_loc
    literal = bool(f.has_rank and inf.mode == P.MODE_COMPAT and inf.is_encoded and not inf.has_N)  # where pgx_count_batch goes through it
    assert bool(f.flags & E.HAS_LITERAL) == literal == any(s["name"] == "lit_runs" for s in f.sections)
    assert literal or name not in ("encoded_no_n_compat", "x_encoded_lds")
    # pgx_image_file_info: the same table
    fi = P.image_file_info(p1)
    assert fi["n_sections"] == f.n_sections and fi["file_bytes"] == len(b1) and fi["header_sum"] == f.header_sum
    assert [(s["id"], s["name"], s["bytes"], s["offset"], s["sum"]) for s in fi["sections"]] == [(s["id"], s["name"], s["bytes"], s["offset"], s["sum"]) for s in f.sections]
    for h in (src, img, ver):
        h.close()


def test_no_locate_image(cases, tmp_path):
    src = _open(cases["mid_pairs"])
    p1, p2 = str(tmp_path / "nl.pgi"), str(tmp_path / "nl2.pgi")
    src.save_image(p1, no_locate=True)
    f = E.ImageFile(open(p1, "rb").read())
    assert not (f.flags & E.HAS_LOCATE) and f.n_sections == 13
    img = P.Index.open_image(p1)
    for w in range(8, 15):
        with pytest.raises(P.PgxError) as e:
            img.image_view(w)
        assert e.value.code == P.ERR_UNSUPPORTED and "locate" in str(e.value)
    for w in (0, 6, 20, 3, 4):
        assert img.image_view(w).tobytes() == src.image_view(w).tobytes()
    assert info_bytes(img) == info_bytes(src)
    with pytest.raises(P.PgxError) as e:
        img.save_image(p2)  # it has no locate image to save
    assert e.value.code == P.ERR_UNSUPPORTED and not os.path.exists(p2)
    img.save_image(p2, no_locate=True)
    assert open(p2, "rb").read() == open(p1, "rb").read()
    assert [n for n in os.listdir(str(tmp_path)) if ".tmp." in n] == []  # no temporary file stays behind
    with pytest.raises(P.PgxError) as e:
        src.save_image(str(tmp_path / "no_such_dir" / "x.pgi"))
    assert e.value.code == P.ERR_IO
    src.close(); img.close()


SUM_LENGTHS = [0, 1, 7, 8, 9, 4095, 4096, 4097, (1 << 20) + 3]


def test_image_sum_host_against_numpy(built):
    rng = np.random.default_rng(5)
    for n in SUM_LENGTHS:
        data = rng.integers(0, 256, n, dtype=np.uint8)
        want = E.section_sum(data)
        assert P.image_sum(data, device=-1) == want, n
        if n == 0:
            assert want == 0
            continue
        for at in sorted({0, n // 2, n - 1}):  # one flipped bit at the first, a middle and the last byte
            d2 = data.copy()
            d2[at] ^= 1 << int(rng.integers(0, 8))
            got = P.image_sum(d2, device=-1)
            assert got != want and got == E.section_sum(d2), (n, at)
        if n >= 16:  # two swapped words
            d2 = data.copy()
            d2[0:8], d2[8:16] = data[8:16], data[0:8]
            if not np.array_equal(d2, data):
                got = P.image_sum(d2, device=-1)
                assert got != want and got == E.section_sum(d2)
    z = np.zeros(4096, dtype=np.uint8)  # equal words at different places do not cancel: zeros of two lengths differ
    assert P.image_sum(z, -1) != P.image_sum(z[:4088], -1) != 0


@pytest.fixture(scope="module")
def good_image(cases, workdir):
    """the image of the x index with its tags (encoded, no N: every section group, the literal one included), its bytes and its parsed form"""
    src = _open(cases["x_encoded_lds"])
    path = os.path.join(workdir, "reject_x.pgi")
    src.save_image(path)
    src.close()
    data = open(path, "rb").read()
    return path, data, E.ImageFile(data)


def _refused(path, data, verify=False):
    with open(path, "wb") as f:
        f.write(data)
    with pytest.raises(P.PgxError) as e:
        P.Index.open_image(path, verify=verify).close()
    assert e.value.code in (P.ERR_FORMAT, P.ERR_UNSUPPORTED) and len(str(e.value)) > 20
    return e.value


def test_truncated_files_are_refused(good_image, tmp_path):
    _, data, f = good_image
    path = str(tmp_path / "cut.pgi")
    cuts = set()
    for s in f.sections:
        for at in (s["offset"], s["offset"] + s["bytes"]):
            cuts.update((at - 1, at, at + 1))
    cuts.update((0, 7, 8, 63, 64, f.head_bytes - 1, f.head_bytes))
    rng = np.random.default_rng(11)
    cuts.update(int(v) for v in rng.integers(0, len(data), 200))
    for n in sorted(c for c in cuts if 0 <= c < len(data)):
        err = _refused(path, data[:n])
        assert err.code == P.ERR_FORMAT, n
        if n >= f.head_bytes:  # the table is whole: the section that no longer fits is named
            first = next(s for s in f.sections if s["offset"] + s["bytes"] > n or s["offset"] > n)
            assert "section " + first["name"] + ":" in str(err), (n, str(err))


def test_header_and_table_fields_are_checked(good_image, tmp_path):
    _, data, f = good_image
    path = str(tmp_path / "field.pgi")

    def with_u32(at, v, seal=True):
        b = bytearray(data)
        struct.pack_into("<I", b, at, v & 0xFFFFFFFF)
        return bytes(E.reseal(b)) if seal else bytes(b)

    def with_u64(at, v):
        b = bytearray(data)
        struct.pack_into("<Q", b, at, v & 0xFFFFFFFFFFFFFFFF)
        return bytes(E.reseal(b))

    # identity: another build
    for at, v in ((8, 2), (12, f.layout + 1), (16, f.consts_bytes + 8), (20, f.loc_consts_bytes - 8), (40, f.meta_bytes + 8)):
        err = _refused(path, with_u32(at, v, seal=False))
        assert err.code == P.ERR_UNSUPPORTED and "another build" in str(err), at
    assert _refused(path, b"PGXIMAGF" + data[8:]).code == P.ERR_FORMAT
    # section count 0 and 2^32 - 1 (nothing is allocated by it), and one section fewer
    for v in (0, 0xFFFFFFFF, 65):
        assert _refused(path, with_u32(36, v, seal=False)).code == P.ERR_FORMAT
    # header fields behind the sum: mode, has_rank, has_tags, flags
    for at, v in ((24, 1), (24, 7), (28, 0), (32, 0), (44, 0), (44, f.flags ^ E.HAS_LOCATE), (44, f.flags ^ E.HAS_LITERAL), (44, f.flags | 4)):
        assert _refused(path, with_u32(at, v)).code == P.ERR_FORMAT, (at, v)
    # an unsealed change of any of them: the header sum
    assert "header sum" in str(_refused(path, with_u32(24, 1, seal=False)))
    # every table entry: id, element size, length, offset
    for s in f.sections:
        e = s["entry_at"]
        named = "section " + s["name"] + ":"
        bad = [with_u32(e, s["id"] + 1), with_u32(e + 4, s["elem_size"] * 2), with_u64(e + 8, s["bytes"] * 2 if s["bytes"] else 8),
               with_u64(e + 8, s["bytes"] + s["elem_size"]), with_u64(e + 8, (1 << 64) - s["offset"] + 8),  # offset + length wraps
               with_u64(e + 8, (1 << 64) - 8), with_u64(e + 16, len(data) + E.ALIGN - len(data) % E.ALIGN), with_u64(e + 16, s["offset"] + E.ALIGN),
               with_u64(e + 16, s["offset"] + 8), with_u64(e + 16, 0), with_u64(e + 16, (1 << 64) - E.ALIGN)]
        for k, b in enumerate(bad):
            err = _refused(path, b)
            assert err.code == P.ERR_FORMAT and named in str(err), (s["name"], k, str(err))
    # the counts of the meta record and the scalars the constants must agree with
    for at in (f.meta_at + 424, f.meta_at + 432, f.meta_at + 336, f.meta_at + 368):
        (v,) = struct.unpack_from("<Q", data, at)
        for nv in (v + 1, v * 2 + (1 << 61), (1 << 64) - 1):
            assert _refused(path, with_u64(at, nv)).code == P.ERR_FORMAT, at
    # a sealed change of a stored sum passes the open (documented: the sums are checked on the device, or on the host with verify)
    s = f.by_name("blocks")
    b = with_u64(s["entry_at"] + 24, s["sum"] ^ 1)
    with open(path, "wb") as fh:
        fh.write(b)
    P.Index.open_image(path).close()
    assert "section blocks:" in str(_refused(path, b, verify=True))


def test_foreign_files_and_random_mutations(good_image, tmp_path, x_index):
    _, data, f = good_image
    path = str(tmp_path / "mut.pgi")
    for junk in (b"", open(x_index[0], "rb").read(), b"PGXIMAG", b"PGXIMAGE", os.urandom(4096)):
        assert _refused(path, junk).code == P.ERR_FORMAT
    with pytest.raises(P.PgxError) as e:
        P.Index.open_image(str(tmp_path / "missing.pgi"))
    assert e.value.code == P.ERR_IO
    with pytest.raises(P.PgxError) as e:
        P.image_file_info(x_index[0])
    assert e.value.code == P.ERR_FORMAT
    rng = np.random.default_rng(23)
    for k in range(300):  # header + table + meta: the header sum covers every byte of the region
        b = bytearray(data)
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, f.head_bytes))
            b[at] ^= int(rng.integers(1, 256))
        _refused(path, bytes(b))
        if k % 3 == 0 and bytes(b[:8]) == E.MAGIC:  # the same damage behind a header sum that agrees with it: the checks behind the sum hold alone
            try:
                sealed = bytes(E.reseal(bytearray(b)))
            except ValueError:
                continue
            with open(path, "wb") as fh:
                fh.write(sealed)
            try:
                P.Index.open_image(path, verify=True).close()  # (a byte no check reads, e.g. of sym_map, may pass)
            except P.PgxError as err:
                assert err.code in (P.ERR_FORMAT, P.ERR_UNSUPPORTED)


def test_flipped_byte_in_every_section(good_image, tmp_path):
    _, data, f = good_image
    path = str(tmp_path / "flip.pgi")
    rng = np.random.default_rng(31)
    for s in f.sections:
        if not s["bytes"] or s["name"] in ("consts", "loc_consts"):
            continue  # (the two constant records are checked field by field on the way in: see below)
        b = bytearray(data)
        b[s["offset"] + int(rng.integers(0, s["bytes"]))] ^= 0x40
        err = _refused(path, bytes(b), verify=True)
        assert err.code == P.ERR_FORMAT and "section " + s["name"] + ":" in str(err), s["name"]
        P.Index.open_image(path).close()  # without verify the open succeeds: the device check catches it (tests/test_gpu_image_file.py)
    for name in ("consts", "loc_consts"):  # a byte of a table inside the constants (no length depends on it): verify names the section
        s = f.by_name(name)
        b = bytearray(data)
        b[s["offset"] + (100 if name == "consts" else 28)] ^= 0x40  # ext_tab / max_length
        err = _refused(path, bytes(b), verify=True)
        assert err.code == P.ERR_FORMAT and "section " + name + ":" in str(err)


def test_cli(built, good_image, x_index, tmp_path):
    _, data, f = good_image
    out = str(tmp_path / "cli.pgi")
    r = subprocess.run([os.path.join(PKG, "pgx_image"), x_index[0], x_index[1], out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == data  # the CLI writes what the library call writes
    r = subprocess.run([os.path.join(PKG, "pgx_image"), "--info", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("section ")]
    assert [(ln[1], int(ln[3]), int(ln[5]), int(ln[7], 16)) for ln in lines] == [(s["name"], s["bytes"], s["offset"], s["sum"]) for s in f.sections]
    strict = str(tmp_path / "strict_nl.pgi")
    r = subprocess.run([os.path.join(PKG, "pgx_image"), x_index[0], "-", strict, "--mode", "strict", "--no-locate", "--image", "rl"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = E.ImageFile(open(strict, "rb").read())
    assert g.mode == P.MODE_STRICT and g.has_tags == 0 and g.n_sections == 13 and not g.by_name("pairs")["bytes"] and g.by_name("blow")["bytes"]
    assert subprocess.run([os.path.join(PKG, "pgx_image"), "--info", x_index[0]], capture_output=True).returncode == 1
    assert subprocess.run([os.path.join(PKG, "pgx_image"), x_index[0], x_index[1], out, "--bogus"], capture_output=True).returncode == 1
    # find_mems / query_tags refuse before any device is touched: the tags positional must be "-", --mode may only repeat the image's
    reads = str(tmp_path / "reads.txt")
    with open(reads, "w") as fh:
        fh.write("ACGTACGTACGTACGTACGT\n")
    for tool, tail in (("find_mems", [reads, "10", "1"]), ("query_tags", [reads])):
        r = subprocess.run([os.path.join(PKG, tool), out, x_index[1]] + tail, capture_output=True, text=True)
        assert r.returncode == 1 and "tags argument must be" in r.stderr, (tool, r.stderr)
        r = subprocess.run([os.path.join(PKG, tool), out, "-"] + tail + ["--mode", "strict"], capture_output=True, text=True)
        assert r.returncode == 1 and "compat" in r.stderr, (tool, r.stderr)
