"""The device encoder of tag query files, as far as it goes without a GPU: the exported symbols and their binding, the new constants
(header against binding), the ABI version, every argument error that is raised before a device is touched, and the CLI's refusal of
an unknown --format."""
import ctypes as C
import os
import re
import subprocess

import pgx_ffi as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pangenome-index_amd")


def test_symbols_exported_and_bound(built):
    L = P.lib()
    for name in ("pgx_tags_encode", "pgx_tags_encode_timing"):
        assert getattr(L, name).argtypes is not None, name
    assert callable(P.tags_encode) and callable(P.tags_encode_timing)
    assert set(P.tags_encode_timing()) == set(P.TAGS_ENCODE_STAGES)
    assert P.TAGS_ENCODE_STAGES[:5] == ("pieces", "sd_vectors", "select", "download", "write")
    assert L.pgx_abi_version() == 7


def test_constants_match_the_header(built):
    h = open(os.path.join(ROOT, "include", "pgx.h")).read()
    for name, value in (("PGX_BUILD_TAGS_OUT_COMPACT", P.BUILD_TAGS_OUT_COMPACT), ("PGX_BUILD_TAGS_OUT_BYTECODE", P.BUILD_TAGS_OUT_BYTECODE),
                        ("PGX_MERGE_DEVICE_ENCODE", P.MERGE_DEVICE_ENCODE), ("PGX_TAGS_COMPACT", P.TAGS_COMPACT), ("PGX_TAGS_BYTECODE", P.TAGS_BYTECODE)):
        m = re.search(r"^#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)u\b" % name, h, re.M)
        assert m and int(m.group(1), 0) == value, name
    assert (P.BUILD_TAGS_OUT_COMPACT, P.BUILD_TAGS_OUT_BYTECODE, P.MERGE_DEVICE_ENCODE) == (0x8, 0x10, 0x10)


def test_argument_errors_before_any_device_use(built, tmp_path):
    L = P.lib()
    out = str(tmp_path / "never.tags")
    v = (C.c_uint64 * 2)(1 << 11, 2 << 11)
    ln = (C.c_uint64 * 2)(3, 4)
    pv, pl = C.cast(v, C.c_void_p), C.cast(ln, C.c_void_p)
    assert L.pgx_tags_encode(0, pv, pl, 2, 0, P.TAGS_COMPACT, None) == P.ERR_ARG
    for fmt in (P.TAGS_AUTO, 3, 0xFFFFFFFF):
        assert L.pgx_tags_encode(0, pv, pl, 2, 0, fmt, out.encode()) == P.ERR_ARG, fmt
        assert b"format" in L.pgx_last_error()
    assert L.pgx_tags_encode(0, None, pl, 2, 0, P.TAGS_COMPACT, out.encode()) == P.ERR_ARG
    assert L.pgx_tags_encode_timing(None, 5) == P.ERR_ARG
    both = P.BUILD_TAGS_OUT_COMPACT | P.BUILD_TAGS_OUT_BYTECODE
    for flags in (both, both | P.BUILD_TAGS_REFERENCE_RUNS, 0x20, 0x20 | P.BUILD_TAGS_OUT_COMPACT):
        assert L.pgx_build_tags(b"no.gbz", b"no.ri", 0, out.encode(), flags) == P.ERR_ARG, flags
        po = (C.c_uint64 * 1)(0)
        assert L.pgx_build_tags_paths(b"no.ri", 0, C.cast(po, C.c_void_p), None, None, 0, 0, 0, out.encode(), flags) == P.ERR_ARG, flags
    assert not os.path.exists(out)


def test_cli_refuses_an_unknown_format(built, tmp_path):
    out = str(tmp_path / "never.tags")
    for tail in (["--format", "bogus"], ["--format", "Compact"]):
        r = subprocess.run([os.path.join(BIN, "build_tags"), "no.gbz", "no.rl_bwt", out] + tail, capture_output=True, timeout=60)
        assert r.returncode == 1 and b"usage: build_tags" in r.stderr and b"--format algorithm|compact|bytecode" in r.stderr
        assert r.stdout == b"" and not os.path.exists(out)
