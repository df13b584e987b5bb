"""CPU tier of the device index build (pgx_build_index_from_text[s]_device): what it answers without a device, the --text form of the
build_rindex CLI, and the case tables of the GPU tier (build_device_cases.py): that they hold the borders they claim, and that the
order rule they state is the CPU builder's (a BWT from a naive sorted() over the suffixes equals the builder's file)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import build_device_cases as BC
import oracle_ffi as O
import pgx_ffi as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pangenome-index_amd")
G = O.GOLDEN


def _has_device():
    n = ctypes.c_int(0)
    return P.lib().pgx_device_count(ctypes.byref(n)) == P.OK and n.value > 0


def test_without_a_device_and_bad_arguments(built, tmp_path):
    L = P.lib()
    text = os.path.join(G, "x.newline_separated").encode()
    rl, ri = str(tmp_path / "x.rl_bwt").encode(), str(tmp_path / "x.ri").encode()
    arr = (ctypes.c_char_p * 1)(text)
    # arguments are checked before the device is looked for
    assert L.pgx_build_index_from_text_device(None, rl, ri, 1, 0) == P.ERR_ARG
    assert L.pgx_build_index_from_text_device(text, rl, None, 1, 0) == P.ERR_ARG
    assert L.pgx_build_index_from_texts_device(None, 1, rl, ri, 1, 0) == P.ERR_ARG
    assert L.pgx_build_index_from_texts_device(arr, 0, rl, ri, 1, 0) == P.ERR_ARG
    assert L.pgx_build_index_from_texts_device((ctypes.c_char_p * 2)(text, None), 2, rl, ri, 1, 0) == P.ERR_ARG
    assert L.pgx_build_index_from_texts_device(arr, 1, rl, None, 1, 0) == P.ERR_ARG
    assert L.pgx_build_index_device_timing(None, 6) == P.ERR_ARG
    assert not os.path.exists(rl) and not os.path.exists(ri)
    if not _has_device():
        assert L.pgx_build_index_from_text_device(text, rl, ri, 1, 0) == P.ERR_NO_DEVICE
        assert b"no usable HIP device" in L.pgx_last_error()
        assert L.pgx_build_index_from_texts_device(arr, 1, rl, ri, 1, 0) == P.ERR_NO_DEVICE
        with pytest.raises(P.PgxError) as e:
            P.build_index_from_text_device(text.decode(), rl.decode(), ri.decode())
        assert e.value.code == P.ERR_NO_DEVICE
        with pytest.raises(P.PgxError) as e:
            P.build_index_from_texts_device([text.decode()], None, ri.decode())
        assert e.value.code == P.ERR_NO_DEVICE
        assert not os.path.exists(rl) and not os.path.exists(ri)
    t = P.build_index_device_timing()
    assert tuple(t) == P.BUILD_INDEX_DEVICE_STAGES and len(t) == 6


def test_cli_text_form_fails_with_the_message_and_the_reference_form_is_unchanged(built, tmp_path):
    exe = os.path.join(BIN, "build_rindex")
    if not _has_device():
        r = subprocess.run([exe, "--text", os.path.join(G, "x.newline_separated"), "--rlbwt", str(tmp_path / "x.rl_bwt")], capture_output=True, timeout=120)
        assert r.returncode == 1 and r.stdout == b"" and b"no usable HIP device" in r.stderr
        assert not os.path.exists(str(tmp_path / "x.rl_bwt"))
    r = subprocess.run([exe, "--text"], capture_output=True, timeout=120)
    assert r.returncode == 1 and r.stdout == b"" and b"usage: build_rindex --text" in r.stderr
    r = subprocess.run([exe, "--text", os.path.join(G, "x.newline_separated"), "--rlbwt"], capture_output=True, timeout=120)
    assert r.returncode == 1 and r.stdout == b"" and b"option" in r.stderr
    r = subprocess.run([exe, "--text", os.path.join(G, "x.newline_separated"), "--frobnicate"], capture_output=True, timeout=120)
    assert r.returncode == 1 and r.stdout == b""
    # the reference form: .rl_bwt -> .ri on stdout, as before
    ref = str(tmp_path / "x.ri")
    P.build_rindex(os.path.join(G, "x.rl_bwt"), ref, encoded=True)
    r = subprocess.run([exe, os.path.join(G, "x.rl_bwt")], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == open(ref, "rb").read()
    bt = os.path.join(G, "bidirectional_test")
    r = subprocess.run([exe, os.path.join(bt, "contigs_xy.rl_bwt"), "--legacy"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == open(os.path.join(bt, "xy.ri"), "rb").read()


def test_constants_are_the_kernels():
    import re

    src = open(os.path.join(BIN, "csrc", "pgx_device.h")).read()
    for name, value in (("PGX_SA_K", BC.SA_K), ("PGX_SA_TILE", BC.SA_TILE), ("PGX_SA_SORT_TILE", BC.SA_SORT_TILE), ("PGX_SCAN1_TILE_ITEMS", BC.SCAN1_TILE_ITEMS)):
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, src, re.M)
        assert m and int(m.group(1)) == value, name


def test_depth_tables_hold_their_depths():
    want = set(range(71))
    for k in range(7, 13):
        want |= {2 ** k - 1, 2 ** k, 2 ** k + 1}
    for k in range(9):
        want |= {BC.SA_K * 2 ** k - 1, BC.SA_K * 2 ** k, BC.SA_K * 2 ** k + 1}
    assert set(BC.DEPTHS) == want
    for L in BC.DEPTHS:
        text = BC.depth_text(L)
        assert 2 <= text.count(b"\n") <= 4 and text.endswith(b"\n")
        assert L in BC.neighbour_lcps(text), L


def test_tie_size_and_group_tables_hold_their_borders():
    ties = BC.tie_texts()
    for c in (2, 3, 255, 256, 257, 1000):
        t = ties["identical_%d" % c]
        seqs = t.split(b"\n")[:-1]
        assert len(seqs) == c and len(set(seqs)) == 1
    seqs = ties["proper_suffix"].split(b"\n")[:-1]
    assert any(a != b and a.endswith(b) for a in seqs for b in seqs)
    assert ties["empty_sequences"] == b"\n\n\n" and ties["single_newline"] == b"\n"
    assert ties["single_sequence"].count(b"\n") == 1 and not ties["no_final_newline"].endswith(b"\n")
    # identical sequences: every group of equal suffixes is ordered by the endmarkers alone
    order, _ = BC.naive_suffix_order(ties["identical_3"])
    assert list(order[:3]) == [7, 15, 23] and list(order[3:6]) == [6, 14, 22]
    totals = set()
    for name, (n, n_seq, _) in BC.SIZE_CASES.items():
        t = BC.size_text(name)
        assert len(t) == n and t.count(b"\n") == n_seq and t.endswith(b"\n") and b"N" in t
        totals.add(n)
    for border in (256, BC.SA_TILE, BC.SA_SORT_TILE, 2 * BC.SA_SORT_TILE, 65536):
        assert {border - 1, border, border + 1} <= totals
    assert 16 * BC.SA_SORT_TILE == 65536 and 256 * 16 == BC.SCAN1_TILE_ITEMS  # the scan tile of the histogram table falls on the same total
    t = BC.many_sequences_text()
    assert len(t) == 3 * 65536 + 1 and t[:2 * 65537].count(b"\n") == 65537 and t.count(b"\n") == 65538 > 1 << 16
    t = BC.large_groups_text()
    assert len(t) == 20000 and b"A" * 5000 in t and b"N" * 3000 in t and b"ACG" * 2000 in t
    lcps = BC.neighbour_lcps(t)
    assert max(lcps) >= 5997 and sum(1 for v in lcps if v >= 1000) >= 8000  # (ACG)^2000 against itself three symbols on; groups of thousands past a dozen rounds
    for seed in range(300):
        t = BC.sweep_text(seed)
        assert 2 <= len(t) <= 5000 and 1 <= t.count(b"\n") <= 40 and t.endswith(b"\n")
    assert len({BC.sweep_text(s) for s in range(300)}) == 300


@pytest.mark.parametrize("which", ["depth_33", "identical_257", "n_4097"])
def test_cpu_builder_follows_the_naive_order(built, tmp_path, which):
    """pins the order rule independently of SA-IS: the .rl_bwt of the CPU builder equals the BWT of the naive order"""
    text = {"depth_33": lambda: BC.depth_text(33), "identical_257": lambda: BC.tie_texts()["identical_257"], "n_4097": lambda: BC.size_text("n_4097")}[which]()
    src, rl, ri = str(tmp_path / "t.txt"), str(tmp_path / "t.rl_bwt"), str(tmp_path / "t.ri")
    open(src, "wb").write(text)
    P.build_index_from_text(src, rl, ri, encoded=True)
    assert open(rl, "rb").read() == BC.rlbwt_bytes(BC.naive_bwt_runs(text))
