"""CPU tier of the read hits: the ABI (exported symbols, the layout of pgx_read_hit and pgx_read_hits, the constants, the version that
stays 7), no CPU fallback, the emulator of tests/hits_emu.py against a second formulation of the definitions, and the option checks of
the find_mems CLI that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as G
import hits_emu as E
import pgx_ffi as P

CLI = os.path.join(G.ROOT, "pangenome-index_amd", "find_mems")
ENTRY_POINTS = ("pgx_batch_read_hits", "pgx_batch_hits", "pgx_batch_device_hits", "pgx_read_hits_arrays")


def _header():
    with open(os.path.join(G.ROOT, "include", "pgx.h")) as f:
        return f.read()


def test_symbols_are_exported(built):
    L = P.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name


def test_abi_version_stays_7(built):
    assert P.lib().pgx_abi_version() == 7 == G.header_abi_version()
    assert "pgx_batch_read_hits" in re.search(r"^#define\s+PGX_ABI_VERSION\s+7\s*/\*(.*?)\*/", _header(), re.M | re.S).group(1)


def test_constants_equal_the_header():
    h = _header()
    for name, val in (("PGX_HITS_BEST_SETS", P.HITS_BEST_SETS), ("PGX_HITS_SCORES", P.HITS_SCORES)):
        m = re.search(r"^#define\s+%s\s+(\d+)u" % name, h, re.M)
        assert m and int(m.group(1)) == val, name
    m = re.search(r"^#define\s+PGX_NO_SEQUENCE\s+0x([0-9A-Fa-f]+)u", h, re.M)
    assert m and int(m.group(1), 16) == P.NO_SEQUENCE == E.NO_SEQUENCE == 0xFFFFFFFF
    assert (P.HITS_BEST_SETS, P.HITS_SCORES) == (1, 2)


def test_read_hit_layout():
    d = P.READ_HIT_DTYPE
    assert d.itemsize == 40 and d == E.HIT_DTYPE
    assert {n: d.fields[n][1] for n in d.names} == dict(best_score=0, next_score=8, covered=16, best_seq=24, n_best=28, n_located=32, n_mems=36)
    assert re.search(r"uint64_t\s+best_score,\s*next_score,\s*covered;\s*uint32_t\s+best_seq,\s*n_best,\s*n_located,\s*n_mems;\s*\}\s*pgx_read_hit;", _header())
    assert ctypes.sizeof(P.ReadHits) == 56
    offs = {n: getattr(P.ReadHits, n).offset for n, _ in P.ReadHits._fields_}
    assert offs == dict(n_reads=0, n_seq=8, set_words=16, flags=20, hits=24, best_sets=32, scores=40, ms_hits=48, reserved=52)


def _no_gpu():
    try:
        return P.device_count() == 0
    except P.PgxError as e:
        return e.code == P.ERR_NO_DEVICE


def test_no_device(built):
    if not _no_gpu():
        pytest.skip("a GPU is present")
    L = P.lib()
    assert L.pgx_batch_read_hits(None, 0, None) == P.ERR_NO_DEVICE
    assert b"no CPU fallback" in L.pgx_last_error()
    with pytest.raises(P.PgxError) as e:
        P.read_hits_arrays(0, np.zeros(2, np.uint64), np.zeros(0, P.MEM_DTYPE), np.zeros((0, 1), np.uint64), 3)
    assert e.value.code == P.ERR_NO_DEVICE
    out = P.ReadHits()
    assert L.pgx_batch_hits(None, ctypes.byref(out)) == P.ERR_ARG
    assert L.pgx_batch_device_hits(None, ctypes.byref(out)) == P.ERR_ARG


def _sweep_hits(mem_offsets, mems, sets, n_seq):
    """the second formulation: per sequence, the MEMs that have its bit sorted by start and merged into disjoint runs, whose lengths add
    up (plain Python integers)"""
    n, w = len(mem_offsets) - 1, (n_seq + 63) // 64
    hits = np.zeros(n, E.HIT_DTYPE)
    scores = np.zeros((n, n_seq), np.uint32)
    best_sets = np.zeros((n, w), np.uint64)

    def union(ivs):
        total, reach = 0, 0
        for a, b in sorted(ivs):
            if b > max(a, reach):
                total += b - max(a, reach)
            reach = max(reach, b)
        return total

    for r in range(n):
        ms = range(int(mem_offsets[r]), int(mem_offsets[r + 1]))
        has = lambda m, s: (int(sets[m][s >> 6]) >> (s & 63)) & 1
        iv = {m: (int(mems["start"][m]), int(mems["end"][m])) for m in ms}
        cov = [union([iv[m] for m in ms if has(m, s)]) for s in range(n_seq)]
        located = [m for m in ms if any(has(m, s) for s in range(n_seq))]
        best = max(cov)
        ties = [s for s in range(n_seq) if cov[s] == best and best > 0]
        below = [c for c in cov if c < best]
        hits[r] = (best, max(below) if below and best > 0 else 0, union([iv[m] for m in located]), ties[0] if ties else E.NO_SEQUENCE, len(ties),
                   len(located), len(ms))
        scores[r] = [min(c, 0xFFFFFFFF) for c in cov]
        for s in ties:
            best_sets[r, s >> 6] |= np.uint64(1 << (s & 63))
    return dict(hits=hits, best_sets=best_sets, scores=scores)


@pytest.mark.parametrize("n_seq", [1, 63, 64, 65, 130])
def test_emulator_agrees_with_the_sweep_formulation(n_seq):
    rng = np.random.default_rng(n_seq)
    for big in (False, True):
        mem_offsets, mems, sets = E.random_case(rng, 12, n_seq, big=big)
        a, b = E.read_hits(mem_offsets, mems, sets, n_seq), _sweep_hits(mem_offsets, mems, sets, n_seq)
        assert a["hits"].tobytes() == b["hits"].tobytes(), (a["hits"], b["hits"])
        assert np.array_equal(a["scores"], b["scores"]) and np.array_equal(a["best_sets"], b["best_sets"])
    assert (a["hits"]["best_score"] > 0).any()


def test_emulator_by_hand():
    # read 0: MEMs [0, 10) in {0, 1}, [5, 20) in {1}, [7, 9) in {0, 2} (nested), [30, 30) in {2} (empty); read 1: no MEM; read 2: one MEM, not located
    mems = np.zeros(5, P.MEM_DTYPE)
    mems["start"], mems["end"] = [0, 5, 7, 30, 4], [10, 20, 9, 30, 8]
    sets = np.array([[0b011], [0b010], [0b101], [0b100], [0]], np.uint64)
    got = E.read_hits(np.array([0, 4, 4, 5], np.uint64), mems, sets, 3)
    assert got["scores"].tolist() == [[10, 20, 2], [0, 0, 0], [0, 0, 0]]
    assert got["hits"].tolist() == [(20, 10, 20, 1, 1, 4, 4), (0, 0, 0, E.NO_SEQUENCE, 0, 0, 0), (0, 0, 0, E.NO_SEQUENCE, 0, 0, 1)]
    assert got["best_sets"].tolist() == [[0b010], [0], [0]]
    assert E.hits_text(got["hits"], first_seq=5) == (E.HEADER + b"6\t4\t4\t20\t20\t1\t1\t10\n" + b"7\t0\t0\t0\t0\t0\t*\t0\n" + b"8\t1\t0\t0\t0\t0\t*\t0\n")


@pytest.mark.parametrize("extra", [["--hits-only"], ["--hits-max", "5"], ["--hits-only", "--hits-max", "5"]])
def test_cli_refuses_hits_options_without_hits(built, extra):
    # decided from the arguments alone, before any file is opened
    r = subprocess.run([CLI, "no.ri", "no.tags", "no_reads.txt", "5", "1"] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.startswith("usage: find_mems") and "--hits FILE" in r.stderr


@pytest.mark.parametrize("locate", [["--locate", "seqs"], ["--locate", "positions", "--locate-max", "3"]])
def test_cli_refuses_hits_only_with_locate(built, locate):
    # --hits-only makes no MEM text, so there is nothing the located values could be printed in: refused, not ignored
    r = subprocess.run([CLI, "no.ri", "no.tags", "no_reads.txt", "5", "1", "--hits", "no.tsv", "--hits-only"] + locate, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "--hits-only" in r.stderr and "--locate" in r.stderr
    assert not os.path.exists("no.tsv")
