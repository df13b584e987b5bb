"""CPU tier of the read placement: the ABI (exported symbols, the layout of pgx_read_place, pgx_placement and pgx_read_places, the
constant, the version that stays), no CPU fallback, the emulator of tests/place_emu.py against a second, sweep-style formulation of the
definitions, and the option checks of the find_mems CLI that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as G
import pgx_ffi as P
import place_emu as E

CLI = os.path.join(G.ROOT, "pangenome-index_amd", "find_mems")
ENTRY_POINTS = ("pgx_batch_read_place", "pgx_batch_places", "pgx_batch_device_places", "pgx_read_place_arrays")


def _header():
    with open(os.path.join(G.ROOT, "include", "pgx.h")) as f:
        return f.read()


def test_symbols_are_exported(built):
    L = P.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name


def test_abi_version_stays(built):
    assert P.lib().pgx_abi_version() == 7 == G.header_abi_version()


def test_constant_equals_the_header():
    m = re.search(r"^#define\s+PGX_PLACE_LIST\s+(\d+)u", _header(), re.M)
    assert m and int(m.group(1)) == P.PLACE_LIST == 1


def test_record_layouts():
    d = P.READ_PLACE_DTYPE
    assert d.itemsize == 64 == ctypes.sizeof(P.ReadPlace) and d == E.READ_PLACE_DTYPE
    want = dict(best_score=0, next_score=8, best_diag=16, n_anchors=24, n_placements=32, best_seq=40, n_best=44, best_mems=48, n_located=52, n_mems=56,
                reserved=60)
    assert {n: d.fields[n][1] for n in d.names} == want
    assert {n: getattr(P.ReadPlace, n).offset for n, _ in P.ReadPlace._fields_} == want
    assert re.search(r"uint64_t\s+best_score,\s*next_score;\s*int64_t\s+best_diag;\s*uint64_t\s+n_anchors,\s*n_placements;\s*uint32_t\s+best_seq,\s*n_best,"
                     r"\s*best_mems,\s*n_located,\s*n_mems,\s*reserved;\s*\}\s*pgx_read_place;", _header())
    d = P.PLACEMENT_DTYPE
    assert d.itemsize == 24 == ctypes.sizeof(P.Placement) and d == E.PLACEMENT_DTYPE
    want = dict(diag=0, score=8, seq=16, mems=20)
    assert {n: d.fields[n][1] for n in d.names} == want
    assert {n: getattr(P.Placement, n).offset for n, _ in P.Placement._fields_} == want
    assert ctypes.sizeof(P.ReadPlaces) == 64
    offs = {n: getattr(P.ReadPlaces, n).offset for n, _ in P.ReadPlaces._fields_}
    assert offs == dict(n_reads=0, n_anchors=8, n_places=16, flags=24, n_passes=28, reads=32, place_offsets=40, places=48, ms_place=56, reserved=60)


def _no_gpu():
    try:
        return P.device_count() == 0
    except P.PgxError as e:
        return e.code == P.ERR_NO_DEVICE


def test_no_device(built):
    if not _no_gpu():
        pytest.skip("a GPU is present")
    L = P.lib()
    assert L.pgx_batch_read_place(None, 0, None) == P.ERR_NO_DEVICE
    assert b"no CPU fallback" in L.pgx_last_error()
    with pytest.raises(P.PgxError) as e:
        P.read_place_arrays(0, np.zeros(2, np.uint64), np.zeros(0, P.MEM_DTYPE), np.zeros(1, np.uint64), np.zeros(0, np.uint64), 3, 100)
    assert e.value.code == P.ERR_NO_DEVICE
    out = P.ReadPlaces()
    assert L.pgx_batch_places(None, ctypes.byref(out)) == P.ERR_ARG
    assert L.pgx_batch_device_places(None, ctypes.byref(out)) == P.ERR_ARG


def _sweep_place(mem_offsets, mems, loc_offsets, values, L):
    """the second formulation: per read the anchors as (seq, diag, start, end) tuples, sorted; a placement is a run of equal (seq, diag)
    whose intervals are merged into disjoint runs with a running reach (plain Python integers)"""
    n = len(mem_offsets) - 1
    recs = np.zeros(n, E.READ_PLACE_DTYPE)
    offs, places = [0], []
    for r in range(n):
        anchors, located, n_anchors = set(), 0, 0
        for m in range(int(mem_offsets[r]), int(mem_offsets[r + 1])):
            vs = [int(v) for v in values[int(loc_offsets[m]):int(loc_offsets[m + 1])]]
            located += bool(vs)
            n_anchors += len(vs)
            s, e = int(mems["start"][m]), int(mems["end"][m])
            anchors |= {(v // L, v % L - s, s, e) for v in vs}
        mine = []
        for a in sorted(anchors):
            if not mine or tuple(mine[-1][:2]) != a[:2]:
                mine.append([a[0], a[1], 0, 0, 0])  # seq, diag, score, mems, reach
            p = mine[-1]
            if a[3] > max(a[2], p[4]):
                p[2] += a[3] - max(a[2], p[4])
            p[4] = max(p[4], a[3])
            p[3] += 1
        best = max([p[2] for p in mine] + [0])
        ties = [p for p in mine if p[2] == best and best > 0]
        below = [p[2] for p in mine if p[2] < best]
        f = ties[0] if ties else [E.NO_SEQUENCE, 0, 0, 0]
        recs[r] = (best, max(below) if below and best > 0 else 0, f[1], n_anchors, len(mine), f[0], len(ties), f[3], located,
                   int(mem_offsets[r + 1]) - int(mem_offsets[r]), 0)
        places += [(p[1], p[2], p[0], p[3]) for p in mine]
        offs.append(len(places))
    return dict(reads=recs, place_offsets=np.asarray(offs, np.uint64), places=np.array(places, dtype=E.PLACEMENT_DTYPE))


@pytest.mark.parametrize("n_seq,max_length", [(1, 100), (2, 64), (65, 1000), (5000, 1 << 20)])
def test_emulator_agrees_with_the_sweep_formulation(n_seq, max_length):
    rng = np.random.default_rng(n_seq)
    for big in (False, True):
        case = E.random_case(rng, 60, n_seq, max_length, big=big)
        a, b = E.read_place(*case, max_length), _sweep_place(*case, max_length)
        assert a["reads"].tobytes() == b["reads"].tobytes(), (a["reads"], b["reads"])
        assert np.array_equal(a["place_offsets"], b["place_offsets"]) and a["places"].tobytes() == b["places"].tobytes()
    assert (a["reads"]["best_score"] > 0).any() and (a["reads"]["n_placements"] > 1).any()


def test_emulator_by_hand():
    L = 100
    # read 0: [0, 10) at 1:40 and 0:5; [5, 20) at 1:45 (the diagonal 40 of sequence 1 again) and 1:2 (diagonal -3); [7, 9) at 0:12 (diagonal 5 of
    # sequence 0 again, nested); [30, 30) at 1:70 (empty: a placement without a score... on diagonal 40, which has one).  read 1: no MEM.
    # read 2: one MEM without a value.
    reads = [[(0, 10, [(1, 40), (0, 5)]), (5, 20, [(1, 45), (1, 2)]), (7, 9, [(0, 12)]), (30, 30, [(1, 70)])], [], [(4, 8, [])]]
    mem_offsets, mems, loc_offsets, packed = E.build_case(reads)
    got = E.read_place(mem_offsets, mems, loc_offsets, packed(L), L)
    assert got["places"].tolist() == [(5, 10, 0, 2), (-3, 15, 1, 1), (40, 20, 1, 3)]
    assert got["place_offsets"].tolist() == [0, 3, 3, 3]
    assert got["reads"].tolist() == [(20, 15, 40, 6, 3, 1, 1, 3, 4, 4, 0), (0, 0, 0, 0, 0, E.NO_SEQUENCE, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, E.NO_SEQUENCE, 0, 0, 0, 1, 0)]
    assert E.place_text(got["reads"], first_seq=5) == (E.HEADER + b"6\t4\t4\t6\t3\t20\t1\t1\t40\t3\t15\n" + b"7\t0\t0\t0\t0\t0\t0\t*\t*\t0\t0\n" +
                                                        b"8\t1\t0\t0\t0\t0\t0\t*\t*\t0\t0\n")


@pytest.mark.parametrize("extra", [["--place-only"], ["--place-max", "5"], ["--place-only", "--place-max", "5"]])
def test_cli_refuses_place_options_without_place(built, extra):
    # decided from the arguments alone, before any file is opened
    r = subprocess.run([CLI, "no.ri", "no.tags", "no_reads.txt", "5", "1"] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.startswith("usage: find_mems") and "--place FILE" in r.stderr


@pytest.mark.parametrize("locate", [["--locate", "seqs"], ["--locate", "positions", "--locate-max", "3"]])
def test_cli_refuses_place_only_with_locate(built, locate):
    # --place-only makes no MEM text, so there is nothing the located values could be printed in: refused, not ignored
    r = subprocess.run([CLI, "no.ri", "no.tags", "no_reads.txt", "5", "1", "--place", "no_place.tsv", "--place-only"] + locate, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "--place-only" in r.stderr and "--locate" in r.stderr
    assert not os.path.exists("no_place.tsv")
