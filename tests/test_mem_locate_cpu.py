"""CPU tier of pgx_batch_locate: the ABI (symbols, version 6), no CPU fallback, the CLI's checks of --locate / --locate-max before
any device is opened, and the output lines of tests/locate_format.py on hand-made results."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pgx_ffi as P
from locate_format import locate_lines, mem_locate_lines, splice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")


def test_symbols_and_abi_version(built):
    L = ctypes.CDLL(P.LIB_PATH)
    for n in ("pgx_batch_locate", "pgx_batch_locations", "pgx_batch_device_locations"):
        assert hasattr(L, n), n
    assert P.lib().pgx_abi_version() == 7
    assert ctypes.sizeof(P.Locations) == 56  # pgx_locations: 3 x u64, 2 x u32, 2 pointers, 2 floats


def _no_gpu():
    try:
        return P.device_count() == 0
    except P.PgxError as e:
        return e.code == P.ERR_NO_DEVICE


def test_locate_without_device(built):
    if not _no_gpu():
        pytest.skip("a GPU is present")
    L = P.lib()
    assert L.pgx_batch_locate(None, 0, 0, None) == P.ERR_NO_DEVICE
    assert b"no CPU fallback" in L.pgx_last_error()
    out = P.Locations()
    assert L.pgx_batch_locations(None, ctypes.byref(out)) == P.ERR_ARG
    assert L.pgx_batch_device_locations(None, ctypes.byref(out)) == P.ERR_ARG


@pytest.mark.parametrize("args,msg", [(["--locate", "bogus"], "--locate: positions or seqs"), (["--locate-max", "-1"], "--locate-max"),
                                      (["--locate", "seqs", "--locate-max", "-1"], "--locate-max"),
                                      (["--locate", "positions", "--locate-max", "1e3"], "--locate-max"), (["--locate"], "missing value"),
                                      (["--locate-max", "5"], "--locate-max needs --locate")])
def test_cli_rejects_bad_locate_options(built, args, msg):
    # the index and reads do not exist: the options are checked before anything is opened
    r = subprocess.run([CLI, "no.ri", "no.tags", "no.txt", "10", "1"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr, r.stderr
    assert "Reading the rindex file" not in r.stderr


def test_locate_lines_hand_made():
    ml = 1000
    assert locate_lines(3, np.array([2 * ml + 5, 7, 2 * ml + 5], np.uint64), "positions", ml) == "Occurrences: 3\n2:5, 0:7, 2:5, \n"
    assert locate_lines(3, np.array([0, 2], np.uint64), "seqs", ml) == "Sequences: 2\n0, 2, \n"
    for mode in ("positions", "seqs"):
        assert locate_lines(40, np.zeros(0, np.uint64), mode, ml) == "Occurrences: 40 (not located)\n\n"


def test_splice_hand_made():
    text = ("Seq: 1\nMEM START: 0, MEM END: 4 BWT START: 10 SIZE: 2\nNumber of unique positions: 1\n5, \n"
            "MEM START: 3, MEM END: 9 BWT START: 2 SIZE: 1\nNumber of unique positions: 0\n\n\nSeq: 2\n\n")
    mems = np.zeros(2, P.MEM_DTYPE)
    mems["size"] = [2, 1]
    per = mem_locate_lines(mems, np.array([0, 2, 3], np.uint64), np.array([3 * 100 + 1, 4, 1 * 100 + 9], np.uint64), "positions", 100)
    assert per == ["Occurrences: 2\n3:1, 0:4, \n", "Occurrences: 1\n1:9, \n"]
    got = splice(text, per)
    assert got == ("Seq: 1\nMEM START: 0, MEM END: 4 BWT START: 10 SIZE: 2\nNumber of unique positions: 1\n5, \nOccurrences: 2\n3:1, 0:4, \n"
                   "MEM START: 3, MEM END: 9 BWT START: 2 SIZE: 1\nNumber of unique positions: 0\n\nOccurrences: 1\n1:9, \n\nSeq: 2\n\n")
    # the second MEM over the cap: an empty line stands for its values
    per = mem_locate_lines(mems, np.array([0, 1, 1], np.uint64), np.array([4], np.uint64), "seqs", 100)
    assert per == ["Sequences: 1\n4, \n", "Occurrences: 1 (not located)\n\n"]
    assert "Number of unique positions: 0\n\nOccurrences: 1 (not located)\n\n\nSeq: 2\n" in splice(text, per)
    with pytest.raises(AssertionError):
        splice(text, per[:1])
