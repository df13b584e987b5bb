"""CPU tier of the device text output (pgx_batch_format, pgx_format_result): the Python statement of the grammar (tests/text_emu.py)
against the committed goldens, the binding's struct sizes, the exported symbols, and what the two calls answer without a device:
the argument errors pgx_format_result decides before it touches one, PGX_ERR_NO_DEVICE otherwise."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import text_emu as T


@pytest.mark.parametrize("name", ["reads_3_1", "reads_5_1", "test_reads_3_1"])
def test_emulator_reproduces_committed_goldens(name):
    exp = open(os.path.join(O.GOLDEN, "expected_find_mems_xy_%s.txt" % name)).read()
    res, first_seq = T.parse(exp)
    assert first_seq == 0 and len(res["mem_offsets"]) > 5 and len(res["mems"]) > 0 and len(res["positions"]) > 0
    text, err, offs = T.emit(res)
    assert text.decode() == exp
    assert offs[0] == 0 and offs[-1] == len(text) and len(offs) == len(res["mem_offsets"])
    for i in (0, len(offs) // 2, len(offs) - 2):  # a read's span starts at its header and ends behind its empty line
        piece = text[int(offs[i]):int(offs[i + 1])]
        assert piece.startswith(b"Seq: %d\n" % (i + 1)) and piece.endswith(b"\n") and b"Seq: " not in piece[5:]
    assert err.count(b"\n") == len(offs) - 1 and err.startswith(b"[find_all_mems] total mems=%d\n" % int(res["mem_offsets"][1]))


def test_emulator_forms():
    """every line form once, by hand"""
    res = dict(mem_offsets=np.array([0, 0, 2], dtype=np.uint64), mems=np.array([(1, 2, 3, -4), (5, 6, 7, 8)], dtype=T.MEM_DTYPE),
               pos_offsets=np.array([0, 0, 2], dtype=np.uint64), positions=np.array([10, 2 ** 64 - 1], dtype=np.uint64))
    loc = dict(loc_offsets=np.array([0, 0, 2], dtype=np.uint64), values=np.array([2006, 5], dtype=np.uint64))
    head = "Seq: 100\n\nSeq: 101\nMEM START: 1, MEM END: 2 BWT START: 3 SIZE: -4\nNumber of unique positions: 0\n\n"
    mem2 = "MEM START: 5, MEM END: 6 BWT START: 7 SIZE: 8\nNumber of unique positions: 2\n10, 18446744073709551615, \n"
    text, err, offs = T.emit(res, first_seq=99)
    assert text.decode() == head + mem2 + "\n" and err == b"[find_all_mems] total mems=0\n[find_all_mems] total mems=2\n" and list(offs) == [0, 10, len(text)]
    text, _, _ = T.emit(res, first_seq=99, locate=T.LOCATE_POSITIONS, locations=loc, max_length=1003)
    assert text.decode() == head + "Occurrences: -4 (not located)\n\n" + mem2 + "Occurrences: 8\n2:0, 0:5, \n\n"
    text, _, _ = T.emit(res, first_seq=99, locate=T.LOCATE_SEQS, locations=loc)
    assert text.decode() == head + "Occurrences: -4 (not located)\n\n" + mem2 + "Sequences: 2\n2006, 5, \n\n"
    back, first_seq = T.parse(T.emit(res, first_seq=99)[0].decode())
    assert first_seq == 99 and back["mems"].tobytes() == res["mems"].tobytes() and np.array_equal(back["positions"], res["positions"])


def test_binding_struct_sizes_and_symbols(built):
    assert C.sizeof(P.FormatParams) == 24 and C.sizeof(P.Text) == 56
    assert P.FormatParams.flags.offset == 16 and P.Text.read_offsets.offset == 24 and P.Text.ms_format.offset == 48
    assert (P.FORMAT_STDERR, P.FORMAT_LOCATE_POSITIONS, P.FORMAT_LOCATE_SEQS) == (1, 2, 4)
    L = P.lib()
    assert hasattr(L, "pgx_batch_format") and hasattr(L, "pgx_format_result")
    assert L.pgx_abi_version() == 7
    hdr = open(os.path.join(P.ROOT, "include", "pgx.h")).read()
    for word in ("pgx_batch_format", "pgx_format_result", "pgx_format_params", "pgx_text", "PGX_FORMAT_STDERR 1u", "PGX_FORMAT_LOCATE_POSITIONS 2u",
                 "PGX_FORMAT_LOCATE_SEQS 4u", "no chunked mode"):
        assert word in hdr, word


def _small():
    res = dict(mem_offsets=np.array([0, 1, 2], dtype=np.uint64), mems=np.zeros(2, dtype=P.MEM_DTYPE),
               pos_offsets=np.array([0, 1, 3], dtype=np.uint64), positions=np.array([7, 8, 9], dtype=np.uint64))
    loc = dict(loc_offsets=np.array([0, 1, 2], dtype=np.uint64), values=np.array([1, 2], dtype=np.uint64))
    return res, loc


def _code(fn):
    with pytest.raises(P.PgxError) as e:
        fn()
    return e.value.code


def test_format_result_argument_errors_need_no_device(built):
    """decided from the arguments alone: the same answer with and without a GPU"""
    res, loc = _small()
    for key, bad in (("mem_offsets", [1, 1, 2]), ("mem_offsets", [0, 2, 1]), ("mem_offsets", [0, 1, 1]), ("mem_offsets", [0, 1, 3]),
                     ("pos_offsets", [1, 1, 3]), ("pos_offsets", [0, 3, 2]), ("pos_offsets", [0, 1, 2]), ("pos_offsets", [0, 1, 4])):
        r = dict(res)
        r[key] = np.array(bad, dtype=np.uint64)
        assert _code(lambda: P.format_result(0, r, text_cap=1 << 12, err_cap=1 << 12)) == P.ERR_ARG, (key, bad)
        assert b"must start at 0" in P.lib().pgx_last_error()
    for bad in ([1, 1, 2], [0, 2, 1], [0, 1, 1], [0, 1, 3]):
        l = dict(loc, loc_offsets=np.array(bad, dtype=np.uint64))
        assert _code(lambda: P.format_result(0, res, flags=P.FORMAT_LOCATE_SEQS, locations=l, text_cap=1 << 12, err_cap=1 << 12)) == P.ERR_ARG, bad
    both = P.FORMAT_LOCATE_POSITIONS | P.FORMAT_LOCATE_SEQS
    assert _code(lambda: P.format_result(0, res, flags=both, locations=loc, max_length=10, text_cap=1 << 12, err_cap=1 << 12)) == P.ERR_ARG
    assert b"exclude each other" in P.lib().pgx_last_error()
    assert _code(lambda: P.format_result(0, res, flags=P.FORMAT_LOCATE_SEQS, text_cap=1 << 12, err_cap=1 << 12)) == P.ERR_ARG  # no loc
    assert _code(lambda: P.format_result(0, res, flags=P.FORMAT_LOCATE_POSITIONS, locations=loc, max_length=0, text_cap=1 << 12, err_cap=1 << 12)) == P.ERR_ARG
    assert _code(lambda: P.format_result(0, res, flags=8, text_cap=1 << 12, err_cap=1 << 12)) == P.ERR_ARG
    assert _code(lambda: P.format_result(0, res, reserved=1, text_cap=1 << 12, err_cap=1 << 12)) == P.ERR_ARG
    untagged = dict(mem_offsets=res["mem_offsets"], mems=res["mems"])
    assert _code(lambda: P.format_result(0, untagged, text_cap=1 << 12, err_cap=1 << 12)) == P.ERR_ARG
    l = dict(loc, n_mems=3)
    assert _code(lambda: P.format_result(0, res, flags=P.FORMAT_LOCATE_SEQS, locations=l, text_cap=1 << 12, err_cap=1 << 12)) == P.ERR_ARG


def _no_gpu():
    try:
        return P.device_count() == 0
    except P.PgxError as e:
        return e.code == P.ERR_NO_DEVICE


def test_no_device(built):
    if not _no_gpu():
        return  # (with a GPU the two entry points are what tests/test_gpu_format.py runs)
    L = P.lib()
    fp, t = P.FormatParams(0, 0, 0, 0), P.Text()
    assert L.pgx_batch_format(None, C.byref(fp), C.byref(t)) == P.ERR_NO_DEVICE and b"no CPU fallback" in L.pgx_last_error()
    res, loc = _small()
    assert _code(lambda: P.format_result(0, res, flags=P.FORMAT_STDERR, text_cap=1 << 12, err_cap=1 << 12)) == P.ERR_NO_DEVICE
    assert _code(lambda: P.format_result(0, res, flags=P.FORMAT_LOCATE_POSITIONS, locations=loc, max_length=7)) == P.ERR_NO_DEVICE
