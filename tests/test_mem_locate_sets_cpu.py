"""CPU tier of PGX_LOCATE_SEQ_SETS: the ABI (version, the layout of pgx_locations with set_words where `reserved` was), the flag
combinations pgx_batch_locate refuses, and no CPU fallback."""
import ctypes
import re

import pytest

import __graft_entry__ as G
import pgx_ffi as P


def _header():
    import os

    with open(os.path.join(G.ROOT, "include", "pgx.h")) as f:
        return f.read()


def test_abi_version_and_flag_values(built):
    assert P.lib().pgx_abi_version() == G.header_abi_version()
    h = _header()
    for name, val in (("PGX_LOCATE_SEQ_IDS", P.LOCATE_SEQ_IDS), ("PGX_LOCATE_UNIQUE", P.LOCATE_UNIQUE), ("PGX_LOCATE_CHAINS", P.LOCATE_CHAINS),
                      ("PGX_LOCATE_SEQ_SETS", P.LOCATE_SEQ_SETS)):
        m = re.search(r"^#define\s+%s\s+(\d+)u" % name, h, re.M)
        assert m and int(m.group(1)) == val, name
    assert P.LOCATE_SEQ_SETS == 8


def test_locations_layout():
    assert ctypes.sizeof(P.Locations) == 56
    offs = {n: getattr(P.Locations, n).offset for n, _ in P.Locations._fields_}
    assert offs == dict(n_mems=0, n_values=8, n_not_located=16, flags=24, resident=28, loc_offsets=32, values=40, ms_locate=48, set_words=52)
    assert P.Locations.set_words.size == 4
    assert not hasattr(P.Locations, "reserved")
    assert re.search(r"float\s+ms_locate;[^\n]*\n\s*uint32_t\s+set_words;[^\n]*\n\}\s*pgx_locations;", _header())


def _no_gpu():
    try:
        return P.device_count() == 0
    except P.PgxError as e:
        return e.code == P.ERR_NO_DEVICE


@pytest.mark.parametrize("flags", [P.LOCATE_SEQ_SETS | P.LOCATE_SEQ_IDS, P.LOCATE_SEQ_SETS | P.LOCATE_UNIQUE,
                                   P.LOCATE_SEQ_SETS | P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE, P.LOCATE_SEQ_SETS | P.LOCATE_UNIQUE | P.LOCATE_CHAINS])
def test_sets_with_ids_or_unique_is_an_arg_error(built, flags):
    # a contradiction in the call itself: refused with or without a device, before the batch is looked at
    L = P.lib()
    assert L.pgx_batch_locate(None, flags, 0, None) == P.ERR_ARG
    assert b"PGX_LOCATE_SEQ_SETS" in L.pgx_last_error()


@pytest.mark.parametrize("flags", [P.LOCATE_SEQ_SETS, P.LOCATE_SEQ_SETS | P.LOCATE_CHAINS])
def test_sets_without_device(built, flags):
    if not _no_gpu():
        pytest.skip("a GPU is present")
    L = P.lib()
    assert L.pgx_batch_locate(None, flags, 0, None) == P.ERR_NO_DEVICE
    assert b"no CPU fallback" in L.pgx_last_error()
    out = P.Locations()
    assert L.pgx_batch_locations(None, ctypes.byref(out)) == P.ERR_ARG
    assert L.pgx_batch_device_locations(None, ctypes.byref(out)) == P.ERR_ARG


@pytest.mark.gpu
def test_sets_on_a_batch_that_has_not_run(built, xy_paths):
    import oracle_ffi as O

    idx = P.Index(*xy_paths)
    b = P.Batch(idx, *O.pack_reads([b"ACGTACGTAC"]))
    for flags in (P.LOCATE_SEQ_SETS, P.LOCATE_SEQ_SETS | P.LOCATE_CHAINS):
        with pytest.raises(P.PgxError) as e:
            b.locate(flags)
        assert e.value.code == P.ERR_ARG and "not been run" in str(e.value)
    with pytest.raises(P.PgxError) as e:
        b.locate(P.LOCATE_SEQ_SETS | P.LOCATE_SEQ_IDS)
    assert e.value.code == P.ERR_ARG and "not been run" not in str(e.value)
    with pytest.raises(P.PgxError) as e:
        b.locations()
    assert e.value.code == P.ERR_ARG
    b.free()
    idx.close()
