"""CPU tier of the read pack: tests/pack_emu.py against hand-worked reads on a three-node graph with one node visited forward and reversed; a
case that trips each of the emulator's mutations; the header's struct and symbols through pgx_ffi; every usage error of find_mems --pack, all of
which exit before a device is opened."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pack_cases as C
import pack_emu as E
import pgx_ffi as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")
ENTRY_POINTS = ("pgx_pack_create", "pgx_pack_free", "pgx_pack_add", "pgx_pack_finish", "pgx_pack_device_result", "pgx_read_pack_arrays")

# nodes 1 (3 bases), 2 (2 bases), 3 (4 bases): base = [0, 0, 3, 5], G = 9.  Sequence 0 is 1+ 2+ 3+, sequence 1 is 3- 1+.
#   read 0: sequence 0 from 1, 2= 1X 1=: offsets 1, 2 of node 1 (g 1, 2), 0 and 1 of node 2 (g 3, 4)
#   read 1: sequence 1 from 0, 1S 2= 1I 1= 1D 2=: d = 0, 1, 2 of 3- are offsets 3, 2, 1 (g 8, 7, 6); the D skips d = 3 (offset 0, g 5); then
#           offsets 0, 1 of node 1 (g 0, 1)
HAND = C.make([[(1 << 1, 3), (2 << 1, 2), (3 << 1, 4)], [(3 << 1 | 1, 4), (1 << 1, 3)]],
              [(0, 1, [(C.EQ, 2), (C.X, 1), (C.EQ, 1)]), (1, 0, [(C.S, 1), (C.EQ, 2), (C.I, 1), (C.EQ, 1), (C.D, 1), (C.EQ, 2)])])
HAND_COV = [1, 2, 1, 1, 1, 0, 1, 1, 1]


def _emu(c, **kw):
    return E.read_pack(c["visit_offsets"], c["visit_nodes"], c["visit_length"], c["seq"], c["text_start"], c["op_offsets"], c["ops"], **kw)


def test_hand_worked_reads():
    r = _emu(HAND)
    assert (r["n_nodes"], r["n_bases"]) == (4, 9)
    assert r["node_length"].tolist() == [0, 3, 2, 4] and r["node_base"].tolist() == [0, 0, 3, 5, 9]
    assert r["cov"].tolist() == HAND_COV
    assert r["covered"].tolist() == [0, 3, 2, 3] and r["sum"].tolist() == [0, 4, 2, 3] and r["max"].tolist() == [0, 2, 1, 1]
    assert (r["reads_counted"], r["reads_filtered"], r["bases_added"]) == (2, 0, 9) and sum(HAND_COV) == 9
    assert E.summary_of(r["node_base"], r["node_length"], r["cov"]) == ([0, 3, 2, 3], [0, 4, 2, 3], [0, 2, 1, 1])


def test_the_filters():
    only1 = _emu(HAND, keep=[0, 1])
    assert only1["cov"].tolist() == [1, 1, 0, 0, 0, 0, 1, 1, 1] and (only1["reads_counted"], only1["reads_filtered"], only1["bases_added"]) == (1, 1, 5)
    by_q = _emu(HAND, mapq=[9, 10], min_mapq=10)
    assert by_q["cov"].tolist() == only1["cov"].tolist() and by_q["reads_filtered"] == 1
    assert _emu(HAND, mapq=[0, 0], min_mapq=0)["cov"].tolist() == HAND_COV  # min_mapq == 0: no filter, whatever the qualities
    ends = _emu(HAND, text_end=[5, 6])
    assert ends["cov"].tolist() == HAND_COV
    assert _emu(HAND, text_end=[5, 0])["reads_counted"] == 1  # text_end <= text_start: not counted


def test_a_read_whose_operations_consume_no_text_is_not_counted():
    c = C.make([[(2, 4)]], [(0, 2, [(C.S, 3), (C.I, 2)]), (E.NO_SEQUENCE, 0, [(C.EQ, 3)]), (0, 0, [(C.D, 2)])])
    r = _emu(c)
    assert r["cov"].tolist() == [0, 0, 0, 0] and (r["reads_counted"], r["bases_added"]) == (1, 0)  # (the D alone consumes text and adds nothing)


def test_two_lengths_of_one_node():
    with pytest.raises(E.FormatError) as e:
        _emu(C.two_lengths())
    assert e.value.node == 4


@pytest.mark.parametrize("mut", E.MUTATIONS)
def test_each_mutation_trips_the_hand_worked_case(mut):
    kw = dict(mapq=[60, 10], min_mapq=10) if mut == "filter_strict" else {}
    good, bad = _emu(HAND, **kw), _emu(HAND, mut=mut, **kw)
    assert good["cov"].tolist() == HAND_COV
    assert bad["cov"].tolist()[:9] != HAND_COV or bad["cov"][9:].any(), mut
    what = dict(d_counted=(5, 1), i_consumes=(5, 1), rev_off_by_one=(9, 1), base_inclusive=(5, 2), x_not_counted=(3, 0), filter_strict=(8, 0))[mut]
    assert int(bad["cov"][what[0]]) == what[1], (mut, bad["cov"].tolist())


def test_the_stated_cases_are_well_formed():
    for name, make in C.CASES.items():
        c = make()
        ends = c["seq_offsets"]
        for r in range(len(c["seq"])):
            if int(c["seq"][r]) == E.NO_SEQUENCE:
                continue
            q = int(c["seq"][r])
            used = sum(int(w) >> 4 for w in c["ops"][int(c["op_offsets"][r]):int(c["op_offsets"][r + 1])] if int(w) & 15 in (C.D, C.EQ, C.X))
            assert int(c["text_start"][r]) + used <= int(ends[q + 1] - ends[q]), (name, r)
        assert (c["visit_length"] >= 1).all() and (c["visit_length"] <= 1024).all(), name


def test_struct_layout_and_header():
    assert ctypes.sizeof(P.PackResult) == 120
    offs = {n: getattr(P.PackResult, n).offset for n, _ in P.PackResult._fields_}
    assert offs == dict(n_nodes=0, n_bases=8, n_text=16, reads_counted=24, reads_filtered=32, bases_added=40, n_projected=48, node_base=56, node_length=64, cov=72,
                        covered=80, sum=88, max=96, ms_add_total=104, ms_fold=112, ms_table=116)
    header = open(os.path.join(ROOT, "include", "pgx.h")).read()
    assert "read pack:" in header and "modulo 2^32" in header and "Must not run concurrently with pgx_pack_add" in header
    assert re.search(r"const uint64_t \*node_base;.*\n\s*const uint32_t \*node_length;.*\n\s*const uint32_t \*cov;", header)
    for name in ENTRY_POINTS:
        assert re.search(r"^(pgx_status|void) %s\(" % name, header, re.M), name
    assert (E.OP_I, E.OP_D, E.OP_S, E.OP_EQ, E.OP_X) == tuple(int(re.search(r"^#define\s+PGX_ALIGN_OP_%s\s+(\d+)u" % k, header, re.M).group(1)) for k in ("I", "D", "S", "EQ", "X"))


def test_symbols_are_exported_and_the_abi_version_stays(built):
    L = P.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    header = open(os.path.join(ROOT, "include", "pgx.h")).read()
    assert L.pgx_abi_version() == int(re.search(r"^#define\s+PGX_ABI_VERSION\s+(\d+)", header, re.M).group(1)) == 7
    assert callable(P.read_pack_arrays) and all(hasattr(P.Pack, m) for m in ("add", "finish", "device_result", "close"))


def test_null_handles_are_refused(built):
    L = P.lib()
    out = P.PackResult()
    assert L.pgx_pack_finish(None, ctypes.byref(out)) == P.ERR_ARG and L.pgx_pack_device_result(None, ctypes.byref(out)) == P.ERR_ARG
    L.pgx_pack_free(None)
    h = ctypes.c_void_p()
    assert L.pgx_pack_create(None, 0, ctypes.byref(h)) in (P.ERR_ARG, P.ERR_NO_DEVICE) and not h.value


def _run(*args):
    return subprocess.run([CLI, "no.ri", "no.tags", "no.reads", "10", "1"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)


def test_cli_usage_errors_exit_before_a_device_is_opened(built, tmp_path):
    out = str(tmp_path / "refused.pack")
    for args in (["--pack-bases", out], ["--pack-min-mapq", 5], ["--pack-only"], ["--mapq", "--gaf", out, "--pack-min-mapq", 5], ["--pack", out, "--pack-min-mapq", 5],
                 ["--gaf", out, "--pack-only"]):
        r = _run(*args)
        assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("usage: find_mems") and "--pack FILE" in r.stderr and not os.path.exists(out), args
    for bad in (0, 61, "x", -3, "7q"):
        r = _run("--pack", out, "--mapq", "--pack-min-mapq", bad)
        assert r.returncode == 1 and r.stdout == "" and "--pack-min-mapq: an integer 1 .. 60" in r.stderr and not os.path.exists(out), bad
    r = _run("--pack", out, "--pack-only", "--locate", "seqs")
    assert r.returncode == 1 and r.stdout == "" and "--pack-only makes no MEM text: it does not go with --locate" in r.stderr
    for name in ("--pack", "--pack-bases"):
        r = _run("--pack", out, name, "")
        assert r.returncode == 1 and name + ": a file name" in r.stderr, name
    # (--mapq is satisfied by --pack: this one gets as far as the files it cannot open)
    r = _run("--pack", out, "--mapq", "--pack-min-mapq", 60, "--pack-bases", out + ".bases", "--pack-only")
    assert r.returncode == 1 and "Cannot open r-index" in r.stderr and "usage" not in r.stderr and not os.path.exists(out)
