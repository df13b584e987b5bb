"""The device index build (pgx_build_index_from_text[s]_device, build_rindex --text) against the reference's fixtures and the CPU builder:
"equal" always means the bytes of both output files.  Case tables: build_device_cases.py (test_build_device_cpu.py shows that they hold
the borders they claim and that the CPU builder follows the naively stated order)."""
import os
import subprocess

import numpy as np
import pytest

import build_device_cases as BC
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
from cli_format import strip_timing

pytestmark = pytest.mark.gpu

G = O.GOLDEN
BT = os.path.join(G, "bidirectional_test")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pangenome-index_amd")

FIXTURES = [  # the five (text, .rl_bwt) pairs of tests/test_formats.py
    ("x.newline_separated", "x.rl_bwt"),
    ("med_test.txt", "med_test.rl_bwt"),
    ("bidirectional_test/contigs_xy", "bidirectional_test/contigs_xy.rl_bwt"),
    ("bidirectional_test/small_test/test.txt", "bidirectional_test/small_test/test.rl_bwt"),
    ("two_contig_graph/contigs_XY.txt", "two_contig_graph/contigs_XY.rl_bwt"),
]
RI_GOLDENS = {"bidirectional_test/contigs_xy": "bidirectional_test/xy.ri", "two_contig_graph/contigs_XY.txt": "two_contig_graph/xy.ri"}  # legacy layout


def _read(p):
    with open(p, "rb") as f:
        return f.read()


def _same_bwt(path, golden):
    """the reference's .rl_bwt fixtures hold what grlBWT wrote: three of the five with two length bytes a record where the runs need one, and
    grlBWT may split a run (tests/test_formats.py) -- so no writer of this project reproduces those three byte for byte, the CPU call included.
    Equal here: the expanded BWT, and the bytes wherever the record width is the same."""
    a, b = _read(path), _read(golden)
    if a[8:16] == b[8:16]:
        return a == b
    s1, l1 = W.read_rlbwt_runs(path)
    s2, l2 = W.read_rlbwt_runs(golden)
    return len(s1) == len(s2) and np.array_equal(s1, s2) and np.array_equal(l1, l2) and np.array_equal(np.repeat(s1, l1.astype(np.int64)), np.repeat(s2, l2.astype(np.int64)))


def _files(d, tag):
    return os.path.join(d, tag + ".rl_bwt"), os.path.join(d, tag + ".ri")


def _check_text(text, d, encoded=True, name="t"):
    """device build of `text` == CPU build of it, both files; returns the stage values"""
    d = str(d)
    src = os.path.join(d, name + ".txt")
    with open(src, "wb") as f:
        f.write(text)
    crl, cri = _files(d, name + ".cpu")
    drl, dri = _files(d, name + ".dev")
    P.build_index_from_text(src, crl, cri, encoded)
    ms = P.build_index_from_text_device(src, drl, dri, encoded)
    assert _read(drl) == _read(crl), name + ": .rl_bwt differs"
    assert _read(dri) == _read(cri), name + ": .ri differs"
    assert sorted(os.listdir(d)) == sorted(os.path.basename(p) for p in (src, crl, cri, drl, dri)), "stray files"
    for p in (src, crl, cri, drl, dri):
        os.remove(p)
    return ms


@pytest.fixture(scope="module")
def pangenome(tmp_path_factory, built):
    """synth_pangenome_text(base_len=40_000, n_hap=8): the text, its forward-only half, and the CPU builder's files for the latter"""
    d = str(tmp_path_factory.mktemp("bd_pan"))
    both = os.path.join(d, "both.txt")
    assert W.synth_pangenome_text(both, base_len=40_000, n_hap=8) == 16
    seqs = _read(both).split(b"\n")[:-1]
    fwd = os.path.join(d, "fwd.txt")
    with open(fwd, "wb") as f:
        f.write(b"".join(s + b"\n" for s in seqs[0::2]))
    rl, ri = _files(d, "fwd.cpu")
    P.build_index_from_text(fwd, rl, ri, True)
    return {"dir": d, "both": both, "fwd": fwd, "seqs": seqs, "fwd_rl": _read(rl), "fwd_ri": _read(ri)}


# ---- 1. reference fixtures
@pytest.mark.parametrize("text,rlbwt", FIXTURES)
def test_reference_fixtures(built, tmp_path, text, rlbwt):
    src = os.path.join(G, text)
    for encoded in (True, False):
        crl, cri = _files(str(tmp_path), "cpu%d" % encoded)
        drl, dri = _files(str(tmp_path), "dev%d" % encoded)
        P.build_index_from_text(src, crl, cri, encoded)
        ms = P.build_index_from_text_device(src, drl, dri, encoded)
        assert _same_bwt(drl, os.path.join(G, rlbwt))  # the reference's own file
        assert _read(drl) == _read(crl) and _read(dri) == _read(cri)
        if not encoded and text in RI_GOLDENS:
            assert _read(dri) == _read(os.path.join(G, RI_GOLDENS[text]))  # the reference's own .ri, from text on the device
        assert tuple(ms) == P.BUILD_INDEX_DEVICE_STAGES and ms["rounds"] == int(ms["rounds"]) and 0 <= ms["rounds"] <= 40
        assert all(ms[k] >= 0 for k in ms) and ms["first_sort"] > 0
    # without the .rl_bwt: the same .ri, no other file
    only = str(tmp_path / "only.ri")
    P.build_index_from_text_device(src, None, only, True)
    assert _read(only) == _read(_files(str(tmp_path), "cpu1")[1])


# ---- 2. depth borders
@pytest.mark.parametrize("L", BC.DEPTHS)
def test_depth_borders(built, tmp_path, L):
    _check_text(BC.depth_text(L), tmp_path, name="depth_%d" % L)


# ---- 3. ties only endmarkers break
@pytest.mark.parametrize("name", sorted(BC.tie_texts()))
def test_ties_only_endmarkers_break(built, tmp_path, name):
    text = BC.tie_texts()[name]
    _check_text(text, tmp_path, name=name)
    if name == "no_final_newline":  # the text gets its newline: the same files as the text that has it
        d = str(tmp_path)
        a, b = os.path.join(d, "a.txt"), os.path.join(d, "b.txt")
        open(a, "wb").write(text)
        open(b, "wb").write(text + b"\n")
        P.build_index_from_text_device(a, *_files(d, "a"))
        P.build_index_from_text_device(b, *_files(d, "b"))
        assert [_read(p) for p in _files(d, "a")] == [_read(p) for p in _files(d, "b")]


# ---- 4. size and digit borders
@pytest.mark.parametrize("name", sorted(BC.SIZE_CASES, key=lambda k: BC.SIZE_CASES[k][0]))
def test_size_and_digit_borders(built, tmp_path, name):
    _check_text(BC.size_text(name), tmp_path, name=name)
    _check_text(BC.size_text(name), tmp_path, encoded=False, name=name + "_legacy")


def test_many_one_symbol_sequences(built, tmp_path):
    _check_text(BC.many_sequences_text(), tmp_path, name="many_seq")


# ---- 5. large groups
def test_large_groups(built, tmp_path):
    ms = _check_text(BC.large_groups_text(), tmp_path, name="groups")
    assert 10 <= ms["rounds"] <= 40  # a common prefix of 5997 symbols from a first depth of 10: ten doublings


def test_pangenome_text_and_its_forward_half(built, tmp_path, pangenome):
    d = str(tmp_path)
    drl, dri = _files(d, "fwd.dev")
    ms = P.build_index_from_text_device(pangenome["fwd"], drl, dri, True)
    assert 1 <= ms["rounds"] <= 40
    assert 1 <= P.build_index_device_timing()["rounds"] <= 40
    assert _read(drl) == pangenome["fwd_rl"] and _read(dri) == pangenome["fwd_ri"]
    crl, cri = _files(d, "both.cpu")
    drl, dri = _files(d, "both.dev")
    P.build_index_from_text(pangenome["both"], crl, cri, True)
    ms = P.build_index_from_text_device(pangenome["both"], drl, dri, True)
    assert 1 <= ms["rounds"] <= 40
    assert _read(drl) == _read(crl) and _read(dri) == _read(cri)
    # the workload helper takes the device path when a device is given
    ri, tags, rl = W.build_index_from_text(pangenome["fwd"], os.path.join(d, "w"), "fwd", with_tags=False, device=0)
    assert tags is None and _read(ri) == pangenome["fwd_ri"] and _read(rl) == pangenome["fwd_rl"]


# ---- 6. several texts
@pytest.mark.parametrize("parts", [1, 3, 16])
def test_several_texts(built, tmp_path, pangenome, parts):
    both = pangenome["seqs"]  # 16 sequences: the whole text, both orientations
    d = str(tmp_path)
    whole = os.path.join(d, "whole.txt")
    open(whole, "wb").write(b"".join(s + b"\n" for s in both))
    paths = []
    for k in range(parts):
        p = os.path.join(d, "part%d.txt" % k)
        open(p, "wb").write(b"".join(s + b"\n" for s in both[len(both) * k // parts:len(both) * (k + 1) // parts]))
        paths.append(p)
    crl, cri = _files(d, "cpu")
    drl, dri = _files(d, "dev")
    orl, ori = _files(d, "one")
    P.build_index_from_texts(paths, crl, cri, True)
    ms = P.build_index_from_texts_device(paths, drl, dri, True)
    P.build_index_from_text_device(whole, orl, ori, True)
    assert 1 <= ms["rounds"] <= 40
    assert _read(drl) == _read(crl) == _read(orl)
    assert _read(dri) == _read(cri) == _read(ori)


# ---- 7. refusals
def _good_call(d):
    rl, ri = _files(d, "good")
    P.build_index_from_text_device(os.path.join(G, "x.newline_separated"), rl, ri, True)
    assert _same_bwt(rl, os.path.join(G, "x.rl_bwt"))
    os.remove(rl)
    os.remove(ri)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_refuses_a_byte_outside_the_alphabet(built, tmp_path, where):
    d = str(tmp_path)
    text = bytearray(BC.size_text("n_4097"))
    off = {"first": 0, "middle": 2500, "last": len(text) - 1}[where]
    text[off] = ord("X")
    src = os.path.join(d, "bad.txt")
    open(src, "wb").write(bytes(text))
    rl, ri = _files(d, "bad")
    with pytest.raises(P.PgxError) as e:
        P.build_index_from_text_device(src, rl, ri, True)
    assert e.value.code == P.ERR_UNSUPPORTED and "0x58" in str(e.value) and ("offset %d of" % off) in str(e.value)
    assert sorted(os.listdir(d)) == ["bad.txt"]
    # in the second of two texts: the offset within that text, and within the collection
    ok = os.path.join(d, "ok.txt")
    open(ok, "wb").write(b"ACGT\nAC")
    with pytest.raises(P.PgxError) as e:
        P.build_index_from_texts_device([ok, src], rl, ri, True)
    assert e.value.code == P.ERR_UNSUPPORTED and ("offset %d of %s" % (off, src)) in str(e.value) and ("offset %d of the collection" % (off + 8)) in str(e.value)
    assert sorted(os.listdir(d)) == ["bad.txt", "ok.txt"]
    _good_call(d)


def test_refuses_beyond_the_memory_budget(built, tmp_path, pangenome, monkeypatch):
    d = str(tmp_path)
    rl, ri = _files(d, "nomem")
    monkeypatch.setenv("PGX_BUILD_DEVICE_BUDGET_MB", "1")
    with pytest.raises(P.PgxError) as e:
        P.build_index_from_text_device(pangenome["fwd"], rl, ri, True)
    assert e.value.code == P.ERR_NOMEM and str(1 << 20) in str(e.value)
    n = os.path.getsize(pangenome["fwd"])
    need = [int(w) for w in str(e.value).replace(",", " ").split() if w.isdigit() and int(w) > n]
    assert need and 30 * n < need[0] < 40 * n  # "some tens of bytes per symbol": DESIGN's formula
    assert os.listdir(d) == []
    monkeypatch.setenv("PGX_BUILD_DEVICE_BUDGET_MB", "0.5")  # fractions
    with pytest.raises(P.PgxError) as e:
        P.build_index_from_text_device(pangenome["fwd"], rl, ri, True)
    assert e.value.code == P.ERR_NOMEM and str(1 << 19) in str(e.value)
    monkeypatch.setenv("PGX_BUILD_DEVICE_BUDGET_MB", "64")  # read per call: enough now
    P.build_index_from_text_device(pangenome["fwd"], rl, ri, True)
    assert _read(rl) == pangenome["fwd_rl"] and _read(ri) == pangenome["fwd_ri"]
    monkeypatch.delenv("PGX_BUILD_DEVICE_BUDGET_MB")
    _good_call(d)


def test_refuses_a_collection_of_2_to_the_32_without_reading_it(built, tmp_path):
    d = str(tmp_path)
    big = os.path.join(d, "sparse.txt")
    open(big, "wb").close()
    os.truncate(big, 1 << 32)
    rl, ri = _files(d, "big")
    with pytest.raises(P.PgxError) as e:
        P.build_index_from_text_device(big, rl, ri, True)
    assert e.value.code == P.ERR_UNSUPPORTED and "pgx_build_index_from_texts" in str(e.value)
    small = os.path.join(d, "small.txt")
    open(small, "wb").write(b"ACGT\n")
    os.truncate(big, (1 << 32) - (1 << 20) - 5)  # with the second text: exactly the bound
    with pytest.raises(P.PgxError) as e:
        P.build_index_from_texts_device([small, big], rl, ri, True)
    assert e.value.code == P.ERR_UNSUPPORTED
    os.remove(big)
    empty = os.path.join(d, "empty.txt")
    open(empty, "wb").close()
    with pytest.raises(P.PgxError) as e:
        P.build_index_from_texts_device([small, empty], rl, ri, True)
    assert e.value.code == P.ERR_FORMAT and "empty text" in str(e.value)
    with pytest.raises(P.PgxError) as e:
        P.build_index_from_text_device(os.path.join(d, "missing.txt"), rl, ri, True)
    assert e.value.code == P.ERR_IO
    assert sorted(os.listdir(d)) == ["empty.txt", "small.txt"]
    _good_call(d)


def test_refuses_an_output_that_cannot_be_written(built, tmp_path):
    d = str(tmp_path)
    src = os.path.join(G, "x.newline_separated")
    blocker = os.path.join(d, "not_a_directory")
    open(blocker, "wb").write(b"x")
    cases = [(os.path.join(d, "ok.rl_bwt"), os.path.join(blocker, "x.ri")), (os.path.join(blocker, "x.rl_bwt"), os.path.join(d, "ok.ri")),
             (os.path.join(d, "ok.rl_bwt"), os.path.join(d, "no_such_dir", "x.ri"))]
    if os.geteuid() != 0:  # (root writes into a directory without write permission)
        ro = os.path.join(d, "read_only")
        os.mkdir(ro)
        os.chmod(ro, 0o555)
        cases.append((os.path.join(d, "ok.rl_bwt"), os.path.join(ro, "x.ri")))
    for rl, ri in cases:
        with pytest.raises(P.PgxError) as e:
            P.build_index_from_text_device(src, rl, ri, True)
        assert e.value.code == P.ERR_IO
        assert sorted(os.listdir(d)) == sorted(["not_a_directory"] + (["read_only"] if os.geteuid() != 0 else []))
    _good_call(d)


# ---- 8. end to end through the CLIs
def _run(exe, *args):
    return subprocess.run([os.path.join(BIN, exe)] + [str(a) for a in args], capture_output=True, timeout=600)


def test_end_to_end_from_the_graph(built, tmp_path):
    d = str(tmp_path)
    r = _run("gbz_extract", "-b", os.path.join(BT, "xy.gbz"))
    assert r.returncode == 0, r.stderr
    text = os.path.join(d, "xy.txt")
    open(text, "wb").write(r.stdout)
    rl, ri = _files(d, "xy")
    r = _run("build_rindex", "--text", text, "--rlbwt", rl, "--device", "0", "--legacy")
    assert r.returncode == 0, r.stderr
    open(ri, "wb").write(r.stdout)
    assert r.stdout == _read(os.path.join(BT, "xy.ri")) and _same_bwt(rl, os.path.join(BT, "contigs_xy.rl_bwt"))
    assert sorted(os.listdir(d)) == ["xy.ri", "xy.rl_bwt", "xy.txt"]
    tags = os.path.join(d, "xy.tags")
    r = _run("build_tags", os.path.join(BT, "xy.gbz"), rl, tags)
    assert r.returncode == 0, r.stderr
    conv = os.path.join(d, "xy_compressed.tags")
    r = _run("convert_tags", tags, conv, "--format", "bytecode")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([os.path.join(BIN, "find_mems"), ri, conv, os.path.join(BT, "reads.txt"), "5", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert strip_timing(r.stdout) == open(os.path.join(G, "expected_find_mems_xy_reads_5_1.txt")).read()
    # the encoded form on stdout, and a failure: status 1, the library's message, nothing on stdout, no file
    r = _run("build_rindex", "--text", text)
    cri = os.path.join(d, "cpu.ri")
    P.build_index_from_text(text, None, cri, True)
    assert r.returncode == 0 and r.stdout == _read(cri)
    r = _run("build_rindex", "--text", os.path.join(d, "missing.txt"), "--rlbwt", os.path.join(d, "none.rl_bwt"))
    assert r.returncode == 1 and r.stdout == b"" and b"Cannot open text" in r.stderr
    r = _run("build_rindex", "--text", text, "--device", "99")
    assert r.returncode == 1 and r.stdout == b"" and b"device ordinal" in r.stderr
    assert not os.path.exists(os.path.join(d, "none.rl_bwt"))


# ---- 9. randomised sweep
def test_randomised_sweep(built, tmp_path):
    d = str(tmp_path)
    src = os.path.join(d, "s.txt")
    crl, cri = _files(d, "cpu")
    drl, dri = _files(d, "dev")
    for seed in range(300):
        with open(src, "wb") as f:
            f.write(BC.sweep_text(seed))
        enc = bool(seed & 1)
        P.build_index_from_text(src, crl, cri, enc)
        P.build_index_from_text_device(src, drl, dri, enc)
        assert _read(drl) == _read(crl) and _read(dri) == _read(cri), "sweep seed %d" % seed
