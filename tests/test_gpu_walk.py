"""GPU tier of pgx_batch_read_walk on the small variation graph of tests/walk_cases.py (8 haplotypes in both orientations over a 3 kb base of
1 .. 64 bp nodes with two-allele bubbles; tags by pgx_build_tags_paths): Index.paths() is the graph's path table; run, locate, read_place,
read_verify, read_align and read_walk equal tests/walk_emu.py fed with Index.paths() and the align records -- as host and as device arrays,
across a later locate of every form and across a refill of the batch; the calls it refuses.

Then without the emulator: 200 error-free reads of 60 bases cut from a known (haplotype, offset), half of them reverse-complemented.  Each walk
is the slice of the source path with path_start as cut, whichever haplotype verify chose: ties between haplotypes that agree over the read are
one walk.  Reads whose bytes also occur in the collection with a different walk (a read that ends inside a bubble on a prefix its two alleles
share) are left out; they are counted on the CPU from the texts, and with seed 3 there are 0 of them (seeds 23, 24, 25: 2, 1, 1; the cap is
5 %).  The same reads with base 30 deleted: the steps, path_start and path_len are those of the source and path_end - path_start is one
more than the read's length -- for every read whose verify winner holds the read's 60 bases.  The others are left out, and the test shows
from the texts alone that each of them has a haplotype that shares one half of the read and carries an allele of its own in the other half:
verify scores one diagonal, on which the other half is a wall of chance matches, so such a haplotype can win, and the stage aligns and walks
the winner only.  With seed 3, 174 of the 200 reads are kept and 26 are left out (the bubbles lie about 100 bp apart, the reads are 60 bp long)"""
import os

import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import walk_cases as C
import walk_emu as E
from test_gpu_hits import _device_read
from test_gpu_mem_locate import _run_batch

pytestmark = pytest.mark.gpu
SETS, UNIQ_IDS = P.LOCATE_SEQ_SETS, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE


@pytest.fixture(scope="module")
def world(workdir):
    g = C.graph()
    text = os.path.join(workdir, "walk_graph.txt")
    with open(text, "wb") as f:
        f.write(b"".join(t + b"\n" for t in g["texts"]))
    ri = W.build_index_from_text(text, workdir, "walk_graph", with_tags=False)[0]
    tags = os.path.join(workdir, "walk_graph.graph.tags")
    P.build_tags_paths(ri, g["path_offsets"], g["path_nodes"], g["node_length"], 1, tags, flags=P.BUILD_TAGS_OUT_COMPACT)
    truth, reads = C.cut_reads(g)
    return g, ri, tags, truth, reads


def _same(a, b):
    assert a["reads"].tobytes() == b["reads"].tobytes()
    for k in ("step_offsets", "steps"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or a[k].tobytes() == b[k].tobytes()), k


def _chain(b, band=8):
    b.locate(0)
    b.read_place(0)
    b.read_verify(1, 4)
    return b.read_align(band, P.ALIGN_CIGAR)


def _check_walk(idx, b, tables):
    po, pn, vl = tables
    a = _chain(b)["reads"]
    n = len(a)
    exp = E.read_walk(po, pn, vl, a["seq"], a["text_start"], a["text_end"])
    got = b.read_walk(P.WALK_STEPS)
    assert (got["n_reads"], got["n_steps"], got["flags"]) == (n, len(exp["steps"]), P.WALK_STEPS)
    bad = np.flatnonzero(got["reads"] != exp["reads"])
    assert len(bad) == 0, (len(bad), int(bad[0]), got["reads"][bad[0]], exp["reads"][bad[0]], a[bad[0]])
    _same(got, exp)
    plain = b.read_walk(0)
    assert plain["reads"].tobytes() == exp["reads"].tobytes() and plain["steps"] is None and plain["step_offsets"] is None
    assert plain["flags"] == 0 and plain["n_steps"] == len(exp["steps"])
    b.read_walk(P.WALK_STEPS)
    dev = b.device_walked()
    assert dev["device"] and (dev["n_reads"], dev["n_steps"], dev["flags"]) == (n, len(exp["steps"]), P.WALK_STEPS)
    for k, nbytes in (("reads", n * 32), ("step_offsets", (n + 1) * 8), ("steps", len(exp["steps"]) * 8)):
        if nbytes:
            assert _device_read(dev[k].__cuda_array_interface__["data"][0], nbytes).tobytes() == exp[k].tobytes(), k
    assert dev["reads"].__cuda_array_interface__["shape"] == (n, 4) and dev["steps"].__cuda_array_interface__["shape"] == (len(exp["steps"]),)
    for flags in (SETS, UNIQ_IDS, P.LOCATE_SEQ_IDS, P.LOCATE_UNIQUE, 0, P.LOCATE_CHAINS):  # walked first, any locate afterwards
        b.locate(flags)
        _same(b.walked(), exp)
    return exp


def test_walk_equals_the_emulator_and_survives_locates_and_a_refill(world):
    g, ri, tags, truth, reads = world
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    tables = idx.paths()
    assert np.array_equal(tables[0], g["path_offsets"]) and np.array_equal(tables[1], g["path_nodes"])
    assert np.array_equal(tables[2], g["node_length"][(g["path_nodes"] >> np.uint64(1)).astype(np.int64) - 1])
    noisy = [r if k % 3 else r[:20] + b"N" + r[21:] for k, r in enumerate(reads[:120])] + [b"ACGT" * 10, b"T", b""]  # substitutions, a stranger, stubs
    cat, offs = O.pack_reads(noisy)
    b, _ = _run_batch(idx, cat, offs, 12, 1)
    first = _check_walk(idx, b, tables)
    assert (first["reads"]["n_steps"] > 1).any() and (first["reads"]["n_steps"] == 0).any()
    cat2, offs2 = O.pack_reads(C.deleted(reads[60:]) + reads[:7])  # the batch filled again, with another number of reads
    b.upload(cat2, offs2)
    b.run(12, 1, P.RUN_TAGS)
    second = _check_walk(idx, b, tables)
    fresh, _ = _run_batch(idx, cat2, offs2, 12, 1)
    _chain(fresh)
    _same(fresh.read_walk(P.WALK_STEPS), second)
    fresh.free()
    b.free()
    idx.close()


def _walked(ri, tags, reads):
    cat, offs = O.pack_reads(reads)
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    b, _ = _run_batch(idx, cat, offs, 12, 1)
    a = _chain(b)["reads"]
    w = b.read_walk(P.WALK_STEPS)
    b.free()
    idx.close()
    steps = [w["steps"][int(w["step_offsets"][r]):int(w["step_offsets"][r + 1])].tolist() for r in range(len(reads))]
    return a, w["reads"], steps


def test_error_free_reads_walk_their_source_path(world):
    g, ri, tags, truth, reads = world
    keep = np.flatnonzero(~C.ambiguous(g, truth, reads))
    assert len(keep) == C.N_READS  # (seed 3: none is left out; the cap would be C.MAX_LEFT_OUT)
    a, w, steps = _walked(ri, tags, reads)
    assert (a["edits"] == 0).all()
    chosen_other = 0
    for r in keep:
        q, o = truth[r]
        pl, ps, pe, st = C.walk_of(g, q, o, o + C.READ_LEN)
        assert steps[r] == st and (int(w["path_len"][r]), int(w["path_start"][r]), int(w["path_end"][r]), int(w["n_steps"][r])) == (pl, ps, pe, len(st)), r
        assert pe - ps == C.READ_LEN and int(w["seq"][r]) == int(a["seq"][r]) and int(w["seq"][r]) % 2 == q % 2
        chosen_other += int(w["seq"][r]) != q
    assert chosen_other > 0  # ties collapsed: verify's winner was another haplotype that agrees over the read, the walk is the same


def test_a_deleted_base_keeps_the_walk(world):
    g, ri, tags, truth, reads = world
    forms = C.deleted(reads)
    a, w, steps = _walked(ri, tags, forms)
    texts = g["texts"]
    holds = np.array([int(a["seq"][r]) != E.NO_SEQUENCE and texts[int(a["seq"][r])].find(reads[r]) >= 0 for r in range(C.N_READS)])
    # verify scores one diagonal, on which half of such a read is a wall of chance matches: its winner may be a haplotype that shares one half of the
    # read and has an allele of its own in the other, and the stage aligns and walks the winner only.  Only such reads may be left out.
    for r in np.flatnonzero(~holds):
        q, o = truth[r]
        halves = (reads[r][:C.AT], reads[r][C.AT + 1:])
        assert any(any(h in t for h in halves) and reads[r] not in t for t in texts[q % 2::2]), r
    keep = np.flatnonzero(holds)
    print("deleted base: %d of %d reads kept, %d left out" % (len(keep), C.N_READS, C.N_READS - len(keep)))
    assert len(keep) >= C.N_READS // 2, len(keep)
    assert (a["edits"][keep] == 1).all() and (a["n_del"][keep] == 1).all() and (a["clip_lo"][keep] == 0).all() and (a["clip_hi"][keep] == 0).all()
    for r in keep:
        q, o = truth[r]
        pl, ps, pe, st = C.walk_of(g, q, o, o + C.READ_LEN)
        assert steps[r] == st and (int(w["path_start"][r]), int(w["path_len"][r])) == (ps, pl), r
        assert int(w["path_end"][r]) - int(w["path_start"][r]) == len(forms[r]) + 1 == C.READ_LEN


def test_refusals_leave_everything_as_it_was(world):
    g, ri, tags, truth, reads = world
    cat, offs = O.pack_reads(reads[:50])
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    b = P.Batch(idx, cat, offs)

    def refused(call):
        with pytest.raises(P.PgxError) as e:
            call()
        assert e.value.code == P.ERR_ARG, str(e.value)
        return str(e.value)

    assert "not been run" in refused(lambda: b.read_walk())
    b.run(12, 1, P.RUN_TAGS)
    assert "no align result" in refused(lambda: b.read_walk())
    refused(b.walked)
    refused(b.device_walked)
    b.locate(0)
    b.read_place(0)
    b.read_verify(1, 4)
    assert "no align result" in refused(lambda: b.read_walk())
    b.read_align(8, 0)
    first = b.read_walk(P.WALK_STEPS)
    assert first["ms_walk"] == 0  # the run had no PGX_RUN_TIMING
    assert "unknown flag" in refused(lambda: b.read_walk(2))
    _same(b.walked(), first)  # the earlier result stays
    b.run(12, 1, P.RUN_TAGS | P.RUN_TIMING)  # a re-run and an upload invalidate it
    refused(b.walked)
    refused(lambda: b.read_walk())  # (the align result belonged to the run before)
    _chain(b)
    timed = b.read_walk(P.WALK_STEPS)
    _same(timed, first)
    assert timed["ms_walk"] > 0
    b.upload(cat, offs)
    refused(b.walked)
    b.free()
    idx.close()
