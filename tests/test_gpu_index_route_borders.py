"""GPU tier of read verify and read align through the index at the ends of its sequences: the route of find_mems --verify / --align
(pgx_batch_read_verify / pgx_batch_read_align: endmark = 1, the text image recovered from the index, candidates from the place stage), which
tests/test_gpu_verify.py and tests/test_gpu_align.py only feed reads that lie wholly inside one sequence.  On READ_CASES of
tests/index_route_cases.py -- reads that hang over the start and the end of a sequence by 1, 7, 8 and 9 bases, over text offset 0 and the
end of the text, over both ends of a sequence shorter than the read, reads at the end of a haplotype that a longer one continues, an indel
next to a sequence end, reads without a MEM and an empty read -- run(12, 1), locate(0), read_place(PLACE_LIST), read_verify and read_align
equal tests/verify_emu.py and tests/align_emu.py byte for byte, records and lists, with and without PGX_VERIFY_LIST / PGX_ALIGN_CIGAR, at
max_cand 1 and 16, penalties 1 and 4 and bands 0, 1, 3, 8, 31.  The emulators get the sequences of the file the index was built from, never
pgx_index_text, and the candidates chosen in Python from the place result.

Without any emulator: the verify winner of every read is the table's truth, which tests/test_index_route_cases.py derives from the text
alone; the reads of the shared-prefix pair have two candidates and the longer haplotype wins; and the records with clip_lo > 0, clip_hi > 0,
a span shorter than the read, text_end == Ls, text_start == 0, band_hit and no sequence come in the counts pinned in EXPECTED_COUNTS, so
that a shortfall of border cases fails.  Through the batch, a budget that forces three passes or more gives the bytes of the default budget
and reports its passes, and a budget below the longest read is refused with PGX_ERR_NOMEM and leaves the earlier result readable.

What is compared and what is not: include/pgx.h:814-815 (a sequence has Ls symbols, endmarker excluded; the span is lo = max(0, -diag),
hi = min(len, Ls - diag)) and include/pgx.h:900-901 (cells off the sequence do not exist: nothing reads the endmarker or a neighbouring
sequence).  The golden bidirectional_test/reads.txt holds no read that hangs over a sequence end (tests/test_index_route_cases.py tries
every diagonal), so nothing here relies on it."""
import os

import numpy as np
import pytest

import align_emu as A
import index_route_cases as C
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import verify_emu as V
from test_gpu_align import _same as _same_align
from test_gpu_mem_locate import _run_batch
from test_gpu_verify import _same as _same_verify

pytestmark = pytest.mark.gpu

R = C.READ_CASES
SEQ_LENS = [len(s) for s in R.seqs]
READ_LENS = [len(x) for x in R.reads]


@pytest.fixture(scope="module")
def placed(workdir):
    """the index of READ_CASES' collection, a batch of its reads after run, locate(0) and read_place(PLACE_LIST), and the place result"""
    path = os.path.join(workdir, "irb_reads.txt")
    with open(path, "wb") as f:
        f.write(R.raw)
    ri, tags = W.build_index_from_text(path, workdir, "irb_reads")[:2]
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    cat, offs = O.pack_reads(R.reads)
    b, res = _run_batch(idx, cat, offs, C.MIN_LEN, 1)
    b.locate(0)
    place = b.read_place(P.PLACE_LIST)
    yield idx, b, place
    b.free()
    idx.close()


_emu = {}


def _verify_emu(place, max_cand, penalty):
    if (max_cand, penalty) not in _emu:
        _emu[(max_cand, penalty)] = V.read_verify(R.seqs, R.reads, V.candidates_from_places(place, max_cand), penalty)
    return _emu[(max_cand, penalty)]


def test_the_place_stage_names_the_candidates_of_the_table(placed):
    idx, b, place = placed
    assert place["n_reads"] == len(R.reads)
    for max_cand in C.MAX_CANDS:
        got = V.candidates_from_places(place, max_cand)
        assert got == [C.truth_candidates(t, max_cand) for t in R.truth], max_cand


@pytest.mark.parametrize("penalty", C.PENALTIES)
@pytest.mark.parametrize("max_cand", C.MAX_CANDS)
def test_verify_equals_the_emulator_and_the_truth(placed, max_cand, penalty):
    idx, b, place = placed
    exp = _verify_emu(place, max_cand, penalty)
    got = b.read_verify(max_cand, penalty, P.VERIFY_LIST)
    assert (got["n_reads"], got["n_cands"], got["flags"], got["max_cand"], got["mismatch_penalty"]) == (len(R.reads), len(exp["cands"]), P.VERIFY_LIST, max_cand, penalty)
    bad = np.flatnonzero(got["reads"] != exp["reads"])
    assert len(bad) == 0, (len(bad), int(bad[0]), R.kinds[bad[0]], got["reads"][bad[0]], exp["reads"][bad[0]])
    _same_verify(got, exp)
    plain = b.read_verify(max_cand, penalty, 0)
    assert plain["reads"].tobytes() == exp["reads"].tobytes() and plain["cands"] is None and plain["cand_offsets"] is None and plain["flags"] == 0
    # without the emulator: the winner is the table's truth
    v = got["reads"]
    for r, truth in enumerate(R.truth):
        want = C.winner_truth(truth, max_cand)
        assert (None if int(v["seq"][r]) == V.NO_SEQUENCE else (int(v["seq"][r]), int(v["diag"][r]))) == want, (r, R.kinds[r], v[r])
        if isinstance(truth, list):
            assert int(v["n_cand"][r]) == min(2, max_cand) and int(v["cand_index"][r]) == (1 if max_cand > 1 else 0) and int(v["n_tied"][r]) == 1, (r, v[r])
            mine = got["cands"][int(got["cand_offsets"][r]):int(got["cand_offsets"][r + 1])]
            assert [(int(c["seq"]), int(c["diag"])) for c in mine] == C.truth_candidates(truth, max_cand)
            if max_cand > 1:  # clipped on the shorter haplotype, whole on the longer one
                assert int(mine[0]["span_hi"]) - int(mine[0]["span_lo"]) < READ_LENS[r] == int(mine[1]["span_hi"]) - int(mine[1]["span_lo"])
        elif truth is not None:
            lo, hi = max(0, -truth[1]), min(READ_LENS[r], SEQ_LENS[truth[0]] - truth[1])
            assert (int(v["span_lo"][r]), int(v["span_hi"][r]), int(v["n_cand"][r])) == (lo, hi, 1), (r, R.kinds[r], v[r])
            a, e = R.core[r]
            assert int(v["longest_run"][r]) >= e - a and int(v["seg_score"][r]) >= e - a, (r, R.kinds[r], v[r])


@pytest.mark.parametrize("band", C.BANDS)
def test_align_equals_the_emulator_and_reaches_every_border(placed, band):
    idx, b, place = placed
    counted = False
    for max_cand, penalty in ((1, 1), (16, 4)):
        vexp = _verify_emu(place, max_cand, penalty)
        verified = b.read_verify(max_cand, penalty)
        assert verified["reads"].tobytes() == vexp["reads"].tobytes()
        exp = A.read_align(R.seqs, R.reads, A.candidates_from_verified(vexp["reads"]), band)
        got = b.read_align(band, P.ALIGN_CIGAR)
        assert (got["n_reads"], got["n_ops"], got["flags"], got["band"], got["passes"]) == (len(R.reads), len(exp["ops"]), P.ALIGN_CIGAR, band, 1)
        bad = np.flatnonzero(got["reads"] != exp["reads"])
        assert len(bad) == 0, (len(bad), int(bad[0]), R.kinds[bad[0]], got["reads"][bad[0]], exp["reads"][bad[0]])
        _same_align(got, exp)
        plain = b.read_align(band, 0)
        assert plain["reads"].tobytes() == exp["reads"].tobytes() and plain["ops"] is None and plain["op_offsets"] is None and plain["flags"] == 0
        if (max_cand, penalty) == (16, 4):  # without the emulator: every border class, in the counts the CPU tier derived from the tables
            counts = C.border_counts(SEQ_LENS, READ_LENS, verified["reads"], got["reads"])
            assert counts == C.EXPECTED_COUNTS[band], (band, counts)
            a = got["reads"]
            assert (a["clip_lo"].astype(np.int64) + a["clip_hi"] + a["n_match"] + a["n_mismatch"] + a["n_ins"] == np.array(READ_LENS))[a["seq"] != A.NO_SEQUENCE].all()
            counted = True
    assert counted


def test_passes_over_a_small_budget_through_the_batch(placed, monkeypatch):
    idx, b, place = placed
    band = 8  # 8 bytes a read position: the longest read of 80 needs 640 bytes, all reads together about 14 000 a pass
    monkeypatch.delenv("PGX_ALIGN_BUDGET_MB", raising=False)
    b.read_verify(16, 4)
    first = b.read_align(band, P.ALIGN_CIGAR)
    assert first["passes"] == 1
    need = [(n * 8 + 15) & ~15 for n in READ_LENS]
    for budget in (sum(need) // 2 + 640, 4096, 640):  # two passes, then a few reads a pass, then as few as one
        passes, cur = 1, 0
        for x in need:  # whole consecutive reads while they fit
            if cur + x > budget:
                passes, cur = passes + 1, 0
            cur += x
        monkeypatch.setenv("PGX_ALIGN_BUDGET_MB", repr(budget / 1048576.0))
        got = b.read_align(band, P.ALIGN_CIGAR)
        assert got["passes"] == passes and got["scratch_bytes"] <= budget, (budget, got["passes"], passes)
        _same_align(got, first)
        plain = b.read_align(band, 0)
        assert plain["reads"].tobytes() == first["reads"].tobytes() and plain["passes"] == passes
    assert passes >= 3
    b.read_align(band, P.ALIGN_CIGAR)
    monkeypatch.setenv("PGX_ALIGN_BUDGET_MB", repr(639 / 1048576.0))  # below the longest read
    long_at = next(r for r, x in enumerate(need) if x > 639)
    with pytest.raises(P.PgxError) as e:
        b.read_align(band, P.ALIGN_CIGAR)
    assert e.value.code == P.ERR_NOMEM and "read %d needs 640" % long_at in str(e.value) and "PGX_ALIGN_BUDGET_MB" in str(e.value)
    _same_align(b.aligned(), first)  # the earlier result stays readable
    monkeypatch.delenv("PGX_ALIGN_BUDGET_MB")
    _same_align(b.read_align(band, P.ALIGN_CIGAR), first)
