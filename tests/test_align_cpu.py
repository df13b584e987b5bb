"""CPU tier of read align: tests/align_emu.py (the definitions of include/pgx.h "read align" as a plain table) against cases worked out by
hand, against properties that hold for every alignment, against tests/verify_emu.py at W = 0 and against an independently written infix edit
distance without a band; and the seed of the reads tests/test_gpu_align.py cuts: few enough of them are left out."""
import numpy as np
import pytest

import align_cases as C
import align_emu as E
import pgx_workload as W
import verify_emu as V


def _cigar(read, seq, diag, band):
    rec, runs = E.align_one(read, seq, diag, band)
    return E.cigar_text([(n << 4) | op for n, op in runs]), rec


def test_one_edit_by_hand():
    text = b"ACGTACGTAC"
    cigar, rec = _cigar(b"ACGAACGT", text, 0, 2)  # T at 3 substituted
    assert cigar == "3=1X4=" and (rec["edits"], rec["n_match"], rec["n_mismatch"], rec["n_ins"], rec["n_del"]) == (1, 7, 1, 0, 0)
    assert (rec["text_start"], rec["text_end"], rec["band_hit"], rec["n_ops"]) == (0, 8, 0, 3)
    cigar, rec = _cigar(b"ACGTGACGT", text, 0, 2)  # G inserted behind ACGT: the path ends on diagonal -1
    assert cigar == "4=1I4=" and (rec["edits"], rec["n_match"], rec["n_mismatch"], rec["n_ins"], rec["n_del"]) == (1, 8, 0, 1, 0)
    assert (rec["text_start"], rec["text_end"], rec["band_hit"]) == (0, 8, 0)
    cigar, rec = _cigar(b"ACGACGTA", text, 0, 2)  # T at 3 deleted: the path ends on diagonal +1
    assert cigar == "3=1D5=" and (rec["edits"], rec["n_match"], rec["n_mismatch"], rec["n_ins"], rec["n_del"]) == (1, 8, 0, 0, 1)
    assert (rec["text_start"], rec["text_end"], rec["band_hit"]) == (0, 9, 0)
    cigar, rec = _cigar(b"ACGACGTA", text, 0, 1)  # the same with the band's edge on that diagonal
    assert cigar == "3=1D5=" and rec["band_hit"] == 1
    cigar, rec = _cigar(b"ACGACGTA", text, 0, 0)  # and without a band: substitutions only
    assert rec["edits"] == rec["n_mismatch"] == 5 and rec["n_del"] == 0 and rec["band_hit"] == 0 and rec["text_start"] == 0 and rec["text_end"] == 8


def test_gap_in_a_homopolymer_goes_leftmost():
    cigar, rec = _cigar(b"ACGTTTTACGG", b"GGACGTTTTTACGGA", 2, 2)
    assert cigar == "3=1D8=" and (rec["text_start"], rec["text_end"], rec["edits"], rec["n_del"]) == (2, 14, 1, 1)


def test_overhang_and_short_sequences_by_hand():
    cigar, rec = _cigar(b"TTACGTACGTGG", b"ACGTACGT", -2, 3)
    assert cigar == "2S8=2S" and (rec["clip_lo"], rec["clip_hi"], rec["text_start"], rec["text_end"], rec["edits"], rec["n_ops"]) == (2, 2, 0, 8, 0, 3)
    assert _cigar(b"A", b"A", 0, 3)[0] == "1="
    assert _cigar(b"CAG", b"A", -1, 3)[0] == "1S1=1S"
    cigar, rec = _cigar(b"C", b"A", 0, 3)  # D = 1 on diagonals -1 (an insertion) and 0 (a substitution): the smallest |k|
    assert cigar == "1X" and (rec["text_start"], rec["text_end"], rec["edits"]) == (0, 1, 1)
    cigar, rec = _cigar(b"ACGT", b"ACGT", 10, 3)  # no overlap: one soft clip
    assert cigar == "4S" and (rec["clip_lo"], rec["clip_hi"], rec["n_ops"], rec["diag"]) == (0, 4, 1, 10)
    assert all(rec[k] == 0 for k in rec if k not in ("clip_hi", "n_ops", "diag"))
    assert _cigar(b"", b"ACGT", 0, 3) == ("", dict(rec, diag=0, clip_hi=0, n_ops=0))
    res = E.read_align([b"ACGT"], [b"ACGT", b"ACGT"], [None, (0, 0)], 2)
    assert res["reads"]["seq"].tolist() == [E.NO_SEQUENCE, 0] and res["op_offsets"].tolist() == [0, 0, 1] and res["ops"].tolist() == [(4 << 4) | 7]
    assert all(int(res["reads"][0][f]) == 0 for f in E.ALIGN_DTYPE.names if f != "seq") and E.ALIGN_DTYPE.itemsize == 64


def sellers(read, seq):
    """the smallest edit distance of the whole read to a substring of seq: two rows over the text, no band"""
    prev = [0] * (len(seq) + 1)
    for i in range(1, len(read) + 1):
        cur = [prev[0] + 1] + [0] * len(seq)
        for j in range(1, len(seq) + 1):
            hit = read[i - 1] in b"ACGT" and read[i - 1] == seq[j - 1]
            cur[j] = min(prev[j - 1] + (0 if hit else 1), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return min(prev)


def _random_case(rng):
    """a sequence, a read cut from it with up to three edits, and the diagonal it was cut from (overhanging now and then)"""
    alphabet = np.frombuffer(b"ACGT" if rng.random() < 0.8 else b"ACGTNacgt", np.uint8)
    seq = bytes(rng.choice(alphabet, size=int(rng.integers(1, 61))))
    start = int(rng.integers(0, len(seq)))
    read = bytearray(seq[start:start + int(rng.integers(1, 61))])
    for _ in range(int(rng.integers(0, 4))):
        at, kind = int(rng.integers(0, len(read) + 1)), int(rng.integers(0, 3))
        if kind == 0 and at < len(read):
            read[at] = b"ACGT"[int(rng.integers(0, 4))]
        elif kind == 1:
            read.insert(at, b"ACGT"[int(rng.integers(0, 4))])
        elif len(read) > 1 and at < len(read):
            del read[at]
    return seq, bytes(read), start + int(rng.integers(-3, 4))


@pytest.mark.parametrize("band", [0, 1, 2, 3, 7])
def test_properties_on_random_strings(band):
    rng = np.random.default_rng(100 + band)
    gapped = 0
    for _ in range(400):
        seq, read, diag = _random_case(rng)
        rec, runs = E.align_one(read, seq, diag, band)
        lo, hi = max(0, -diag), min(len(read), len(seq) - diag)
        if hi <= lo:
            assert runs == [(len(read), E.OP_S)]
            continue
        m = hi - lo
        assert rec["n_match"] + rec["n_mismatch"] + rec["n_ins"] == m
        assert rec["n_match"] + rec["n_mismatch"] + rec["n_del"] == rec["text_end"] - rec["text_start"]
        assert rec["edits"] == rec["n_mismatch"] + rec["n_ins"] + rec["n_del"]
        inner = [x for x in runs if x[1] != E.OP_S]
        assert inner[0][1] != E.OP_D and inner[-1][1] != E.OP_D and all(a[1] != b[1] for a, b in zip(runs, runs[1:]))
        assert rec["n_ops"] == len(runs) and 0 <= rec["text_start"] <= rec["text_end"] <= len(seq)
        i, j = 0, rec["text_start"]  # the CIGAR applied to the read walks T[text_start, text_end) and meets equal symbols on every = column
        for n, op in runs:
            for _k in range(n):
                if op in (E.OP_EQ, E.OP_X):
                    assert (read[i] in b"ACGT" and read[i] == seq[j]) == (op == E.OP_EQ)
                i += op != E.OP_D
                j += op in (E.OP_EQ, E.OP_X, E.OP_D)
        assert i == len(read) and j == rec["text_end"]
        gapped += rec["n_ins"] + rec["n_del"] > 0
        if band == 0:
            v = V.verify_one(read, seq, diag, 4)
            assert (rec["edits"], rec["n_match"], rec["text_start"], rec["clip_lo"], len(read) - rec["clip_hi"]) == (v["mismatches"], v["matches"], diag + lo, v["span_lo"], v["span_hi"])
        wide, _ = E.align_one(read, seq, diag, len(read) + len(seq))  # a band that cuts nothing: the distance of Q to a substring of the sequence
        assert wide["edits"] == sellers(read[lo:hi], seq) == int(E.infix_distances(read[lo:hi], [seq])[0]) and wide["edits"] <= rec["edits"]
    assert (gapped > 20) == (band > 0)


@pytest.fixture(scope="module")
def collection(tmp_path_factory):
    c = C.COLLECTION
    text = str(tmp_path_factory.mktemp("align_cpu") / "collection.txt")
    W.synth_pangenome_text(text, base_len=c["base_len"], n_hap=c["n_hap"], seed=c["seed"], n_runs=1, n_run_len=(10, 40))
    return [bytes(s) for s in W.load_sequences(text)]


def test_the_seed_leaves_few_reads_out(collection):
    truth, reads = C.cut_reads(collection)
    assert len(reads) == C.N_READS and all(len(r) == C.LENGTH and collection[q][o:o + C.LENGTH] == r for (q, o), r in zip(truth, reads))
    out = C.fewer_edits_elsewhere(C.deleted(reads), collection) | C.fewer_edits_elsewhere(C.inserted(reads), collection)
    assert out.sum() <= C.MAX_LEFT_OUT, int(out.sum())
    for form in (C.deleted(reads), C.inserted(reads)):  # the substring search is the emulator's answer: checked on every tenth read and on those left out
        pick = sorted(set(range(0, C.N_READS, 10)) | set(np.flatnonzero(out).tolist()))
        slow = np.array([int(E.infix_distances(form[r], collection).min()) < 1 for r in pick])
        assert slow.tolist() == C.fewer_edits_elsewhere([form[r] for r in pick], collection).tolist()
        # and where the read was cut it has one edit, a gap: the emulator at the place of the cut
        for r in pick:
            q, o = truth[r]
            rec, runs = E.align_one(form[r], collection[q], o, 8)
            assert rec["edits"] <= 1 and rec["n_ins"] + rec["n_del"] == rec["edits"]
