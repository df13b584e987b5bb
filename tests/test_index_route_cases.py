"""CPU tier of the index-route case tables (index_route_cases.py; the GPU tiers are test_gpu_text_image_borders.py and
test_gpu_index_route_borders.py): every table holds the borders it claims, by number; every TEXT_CASES entry builds with the host builder
and opens (pgx_index_open needs no device); the intended placement of every read of READ_CASES follows from the text alone; the emulators
on the truth candidates reach every border class in the counts pinned in EXPECTED_COUNTS, which the GPU tier re-asserts; and the mutation
check, argued by restating each change in the emulators (never by running a changed kernel):

  (a) Ls without `- endmark` in pgx_verify_kernel   = verify_emu on every sequence with its endmarker appended (a symbol that matches nothing)
  (b) the same in align_span                        = align_emu on the same lengthened sequences
  (c) lo not clipped at 0                           = verify_emu on the sequence with the -diag text symbols before it in front, at diagonal 0
  (d) the endmarker code equal to the code of N     = the text image with N where the endmarkers are (pgx_text_mark_kernel skipped)

(d) cannot change a read record, whatever the reads: a read code is one of 1 2 3 5 15 (pgx_verify_code_kernel) and neither the endmarker code
0 nor the code of N, 4, is among them, so a text position that holds either mismatches every read byte both ways; and with Ls right no
compared position is an endmarker in the first place.  The test asserts that 0, also on top of (a) and (b), and counts what (d) does change:
the bytes of pgx_index_text, which is what tests/test_gpu_text_image_borders.py compares on every case of TEXT_CASES.

The golden bidirectional_test/reads.txt holds no read that hangs over a sequence end: the last test decides that by trying every diagonal."""
import os

import numpy as np
import pytest

import align_emu as A
import index_route_cases as C
import pgx_ffi as P
import pgx_workload as W
import verify_emu as V

R = C.READ_CASES
NAMES = list(C.TEXT_CASES)


# ---------------------------------------------------------------------------------------------------------------------------------
# TEXT_CASES
def test_the_groups_and_their_cases():
    assert {g: len(v) for g, v in C.TEXT_GROUPS.items()} == dict(totals=14, n_seq=8, word_borders=8, n_symbols=7, longest=4, identical=4, empty=3, reads=1)
    assert sorted(sum(C.TEXT_GROUPS.values(), [])) == sorted(NAMES) and len(NAMES) == 49
    assert len(C.PGI_CASES) == len(C.TEXT_GROUPS) and all(n in C.TEXT_CASES for n in C.PGI_CASES)
    for name, raw in C.TEXT_CASES.items():
        assert 0 < len(raw) <= 20000 and raw.endswith(b"\n") and set(raw) <= set(b"ACGTN\n"), name
        assert set(b"ACGT") <= set(raw), name  # (an index opens only then)
    for group, names in C.TEXT_GROUPS.items():  # both routes of the text image can run on every group
        big = [n for n in names if C.is_bidirectional(C.TEXT_CASES[n]) and len(C.TEXT_CASES[n]) >= C.LCE_MIN]
        assert big, group


def test_totals_lie_on_every_residue_and_around_the_blocks():
    totals = [len(C.TEXT_CASES[n]) for n in C.TEXT_GROUPS["totals"]]
    assert totals == list(C.RESIDUE_TOTALS + C.BLOCK_TOTALS)
    assert sorted(t % 8 for t in C.RESIDUE_TOTALS) == list(range(8)) and min(C.RESIDUE_TOTALS) > 2 * 2048
    assert C.BLOCK_TOTALS == (2047, 2048, 2049, 4095, 4096, 4097)  # one block of the pack / unpack kernels: 256 words of 8 symbols
    assert [(t + 7) // 8 for t in C.BLOCK_TOTALS] == [256, 256, 257, 512, 512, 513]
    for n in C.TEXT_GROUPS["totals"]:
        raw = C.TEXT_CASES[n]
        assert C.is_bidirectional(raw) == (len(raw) % 2 == 0) and b"N" in raw, n


def test_sequence_counts_lie_around_the_blocks_of_the_mark_kernel():
    counts = {n: C.TEXT_CASES[n].count(b"\n") for n in C.TEXT_GROUPS["n_seq"]}
    assert counts == {"n_seq_%d" % k: k for k in C.SEQ_COUNTS_FORWARD + C.SEQ_COUNTS_PAIRED}
    assert C.SEQ_COUNTS_FORWARD == (1, 255, 257) and C.SEQ_COUNTS_PAIRED == (2, 256, 510, 512, 514)
    assert [(k + 255) // 256 for k in (1, 2, 255, 256, 257, 510, 512, 514)] == [1, 1, 1, 1, 2, 2, 2, 3]  # blocks of 256 threads
    for k in C.SEQ_COUNTS_FORWARD:  # forward-only with an odd count
        assert k % 2 == 1 and not C.is_bidirectional(C.TEXT_CASES["n_seq_%d" % k])
    for k in C.SEQ_COUNTS_PAIRED:
        raw = C.TEXT_CASES["n_seq_%d" % k]
        assert C.is_bidirectional(raw) and len(raw) >= C.LCE_MIN, k


def test_sequence_ends_and_starts_lie_on_every_residue_of_a_word():
    last_at, start_at = set(), set()
    for r in range(8):
        raw = C.TEXT_CASES["ends_%d" % r]
        st, seqs = C.starts(raw), C.split(raw)
        assert C.is_bidirectional(raw) and len(seqs) == 6
        assert (st[2] + len(seqs[2]) - 1) % 8 == r and raw[st[2] + len(seqs[2])] == 10  # the last symbol, then its endmarker
        assert st[3] % 8 == (r + 2) % 8 and st[3] > 0
        last_at.add((st[2] + len(seqs[2]) - 1) % 8)
        start_at.add(st[3] % 8)
    assert last_at == start_at == set(range(8))  # 7 and 0 among them, for last symbols and for starts


def test_n_lies_next_to_endmarkers():
    t = C.TEXT_CASES
    assert b"N\n" in t["n_before_end"] and b"NN\n" in t["n_before_end"] and b"\nN" in t["n_before_end"]
    assert t["n_first"].startswith(b"N") and t["n_first"][1:2] != b"N" and b"N\n" in t["n_first"]
    assert b"\nNNNNNNNNN\nNNNNNNNNN\n" in t["all_n"]
    assert b"\nN\nN\n" in t["n_alone"]
    assert t["n_alone_first_last"].startswith(b"N\nN\n") and t["n_alone_first_last"].endswith(b"\nN\nN\n")
    assert b"\nG\nC\nA\nT\n" in t["length_one"] and t["length_one"].endswith(b"\nT\nA\n")
    small = C.split(t["small_with_n"])
    assert small == [b"ACGTN", b"NACGT", b"N", b"N", b"NNN", b"NNN", b"G", b"C", b"NACGT", b"ACGTN"] and len(t["small_with_n"]) < C.LCE_MIN
    for n in C.TEXT_GROUPS["n_symbols"]:
        assert C.is_bidirectional(t[n]), n


def test_the_longest_sequence_lies_first_last_and_in_the_middle():
    where = {}
    for n in C.TEXT_GROUPS["longest"]:
        lens = [len(s) for s in C.split(C.TEXT_CASES[n])]
        top = max(lens)
        assert top - 1 in lens, n  # a sequence exactly one symbol shorter
        where[n] = [k for k, ln in enumerate(lens) if ln == top], len(lens)
    assert where == dict(longest_first=([0, 1], 6), longest_last=([4, 5], 6), longest_middle=([2, 3], 8), longest_forward_only=([1], 3))


def test_identical_sequences_and_empty_ones():
    for c in C.IDENTICAL:
        seqs = C.split(C.TEXT_CASES["identical_%d" % c])
        assert len(seqs) == c and len(set(seqs)) == 1
        assert C.is_bidirectional(C.TEXT_CASES["identical_%d" % c]) == (c % 2 == 0)
    assert C.IDENTICAL == (2, 3, 256, 257)
    assert [len(s) for s in C.split(C.TEXT_CASES["empty_between"])][:8] == [7, 7, 0, 0, 8, 8, 0, 0]
    e = C.split(C.TEXT_CASES["empty_first_last"])
    assert [len(s) for s in e] == [0, 0, 2100, 2100, 0, 0, 0, 0]
    assert C.TEXT_CASES["empty_small"] == b"ACGT\n\nACGT\n\n"


@pytest.mark.parametrize("name", NAMES)
def test_every_text_case_builds_and_opens(workdir, name):
    raw = C.TEXT_CASES[name]
    path = os.path.join(workdir, "irc_%s.txt" % name)
    with open(path, "wb") as f:
        f.write(raw)
    for encoded in (True, False):
        ri = W.build_index_from_text(path, workdir, "irc_" + name, encoded=encoded, with_tags=False)[0]
        idx = P.Index(ri, mode=P.MODE_STRICT)
        info = idx.info()
        assert (int(info.bwt_size), int(info.n_sequences), bool(info.is_encoded)) == (len(raw), raw.count(b"\n"), encoded)
        idx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# READ_CASES
def _occurrences(needle):
    """every (seq, offset) of needle in the collection (the newline between two sequences is in no read)"""
    out, at = [], R.raw.find(needle)
    while at >= 0:
        q = int(np.searchsorted(R.starts, at, side="right")) - 1
        out.append((q, at - R.starts[q]))
        at = R.raw.find(needle, at + 1)
    return out


def test_the_collection_of_the_reads():
    lens = [len(s) for s in R.seqs]
    assert lens[0::2] == lens[1::2] == list(C.FORWARD_LENGTHS) and C.is_bidirectional(R.raw) and R.n_seq == 24
    assert {1, 8, 9, 23, 40} <= set(lens) and sum(200 <= ln <= 400 for ln in C.FORWARD_LENGTHS) >= 6
    assert lens[0] >= 200 and lens[-1] >= 200 and len(R.raw) >= C.LCE_MIN  # a read can hang over text offset 0 and over the end of the text
    a, b = R.seqs[2 * C.A_FWD], R.seqs[2 * C.B_FWD]
    assert b[:len(a)] == a and len(b) == len(a) + C.EXTRA == len(a) + 60
    assert len(R.reads) == len(R.truth) == len(R.kinds) == 286 <= 400
    assert all(30 <= len(r) <= 80 for r in R.reads if r) and R.reads.count(b"") == 1


def test_every_core_occurs_where_it_was_cut_and_nowhere_else():
    for r, (read, truth, core) in enumerate(zip(R.reads, R.truth, R.core)):
        if truth is None:
            assert core is None
            continue
        a, b = core
        assert b - a >= 20, r
        want = sorted((q, diag + a) for q, diag in ([truth] if isinstance(truth, tuple) else truth))
        assert R.raw.count(read[a:b]) == len(want) == (1 if isinstance(truth, tuple) else 2), r
        assert sorted(_occurrences(read[a:b])) == want, r


def test_no_junk_base_lengthens_a_core_and_no_other_mem_exists():
    for r, (read, truth, core) in enumerate(zip(R.reads, R.truth, R.core)):
        places = [] if truth is None else [truth] if isinstance(truth, tuple) else truth
        for q, diag in places:  # the read bytes next to the core differ from the text symbol they face (the endmarker differs from all)
            for i in (core[0] - 1, core[1]):
                if 0 <= i < len(read) and 0 <= diag + i < len(R.seqs[q]):
                    assert read[i] != R.seqs[q][diag + i], (r, i)
            assert read[core[0]:core[1]] == R.seqs[q][diag + core[0]:diag + core[1]], r
        # every MIN_LEN symbols of the read that occur in the text lie on an intended diagonal: the place stage has nothing else to score
        for i in range(len(read) - C.MIN_LEN + 1):
            for q, off in _occurrences(read[i:i + C.MIN_LEN]):
                assert (q, off - i) in places, (r, i, q, off)
        if truth is None:
            assert all(R.raw.find(read[i:i + C.MIN_LEN]) < 0 for i in range(max(len(read) - C.MIN_LEN + 1, 0))), r


def test_every_overhang_class_is_present():
    kinds = {k: R.kinds.count(k) for k in set(R.kinds)}
    assert kinds == dict(both=62, exact_end=14, exact_start=14, inside=9, ab_end=9, ab_start=9, del_end=9, ins_end=9, del_start=9, ins_start=9, del3_end=3, ins3_start=3, no_mem=6,
                         empty=1, **{"%s_%d" % (side, a): 15 for side in ("front", "back") for a in C.JUNK})
    last = R.n_seq - 1
    for r, (read, truth, kind) in enumerate(zip(R.reads, R.truth, R.kinds)):
        if kind.startswith("front_"):
            assert truth[1] == -int(kind[6:]) and truth[1] + len(read) <= len(R.seqs[truth[0]])
        if kind.startswith("back_"):
            assert truth[1] > 0 and truth[1] + len(read) - len(R.seqs[truth[0]]) == int(kind[5:])
        if kind == "both":
            assert -truth[1] in C.JUNK and truth[1] + len(read) - len(R.seqs[truth[0]]) in C.JUNK and len(R.seqs[truth[0]]) < len(read)
        if kind == "exact_end":
            assert truth[1] >= 0 and truth[1] + len(read) == len(R.seqs[truth[0]])
        if kind == "exact_start":
            assert truth[1] == 0 and len(read) <= len(R.seqs[truth[0]])
    for side in ("front", "back"):  # both kinds on sequence 0 and on the last sequence, with every junk length
        for q in (0, last):
            assert {k for k, t in zip(R.kinds, R.truth) if k.startswith(side) and t[0] == q} == {"%s_%d" % (side, a) for a in C.JUNK}
    assert {t[0] for k, t in zip(R.kinds, R.truth) if k == "both"} == {8, 9, 10, 11}
    for kind in ("del_end", "ins_end", "del_start", "ins_start", "del3_end", "ins3_start"):
        assert {t[0] for k, t in zip(R.kinds, R.truth) if k == kind} == {0, 16, last}


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulators on the truth candidates
_memo = {}


def _truth_verify(max_cand, penalty, seqs=None):
    """verify_emu at the candidates of the table; seqs: other sequences in their place (the mutations), not kept"""
    cands = [C.truth_candidates(t, max_cand) for t in R.truth]
    if seqs is not None:
        return V.read_verify(seqs, R.reads, cands, penalty)
    if ("v", max_cand, penalty) not in _memo:
        _memo[("v", max_cand, penalty)] = V.read_verify(R.seqs, R.reads, cands, penalty)
    return _memo[("v", max_cand, penalty)]


def _truth_align(band, seqs=None):
    cands = A.candidates_from_verified(_truth_verify(16, 4)["reads"])
    if seqs is not None:
        return A.read_align(seqs, R.reads, cands, band)
    if ("a", band) not in _memo:
        _memo[("a", band)] = A.read_align(R.seqs, R.reads, cands, band)
    return _memo[("a", band)]


def test_the_emulators_name_the_truth_as_the_winner():
    for max_cand in C.MAX_CANDS:
        for penalty in C.PENALTIES:
            v = _truth_verify(max_cand, penalty)["reads"]
            for r, truth in enumerate(R.truth):
                want = C.winner_truth(truth, max_cand)
                got = None if int(v["seq"][r]) == V.NO_SEQUENCE else (int(v["seq"][r]), int(v["diag"][r]))
                assert got == want, (max_cand, penalty, r, R.kinds[r])
                if isinstance(truth, list) and max_cand > 1:
                    assert int(v["n_cand"][r]) == 2 and int(v["cand_index"][r]) == 1 and int(v["n_tied"][r]) == 1


@pytest.mark.parametrize("band", C.BANDS)
def test_the_border_classes_are_reached_in_the_pinned_counts(band):
    v, a = _truth_verify(16, 4)["reads"], _truth_align(band)["reads"]
    counts = C.border_counts([len(s) for s in R.seqs], [len(x) for x in R.reads], v, a)
    print("band %d: %r" % (band, counts))
    assert counts == C.EXPECTED_COUNTS[band]
    assert all(counts[k] > 0 for k in counts if k != "band_hit") and (counts["band_hit"] > 0) == (band in (1, 3))  # (a run of 8 edits never beats the mismatches it avoids)
    assert counts["no_sequence"] == sum(t is None for t in R.truth)


def _changed(a, b):
    return int((a != b).sum())


def test_mutation_counts():
    """the number of read records of READ_CASES that each mutation of the module docstring changes"""
    v, al = _truth_verify(16, 4), _truth_align(8)
    longer = [s + b"\n" for s in R.seqs]  # Ls without `- endmark`: the endmarker is one more symbol, and it matches nothing
    n_a = _changed(_truth_verify(16, 4, seqs=longer)["reads"], v["reads"])
    n_b = _changed(_truth_align(8, seqs=longer)["reads"], al["reads"])
    # (c) lo = 0 whatever the diagonal: the read's first -diag bytes face the text before the sequence (nothing before text offset 0: the kernel's
    # tw >= 0 guard gives the endmarker code there)
    n_c = 0
    for r, rec in enumerate(v["reads"]):
        q, diag = int(rec["seq"]), int(rec["diag"])
        if q == V.NO_SEQUENCE:
            continue
        before = (b"\n" * -diag + R.raw[:R.starts[q]])[diag:] if diag < 0 else b""
        mut = V.verify_one(R.reads[r], before + R.seqs[q], diag + len(before), 4)
        n_c += any(int(rec[f]) != mut[f] for f in ("span_lo", "span_hi", "matches", "mismatches", "seg_start", "seg_end", "seg_score", "longest_run"))
    # (d) N where the endmarkers are: the sequences the kernels compare are the same symbols, and on top of (a) / (b) the one more symbol is an N,
    # which matches nothing either
    as_n = R.raw.replace(b"\n", b"N")
    same = [as_n[s:s + len(x)] for s, x in zip(R.starts, R.seqs)]
    n_d = _changed(_truth_verify(16, 4, seqs=same)["reads"], v["reads"]) + _changed(_truth_align(8, seqs=same)["reads"], al["reads"])
    n_d_on_a = _changed(_truth_verify(16, 4, seqs=[s + b"N" for s in R.seqs])["reads"], _truth_verify(16, 4, seqs=longer)["reads"])
    n_d_text = sum(x != y for x, y in zip(as_n, R.raw))
    n_d_cases = sum(b"N\n" in raw for raw in C.TEXT_CASES.values())
    print("mutation counts over the %d reads: (a) %d verify records, (b) %d align records, (c) %d verify records, (d) %d read records, "
          "%d bytes of the text image, %d TEXT_CASES with an N before an endmarker" % (len(R.reads), n_a, n_b, n_c, n_d, n_d_text, n_d_cases))
    assert (n_a, n_b, n_c) == C.MUTATION_COUNTS and min(n_a, n_b, n_c) > 0
    assert n_d == 0 and n_d_on_a == 0  # (cannot be otherwise: the module docstring)
    assert n_d_text == R.n_seq > 0 and n_d_cases >= 3


def test_no_golden_xy_read_hangs_over_a_sequence_end(golden):
    """every diagonal of every sequence: the placements with the most matches all hold the whole read, and no end of a read of three symbols
    or more is the start or the end of a sequence"""
    bt = os.path.join(golden, "bidirectional_test")
    seqs = C.split(open(os.path.join(bt, "contigs_xy"), "rb").read())
    reads = [x for x in open(os.path.join(bt, "reads.txt"), "rb").read().split(b"\n") if x]
    assert len(reads) == 5
    for read in reads:
        best, partial = 0, False
        for s in seqs:
            for diag in range(-len(read) + 1, len(s)):
                lo, hi = max(0, -diag), min(len(read), len(s) - diag)
                m = sum(read[i] == s[diag + i] for i in range(lo, hi))
                if m > best:
                    best, partial = m, False
                if m == best and (lo > 0 or hi < len(read)):
                    partial = True
            assert not any(s.endswith(read[:k]) or s.startswith(read[-k:]) for k in range(3, len(read)))
        assert best > 0 and not partial
