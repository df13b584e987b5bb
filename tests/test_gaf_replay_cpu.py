"""CPU tier of the GAF replay (tests/gaf_replay.py; the GPU tier is tests/test_gpu_gaf_replay.py): the checker proves itself on the reads of
tests/replay_cases.py.

  a. the emulators pass: align_emu and walk_emu at the planted candidate of every read at bands 0, 8 and 31 satisfy replay_record, and every
     walk_emu.gaf_line satisfies replay_gaf_line
  b. mutations fail: every change of MUTATIONS / LINE_MUTATIONS to those records and lines makes the checker raise; the number of reads each one
     trips is pinned in TRIPPED (reads the change applies to, reads on which the checker raises)
  c. the cases are not vacuous: the classes of replay_cases.class_counts are pinned by value in EXPECTED_COUNTS and hold at least 10 reads each
     wherever gaps are allowed (bands 8 and 31)
  d. the kept-read bound: on the emulator chain from the oracle's MEMs (located with the oracle, placed by place_emu, verified by verify_emu,
     aligned by align_emu at band 31) every mixed, heavy and byte read has a winner and at least 90 % of the mixed reads are kept by
     replay_cases.kept (CHAIN_KEPT: 279 kept, 21 left out); a kept read has edits <= the planted cost.  kept looks the source stretch up as it is;
     with the stretch widened by the band 218 of the 279 would be kept -- the bound holds for the others just the same, so they are asserted too"""
import os

import numpy as np
import pytest

import align_emu as A
import gaf_replay as G
import oracle_ffi as O
import pgx_workload as W
import place_emu as PE
import replay_cases as C
import verify_emu as V
import walk_emu as E

K = C.CASES
N = len(K.reads)
FLOOR = 10
# band -> the classes of replay_cases.class_counts on the emulators at the planted candidates
EXPECTED_COUNTS = {0: dict(ins=0, dels=0, both=0, clip_lo=16, clip_hi=17, many_steps=17, one_step=14, reverse_step=253, star=20),
                   8: dict(ins=211, dels=206, both=115, clip_lo=16, clip_hi=17, many_steps=15, one_step=14, reverse_step=253, star=20),
                   31: dict(ins=209, dels=206, both=113, clip_lo=16, clip_hi=17, many_steps=15, one_step=14, reverse_step=253, star=20)}
# mutation -> (reads it applies to, reads on which the checker raises), on the records of band 31
TRIPPED = {"a step's orientation bit flipped": (516, 505),  # (the rest: what the slice holds of the flipped node reads the same either way)
           "the step list reversed": (502, 502), "path_start + 1": (516, 516), "path_len - 1": (516, 516), "the first step dropped": (502, 502),
           "the last step dropped": (502, 502), "an idle step added in front": (516, 516), "an idle step added behind": (516, 516),
           "text_start + 1 with the same ops": (516, 516), "an = turned into X": (516, 516), "an I swapped with the neighbouring D": (113, 113),
           "clip_lo + 1": (516, 516), "n_match + 1": (516, 516), "line: hs set to the twin sequence": (516, 516),
           "line: columns 10 and 11 swapped": (516, 360),  # (the rest has no edit: both columns hold the same number)
           "line: the first step's < > flipped": (516, 505), "line: column 8 + 1": (516, 516), "line: column 3 + 1": (516, 516)}
# the emulator chain of test d at band 31: (mixed reads kept, left out)
CHAIN_KEPT = (279, 21)

_one = {}
_memo = {}


def emu_align(cands, band):
    """align_emu.read_align, with every (read, candidate, band) computed once for the module"""
    recs, offs, words = np.zeros(N, A.ALIGN_DTYPE), np.zeros(N + 1, np.uint64), []
    for r in range(N):
        if cands[r] is None or cands[r][0] == A.NO_SEQUENCE:
            recs[r]["seq"] = A.NO_SEQUENCE
        else:
            key = (r, int(cands[r][0]), int(cands[r][1]), band)
            if key not in _one:
                _one[key] = A.align_one(K.reads[r], K.texts[key[1]], key[2], band)
            rec, runs = _one[key]
            recs[r]["seq"] = key[1]
            for f in rec:
                recs[r][f] = rec[f]
            words.extend((length << 4) | op for length, op in runs)
        offs[r + 1] = len(words)
    return dict(reads=recs, op_offsets=offs, ops=np.array(words, dtype=np.uint32))


def emu_walk(align):
    g = K.graph
    visit_length = g["node_length"][(g["path_nodes"] >> np.uint64(1)).astype(np.int64) - 1]
    a = align["reads"]
    return E.read_walk(g["path_offsets"], g["path_nodes"], visit_length, a["seq"], a["text_start"], a["text_end"])


def per_read(align, walk, r):
    """(align record, walk record, steps, operation words) of read r"""
    return (align["reads"][r], walk["reads"][r], walk["steps"][int(walk["step_offsets"][r]):int(walk["step_offsets"][r + 1])].tolist(),
            align["ops"][int(align["op_offsets"][r]):int(align["op_offsets"][r + 1])].tolist())


def planted(band):
    if band not in _memo:
        align = emu_align(K.candidates(), band)
        _memo[band] = align, emu_walk(align)
    return _memo[band]


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases themselves
def test_the_reads_are_what_their_truth_says():
    assert [(k, len(K.of(k))) for k in K.classes] == [("mixed", 300), ("heavy", 120), ("end", 32), ("byte_n", 12), ("byte_lower", 12), ("byte_other", 12), ("none", 14), ("stranger", 6),
                                                      ("node_last", 4), ("node_first", 4), ("node_inside", 8), ("node_whole", 6), ("one_bp", 6)]
    assert K.of("mixed") == list(range(C.N_MIXED)) and K.reads.count(b"") == 1
    texts = K.texts
    assert len(texts) == 16 and all(texts[q + 1] == C.W.revcomp(texts[q]) for q in range(0, 16, 2))
    n_edits = []
    for r in K.of("mixed", "heavy", "byte_"):
        q, o, edits = K.truth[r]
        assert len(K.reads[r]) == C.MIXED_LEN and o >= 0
        src = texts[q][o:o + C.source_length(C.MIXED_LEN, edits)]
        assert C.apply_edits(src, edits) == K.reads[r] and len(C.planted_cells(K.truth[r], C.MIXED_LEN)) >= C.MIXED_LEN + 1
        if K.kind[r] in ("mixed", "heavy"):
            assert (q % 2 == 1) == (r >= C.N_MIXED // 2 if r < C.N_MIXED else r - C.N_MIXED >= C.N_HEAVY // 2) and set(K.reads[r]) <= set(b"ACGT")
            assert len(edits) <= C.MAX_EDITS if r < C.N_MIXED else 3 <= len(edits) <= C.HEAVY_EDITS
            n_edits.append(len(edits))
        # the longest stretch of the read that the edits leave untouched: at least 19 of 150 bases (six insertions of three bases leave 132 bases in
        # seven stretches), so with min_len 12 the source holds a match that a MEM has to cover
        assert len(edits) <= 6 and C.longest_untouched(K.truth[r], C.MIXED_LEN) >= 19
    assert sorted(set(n_edits)) == list(range(C.HEAVY_EDITS + 1)) and (C.MAX_EDITS, C.HEAVY_EDITS) == (2, 6)
    kinds = {k: sum(e[0] == k for r in K.of("mixed", "heavy") for e in K.truth[r][2]) for k in "XID"}
    assert min(kinds.values()) >= 200, kinds
    sizes = {len(e[2]) if e[0] == "I" else e[2] for r in K.of("mixed", "heavy") for e in K.truth[r][2] if e[0] in "ID"}
    assert sizes == {1, 2, 3}
    hangs = sorted((q, o < 0, -o if o < 0 else o + C.END_LEN - len(texts[q])) for q, o, _ in (K.truth[r] for r in K.of("end")))
    assert hangs == sorted((q, front, a) for q in C.END_SEQS for front in (False, True) for a in C.HANG)
    for r in K.of("byte_n"):
        assert 1 <= K.reads[r].count(b"N") <= 3
    for r in K.of("byte_lower"):
        assert 1 <= sum(c in b"acgt" for c in K.reads[r]) <= 3 and K.reads[r].upper() != K.reads[r]
    for r in K.of("byte_other"):
        assert 1 <= sum(c in C.OTHER_BYTES for c in K.reads[r]) <= 3
    assert sorted(len(K.reads[r]) for r in K.of("none")) == [0, 1, 11, 12, 13] + [150] * 9
    for r in K.of("none"):
        assert not any(K.reads[r][i:i + C.MIN_LEN] in t for t in texts for i in range(len(K.reads[r]) - C.MIN_LEN + 1))
    for r in K.of("node_", "one_bp"):
        q, o, _ = K.truth[r]
        vs = [v for v in C.visits(K.graph, q) if v[0] < o + len(K.reads[r]) and v[1] > o]
        assert texts[q][o:o + len(K.reads[r])] == K.reads[r] and len(K.reads[r]) >= C.MIN_LEN
        if K.kind[r] == "node_last":
            assert vs[0][1] == o + 1 and vs[0][1] - vs[0][0] >= 2
        if K.kind[r] == "node_first":
            assert vs[-1][0] == o + len(K.reads[r]) - 1 and vs[-1][1] - vs[-1][0] >= 2
        if K.kind[r] == "node_inside":
            assert len(vs) == 1 and vs[0][0] < o and o + len(K.reads[r]) < vs[0][1]
        if K.kind[r] == "node_whole":
            assert len(vs) == 1 and (vs[0][0], vs[0][1]) == (o, o + len(K.reads[r]))
        if K.kind[r] == "one_bp":
            assert any(a[1] - a[0] == 1 and b[1] - b[0] == 1 for a, b in zip(vs[1:-1], vs[2:-1]))


# ---------------------------------------------------------------------------------------------------------------------------------
# a. the emulators pass
@pytest.mark.parametrize("band", C.BANDS)
def test_the_emulators_replay(band):
    align, walk = planted(band)
    for r in range(N):
        a, w, steps, ops = per_read(align, walk, r)
        G.replay_record(K.reads[r], K.texts, K.node_seq, a, w, steps, ops, band=band, number=r)
        line = E.gaf_line(r + 1, len(K.reads[r]), a, w, steps, ops)
        fields = G.replay_gaf_line(line, K.reads[r], K.node_seq, texts=K.texts, number=r + 1)
        assert (fields is None) == (int(w["n_steps"]) == 0), r
    assert (align["reads"]["seq"] != A.NO_SEQUENCE).sum() == N - len(K.of("none", "stranger"))


def test_the_emulators_replay_across_the_bands():
    for r in range(N):
        cand = K.candidates()[r]
        mism = None if cand is None else V.verify_one(K.reads[r], K.texts[cand[0]], cand[1], 4)["mismatches"]
        G.replay_bands({band: planted(band)[0]["reads"][r] for band in C.BANDS}, mism, number=r)


def test_an_empty_span_and_a_read_without_sequence_replay():
    """a candidate that does not overlap its sequence (the batch never makes one: a MEM's anchor lies inside) and the checker's refusals on it"""
    read, texts = K.reads[0], K.texts
    for diag in (len(texts[2]), len(texts[2]) + 9, -len(read), -len(read) - 3):
        align = A.read_align(texts, [read], [(2, diag)], 8)
        walk = E.read_walk(*_tables(), align["reads"]["seq"], align["reads"]["text_start"], align["reads"]["text_end"])
        a, w, steps, ops = per_read(align, walk, 0)
        assert (int(a["clip_hi"]), int(w["n_steps"]), len(ops)) == (len(read), 0, 1)
        G.replay_record(read, texts, K.node_seq, a, w, steps, ops, band=8, number=0)
        assert G.replay_gaf_line(E.gaf_line(1, len(read), a, w, steps, ops), read, K.node_seq, number=1) is None
        for field, value in (("clip_hi", len(read) - 1), ("clip_lo", 1), ("n_match", 1), ("text_end", 1)):
            bad = {f: int(a[f]) for f in A.ALIGN_DTYPE.names}
            bad[field] = value
            with pytest.raises(AssertionError, match="read 0"):
                G.replay_record(read, texts, K.node_seq, bad, w, steps, ops, band=8, number=0)
        with pytest.raises(AssertionError):
            G.replay_record(read, texts, K.node_seq, a, dict(path_len=0, path_start=0, path_end=0, n_steps=1, seq=2), [2], ops, band=8, number=0)
    none = K.of("none")[0]
    a, w, steps, ops = per_read(*planted(8), none)
    bad = {f: int(a[f]) for f in A.ALIGN_DTYPE.names}
    bad["edits"] = 1
    with pytest.raises(AssertionError, match="read %d, edits" % none):
        G.replay_record(K.reads[none], texts, K.node_seq, bad, w, steps, ops, number=none)
    for line in ("7\t150" + "\t*" * 9 + "\t255\tNM:i:0", "7\t150" + "\t*" * 8 + "\t0\t255", "7\t150" + "\t*" * 9 + "\t0", "7\t149" + "\t*" * 9 + "\t255"):
        with pytest.raises(AssertionError):
            G.replay_gaf_line(line, K.reads[none], K.node_seq, number=7)
    assert G.replay_gaf_line("7\t150" + "\t*" * 9 + "\t255", K.reads[none], K.node_seq, number=7) is None


def _tables():
    g = K.graph
    return g["path_offsets"], g["path_nodes"], g["node_length"][(g["path_nodes"] >> np.uint64(1)).astype(np.int64) - 1]


# ---------------------------------------------------------------------------------------------------------------------------------
# b. mutations fail
def _symbols(ops):
    """(leading clip, the alignment a symbol a letter, trailing clip) of operation words"""
    ops = [(int(x) >> 4, G.KINDS[int(x) & 15]) for x in ops]
    lead = ops.pop(0)[0] if ops and ops[0][1] == "S" else 0
    trail = ops.pop()[0] if ops and ops[-1][1] == "S" else 0
    return lead, "".join(k * n for n, k in ops), trail


def _words(lead, symbols, trail):
    code = {v: k for k, v in G.KINDS.items()}
    runs = [[lead, "S"]] if lead else []
    for k in symbols:
        if runs and runs[-1][1] == k and k != "S":
            runs[-1][0] += 1
        else:
            runs.append([1, k])
    if trail:
        runs.append([trail, "S"])
    return [n << 4 | code[k] for n, k in runs]


def _node_len(step):
    return len(K.node_seq[step >> 1])


def _m_flip(a, w, steps, ops):
    return a, w, [steps[0] ^ 1] + steps[1:], ops


def _m_reverse(a, w, steps, ops):
    return (a, w, steps[::-1], ops) if len(steps) > 1 else None


def _m_path_start(a, w, steps, ops):
    return a, dict(w, path_start=w["path_start"] + 1), steps, ops


def _m_path_len(a, w, steps, ops):
    return a, dict(w, path_len=w["path_len"] - 1), steps, ops


def _m_drop_first(a, w, steps, ops):
    return (a, dict(w, n_steps=w["n_steps"] - 1), steps[1:], ops) if len(steps) > 1 else None


def _m_drop_last(a, w, steps, ops):
    return (a, dict(w, n_steps=w["n_steps"] - 1), steps[:-1], ops) if len(steps) > 1 else None


def _m_idle_first(a, w, steps, ops):
    n = _node_len(steps[0])  # one more visit in front, the offsets moved with it: the slice still spells the text
    return a, dict(w, n_steps=w["n_steps"] + 1, path_len=w["path_len"] + n, path_start=w["path_start"] + n, path_end=w["path_end"] + n), steps[:1] + steps, ops


def _m_idle_last(a, w, steps, ops):
    return a, dict(w, n_steps=w["n_steps"] + 1, path_len=w["path_len"] + _node_len(steps[-1])), steps + steps[-1:], ops


def _m_text_start(a, w, steps, ops):
    return dict(a, text_start=a["text_start"] + 1), w, steps, ops


def _m_eq_to_x(a, w, steps, ops):
    lead, sym, trail = _symbols(ops)
    at = sym.find("=")
    if at < 0:
        return None
    new = _words(lead, sym[:at] + "X" + sym[at + 1:], trail)  # (the totals move with it: only the read and the text can tell)
    return dict(a, n_match=a["n_match"] - 1, n_mismatch=a["n_mismatch"] + 1, edits=a["edits"] + 1, n_ops=len(new)), w, steps, new


def _m_swap_i_d(a, w, steps, ops):
    kinds = [G.KINDS[x & 15] for x in ops]
    if "I" not in kinds or "D" not in kinds:
        return None
    i = kinds.index("I")
    d = min((k for k, x in enumerate(kinds) if x == "D"), key=lambda k: abs(k - i))
    new = list(ops)
    new[i], new[d] = new[d], new[i]
    return a, w, steps, new


def _m_clip_lo(a, w, steps, ops):
    return dict(a, clip_lo=a["clip_lo"] + 1), w, steps, ops


def _m_n_match(a, w, steps, ops):
    return dict(a, n_match=a["n_match"] + 1), w, steps, ops


MUTATIONS = [("a step's orientation bit flipped", _m_flip), ("the step list reversed", _m_reverse), ("path_start + 1", _m_path_start), ("path_len - 1", _m_path_len),
             ("the first step dropped", _m_drop_first), ("the last step dropped", _m_drop_last), ("an idle step added in front", _m_idle_first),
             ("an idle step added behind", _m_idle_last), ("text_start + 1 with the same ops", _m_text_start), ("an = turned into X", _m_eq_to_x),
             ("an I swapped with the neighbouring D", _m_swap_i_d), ("clip_lo + 1", _m_clip_lo), ("n_match + 1", _m_n_match)]


def _l_hs_twin(cols):
    cols[13] = "hs:i:%d" % (int(cols[13][5:]) ^ 1)


def _l_swap_10_11(cols):
    cols[9], cols[10] = cols[10], cols[9]


def _l_flip(cols):
    cols[5] = "<>"[cols[5][0] == "<"] + cols[5][1:]


def _l_path_start(cols):
    cols[7] = str(int(cols[7]) + 1)


def _l_qstart(cols):
    cols[2] = str(int(cols[2]) + 1)


LINE_MUTATIONS = [("line: hs set to the twin sequence", _l_hs_twin), ("line: columns 10 and 11 swapped", _l_swap_10_11), ("line: the first step's < > flipped", _l_flip),
                  ("line: column 8 + 1", _l_path_start), ("line: column 3 + 1", _l_qstart)]


def test_every_mutation_is_caught():
    align, walk = planted(31)
    table = {}
    for name, mutate in MUTATIONS:
        applies = tripped = 0
        for r in range(N):
            a, w, steps, ops = per_read(align, walk, r)
            if int(w["n_steps"]) == 0:
                continue
            out = mutate({f: int(a[f]) for f in A.ALIGN_DTYPE.names}, {f: int(w[f]) for f in E.WALK_DTYPE.names}, list(steps), list(ops))
            if out is None:
                continue
            applies += 1
            try:
                G.replay_record(K.reads[r], K.texts, K.node_seq, *out, band=31, number=r)
            except AssertionError as e:
                assert str(e).startswith("read %d, " % r)
                tripped += 1
        table[name] = (applies, tripped)
    for name, mutate in LINE_MUTATIONS:
        applies = tripped = 0
        for r in range(N):
            a, w, steps, ops = per_read(align, walk, r)
            if int(w["n_steps"]) == 0:
                continue
            cols = E.gaf_line(r + 1, len(K.reads[r]), a, w, steps, ops).split("\t")
            mutate(cols)
            applies += 1
            try:
                G.replay_gaf_line("\t".join(cols), K.reads[r], K.node_seq, texts=K.texts, number=r + 1)
            except AssertionError:
                tripped += 1
        table[name] = (applies, tripped)
    for name, (applies, tripped) in table.items():
        print("%-40s applies to %3d reads, trips %3d" % (name, applies, tripped))
    assert all(tripped >= 1 for _, tripped in table.values()), table
    assert table == TRIPPED


# ---------------------------------------------------------------------------------------------------------------------------------
# c. the cases are not vacuous
@pytest.mark.parametrize("band", C.BANDS)
def test_the_classes_are_reached_in_the_pinned_counts(band):
    align, walk = planted(band)
    counts = C.class_counts(align["reads"], walk["reads"], [per_read(align, walk, r)[2] for r in range(N)])
    print("band %d: %r" % (band, counts))
    assert counts == EXPECTED_COUNTS[band]
    if band > 0:  # (band 0 knows no gap)
        assert min(counts.values()) >= FLOOR, counts
    assert counts["star"] == len(K.of("none", "stranger"))


# ---------------------------------------------------------------------------------------------------------------------------------
# d. the kept-read bound on the emulator chain
def _chain(workdir):
    """oracle MEMs (min_len 12, min_occ 1) and their positions -> place_emu -> verify_emu (one candidate, penalty 4): the verify records"""
    if "chain" in _memo:
        return _memo["chain"]
    path = os.path.join(workdir, "replay_graph.txt")
    with open(path, "wb") as f:
        f.write(b"".join(t + b"\n" for t in K.texts))
    ri = O.RIndex(W.build_index_from_text(path, workdir, "replay_graph", with_tags=False)[0])
    mem_offsets, mems, loc_offsets, values = [0], [], [0], []
    for read in K.reads:
        for m in ri.find_all_mems(read, C.MIN_LEN, 1, mode=O.MODE_STRICT):
            mems.append(m)
            values += ri.locate_sa(m[2], m[2] + m[3] - 1, mode=O.MODE_STRICT).tolist()
            loc_offsets.append(len(values))
        mem_offsets.append(len(mems))
    place = PE.read_place(np.array(mem_offsets, np.uint64), np.array(mems, dtype=PE.MEM_DTYPE).reshape(-1), np.array(loc_offsets, np.uint64),
                          np.array(values, np.uint64), ri.max_length)
    _memo["chain"] = V.read_verify(K.texts, K.reads, V.candidates_from_places(place, 1), 4)["reads"]
    return _memo["chain"]


def test_the_emulator_chain_keeps_nine_mixed_reads_in_ten(workdir):
    verified = _chain(workdir)
    mixed = K.of("mixed")
    assert (verified["seq"][K.of("mixed", "heavy", "byte_")] != V.NO_SEQUENCE).all()  # every mixed read keeps an untouched stretch of 19 bases or more: it has a MEM, so a winner
    assert (verified["seq"][K.of("none")] == V.NO_SEQUENCE).all()
    align = emu_align(A.candidates_from_verified(verified), 31)
    walk = emu_walk(align)
    for r in range(N):  # the chain's winners replay too, whichever haplotype they are
        G.replay_record(K.reads[r], K.texts, K.node_seq, *per_read(align, walk, r), band=31, number=r)
    n_keep, n_out, n_wide = C.check_kept_bound(K, align["reads"], 31, mixed, capped=True)
    heavy = C.check_kept_bound(K, align["reads"], 31, K.of("heavy", "byte_"), capped=False)
    print("emulator chain, band 31: %d of %d mixed reads kept, %d left out (%d kept with the stretch widened by the band); heavy and byte reads: %d kept, "
          "%d left out" % (n_keep, len(mixed), n_out, n_wide, heavy[0], heavy[1]))
    assert (n_keep, n_out) == CHAIN_KEPT and n_out <= C.MAX_LEFT_OUT == 30
    # at the planted candidates nothing is left out, even with the stretch widened, and the bound holds for every read with a truth
    align, _ = planted(31)
    for r in range(N):
        if K.truth[r] is not None and K.kind[r] != "end":
            assert C.kept(K.texts, K.truth[r], len(K.reads[r]), align["reads"][r], 31, widen=31), r
            assert int(align["reads"]["edits"][r]) <= C.planted_cost(K.truth[r][2]), r
