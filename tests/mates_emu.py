"""Read mates in plain Python: the definitions of include/pgx.h "read mates" as double loops over i and j.  Reads 2k and 2k + 1 are mates A
and B of pair k; each has the candidates of a verify list, of which (seq, diag, seg_score, matches) count.

  compatible    seq_i ^ 1 == seq_j and frag_min <= L[seq_i] - diag_i - diag_j <= frag_max
  solo winner   largest seg_score, then most matches, then the first
  best pair     largest score sum, then largest matches sum, then the smallest i, then the smallest j; n_compatible, n_best (equal in both
                sums), next_score (the largest score sum below the best one's, 0 without)
  PROPER        a compatible pair exists and pair_score + U >= solo_score
  ELECT         the chosen candidate's list record becomes the read's winner record, with n_cand, cand_index, n_tied put in

Nothing here is shared with the library: the kernel spreads the candidates over lanes, shuffles and reduces a monoid; this file loops.
MUTATIONS are deliberate mistakes (tests/test_mates_cpu.py counts what each changes); the default is none."""
import numpy as np

VERIFY_DTYPE = np.dtype([("diag", "<i8"), ("seq", "<u4"), ("n_cand", "<u4"), ("span_lo", "<u4"), ("span_hi", "<u4"), ("matches", "<u4"), ("mismatches", "<u4"),
                         ("seg_start", "<u4"), ("seg_end", "<u4"), ("seg_score", "<u4"), ("seg_mismatches", "<u4"), ("longest_run", "<u4"), ("run_start", "<u4"),
                         ("cand_index", "<u4"), ("n_tied", "<u4")])
MATES_DTYPE = np.dtype([("frag", "<i8"), ("pair_score", "<u4"), ("solo_score", "<u4"), ("cand_a", "<u4"), ("cand_b", "<u4"), ("solo_a", "<u4"), ("solo_b", "<u4"),
                        ("n_compatible", "<u4"), ("n_best", "<u4"), ("next_score", "<u4"), ("pair_matches", "<u4"), ("seq_a", "<u4"), ("seq_b", "<u4"),
                        ("flags", "<u4"), ("reserved", "<u4")])
NO_SEQUENCE = 0xFFFFFFFF
ELECT = 1
PROPER, COMPATIBLE, HAS_A, HAS_B, MOVED_A, MOVED_B = 1, 2, 4, 8, 16, 32
MUTATIONS = ("no_twin", "same_seq", "diag_sign", "lt_min", "lt_max", "tie_swap", "no_penalty")
U32 = 0xFFFFFFFF


def is_twinned(seq_lengths):
    """None when every sequence 2p has a twin 2p + 1 of its length, else the first p without (n_seq // 2 for an odd count)"""
    n = len(seq_lengths)
    for p in range(n // 2):
        if int(seq_lengths[2 * p]) != int(seq_lengths[2 * p + 1]):
            return p
    return n // 2 if n % 2 else None


def frag_of(seq_lengths, ca, cb):
    return int(seq_lengths[int(ca["seq"])]) - int(ca["diag"]) - int(cb["diag"])


def solo_winner(cands):
    """ordinal of the winner of a list of candidates; None for an empty list"""
    win = None
    for k, c in enumerate(cands):
        if win is None or (int(c["seg_score"]), int(c["matches"])) > (int(cands[win]["seg_score"]), int(cands[win]["matches"])):
            win = k
    return win


def mate_pair(seq_lengths, a, b, frag_min, frag_max, penalty, mutation=None):
    """the record of one pair as a dict, from the candidate lists a and b (sequences of VERIFY_DTYPE records or dicts)"""
    assert mutation is None or mutation in MUTATIONS
    fields = lambda cands: [(int(c["seq"]), int(c["diag"]), int(c["seg_score"]), int(c["matches"])) for c in cands]
    compat = []  # (score sum, matches sum, i, j, frag) of every compatible pair
    for i, (qa, da, sa, ma) in enumerate(fields(a)):
        for j, (qb, db, sb, mb) in enumerate(fields(b)):
            if mutation == "same_seq":
                twin = qa == qb
            elif mutation == "no_twin":
                twin = True
            else:
                twin = qa ^ 1 == qb
            frag = int(seq_lengths[qa]) - da - (-db if mutation == "diag_sign" else db)
            lo_ok = frag_min < frag if mutation == "lt_min" else frag_min <= frag
            hi_ok = frag < frag_max if mutation == "lt_max" else frag <= frag_max
            if twin and lo_ok and hi_ok:
                compat.append((sa + sb, ma + mb, i, j, frag))
    sa, sb = solo_winner(a), solo_winner(b)
    solo = (int(a[sa]["seg_score"]) if len(a) else 0) + (int(b[sb]["seg_score"]) if len(b) else 0)
    sa, sb = sa or 0, sb or 0
    rec = dict(frag=0, pair_score=0, solo_score=min(solo, U32), solo_a=sa, solo_b=sb, n_compatible=len(compat), n_best=0, next_score=0, pair_matches=0, reserved=0)
    proper, ci, cj = False, sa, sb
    if compat:
        best = None
        for s, m, i, j, frag in compat:  # (i ascends, then j: the first to reach a key keeps it)
            first, second = (j, i) if mutation == "tie_swap" else (i, j)
            key = (s, m, -first, -second)
            if best is None or key > best[0]:
                best = (key, s, m, i, j, frag)
        _, s, m, i, j, frag = best
        below = [x[0] for x in compat if x[0] < s]
        rec.update(frag=frag, pair_score=min(s, U32), pair_matches=min(m, U32), next_score=min(max(below), U32) if below else 0,
                   n_best=sum(1 for x in compat if (x[0], x[1]) == (s, m)))
        proper = s + (0 if mutation == "no_penalty" else int(penalty)) >= solo
        if proper:
            ci, cj = i, j
    rec.update(cand_a=ci, cand_b=cj, seq_a=int(a[ci]["seq"]) if len(a) else NO_SEQUENCE, seq_b=int(b[cj]["seq"]) if len(b) else NO_SEQUENCE)
    rec["flags"] = ((PROPER if proper else 0) | (COMPATIBLE if compat else 0) | (HAS_A if len(a) else 0) | (HAS_B if len(b) else 0) |
                    (MOVED_A if proper and ci != sa else 0) | (MOVED_B if proper and cj != sb else 0))
    return rec


def elected(cands, chosen):
    """the winner record of a read whose candidates are `cands` (VERIFY_DTYPE array) when candidate `chosen` is elected"""
    w = np.zeros((), VERIFY_DTYPE)
    if len(cands) == 0:
        w["seq"] = NO_SEQUENCE
        return w
    w[...] = cands[chosen]
    key = (int(cands[chosen]["seg_score"]), int(cands[chosen]["matches"]))
    w["n_cand"], w["cand_index"] = len(cands), chosen
    w["n_tied"] = sum(1 for c in cands if (int(c["seg_score"]), int(c["matches"])) == key)
    return w


def read_mates(seq_lengths, cand_offsets, cands, frag_min, frag_max, penalty, flags=0, mutation=None):
    """dict(pairs MATES_DTYPE[n_reads / 2], winners VERIFY_DTYPE[n_reads] with ELECT else None, n_proper, n_compatible, n_moved_a, n_moved_b)"""
    n = len(cand_offsets) - 1
    assert n % 2 == 0 and (mutation == "no_twin" or is_twinned(seq_lengths) is None)
    cands = np.asarray(cands, dtype=VERIFY_DTYPE)
    pairs = np.zeros(n // 2, MATES_DTYPE)
    winners = np.zeros(n, VERIFY_DTYPE) if flags & ELECT else None
    for k in range(n // 2):
        a = cands[int(cand_offsets[2 * k]):int(cand_offsets[2 * k + 1])]
        b = cands[int(cand_offsets[2 * k + 1]):int(cand_offsets[2 * k + 2])]
        rec = mate_pair(seq_lengths, a, b, frag_min, frag_max, penalty, mutation)
        for f in MATES_DTYPE.names:
            pairs[k][f] = rec[f]
        if winners is not None:
            winners[2 * k] = elected(a, rec["cand_a"])
            winners[2 * k + 1] = elected(b, rec["cand_b"])
    fl = pairs["flags"]
    count = lambda bit: int(((fl & bit) != 0).sum())
    return dict(pairs=pairs, winners=winners, n_proper=count(PROPER), n_compatible=count(COMPATIBLE), n_moved_a=count(MOVED_A), n_moved_b=count(MOVED_B))
