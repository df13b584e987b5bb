"""Read rescue in plain Python: the definitions of include/pgx.h "read rescue" as loops over reads, anchors and diagonals.  Reads 2k and
2k + 1 are mates; each has the candidates of a verify list.

  target        the pair has no compatible candidate pair (mates_emu.mate_pair under the call's frag bounds), the mate has a candidate and
                the read has fewer than 64; with 64 it is FULL and no target
  anchors       the mate's candidates equal to its solo winner in (seg_score, matches), in candidate order, the first max_anchors
  task          sequence s = seq_i ^ 1, diagonals d with frag_min <= L[s] - diag_i - d <= frag_max and -(len - 1) <= d <= L[s] - 1
  score         verify's (seg_score, matches) of the read at (s, d): verify_emu.match_string, and the segment score by the linear recurrence
                E = max(E, 0) + (1 or -P), which test_rescue_cpu.py holds against verify_emu.verify_one's quadratic search
  best          largest seg_score, then most matches, then the smallest anchor ordinal, then the smallest d; n_diags, n_best, next_score
  RESCUED       n_diags > 0 and seg_score >= min_score
  MERGE         the best diagonal of a RESCUED read becomes the last candidate of its list, as verify_emu.verify_one writes it; the winners
                are recomputed by verify's rule

Nothing here is shared with the library: the kernels walk packed words a lane a diagonal and merge a monoid; this file loops.
MUTATIONS are deliberate mistakes (tests/test_rescue_cpu.py counts what each changes); the default is none."""
import numpy as np

import mates_emu as M
import verify_emu as V

VERIFY_DTYPE = V.VERIFY_DTYPE
RESCUE_DTYPE = np.dtype([("diag", "<i8"), ("n_diags", "<u8"), ("seq", "<u4"), ("flags", "<u4"), ("anchor", "<u4"), ("n_anchors", "<u4"), ("seg_score", "<u4"),
                         ("matches", "<u4"), ("n_best", "<u4"), ("next_score", "<u4"), ("reserved", "<u4", (4,))])
NO_SEQUENCE = 0xFFFFFFFF
MERGE = 1
TARGET, RESCUED, FULL = 1, 2, 4
MAX_CAND, MAX_ANCHORS, MAX_WINDOW = 64, 8, 65536
MUTATIONS = ("win_lo", "win_hi", "clip_lo", "clip_hi", "tie_large_d", "all_anchors", "gt_min", "merge_first")
U32 = 0xFFFFFFFF


def score_diag(read, seq, diag, penalty):
    """(seg_score, matches) of the read on diagonal diag of seq"""
    _, _, m = V.match_string(read, seq, diag)
    e = best = 0
    for x in m:
        e = max(e, 0) + (1 if x else -int(penalty))
        best = max(best, e)
    return best, sum(m)


def window(seq_len, read_len, anchor_diag, frag_min, frag_max, mutation=None):
    """(d_lo, d_hi) of a task, d_hi < d_lo when it is empty"""
    lo = seq_len - anchor_diag - frag_max + (1 if mutation == "win_lo" else 0)
    hi = seq_len - anchor_diag - frag_min - (1 if mutation == "win_hi" else 0)
    lo = max(lo, -(read_len - 1) + (1 if mutation == "clip_lo" else 0))
    hi = min(hi, seq_len - 1 - (1 if mutation == "clip_hi" else 0))
    if read_len == 0 or hi < lo:
        return 0, -1
    return lo, hi


def anchors_of(mate_cands, solo, max_anchors, mutation=None):
    """ordinals of the anchors among the mate's candidates"""
    key = (int(mate_cands[solo]["seg_score"]), int(mate_cands[solo]["matches"]))
    out = [i for i, c in enumerate(mate_cands) if mutation == "all_anchors" or (int(c["seg_score"]), int(c["matches"])) == key]
    return out[:max_anchors]


def rescue_read(seqs, read, own_count, mate_cands, solo, frag_min, frag_max, penalty, min_score, max_anchors, mutation=None):
    """the record of a read in a pair without a compatible candidate pair, as a dict"""
    rec = dict(diag=0, n_diags=0, seq=NO_SEQUENCE, flags=0, anchor=0, n_anchors=0, seg_score=0, matches=0, n_best=0, next_score=0)
    if len(mate_cands) == 0:
        return rec
    if own_count >= MAX_CAND:
        rec["flags"] = FULL
        return rec
    anchors = anchors_of(mate_cands, solo, max_anchors, mutation)
    scored = []  # (seg_score, matches, anchor, d, seq)
    for i in anchors:
        s = int(mate_cands[i]["seq"]) ^ 1
        lo, hi = window(len(seqs[s]), len(read), int(mate_cands[i]["diag"]), frag_min, frag_max, mutation)
        for d in range(lo, hi + 1):
            score, matches = score_diag(read, seqs[s], d, penalty)
            scored.append((score, matches, i, d, s))
    rec.update(flags=TARGET, n_anchors=len(anchors), n_diags=len(scored))
    if scored:
        sign = 1 if mutation == "tie_large_d" else -1
        score, matches, i, d, s = max(scored, key=lambda x: (x[0], x[1], -x[2], sign * x[3]))
        below = [x[0] for x in scored if x[0] < score]
        rec.update(diag=d, seq=s, anchor=i, seg_score=score, matches=matches, n_best=min(sum(1 for x in scored if (x[0], x[1]) == (score, matches)), U32),
                   next_score=max(below) if below else 0)
        if (score > min_score) if mutation == "gt_min" else (score >= min_score):
            rec["flags"] |= RESCUED
    return rec


def read_rescue(seqs, reads, cand_offsets, cands, frag_min, frag_max, penalty, min_score, max_anchors, flags=0, mutation=None):
    """dict(reads RESCUE_DTYPE[n_reads], n_targets, n_rescued, n_full, n_tasks, n_diags; with MERGE cand_offsets, cands and winners as verify lays them
    out, else None)"""
    assert mutation is None or mutation in MUTATIONS
    n = len(reads)
    assert n % 2 == 0 and len(cand_offsets) == n + 1 and min_score >= 1 and 1 <= max_anchors <= MAX_ANCHORS and 0 <= frag_max - frag_min < MAX_WINDOW
    lens = [len(s) for s in seqs]
    cands = np.asarray(cands, dtype=VERIFY_DTYPE)
    mine = lambda r: cands[int(cand_offsets[r]):int(cand_offsets[r + 1])]
    out = np.zeros(n, RESCUE_DTYPE)
    out["seq"] = NO_SEQUENCE
    for k in range(n // 2):
        a, b = mine(2 * k), mine(2 * k + 1)
        pair = M.mate_pair(lens, a, b, frag_min, frag_max, 0)
        if pair["n_compatible"]:
            continue
        for t, own, mate, solo in ((2 * k, a, b, pair["solo_b"]), (2 * k + 1, b, a, pair["solo_a"])):
            rec = rescue_read(seqs, reads[t], len(own), mate, solo, frag_min, frag_max, penalty, min_score, max_anchors, mutation)
            for f, v in rec.items():
                out[t][f] = v
    fl = out["flags"]
    res = dict(reads=out, n_targets=int(((fl & TARGET) != 0).sum()), n_rescued=int(((fl & RESCUED) != 0).sum()), n_full=int(((fl & FULL) != 0).sum()),
               n_tasks=int(out["n_anchors"].sum()), n_diags=int(out["n_diags"].sum()), cand_offsets=None, cands=None, winners=None)
    if flags & MERGE:
        res.update(merged(seqs, reads, cand_offsets, cands, out, penalty, mutation))
    return res


def merged(seqs, reads, cand_offsets, cands, recs, penalty, mutation=None):
    """the list with the rescued candidates appended, its offsets, and the winners by verify's rule"""
    n = len(reads)
    offs, flat, winners = np.zeros(n + 1, np.uint64), [], np.zeros(n, VERIFY_DTYPE)
    for r in range(n):
        lst = [c.copy() for c in cands[int(cand_offsets[r]):int(cand_offsets[r + 1])]]
        if int(recs[r]["flags"]) & RESCUED:
            v = V.verify_one(reads[r], seqs[int(recs[r]["seq"])], int(recs[r]["diag"]), penalty)
            v.update(seq=int(recs[r]["seq"]), n_cand=len(lst), cand_index=len(lst), n_tied=0)
            c = np.zeros((), VERIFY_DTYPE)
            for f in VERIFY_DTYPE.names:
                c[f] = v[f]
            if mutation == "merge_first":
                lst.insert(0, c)
            else:
                lst.append(c)
        offs[r + 1] = offs[r] + np.uint64(len(lst))
        flat += lst
        win = M.solo_winner(lst)
        winners[r] = M.elected(lst, win) if lst else M.elected([], 0)
    return dict(cand_offsets=offs, cands=np.array(flat, dtype=VERIFY_DTYPE) if flat else np.zeros(0, VERIFY_DTYPE), winners=winners)
