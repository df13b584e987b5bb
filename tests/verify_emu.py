"""Read verify in plain Python: the definitions of include/pgx.h "read verify", restated position by position.  A candidate (seq, diag) of a
read R of len bytes on a sequence T of Ls symbols (no endmarker):

  span        [lo, hi) = [max(0, -diag), min(len, Ls - diag)), or lo = hi = 0 when that is empty
  match at i  R[i] is one of upper-case A C G T and equals T[diag + i]; everything else in the span is a mismatch
  run         the longest stretch of matches and the smallest start of one (0, 0 without a match)
  segment     the non-empty [a, b) inside the span with the largest (matches - P * mismatches), ties to the smallest a, then the smallest b;
              found here by the O(len^2) double loop.  Without a match: score 0, [lo, lo), no mismatches.
  winner      of a read's candidates: largest seg_score, then most matches, then the first

Nothing here is shared with the library: the kernels walk packed words and jump from mismatch to mismatch; this file loops over positions."""
import numpy as np

VERIFY_DTYPE = np.dtype([("diag", "<i8"), ("seq", "<u4"), ("n_cand", "<u4"), ("span_lo", "<u4"), ("span_hi", "<u4"), ("matches", "<u4"), ("mismatches", "<u4"),
                         ("seg_start", "<u4"), ("seg_end", "<u4"), ("seg_score", "<u4"), ("seg_mismatches", "<u4"), ("longest_run", "<u4"), ("run_start", "<u4"),
                         ("cand_index", "<u4"), ("n_tied", "<u4")])
NO_SEQUENCE = 0xFFFFFFFF
ACGT = frozenset(b"ACGT")


def match_string(read, seq, diag):
    """(lo, hi, [True where read position lo + k matches])"""
    lo, hi = max(0, -diag), min(len(read), len(seq) - diag)
    if hi <= lo:
        return 0, 0, []
    return lo, hi, [read[i] in ACGT and read[i] == seq[diag + i] for i in range(lo, hi)]


def best_segment_quadratic(m, penalty):
    """(score, a, b, mismatches inside) over a list of booleans: every non-empty [a, b), ties to the smallest a, then the smallest b;
    (0, 0, 0, 0) when nothing matches"""
    if not any(m):
        return 0, 0, 0, 0
    value = np.where(np.asarray(m, dtype=bool), 1, -int(penalty)).astype(np.int64)
    best = None
    for a in range(len(m)):  # every start; the inner loop over the ends b = a + 1 .. is the running sum
        scores = np.cumsum(value[a:])
        k = int(np.argmax(scores))  # (the first maximum: the smallest b)
        if best is None or int(scores[k]) > best[0]:  # (a ascends: the first start to reach a score keeps it)
            best = (int(scores[k]), a, a + k + 1)
    score, a, b = best
    return score, a, b, sum(1 for x in m[a:b] if not x)


def longest_run(m):
    """(length, start) of the longest stretch of True, the smallest start of one; (0, 0) without"""
    best, start, run = 0, 0, 0
    for i, x in enumerate(m):
        run = run + 1 if x else 0
        if run > best:
            best, start = run, i + 1 - run
    return best, start


def verify_one(read, seq, diag, penalty):
    """the fields of one candidate as a dict (seq, n_cand, cand_index, n_tied are the caller's)"""
    lo, hi, m = match_string(read, seq, diag)
    score, a, b, mm = best_segment_quadratic(m, penalty)
    run, rs = longest_run(m)
    n_match = sum(m)
    return dict(diag=diag, span_lo=lo, span_hi=hi, matches=n_match, mismatches=len(m) - n_match, seg_start=lo + a, seg_end=lo + b, seg_score=score,
                seg_mismatches=mm, longest_run=run, run_start=(lo + rs) if run else 0)


def read_verify(seqs, reads, cands, penalty=4):
    """seqs: list of bytes (no endmarkers); reads: list of bytes; cands: per read a list of (seq, diag).  Returns dict(reads VERIFY_DTYPE[n_reads],
    cand_offsets uint64[n_reads + 1], cands VERIFY_DTYPE[n_cands]) as the library lays them out."""
    n = len(reads)
    offs = np.zeros(n + 1, np.uint64)
    per_read = np.zeros(n, VERIFY_DTYPE)
    flat = []
    for r in range(n):
        mine = []
        for k, (q, diag) in enumerate(cands[r]):
            v = verify_one(reads[r], seqs[q], int(diag), penalty)
            v.update(seq=q, n_cand=k, cand_index=k, n_tied=0)
            mine.append(v)
        offs[r + 1] = offs[r] + np.uint64(len(mine))
        flat.extend(mine)
        if not mine:
            per_read[r]["seq"] = NO_SEQUENCE
            continue
        win = 0
        for k in range(1, len(mine)):
            if (mine[k]["seg_score"], mine[k]["matches"]) > (mine[win]["seg_score"], mine[win]["matches"]):
                win = k
        w = dict(mine[win])
        w.update(n_cand=len(mine), cand_index=win,
                 n_tied=sum(1 for v in mine if (v["seg_score"], v["matches"]) == (mine[win]["seg_score"], mine[win]["matches"])))
        for f in VERIFY_DTYPE.names:
            per_read[r][f] = w[f]
    lst = np.zeros(len(flat), VERIFY_DTYPE)
    for i, v in enumerate(flat):
        for f in VERIFY_DTYPE.names:
            lst[i][f] = v[f]
    return dict(reads=per_read, cand_offsets=offs, cands=lst)


def candidates_from_places(place, max_cand):
    """the candidates of every read from a read-place result (reads, and place_offsets / places when max_cand > 1): the placements with
    score == best_score > 0 in list order, the first max_cand of them"""
    out = []
    for r, rec in enumerate(place["reads"]):
        best = int(rec["best_score"])
        if best == 0:
            out.append([])
        elif max_cand == 1:
            out.append([(int(rec["best_seq"]), int(rec["best_diag"]))])
        else:
            mine = place["places"][int(place["place_offsets"][r]):int(place["place_offsets"][r + 1])]
            out.append([(int(p["seq"]), int(p["diag"])) for p in mine if int(p["score"]) == best][:max_cand])
    return out
