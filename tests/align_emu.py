"""Read align in plain Python: the definitions of include/pgx.h "read align", restated as the plain O(m * W) table.  Read R of len bytes, its
candidate (seq, diag) on a sequence T of Ls symbols (no endmarker), band half-width W, 0 <= W <= 31:

  clips       [lo, hi) is the verify span of the candidate: lo = max(0, -diag), hi = min(len, Ls - diag).  Only Q = R[lo, hi) is aligned, with
              m = hi - lo and d0 = diag + lo; clip_lo = lo and clip_hi = len - hi are soft clips.  Empty span: clip_lo = 0, clip_hi = len,
              everything else 0 (seq and diag stay the candidate's), and one S operation if len > 0.
  cells       (i, j): i symbols of Q and text offset j consumed; valid iff 0 <= i <= m, 0 <= j <= Ls and |k| <= W, where k = j - i - d0
  match       Q[i-1] is an upper-case A C G T and equals T[j-1]
  recurrence  D[0][j] = 0 for every valid j.  D[i][j] is the minimum over valid predecessors of D[i-1][j-1] + (0 if match else 1),
              D[i-1][j] + 1 (insertion: a read symbol without text), D[i][j-1] + 1 (deletion)
  end cell    the valid cell of row m with the smallest D; ties go to the smallest |k|, then to the negative k
  traceback   from the end cell to row 0, the first of these that reproduces D[i][j] is taken: 1. the diagonal move (= on a match, else X),
              2. the insertion (I), 3. the deletion (D)
  band_hit    1 iff W > 0 and some cell of the traced path, ends included, has |k| == W
  cigar       u32 words of length << 4 | op with the BAM codes I = 1, D = 2, S = 4, = is 7, X = 8, in read order, equal neighbours merged; a
              leading S is clip_lo, a trailing S is clip_hi, each only when non-zero

Nothing here is shared with the library: the kernels keep a diagonal a lane, min-scan the deletion term and pack two direction bits a cell;
this file fills a table cell by cell."""
import numpy as np

ALIGN_DTYPE = np.dtype([("diag", "<i8"), ("text_start", "<u8"), ("text_end", "<u8"), ("seq", "<u4"), ("clip_lo", "<u4"), ("clip_hi", "<u4"), ("edits", "<u4"),
                        ("n_match", "<u4"), ("n_mismatch", "<u4"), ("n_ins", "<u4"), ("n_del", "<u4"), ("n_ops", "<u4"), ("band_hit", "<u4")])
NO_SEQUENCE = 0xFFFFFFFF
ACGT = frozenset(b"ACGT")
OP_I, OP_D, OP_S, OP_EQ, OP_X = 1, 2, 4, 7, 8
OP_CHAR = {OP_I: "I", OP_D: "D", OP_S: "S", OP_EQ: "=", OP_X: "X"}
INF = 1 << 60


def align_one(read, seq, diag, band):
    """(fields of the record as a dict without seq, [(length, op)] in read order)"""
    n, ls, w = len(read), len(seq), int(band)
    lo, hi = max(0, -diag), min(n, ls - diag)
    rec = dict(diag=diag, text_start=0, text_end=0, clip_lo=0, clip_hi=n, edits=0, n_match=0, n_mismatch=0, n_ins=0, n_del=0, n_ops=0, band_hit=0)
    if hi <= lo:
        ops = [(n, OP_S)] if n else []
        rec["n_ops"] = len(ops)
        return rec, ops
    q, m, d0 = read[lo:hi], hi - lo, diag + lo
    valid = lambda i, k: 0 <= i <= m and 0 <= i + d0 + k <= ls and -w <= k <= w
    table = [[INF] * (2 * w + 1) for _ in range(m + 1)]  # table[i][k + w] = D[i][i + d0 + k]
    for k in range(-w, w + 1):
        if valid(0, k):
            table[0][k + w] = 0
    for i in range(1, m + 1):
        for k in range(-w, w + 1):
            if not valid(i, k):
                continue
            j, best = i + d0 + k, INF
            if valid(i - 1, k) and j >= 1:  # (i - 1, j - 1) lies on the same diagonal
                best = min(best, table[i - 1][k + w] + (0 if q[i - 1] in ACGT and q[i - 1] == seq[j - 1] else 1))
            if valid(i - 1, k + 1):  # (i - 1, j)
                best = min(best, table[i - 1][k + 1 + w] + 1)
            if valid(i, k - 1):  # (i, j - 1)
                best = min(best, table[i][k - 1 + w] + 1)
            table[i][k + w] = best
    k = min((kk for kk in range(-w, w + 1) if valid(m, kk)), key=lambda kk: (table[m][kk + w], abs(kk), kk > 0))
    i, hit, ops = m, abs(k) == w, []
    rec["text_end"], rec["edits"] = m + d0 + k, table[m][k + w]
    while i > 0:
        j, here = i + d0 + k, table[i][k + w]
        match = j >= 1 and q[i - 1] in ACGT and q[i - 1] == seq[j - 1]
        if valid(i - 1, k) and j >= 1 and table[i - 1][k + w] + (0 if match else 1) == here:
            op, i = (OP_EQ if match else OP_X), i - 1
        elif valid(i - 1, k + 1) and table[i - 1][k + 1 + w] + 1 == here:
            op, i, k = OP_I, i - 1, k + 1
        else:
            assert valid(i, k - 1) and table[i][k - 1 + w] + 1 == here
            op, k = OP_D, k - 1
        hit = hit or abs(k) == w
        ops.append(op)
    ops.reverse()
    rec["text_start"] = d0 + k
    rec.update(clip_lo=lo, clip_hi=n - hi, n_match=ops.count(OP_EQ), n_mismatch=ops.count(OP_X), n_ins=ops.count(OP_I), n_del=ops.count(OP_D), band_hit=int(w > 0 and hit))
    runs = [(lo, OP_S)] if lo else []
    for op in ops:
        if runs and runs[-1][1] == op:
            runs[-1] = (runs[-1][0] + 1, op)
        else:
            runs.append((1, op))
    if n - hi:
        runs.append((n - hi, OP_S))
    rec["n_ops"] = len(runs)
    return rec, runs


def read_align(seqs, reads, cands, band):
    """seqs: list of bytes (no endmarkers); reads: list of bytes; cands: per read (seq, diag) or None.  Returns dict(reads ALIGN_DTYPE[n_reads],
    op_offsets uint64[n_reads + 1], ops uint32[n_ops]) as the library lays them out."""
    n = len(reads)
    recs = np.zeros(n, ALIGN_DTYPE)
    offs = np.zeros(n + 1, np.uint64)
    words = []
    for r in range(n):
        if cands[r] is None or cands[r][0] == NO_SEQUENCE:
            recs[r]["seq"] = NO_SEQUENCE
        else:
            q, diag = cands[r]
            rec, runs = align_one(reads[r], seqs[q], int(diag), band)
            rec["seq"] = q
            for f in ALIGN_DTYPE.names:
                recs[r][f] = rec[f]
            words.extend((length << 4) | op for length, op in runs)
        offs[r + 1] = len(words)
    return dict(reads=recs, op_offsets=offs, ops=np.array(words, dtype=np.uint32))


def cigar_text(words):
    """3S70=1D76=1X from the operation words"""
    return "".join("%d%s" % (int(x) >> 4, OP_CHAR[int(x) & 15]) for x in words)


def candidates_from_verified(verified):
    """the candidate of every read from the records of a read-verify result: its winner, None without one"""
    return [None if int(v["seq"]) == NO_SEQUENCE else (int(v["seq"]), int(v["diag"])) for v in verified]


def infix_distances(read, seqs):
    """the smallest unit-cost edit distance of the whole read to a substring of every sequence (no band, free start and end in the text): rows over
    the read, every row vectorised over the text positions of all sequences at once; the deletion term is a running minimum of D - j"""
    width = max((len(s) for s in seqs), default=0)
    text = np.zeros((len(seqs), width + 1), np.uint8)  # column j holds T[j - 1]; 0 matches nothing
    ok = np.zeros((len(seqs), width + 1), bool)
    for q, s in enumerate(seqs):
        text[q, 1:len(s) + 1] = np.frombuffer(bytes(s), np.uint8)
        ok[q, :len(s) + 1] = True
    col = np.arange(width + 1, dtype=np.int64)
    row = np.zeros((len(seqs), width + 1), np.int64)
    for c in read:
        sub = np.ones_like(row) if c not in ACGT else (text != c).astype(np.int64)
        x = row + 1  # insertion
        x[:, 1:] = np.minimum(x[:, 1:], row[:, :-1] + sub[:, 1:])
        row = np.minimum.accumulate(x - col, axis=1) + col
    return np.where(ok, row, INF).min(axis=1)
