"""Case table of the read rescue stage (test_rescue_cpu.py on the CPU, test_gpu_rescue.py and test_gpu_cli_rescue.py on the GPU).  Pure Python /
numpy: nothing of the library is called here.

The collection: the six twinned sequences of mates_cases.CASES (1200, 1500, 900, 2000, 700 and 64 symbols forward, each followed by its
reverse complement, a segment of 100 copied in the first four), with a tandem repeat of period 5 and 80 symbols planted at offset 300 of the
fifth.  The pairs are cut as there: A the first 50 bases of a fragment [f, f + I) of sequence q, on q at diag f; B the reverse complement of its
last 50, on q ^ 1 at diag L - f - I.  A `dense` mate carries a substitution every 9 to 11 bases, so that no exact run reaches MIN_LEN and no
MEM places it.  Every pair names its mate to rescue (`mate`: 'a', 'b' or None) and the truth (seq, diag) of both mates.  The run has
frag_min 0 and frag_max 500, penalty 4 and min_score MIN_LEN."""
import numpy as np

import mates_cases as MC

MIN_LEN = MC.MIN_LEN  # 12: the run's min_len and the stage's min_score
READ_LEN = MC.READ_LEN
FRAG_MIN, FRAG_MAX, BORDER_FRAG_MIN = MC.FRAG_MIN, MC.FRAG_MAX, MC.BORDER_FRAG_MIN
PENALTY = 4
COPY_LEN = MC.COPY_LEN
HANGS = MC.HANGS
TANDEM_SEQ, TANDEM_AT, TANDEM_LEN, TANDEM_PERIOD = 8, 300, 80, 5
rc = MC.rc


class RescueCases:
    """seqs, raw, lens; pairs: dicts with kind, a, b (bytes), truth_a, truth_b ((seq, diag) or None), frag, mate and, for `threshold`, score; for
    `tandem`, ties (the diagonals that tie with the truth, ascending)"""

    def __init__(self):
        self._rng = np.random.default_rng(61021)
        fwd = [bytearray(s) for s in MC.CASES.seqs[0::2]]
        unit = b"ACGTT"
        fwd[TANDEM_SEQ // 2][TANDEM_AT:TANDEM_AT + TANDEM_LEN] = unit * (TANDEM_LEN // TANDEM_PERIOD)
        self.seqs = []
        for s in fwd:
            self.seqs += [bytes(s), rc(bytes(s))]
        self.raw = b"".join(s + b"\n" for s in self.seqs)
        self.lens = [len(s) for s in self.seqs]
        self.pairs = []
        self._build()
        self.reads = []
        for p in self.pairs:
            self.reads += [p["a"], p["b"]]
        self.kinds = [p["kind"] for p in self.pairs]

    # -- pieces
    def copies(self, q):
        return MC.CASES.copies(q)

    def tandem(self, q):
        """[start, end) of the tandem repeat on sequence q (8 or 9)"""
        return (TANDEM_AT, TANDEM_AT + TANDEM_LEN) if q == TANDEM_SEQ else (self.lens[q] - TANDEM_AT - TANDEM_LEN, self.lens[q] - TANDEM_AT)

    def _outside(self, q, start):
        """the read [start, start + 50) of q lies inside the sequence and meets neither a copy nor the tandem repeat"""
        if start < 0 or start + READ_LEN > self.lens[q]:
            return False
        if q // 2 == TANDEM_SEQ // 2:
            t0, t1 = self.tandem(q)
            return start + READ_LEN <= t0 or start >= t1
        return q // 2 >= len(MC.COPIES) or all(start + READ_LEN <= c or start >= c + COPY_LEN for c in self.copies(q))

    def _other(self, c):
        ok = [x for x in b"ACGT" if x != c]
        return ok[int(self._rng.integers(0, 3))]

    def _junk(self, n):
        return bytes(b"ACGT"[int(x)] for x in self._rng.integers(0, 4, size=n))

    def _placeless(self, read):
        """no MIN_LEN bases of the read occur in the collection: no MEM of the run places it anywhere"""
        return all(read[i:i + MIN_LEN] not in self.raw for i in range(len(read) - MIN_LEN + 1))

    def _dense(self, s, lo=0, hi=None):
        """s with a substitution every 9 to 11 bases inside [lo, hi): no exact run of MIN_LEN there (the first after 8 to 10 bases in a short
        stretch, so that its score still reaches MIN_LEN), drawn again until no MEM places it anywhere"""
        hi = len(s) if hi is None else hi
        for _ in range(1000):
            out = bytearray(s)
            at = lo + int(self._rng.integers(8 if hi - lo < 25 else 4, 11))
            last = lo - 1
            while at < hi:
                out[at] = self._other(out[at])
                last = at
                at += int(self._rng.integers(10, 13))  # (9 to 11 matching bases between two substitutions)
            assert hi - 1 - last <= 11
            if self._placeless(bytes(out)):
                return bytes(out)
        raise AssertionError("no dense form without a MEM")

    def _scores(self, read, q, d):
        """(seg_score, matches) of the read on diagonal d of sequence q at PENALTY"""
        e = best = matches = 0
        for i, c in enumerate(read):
            if 0 <= d + i < self.lens[q]:
                hit = c == self.seqs[q][d + i]
                matches += hit
                e = max(e, 0) + (1 if hit else -PENALTY)
                best = max(best, e)
        return best, matches

    def _cut(self, kind, q, f, size, mate, **more):
        """the pair of the fragment [f, f + size) of sequence q, with `mate` made dense"""
        s, ln = self.seqs[q], self.lens[q]
        assert 0 <= f and f + size <= ln and size >= READ_LEN
        a, b = s[f:f + READ_LEN], rc(s[f + size - READ_LEN:f + size])
        if mate == "a":
            a = self._dense(a)
        elif mate == "b":
            b = self._dense(b)
        self.pairs.append(dict(kind=kind, a=a, b=b, truth_a=(q, f), truth_b=(q ^ 1, ln - f - size), frag=size, mate=mate, **more))

    def _free_fragment(self, q, size):
        for _ in range(100000):
            f = int(self._rng.integers(0, self.lens[q] - size + 1))
            if self._outside(q, f) and self._outside(q, f + size - READ_LEN):
                return f
        raise AssertionError("no free fragment of %d on sequence %d" % (size, q))

    def _build(self):
        rng = self._rng
        size = lambda: int(rng.integers(200, 451))
        # a dense mate a fragment away from a unique one; four of them exactly at the bounds of a run with frag_min 150
        for k, q in enumerate((0, 2, 4, 6, 8, 0, 2, 4, 6, 8, 6, 2)):
            n = (BORDER_FRAG_MIN, FRAG_MAX, BORDER_FRAG_MIN, FRAG_MAX)[k - 8] if k >= 8 else size()
            self._cut("dense", q, self._free_fragment(q, n), n, "ab"[k % 2])
        for k, q in enumerate((1, 3, 5, 7, 9, 1, 3, 5, 7, 9)):
            n = size()
            self._cut("dense_both_strands", q, self._free_fragment(q, n), n, "ab"[k % 2])
        # A lies in the copy of q with the larger diag (its candidate 1, tied with candidate 0), the dense B a fragment further on
        for k in range(10):
            q = (0, 1, 2, 3, 4, 5, 6, 7, 0, 3)[k]
            c = self.copies(q)[1]
            for _ in range(100000):
                n = int(rng.integers(150, 451))
                f = c + int(rng.integers(0, COPY_LEN - READ_LEN + 1))
                if f + n <= self.lens[q] and self._outside(q, f + n - READ_LEN):
                    break
            else:
                raise AssertionError("no fragment from the second copy of sequence %d" % q)
            self._cut("repeat_anchor", q, f, n, "b")
        # the fragment runs over the start / the end of its sequence by h bases: the dense mate hangs over, its h outer bases match nothing
        for k, q in enumerate((0, 9, 10, 11)):
            s, ln = self.seqs[q], self.lens[q]
            for h in HANGS:
                n = min(300, ln) + h
                if k % 2 == 0:  # [-h, n - h): A = h junk bases + the first 50 - h of q, dense; B lies inside
                    a = self._dense(self._junk(h) + s[:READ_LEN - h], h, READ_LEN)
                    self.pairs.append(dict(kind="edge", a=a, b=rc(s[n - h - READ_LEN:n - h]), truth_a=(q, -h), truth_b=(q ^ 1, ln + h - n), frag=n, mate="a"))
                else:           # [ln - n + h, ln + h): B = the reverse complement of (the last 50 - h of q + h junk bases), dense: it hangs over the start of q ^ 1
                    f = ln - n + h
                    b = self._dense(rc(s[ln - (READ_LEN - h):] + self._junk(h)), h, READ_LEN)
                    self.pairs.append(dict(kind="edge", a=s[f:f + READ_LEN], b=b, truth_a=(q, f), truth_b=(q ^ 1, -h), frag=n, mate="b"))
        # B is random bases
        for k in range(10):
            q = (0, 3, 4, 7, 8, 1, 2, 5, 6, 9)[k]
            f = self._free_fragment(q, READ_LEN)
            b = self._junk(READ_LEN)
            while not self._placeless(b):
                b = self._junk(READ_LEN)
            self.pairs.append(dict(kind="junk", a=self.seqs[q][f:f + READ_LEN], b=b, truth_a=(q, f), truth_b=None, frag=None, mate=None))
        # B matches its truth in 10 bases, a mismatch, and 6 (score 12 at penalty 4) or 5 (score 11) more; every other base differs from the truth
        for k in range(10):
            q = (0, 2, 4, 6, 8, 1, 3, 5, 7, 9)[k]
            n, second = size(), 6 if k % 2 == 0 else 5
            f = self._free_fragment(q, n)
            true_b = rc(self.seqs[q][f + n - READ_LEN:f + n])
            for _ in range(1000):
                at = int(rng.integers(0, READ_LEN - 11 - second + 1))
                keep = set(range(at, at + 10)) | set(range(at + 11, at + 11 + second))
                b = bytes(c if i in keep else self._other(c) for i, c in enumerate(true_b))
                if self._placeless(b):
                    break
            self.pairs.append(dict(kind="threshold", a=self.seqs[q][f:f + READ_LEN], b=b, truth_a=(q, f), truth_b=(q ^ 1, self.lens[q] - f - n), frag=n, mate="b",
                                   score=10 - PENALTY + second))
        # the dense mate lies inside the tandem repeat, 10 symbols behind its start on its sequence: the diagonals a multiple of the period away tie
        for k in range(10):
            q = TANDEM_SEQ + k % 2
            t0, t1 = self.tandem(q)
            for _ in range(100000):
                n = int(rng.integers(150, 401))
                f = t0 + 10
                if f + n <= self.lens[q]:
                    break
            s = self.seqs[q]
            ties = [d for d in range(t0, t1 - READ_LEN + 1) if (d - f) % TANDEM_PERIOD == 0]
            for _ in range(1000):  # (a substituted base may match the flank of the repeat on a diagonal that leaves it: drawn again until none beats the truth)
                a = self._dense(s[f:f + READ_LEN])
                top = self._scores(a, q, f)
                if all((self._scores(a, q, d) < top) != (d in ties) for d in range(t0 - READ_LEN, t1)):
                    break
            else:
                raise AssertionError("no dense form that ties inside the repeat alone")
            self.pairs.append(dict(kind="tandem", a=a, b=rc(s[f + n - READ_LEN:f + n]), truth_a=(q, f), truth_b=(q ^ 1, self.lens[q] - f - n), frag=n, mate="a", ties=ties))
        # both mates placed, a fragment of 950 apart: no pair is compatible, each is a target around the other, and nothing is found there
        for q in (0, 2, 6, 1, 3, 7, 0, 2, 6, 7):
            self._cut("both", q, self._free_fragment(q, 900 + READ_LEN), 900 + READ_LEN, None)
        for q in (0, 2, 4, 6, 8, 1, 3, 5, 7, 9):
            n = size()
            self._cut("proper", q, self._free_fragment(q, n), n, None)


CASES = RescueCases()
KIND_COUNTS = dict(dense=12, dense_both_strands=10, repeat_anchor=10, edge=12, junk=10, threshold=10, tandem=10, both=10, proper=10)
