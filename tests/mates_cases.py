"""Case table of the read mates stage (test_mates_cpu.py on the CPU, test_gpu_mates.py and test_gpu_cli_mates.py on the GPU).  Pure Python /
numpy: nothing of the library is called here.

The collection: six i.i.d. forward sequences of 1200, 1500, 900, 2000, 700 and 64 symbols, each followed by its reverse complement, so that
path p is sequence 2p forward and 2p + 1 reversed.  In the first four a segment of 100 symbols (copy 1) is copied to a second place at
least 600 symbols further on (copy 2).  On the odd twin the copies lie mirrored: the copy with the smaller offset there is forward copy 2.

The pairs: two reads of 50 bases cut from the ends of a fragment [f, f + I) of one sequence q: A its first 50 bases, on q at diag f; B the
reverse complement of its last 50, on q ^ 1 at diag L - f - I.  Every pair carries the truth (seq, diag) of both mates, which follows from
how it was cut, its class and, for the classes with a mate inside a repeat, `which`: 0 when the mate lies in the copy with the smaller
diag on its sequence (the one verify's "first in candidate order" names), 1 for the other.  FRAG_MAX is 500; the `border` class is made for
a run with frag_min 150.  Two classes make the pair overrule verify without a repeat tie to break: `tie` (a fragment inside one copy: the
compatible pairs are (0, 1) and (1, 0) alone and tie in both sums) and `below` (A prefers the second copy by one mismatch, B lies a
fragment from the first: the one compatible pair scores below the solo winners); their truth is what the definitions choose at U = 10."""
import numpy as np

MIN_LEN = 12  # the run's min_len
READ_LEN = 50
FRAG_MIN, FRAG_MAX, BORDER_FRAG_MIN = 0, 500, 150
FORWARD_LENGTHS = (1200, 1500, 900, 2000, 700, 64)
COPIES = ((150, 800), (200, 1000), (100, 720), (300, 1300))  # offsets of copy 1 and copy 2 in the forward sequences 0 .. 3
COPY_LEN = 100
HANGS = (1, 7, 31)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def rc(s):
    return bytes(s).translate(_COMP)[::-1]


class MatesCases:
    """seqs, raw, lens; pairs: dicts with kind, a, b (bytes), truth_a, truth_b ((seq, diag) or None), frag (of the truth, None without), which and
    mate ('a' or 'b': the mate inside the repeat; None for the other classes)"""

    def __init__(self):
        rng = np.random.default_rng(8107)
        self._rng = rng
        fwd = []
        for p, n in enumerate(FORWARD_LENGTHS):
            s = bytearray(_ACGT[rng.integers(0, 4, size=n)].tobytes())
            if p < len(COPIES):
                c1, c2 = COPIES[p]
                assert c2 - c1 >= 600 and c2 + COPY_LEN <= n
                s[c2:c2 + COPY_LEN] = s[c1:c1 + COPY_LEN]
            fwd.append(bytes(s))
        self.seqs = []
        for s in fwd:
            self.seqs += [s, rc(s)]
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
        """offsets of the two copies on sequence q, ascending"""
        c1, c2 = COPIES[q // 2]
        return (c1, c2) if q % 2 == 0 else (self.lens[q] - c2 - COPY_LEN, self.lens[q] - c1 - COPY_LEN)

    def _outside(self, q, start):
        """the read [start, start + 50) of q lies inside the sequence and meets no copy"""
        if start < 0 or start + READ_LEN > self.lens[q]:
            return False
        return q // 2 >= len(COPIES) or all(start + READ_LEN <= c or start >= c + COPY_LEN for c in self.copies(q))

    def _junk(self, n, faces=b""):
        """n bases; base k differs from faces[k] where there is one"""
        out = bytearray()
        for k in range(n):
            ok = [c for c in b"ACGT" if k >= len(faces) or c != faces[k]]
            out.append(ok[int(self._rng.integers(0, len(ok)))])
        return bytes(out)

    def _cut(self, kind, q, f, size, which=None, mate=None):
        """the pair of the fragment [f, f + size) of sequence q"""
        s, ln = self.seqs[q], self.lens[q]
        assert 0 <= f and f + size <= ln and size >= READ_LEN
        self.pairs.append(dict(kind=kind, a=s[f:f + READ_LEN], b=rc(s[f + size - READ_LEN:f + size]), truth_a=(q, f), truth_b=(q ^ 1, ln - f - size), frag=size, which=which, mate=mate))

    def _free_fragment(self, q, size):
        """a start f at which both mates of [f, f + size) of q lie outside the copies"""
        for _ in range(100000):
            f = int(self._rng.integers(0, self.lens[q] - size + 1))
            if self._outside(q, f) and self._outside(q, f + size - READ_LEN):
                return f
        raise AssertionError("no free fragment of %d on sequence %d" % (size, q))

    def _repeat(self, kind, q, which, mate):
        """mate 'a' or 'b' of a fragment of 150 .. 450 lies wholly inside copy `which` of q, the other mate outside the copies"""
        c = self.copies(q)[which]
        for _ in range(100000):
            size = int(self._rng.integers(150, 451))
            at = c + int(self._rng.integers(0, COPY_LEN - READ_LEN + 1))
            f = at if mate == "a" else at - (size - READ_LEN)
            other = f + size - READ_LEN if mate == "a" else f
            if f >= 0 and f + size <= self.lens[q] and self._outside(q, other):
                return self._cut(kind, q, f, size, which if mate == "a" else 1 - which, mate)  # (B lies on q ^ 1, where the copies are mirrored)
        raise AssertionError("no fragment with mate %s in copy %d of sequence %d" % (mate, which, q))

    def _build(self):
        rng = self._rng
        size = lambda: int(rng.integers(200, 451))
        for q in (0, 2, 4, 6, 8, 0, 2, 4, 6, 8, 6, 2):
            n = size()
            self._cut("unique", q, self._free_fragment(q, n), n)
        for kind, mate in (("repeat_a", "a"), ("repeat_b", "b")):
            for q in (0, 2, 4, 6):
                for which in (0, 1):
                    for _ in range(2):
                        self._repeat(kind, q, which, mate)
        # each of the above, cut from the odd twin
        for q in (1, 3, 5, 7, 9, 7):
            n = size()
            self._cut("reverse", q, self._free_fragment(q, n), n)
        for mate in ("a", "b"):
            for q in (1, 3, 5, 7):
                for which in (0, 1):
                    self._repeat("reverse", q, which, mate)
        # not compatible: too far apart, on different paths, on the same strand
        for q in (0, 2, 6, 1, 3, 7, 0, 2, 6, 7):
            self._cut("far", q, self._free_fragment(q, 900 + READ_LEN), 900 + READ_LEN)
        for k in range(10):
            qa, qb = (0, 2, 4, 6, 8)[k % 5], (3, 5, 7, 9, 1)[k % 5]  # A forward on one path, B reversed on another
            fa, fb = self._free_fragment(qa, READ_LEN), self._free_fragment(qb, READ_LEN)
            self.pairs.append(dict(kind="cross", a=self.seqs[qa][fa:fa + READ_LEN], b=self.seqs[qb][fb:fb + READ_LEN], truth_a=(qa, fa), truth_b=(qb, fb), frag=None, which=None, mate=None))
        for q in (0, 2, 4, 6, 8, 1, 3, 5, 7, 9):
            n = size()
            f = self._free_fragment(q, n)
            self.pairs.append(dict(kind="same_strand", a=self.seqs[q][f:f + READ_LEN], b=self.seqs[q][f + n - READ_LEN:f + n], truth_a=(q, f),
                                   truth_b=(q, f + n - READ_LEN), frag=None, which=None, mate=None))
        # frag exactly at the bounds of a run with frag_min 150 and one off
        for q in (0, 6, 9):
            for n in (BORDER_FRAG_MIN - 1, BORDER_FRAG_MIN, FRAG_MAX, FRAG_MAX + 1):
                self._cut("border", q, self._free_fragment(q, n), n)
        # B is random bytes, or empty
        for k in range(10):
            q = (0, 3, 4, 7, 8)[k % 5]
            f = self._free_fragment(q, READ_LEN)
            self.pairs.append(dict(kind="orphan", a=self.seqs[q][f:f + READ_LEN], b=self._junk(READ_LEN) if k < 6 else b"", truth_a=(q, f), truth_b=None, frag=None, which=None, mate=None))
        # the fragment runs over the start / the end of its sequence by h bases: one mate hangs over, its h outer bases match nothing
        for q in (0, 9, 10, 11):
            s, ln = self.seqs[q], self.lens[q]
            for h in HANGS:
                n = min(300, ln) + h
                # [-h, n - h): A = h junk bases + the first 50 - h of q; B lies inside
                self.pairs.append(dict(kind="hang", a=self._junk(h) + s[:READ_LEN - h], b=rc(s[n - h - READ_LEN:n - h]), truth_a=(q, -h), truth_b=(q ^ 1, ln + h - n), frag=n, which=None, mate=None))
                # [ln - n + h, ln + h): B = the reverse complement of (the last 50 - h of q + h junk bases): it hangs over the start of q ^ 1
                f = ln - n + h
                self.pairs.append(dict(kind="hang", a=s[f:f + READ_LEN], b=rc(s[ln - (READ_LEN - h):] + self._junk(h)), truth_a=(q, f), truth_b=(q ^ 1, -h), frag=n, which=None, mate=None))
        # a fragment of 50 .. 100 wholly inside the first copy of q: both mates have both copies as candidates, A's in the order (first, second),
        # B's on q ^ 1 in the order (second, first), so the compatible pairs are (0, 1) and (1, 0) alone and tie in both sums: the smallest i decides
        for k in range(10):
            q = (0, 1, 2, 3, 4, 5, 6, 7, 0, 3)[k]
            n = int(rng.integers(READ_LEN, COPY_LEN + 1))
            self._cut("tie", q, self.copies(q)[0] + int(rng.integers(0, COPY_LEN - n + 1)), n)
        # A: the last 38 bases of the second copy of q, one substituted base, 11 bases of what follows that copy: one MEM with two occurrences, so both
        # copies are candidates, and verify prefers the second (one mismatch in 50) to the first (38 matches, then the other flank).  B lies a fragment
        # away from the FIRST copy: the only compatible pair scores below the solo winners, and the unpaired penalty decides
        for k in range(10):
            q = (0, 1, 2, 3, 4, 5, 6, 7, 2, 5)[k]
            s, ln = self.seqs[q], self.lens[q]
            lo, hi = self.copies(q)
            end = hi + COPY_LEN
            a = s[end - 38:end] + self._junk(1, bytes([s[end]])) + s[end + 1:end + 12]
            while a[38] == s[lo + COPY_LEN]:  # (the substituted base differs from what follows either copy)
                a = a[:38] + self._junk(1, bytes([s[end]])) + a[39:]
            a0 = lo + COPY_LEN - 38
            for _ in range(100000):
                n = int(rng.integers(150, 451))
                if a0 + n <= ln and self._outside(q, a0 + n - READ_LEN):
                    break
            self.pairs.append(dict(kind="below", a=a, b=rc(s[a0 + n - READ_LEN:a0 + n]), truth_a=(q, a0), truth_b=(q ^ 1, ln - a0 - n), frag=n, which=None, mate=None))


CASES = MatesCases()
KIND_COUNTS = dict(unique=12, repeat_a=16, repeat_b=16, reverse=22, far=10, cross=10, same_strand=10, border=12, orphan=10, hang=24, tie=10, below=10)
