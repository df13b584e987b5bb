"""The reads of tests/test_gaf_replay_cpu.py and tests/test_gpu_gaf_replay.py: reads on the graph of tests/walk_cases.py (16 sequences of about
3 kb, nodes of 1 to 64 bp, bubbles of 1 to 8 bp that may be indels) that stress align and walk together, each with its truth.

The truth of a read is (sequence, offset, edits) or None: read position 0 lies at `offset` of `sequence` (negative when the read hangs over the
sequence's start), and `edits` is the planted list, sorted, of
  ("X", p, byte)   the source symbol p positions behind the offset is replaced by byte (never the symbol itself; N, lower case and bytes outside
                   the alphabet are such edits too)
  ("I", p, bytes)  bytes are inserted in front of source position p
  ("D", p, n)      the n source symbols from p are left out
with at least four untouched symbols between two edits and in front of the first.  The planted candidate of a read is (sequence, offset).

Classes, in the order of CASES.reads (CASES.kind names the class of every read):
  mixed     N_MIXED reads of 150 bases with 0 .. MAX_EDITS planted edits (substitutions, insertions and deletions of 1 .. 3 bases); the second
            half is cut from a forward sequence and reverse-complemented before the edits are planted, so it lies on the odd twin
  heavy     N_HEAVY more of them with 3 .. HEAVY_EDITS planted edits
  end       reads of 100 bases that hang over the first / the last base of sequences 0, 1, 14 and 15 by 1, 7, 31 and 40 random bases
  byte_n, byte_lower, byte_other   mixed reads with one to three more bytes turned into N, into the lower case of the source symbol, into a byte
            outside the alphabet
  none      reads that share no 12 symbols with the collection (random ones, poly-A, the empty read, reads of 1, 11, 12 and 13 bases)
  stranger  random reads as they fall: a chance MEM may place them anywhere, they have no truth
  node_last, node_first, node_inside, node_whole, one_bp   error-free reads that start at the last base of a node, end on the first base of one,
            lie strictly inside one node, are one whole node, and cross two 1-bp visits in a row (a 1-bp node next to a 1-bp bubble allele; the
            graph has no longer run of them)"""
import numpy as np

import walk_cases as W

SEED, MIN_LEN = 12, 12
# MAX_EDITS: the place stage scores one diagonal and hands verify its first best placement, so the winner of a read with several indels is often a
# haplotype that shares the longest exact stretch and carries an allele of its own elsewhere in the read.  The kept-read bound (kept() below) may
# leave out 10 % of the mixed reads; with up to 6, 4 and 3 planted edits the emulator chain leaves out 16 to 17 %, 12 to 15 % and 10 to 14 % (seeds 11
# to 13 each), with up to 2 it leaves out 7 to 9 %.  The reads with more edits are the class `heavy`: replayed like all others, bounded where kept, outside that cap.
N_MIXED, MIXED_LEN, MAX_EDITS, MAX_INDEL = 300, 150, 2, 3
N_HEAVY, HEAVY_EDITS = 120, 6
END_LEN, HANG, END_SEQS = 100, (1, 7, 31, 40), (0, 1, 14, 15)
N_BYTE = 12  # per byte class
BANDS = (0, 8, 31)
MAX_LEFT_OUT = N_MIXED // 10  # the kept-read bound may leave out 10 % of the mixed reads, never more
OTHER_BYTES = b".R*-"


def _rand(rng, n):
    return bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, size=n))


def _other_base(rng, c):
    return bytes([[x for x in b"ACGT" if x != c][int(rng.integers(0, 3))]])


def apply_edits(src, edits):
    """the read bytes of a source stretch with its planted edits"""
    out, p = [], 0
    for kind, at, arg in edits:
        assert at >= p, "edits overlap"
        out.append(src[p:at])
        p = at
        if kind == "X":
            assert arg != src[at:at + 1]
            out.append(arg)
            p += 1
        elif kind == "I":
            out.append(arg)
        else:
            p += arg
    assert p <= len(src)
    out.append(src[p:])
    return b"".join(out)


def source_length(read_len, edits):
    return read_len - sum(len(e[2]) for e in edits if e[0] == "I") + sum(e[2] for e in edits if e[0] == "D")


def planted_cost(edits):
    """the unit cost of the planted alignment: a symbol an edit"""
    return sum(1 if e[0] == "X" else len(e[2]) if e[0] == "I" else e[2] for e in edits)


def longest_untouched(truth, read_len):
    """the longest stretch of source symbols that the read holds as they are"""
    best, p = 0, 0
    for kind, at, arg in truth[2] + [("end", source_length(read_len, truth[2]), 0)]:
        best = max(best, at - p)
        p = at + (1 if kind == "X" else arg if kind == "D" else 0)
    return best


def planted_cells(truth, read_len):
    """the cells (read position, text offset on the truth's sequence) of the planted alignment, both ends included"""
    q, o, edits = truth
    i, j, p = 0, o, 0
    cells = [(i, j)]

    def go(di, dj, n):
        nonlocal i, j
        for _ in range(n):
            i, j = i + di, j + dj
            cells.append((i, j))

    for kind, at, arg in edits:
        go(1, 1, at - p)
        p = at
        if kind == "X":
            go(1, 1, 1)
            p += 1
        elif kind == "I":
            go(1, 0, len(arg))
        else:
            go(0, 1, arg)
            p += arg
    go(1, 1, source_length(read_len, edits) - p)
    assert i == read_len
    return cells


def _plant(rng, n_edits, read_len, special=None, n_special=0):
    """a sorted edit list without the bytes (kinds, positions, lengths) and the source length that makes the read read_len long"""
    while True:
        kinds = [("X", "I", "D")[int(rng.integers(0, 3))] for _ in range(n_edits)] + ["S"] * n_special
        sizes = [1 if k in "XS" else int(rng.integers(1, MAX_INDEL + 1)) for k in kinds]
        src_len = read_len - sum(s for k, s in zip(kinds, sizes) if k == "I") + sum(s for k, s in zip(kinds, sizes) if k == "D")
        at = np.sort(rng.integers(4, src_len - 8, size=len(kinds))).tolist()
        order = rng.permutation(len(kinds)).tolist()
        kinds, sizes = [kinds[x] for x in order], [sizes[x] for x in order]
        if all(b - a >= MAX_INDEL + 5 for a, b in zip(at, at[1:])):
            return list(zip(kinds, at, sizes)), src_len


def _edited_read(rng, texts, q_forward, read_len, n_edits, reverse, special=None, n_special=0):
    """(read, truth): a stretch cut from the forward sequence q_forward, reverse-complemented first when `reverse`, then edited"""
    plan, src_len = _plant(rng, n_edits, read_len, special, n_special)
    text = texts[q_forward]
    at = int(rng.integers(0, len(text) - src_len + 1))
    src = text[at:at + src_len]
    q, o = q_forward, at
    if reverse:
        src, q, o = W.revcomp(src), q_forward + 1, len(text) - at - src_len
    edits = []
    for kind, p, size in plan:
        if kind == "X":
            edits.append(("X", p, _other_base(rng, src[p])))
        elif kind == "S":
            edits.append(("X", p, {"n": b"N", "lower": src[p:p + 1].lower(), "other": bytes([OTHER_BYTES[int(rng.integers(0, len(OTHER_BYTES)))]])}[special]))
        elif kind == "I":
            edits.append(("I", p, _rand(rng, size)))
        else:
            edits.append(("D", p, size))
    read = apply_edits(src, edits)
    assert len(read) == read_len
    return read, (q, o, edits)


def visits(g, q):
    """[(start, end, node << 1 | rev)] of sequence q"""
    out, pos = [], 0
    for v, ln in zip(g["paths"][q], W.path_lengths(g, q)):
        out.append((pos, pos + ln, v))
        pos += ln
    return out


class Cases:
    def __init__(self, seed=SEED):
        rng = np.random.default_rng(seed)
        g = self.graph = W.graph()
        texts = self.texts = g["texts"]
        self.node_seq = {k + 1: s for k, s in enumerate(g["node_seq"])}
        self.reads, self.truth, self.kind = [], [], []

        def add(kind, read, truth):
            self.reads.append(read)
            self.truth.append(truth)
            self.kind.append(kind)

        for r in range(N_MIXED):
            read, truth = _edited_read(rng, texts, 2 * int(rng.integers(0, W.N_HAP)), MIXED_LEN, int(rng.integers(0, MAX_EDITS + 1)), r >= N_MIXED // 2)
            add("mixed", read, truth)
        for r in range(N_HEAVY):
            read, truth = _edited_read(rng, texts, 2 * int(rng.integers(0, W.N_HAP)), MIXED_LEN, int(rng.integers(3, HEAVY_EDITS + 1)), r >= N_HEAVY // 2)
            add("heavy", read, truth)
        for q in END_SEQS:
            ls = len(texts[q])
            for a in HANG:
                add("end", _rand(rng, a) + texts[q][:END_LEN - a], (q, -a, []))
                add("end", texts[q][ls - (END_LEN - a):] + _rand(rng, a), (q, ls - (END_LEN - a), []))
        for special in ("n", "lower", "other"):
            for r in range(N_BYTE):
                read, truth = _edited_read(rng, texts, 2 * int(rng.integers(0, W.N_HAP)), MIXED_LEN, int(rng.integers(0, 4)), r % 2 == 1, special, 1 + r % 3)
                add("byte_" + special, read, truth)
        known = {t[i:i + MIN_LEN] for t in texts for i in range(len(t) - MIN_LEN + 1)}
        fresh = lambda read: all(read[i:i + MIN_LEN] not in known for i in range(len(read) - MIN_LEN + 1))
        n_random = 0
        while n_random < 8:
            read = _rand(rng, MIXED_LEN)
            if fresh(read):
                add("none", read, None)
                n_random += 1
        for read in (b"A" * MIXED_LEN, b"", _rand(rng, 1), _rand(rng, 11)):
            assert fresh(read)
            add("none", read, None)
        for n in (12, 13):
            read = _rand(rng, n)
            while not fresh(read):
                read = _rand(rng, n)
            add("none", read, None)
        for _ in range(6):
            add("stranger", _rand(rng, MIXED_LEN), None)
        self._short_nodes()
        self.classes = sorted(set(self.kind), key=self.kind.index)

    def _short_nodes(self):
        g, texts = self.graph, self.texts
        for q in (0, 3, 6, 9):  # a read that starts at the last base of a node, one that ends on the first base of a node
            vs, ls = visits(g, q), len(texts[q])
            s, e, _ = next(v for v in vs if v[1] - v[0] >= 2 and v[0] > 200)
            self._cut("node_last", q, e - 1, e - 1 + END_LEN)
            s, e, _ = next(v for v in vs if v[1] - v[0] >= 2 and v[0] > ls // 2)
            self._cut("node_first", q, s + 1 - END_LEN, s + 1)
        long_nodes = [(q, v) for q in (0, 1, 4, 7, 10, 13) for v in visits(g, q) if v[1] - v[0] >= 30]
        for q, (s, e, _) in long_nodes[3::9][:8]:
            self._cut("node_inside", q, s + 1, e - 1)
        for q, (s, e, _) in long_nodes[5::9][:6]:
            self._cut("node_whole", q, s, e)
        n_runs = 0
        for q in range(len(texts)):  # two 1-bp visits in a row (a 1-bp node next to a 1-bp allele), in the middle of the read
            vs = visits(g, q)
            runs = [a[0] for a, b in zip(vs, vs[1:]) if a[1] - a[0] == 1 and b[1] - b[0] == 1]
            if runs and n_runs < 6:
                self._cut("one_bp", q, runs[0] - END_LEN // 2, runs[0] + END_LEN // 2)
                n_runs += 1
        assert n_runs == 6

    def _cut(self, kind, q, a, b):
        assert 0 <= a < b <= len(self.texts[q])
        self.reads.append(self.texts[q][a:b])
        self.truth.append((q, a, []))
        self.kind.append(kind)

    def of(self, *kinds):
        """the read numbers of the classes whose name starts with one of kinds"""
        return [r for r, k in enumerate(self.kind) if k.startswith(kinds)]

    def candidates(self):
        """the planted candidate (sequence, diagonal) of every read, None without a truth"""
        return [None if t is None else (t[0], t[1]) for t in self.truth]


CASES = Cases()


def kept(texts, truth, read_len, rec, band, widen=0):
    """whether the bound edits <= planted cost has to hold for a read, from its truth and its align record alone: the winner's text holds the
    source stretch as it is (at whatever offset), and the planted alignment, moved there, stays within `band` of the record's diagonal.  The
    planted alignment is then a valid path of the banded table on the winner -- it touches no text outside the stretch --, and a banded optimum
    cannot exceed a feasible path.  widen: the stretch is lengthened by that many symbols on both sides before it is looked up (cut at the ends
    of the source sequence).  Whatever is kept with widen > 0 is kept with 0, so 0 asserts the bound on the most reads; the tests count both."""
    q, o, edits = truth
    win = int(rec["seq"])
    if win >= len(texts):
        return False
    a, b = max(0, o - widen), min(len(texts[q]), o + source_length(read_len, edits) + widen)
    stretch, cells, diag = texts[q][a:b], planted_cells(truth, read_len), int(rec["diag"])
    at = texts[win].find(stretch)
    while at >= 0:
        if all(abs(j + at - a - i - diag) <= band for i, j in cells):
            return True
        at = texts[win].find(stretch, at + 1)
    return False


def check_kept_bound(cases, align_reads, band, reads, capped):
    """the kept-read bound over `reads`: every kept read has edits <= the planted cost; capped: no more than MAX_LEFT_OUT of them may be left
    out (the mixed reads at band 31; a narrower band leaves out every read whose indels outgrow it, whatever the library does).  Returns
    (kept, left out, kept with the stretch widened by the band)"""
    keep = [r for r in reads if kept(cases.texts, cases.truth[r], len(cases.reads[r]), align_reads[r], band)]
    wide = sum(kept(cases.texts, cases.truth[r], len(cases.reads[r]), align_reads[r], band, widen=band) for r in keep)
    for r in keep:
        assert int(align_reads["edits"][r]) <= planted_cost(cases.truth[r][2]), (r, band, int(align_reads["edits"][r]), planted_cost(cases.truth[r][2]))
    assert not capped or len(reads) - len(keep) <= MAX_LEFT_OUT, (band, len(keep), len(reads))
    return len(keep), len(reads) - len(keep), wide


def class_counts(align, walk, steps):
    """the classes of tests/test_gaf_replay_cpu.py's pinned counts over the records of all reads; steps: the step list of every read"""
    a, w = align, walk
    return dict(ins=int((a["n_ins"] > 0).sum()), dels=int((a["n_del"] > 0).sum()), both=int(((a["n_ins"] > 0) & (a["n_del"] > 0)).sum()),
                clip_lo=int((a["clip_lo"] > 0).sum()), clip_hi=int((a["clip_hi"] > 0).sum()), many_steps=int((w["n_steps"] > 8).sum()),
                one_step=int((w["n_steps"] == 1).sum()), reverse_step=sum(any(int(s) & 1 for s in st) for st in steps), star=int((w["n_steps"] == 0).sum()))
