"""Case tables of the index route at the ends of its sequences (test_index_route_cases.py on the CPU, test_gpu_text_image_borders.py and
test_gpu_index_route_borders.py on the GPU).  Pure Python / numpy: nothing of the library is called here.

TEXT_CASES   name -> newline-terminated collection (<= 20 kB), grouped by TEXT_GROUPS: totals on every word residue and around the blocks
             of the pack / unpack kernels, sequence counts around the blocks of the mark / seqlen kernels, sequence ends and starts on
             every residue of a text word, N next to endmarkers, the longest sequence in every place, identical sequences, and
             empty sequences between others.  Three things bound what a case can be:
               - an index opens only with all of A C G T in its text (an encoded .ri wants sigma 5 or 6), so every case holds all four;
               - a collection that holds every sequence next to its reverse complement has an even number of sequences and an even
                 total, so the odd totals and the odd sequence counts (1, 255, 257, and 3 / 257 identical ones) are forward-only, and the
                 sequence counts come a second time as pairs (510, 512, 514 sequences);
               - the LCE image exists from 4096 symbols on, so every group holds bidirectional cases of that size: both routes of the
                 text image run on every group.
             Empty sequences: the host builder and pgx_index_open accept them next to others (a collection of empty sequences alone has
             no alphabet and is refused), so `empty_between` and `empty_first_last` are kept.
READ_CASES   one collection of twelve i.i.d. sequences, each followed by its reverse complement, and reads whose intended placement
             follows from the text alone: a core of >= 20 symbols cut from a known (sequence, offset) that occurs nowhere else, and junk
             bases around it that differ from the text symbol they face.  truth[r] is (seq, diag), None (no MEM of 12 symbols: no
             candidate), or for the reads of the shared-prefix pair A, B the two candidates [(A, diag), (B, diag)]: their core is the end
             of A, which B holds too; one substituted base follows and then up to 11 symbols of B's extra part -- too short for a MEM of
             their own, so that both placements score the same and the verify stage has to pick B (whole span, one mismatch) over A
             (span clipped at the end of A).  Without the substitution the whole read is one MEM that occurs in B alone and A is no
             candidate at all.
"""
import numpy as np

MIN_LEN = 12  # the run's min_len in the GPU tier: no 12 symbols of a read may occur off its intended diagonal
LCE_MIN = 4096  # the LCE image exists from this many symbols on (ensure_lce)
ACGT = b"ACGT"
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_ACGT = np.frombuffer(ACGT, np.uint8)


def rc(s):
    return bytes(s).translate(_COMP)[::-1]


def join(seqs):
    return b"".join(bytes(s) + b"\n" for s in seqs)


def split(raw):
    return raw.split(b"\n")[:-1]


def bidir(fwd):
    out = []
    for s in fwd:
        out += [bytes(s), rc(s)]
    return out


def is_bidirectional(raw):
    seqs = split(raw)
    return len(seqs) % 2 == 0 and all(seqs[k + 1] == rc(seqs[k]) for k in range(0, len(seqs), 2))


def starts(raw):
    """text position of the first symbol of every sequence (of its endmarker for an empty one)"""
    out, at = [], 0
    for s in split(raw):
        out.append(at)
        at += len(s) + 1
    return out


def _rand(rng, n, p_n=0.0):
    if not n:
        return b""
    s = _ACGT[rng.integers(0, 4, size=n)].copy()
    if p_n:
        s[rng.random(n) < p_n] = ord("N")
    return s.tobytes()


def _lens_summing(rng, total, k):
    """k lengths >= 4 that sum to total"""
    assert total >= 4 * k
    cuts = np.sort(rng.integers(0, total - 4 * k + 1, size=k - 1))
    return (np.diff(np.concatenate(([0], cuts, [total - 4 * k]))) + 4).tolist()


def _total_case(n):
    """a collection of exactly n symbols, endmarkers included: even n as three sequences and their reverse complements, odd n forward-only"""
    rng = np.random.default_rng(7000 + n)
    if n % 2 == 0:
        raw = join(bidir(_rand(rng, k, 0.02) for k in _lens_summing(rng, n // 2 - 3, 3)))
    else:
        raw = join(_rand(rng, k, 0.02) for k in _lens_summing(rng, n - 3, 3))
    assert len(raw) == n
    return raw


def _filler(rng, n=2100):
    return [_rand(rng, n, 0.01)]


TEXT_CASES, TEXT_GROUPS = {}, {}


def _add(group, name, raw):
    assert name not in TEXT_CASES and len(raw) <= 20000 and raw.endswith(b"\n")
    TEXT_CASES[name] = raw
    TEXT_GROUPS.setdefault(group, []).append(name)


# ---- totals: every residue of a word of eight symbols; one block of the pack / unpack kernels is 256 words = 2048 symbols
RESIDUE_TOTALS = tuple(range(4104, 4112))
BLOCK_TOTALS = (2047, 2048, 2049, 4095, 4096, 4097)
for _n in RESIDUE_TOTALS + BLOCK_TOTALS:
    _add("totals", "total_%d" % _n, _total_case(_n))

# ---- sequence counts: one block of pgx_text_mark_kernel / pgx_lce_seqlen_kernel is 256 sequences
SEQ_COUNTS_FORWARD = (1, 255, 257)  # odd: forward-only
SEQ_COUNTS_PAIRED = (2, 256, 510, 512, 514)  # every sequence next to its reverse complement
for _k in SEQ_COUNTS_FORWARD:
    _rng = np.random.default_rng(7100 + _k)
    _add("n_seq", "n_seq_%d" % _k, join(_rand(_rng, int(ln), 0.03) for ln in (_rng.integers(1, 14, size=_k) if _k > 1 else [60])))
for _k in SEQ_COUNTS_PAIRED:
    _rng = np.random.default_rng(7100 + _k)
    _add("n_seq", "n_seq_%d" % _k, join(bidir(_rand(_rng, int(ln), 0.03) for ln in (_rng.integers(*((14, 24) if _k == 256 else (4, 14)), size=_k // 2) if _k > 2 else [2100]))))

# ---- word borders: sequence 2 of `ends_r` has its last symbol on text position = r (mod 8), so its endmarker on r + 1 and the start of
# sequence 3 on r + 2: the eight cases put a last symbol, an endmarker and a first symbol on every residue
for _r in range(8):
    _rng = np.random.default_rng(7200 + _r)
    _add("word_borders", "ends_%d" % _r, join(bidir([_rand(_rng, 4), _rand(_rng, 16 + (_r - 9) % 8)] + _filler(_rng))))

# ---- N next to endmarkers, the one thing pgx_text_mark_kernel tells apart
_rng = np.random.default_rng(7300)
_add("n_symbols", "n_before_end", join(bidir([_rand(_rng, 30) + b"N", _rand(_rng, 11) + b"NN"] + _filler(_rng))))
_add("n_symbols", "n_first", join(bidir([b"N" + _rand(_rng, 30), _rand(_rng, 9)] + _filler(_rng))))
_add("n_symbols", "all_n", join(bidir([_rand(_rng, 13), b"N" * 9, _rand(_rng, 6)] + _filler(_rng))))
_add("n_symbols", "n_alone", join(bidir([_rand(_rng, 13), b"N", _rand(_rng, 6)] + _filler(_rng))))
_add("n_symbols", "n_alone_first_last", join(bidir([b"N"] + _filler(_rng) + [b"N"])))
_add("n_symbols", "length_one", join(bidir([_rand(_rng, 21), b"G", b"A"] + _filler(_rng) + [b"T"])))
_add("n_symbols", "small_with_n", join(bidir([b"ACGTN", b"N", b"NNN", b"G", b"NACGT"])))

# ---- the longest sequence (the index's max_length is its length + 1: pgx_lce_seqlen_kernel and the scatter split a packed value by it)
# first, last and in the middle, next to a sequence exactly one symbol shorter
_rng = np.random.default_rng(7400)
_add("longest", "longest_first", join(bidir([_rand(_rng, 2100), _rand(_rng, 2099), _rand(_rng, 20)])))
_add("longest", "longest_last", join(bidir([_rand(_rng, 20), _rand(_rng, 2099), _rand(_rng, 2100)])))
_add("longest", "longest_middle", join(bidir([_rand(_rng, 20), _rand(_rng, 2100), _rand(_rng, 2099), _rand(_rng, 9)])))
_add("longest", "longest_forward_only", join([_rand(_rng, 70), _rand(_rng, 71), _rand(_rng, 1)]))

# ---- identical sequences: only endmarkers break the ties.  A palindrome is its own reverse complement, so c copies of one are a
# bidirectional collection for even c
IDENTICAL = (2, 3, 256, 257)
_rng = np.random.default_rng(7500)
_half = _rand(_rng, 1050)
_add("identical", "identical_2", join([_half + rc(_half)] * 2))
_add("identical", "identical_3", b"GATTACAGC\n" * 3)
_half = _rand(_rng, 8)
_add("identical", "identical_256", join([_half + rc(_half)] * 256))
_add("identical", "identical_257", b"GATTACAGC\n" * 257)

# ---- empty sequences between others (accepted by the host builder and by pgx_index_open: see the docstring)
_rng = np.random.default_rng(7600)
_add("empty", "empty_between", join(bidir([_rand(_rng, 7), b"", _rand(_rng, 8), b""] + _filler(_rng))))
_add("empty", "empty_first_last", join(bidir([b""] + _filler(_rng) + [b"", b""])))
_add("empty", "empty_small", b"ACGT\n\nACGT\n\n")



# ---------------------------------------------------------------------------------------------------------------------------------
# READ_CASES
FORWARD_LENGTHS = (300, 1, 8, 9, 23, 40, 250, 310, 200, 400, 350, 280)  # sequence 2 k is forward sequence k, 2 k + 1 its reverse complement
A_FWD, B_FWD, EXTRA = 6, 7, 60  # B = A + 60 more symbols: a shared haplotype prefix
JUNK = (1, 7, 8, 9)


class ReadCases:
    """raw, seqs, starts; reads, truth, kinds (one class name a read) and core (the read's [a, b) that was cut from the text, None without)"""

    def __init__(self):
        rng = np.random.default_rng(8004)  # (a seed without a chance repeat of MIN_LEN symbols under a read: 4366 i.i.d. symbols hold 0.6 such pairs on average)
        fwd = [_rand(rng, k) for k in FORWARD_LENGTHS]
        fwd[B_FWD] = fwd[A_FWD] + _rand(rng, EXTRA)
        self.seqs = bidir(fwd)
        self.raw = join(self.seqs)
        self.starts = starts(self.raw)
        self.n_seq = len(self.seqs)
        self.reads, self.truth, self.kinds, self.core = [], [], [], []
        self._rng = rng
        self._build()

    # -- pieces
    def _other(self, *avoid):
        """a base that is none of `avoid` (byte values; anything outside A C G T avoids nothing)"""
        ok = [c for c in ACGT if c not in avoid]
        return ok[int(self._rng.integers(0, len(ok)))]

    def _junk(self, q, diag, at, n):
        """n bases for read positions at .. at + n of a read on (q, diag): each differs from the text symbol it faces, where there is one"""
        out = bytearray()
        for i in range(at, at + n):
            g = self.starts[q] + diag + i
            out.append(self._other(self.raw[g] if 0 <= g < len(self.raw) else 0))
        return bytes(out)

    def _put(self, kind, read, truth, core):
        self.reads.append(bytes(read))
        self.truth.append(truth)
        self.kinds.append(kind)
        self.core.append(core)

    def _overhang(self, kind, q, off, n_core, front, back):
        """front junk bases, seqs[q][off : off + n_core], back junk bases"""
        diag = off - front
        read = self._junk(q, diag, 0, front) + self.seqs[q][off:off + n_core] + self._junk(q, diag, front + n_core, back)
        self._put(kind, read, (q, diag), (front, front + n_core))

    def _build(self):
        rng, seqs = self._rng, self.seqs
        last = self.n_seq - 1
        long_ones = [0, 17, 18, 21, last]  # sequence 0, three in the middle, the last of the text (not A or B: their ends occur twice)
        # 1. the core begins at the sequence start / ends at the sequence end, junk of 1, 7, 8, 9 hangs over
        for q in long_ones:
            for a in JUNK:
                for n_core in (30 - a, 29 + a, 64):
                    self._overhang("front_%d" % a, q, 0, n_core, a, 0)
                    self._overhang("back_%d" % a, q, len(seqs[q]) - n_core, n_core, 0, a)
        # 2. both at once on a sequence shorter than the read: the whole sequence is the core
        for q in (8, 9, 10, 11):  # 23 and 40 symbols and their reverse complements
            for a in JUNK:
                for b in JUNK:
                    if 30 <= a + len(seqs[q]) + b <= 80:
                        self._overhang("both", q, 0, len(seqs[q]), a, b)
        # 3. reads that end exactly on the last symbol or start exactly on the first; a few wholly inside
        for q in long_ones + [10, 11]:
            for n_core in (30, 40):
                self._overhang("exact_end", q, len(seqs[q]) - n_core, n_core, 0, 0)
                self._overhang("exact_start", q, 0, n_core, 0, 0)
        for q in (0, 19, last):
            for off in (1, 7, 33):
                self._overhang("inside", q, off, 50, 0, 0)
        # 4. the end of A, one substituted base, then symbols of B's extra part; and the mirror image on the reverse complements, where the
        #    extra part comes first: RC(B) = RC(extra) + RC(A)
        qa, qb = 2 * A_FWD, 2 * B_FWD
        la = len(seqs[qa])
        for k in (26, 30, 45):
            for ext in (3, 8, 11):  # (3: the segment scores tie at penalty 4 and the matches decide)
                if not 30 <= k + 1 + ext <= 80:
                    continue
                b = seqs[qb]
                read = b[la - k:la] + bytes([self._other(b[la])]) + b[la + 1:la + 1 + ext]
                self._put("ab_end", read, [(qa, la - k), (qb, la - k)], (0, k))
                rb = seqs[qb + 1]  # RC(A) starts at EXTRA in it
                read = rb[EXTRA - 1 - ext:EXTRA - 1] + bytes([self._other(rb[EXTRA - 1])]) + rb[EXTRA:EXTRA + k]
                self._put("ab_start", read, [(qa + 1, -(ext + 1)), (qb + 1, EXTRA - 1 - ext)], (ext + 1, ext + 1 + k))
        # 5. one base deleted or inserted d symbols from a sequence end: the short side holds no MEM, the band meets the end of the sequence
        for q in (0, 16, last):
            s, ls = seqs[q], len(seqs[q])
            for d in (2, 5, 9):
                while s[ls - d] == s[ls - d - 1] or s[d] == s[d - 1]:  # (the base behind a deletion must not continue the match)
                    d += 1
                assert d + 1 < MIN_LEN  # (the short side, with a neighbour that happens to match, stays below a MEM)
                self._put("del_end", s[ls - 50:ls - d - 1] + s[ls - d:], (q, ls - 50), (0, 50 - d - 1))
                self._put("ins_end", s[ls - 50:ls - d] + bytes([self._other(s[ls - d], s[ls - d - 1])]) + s[ls - d:], (q, ls - 50), (0, 50 - d))
                self._put("del_start", s[:d] + s[d + 1:50], (q, 1), (d, 49))
                self._put("ins_start", s[:d] + bytes([self._other(s[d - 1], s[d])]) + s[d:50], (q, -1), (d + 1, 51))
            # a run of three: at band 3 the path walks to the band's edge next to the sequence end
            d = 9
            while s[ls - d] == s[ls - d - 3] or d >= MIN_LEN:
                d -= 1
            self._put("del3_end", s[ls - 53:ls - d - 3] + s[ls - d:], (q, ls - 53), (0, 50 - d))
            self._put("ins3_start", s[:d] + self._junk(q, -3, d, 3) + s[d:50], (q, -3), (d + 3, 53))
        # 6. reads without a MEM: random bases, N and lower case, an empty read
        for n in (30, 47, 80):
            self._put("no_mem", _rand(rng, n), None, None)
        self._put("no_mem", b"N" * 40, None, None)
        self._put("no_mem", seqs[0][100:140].lower(), None, None)
        self._put("no_mem", seqs[0][100:111] + b"N" + seqs[0][112:123] + b"N" + seqs[0][124:135], None, None)  # 11 symbols at a time
        self._put("empty", b"", None, None)


READ_CASES = ReadCases()
_add("reads", "read_cases", READ_CASES.raw)  # the collection of the reads goes through the text image's routes too

PGI_CASES = tuple(names[0] for names in TEXT_GROUPS.values())  # one case a group is saved as an image file and reopened

PENALTIES = (1, 4)
BANDS = (0, 1, 3, 8, 31)
MAX_CANDS = (1, 16)


def winner_truth(truth, max_cand):
    """the (seq, diag) the verify stage has to name for a read: the table's truth; of a shared-prefix pair B at max_cand > 1 and the first
    placement at max_cand == 1 (the place record names the smallest (seq, diag) of the tied ones)"""
    if truth is None or isinstance(truth, tuple):
        return truth
    return truth[1] if max_cand > 1 else min(truth)


def truth_candidates(truth, max_cand):
    """the candidates the verify stage gets for a read, in placement order"""
    if truth is None:
        return []
    if isinstance(truth, tuple):
        return [truth]
    return sorted(truth)[:max_cand]


def border_counts(seq_lens, read_lens, verify_recs, align_recs):
    """the border classes reached, counted over the records of a verify and an align result of the same reads (numpy record arrays)"""
    v, a = verify_recs, align_recs
    placed = a["seq"] != 0xFFFFFFFF
    ls = np.array([seq_lens[int(q)] if ok else -1 for q, ok in zip(a["seq"], placed)], dtype=np.int64)
    span = v["span_hi"].astype(np.int64) - v["span_lo"]
    aligned = placed & (span > 0)
    return dict(no_sequence=int((~placed).sum()), clip_lo=int((a["clip_lo"] > 0).sum()), clip_hi=int((a["clip_hi"] > 0).sum()),
                span_short=int((placed & (span < np.asarray(read_lens, dtype=np.int64))).sum()),
                text_end_is_ls=int((aligned & (a["text_end"].astype(np.int64) == ls)).sum()),
                text_start_is_0=int((aligned & (a["text_start"] == 0)).sum()), band_hit=int((a["band_hit"] > 0).sum()))


# the counts of border_counts at max_cand 16, penalty 4 on READ_CASES by band, pinned here so that the GPU tier asserts them without an
# emulator; test_index_route_cases.py computes them from the tables with the emulators and asserts these numbers
EXPECTED_COUNTS = {
    0: dict(no_sequence=7, clip_lo=134, clip_hi=131, span_short=203, text_end_is_ls=147, text_start_is_0=150, band_hit=0),
    1: dict(no_sequence=7, clip_lo=134, clip_hi=131, span_short=203, text_end_is_ls=147, text_start_is_0=149, band_hit=34),
    3: dict(no_sequence=7, clip_lo=134, clip_hi=131, span_short=203, text_end_is_ls=149, text_start_is_0=147, band_hit=4),
    8: dict(no_sequence=7, clip_lo=134, clip_hi=131, span_short=203, text_end_is_ls=149, text_start_is_0=147, band_hit=0),
    31: dict(no_sequence=7, clip_lo=134, clip_hi=131, span_short=203, text_end_is_ls=149, text_start_is_0=147, band_hit=0),
}
# read records of READ_CASES that change under the mutations (a), (b), (c) of test_index_route_cases.py (max_cand 16, penalty 4, band 8)
MUTATION_COUNTS = (131, 131, 134)
