"""Case tables of the device read parser (pgx_batch_upload_text, csrc/pgx_fastx_kernels.hip): one text per case, each placed on a border
of the kernels' geometry.  test_fastx_cases_cpu.py asserts on the CPU that the literals below are the kernels' own, that every text holds the
border it claims and that tests/fastx_emu.py accepts or refuses it as the table says; test_gpu_fastx_borders.py uploads every text and
compares the reads the batch then holds (pgx_batch_reads) with the emulator's, byte for byte.

A case claims what can be said without a parser: bytes at absolute positions (`at`), the number of lines (`n_lines`), the sequence bytes the
reads sum to (`total`) and whether the text is well-formed (`ok`).  What the reads are, and the message, record and byte of a refusal, come
from the emulator."""
import functools
import os

import numpy as np

import fastx_emu as E

LINES, FASTA, FASTQ = E.LINES, E.FASTA, E.FASTQ

CHUNK = 16                      # bytes per load of the count and lines passes
ROUND = 4096                    # bytes a block loads per round: 256 threads x CHUNK
TILE = 16384                    # PGX_FASTX_TILE: bytes per block of the count and lines passes (PGX_FASTX_ROUNDS = 4 rounds)
LINE_BLOCK = 256                # lines per block of the role and records passes
SCAN1_TILE_ITEMS = 4096         # items per tile of the one-pass scan (tile counts, line contributions, record flags)
COPY_BLOCK = 4096               # output bytes per block of the copy pass
COPY_THREADS = 4096 // 16       # its threads: 16 output bytes each, one aligned store
LONGEST_GRID_READS = 2048 * 256  # reads the longest-read pass covers before its grid strides

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_X = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x.newline_separated")


class Case:
    def __init__(self, name, fmt, text, ok, why, at=None, n_lines=None, total=None):
        self.name, self.fmt, self.text, self.ok, self.why = "%s-%s" % (name, E.NAMES[fmt].lower()), fmt, bytes(text), ok, why
        self.at, self.n_lines, self.total = dict(at or {}), n_lines, total

    def __repr__(self):
        return self.name


def _rand(rng, n):
    return _ACGT[rng.integers(0, 4, size=n)].tobytes() if n else b""


@functools.lru_cache(maxsize=None)
def _x_seqs():
    return [s for s in open(_X, "rb").read().split(b"\n") if s]


def _indexed(rng, n):
    """n symbols of the text behind the x_index fixture: pieces of up to 150 symbols, 2 % substituted (a search finds MEMs in them)"""
    out, seqs = [], _x_seqs()
    left = n
    while left:
        s = seqs[int(rng.integers(0, len(seqs)))]
        k = min(left, 150, len(s))
        a = int(rng.integers(0, len(s) - k + 1))
        piece = np.frombuffer(s[a:a + k], dtype=np.uint8).copy()
        flip = rng.random(k) < 0.02
        piece[flip] = _ACGT[rng.integers(0, 4, int(flip.sum()))]
        out.append(piece.tobytes())
        left -= k
    return b"".join(out)


def _fastq(reads, eol=b"\n", final=True):
    out = []
    for i, s in enumerate(reads):
        out += [b"@r%d" % i, eol, s, eol, b"+", eol, b"I" * len(s), eol]
    t = b"".join(out)
    return t if final or not out else t[:len(t) - len(eol)]


# ---- a. one newline (or the pair \r \n) at absolute byte p
NEWLINE_AT = (0, 15, 16, 17, 4095, 4096, 4097, 16383, 16384, 16385, 32767, 32768)


def newline_case(fmt, p, crlf):
    """the first line end of the text, for FASTA / FASTQ the end of the first sequence line, is '\\n' at byte p (crlf: '\\r' at p, '\\n' at
    p + 1).  p = 0 leaves no room for a header: the line is blank (FASTA: accepted before the first '>'; FASTQ: a header without '@')"""
    rng = np.random.default_rng(100 + 2 * p + crlf)
    eol = b"\r\n" if crlf else b"\n"
    name = "nl_%s%d" % ("crlf_" if crlf else "", p)
    at = {p: 13, p + 1: 10} if crlf else {p: 10}
    why = "line end at byte %d of chunk / round / tile" % p
    tail = _rand(rng, 37)
    if fmt == LINES:
        t = _rand(rng, p) + eol + tail + eol
        return Case(name, fmt, t, True, why, at, 2, p + 37 + (2 if crlf else 0))  # (the '\r' stays in a LINES read)
    head = (b">" if fmt == FASTA else b"@") + b"h" + eol
    if p == 0:
        t = eol + (b">h\nACGT\n" if fmt == FASTA else b"@h\nACGT\n+\nIIII\n")
        return Case(name, fmt, t, fmt == FASTA, why, at, 3 if fmt == FASTA else 5, 4 if fmt == FASTA else None)
    k = p - len(head)
    assert k >= 0
    s = _rand(rng, k)
    if fmt == FASTA:
        t = head + s + eol + tail + eol + b">second" + eol + tail + eol
        return Case(name, fmt, t, True, why, at, 5, k + 2 * 37)
    t = head + s + eol + b"+" + eol + b"J" * k + eol + b"@second" + eol + tail + eol + b"+second" + eol + b"K" * 37 + eol
    return Case(name, fmt, t, True, why, at, 8, k + 37)


# ---- b. texts of n bytes, with and without the final newline
TEXT_LENGTHS = (1, 2, 15, 16, 17, 4095, 4096, 4097, 16383, 16384, 16385, 32768, 32769)


def length_case(fmt, n, final):
    """a text of exactly n bytes whose last line has (final) or lacks its newline"""
    rng = np.random.default_rng(200 + 2 * n + final)
    name = "len_%d%s" % (n, "_nl" if final else "")
    why = "text of %d bytes: the last chunk / round / tile is partial by %d" % (n, n % CHUNK)
    at = {n - 1: 10} if final else {}
    if fmt == LINES:
        t = _rand(rng, n - 1) + b"\n" if final else _rand(rng, n)
        return Case(name, fmt, t, True, why, at, 1, n - final)
    if fmt == FASTA:
        if n <= 2:
            t = {(1, False): b">", (2, False): b">h", (1, True): b"\n", (2, True): b">\n"}[(n, final)]
            return Case(name, fmt, t, True, why, at, 1, 0)
        t = b">\n" + _rand(rng, n - 2 - final) + (b"\n" if final else b"")
        return Case(name, fmt, t, True, why, at, 2, n - 2 - final)
    if n <= 2:  # no room for four lines: refused
        t = {(1, False): b"@", (2, False): b"@h", (1, True): b"\n", (2, True): b"@\n"}[(n, final)]
        return Case(name, fmt, t, False, why, at, 1, None)
    body = n - final - 5  # '@' [h] \n seq \n + \n qual
    head = b"@" if body % 2 == 0 else b"@h"
    k = (body - (len(head) - 1)) // 2
    s = _rand(rng, k)
    t = head + b"\n" + s + b"\n+\n" + b"I" * k + (b"\n" if final else b"")
    return Case(name, fmt, t, True, why, at, 4, k)


def tiny_cases():
    out = []
    for fmt in (LINES, FASTA, FASTQ):
        out.append(Case("one_A", fmt, b"A", fmt == LINES, "a text of one byte", {0: 65}, 1, 1 if fmt == LINES else None))
        out.append(Case("one_nl", fmt, b"\n", fmt != FASTQ, "a text of one newline", {0: 10}, 1, 0 if fmt != FASTQ else None))
        out.append(Case("one_cr", fmt, b"\r", fmt != FASTQ, "a text of one '\\r': a read in LINES, blank in FASTA", {0: 13}, 1,
                        {LINES: 1, FASTA: 0, FASTQ: None}[fmt]))
    out.append(Case("qual_ends_cr", FASTQ, b"@h\r\nACGT\r\n+\r\nIIII\r", True, "the last quality line ends in '\\r' without '\\n'", {17: 13}, 4, 4))
    return out


# ---- c. line counts
LINE_COUNTS = (255, 256, 257, 4095, 4096, 4097)


def line_count_case(fmt, k):
    """k lines.  FASTQ is well-formed only where k is a multiple of 4: the other counts end inside a record on a block border"""
    rng = np.random.default_rng(300 + k)
    name = "lines_%d" % k
    why = "%d lines: role / records block of %d, scan tile of %d" % (k, LINE_BLOCK, SCAN1_TILE_ITEMS)
    lens = rng.integers(1, 6, size=k)
    if fmt == LINES:
        t = b"".join(_rand(rng, int(n)) + b"\n" for n in lens)
        return Case(name, fmt, t, True, why, None, k, int(lens.sum()))
    if fmt == FASTA:  # a header on every third line
        t = b"".join((b">h%d\n" % i) if i % 3 == 0 else _rand(rng, int(lens[i])) + b"\n" for i in range(k))
        return Case(name, fmt, t, True, why, None, k, int(sum(lens[i] for i in range(k) if i % 3)))
    reads = [_rand(rng, int(n)) for n in lens[:(k + 3) // 4]]
    t = b"".join(l + b"\n" for l in _fastq(reads).split(b"\n")[:k])
    return Case(name, fmt, t, k % 4 == 0, why, None, k, int(lens[:k // 4].sum()) if k % 4 == 0 else None)


def newline_tile_cases():
    out = []
    full = b"\n" * TILE
    why = "a tile of %d newlines: every chunk mask is 0xFFFF" % TILE
    follow = {LINES: b"ACGTA\n", FASTA: b">r\nACGTA\n", FASTQ: b"@r\nACGTA\n+\nIIIII\n"}
    for fmt in (LINES, FASTA, FASTQ):
        ok = fmt != FASTQ
        out.append(Case("newline_tile", fmt, full, ok, why, {0: 10, TILE - 1: 10}, TILE, 0 if ok else None))
        out.append(Case("newline_tile_then_read", fmt, full + follow[fmt], ok, why + ", one read behind it", {TILE - 1: 10, TILE: follow[fmt][0]},
                        TILE + follow[fmt].count(b"\n"), 5 if ok else None))
    for fmt in (LINES, FASTA):
        out.append(Case("blank_lines", fmt, b"\n" * 5, True, "blank lines only: no read, no copy pass", None, 5, 0))
        out.append(Case("blank_crlf_lines", fmt, b"\r\n" * 3, True, "'\\r' lines only: reads in LINES, nothing in FASTA", None, 3, 3 if fmt == LINES else 0))
    out.append(Case("headers_only", FASTA, b">a\n>b\n>c\n", True, "three reads and no sequence byte: the copy pass is not launched", None, 3, 0))
    return out


# ---- d. the copy pass
def _fasta(reads, width, eol=b"\n", blank_every=0):
    out, k = [], 0
    for i, s in enumerate(reads):
        out += [b">r%d" % i, eol]
        for a in range(0, len(s), width):
            out += [s[a:a + width], eol]
            k += 1
            if blank_every and k % blank_every == 0:
                out.append(eol)
    return b"".join(out)


def copy_cases():
    out = []
    rng = np.random.default_rng(400)
    reads = [_indexed(rng, n) for n in (40, 1, 0, 33, 16, 17, 300)]
    total = sum(len(s) for s in reads)
    for crlf in (False, True):
        for blank in (0, 3):
            name = "width_1%s%s" % ("_crlf" if crlf else "", "_blanks" if blank else "")
            out.append(Case(name, FASTA, _fasta(reads, 1, b"\r\n" if crlf else b"\n", blank), True,
                            "one symbol per line: %d lines feed one %d-byte store" % (CHUNK, CHUNK), None, None, total))
    for w in (15, 16, 17):
        out.append(Case("width_%d" % w, FASTA, _fasta(reads, w), True, "lines of %d symbols against stores of %d" % (w, CHUNK), None, None, total))
    for tot in (4095, 4096, 4097, 8192):
        rs = [_indexed(rng, n) for n in (1000, 0, tot - 3000, 2000)]
        why = "%d sequence bytes: the copy pass has %d block(s), the last store is %d bytes" % (tot, (tot + COPY_BLOCK - 1) // COPY_BLOCK, (tot - 1) % CHUNK + 1)
        out.append(Case("total_%d" % tot, FASTA, _fasta(rs, 60), True, why, None, None, tot))
        out.append(Case("total_%d" % tot, FASTQ, _fastq(rs), True, why, None, 16, tot))
        out.append(Case("total_%d" % tot, LINES, b"".join(s + b"\n" for s in rs), True, why, None, 4, tot))
    rs = [_indexed(rng, n) for n in (COPY_BLOCK - 6, 12, 50)]
    for fmt, t in ((FASTA, _fasta(rs, 70)), (FASTQ, _fastq(rs)), (LINES, b"".join(s + b"\n" for s in rs))):
        out.append(Case("read_over_4096", fmt, t, True, "a read of 12 bytes over output bytes %d .. %d" % (COPY_BLOCK - 6, COPY_BLOCK + 5), None, None, COPY_BLOCK + 56))
    long = _indexed(rng, 10000)
    for fmt, t in ((FASTA, b">long\n" + long + b"\n"), (FASTQ, _fastq([long])), (LINES, long + b"\n")):
        out.append(Case("line_10000", fmt, t, True, "one line of 10 000 bytes: three copy blocks read one line", {t.index(long) + 10000: 10}, None, 10000))
    a, b = _indexed(rng, 21), _x_seqs()[1][100:530]  # (b: long enough for the search behind it to find MEMs)
    for name, rs in (("empty_first", [b"", a, b]), ("empty_last", [a, b, b""]), ("empty_three", [a, b"", b"", b"", b]), ("empty_all_over", [b"", a, b"", b"", b"", b, b""])):
        out.append(Case(name, FASTA, _fasta(rs, 60), True, "empty records: offsets repeat", None, None, 451))
        out.append(Case(name, FASTQ, _fastq(rs), True, "empty records: offsets repeat", None, 4 * len(rs), 451))
    return out


# ---- e. FASTQ (and FASTA) content that looks like structure
def lookalike_cases():
    out = []
    why = "lines that start with '@', '+' or '>' where the format does not look at them"
    for i, c in enumerate(b"@+>"):
        ch = bytes([c])
        t = b"@" + ch + b"name\nACGT\n+" + ch + b"again\n" + ch + b"III\n" + b"@r2\n" + ch + b"CGT\n+\n" + ch + b"JJJ\n"
        out.append(Case("lookalike_%d" % i, FASTQ, t, True, why, {1: c}, 8, 8))
        t = b">" + ch + b"name\n" + (b"" if c == 62 else ch + b"CGT\n") + b"ACGT\n>r2 " + ch + b"\nAC\n"
        out.append(Case("lookalike_%d" % i, FASTA, t, True, why, {1: c}, None, 6 if c == 62 else 10))
    out.append(Case("no_sequence", FASTQ, b"@a\n\n+\n\n", True, "a record of four lines with an empty sequence", None, 4, 0))
    out.append(Case("no_sequence_3", FASTQ, b"@a\n\n+\n\n@b\n\r\n+\r\n\n@c\n\n+\n\n", True, "three of them, '\\r' on some lines", None, 12, 0))
    out.append(Case("seq_cr_qual_bare", FASTQ, b"@a\nACGT\r\n+\nIIII\n", True, "sequence line with '\\r', quality line without: equal after the strip", {7: 13}, 4, 4))
    out.append(Case("seq_bare_qual_cr", FASTQ, b"@a\nACGT\n+\nIIII\r\n", True, "the other way round", {14: 13}, 4, 4))
    out.append(Case("seq_cr_qual_short", FASTQ, b"@a\nACGT\r\n+\nIII\r\n", False, "lengths differ after the strip", None, 4, None))
    return out


# ---- g. the error matrix
KINDS = ("no_at", "no_plus", "qual_len")


def _records(n, seed=500):
    rng = np.random.default_rng(seed)
    return [[b"@r%d" % i, s, b"+", b"I" * len(s)] for i, s in enumerate(_rand(rng, int(k)) for k in rng.integers(1, 9, size=n))]


def _break(rec, kind):
    if kind == "no_at":
        rec[0] = b"r" + rec[0][1:]
    elif kind == "no_plus":
        rec[2] = b"-"
    elif kind == "qual_len":
        rec[3] += b"I"
    else:
        raise ValueError(kind)


def _join(recs):
    return b"".join(l + b"\n" for r in recs for l in r)


def error_cases():
    """record 65 is lines 256 .. 259: the first four of the second block of the role pass"""
    out = []
    N = 100
    for kind in KINDS:
        for pos, n in ((1, N), (65, N), (N, N)):
            recs = _records(n)
            _break(recs[pos - 1], kind)
            out.append(Case("err_%s_rec%d" % (kind, pos), FASTQ, _join(recs), False, "%s in record %d of %d" % (kind, pos, n), None, 4 * n, None))
    for pos in (1, 65, N):  # a truncated record is the last one: the text ends there
        for have in (1, 2, 3):
            recs = _records(pos)
            recs[-1] = recs[-1][:have]
            out.append(Case("err_truncated_%d_rec%d" % (have, pos), FASTQ, _join(recs), False, "record %d ends after %d of 4 lines" % (pos, have), None, 4 * pos - 4 + have, None))
            t = _join(recs)
            out.append(Case("err_truncated_%d_rec%d_no_final_nl" % (have, pos), FASTQ, t[:-1], False, "the same without the final newline", None, 4 * pos - 4 + have, None))
            recs[-1][0] = b"r"
            out.append(Case("err_truncated_%d_no_at_rec%d" % (have, pos), FASTQ, _join(recs), False, "a header without '@' on a truncated record: the header's own error", None,
                            4 * pos - 4 + have, None))
        recs = _records(pos)
        recs[-1] = [recs[-1][0], recs[-1][1], b"IIII"]
        out.append(Case("err_truncated_3_no_plus_rec%d" % pos, FASTQ, _join(recs)[:-1], False, "three lines, the third without '+': truncation (the header line) comes first", None,
                        4 * pos - 1, None))
    out.append(Case("err_truncated_3_no_plus_issue", FASTQ, b"@a\nACGT\nIIII", False, "the same, the smallest text", {8: 73}, 3, None))
    # two bad records: the earlier line wins, whichever kind it has
    for a, b in (("qual_len", "no_at"), ("no_at", "qual_len"), ("no_plus", "qual_len"), ("qual_len", "no_plus"), ("no_plus", "no_at"), ("no_at", "no_plus")):
        recs = _records(N)
        _break(recs[69], a)
        _break(recs[89], b)
        out.append(Case("err_two_late_%s_%s" % (a, b), FASTQ, _join(recs), False, "%s in record 70 (block 1), %s in record 90: the earlier wins" % (a, b), None, 4 * N, None))
        recs = _records(3000)
        _break(recs[2], a)
        for r in recs[9:]:
            _break(r, b)
        out.append(Case("err_two_first_block_%s_%s" % (a, b), FASTQ, _join(recs), False, "%s in record 3, %s in every record from 10 to 3000" % (a, b), None, 12000, None))
    recs = _records(N)
    _break(recs[69], "qual_len")
    recs[-1] = recs[-1][:2]
    out.append(Case("err_two_qual_len_truncated", FASTQ, _join(recs), False, "qual_len in record 70, the last record truncated", None, 4 * N - 2, None))
    # FASTA: text before the first '>'
    out.append(Case("before_first_blank_ok", FASTA, b"\n\r\n\n\r\n>a\nACGT\n", True, "blank and '\\r'-only lines before the first '>' are no text", None, 6, 4))
    out.append(Case("err_before_first_line0", FASTA, b"ACGT\n>a\nACGT\n", False, "text on line 0", None, 3, None))
    out.append(Case("err_before_first_behind_blanks", FASTA, b"\n\r\n\nAC\n>a\nACGT\n", False, "a non-blank line behind blank ones: its byte offset", {4: 65}, 6, None))
    out.append(Case("err_before_first_line256", FASTA, b"\n" * LINE_BLOCK + b"ACGT\n>a\nACGT\n", False, "text on line %d: the second block of the records pass" % LINE_BLOCK,
                    {LINE_BLOCK: 65}, LINE_BLOCK + 3, None))
    out.append(Case("err_before_first_last_line", FASTA, b"\r\n" * 300 + b"ACGT", False, "no '>' at all: text on the last line", {600: 65}, 301, None))
    out.append(Case("err_before_first_two", FASTA, b"\n\n\nAC\n" + b"\n" * 296 + b"GT\n>a\nA\n", False, "text on lines 3 and 300: the earlier wins", {3: 65}, 303, None))
    return out


@functools.lru_cache(maxsize=None)
def small_cases():
    out = []
    for fmt in (LINES, FASTA, FASTQ):
        for p in NEWLINE_AT:
            for crlf in (False, True):
                out.append(newline_case(fmt, p, crlf))
        for n in TEXT_LENGTHS:
            for final in (False, True):
                out.append(length_case(fmt, n, final))
        for k in LINE_COUNTS:
            out.append(line_count_case(fmt, k))
    out += tiny_cases() + newline_tile_cases() + copy_cases() + lookalike_cases() + error_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


COPY_CASE_PREFIXES = ("width_", "total_", "read_over_4096", "line_10000", "empty_")  # the cases of table d (a search runs behind them)


# ---- f. many reads, many tiles
MANY_READS = 600_000
MANY_TILES = 4100
_PHASES = (0, 15, 16, 17, 4095, 4096, 4097, 16383)


@functools.lru_cache(maxsize=None)
def many_reads_case():
    """600 000 reads of one symbol and then one of 300 from the indexed text: the reads lie beyond 2048 x 256, so the longest-read pass
    strides, and the longest read is the last one"""
    rng = np.random.default_rng(600)
    t = np.full(2 * MANY_READS, 10, dtype=np.uint8)
    t[0::2] = _ACGT[rng.integers(0, 4, size=MANY_READS)]
    last = _x_seqs()[0][200:500]
    assert len(last) == 300
    return Case("many_reads", LINES, t.tobytes() + last + b"\n", True, "%d reads > %d: the longest-read pass strides" % (MANY_READS + 1, LONGEST_GRID_READS),
                {2 * MANY_READS - 1: 10, 2 * MANY_READS + 300: 10}, MANY_READS + 1, MANY_READS + 300)


def tile_phase(t):
    """where in tile t its one newline lies"""
    return _PHASES[t] if t < len(_PHASES) else (t * 4099) % TILE


@functools.lru_cache(maxsize=None)
def _many_tiles_text():
    rng = np.random.default_rng(601)
    t = _ACGT[rng.integers(0, 4, size=MANY_TILES * TILE, dtype=np.uint8)]
    for k in range(MANY_TILES):
        t[k * TILE + tile_phase(k)] = 10
    return t


def many_tiles_case(fmt):
    """4100 tiles with one newline each: the scan of the tile counts crosses its own tile of 4096 items.  LINES: 4100 reads (the first line
    is blank, the last lacks its newline).  FASTA: byte 1 is '>', so everything behind the second line is one read"""
    t = _many_tiles_text()
    n = MANY_TILES * TILE
    why = "%d tiles > %d: the tile-count scan has two tiles" % (MANY_TILES, SCAN1_TILE_ITEMS)
    at = {0: 10, TILE + 15: 10, 2 * TILE + 16: 10, 7 * TILE + TILE - 1: 10}
    if fmt == LINES:
        return Case("many_tiles", LINES, t.tobytes(), True, why, at, MANY_TILES + 1, n - MANY_TILES)
    assert fmt == FASTA
    u = t.copy()
    u[1] = ord(">")
    header = TILE + tile_phase(1) - 1  # the bytes of line 1
    return Case("many_tiles", FASTA, u.tobytes(), True, why, {**at, 1: 62}, MANY_TILES + 1, n - MANY_TILES - header)
