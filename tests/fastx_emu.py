"""The record rules of pgx_batch_upload_text / pgx_fastx_cut (include/pgx.h) restated in Python, and writers of the three
formats from a (cat, offs) batch.

Lines: the text split at '\\n'; a last line without its newline counts, nothing follows a final newline.
  LINES  every non-empty line is a read, '\\r' kept (std::getline in the reference's find_mems).
  FASTQ  strict 4-line records '@' / sequence / '+' / quality; a trailing '\\r' stripped from each line; quality length ==
         sequence length; a text that ends inside a record is an error.
  FASTA  a '>' line plus the lines up to the next '>' line, concatenated ('\\r' stripped); blank lines add nothing; a
         non-blank line before the first '>' is an error.
Every FASTA / FASTQ record is a read, an empty one included.  Errors: FastxError(record (1-based), byte of the line, text)."""
import numpy as np

LINES, FASTA, FASTQ = 0, 1, 2
NAMES = {LINES: "LINES", FASTA: "FASTA", FASTQ: "FASTQ"}


class FastxError(ValueError):
    def __init__(self, fmt, record, byte, what):
        super().__init__("%s record %d (byte %d): %s" % (NAMES[fmt], record, byte, what))
        self.record, self.byte = record, byte


def lines(text):
    """[(start, bytes of the line without its '\\n')]"""
    out, at, n = [], 0, len(text)
    while at < n:
        nl = text.find(b"\n", at)
        end = n if nl < 0 else nl
        out.append((at, text[at:end]))
        at = end + 1
    return out


def _strip(line):
    return line[:-1] if line.endswith(b"\r") else line


def parse(text, fmt):
    """-> (list of sequences as bytes, list of record start bytes); FastxError on a malformed text"""
    text = bytes(text)
    ls = lines(text)
    seqs, starts = [], []
    if fmt == LINES:
        for at, l in ls:
            if l:
                seqs.append(l)
                starts.append(at)
    elif fmt == FASTQ:
        for r in range(0, len(ls), 4):
            rec = ls[r:r + 4]
            at = rec[0][0]
            if not rec[0][1].startswith(b"@"):
                raise FastxError(fmt, r // 4 + 1, at, "header line does not start with '@'")
            if len(rec) < 4:
                raise FastxError(fmt, r // 4 + 1, at, "truncated record (%d of 4 lines)" % len(rec))
            if not rec[2][1].startswith(b"+"):
                raise FastxError(fmt, r // 4 + 1, rec[2][0], "third line does not start with '+'")
            s, q = _strip(rec[1][1]), _strip(rec[3][1])
            if len(q) != len(s):
                raise FastxError(fmt, r // 4 + 1, rec[3][0], "quality length %d != sequence length %d" % (len(q), len(s)))
            seqs.append(s)
            starts.append(at)
    elif fmt == FASTA:
        cur = None
        for at, l in ls:
            if l.startswith(b">"):
                if cur is not None:
                    seqs.append(b"".join(cur))
                cur = []
                starts.append(at)
            elif cur is None:
                if _strip(l):
                    raise FastxError(fmt, 1, at, "text before the first '>'")
            else:
                cur.append(_strip(l))
        if cur is not None:
            seqs.append(b"".join(cur))
    else:
        raise ValueError("unknown format %r" % fmt)
    return seqs, starts


def cut(text, fmt, want):
    """pgx_fastx_cut: the first line start L >= want that passes the format's test (len(text) if none)"""
    text = bytes(text)
    n = len(text)
    ls = lines(text)
    for k, (at, l) in enumerate(ls):
        if at < want:
            continue
        if fmt == LINES and l:
            return at
        if fmt == FASTA and l.startswith(b">"):
            return at
        if fmt == FASTQ and l.startswith(b"@") and k + 2 < len(ls) and ls[k + 2][1].startswith(b"+"):
            return at if k + 3 < len(ls) else n
    if fmt not in (LINES, FASTA, FASTQ):
        raise ValueError("unknown format %r" % fmt)
    return n


def to_batch(seqs):
    """list of bytes -> (cat uint8, offs uint64) as pgx_batch_upload takes them"""
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs]) if seqs else []
    cat = np.frombuffer(b"".join(seqs), dtype=np.uint8) if seqs else np.zeros(0, np.uint8)
    return cat.copy(), offs


def _reads(cat, offs):
    cat = np.asarray(cat, dtype=np.uint8)
    return [cat[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(offs) - 1)]


def _qual(rng, n):
    q = rng.integers(33, 75, size=n, dtype=np.uint8)
    if n:  # quality lines that start with '@' (64) and '+' (43) now and then: the cut must not take them for a record start
        q[0] = rng.choice([64, 43, int(q[0])])
    return q.tobytes()


def write_fastq(cat, offs, crlf=False, seed=0):
    rng = np.random.default_rng(seed)
    eol = b"\r\n" if crlf else b"\n"
    out = []
    for i, s in enumerate(_reads(cat, offs)):
        out += [b"@read%d extra" % i, eol, s, eol, b"+" if i % 2 else b"+read%d" % i, eol, _qual(rng, len(s)), eol]
    return b"".join(out)


def write_fasta(cat, offs, width=0, crlf=False):
    """width 0: one sequence line per record; otherwise wrapped at `width` columns.  Headers hold a '>' of their own"""
    eol = b"\r\n" if crlf else b"\n"
    out = []
    for i, s in enumerate(_reads(cat, offs)):
        out += [b">read%d a>b" % i, eol]
        if width:
            for a in range(0, len(s), width):
                out += [s[a:a + width], eol]
        elif s:
            out += [s, eol]
    return b"".join(out)


def write_lines(cat, offs, blank_every=0, crlf=False):
    eol = b"\r\n" if crlf else b"\n"
    out = []
    for i, s in enumerate(_reads(cat, offs)):
        out += [s, eol]
        if blank_every and i % blank_every == 0:
            out.append(b"\n")
    return b"".join(out)
