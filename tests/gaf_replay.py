"""Replay of the read pipeline's last link -- TEST INFRASTRUCTURE ONLY.

What a record of pgx_batch_read_align, a record of pgx_batch_read_walk and a line of find_mems --gaf claim, checked by doing what they say: the
CIGAR is walked over the read and over the text it names, the oriented nodes of the path are spelled out and sliced, and the slice, edited by
the CIGAR, has to give back the read.  Nothing of the library, of tests/walk_emu.py's gaf_line or of tests/align_emu.py's table is used; the
one import, align_emu.infix_distances, is the unbanded optimum that no record may beat.  Every check names the read and the field.

replay_record    A (CIGAR against the text), B (walk against the graph) and the lower bound of C on one read's records
replay_bands     the two bounds of C that compare the records of one read at several bands
replay_gaf_line  the same from the text of one GAF line alone"""
import functools
import re

import align_emu

NO_SEQUENCE = 0xFFFFFFFF
KINDS = {1: "I", 2: "D", 4: "S", 7: "=", 8: "X"}  # the BAM codes of the operation words, length << 4 | code
UPPER = frozenset(b"ACGT")
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
_STEP = re.compile(r"[<>]\d+")
_CG = re.compile(r"(\d+)([=XIDS])")
_ALIGN_FIELDS = ("diag", "text_start", "text_end", "clip_lo", "clip_hi", "edits", "n_match", "n_mismatch", "n_ins", "n_del", "n_ops", "band_hit")
_WALK_FIELDS = ("path_len", "path_start", "path_end", "n_steps")


def _need(ok, number, field, *what):
    if not ok:
        raise AssertionError("read %s, %s: %s" % (number, field, " ".join(str(w) for w in what)))


def oriented(node_seq, step):
    """the bytes of node step >> 1 as the step reads them: reverse-complemented when step & 1"""
    s = bytes(node_seq[int(step) >> 1])
    return s.translate(_COMP)[::-1] if int(step) & 1 else s


def spell(node_seq, steps):
    return b"".join(oriented(node_seq, s) for s in steps)


@functools.lru_cache(maxsize=None)
def _floor(q, text):
    return int(align_emu.infix_distances(q, [text])[0])


def _edit(number, field, ops, q, t):
    """[(length, kind)] without clips over the read part q and the text part t: every operation as section A states it, both consumed exactly.
    Returns the symbol totals per kind and the cells (i, j) of the path, start included"""
    i = j = 0
    totals = {"=": 0, "X": 0, "I": 0, "D": 0}
    cells = [(0, 0)]
    before = None
    for n, kind in ops:
        _need(kind in totals, number, field, "operation", kind, "inside the alignment")
        _need(n > 0, number, field, "an operation of length 0")
        _need(kind != before, number, field, "two neighbouring", kind, "operations")
        before = kind
        for _ in range(n):
            if kind in "=X":
                _need(i < len(q) and j < len(t), number, field, "%s at read %d, text %d runs past the end (%d, %d)" % (kind, i, j, len(q), len(t)))
                same = q[i] in UPPER and q[i] == t[j]
                _need(same == (kind == "="), number, field, "%s at read %d, text %d: %r against %r" % (kind, i, j, q[i:i + 1], t[j:j + 1]))
                i, j = i + 1, j + 1
            elif kind == "I":
                _need(i < len(q), number, field, "I runs past the read's end")
                i += 1
            else:
                _need(j < len(t), number, field, "D runs past the text's end")
                j += 1
            cells.append((i, j))
        totals[kind] += n
    _need(i == len(q), number, field, "the operations consume %d read symbols of %d" % (i, len(q)))
    _need(j == len(t), number, field, "the operations consume %d text symbols of %d" % (j, len(t)))
    return totals, cells


def replay_record(read, texts, node_seq, align_rec, walk_rec, steps, ops, band=None, number="?"):
    """read: bytes; texts: the collection's sequences; node_seq: node id -> bytes; align_rec / walk_rec: one record each (anything indexed by
    field name); steps: node << 1 | rev; ops: the read's operation words; band: the band the align stage ran with, when known"""
    read = bytes(read)
    a = {f: int(align_rec[f]) for f in _ALIGN_FIELDS + ("seq",)}
    w = {f: int(walk_rec[f]) for f in _WALK_FIELDS + ("seq",)}
    steps = [int(s) for s in steps]
    ops = [(int(x) >> 4, KINDS.get(int(x) & 15, "?")) for x in ops]
    _need(w["seq"] == a["seq"], number, "walk.seq", w["seq"], "!=", a["seq"])
    _need(w["n_steps"] == len(steps), number, "n_steps", w["n_steps"], "but", len(steps), "steps")
    _need(a["n_ops"] == len(ops), number, "n_ops", a["n_ops"], "but", len(ops), "words")
    if a["seq"] == NO_SEQUENCE:
        for f in _ALIGN_FIELDS:
            _need(a[f] == 0, number, f, a[f], "in a record without a sequence")
        for f in _WALK_FIELDS:
            _need(w[f] == 0, number, f, w[f], "in a walk without a sequence")
        return
    _need(0 <= a["seq"] < len(texts), number, "seq", a["seq"], "of", len(texts))
    text = bytes(texts[a["seq"]])
    lo, hi = max(0, -a["diag"]), min(len(read), len(text) - a["diag"])
    if hi <= lo:  # the candidate does not overlap its sequence
        _need((a["clip_lo"], a["clip_hi"]) == (0, len(read)), number, "clips", a["clip_lo"], a["clip_hi"], "on an empty span of a read of", len(read))
        _need(ops == ([(len(read), "S")] if read else []), number, "ops", ops, "on an empty span")
        for f in ("text_start", "text_end", "edits", "n_match", "n_mismatch", "n_ins", "n_del", "band_hit") + _WALK_FIELDS:
            _need((a[f] if f in a else w[f]) == 0, number, f, "not 0 on an empty span")
        return
    # ---- A: the CIGAR against the text
    _need((a["clip_lo"], a["clip_hi"]) == (lo, len(read) - hi), number, "clips", a["clip_lo"], a["clip_hi"], "but the span is", lo, hi)
    _need(0 <= a["text_start"] <= a["text_end"] <= len(text), number, "text_start / text_end", a["text_start"], a["text_end"], "on", len(text), "symbols")
    inner = list(ops)
    for at, f in ((0, "clip_lo"), (-1, "clip_hi")):
        if inner and inner[at][1] == "S":
            _need(inner[at][0] == a[f] > 0, number, f, a[f], "but the S operation has", inner[at][0])
            del inner[at]
        else:
            _need(a[f] == 0, number, f, a[f], "without an S operation")
    q, t = read[lo:hi], text[a["text_start"]:a["text_end"]]
    totals, cells = _edit(number, "ops", inner, q, t)
    for f, kind in (("n_match", "="), ("n_mismatch", "X"), ("n_ins", "I"), ("n_del", "D")):
        _need(a[f] == totals[kind], number, f, a[f], "but the operations hold", totals[kind])
    _need(a["edits"] == totals["X"] + totals["I"] + totals["D"], number, "edits", a["edits"], totals)
    ks = [a["text_start"] + j - i - (a["diag"] + lo) for i, j in cells]  # the diagonal of every cell, relative to the candidate's
    if band is not None:
        _need(max(abs(k) for k in ks) <= band, number, "band", "the path leaves the band", band, "by", max(abs(k) for k in ks))
        _need(a["band_hit"] == int(band > 0 and max(abs(k) for k in ks) == band), number, "band_hit", a["band_hit"], "widest", max(abs(k) for k in ks), "band", band)
    # ---- B: the walk against the graph
    _need(len(steps) > 0, number, "n_steps", "no step for a stretch of", len(t))
    spelled = spell(node_seq, steps)
    _need(len(spelled) == w["path_len"], number, "path_len", w["path_len"], "but the nodes hold", len(spelled))
    _need(w["path_end"] - w["path_start"] == len(t), number, "path_end - path_start", w["path_start"], w["path_end"], "for a stretch of", len(t))
    _need(0 <= w["path_start"] <= w["path_end"] <= w["path_len"], number, "path_start / path_end", w["path_start"], w["path_end"], w["path_len"])
    _need(spelled[w["path_start"]:w["path_end"]] == t, number, "path", "the slice of the path is not the text stretch")
    _need(w["path_start"] < len(node_seq[steps[0] >> 1]), number, "path_start", w["path_start"], "lies behind the first node: an idle step")
    _need(w["path_len"] - w["path_end"] < len(node_seq[steps[-1] >> 1]), number, "path_end", w["path_end"], "lies before the last node: an idle step")
    # ---- C: nothing beats the unbanded optimum on that sequence
    floor = _floor(q, text)
    _need(a["edits"] >= floor, number, "edits", a["edits"], "below the unbanded optimum", floor)


def replay_bands(by_band, mismatches=None, number="?"):
    """by_band: {band: align record of one read at one candidate}; mismatches: verify's count on that candidate, when known"""
    bands = sorted(by_band)
    for b0, b1 in zip(bands, bands[1:]):
        _need(int(by_band[b1]["edits"]) <= int(by_band[b0]["edits"]), number, "edits", "grow from band", b0, "to", b1, int(by_band[b0]["edits"]), int(by_band[b1]["edits"]))
    if mismatches is not None and 0 in by_band and int(by_band[0]["seq"]) != NO_SEQUENCE:
        _need(int(by_band[0]["edits"]) == int(mismatches), number, "edits", int(by_band[0]["edits"]), "at band 0, verify's mismatches", int(mismatches))


def unplaced_line(number, length):
    """the line of a read without steps as the README states it: the read's number, its length, * in columns 3 to 11 and 255, and no tag"""
    return "\t".join([str(number), str(length)] + ["*"] * 9 + ["255"])


def replay_gaf_line(line, read, node_seq, texts=None, number=None):
    """line: one line of find_mems --gaf as str, without its newline; read: the bytes of the read of that number; texts: the collection, when
    hs / ho are to be checked against the path.  Returns the parsed fields (None for a * line)"""
    read = bytes(read)
    cols = line.split("\t")
    tag = cols[0] if number is None else number
    _need(len(cols) >= 12, tag, "columns", len(cols))
    _need(number is None or cols[0] == str(number), tag, "column 1", cols[0])
    _need(cols[1] == str(len(read)), tag, "column 2", cols[1], "for a read of", len(read))
    if "*" in cols[2:11]:
        _need(line == unplaced_line(cols[0], len(read)), tag, "* line", repr(line))
        return None
    _need(len(cols) == 16, tag, "columns", len(cols))
    _need(all(re.fullmatch(r"\d+", cols[k]) for k in (2, 3, 6, 7, 8, 9, 10, 11)), tag, "columns", "a number column is no number")
    qstart, qend, path_len, ps, pe, n_eq, n_all, mapq = (int(cols[k]) for k in (2, 3, 6, 7, 8, 9, 10, 11))
    _need(cols[4] == "+", tag, "column 5", cols[4])
    _need(mapq == 255, tag, "column 12", mapq)
    steps = _STEP.findall(cols[5])
    _need(steps and "".join(steps) == cols[5], tag, "column 6", cols[5])
    tags = {}
    for k, (name, kind) in enumerate((("NM", "i"), ("hs", "i"), ("ho", "i"), ("cg", "Z"))):
        head = "%s:%s:" % (name, kind)
        _need(cols[12 + k].startswith(head), tag, "tag " + name, cols[12 + k])
        tags[name] = cols[12 + k][len(head):]
    _need("S" not in tags["cg"], tag, "cg", "holds a soft clip")
    ops = [(int(n), kind) for n, kind in _CG.findall(tags["cg"])]
    _need("".join("%d%s" % o for o in ops) == tags["cg"] != "", tag, "cg", tags["cg"])
    _need(0 <= qstart <= qend <= len(read), tag, "columns 3 and 4", qstart, qend)
    _need(0 <= ps <= pe <= path_len, tag, "columns 8 and 9", ps, pe, path_len)
    spelled = spell(node_seq, [int(s[1:]) << 1 | (s[0] == "<") for s in steps])
    _need(len(spelled) == path_len, tag, "column 7", path_len, "but the nodes hold", len(spelled))
    totals, _ = _edit(tag, "cg", ops, read[qstart:qend], spelled[ps:pe])
    _need(qend - qstart == totals["="] + totals["X"] + totals["I"], tag, "columns 3 and 4", qstart, qend, totals)
    _need(pe - ps == totals["="] + totals["X"] + totals["D"], tag, "columns 8 and 9", ps, pe, totals)
    _need(n_eq == totals["="], tag, "column 10", n_eq, totals)
    _need(n_all == sum(totals.values()), tag, "column 11", n_all, totals)
    _need(tags["NM"] == str(totals["X"] + totals["I"] + totals["D"]), tag, "NM", tags["NM"], totals)
    _need(ps < len(node_seq[int(steps[0][1:])]), tag, "column 8", ps, "lies behind the first node")
    _need(path_len - pe < len(node_seq[int(steps[-1][1:])]), tag, "column 9", pe, "lies before the last node")
    _need(tags["hs"].isdigit() and tags["ho"].isdigit(), tag, "hs / ho", tags["hs"], tags["ho"])
    hs, ho = int(tags["hs"]), int(tags["ho"])
    if texts is not None:
        _need(hs < len(texts), tag, "hs", hs)
        _need(bytes(texts[hs])[ho:ho + pe - ps] == spelled[ps:pe] and ho + pe - ps <= len(texts[hs]), tag, "hs / ho", hs, ho, "do not hold the path's stretch")
    return dict(qstart=qstart, qend=qend, path_len=path_len, path_start=ps, path_end=pe, steps=steps, hs=hs, ho=ho, totals=totals)
