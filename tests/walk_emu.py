"""Pure-Python restatement of the read walk -- TEST INFRASTRUCTURE ONLY.

The definitions of include/pgx.h "read walk" as plain loops, with no bit vector and no rank: the marks of a collection from the tag of
every BWT row, the visits of every sequence from its marks, the walk of a text stretch by stepping through the path node by node, and
the GAF line find_mems --gaf prints from an align record and a walk."""
import numpy as np

NO_SEQUENCE = 0xFFFFFFFF
WALK_STEPS = 1
WALK_DTYPE = np.dtype([("path_len", "<u8"), ("path_start", "<u8"), ("path_end", "<u8"), ("n_steps", "<u4"), ("seq", "<u4")])
_OPS = {1: "I", 2: "D", 4: "S", 7: "=", 8: "X"}


def marks_from_row_tags(sa, tags, n_seq, max_length):
    """per sequence the sorted list of (offset, node << 1 | rev) of the positions whose row tag has offset 0; rows below n_seq are endmarkers"""
    out = [[] for _ in range(n_seq)]
    for i in range(n_seq, len(sa)):
        tag = int(tags[i])
        if tag & 0x3FF == 0:
            out[int(sa[i]) // max_length].append((int(sa[i]) % max_length, tag >> 10))
    for m in out:
        m.sort()
    return out


def visits_from_marks(marks, seq_lengths):
    """(path_offsets, path_nodes, visit_length): visit k of a sequence runs from its mark to the next one, the last to the sequence's end"""
    po, pn, vl = [0], [], []
    for m, ls in zip(marks, seq_lengths):
        for k, (off, node) in enumerate(m):
            pn.append(node)
            vl.append((m[k + 1][0] if k + 1 < len(m) else int(ls)) - off)
        po.append(len(pn))
    return np.array(po, dtype=np.uint64), np.array(pn, dtype=np.uint64), np.array(vl, dtype=np.uint32)


def walk(nodes, lengths, start, end):
    """the walk of [start, end) on a path stated as its nodes and their lengths: (path_len, path_start, path_end, steps)"""
    if end <= start:
        return 0, 0, 0, []
    pos, steps, first, path_len = 0, [], None, 0
    for node, ln in zip(nodes, lengths):
        ln = int(ln)
        if pos < end and pos + ln > start:  # the visit [pos, pos + ln) meets the stretch
            if first is None:
                first = pos
            steps.append(int(node))
            path_len += ln
        pos += ln
    assert first is not None and end <= pos, "stretch outside its path"
    return path_len, start - first, start - first + (end - start), steps


def read_walk(path_offsets, path_nodes, visit_length, seq, text_start, text_end, flags=WALK_STEPS):
    """what pgx_read_walk_arrays / pgx_batch_walked return: dict(reads, step_offsets, steps)"""
    n = len(seq)
    recs = np.zeros(n, dtype=WALK_DTYPE)
    offs, steps = [0], []
    for r in range(n):
        q = int(seq[r])
        recs[r]["seq"] = q
        if q != NO_SEQUENCE:
            a, b = int(path_offsets[q]), int(path_offsets[q + 1])
            pl, ps, pe, st = walk(path_nodes[a:b], visit_length[a:b], int(text_start[r]), int(text_end[r]))
            recs[r]["path_len"], recs[r]["path_start"], recs[r]["path_end"], recs[r]["n_steps"] = pl, ps, pe, len(st)
            steps += st
        offs.append(len(steps))
    lst = bool(flags & WALK_STEPS)
    return dict(reads=recs, step_offsets=np.array(offs, dtype=np.uint64) if lst else None, steps=np.array(steps, dtype=np.uint64) if lst else None)


def gaf_line(number, length, align, wrec, steps, ops):
    """one line of find_mems --gaf, without the newline: align a pgx_read_align record, wrec a pgx_read_walk record, steps its node << 1 | rev list,
    ops the read's CIGAR words (length << 4 | op)"""
    if int(wrec["n_steps"]) == 0:
        return "\t".join([str(number), str(length)] + ["*"] * 9 + ["255"])
    path = "".join(("<" if int(s) & 1 else ">") + str(int(s) >> 1) for s in steps)
    nm, mm, ni, nd = int(align["n_match"]), int(align["n_mismatch"]), int(align["n_ins"]), int(align["n_del"])
    cigar = "".join("%d%s" % (int(x) >> 4, _OPS[int(x) & 15]) for x in ops if int(x) & 15 != 4)
    cols = [number, length, int(align["clip_lo"]), length - int(align["clip_hi"]), "+", path, int(wrec["path_len"]), int(wrec["path_start"]), int(wrec["path_end"]),
            nm, nm + mm + ni + nd, 255, "NM:i:%d" % int(align["edits"]), "hs:i:%d" % int(align["seq"]), "ho:i:%d" % int(align["text_start"]), "cg:Z:" + cigar]
    return "\t".join(str(c) for c in cols)
