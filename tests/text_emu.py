"""The text grammar of pgx_batch_format / pgx_format_result (include/pgx.h "text output") restated in plain Python -- test infrastructure.
emit() is the expected value of every format test; parse() reads a find_mems stdout back into numbers, so that the emulator itself can be
checked against the committed goldens (tests/test_format_cpu.py)."""
import re

import numpy as np

MEM_DTYPE = np.dtype([("start", "<u8"), ("end", "<u8"), ("bwt_start", "<u8"), ("size", "<i8")])

LOCATE_NONE, LOCATE_POSITIONS, LOCATE_SEQS = 0, 1, 2


def emit(res, first_seq=0, locate=LOCATE_NONE, locations=None, max_length=1):
    """(text, err_text, read_offsets) of a result dict (mem_offsets, mems, pos_offsets, positions) as bytes, bytes and a uint64 array;
    with locate, `locations` holds loc_offsets / values"""
    mo = [int(v) for v in res["mem_offsets"]]
    po = [int(v) for v in res["pos_offsets"]]
    pos = [int(v) for v in res["positions"]]
    mems = res["mems"]
    lo = [int(v) for v in locations["loc_offsets"]] if locate else None
    vals = [int(v) for v in locations["values"]] if locate else None
    out, err, offs, at = [], [], [0], 0
    for i in range(len(mo) - 1):
        piece = ["Seq: %d\n" % (first_seq + i + 1)]
        err.append("[find_all_mems] total mems=%d\n" % (mo[i + 1] - mo[i]))
        for m in range(mo[i], mo[i + 1]):
            mm = mems[m]
            size = int(mm["size"])
            piece.append("MEM START: %d, MEM END: %d BWT START: %d SIZE: %d\n" % (int(mm["start"]), int(mm["end"]), int(mm["bwt_start"]), size))
            piece.append("Number of unique positions: %d\n" % (po[m + 1] - po[m]))
            piece.append("".join("%d, " % v for v in pos[po[m]:po[m + 1]]) + "\n")
            if locate:
                v = vals[lo[m]:lo[m + 1]]
                if not v:
                    piece.append("Occurrences: %d (not located)\n" % size)
                elif locate == LOCATE_POSITIONS:
                    piece.append("Occurrences: %d\n" % size)
                    piece.append("".join("%d:%d, " % (x // max_length, x % max_length) for x in v))
                else:
                    piece.append("Sequences: %d\n" % len(v))
                    piece.append("".join("%d, " % x for x in v))
                piece.append("\n")
        piece.append("\n")
        s = "".join(piece)
        out.append(s)
        at += len(s)
        offs.append(at)
    return "".join(out).encode(), "".join(err).encode(), np.array(offs, dtype=np.uint64)


_MEM_LINE = re.compile(r"^MEM START: (\d+), MEM END: (\d+) BWT START: (\d+) SIZE: (-?\d+)$")


def parse(text):
    """a find_mems stdout without locate lines and without the timing trailer -> (result dict, first_seq): the inverse of emit()"""
    lines = text.split("\n")
    assert lines[-1] == "", "the text ends in a newline"
    lines.pop()
    mo, mems, po, pos = [0], [], [0], []
    first_seq = None
    i = 0
    while i < len(lines):
        assert lines[i].startswith("Seq: "), lines[i]
        seq = int(lines[i][5:])
        if first_seq is None:
            first_seq = seq - 1
        assert seq == first_seq + len(mo)
        i += 1
        while lines[i] != "":
            g = _MEM_LINE.match(lines[i])
            assert g, lines[i]
            mems.append(tuple(int(x) for x in g.groups()))
            assert lines[i + 1].startswith("Number of unique positions: ")
            cnt = int(lines[i + 1][len("Number of unique positions: "):])
            items = lines[i + 2].split(", ")
            assert items[-1] == "" and len(items) == cnt + 1, lines[i + 2]
            pos += [int(x) for x in items[:-1]]
            po.append(len(pos))
            i += 3
        mo.append(len(mems))
        i += 1
    res = dict(mem_offsets=np.array(mo, dtype=np.uint64), mems=np.array(mems, dtype=MEM_DTYPE) if mems else np.zeros(0, dtype=MEM_DTYPE),
               pos_offsets=np.array(po, dtype=np.uint64), positions=np.array(pos, dtype=np.uint64))
    return res, first_seq or 0
