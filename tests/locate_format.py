"""The two lines `find_mems --locate positions|seqs` adds to every MEM block, restated from include/pgx.h / src/find_mems.cpp, and
their splicing into a plain find_mems text -- test infrastructure for the locate CLI tests."""


def locate_lines(size, vals, mode, max_length):
    """the lines of one MEM: `vals` are its located values (packed positions for "positions", sorted unique sequence ids for
    "seqs"); no values = not located"""
    if len(vals) == 0:
        return "Occurrences: %d (not located)\n\n" % size
    if mode == "positions":
        return "Occurrences: %d\n" % size + "".join("%d:%d, " % (int(v) // max_length, int(v) % max_length) for v in vals) + "\n"
    if mode == "seqs":
        return "Sequences: %d\n" % len(vals) + "".join("%d, " % int(v) for v in vals) + "\n"
    raise ValueError(mode)


def mem_locate_lines(mems, loc_offsets, values, mode, max_length):
    """one string per MEM, in MEM order (mems: MEM_DTYPE array, loc_offsets: n_mems + 1 entries)"""
    return [locate_lines(int(mems[m]["size"]), values[int(loc_offsets[m]):int(loc_offsets[m + 1])], mode, max_length) for m in range(len(mems))]


def splice(text, per_mem):
    """insert per_mem[k] behind the positions line of the k-th MEM block of a find_mems text (`MEM START` line, `Number of unique
    positions` line, positions line)"""
    lines = text.split("\n")
    out, k, i = [], 0, 0
    while i < len(lines):
        out.append(lines[i])
        if lines[i].startswith("MEM START: "):
            assert lines[i + 1].startswith("Number of unique positions: "), lines[i + 1]
            out.append(lines[i + 1])
            assert k < len(per_mem) and per_mem[k].endswith("\n"), k
            out.append(lines[i + 2] + "\n" + per_mem[k][:-1])  # (the join puts the last newline back)
            k += 1
            i += 3
            continue
        i += 1
    assert k == len(per_mem), (k, len(per_mem))
    return "\n".join(out)
