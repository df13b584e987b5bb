"""The read placement of include/pgx.h ("read placement"), stated from first principles: per read a dictionary from (seq, diag) to a
boolean mask over the read positions -- position p is set iff some MEM of the read with an anchor on (seq, diag) covers p -- and to the
set of those MEMs; then max, ties, first and runner-up with plain Python over the dictionary.  No keys are built or sorted, there is no
running reach, and nothing of the library is called.  (The listed placements come in the order of Python's tuple comparison of
(seq, diag), which is the order the header defines; best, first and runner-up do not use that order.)

As in hits_emu, the mask has one cell per read position while the read's MEMs end below DENSE_LIMIT, and beyond that a cell is the run
of positions between two neighbouring interval borders, weighted by its length."""
import numpy as np

from hits_emu import MEM_DTYPE, NO_SEQUENCE, _cells

READ_PLACE_DTYPE = np.dtype([("best_score", "<u8"), ("next_score", "<u8"), ("best_diag", "<i8"), ("n_anchors", "<u8"), ("n_placements", "<u8"),
                             ("best_seq", "<u4"), ("n_best", "<u4"), ("best_mems", "<u4"), ("n_located", "<u4"), ("n_mems", "<u4"),
                             ("reserved", "<u4")])
PLACEMENT_DTYPE = np.dtype([("diag", "<i8"), ("score", "<u8"), ("seq", "<u4"), ("mems", "<u4")])
HEADER = b"#read\tmems\tlocated\tanchors\tplacements\tbest\tn_best\tbest_seq\tbest_pos\tbest_mems\tnext\n"


def read_place(mem_offsets, mems, loc_offsets, values, max_length):
    """dict(reads READ_PLACE_DTYPE[n_reads], place_offsets uint64[n_reads + 1], places PLACEMENT_DTYPE[...]) for MEM arrays in the form
    of the result of a run and the packed positions of a locate (loc_offsets[n_mems + 1], values)"""
    n = len(mem_offsets) - 1
    L = int(max_length)
    recs = np.zeros(n, READ_PLACE_DTYPE)
    place_offsets = np.zeros(n + 1, np.uint64)
    listed = []
    for r in range(n):
        m0, m1 = int(mem_offsets[r]), int(mem_offsets[r + 1])
        start = np.asarray(mems["start"][m0:m1], dtype=np.uint64)
        end = np.asarray(mems["end"][m0:m1], dtype=np.uint64)
        end = np.where(end > start, end, start)  # len = 0 unless end > start
        borders, weight = _cells(start, end)
        lo, hi = borders[:-1], borders[1:]
        table = {}  # (seq, diag) -> [mask over the cells, set of MEMs]
        n_anchors = n_located = 0
        for j in range(m1 - m0):
            a, b = int(loc_offsets[m0 + j]), int(loc_offsets[m0 + j + 1])
            n_anchors += b - a
            n_located += b > a
            if b == a:
                continue
            covers = (start[j] <= lo) & (hi <= end[j])
            for v in values[a:b]:
                seq, off = divmod(int(v), L)
                entry = table.setdefault((seq, off - int(start[j])), [np.zeros(len(lo), bool), set()])
                entry[0] |= covers
                entry[1].add(j)
        score = {k: int((e[0] * weight).sum(dtype=np.uint64)) for k, e in table.items()}
        h = recs[r]
        h["n_mems"], h["n_located"], h["n_anchors"], h["n_placements"] = m1 - m0, n_located, n_anchors, len(table)
        best = max(score.values()) if score else 0
        h["best_score"] = best
        if best > 0:
            ties = [k for k, s in score.items() if s == best]
            below = [s for s in score.values() if s < best]
            first = min(ties)
            h["best_seq"], h["best_diag"], h["n_best"] = first[0], first[1], min(len(ties), 0xFFFFFFFF)
            h["best_mems"] = len(table[first][1])
            h["next_score"] = max(below) if below else 0
        else:
            h["best_seq"] = NO_SEQUENCE
        for k in sorted(table):
            listed.append((k[1], score[k], k[0], len(table[k][1])))
        place_offsets[r + 1] = len(listed)
    places = np.zeros(len(listed), PLACEMENT_DTYPE)
    if listed:
        cols = list(zip(*listed))
        places["diag"], places["score"], places["seq"], places["mems"] = cols[0], cols[1], cols[2], cols[3]
    return dict(reads=recs, place_offsets=place_offsets, places=places)


def place_text(records, first_seq=0, header=True):
    """the bytes find_mems --place writes for these records: read i prints as first_seq + i + 1, best_seq and best_pos as * when no
    placement has a score"""
    out = [HEADER] if header else []
    for i, h in enumerate(records):
        none = int(h["best_score"]) == 0
        seq = b"*" if none else b"%d" % int(h["best_seq"])
        pos = b"*" if none else b"%d" % int(h["best_diag"])
        out.append(b"%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\n" % (first_seq + i + 1, int(h["n_mems"]), int(h["n_located"]), int(h["n_anchors"]),
                                                                      int(h["n_placements"]), int(h["best_score"]), int(h["n_best"]), seq, pos,
                                                                      int(h["best_mems"]), int(h["next_score"])))
    return b"".join(out)


def build_case(reads):
    """(mem_offsets, mems, loc_offsets, packed) from reads given as lists of (start, end, [(seq, off), ...]); packed(max_length) gives the
    values"""
    flat = [m for r in reads for m in r]
    mem_offsets = np.concatenate(([0], np.cumsum([len(r) for r in reads]))).astype(np.uint64)
    mems = np.zeros(len(flat), MEM_DTYPE)
    loc_offsets = np.zeros(len(flat) + 1, np.uint64)
    seqs, offs = [], []
    for i, (a, b, anchors) in enumerate(flat):
        mems["start"][i], mems["end"][i] = a, b
        mems["size"][i] = len(anchors)
        seqs += [s for s, _ in anchors]
        offs += [o for _, o in anchors]
        loc_offsets[i + 1] = len(seqs)
    seqs, offs = np.asarray(seqs, dtype=np.uint64), np.asarray(offs, dtype=np.uint64)

    def packed(max_length):
        return seqs * np.uint64(max_length) + offs

    return mem_offsets, mems, loc_offsets, packed


def random_reads(rng, n_reads, n_seq, max_length, max_mems=9, span=60, max_occ=6, big=False):
    """reads for build_case: 0 .. max_mems MEMs with strictly ascending starts, ends that abut, overlap and nest, some end <= start;
    0 .. max_occ anchors a MEM, drawn so that MEMs of a read often share a diagonal (a few true placements a read plus noise), diagonals
    that are negative, and offsets up to max_length - 1; big: one MEM of some read ends at 2^33"""
    reads = []
    for _ in range(n_reads):
        k = int(rng.integers(0, max_mems + 1))
        starts = np.sort(rng.choice(span, k, replace=False))
        homes = [(int(rng.integers(0, n_seq)), int(rng.integers(-3, max_length - span))) for _ in range(3)]
        read = []
        for s in starts:
            s = int(s)
            e = max(s + int(rng.integers(-3, span)), 0)
            anchors = set()
            for _ in range(int(rng.integers(0, max_occ + 1))):
                if rng.random() < 0.7:
                    q, d = homes[int(rng.integers(0, 3))]
                    d += int(rng.integers(0, 2)) if rng.random() < 0.2 else 0
                else:
                    q, d = int(rng.integers(0, n_seq)), int(rng.integers(-s, max_length - s))
                off = d + s
                if 0 <= off < max_length:
                    anchors.add((q, off))
            anchors = list(anchors)
            rng.shuffle(anchors)
            read.append((s, e, [(int(q), int(o)) for q, o in anchors]))
        reads.append(read)
    if big:
        cand = [r for r in reads if r]
        if cand:
            r = cand[int(rng.integers(0, len(cand)))]
            j = int(rng.integers(0, len(r)))
            r[j] = (r[j][0], 1 << 33, r[j][2])
    return reads


def random_case(rng, n_reads, n_seq, max_length, **kw):
    """(mem_offsets, mems, loc_offsets, values) of random_reads"""
    mem_offsets, mems, loc_offsets, packed = build_case(random_reads(rng, n_reads, n_seq, max_length, **kw))
    return mem_offsets, mems, loc_offsets, packed(max_length)
