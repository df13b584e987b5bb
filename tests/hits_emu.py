"""The read hits of include/pgx.h ("read hits"), stated from first principles: for every read and sequence a boolean mask over the read
positions -- position p is set iff some MEM of the read whose set has the sequence's bit covers p -- then max, ties and runner-up of
the mask sums with numpy.  No sweep over sorted intervals, no running reach, and nothing of the library is called.

The mask has one cell per read position while the read's MEMs end below DENSE_LIMIT.  Beyond that (a MEM that ends at 2^33) a cell
is the run of positions between two neighbouring interval borders, weighted by its length: every position of such a run is covered by
exactly the same MEMs, so the mask over the runs says the same as the mask over their positions."""
import numpy as np

NO_SEQUENCE = 0xFFFFFFFF
HIT_DTYPE = np.dtype([("best_score", "<u8"), ("next_score", "<u8"), ("covered", "<u8"), ("best_seq", "<u4"), ("n_best", "<u4"),
                      ("n_located", "<u4"), ("n_mems", "<u4")])
MEM_DTYPE = np.dtype([("start", "<u8"), ("end", "<u8"), ("bwt_start", "<u8"), ("size", "<i8")])
DENSE_LIMIT = 1 << 12
HEADER = b"#read\tmems\tlocated\tcovered\tbest\tn_best\tbest_seq\tnext\n"


def set_bits(sets, n_seq):
    """bool[n_mems, n_seq] from uint64[n_mems, W]; bits at or beyond n_seq are dropped"""
    sets = np.ascontiguousarray(sets, dtype="<u8")
    if sets.shape[0] == 0:
        return np.zeros((0, n_seq), bool)
    return np.unpackbits(sets.view(np.uint8), axis=1, bitorder="little")[:, :n_seq].astype(bool)


def pack_bits(flags, w):
    """uint64[w] from bool[n_seq]"""
    padded = np.zeros(w * 64, np.uint8)
    padded[:len(flags)] = flags
    return np.packbits(padded, bitorder="little").view("<u8").copy()


def _cells(starts, ends):
    """(borders, weights): cell c is the positions [borders[c], borders[c + 1])"""
    top = max([int(e) for e in ends] + [0])
    if top <= DENSE_LIMIT:
        borders = np.arange(top + 1, dtype=np.uint64)
    else:
        borders = np.unique(np.concatenate([np.zeros(1, np.uint64), starts, ends]).astype(np.uint64))
    return borders, np.diff(borders)


def read_hits(mem_offsets, mems, sets, n_seq):
    """dict(hits HIT_DTYPE[n_reads], best_sets uint64[n_reads, W], scores uint32[n_reads, n_seq]) for MEM arrays in the form of the result
    of a run (mem_offsets[n_reads + 1], mems with start / end) and sets uint64[n_mems, W]"""
    n = len(mem_offsets) - 1
    w = (n_seq + 63) // 64
    bits_all = set_bits(np.asarray(sets, dtype=np.uint64).reshape(-1, w), n_seq)
    hits = np.zeros(n, HIT_DTYPE)
    best_sets = np.zeros((n, w), np.uint64)
    scores = np.zeros((n, n_seq), np.uint32)
    for r in range(n):
        m0, m1 = int(mem_offsets[r]), int(mem_offsets[r + 1])
        start = np.asarray(mems["start"][m0:m1], dtype=np.uint64)
        end = np.asarray(mems["end"][m0:m1], dtype=np.uint64)
        end = np.where(end > start, end, start)  # len = 0 unless end > start
        bits = bits_all[m0:m1]
        borders, weight = _cells(start, end)
        lo, hi = borders[:-1], borders[1:]
        covers = (start[:, None] <= lo[None, :]) & (hi[None, :] <= end[:, None])  # [MEM, cell]
        mask = (bits.T.astype(np.int64) @ covers.astype(np.int64)) > 0            # [sequence, cell]
        cov = (mask * weight[None, :]).sum(axis=1, dtype=np.uint64)
        located = bits.any(axis=1)
        covered = int((covers[located].any(axis=0) * weight).sum(dtype=np.uint64))
        best = int(cov.max())
        h = hits[r]
        h["n_mems"], h["n_located"], h["covered"], h["best_score"] = m1 - m0, int(located.sum()), covered, best
        if best > 0:
            tie = cov == np.uint64(best)
            below = cov[cov < np.uint64(best)]
            h["best_seq"], h["n_best"] = int(np.flatnonzero(tie)[0]), int(tie.sum())
            h["next_score"] = int(below.max()) if len(below) else 0
            best_sets[r] = pack_bits(tie, w)
        else:
            h["best_seq"], h["n_best"], h["next_score"] = NO_SEQUENCE, 0, 0
        scores[r] = np.minimum(cov, np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return dict(hits=hits, best_sets=best_sets, scores=scores)


def sets_from_ids(loc_offsets, values, n_mems, n_seq):
    """uint64[n_mems, W] from the sorted unique sequence ids of every MEM (pgx_locate_batch's form)"""
    w = (n_seq + 63) // 64
    out = np.zeros((n_mems, w), np.uint64)
    values = np.asarray(values, dtype=np.uint64)
    m_of = np.repeat(np.arange(n_mems), np.diff(np.asarray(loc_offsets).astype(np.int64)))
    np.bitwise_or.at(out, (m_of, (values >> np.uint64(6)).astype(np.int64)), np.uint64(1) << (values & np.uint64(63)))
    return out


def hits_text(hits, first_seq=0, header=True):
    """the bytes find_mems --hits writes for these records: read i prints as first_seq + i + 1, best_seq as * when there is none"""
    out = [HEADER] if header else []
    for i, h in enumerate(hits):
        seq = b"*" if int(h["best_seq"]) == NO_SEQUENCE else b"%d" % int(h["best_seq"])
        out.append(b"%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\n" % (first_seq + i + 1, int(h["n_mems"]), int(h["n_located"]), int(h["covered"]),
                                                          int(h["best_score"]), int(h["n_best"]), seq, int(h["next_score"])))
    return b"".join(out)


def random_case(rng, n_reads, n_seq, max_mems=9, span=60, big=False):
    """(mem_offsets, mems, sets): reads with 0 .. max_mems MEMs, strictly ascending starts, ends that abut, overlap and nest, some
    end <= start, sets that are empty, sparse, dense and full, input bits at and beyond n_seq set; big: one MEM ends at 2^33"""
    w = (n_seq + 63) // 64
    counts = rng.integers(0, max_mems + 1, n_reads)
    mem_offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.uint64)
    m = int(mem_offsets[-1])
    mems = np.zeros(m, MEM_DTYPE)
    for r in range(n_reads):
        a, b = int(mem_offsets[r]), int(mem_offsets[r + 1])
        mems["start"][a:b] = np.sort(rng.choice(span, b - a, replace=False))
    length = rng.integers(-3, span, m)
    mems["end"] = (mems["start"].astype(np.int64) + length).clip(0).astype(np.uint64)
    if big and m:
        mems["end"][rng.integers(0, m)] = 1 << 33
    density = rng.choice([0.0, 0.05, 0.5, 1.0], m)[:, None]
    bits = rng.random((m, w * 64)) < density
    sets = np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(m, w).copy()
    return mem_offsets, mems, sets


def build_case(reads, n_seq):
    """(mem_offsets, mems, sets) from reads given as lists of (start, end, sequence ids)"""
    w = (n_seq + 63) // 64
    flat = [m for r in reads for m in r]
    mem_offsets = np.concatenate(([0], np.cumsum([len(r) for r in reads]))).astype(np.uint64)
    mems = np.zeros(len(flat), MEM_DTYPE)
    sets = np.zeros((len(flat), w), np.uint64)
    for i, (a, b, ids) in enumerate(flat):
        mems["start"][i], mems["end"][i] = a, b
        for q in ids:
            sets[i, q >> 6] |= np.uint64(1 << (q & 63))
    return mem_offsets, mems, sets
