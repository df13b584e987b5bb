"""Cases of the read mapq stage (test_mapq_cpu.py on the CPU, test_gpu_mapq.py and test_gpu_cli_mapq.py on the GPU).  Pure Python / numpy: nothing
of the library is called here.

On the variation graph of tests/walk_cases.py (8 haplotypes, both strands):
  walk        the 200 error-free reads of walk_cases.cut_reads: most occur on two to eight haplotypes, always at one place of the graph
  indel_mid   reads of 60 bases: 61 bases of a haplotype with the middle one (index 30) deleted, half of them reverse-complemented.  The 61 bases are
              taken where all haplotypes run through the same nodes, so every haplotype carries the read on two neighbouring diagonals, 30 bases
              (and what chance adds) on each: the two tie or nearly tie, and the second one is a list candidate or an extra
  none        reads no MEM places: bytes that are no bases
A collection of its own (near_copy): one path of 1500 bases, forward and reversed, cut into nodes of 64; the 100 bases at 200 are copied to 900 with
the base at +50 substituted.  An error-free read of the first copy is one MEM with one occurrence, and the second copy is no placement at all; so the
reads are 60 bases of the first copy with one read error (a substituted base), 18 positions from the copies' difference, both at least 10 bases from
either end.  The error cuts the read into two MEMs: both occur in the first copy (coverage 59), the one that does not hold the copies' difference
also in the second, which is the next coverage level.  The first copy scores 59 - P, the second 58 - 2 P: P + 1 units down.
The pairs are those of mates_cases.CASES and rescue_cases.CASES; chunk_tables() cuts their twinned collections into nodes of CHUNK bases, every
path forward on sequence 2p and reversed on 2p + 1, so that the two copies of a repeat are two places of the graph."""
import numpy as np

import walk_cases as WC

CHUNK = 37
N_INDEL, N_NONE, N_NEAR = 40, 6, 20
INDEL_AT = 30
NEAR_LEN, NEAR_A, NEAR_B, NEAR_COPY, NEAR_SUB, NEAR_NODE, NEAR_READ, NEAR_ERR = 1500, 200, 900, 100, 50, 64, 60, 18


def graph_tables(g):
    """(path_offsets, path_nodes, visit_length) of the walk graph, as Index.paths() gives them"""
    pn = g["path_nodes"]
    return g["path_offsets"], pn, g["node_length"][(pn >> np.uint64(1)).astype(np.int64) - 1].astype(np.uint32)


def chunk_tables(lens, chunk=CHUNK):
    """(path_offsets, path_nodes, visit_length, node_length) of a twinned collection whose path p (sequences 2p forward, 2p + 1 reversed) is cut into
    nodes of `chunk` bases, the last one shorter; node ids from 1"""
    assert len(lens) % 2 == 0 and all(lens[q] == lens[q + 1] for q in range(0, len(lens), 2))
    po, pn, vl, nl, node = [0], [], [], [], 1
    for q in range(0, len(lens), 2):
        sizes = [min(chunk, lens[q] - at) for at in range(0, lens[q], chunk)]
        ids = list(range(node, node + len(sizes)))
        node += len(sizes)
        nl += sizes
        pn += [i << 1 for i in ids]
        vl += sizes
        po.append(len(pn))
        pn += [i << 1 | 1 for i in reversed(ids)]
        vl += list(reversed(sizes))
        po.append(len(pn))
    return np.array(po, np.uint64), np.array(pn, np.uint64), np.array(vl, np.uint32), np.array(nl, np.uint32)


def indel_mid(g, n=N_INDEL, seed=WC.SEED):
    """(truth, reads): truth[r] = (sequence, offset of the 61 bases); the windows lie where every forward haplotype runs through the same nodes"""
    rng = np.random.default_rng(seed + 2)
    fwd = g["paths"][0::2]
    common = set(fwd[0]).intersection(*[set(p) for p in fwd[1:]])
    truth, reads = [], []
    while len(reads) < n:
        h = int(rng.integers(0, WC.N_HAP))
        text, lengths = g["texts"][2 * h], WC.path_lengths(g, 2 * h)
        o = int(rng.integers(0, len(text) - WC.READ_LEN))
        at, inside = 0, True
        for node, ln in zip(g["paths"][2 * h], lengths):  # every node the window [o, o + 61) meets is common to all haplotypes
            if at < o + WC.READ_LEN + 1 and at + ln > o and node not in common:
                inside = False
            at += ln
        if not inside:
            continue
        piece = text[o:o + WC.READ_LEN + 1]
        read = piece[:INDEL_AT] + piece[INDEL_AT + 1:]
        if len(reads) % 2 == 0:
            truth.append((2 * h, o)); reads.append(read)
        else:
            truth.append((2 * h + 1, len(text) - o - WC.READ_LEN - 1)); reads.append(WC.revcomp(read))
    return truth, reads


def none_reads(n=N_NONE, length=WC.READ_LEN):
    return [bytes([b"NRYK"[(k + i) % 4] for i in range(length)]) for k in range(n)]


class NearCopy:
    """seqs, raw, lens, tables (path_offsets, path_nodes, visit_length), node_length; reads, truth[r] = (seq, diag) in the first copy, other[r] = the
    same in the second"""

    def __init__(self):
        rng = np.random.default_rng(7411)
        s = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=NEAR_LEN)].tobytes())
        s[NEAR_B:NEAR_B + NEAR_COPY] = s[NEAR_A:NEAR_A + NEAR_COPY]
        s[NEAR_B + NEAR_SUB] = b"ACGT"[(b"ACGT".index(s[NEAR_B + NEAR_SUB]) + 1) % 4]
        fwd = bytes(s)
        self.seqs = [fwd, WC.revcomp(fwd)]
        self.raw = b"".join(x + b"\n" for x in self.seqs)
        self.lens = [NEAR_LEN, NEAR_LEN]
        po, pn, vl, nl = chunk_tables(self.lens, NEAR_NODE)
        self.tables, self.node_length = (po, pn, vl), nl
        self.reads, self.truth, self.other = [], [], []
        for k, o in enumerate(range(1, NEAR_COPY - NEAR_READ + 1, 2)):  # the copies differ at read position 50 - o: 49 down to 11
            piece = bytearray(fwd[NEAR_A + o:NEAR_A + o + NEAR_READ])
            at = NEAR_SUB - o
            err = at - NEAR_ERR if at >= NEAR_READ // 2 else at + NEAR_ERR  # the read error: the MEM on its far side has at least 12 bases and occurs in both copies
            piece[err] = b"ACGT"[(b"ACGT".index(piece[err]) + 2) % 4]
            piece = bytes(piece)
            if k % 2 == 0:
                self.reads.append(piece); self.truth.append((0, NEAR_A + o)); self.other.append((0, NEAR_B + o))
            else:
                self.reads.append(WC.revcomp(piece))
                self.truth.append((1, NEAR_LEN - NEAR_A - o - NEAR_READ)); self.other.append((1, NEAR_LEN - NEAR_B - o - NEAR_READ))
        assert len(self.reads) == N_NEAR


NEAR = NearCopy()
