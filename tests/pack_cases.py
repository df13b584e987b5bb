"""The stated tables of tests/test_gpu_pack_borders.py: the smallest shapes at which the pack kernels can go wrong, each a dict that
pgx_ffi.read_pack_arrays and pack_emu.read_pack take alike (seq_offsets, visit_offsets, visit_nodes, visit_length, seq, text_start, op_offsets,
ops, keep).  TILE is PGX_SCAN_BLOCK_ITEMS, the fold's tile; 64 and 512 are the WALK image's word and directory block."""
import numpy as np

import pack_emu as E

TILE = 2048
NO = E.NO_SEQUENCE
I, D, S, EQ, X = E.OP_I, E.OP_D, E.OP_S, E.OP_EQ, E.OP_X


def make(paths, reads, keep=None):
    """paths: per sequence a list of (node << 1 | rev, length); reads: (seq, text_start, [(op, length), ...])"""
    so, vo, vn, vl = [0], [0], [], []
    for path in paths:
        vn += [v for v, _ in path]
        vl += [ln for _, ln in path]
        so.append(so[-1] + sum(ln for _, ln in path))
        vo.append(len(vn))
    oo, ops = [0], []
    for _, _, cigar in reads:
        ops += [(ln << 4) | op for op, ln in cigar]
        oo.append(len(ops))
    return dict(seq_offsets=np.array(so, np.uint64), visit_offsets=np.array(vo, np.uint64), visit_nodes=np.array(vn, np.uint64), visit_length=np.array(vl, np.uint32),
                seq=np.array([q for q, _, _ in reads], np.uint32), text_start=np.array([a for _, a, _ in reads], np.uint64), op_offsets=np.array(oo, np.uint64),
                ops=np.array(ops, np.uint32), keep=None if keep is None else np.array(keep, np.uint8))


def chain(total, lengths, first_id=1, rev_every=3):
    """a path of `total` symbols over fresh ids with the lengths taken in turn (the last cut), every rev_every-th visit reversed"""
    path, k = [], 0
    while total:
        ln = min(lengths[k % len(lengths)], total)
        path.append((((first_id + k) << 1) | (1 if k % rev_every == rev_every - 1 else 0), ln))
        total -= ln
        k += 1
    return path


def word_and_directory_borders():
    """intervals that start on every bit residue on both sides of a 64-bit word border, of the 512-position directory border and of 1024, and end on
    every residue before, on and behind it"""
    reads = []
    for B in (64, 512, 1024):
        for a in range(B - 66, B + 2):
            if a < 0:
                continue
            for e in (a + 1, B - 1, B, B + 1, a + 65, B + 64 + a % 64):
                if e > a:
                    reads.append((0, a, [(EQ, e - a)]))
    return make([chain(1300, (7, 13, 64, 1, 2, 100, 63, 65))], reads)


def tile_borders(n):
    """a collection of n positions (tdiff holds n + 1): intervals that end one before, on and one behind every tile border that exists, and on n"""
    ends = sorted({e for t in range(TILE, n + TILE, TILE) for e in (t - 1, t, t + 1) if 0 < e <= n} | {n})
    reads = [(0, max(0, e - 40), [(EQ, e - max(0, e - 40))]) for e in ends]
    reads += [(0, 0, [(EQ, n)]), (0, n - 1, [(X, 1)]), (0, 5, [(EQ, max(1, n - 300))])]
    reads += [(0, t, [(EQ, 1)]) for t in range(TILE - 1, n, TILE)] + [(0, t, [(EQ, min(3, n - t))]) for t in range(TILE, n, TILE)]
    return make([chain(n, (1024, 1000, 23, 1, 512))], reads)


def visit_sizes():
    """visits of 1, 2, 1023 and 1024 symbols in both orientations; every node visited by several sequences, forward and reversed"""
    A, B, C, Dn = (1, 1), (2, 2), (3, 1023), (4, 1024)
    fwd = [(i << 1, ln) for i, ln in (A, B, C, Dn)]
    rev = [((i << 1) | 1, ln) for i, ln in (Dn, C, B, A)]
    paths = [fwd, rev, [fwd[1], fwd[3], rev[0], rev[3]], [rev[0], fwd[0], fwd[2]]]
    reads = []
    for q, path in enumerate(paths):
        total = sum(ln for _, ln in path)
        reads += [(q, 0, [(EQ, total)]), (q, 0, [(EQ, 1)]), (q, total - 1, [(EQ, 1)]), (q, 1, [(EQ, 2)]), (q, 2, [(X, 1030)]), (q, total - 1025, [(EQ, 1024)]), (q, 3, [(EQ, 1022)])]
    return make(paths, reads)


def sequence_ends():
    """an interval that ends on its sequence's last position next to one that starts on the next sequence's first; empty sequences between and
    at both ends; reads without a candidate; reads the filter drops"""
    paths = [[], [(2, 4), (4, 6)], [], [], [(5, 6), (6, 3), (2, 4)], []]
    reads = [(1, 5, [(EQ, 5)]), (4, 0, [(EQ, 4)]), (1, 0, [(EQ, 10)]), (4, 9, [(EQ, 4)]), (NO, 0, []), (NO, 7, [(EQ, 3)]), (4, 2, [(EQ, 9)]), (1, 9, [(X, 1)]), (4, 12, [(EQ, 1)]),
             (1, 3, [(S, 5)]), (4, 0, [(EQ, 13)]), (4, 6, [(S, 2), (I, 3)]), (NO, 0, [(EQ, 2)])]
    keep = [1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1, 0, 0]  # (the last two: dropped by the filter, but no placed reads, so not "filtered" either)
    return make(paths, reads, keep)


def cigars():
    """leading and trailing S; an I between two =; a D that leaves a hole of exactly its length; a D across a node border; an = over three and more
    nodes; neighbouring = X =; an I first and last; a D alone"""
    paths = [chain(60, (5,), 1, 2), chain(40, (5, 7), 20, 4)]
    reads = [(0, 3, [(S, 4), (EQ, 10), (S, 2)]), (0, 10, [(EQ, 4), (I, 3), (EQ, 6)]), (0, 20, [(EQ, 3), (D, 2), (EQ, 5)]), (0, 2, [(EQ, 2), (D, 3), (EQ, 2)]),
             (0, 1, [(EQ, 17)]), (0, 30, [(EQ, 26)]), (1, 4, [(EQ, 3), (X, 1), (EQ, 4)]), (1, 0, [(I, 2), (EQ, 5), (I, 1)]), (1, 11, [(D, 4)]), (1, 20, [(X, 2), (D, 1), (X, 2), (I, 1), (X, 2)]),
             (1, 30, [(S, 1), (EQ, 1), (D, 8), (EQ, 1), (S, 1)]), (0, 59, [(EQ, 1)])]
    return make(paths, reads)


def deep():
    """70 000 reads on one base: a 16-bit count shows"""
    return make([[(2, 3), (4, 2)]], [(0, 3, [(EQ, 1)])] * 70000)


def gaps():
    """ids with gaps, and max_id = 2^20 with three nodes"""
    paths = [[(3 << 1, 4), ((1 << 20) << 1 | 1, 5)], [(10 << 1 | 1, 2), (3 << 1 | 1, 4)]]
    return make(paths, [(0, 1, [(EQ, 7)]), (1, 0, [(EQ, 6)]), (0, 8, [(X, 1)])])


def two_lengths():
    """ids 7 and 4 are each visited with two lengths: the smaller id is named"""
    return make([[(7 << 1, 3), (4 << 1, 5), (2 << 1, 2)], [(4 << 1 | 1, 6), (7 << 1, 4), (2 << 1, 2)]], [(0, 0, [(EQ, 3)])])


CASES = dict(word_and_directory_borders=word_and_directory_borders, tile_2047=lambda: tile_borders(TILE - 1), tile_2048=lambda: tile_borders(TILE),
             tile_2049=lambda: tile_borders(TILE + 1), tile_6145=lambda: tile_borders(3 * TILE + 1), visit_sizes=visit_sizes, sequence_ends=sequence_ends, cigars=cigars,
             deep=deep, gaps=gaps)
