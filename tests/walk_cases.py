"""The small variation graph of tests/test_gpu_walk.py and tests/test_gpu_cli_gaf.py, and the reads cut from it.

A base of about 3 kb cut into nodes of 1 to 64 bp; behind every two to four of them a bubble of two alleles (distinct sequences of 1 to 8 bp,
lengths drawn apart, so that a bubble may be an indel); 8 haplotypes that choose an allele per bubble, each held in both orientations: sequence
2 h is haplotype h, sequence 2 h + 1 its reverse complement on the reversed node list with the orientation bits flipped.  Node ids from 1."""
import numpy as np

import walk_emu as E

SEED, N_HAP, BASE, N_READS, READ_LEN, AT = 3, 8, 3000, 200, 60, 30
MAX_LEFT_OUT = N_READS // 20  # 5 %
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _rand(rng, n):
    return bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, size=n))


def revcomp(s):
    return s.translate(_COMP)[::-1]


def graph(seed=SEED):
    """dict(node_seq: sequences by id - 1, paths: node << 1 | rev lists of the 2 N_HAP sequences, texts: their bytes, and the tables
    path_offsets, path_nodes, node_length as pgx_build_tags_paths takes them)"""
    rng = np.random.default_rng(seed)
    node_seq, backbone, total = [], [], 0  # backbone: node ids, or (id, id) for a bubble
    while total < BASE:
        for _ in range(int(rng.integers(2, 5))):
            node_seq.append(_rand(rng, int(rng.integers(1, 65))))
            backbone.append(len(node_seq))
            total += len(node_seq[-1])
        a = _rand(rng, int(rng.integers(1, 9)))
        b = a
        while b == a:
            b = _rand(rng, int(rng.integers(1, 9)))
        node_seq += [a, b]
        backbone.append((len(node_seq) - 1, len(node_seq)))
        total += len(a)
    paths, texts = [], []
    for h in range(N_HAP):
        fwd = [(x if isinstance(x, int) else x[int(rng.integers(0, 2))]) << 1 for x in backbone]
        text = b"".join(node_seq[(v >> 1) - 1] for v in fwd)
        paths += [fwd, [v ^ 1 for v in reversed(fwd)]]
        texts += [text, revcomp(text)]
    po = np.concatenate(([0], np.cumsum([len(p) for p in paths]))).astype(np.uint64)
    pn = np.array([v for p in paths for v in p], dtype=np.uint64)
    nl = np.array([len(s) for s in node_seq], dtype=np.uint32)
    return dict(node_seq=node_seq, paths=paths, texts=texts, path_offsets=po, path_nodes=pn, node_length=nl)


def path_lengths(g, q):
    return [int(g["node_length"][(v >> 1) - 1]) for v in g["paths"][q]]


def cut_reads(g, seed=SEED):
    """N_READS error-free reads of READ_LEN bases: (truth, reads); truth[r] = (sequence, offset) the read's bytes lie at.  The first half is cut from
    the forward sequences as they are; the second half is cut from a forward sequence and reverse-complemented, so its bytes lie on the odd twin"""
    rng = np.random.default_rng(seed + 1)
    truth, reads = [], []
    for r in range(N_READS):
        h = int(rng.integers(0, N_HAP))
        text = g["texts"][2 * h]
        o = int(rng.integers(0, len(text) - READ_LEN + 1))
        piece = text[o:o + READ_LEN]
        if r < N_READS // 2:
            truth.append((2 * h, o)); reads.append(piece)
        else:
            truth.append((2 * h + 1, len(text) - o - READ_LEN)); reads.append(revcomp(piece))
    return truth, reads


def deleted(reads):
    return [r[:AT] + r[AT + 1:] for r in reads]


def walk_of(g, q, a, b):
    """(path_len, path_start, path_end, steps) of [a, b) on sequence q"""
    return E.walk(g["paths"][q], path_lengths(g, q), a, b)


def ambiguous(g, truth, reads):
    """the reads whose bytes also occur somewhere in the collection with a different walk (steps or path_start): bool[N_READS], from the texts alone"""
    out = np.zeros(len(reads), dtype=bool)
    for r, (read, (q, o)) in enumerate(zip(reads, truth)):
        assert g["texts"][q][o:o + len(read)] == read
        want = walk_of(g, q, o, o + len(read))
        for s, text in enumerate(g["texts"]):
            at = text.find(read)
            while at >= 0:
                if walk_of(g, s, at, at + len(read)) != want:
                    out[r] = True
                at = text.find(read, at + 1)
    return out
