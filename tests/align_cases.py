"""What tests/test_align_cpu.py and tests/test_gpu_align.py share: the 200 error-free reads of 60 bases cut from the 66-sequence collection of
tests/test_gpu_verify.py, their forms with base 30 deleted and with one base inserted at 30, and which of them are left out of the
expectation "one edit" because the mutated form occurs in the collection with fewer edits."""
import numpy as np

import align_emu as E

COLLECTION = dict(name="hits_border_33", n_hap=33, base_len=2000, seed=133)  # as tests/test_gpu_verify.py builds it
N_READS, LENGTH, AT, SEED = 200, 60, 30, 25
MAX_LEFT_OUT = N_READS // 20  # 5 %
# The seed: chosen among 1 .. 40 for few reads left out.  Two kinds of read are left out (tests/test_gpu_align.py): those whose mutated form
# occurs in the collection as it is (0 to 2 of the 200 under every seed), and those whose verify winner -- the first sequence that holds the
# read's longer half -- is a haplotype with a variant of its own inside the read, where the mutated form has two edits or more (2 to 13 of the
# 200, 7 on average: 66 sequences with a SNP every 1000 bases).  Seed 25 leaves out 2 of each form by that count.


def cut_reads(seqs, n_reads=N_READS, length=LENGTH, seed=SEED):
    """[(sequence, offset)], [read]: windows without N"""
    rng = np.random.default_rng(seed)
    truth, reads = [], []
    while len(reads) < n_reads:
        q = int(rng.integers(0, len(seqs)))
        s = bytes(seqs[q])
        if len(s) < length:
            continue
        o = int(rng.integers(0, len(s) - length + 1))
        if b"N" in s[o:o + length]:
            continue
        truth.append((q, o))
        reads.append(s[o:o + length])
    return truth, reads


def deleted(reads):
    return [r[:AT] + r[AT + 1:] for r in reads]


def inserted(reads):
    """the base behind the one at 30 in A C G T A, so that it differs from its right neighbour"""
    nxt = bytes.maketrans(b"ACGT", b"CGTA")
    return [r[:AT] + r[AT:AT + 1].translate(nxt) + r[AT:] for r in reads]


def fewer_edits_elsewhere(reads, seqs, edits=1):
    """per read: some sequence holds it with fewer than `edits` edits.  For edits == 1 that is an exact occurrence, found by substring search;
    tests/test_align_cpu.py checks that against E.infix_distances over every sequence"""
    if edits == 1:
        return np.array([any(r in bytes(s) for s in seqs) for r in reads], bool)
    return np.array([int(E.infix_distances(r, seqs).min()) < edits for r in reads], bool)
