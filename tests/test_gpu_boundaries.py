"""The lengths at which the pairs kernel changes its path, pinned on purpose: the longest read of a batch around the limit of the packed reads
(launch_pairs: (15 + longest + 15) / 16 + 1 <= 24 words, i.e. up to 353 symbols) and around the 144-symbol text window of the LCE path; reads at
every phase of the 16-symbol packing word; intervals of exactly 127, 128 and 129 occurrences around PGX_LCE_MAX_OCC.  PAIRS + LCE index,
min_len 20 and 12, min_occ 1, bit for bit against the oracle."""
import os

import numpy as np
import pytest

import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import variant_cases as V

pytestmark = pytest.mark.gpu

PAIRS = [(20, 1), (12, 1)]
MODE = P.MODE_COMPAT | P.MODE_IMAGE_PAIRS
LONGEST = [143, 144, 145, 160, 336, 337, 352, 353, 354, 355, 383, 384, 385, 400]


@pytest.fixture(scope="module")
def mid(workdir):
    return V.mid_case(workdir)


@pytest.fixture(scope="module")
def index(mid):
    idx = P.Index(mid["ri_path"], mid["tags_path"], mode=MODE)
    yield idx
    idx.close()


def _cut(seqs, rng, ln):
    """ln symbols of the text without an N: the read matches end to end"""
    while True:
        s = seqs[int(rng.integers(0, len(seqs)))]
        a = int(rng.integers(0, len(s) - ln))
        r = s[a:a + ln]
        if not (r == ord("N")).any():
            return bytes(r)


def _check(index, mid, key, reads, packed):
    cat, offs = O.pack_reads(reads)
    assert int(np.diff(offs.astype(np.int64)).max()) == max(len(r) for r in reads)
    for min_len, min_occ in PAIRS:
        ref = V.oracle(mid, min_len, min_occ, key=key, cat=cat, offs=offs)
        res, t = V.run(index, cat, offs, min_len, min_occ)
        assert t.kernels & P.KERNELS_PAIRS and bool(t.kernels & P.KERNELS_PAIRS_PACKED) == packed, (key, hex(t.kernels))
        assert bool(t.kernels & P.KERNELS_PAIRS_LCE) == packed, (key, hex(t.kernels))
        V.same(res, ref)
    return ref


@pytest.mark.parametrize("longest", LONGEST)
def test_longest_read_of_the_batch(index, mid, longest):
    """1 500 reads of the usual 150 symbols and, in their middle, one read of exactly `longest`, cut from the text (the forward stages run its
    whole length); packed reads up to 353 symbols, byte windows beyond"""
    rng = np.random.default_rng(longest)
    cat, offs = W.sample_reads(mid["seqs"], 1500, 150, seed=longest, n_frac=0.01)
    usual = [bytes(cat[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)]
    long_read = _cut(mid["seqs"], rng, longest)
    ref = _check(index, mid, "longest-%d" % longest, usual[:700] + [long_read] + usual[700:], longest <= 353)
    m = ref["mems"][int(ref["mem_offsets"][700]):int(ref["mem_offsets"][701])]
    assert len(m) >= 1 and int((m["end"] - m["start"]).max()) == longest, m  # matched end to end


@pytest.mark.parametrize("phase", list(range(16)))
def test_reads_at_every_phase_of_the_packing_word(index, mid, phase):
    """a first read of `phase` symbols shifts what follows; then reads of every length 0 .. 48, each starting at a byte offset = phase mod 16
    (a filler read behind each restores the phase), a read of 353 symbols (the longest the packed form takes) at that phase, and usual reads"""
    rng = np.random.default_rng(100 + phase)
    reads = [_cut(mid["seqs"], rng, phase) if phase else b""]
    at = phase
    for ln in list(range(49)) + [353, 150, 144, 145]:
        assert at % 16 == phase
        reads.append(_cut(mid["seqs"], rng, ln) if ln else b"")
        fill = (-ln) % 16
        reads.append(_cut(mid["seqs"], rng, fill) if fill else b"")
        at += ln + fill
    cat, offs = W.sample_reads(mid["seqs"], 300, 150, seed=200 + phase)
    reads += [bytes(cat[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)]
    _check(index, mid, "phase-%d" % phase, reads, True)


def test_intervals_of_127_128_129_occurrences(workdir):
    """PGX_LCE_MAX_OCC = 128: a forward stage goes through the text while its interval holds at most 128 occurrences.  134 copies of a short base
    (each with its reverse complement); three marked regions are shared by exactly 127, 128 and 129 copies -- the other copies carry a substitution
    in the middle of the region -- so reads cut from them give MEMs of exactly these sizes, and reads that run into a region narrow from 134"""
    rng = np.random.default_rng(41)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    base = acgt[rng.integers(0, 4, 700)].copy()
    n_copies, regions = 134, {127: 130, 128: 330, 129: 530}  # occurrences -> middle of the region
    seqs = []
    for c in range(n_copies):
        s = base.copy()
        for occ, mid_pos in regions.items():
            if c >= occ:  # a copy outside the region's family: one substitution, different from the base
                s[mid_pos] = acgt[(int(np.flatnonzero(acgt == base[mid_pos])[0]) + 1 + (c % 3)) % 4]
        if c == 0:
            s[690:694] = ord("N")  # (a collection without N has five symbols: COMPAT reproduces the reference's mis-parse there and finds nothing)
        seqs.append(s)
    text = os.path.join(workdir, "max_occ.txt")
    with open(text, "wb") as f:
        for s in seqs:
            f.write(s.tobytes() + b"\n")
            f.write(W._COMP[s[::-1]].tobytes() + b"\n")
    ri_path, tags_path = W.build_index_from_text(text, workdir, "max_occ")[:2]
    case = dict(name="max_occ", ri_path=ri_path, tags_path=tags_path, tags_fmt=O.TAGS_COMPACT)
    reads = []
    for occ, mid_pos in regions.items():
        for half in (15, 30, 45):
            reads.append(bytes(base[mid_pos - half:mid_pos + half + 1]))                  # the region alone: a MEM of `occ` occurrences
            reads.append(bytes(W._COMP[base[mid_pos - half:mid_pos + half + 1][::-1]]))  # and its reverse complement
        for a in range(mid_pos - 120, mid_pos + 1, 7):                                     # reads that run into and across the region
            r = bytearray(bytes(base[a:a + 150]))
            reads.append(bytes(r))
            r[int(rng.integers(0, 150))] = ord("A")
            reads.append(bytes(r))
    for s in (seqs[0], seqs[127], seqs[133]):
        reads += [bytes(s[a:a + 150]) for a in range(0, 550, 61)]
    cat, offs = O.pack_reads(reads)
    case["cat"], case["offs"] = cat, offs
    idx = P.Index(ri_path, tags_path, mode=MODE)
    for min_len, min_occ in PAIRS:
        ref = V.oracle(case, min_len, min_occ)
        sizes = set(int(v) for v in ref["mems"]["size"])
        assert {127, 128, 129} <= sizes, sorted(sizes)
        res, t = V.run(idx, cat, offs, min_len, min_occ)
        assert t.kernels & P.KERNELS_PAIRS_LCE, hex(t.kernels)
        V.same(res, ref)
    idx.close()


def test_common_prefixes_at_the_cap_and_unknown(workdir):
    """The table of common prefixes of neighbouring suffixes holds at most 254 (the cap: "254 or more") and 255 for unknown (the comparison met a
    flagged text line).  Four haplotypes identical over thousands of symbols -- one with substitutions every 400, one with a short N run -- put
    253, 254 and 255 next to each other in the table (asserted on the device's table); reads of 260 .. 340 symbols from every region, exact
    and with a substitution, make the forward stages compare across those entries"""
    rng = np.random.default_rng(43)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    base = acgt[rng.integers(0, 4, 3000)].copy()
    haps = [base.copy(), base.copy(), base.copy(), base.copy()]
    for q in range(200, 3000, 400):
        haps[2][q] = acgt[(int(np.flatnonzero(acgt == base[q])[0]) + 1) % 4]
    haps[3][1500:1506] = ord("N")
    text = os.path.join(workdir, "lcp_cap.txt")
    with open(text, "wb") as f:
        for s in haps:
            f.write(s.tobytes() + b"\n")
            f.write(W._COMP[s[::-1]].tobytes() + b"\n")
    ri_path, tags_path = W.build_index_from_text(text, workdir, "lcp_cap")[:2]
    reads = []
    for h in haps:
        for a in range(0, len(h) - 340, 29):
            ln = 260 + (a * 7) % 81
            r = bytearray(bytes(h[a:a + ln]))
            reads.append(bytes(r))
            if a % 3 == 0:
                r[int(rng.integers(0, ln))] = int(acgt[rng.integers(0, 4)])
                reads.append(bytes(r))
            if a % 5 == 0:
                reads.append(bytes(W._COMP[h[a:a + ln][::-1]]))
    cat, offs = O.pack_reads(reads)
    case = dict(name="lcp_cap", ri_path=ri_path, tags_path=tags_path, tags_fmt=O.TAGS_COMPACT, cat=cat, offs=offs)
    idx = P.Index(ri_path, tags_path, mode=MODE)
    n = int(idx.info().bwt_size)
    lcp = idx.lce_view(33, n).astype(np.int64)
    at = np.flatnonzero(lcp == 253)
    assert any({253, 254, 255} <= set(lcp[max(0, i - 2):i + 3].tolist()) for i in at), np.bincount(lcp, minlength=256)[250:]
    for min_len, min_occ in PAIRS:
        ref = V.oracle(case, min_len, min_occ)
        assert int((ref["mems"]["end"] - ref["mems"]["start"]).max()) >= 300
        res, t = V.run(idx, cat, offs, min_len, min_occ)
        assert t.kernels & P.KERNELS_PAIRS_LCE, hex(t.kernels)
        V.same(res, ref)
    idx.close()
