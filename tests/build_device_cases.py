"""Case tables of the device index build (test_build_device_cpu.py on the CPU, test_gpu_build_device.py on the GPU): small text
collections that put a shared prefix on either side of every doubling depth, ties that only endmarkers break, totals on the tile and
digit borders of the new kernels, and groups of thousands of suffixes.  The CPU file asserts with numpy and a naive sorted() over the
suffixes that every table holds the borders it claims; the GPU file compares the device build with the CPU builder on the same texts.

Order rule (include/pgx.h, pgx_build_index_from_text_device): symbols compare by byte value (\\n < A < C < G < N < T), two endmarkers by
sequence number, and the symbol before text position 0 is \\n."""
import numpy as np

SA_K = 10             # PGX_SA_K: symbols of the first key = the depth the doubling starts from (10, 20, 40, ...)
SA_TILE = 2048        # PGX_SA_TILE: symbols / rows per block of the counting passes (classify, keys, heads, ranks, run_heads, runs)
SA_SORT_TILE = 4096   # PGX_SA_SORT_TILE: elements per block of a radix pass (pgx_sa_hist_kernel, pgx_sa_scatter_kernel)
SA_ROW_BLOCK = 256    # rows per block of the thread-per-row passes (gather, bwt); also one round of the scatter kernel
SCAN1_TILE_ITEMS = 4096  # one tile of pgx_scan_onepass_kernel: 4096 histogram entries = 16 sort blocks = 65 536 elements

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rand(rng, n, alphabet=_ACGT, p=None):
    return alphabet[rng.choice(len(alphabet), size=n, p=p)].tobytes() if n else b""


# ---- 2. depth borders: two suffixes that share exactly L symbols
DEPTHS = sorted(set(range(71))
                | {(1 << k) + d for k in range(7, 13) for d in (-1, 0, 1)}
                | {SA_K * (1 << k) + d for k in range(9) for d in (-1, 0, 1)})


def depth_text(L):
    """two to four sequences; the first two are P C and P G for a random P of L symbols: those two suffixes share exactly L symbols and
    nothing sorts between them (a suffix between them would start with P and a symbol, L + 1 symbols before its endmarker; only the
    two whole sequences are that long and start with P)"""
    rng = np.random.default_rng(1000 + L)
    P = _rand(rng, L)
    seqs = [P + b"C", P + b"G"] + [b"T", b"NA"][:L % 3]
    return b"".join(s + b"\n" for s in seqs)


# ---- 3. ties only endmarkers break
def tie_texts():
    t = {}
    for c in (2, 3, 255, 256, 257, 1000):
        t["identical_%d" % c] = b"GATTACA\n" * c
    t["proper_suffix"] = b"ACGTACGTTACA\nTACA\nACA\nCGTACGTTACA\n"
    t["empty_sequences"] = b"\n\n\n"
    t["empty_between"] = b"AC\n\nAC\n\n"
    t["single_sequence"] = b"GATTACAGATTACAGATTA\n"
    t["single_newline"] = b"\n"
    t["no_final_newline"] = b"ACGT\nACG"
    return t


# ---- 4. size and digit borders
def random_collection(n, n_seq, seed, skew=None, n_run=0):
    """n symbols in n_seq newline-terminated sequences over ACGT (probabilities skew), with one run of n_run N"""
    rng = np.random.default_rng(seed)
    body = n - n_seq
    assert body >= 0 and n_seq >= 1
    cuts = np.sort(rng.integers(0, body + 1, size=n_seq - 1)) if n_seq > 1 else np.zeros(0, dtype=np.int64)
    lens = np.diff(np.concatenate(([0], cuts, [body])))
    sym = np.frombuffer(_rand(rng, body, p=skew), dtype=np.uint8).copy()
    if n_run and body > n_run:
        st = int(rng.integers(0, body - n_run))
        sym[st:st + n_run] = ord("N")
    out, at = [], 0
    for ln in lens:
        out.append(sym[at:at + int(ln)].tobytes() + b"\n")
        at += int(ln)
    t = b"".join(out)
    assert len(t) == n
    return t


# name -> (total symbols, sequences, what lies there)
SIZE_CASES = {}
for _n in (255, 256, 257):
    SIZE_CASES["n_%d" % _n] = (_n, 3, "SA_ROW_BLOCK: one block / one round of the row passes and of the scatter")
for _n in (2047, 2048, 2049):
    SIZE_CASES["n_%d" % _n] = (_n, 4, "SA_TILE: one tile of the counting passes")
for _n in (4095, 4096, 4097):
    SIZE_CASES["n_%d" % _n] = (_n, 5, "SA_SORT_TILE: one block of a radix pass; two tiles of the counting passes")
for _n in (8191, 8192, 8193):
    SIZE_CASES["n_%d" % _n] = (_n, 2, "two radix blocks: the digit-major histogram table has two columns")
for _n in (65535, 65536, 65537):
    SIZE_CASES["n_%d" % _n] = (_n, 7, "ranks cross 16 bits (a third radix digit); the histogram table crosses one SCAN1_TILE_ITEMS tile of the scan")
MANY_SEQ = (3 * (1 << 16) + 1, 65537)  # total, one-symbol sequences: endmarker numbers cross 16 bits, ranks two radix digits


def size_text(name):
    n, n_seq, _ = SIZE_CASES[name]
    return random_collection(n, n_seq, seed=n, n_run=min(40, n // 8))


def many_sequences_text():
    n, ones = MANY_SEQ
    rng = np.random.default_rng(77)
    short = np.empty((ones, 2), dtype=np.uint8)
    short[:, 0] = _ACGT[rng.integers(0, 4, size=ones)]
    short[:, 1] = 10
    rest = n - 2 * ones
    t = short.tobytes() + _rand(rng, rest - 1) + b"\n"
    assert len(t) == n
    return t


# ---- 5. large groups
def large_groups_text():
    """a poly-A run of 5000, an N run of 3000 and the tandem repeat (ACG)^2000 inside one collection of 20 000 symbols"""
    rng = np.random.default_rng(5)
    parts = [_rand(rng, 1500), b"A" * 5000, _rand(rng, 700), b"\n", _rand(rng, 900), b"N" * 3000, _rand(rng, 400), b"\n", _rand(rng, 1000), b"ACG" * 2000,
             _rand(rng, 1497), b"\n"]
    t = b"".join(parts)
    assert len(t) == 20000
    return t


# ---- 9. randomised sweep
def sweep_text(seed):
    rng = np.random.default_rng(seed)
    n_seq = int(rng.integers(1, 41))
    n = int(rng.integers(max(2, n_seq), 5001))
    w = rng.random(4) ** 3 + 1e-3  # symbol skew: from even to one symbol nearly alone
    return random_collection(n, n_seq, seed=seed + 1, skew=w / w.sum(), n_run=int(rng.integers(0, 30)))


# ---- the order rule, naively
def naive_suffix_order(text):
    """suffix positions of a newline-terminated collection in the order rule above, by sorted() over the suffixes: every symbol becomes
    three big-endian bytes -- endmarker q the number q, a symbol n_seq + its byte -- so that byte order is the order rule"""
    t = np.frombuffer(text, dtype=np.uint8)
    assert len(t) and t[-1] == 10
    nl = t == 10
    n_seq = int(nl.sum())
    v = np.where(nl, np.cumsum(nl) - 1, n_seq + t.astype(np.int64))
    enc = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=1).astype(np.uint8).tobytes()
    order = sorted(range(len(t)), key=lambda i: enc[3 * i:])
    return np.array(order, dtype=np.int64), enc


def neighbour_lcps(text):
    """common prefix (symbols) of every pair of neighbouring suffixes in that order; endmarkers are distinct symbols"""
    order, enc = naive_suffix_order(text)
    n = len(text)
    a = np.frombuffer(enc, dtype=np.uint8).reshape(n, 3)
    sym = (a[:, 0].astype(np.int64) << 16) | (a[:, 1].astype(np.int64) << 8) | a[:, 2]
    out = []
    for x, y in zip(order[:-1], order[1:]):
        m = min(n - x, n - y)
        d = np.flatnonzero(sym[x:x + m] != sym[y:y + m])
        out.append(int(d[0]) if len(d) else m)
    return out


def naive_bwt_runs(text):
    """(symbol, length) runs of the BWT in that order, as the .rl_bwt file holds them: maximal runs, endmarkers not split"""
    order, _ = naive_suffix_order(text)
    t = np.frombuffer(text, dtype=np.uint8)
    bwt = np.where(order == 0, 10, t[order - 1])
    cut = np.flatnonzero(np.diff(bwt)) + 1
    starts = np.concatenate(([0], cut))
    lens = np.diff(np.concatenate((starts, [len(bwt)])))
    return [(int(bwt[s]), int(l)) for s, l in zip(starts, lens)]


def rlbwt_bytes(runs):
    """the grlBWT file of those runs (u64 1, u64 bytes a length, then symbol + length records), as pgx_build_rlbwt writes it"""
    longest = max(l for _, l in runs)
    bl = 1
    while bl < 8 and (longest >> (8 * bl)):
        bl += 1
    out = bytearray((1).to_bytes(8, "little") + bl.to_bytes(8, "little"))
    for s, l in runs:
        out.append(s)
        out += l.to_bytes(bl, "little")
    return bytes(out)
