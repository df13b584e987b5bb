"""Shared pieces of the border tests (test_border_cases.py on the CPU; test_gpu_tag_borders.py, test_gpu_spec_borders.py,
test_gpu_locate_borders.py, test_gpu_mem_locate_borders.py and test_gpu_heavy_limits.py on the GPU): case tables that put a query, a
range, a MEM or a read exactly on a device capacity, and the oracle's answers (computed once per table).  The CPU file asserts with the
oracle and numpy alone that every table hits what it claims; the GPU files compare the device with the same answers."""
import os

import numpy as np

import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W

TAG_SMALL = 16           # PGX_TAG_SMALL: up to here the 16-lane kernel (pgx_tag_small_kernel)
SORT_WAVE_REGS = 64      # the `cnt <= 64` branch of pgx_tag_sort_unique_kernel: bitonic network in registers
SORT_LDS_CAP = 2048      # PGX_SORT_LDS_CAP: per-wave LDS slice; beyond it the large list
SORT_WG_LDS_CAP = 16384  # PGX_SORT_WG_LDS_CAP: dynamic LDS of pgx_tag_sort_large_kernel; beyond it global scratch
SCAN1_TILE_ITEMS = 4096  # PGX_SCAN1_TILE_ITEMS: one tile of pgx_scan_onepass_kernel
TAG_STARTS_STEP = 10     # the sampling of the run starts: a query whose first run f has f % 10 == 0 reads item f, not f - 1 (quirk 7)
FM_HEAVY_CAP = 8192      # PGX_FM_HEAVY_CAP: heavy reads per launch
FM_HEAVY_MAXLEN = 4096   # PGX_FM_HEAVY_MAXLEN: longer reads are never handed on

_CACHE = {}


def size_class(c):
    """which kernel path answers a query of c runs / sorts a range of c values"""
    if c <= 1:
        return "none" if c == 0 else "single"
    if c <= TAG_SMALL:
        return "small"
    if c <= SORT_WAVE_REGS:
        return "wave_regs"
    if c <= SORT_LDS_CAP:
        return "wave_lds"
    if c <= SORT_WG_LDS_CAP:
        return "wg_lds"
    return "wg_scratch"


def pad2(c):
    """the power of two the bitonic sorts pad c values to"""
    p = 64
    while p < c:
        p <<= 1
    return p


# ---- 1. the tag stage through pgx_tag_query_batch ---------------------------------------------------------------------------------------
N_TAG_RUNS = 70_000
TAG_PATTERNS = ("random", "equal", "distinct")
BORDER_C = (1, 2, 15, 16, 17, 63, 64, 65, 1024, 1025, 2047, 2048, 2049, 8192, 8193, 16383, 16384, 16385, 32768, 32769)
BORDER_F_MOD = (0, 1, 7)  # f mod 10 of the three first runs of every c


class TagArray:
    """a compact tag array of N_TAG_RUNS runs of 1..3 positions (the same lengths for every value pattern); run r (0-based) starts at
    starts[r], and a query [starts[f - 1], starts[f + c - 2]] has first run f = rank_1(start + 1) and exactly c runs"""

    def __init__(self, workdir, pattern):
        rng = np.random.default_rng(21)
        n = N_TAG_RUNS
        self.lens = rng.integers(1, 4, n).astype(np.uint64)
        if pattern == "random":  # 2999 different values: a few duplicates in 64 values, mostly duplicates in 8192
            self.vals = rng.integers(1, 3000, n).astype(np.uint64) << np.uint64(11)
        elif pattern == "equal":
            self.vals = np.full(n, (77 << 11) | 5, dtype=np.uint64)
        else:
            self.vals = ((rng.permutation(n).astype(np.uint64) + np.uint64(1)) << np.uint64(11)) | (np.arange(n, dtype=np.uint64) % np.uint64(1024))
        self.starts = np.concatenate([[0], np.cumsum(self.lens)[:-1]]).astype(np.uint64)
        self.total = int(self.lens.sum())
        self.pattern = pattern
        self.path = os.path.join(workdir, "border_%s.tags" % pattern)
        P.write_compact_tags(self.path, self.vals, self.lens)
        self._oracle = None
        self._answers = {}

    def oracle(self):
        if self._oracle is None:
            self._oracle = O.Tags(self.path, O.TAGS_COMPACT)
        return self._oracle

    def query(self, f, c):
        """(start, end) of the query of c >= 1 runs whose first run is f (1-based: the f-th run)"""
        return int(self.starts[f - 1]), int(self.starts[f + c - 2])

    def queries(self, fc):
        se = [self.query(f, c) for f, c in fc]
        return np.array([s for s, _ in se], dtype=np.uint64), np.array([e for _, e in se], dtype=np.uint64)

    def expected(self, f, c):
        """numpy's answer: (sorted unique values of the c items read, whether an item beyond the stored ones is read (as 0))"""
        fi = f if f % TAG_STARTS_STEP == 0 else f - 1
        v = self.vals[fi:fi + c]
        over = fi + c > N_TAG_RUNS
        if over:
            v = np.concatenate([v, np.zeros(c - len(v), dtype=np.uint64)])
        return np.unique(v), over

    def answers(self, key, st, en):
        """the oracle's answers for a batch, once per key: run counts, position offsets, positions, overflow flags"""
        if key not in self._answers:
            t = self.oracle()
            rn = np.zeros(len(st), dtype=np.uint64)
            over = np.zeros(len(st), dtype=bool)
            pos = []
            for i in range(len(st)):
                r, p, o = t.query(int(st[i]), int(en[i]))
                rn[i], over[i] = r, o
                pos.append(np.array(p, dtype=np.uint64))
            po = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.uint64)
            self._answers[key] = (rn, po, np.concatenate(pos) if pos else np.zeros(0, np.uint64), over)
        return self._answers[key]


def tag_array(workdir, pattern):
    k = ("tags", pattern)
    if k not in _CACHE:
        _CACHE[k] = TagArray(workdir, pattern)
    return _CACHE[k]


def border_first_runs(c):
    """three first runs for a query of c runs, f mod 10 = BORDER_F_MOD, far enough from the end that no item beyond the array is read"""
    rng = np.random.default_rng(1000 + c)
    tens = rng.choice(np.arange(1, (N_TAG_RUNS - c - 20) // 10), 3, replace=False)
    return [int(10 * t + m) for t, m in zip(tens, BORDER_F_MOD)]


def border_queries(c):
    return [(f, c) for f in border_first_runs(c)]


# the overflow sites of the device: (first run, number of copies); every query ends in the last run, c = N_TAG_RUNS - f + 1
OVERFLOW_SITES = {
    "single": [(70000, 1)],      # c = 1: the single-run branch of pgx_tag_locate_kernel
    "small": [(69990, 1)],       # c = 11: pgx_tag_small_kernel
    "big": [(69900, 1)],         # c = 101: pgx_tag_gather_kernel over the big list
    "large": [(65000, 1)],       # c = 5001: pgx_tag_gather_kernel over the representatives of the large list
    "large_scratch": [(50000, 1)],  # c = 20001: the same, sorted in global scratch
    "large_dups": [(65000, 3)],  # one representative and two copies through pgx_tag_copy_dups_kernel
}
# beside them in every sub-batch: queries of every class that do not overflow -- f = 69991 ends in the last run as well (c = 10, f % 10 = 1),
# and an identical pair of large queries goes through pgx_tag_copy_dups_kernel without overflowing
OVERFLOW_CONTROLS = [(69991, 10), (69999, 1), (40, 1), (120, 11), (2050, 101), (30000, 5001), (30000, 5001), (20000, 20001), (69001, 1000)]


def overflow_batch(sites):
    """(f, c) of the sub-batch of the named sites: their queries between the controls"""
    fc = list(OVERFLOW_CONTROLS[:4])
    for name in sites:
        for f, copies in OVERFLOW_SITES[name]:
            fc += [(f, N_TAG_RUNS - f + 1)] * copies
    return fc + list(OVERFLOW_CONTROLS[4:])


INVERTED_RUNS = (5, 9, 12345, 39999)  # 0-based runs a: the query [starts[a], starts[a] - 1] has 0 runs (f = a + 1; f % 10 == 0 for two of them)


def inverted_queries(arr):
    st = arr.starts[list(INVERTED_RUNS)]
    return st, st - np.uint64(1)


QUERY_COUNTS = (4095, 4096, 4097, 8192, 8193)


def count_queries():
    """8193 (f, c) of mixed classes; the batches are its prefixes of QUERY_COUNTS queries.  The queries around every prefix end are not single
    runs, so that the last items of both scans (run counts of the segments, unique counts) are not zero"""
    rng = np.random.default_rng(77)
    n = max(QUERY_COUNTS)
    c = np.ones(n, dtype=np.int64)
    kind = rng.random(n)
    c[kind > 0.5] = rng.integers(2, TAG_SMALL + 1, int((kind > 0.5).sum()))
    c[kind > 0.9] = rng.integers(TAG_SMALL + 1, 300, int((kind > 0.9).sum()))
    for i, v in ((100, 3000), (4000, 2049), (5000, 20000), (8000, 2048)):
        c[i] = v
    for m in QUERY_COUNTS:
        c[m - 2:m] = (5, 40) if m % 2 else (40, 5)
    f = rng.integers(1, N_TAG_RUNS - 20100, n)
    return [(int(a), int(b)) for a, b in zip(f, c)]


# ---- 3. the shared sort behind pgx_locate_batch --------------------------------------------------------------------------------------------
LOCATE_C = (1, 2, 63, 64, 65, 2047, 2048, 2049, 16383, 16384, 16385, 32769)


def locate_case(workdir):
    """a synthetic pangenome of 4 haplotypes in both strands (8 sequences, n ~ 160 k), opened STRICT: any range of more than 8 positions holds a
    sequence twice.  -> dict(ri_path, sa, max_length, first, last) with three ranges of exactly c positions for every c of LOCATE_C; for
    c >= 2 the first of them holds a duplicate sequence id"""
    if "locate" not in _CACHE:
        text = os.path.join(workdir, "border_loc.txt")
        W.synth_pangenome_text(text, base_len=20000, n_hap=4, seed=78)
        ri_path = W.build_index_from_text(text, workdir, "border_loc", encoded=True, with_tags=False)[0]
        r = O.RIndex(ri_path)
        sa = r.decompress_sa()
        ids = sa // np.uint64(r.max_length)
        n = int(r.n)
        rng = np.random.default_rng(5)
        first = []
        for c in LOCATE_C:
            a = [int(x) for x in rng.integers(0, n - c, 3)]
            if c == 2:
                a[0] = int(np.flatnonzero(ids[:-1] == ids[1:])[7])
            a[2] = n - c if c in (1, 32769) else a[2]  # a range that ends with the BWT
            first += a
        first = np.array(first, dtype=np.uint64)
        last = first + np.repeat(np.array(LOCATE_C, dtype=np.uint64), 3) - np.uint64(1)
        _CACHE["locate"] = dict(ri_path=ri_path, sa=sa, max_length=int(r.max_length), n=n, first=first, last=last)
    return _CACHE["locate"]


def locate_expected(case, flags):
    """numpy on the oracle's suffix array -> (offsets, values)"""
    ml = np.uint64(case["max_length"])
    out = []
    for a, b in zip(case["first"], case["last"]):
        e = case["sa"][int(a):int(b) + 1]
        if flags & P.LOCATE_SEQ_IDS:
            e = e // ml
        if flags & P.LOCATE_UNIQUE:
            e = np.unique(e)
        out.append(e)
    return np.concatenate([[0], np.cumsum([len(e) for e in out])]).astype(np.uint64), np.concatenate(out)


# ---- 4. heavy reads at their two limits ------------------------------------------------------------------------------------------------
HEAVY_EXT = 24  # PGX_FM_HEAVY_EXT of these tests: practically every read is handed on after its first start positions
HEAVY_CAP_READS = 9000
HEAVY_LENGTHS = (1000, 4095, 4096, 4097)


def heavy_cap_reads(mid):
    """9 000 reads of 150 symbols sampled from the mid-size index's text with 5 % substitutions (a read without any is one MEM and never reaches
    a second start position): more than FM_HEAVY_CAP of them are offered to the heavy-read kernel"""
    return W.sample_reads(mid["seqs"], HEAVY_CAP_READS, 150, seed=23, sub_rate=0.05)


def heavy_long_reads(mid, lengths=HEAVY_LENGTHS):
    """reads of the given lengths cut from the text (no N) with a substitution about every 100 symbols -- MEMs of ~100 symbols bound the work of
    the every-start evaluation -- behind 200 ordinary reads"""
    rng = np.random.default_rng(29)
    comp = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}
    reads = []
    for k, ln in enumerate(lengths):
        s = mid["seqs"][2 * k]
        a = 3000
        while np.any(s[a:a + ln] == ord("N")):
            a += 5000
        r = bytearray(bytes(s[a:a + ln]))
        at = int(rng.integers(40, 100))
        while at < ln:
            r[at] = comp[r[at]]
            at += int(rng.integers(80, 120))
        reads.append(bytes(r))
    cat, offs = W.sample_reads(mid["seqs"], 200, 150, seed=24)
    ecat, eoffs = O.pack_reads(reads)
    return np.concatenate([cat, ecat]), np.concatenate([offs, eoffs[1:] + offs[-1]])


# ---- 2. the tag stage through pgx_batch_run: non-zero overflow, one capacity at a time ------------------------------------------------------------
SPEC_MIN_LEN, SPEC_MIN_OCC = 20, 1
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def with_slack(v):
    """the capacity a speculative run takes from the previous run's count (pgx_runtime_internal.hpp)"""
    return v + v // 4 + 64


def largest_capacity(last_largest):
    """the run count the dynamic LDS of pgx_tag_sort_large_kernel is sized for: the power of two >= 2 x the last largest one, at least 64, at
    most SORT_WG_LDS_CAP"""
    p2 = 64
    while p2 < 2 * last_largest and p2 < SORT_WG_LDS_CAP:
        p2 <<= 1
    return p2


# demand() / capacities() restate the host's sizing rule (tag_pipeline in pgx_runtime_internal.hpp: with_slack of the last G, list lengths and P,
# the power of two for the largest run count; run_pass in pgx_batch.hip: with_slack of the last MEM total) -- a change there has to be made here too
def demand(ref):
    """what a run asks of each capacity, from the oracle's answer: MEM total, gathered values G (single runs have no segment), the lengths of the
    small / big / large lists, the largest run count on the large list, positions P"""
    rc = ref["tag_run_counts"].astype(np.int64)
    large = rc[rc > SORT_LDS_CAP]
    return dict(mems=len(rc), G=int(rc[rc > 1].sum()), small=int(((rc >= 2) & (rc <= TAG_SMALL)).sum()),
                big=int(((rc > TAG_SMALL) & (rc <= SORT_LDS_CAP)).sum()), large=len(large), largest=int(large.max()) if len(large) else 0,
                P=len(ref["positions"]))


def capacities(ref):
    d = demand(ref)
    return {k: (largest_capacity(v) if k == "largest" else with_slack(v)) for k, v in d.items()}


def exceeded(ref_a, ref_b):
    """the capacities, taken from a run of A, that a run of B exceeds"""
    cap, d = capacities(ref_a), demand(ref_b)
    return {k for k in cap if d[k] > cap[k]}


def _per_position_values(n_runs):
    return (np.arange(n_runs, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(3000) + np.uint64(1)) << np.uint64(11)


class SpecCase:
    """a pangenome of 4 haplotypes in both strands with N runs of 700 .. 1000 symbols, 40 copies of a 60-symbol region (a MEM of 17 .. 2048
    occurrences) and 12 private contigs of 200 symbols (a read that ends one has 131 MEMs of one occurrence each), n ~ 0.49 M, and tag arrays with
    one run per BWT position: the run count of a MEM's query is the size of its interval, a read of k N has one MEM of thousands of runs"""

    def __init__(self, workdir):
        self.workdir = workdir
        text = os.path.join(workdir, "border_spec.txt")
        W.synth_pangenome_text(text, base_len=60000, n_hap=4, seed=41, n_runs=3, n_run_len=(700, 1000))
        haps = W.load_sequences(text)
        rng = np.random.default_rng(3)
        self.repeat = bytes(haps[0][1000:1060])
        assert b"N" not in self.repeat
        self.private = [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 200)]) for _ in range(12)]
        with open(text, "ab") as f:
            for s in [self.repeat] * 40 + self.private:
                f.write(s + b"\n" + s.translate(_COMP)[::-1] + b"\n")
        self.ri_path = W.build_index_from_text(text, workdir, "border_spec", with_tags=False)[0]
        self.ri = O.RIndex(self.ri_path)
        self.n = int(self.ri.n)
        self.haps = haps
        self.full_tags = self.write_tags("full", self.n, 0)
        self._tags = {}
        self._ref = {}
        cat, offs = W.sample_reads(haps, 6000, 150, seed=3, n_frac=0.0)
        self.sampled = [bytes(cat[int(offs[i]):int(offs[i + 1])]) for i in range(6000)]

    def write_tags(self, name, T, d):
        """one run per BWT position over [0, T), the first run lengthened by d: n_runs = T - d, and position p >= d is in run p + 1 - d"""
        path = os.path.join(self.workdir, "border_spec_%s.tags" % name)
        lens = np.ones(T - d, dtype=np.uint64)
        lens[0] += np.uint64(d)
        P.write_compact_tags(path, _per_position_values(T - d), lens)
        return path

    def n_read_mem(self, k):
        """the one MEM of a read of k N: (bwt_start, size)"""
        mems = self.ri.find_all_mems(b"N" * k, SPEC_MIN_LEN, SPEC_MIN_OCC)
        assert len(mems) == 1 and mems[0][:2] == (0, k)
        return mems[0][2], mems[0][3]

    def n_read_with_size(self, lo, hi, longest=False):
        """the shortest (or longest) read of N whose MEM has lo < size <= hi; the size falls as the read grows"""
        for k in (range(699, SPEC_MIN_LEN - 1, -1) if longest else range(SPEC_MIN_LEN, 700)):
            if lo < self.n_read_mem(k)[1] <= hi:
                return b"N" * k
        raise ValueError("no read of N with a MEM of %d < size <= %d" % (lo, hi))

    def private_tails(self):
        return [s[-150:] for s in self.private] + [s.translate(_COMP)[::-1][-150:] for s in self.private]

    def ref(self, key, tags_path, reads):
        """the oracle's answer for a list of reads on a tag array, once per key -> (cat, offs, answer)"""
        if key not in self._ref:
            if tags_path not in self._tags:
                self._tags[tags_path] = O.Tags(tags_path, O.TAGS_COMPACT)
            cat, offs = O.pack_reads(reads)
            self._ref[key] = (cat, offs, O.find_mems_batch(self.ri, self._tags[tags_path], cat, offs, SPEC_MIN_LEN, SPEC_MIN_OCC,
                                                           threads=O.lib().orc_max_threads()))
        return self._ref[key]

    def mem_overflows(self, tags_path, ref):
        """per MEM of an answer: does its query read beyond the stored runs (the oracle's flag, query by query)"""
        t = self._tags[tags_path]
        memo = {}
        out = np.zeros(len(ref["mems"]), dtype=bool)
        for i, m in enumerate(ref["mems"]):
            k = (int(m["bwt_start"]), int(m["size"]))
            if k not in memo:
                memo[k] = t.query(k[0], k[0] + k[1] - 1)[2]
            out[i] = memo[k]
        return out


def spec_case(workdir):
    if "spec" not in _CACHE:
        _CACHE["spec"] = SpecCase(workdir)
    return _CACHE["spec"]


OVERFLOW_FILES = ("single", "small", "big", "large", "large_dups")


def overflow_file(case, site):
    """-> (key, tags_path, reads): a tag array cut short at T so that the MEMs of one device site read beyond it, and the reads of the batch.
    A MEM [bwt_start, bwt_start + size) with T = bwt_start + size ends in the last run; with the first run lengthened by
    d = (bwt_start + 1) % 10 its first run is f = bwt_start + 1 - d, f % 10 == 0, and it reads items f .. f + size - 1 = n_runs: one too many.
    MEMs at or beyond T have one run, the last one, and read item n_runs only where n_runs % 10 == 0."""
    reads = list(case.sampled[:3000])
    if site == "single":  # T below the N block and the repeat's MEM, n_runs % 10 == 0: every MEM beyond T overflows
        ref = case.ref("spec_sampled", case.full_tags, reads)[2]
        st, en = ref["mems"]["bwt_start"].astype(np.int64), ref["mems"]["bwt_start"].astype(np.int64) + ref["mems"]["size"] - 1
        T = 200000
        while np.any((st < T) & (en >= T)):  # no MEM straddles T
            T += 10
        d = 0
        reads += [b"N" * 40, b"N" * 300, case.repeat]
    else:
        if site == "small":
            ref = case.ref("spec_sampled", case.full_tags, reads)[2]
            pick = np.flatnonzero((ref["mems"]["size"] >= 3) & (ref["mems"]["size"] <= TAG_SMALL) & (ref["mems"]["bwt_start"] > 100000))[0]
            bs, size = int(ref["mems"]["bwt_start"][pick]), int(ref["mems"]["size"][pick])
            reads += [b"N" * 40, case.repeat]
        elif site == "big":
            mems = case.ri.find_all_mems(case.repeat, SPEC_MIN_LEN, SPEC_MIN_OCC)
            bs, size = mems[0][2], mems[0][3]
            reads += [b"N" * 40, case.repeat]
        else:
            n_read = case.n_read_with_size(SORT_LDS_CAP, 4096)
            bs, size = case.n_read_mem(len(n_read))
            reads += [n_read] * (3 if site == "large_dups" else 1) + [case.repeat]
        T, d = bs + size, (bs + 1) % 10
    return "over_" + site, case.write_tags("over_" + site, T, d), reads


def junk_reads(n, seed=5):
    """random reads: hardly any MEM of 20 symbols"""
    rng = np.random.default_rng(seed)
    return [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 150)]) for _ in range(n)]


def capacity_batches(case):
    """batch A and the batches B (the same number of reads) that exceed capacities taken from a run of A; every batch on the full tag array.
    -> dict name -> reads.  A: 6000 sampled reads, a read of N with a MEM of 2048 < size <= 4096 runs, the repeat."""
    base = case.sampled
    n_a = case.n_read_with_size(SORT_LDS_CAP, 4096)
    n_b = case.n_read_with_size(8192, SORT_WG_LDS_CAP, longest=True)
    tails = case.private_tails()
    hap_tails = [bytes(s[-150:]) for s in case.haps]
    out = {"A": base + [n_a, case.repeat]}
    out["largest"] = base + [n_b, case.repeat]                    # the read of N shorter: a MEM of 8192 < size <= 16384 runs, just above 8192
    out["mems"] = base[:-len(tails)] + tails + [n_a, case.repeat]  # 24 reads of 131 one-run MEMs each: no segment, one position each
    out["small"] = base[:-22] + (hap_tails * 3)[:22] + [n_a, case.repeat]  # 22 reads of 131 MEMs of 3 .. 4 runs: the small list alone
    out["big"] = base[:-3] + [case.repeat] * 3 + [n_a, case.repeat]  # 41 MEMs of 43 runs a read
    out["large"] = base[:-80] + [b"N" * k for k in range(len(n_a), len(n_a) + 80)] + [n_a, case.repeat]  # 80 more MEMs on the large list: G and P too
    return out


# what each B exceeds of the capacities taken from a run of A (asserted from the oracle's answers on the CPU and again before the GPU run)
CAPACITY_EXCEEDED = {"largest": {"largest"}, "mems": {"mems"}, "small": {"small"}, "big": {"big"}, "large": {"large", "G", "P"}}


# the abort flags the device raises in the speculative run of each B (PGX_DEBUG_COUNTERS prints them): pgx_spec_check_kernel's bit 0 = gathered
# values (and, in its later launches, the small list and the positions), 1 = large list, 2 = largest run count, 3 = big list; 16 =
# pgx_compact_mems_kernel's MEM total, behind which the tag stage's kernels return at once (its checks then see counts of no meaning)
CAPACITY_ABORT_FLAGS = {"largest": 4, "mems": 16, "small": 1, "big": 8, "large": 3}


def over_16384_reads(case):
    return case.sampled[:3000] + [case.n_read_with_size(SORT_WG_LDS_CAP, 1 << 40), case.repeat]


# ---- 3b. the shared sort behind pgx_batch_locate ---------------------------------------------------------------------------------------------
MEM_LOCATE_OCC = {2047: 5, 2048: 14, 2049: 23, 16384: 32, 16385: 41}  # occurrences -> middle of the marked region (regions of 9 symbols, disjoint)
MEM_LOCATE_COPIES = 16400
MEM_LOCATE_MIN_LEN = 8


def mem_locate_case(workdir):
    """16 400 copies of a 48-symbol base, each with its reverse complement (n ~ 1.6 M); five marked regions are shared by exactly 2047, 2048,
    2049, 16384 and 16385 copies -- every other copy carries a substitution in the middle of the region -- so a read cut from a region has one MEM
    of exactly that many occurrences.  -> dict(ri_path, cat, offs, ref (the oracle's MEMs), sa, max_length)"""
    if "mem_locate" not in _CACHE:
        rng = np.random.default_rng(47)
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        base = acgt[rng.integers(0, 4, 48)].copy()
        lines = []
        for c in range(MEM_LOCATE_COPIES):
            s = base.copy()
            for occ, m in MEM_LOCATE_OCC.items():
                if c >= occ:
                    s[m] = acgt[(int(np.flatnonzero(acgt == base[m])[0]) + 1 + (c % 3)) % 4]
            if c == 0:
                s[47] = ord("N")  # (a collection without N has five symbols: COMPAT mis-parses it as the reference does)
            b = s.tobytes()
            lines.append(b)
            lines.append(b.translate(_COMP)[::-1])
        text = os.path.join(workdir, "border_mloc.txt")
        with open(text, "wb") as f:
            f.write(b"\n".join(lines) + b"\n")
        ri_path = W.build_index_from_text(text, workdir, "border_mloc", with_tags=False)[0]
        ri = O.RIndex(ri_path)
        reads = []
        for occ, m in MEM_LOCATE_OCC.items():
            r = base[m - 4:m + 5].tobytes()
            reads += [r, r.translate(_COMP)[::-1]]
        reads += [base.tobytes(), lines[2 * 3000], lines[2 * 16390 + 1], base[:30].tobytes(), base[20:].tobytes()]
        cat, offs = O.pack_reads(reads)
        ref = O.find_mems_batch(ri, None, cat, offs, MEM_LOCATE_MIN_LEN, 1, threads=O.lib().orc_max_threads())
        _CACHE["mem_locate"] = dict(ri_path=ri_path, cat=cat, offs=offs, ref=ref, sa=ri.decompress_sa(), max_length=int(ri.max_length), n=int(ri.n))
    return _CACHE["mem_locate"]


def mem_locate_expected(case, flags):
    """numpy on the oracle's suffix array, MEM by MEM of the oracle's answer -> (offsets, values)"""
    ml = np.uint64(case["max_length"])
    out = []
    for m in case["ref"]["mems"]:
        e = case["sa"][int(m["bwt_start"]):int(m["bwt_start"]) + int(m["size"])]
        if flags & P.LOCATE_SEQ_IDS:
            e = e // ml
        if flags & P.LOCATE_UNIQUE:
            e = np.unique(e)
        out.append(e)
    return np.concatenate([[0], np.cumsum([len(e) for e in out])]).astype(np.uint64), np.concatenate(out)
