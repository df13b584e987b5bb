"""Full-size parity of the sigma = 6 synthetic pangenome workload inside the -m gpu tier: SURVEY 8d
config-3 recipe at 1/10 scale (4 Mbp x 8 haplotypes x 2 strands, n = 64 M, r = 6.3 M), 1 M synthetic 150-bp reads,
min_len 20 -- about 1.9 M MEMs, 23 M positions, 196 M extensions -- every MEM, run count and position against the CPU
oracle, under every layout of the device rank image.  (The same check at chr22 scale, n = 640 M, is
scripts/parity_full_synth.py; its output is committed under profiles/.)

Batches at the size the bench measures (10 M reads and more) are checked over their whole length, not only their first reads: a sample
of reads from the whole batch -- every 61st read, the last 20 000, every read with a byte outside A C G T, 2 000 drawn at random past the
prefix -- against the oracle (tests/batch_sample.py), and the whole arrays against other product runs of the same reads (speculative
re-runs, several chunks, the packed upload)."""
import os
import types

import numpy as np
import pytest

import batch_sample as S
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W

pytestmark = pytest.mark.gpu

FLAGS = P.RUN_TAGS | P.RUN_TIMING  # what bench.py runs
SORT_WG_LDS_CAP = 16384  # PGX_SORT_WG_LDS_CAP (csrc/pgx_device.h): a speculative tag stage sorts every query's runs in one workgroup's LDS


def _oracle(ri, tags, cat, offs):
    return O.find_mems_batch(ri, tags, cat, offs, 20, 1, threads=O.lib().orc_max_threads())


def _sample(cat, offs, seed, random_from, extra=()):
    """the read ids a full-size batch is checked on (every 61st, the last 20 000, 2 000 at random from [random_from, n), every read with a
    byte outside A C G T, `extra`) -> (ids, the non-A C G T reads)"""
    side = S.non_acgt_reads(cat, offs)
    return S.sample_ids(offs, seed, random_from=random_from, extra=np.concatenate([side, np.asarray(extra, dtype=np.int64)])), side


def _speculative_reruns(b, first, what, require_spec=False):
    """the bench's timed steps: the same batch again, sized from the run before (no mid-run read-back); every array and the totals byte
    for byte equal to the exact first run, over the whole batch.  A one-chunk batch re-runs speculatively unless one of its tag queries
    spans more than SORT_WG_LDS_CAP runs (pgx_batch_run: the speculative tag stage has no global-memory sort); then the re-runs are exact
    ones sized from the run before, and are compared all the same.  require_spec: the batch must qualify (the bench's default workload)."""
    largest = int(first["tag_run_counts"].max()) if len(first["tag_run_counts"]) else 0
    spec = largest <= SORT_WG_LDS_CAP
    assert spec or not require_spec, "%s: a tag query of %d runs: the re-runs cannot be speculative" % (what, largest)
    print("\n[fullsize] %s: largest tag query %d runs: re-runs %s" % (what, largest, "speculative" if spec else "exact (beyond the LDS sort)"))
    assert b.spec_stats() == (0, 0)  # the first run of the batch was exact
    for k in (1, 2):
        b.run(20, 1, FLAGS)
        assert b.spec_stats() == ((k, 0) if spec else (0, 0)), "%s: run %d, largest tag query %d runs: %s" % (what, k + 1, largest, b.spec_stats())
        assert b.timing().find_mems_launches == 1
        S.compare(b.result(), first, totals=True, what="%s, re-run %d against the first run" % (what, k + 1))


def test_synth_pangenome_one_million_reads(workdir):
    text = os.path.join(workdir, "full_synth.txt")
    W.synth_pangenome_text(text, base_len=4_000_000)
    ri_path, tags_path = W.build_index_from_text(text, workdir, "full_synth")[:2]
    seqs = W.load_sequences(text)
    cat, offs = W.sample_reads(seqs, 1_000_000, 150, seed=42 + 3)
    ri, tags = O.RIndex(ri_path), O.Tags(tags_path, O.TAGS_COMPACT)
    assert ri.sigma == 6 and ri.n > 60_000_000
    ref = O.find_mems_batch(ri, tags, cat, offs, 20, 1, threads=O.lib().orc_max_threads())
    assert len(ref["mems"]) > 1_500_000 and len(ref["positions"]) > 10_000_000 and ref["n_extensions"] > 150_000_000
    # the automatic layout (64-byte dense blocks + the two-step pairs image + seed table), dense2 + pairs (the automatic layout of longer BWTs),
    # the 64-byte blocks alone, dense2 alone, run-length blocks
    for force in (0, P.MODE_IMAGE_PAIRS, P.MODE_IMAGE_DENSE, P.MODE_IMAGE_DENSE2, P.MODE_IMAGE_RL):
        idx = P.Index(ri_path, tags_path, mode=P.MODE_COMPAT | force)
        assert force or idx.info().image_kind == P.IMAGE_DENSE
        assert idx.info().image_pairs == (1 if force in (0, P.MODE_IMAGE_PAIRS) else 0)
        res = idx.find_mems(cat, offs, 20, 1, tags=True)
        assert np.array_equal(res["mem_offsets"], ref["mem_offsets"])
        assert res["mems"].tobytes() == ref["mems"].tobytes()
        assert res["n_extensions"] == ref["n_extensions"]
        assert np.array_equal(res["tag_run_counts"], ref["tag_run_counts"])
        assert np.array_equal(res["pos_offsets"], ref["pos_offsets"])
        assert np.array_equal(res["positions"], ref["positions"])
        assert res["n_tag_overflow"] == ref["n_tag_overflow"]
        idx.close()


@pytest.fixture(scope="module")
def chr22(workdir):
    """BASELINE configs[2] at its own size: the chr22-scale index (n = 640 M), the bench's 10 M reads, the oracle on their first 1 M reads and
    on a sample of reads from the whole batch"""
    text = os.path.join(workdir, "chr22_synth.txt")
    W.synth_pangenome_text(text, base_len=40_000_000, n_hap=8, seed=45)  # bench.py's chr22 workload
    ri_path, tags_path = W.build_index_from_text(text, workdir, "chr22_synth")[:2]
    seqs = W.load_sequences(text)
    cat, offs = W.sample_reads(seqs, 10_000_000, 150, seed=42 + 3)
    del seqs
    n1 = 1_000_000
    cat1, offs1 = cat[: n1 * 150], offs[: n1 + 1]
    ri, tags = O.RIndex(ri_path), O.Tags(tags_path, O.TAGS_COMPACT)
    assert ri.sigma == 6 and ri.n > 600_000_000
    ref = _oracle(ri, tags, cat1, offs1)
    sample, side = _sample(cat, offs, seed=61, random_from=n1)
    scat, soffs = S.gather_reads(cat, offs, sample)
    sref = _oracle(ri, tags, scat, soffs)
    del ri, tags
    assert len(side) > 1000  # reads over the text's N runs: the second stream's kernel across the whole batch
    print("\n[fullsize] chr22: sample of %d reads of 10 M (%d with a byte outside ACGT), %d MEMs, %d positions"
          % (len(sample), len(side), len(sref["mems"]), len(sref["positions"])))
    idx = P.Index(ri_path, tags_path, mode=P.MODE_COMPAT)
    env = types.SimpleNamespace(text=text, ri_path=ri_path, tags_path=tags_path, cat=cat, offs=offs, n1=n1, cat1=cat1, offs1=offs1, ref=ref,
                                sample=sample, side=side, scat=scat, soffs=soffs, sref=sref, idx=idx)
    yield env
    idx.close()


@pytest.fixture(scope="module")
def chr22_10m(chr22):
    """the bench batch shape -- 10 M reads in ONE chunk -- run once (exactly: the first run of the batch); the batch is kept for its
    speculative re-runs"""
    b10 = chr22.idx.batch(chr22.cat, chr22.offs)
    b10.run(20, 1, FLAGS)
    env = types.SimpleNamespace(batch=b10, timing=b10.timing(), res=b10.result())
    yield env
    b10.free()


def test_chr22_scale_automatic_layout(chr22, chr22_10m):
    """BASELINE configs[2] at its own size (the bench default; reference unit: src/find_mems.cpp:94-139): n = 640 M, automatic layout
    (dense2 + two-step pairs image, seed table of depth 16 = 64 GiB + the depth-10 table + end table), 1 M reads bit-identical to the
    oracle; then the bench batch shape -- 10 M reads in ONE chunk -- whose first 1 M reads are those reads: same results inside the bigger
    batch; and its sample from the whole batch (last 20 000 reads included) bit-identical to the oracle."""
    ref, n1, idx = chr22.ref, chr22.n1, chr22.idx
    assert len(ref["mems"]) > 1_500_000 and ref["n_extensions"] > 150_000_000
    info = idx.info()
    assert info.image_kind == P.IMAGE_DENSE2 and info.image_pairs == 1 and not info.image_in_lds
    b1 = idx.batch(chr22.cat1, chr22.offs1)
    b1.run(20, 1, P.RUN_TAGS | P.RUN_TIMING)
    t = b1.timing()
    assert t.pairs_reads == 4 and t.main_lines > 0 and t.main_seed_loads > 0  # the two-step kernel behind the seed table ran, reads packed in LDS, narrow forward stages through the text
    assert t.seed_depth == 16 and t.find_mems_launches == 1
    res = b1.result()
    b1.free()

    def same(res, m, npos):
        assert np.array_equal(res["mem_offsets"][: n1 + 1], ref["mem_offsets"])
        assert res["mems"][:m].tobytes() == ref["mems"].tobytes()
        assert np.array_equal(res["tag_run_counts"][:m], ref["tag_run_counts"])
        assert np.array_equal(res["pos_offsets"][: m + 1], ref["pos_offsets"])
        assert np.array_equal(res["positions"][:npos], ref["positions"])

    m, npos = len(ref["mems"]), len(ref["positions"])
    same(res, m, npos)
    assert res["n_extensions"] == ref["n_extensions"] and res["n_tag_overflow"] == ref["n_tag_overflow"]
    assert len(res["mems"]) == m and len(res["positions"]) == npos
    del res
    assert chr22_10m.timing.find_mems_launches == 1 and chr22_10m.timing.seed_depth == 16  # one chunk, as bench.py measures it
    res10 = chr22_10m.res
    same(res10, m, npos)
    assert len(res10["mem_offsets"]) == 10_000_001 and res10["n_extensions"] > 9 * ref["n_extensions"]
    # (a) reads from the whole batch, not only its first 1 M
    S.compare(S.subset(res10, chr22.sample), chr22.sref, chr22.sample, what="chr22 10 M, exact first run, sample")


def test_chr22_speculative_reruns_whole_batch(chr22_10m):
    """(b) the bench's timed steps re-run the resident 10 M batch speculatively (one chunk, largest tag query <= 16384 runs): steps 2 and 3
    byte for byte equal to the exact first run over the whole batch, n_extensions and n_tag_overflow included"""
    _speculative_reruns(chr22_10m.batch, chr22_10m.res, "chr22 10 M", require_spec=True)
    chr22_10m.batch.free()


def test_chr22_sample_as_its_own_batch(chr22):
    """(c) bench.py's ext_ok over reads from the whole batch: the sample run as a batch of its own equals the oracle, n_extensions included"""
    own = chr22.idx.find_mems(chr22.scat, chr22.soffs, 20, 1, tags=True)
    S.compare(own, chr22.sref, chr22.sample, totals=True, what="chr22 sample as its own batch")


def test_chr22_several_chunks_whole_batch(chr22, chr22_10m, monkeypatch):
    """(d) the 10 M reads cut into several chunks by a smaller slot budget (a chunk's worst-case slots are about its read bytes, 32 B each):
    per-chunk scans, arenas and offsets, the same bytes as the one-chunk run over the whole batch"""
    monkeypatch.setenv("PGX_SLOT_BUDGET_MB", "11000")
    b = chr22.idx.batch(chr22.cat, chr22.offs)
    b.run(20, 1, FLAGS)
    launches = b.timing().find_mems_launches
    res = b.result()
    b.free()
    print("\n[fullsize] chr22 10 M under a slot budget of 11000 MB: %d chunks" % launches)
    assert 3 <= launches <= 6
    S.compare(res, chr22_10m.res, totals=True, what="chr22 10 M in %d chunks against one chunk" % launches)


def test_chr22_packed_upload_whole_batch(chr22, chr22_10m):
    """(e) the bench's fresh-batch shape: the 10 M reads packed to two bits on the host (pgx_pack_reads), the reads with a byte outside
    A C G T listed beside them, uploaded from pinned memory (pgx_batch_upload_packed) -- the same bytes as the byte upload over the whole batch"""
    cat, offs = chr22.cat, chr22.offs
    n = len(offs) - 1
    poffs = P.pinned_array(n + 1, np.uint64)
    poffs[:] = offs
    packed = P.pinned_array((len(cat) + 15) // 16, np.uint32)
    side_ids = P.pinned_array(n // 8 + 1024, np.uint64)
    side_bytes = P.pinned_array(len(cat) // 8 + 4096, np.uint8)
    n_side, n_side_bytes = P.pack_reads(cat, offs, packed, side_ids, side_bytes)
    assert n_side == len(chr22.side) and np.array_equal(side_ids[:n_side], chr22.side) and n_side_bytes == 150 * n_side
    b = chr22.idx.batch_empty()
    b.upload_packed(packed, poffs, side_ids, side_bytes, n_side)
    b.run(20, 1, FLAGS)
    assert b.timing().find_mems_launches == 1
    res = b.result()
    b.free()
    S.compare(res, chr22_10m.res, totals=True, what="chr22 10 M, packed upload against the byte upload")


def test_chr22_read_bytes_past_2_31(chr22):
    """(f) one batch of 15 M reads x 150 = 2.25e9 bytes, past 2^31 (read offsets, slot offsets and byte indices beyond 31 bits), other reads
    than the 10 M: its sample, plus every read with bytes within 10^4 of byte 2^31, against the oracle.  Whether it is one chunk depends on
    the device's memory (the slot budget is a quarter of it); parity is asserted, the chunk count recorded."""
    seqs = W.load_sequences(chr22.text)
    cat, offs = W.sample_reads(seqs, 15_000_000, 150, seed=42 + 7)
    del seqs
    assert len(cat) == 2_250_000_000
    lo, hi = (1 << 31) - 10_000, (1 << 31) + 10_000
    o = offs.astype(np.int64)
    border = np.flatnonzero((o[1:] > lo) & (o[:-1] < hi))
    sample, side = _sample(cat, offs, seed=62, random_from=chr22.n1, extra=border)
    scat, soffs = S.gather_reads(cat, offs, sample)
    ri, tags = O.RIndex(chr22.ri_path), O.Tags(chr22.tags_path, O.TAGS_COMPACT)
    sref = _oracle(ri, tags, scat, soffs)
    del ri, tags, scat, soffs
    b = chr22.idx.batch(cat, offs)
    del cat
    b.run(20, 1, FLAGS)
    launches = b.timing().find_mems_launches
    res = b.result()
    b.free()
    print("\n[fullsize] chr22 15 M reads (2.25e9 bytes): %d chunk(s); sample of %d reads (%d with a byte outside ACGT, %d around byte 2^31)"
          % (launches, len(sample), len(side), len(border)))
    assert len(border) >= 130 and len(res["mem_offsets"]) == 15_000_001
    S.compare(S.subset(res, sample), sref, sample, what="chr22 15 M reads, sample")


def _whole_genome_case(workdir, name, chroms, base_len, haps, n_reads, n1, full):
    """the body of the whole-genome-scale test; full = False: the same recipe on a small collection forced into the 64-bit form with
    superblocks of a few blocks (PGX_SB_SHIFT set by the caller), so that the recipe itself -- border reads included -- is exercised in seconds"""
    from image_emu import Consts

    texts = W.synth_chromosome_texts(workdir, name, chroms, base_len, haps, seed=45, n_runs=2, n_run_len=(1000, 10000) if full else (50, 400))
    ri_path, tags_path = W.build_index_from_texts(texts, workdir, name)[:2]
    seqs = []
    for t in texts:
        seqs += W.load_sequences(t)
    assert len(seqs) == 2 * chroms * haps
    cat, offs = W.sample_reads(seqs, n_reads, 150, seed=42 + 5)
    ri, tags = O.RIndex(ri_path), O.Tags(tags_path, O.TAGS_COMPACT)
    assert ri.sigma == 6
    if full:
        assert ri.n == 4_351_996_034 and ri.n > 1 << 32

    idx = P.Index(ri_path, tags_path, mode=P.MODE_COMPAT | (0 if full else P.MODE_IMAGE_WIDE))
    info = idx.info()
    assert info.image_kind == P.IMAGE_DENSE2 and info.image_pairs == 1 and info.image_wide == 1 and info.pairs_stride == 64 and not info.image_in_lds
    c = Consts(idx.image_view(6))
    assert c.wide == 1 and 2 <= c.n_sb2 <= 64 and 2 <= c.n_sbp <= 64
    # reads whose search ends in an interval next to a superblock border: the text at the suffix array's values there (packed as
    # sequence * max_length + offset, src/r-index.cpp:1300-1343)
    borders = [k * (384 << c.d2_sb_shift) for k in range(1, c.n_sb2)] + [k * (c.pairs_stride << c.pairs_sb_shift) for k in range(1, c.n_sbp)]
    borders = [b for b in borders if 100 < b < ri.n - 100]
    assert len(borders) >= 4
    extra, near = [], 0
    ml = ri.max_length
    for b in borders:
        sa = ri.locate_sa(b - 24, b + 24)
        for i, v in enumerate(sa):
            s, o = int(v) // ml, int(v) % ml
            rd = bytes(seqs[s][o:o + 150])
            if len(rd) == 150 and b"N" not in rd:
                lo, hi = ri.count(rd)
                assert lo <= b - 24 + i <= hi
                near += 1 if lo <= b <= hi + 1 else 0
                extra.append(rd)
    assert near >= len(borders) // 2  # final intervals that touch a border itself
    q = len(seqs) // 2
    extra += [b"N" * 150, bytes(seqs[0][-150:]), bytes(seqs[1][:150]), bytes(seqs[-1][-150:]), bytes(seqs[q][:150]), b"acgt" * 30, b"ACGTNACGT" * 10, b"",
              bytes(seqs[7][1000:1100]), bytes(seqs[q + 1][-40:])]
    del seqs
    ecat, eoffs = O.pack_reads(extra)
    cat1 = np.concatenate([cat[: n1 * 150], ecat])
    offs1 = np.concatenate([offs[: n1 + 1], eoffs[1:] + offs[n1]])
    ref = O.find_mems_batch(ri, tags, cat1, offs1, 20, 1, threads=O.lib().orc_max_threads())
    # reads from the whole big batch (its last 20 000 included) for the oracle
    sample, side = _sample(cat, offs, seed=63, random_from=n1)
    sref = _oracle(ri, tags, *S.gather_reads(cat, offs, sample))
    del ri, tags
    assert len(ref["mems"]) > 1.5 * n1 and ref["n_extensions"] > 150 * n1
    print("\n[fullsize] %s: sample of %d reads of %d (%d with a byte outside ACGT)" % (name, len(sample), n_reads, len(side)))

    b1 = idx.batch(cat1, offs1)
    b1.run(20, 1, P.RUN_TAGS | P.RUN_TIMING)
    t = b1.timing()
    assert t.find_mems_launches == 1 and t.main_lines > 0 and t.seed_depth > 0
    if full:
        assert t.pairs_reads == 3 and t.seed_depth == 16  # cooperative line fetches + packed reads, seed table of depth 16 (64 GiB, 40-bit fields)
    else:
        assert t.pairs_reads == 2
    res = b1.result()
    b1.free()
    assert np.array_equal(res["mem_offsets"], ref["mem_offsets"])
    assert res["mems"].tobytes() == ref["mems"].tobytes()
    assert res["n_extensions"] == ref["n_extensions"] and res["n_tag_overflow"] == ref["n_tag_overflow"]
    assert np.array_equal(res["tag_run_counts"], ref["tag_run_counts"])
    assert np.array_equal(res["pos_offsets"], ref["pos_offsets"])
    assert np.array_equal(res["positions"], ref["positions"])
    if full:
        assert int(res["mems"]["bwt_start"].max()) > 1 << 32  # (64-bit coordinates in the output)
    del res
    b10 = idx.batch(cat, offs)
    b10.run(20, 1, P.RUN_TAGS | P.RUN_TIMING)
    assert b10.timing().find_mems_launches == 1 and b10.timing().pairs_reads == (3 if full else 2)  # one chunk, as bench.py --workload wg measures it
    res10 = b10.result()
    m = int(ref["mem_offsets"][n1])
    npos = int(ref["pos_offsets"][m])
    assert np.array_equal(res10["mem_offsets"][: n1 + 1], ref["mem_offsets"][: n1 + 1])
    assert res10["mems"][:m].tobytes() == ref["mems"][:m].tobytes()
    assert np.array_equal(res10["tag_run_counts"][:m], ref["tag_run_counts"][:m])
    assert np.array_equal(res10["pos_offsets"][: m + 1], ref["pos_offsets"][: m + 1])
    assert np.array_equal(res10["positions"][:npos], ref["positions"][:npos])
    assert len(res10["mem_offsets"]) == n_reads + 1
    # (a) the exact first run on reads from the whole batch; (b) the bench's speculative re-runs over the whole batch
    S.compare(S.subset(res10, sample), sref, sample, what="%s, exact first run, sample" % name)
    _speculative_reruns(b10, res10, name)
    b10.free()
    idx.close()
    for p in texts:
        os.remove(p)


def test_whole_genome_recipe_on_a_small_collection(workdir, monkeypatch):
    """the recipe of the next test -- several chromosome texts merged by pgx_build_index_from_texts, reads at the superblock borders of both
    64-bit images, a small batch, the prefix of a big one, a sample of the big one from its whole length and its speculative re-runs -- on
    3 chromosomes x 60 kbp x 4 haplotypes, forced into the 64-bit form with superblocks of 2^7 dense2 blocks and 2^9 PAIRS blocks (about 30
    and 44 of them)"""
    monkeypatch.setenv("PGX_SB_SHIFT", "7")
    _whole_genome_case(workdir, "wg_small", 3, 60_000, 4, 200_000, 20_000, full=False)


def test_whole_genome_scale_wide_layout(workdir):
    """BASELINE configs[4]'s single-GPU ingredient at its own size (the reference is size_t end to end: include/pangenome_index/r-index.hpp:118-130,
    src/r-index.cpp:713-756): one merged index of n = 4 351 996 034 > 2^32 symbols (bench.py --workload wg: 8 chromosomes x 8.5 Mbp x 32 haplotypes
    x 2 strands, 512 sequences) built by pgx_build_index_from_texts; the automatic layout must be the 64-bit one (WIDE dense2 + WIDE PAIRS at
    stride 64 behind cooperative line fetches, seed table of depth 16 with 40-bit fields).  100 k sampled reads plus reads that end / start a
    sequence, an all-N read, lower case, and reads whose BWT intervals lie across the superblock borders of both images (their 64-bit bases
    change there) bit-identical to the oracle incl. tags and n_extensions; then the bench batch shape -- 10 M reads in one chunk -- whose first
    100 k reads give the same bytes, whose sample from the whole batch equals the oracle, and whose speculative re-runs give the same bytes
    over the whole batch."""
    _whole_genome_case(workdir, "wg_8_8500000_32", 8, 8_500_000, 32, 10_000_000, 100_000, full=True)
