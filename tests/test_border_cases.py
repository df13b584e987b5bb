"""The case tables of border_cases.py realise what they claim -- asserted with the oracle and numpy alone, so that no GPU test of
test_gpu_tag_borders.py, test_gpu_spec_borders.py, test_gpu_locate_borders.py, test_gpu_mem_locate_borders.py or test_gpu_heavy_limits.py can pass
by missing its target."""
import numpy as np
import pytest

import border_cases as B
import oracle_ffi as O
import pgx_ffi as P
import variant_cases as V


# ---- 1. tag queries -------------------------------------------------------------------------------------------------------------------------
def test_border_table_sits_on_every_threshold():
    """k - 1, k and k + 1 of every class border, both sides of the power-of-two pads 1024 and 8192, the full LDS allocation and the first
    global-scratch segment"""
    for k in (B.TAG_SMALL, B.SORT_WAVE_REGS, B.SORT_LDS_CAP, B.SORT_WG_LDS_CAP):
        assert {k - 1, k, k + 1} <= set(B.BORDER_C), k
        assert B.size_class(k) != B.size_class(k + 1) and B.size_class(k - 1) == B.size_class(k)
    assert {1, 2, 1024, 1025, 8192, 8193, 32768, 32769} <= set(B.BORDER_C)
    assert B.pad2(1024) == 1024 and B.pad2(1025) == 2048 and B.pad2(8192) == 8192 and B.pad2(8193) == 16384
    assert B.pad2(16384) == B.SORT_WG_LDS_CAP and B.pad2(16385) == 32768 and B.pad2(32769) == 65536
    assert {B.size_class(c) for c in B.BORDER_C} == {"single", "small", "wave_regs", "wave_lds", "wg_lds", "wg_scratch"}


@pytest.mark.parametrize("pattern", B.TAG_PATTERNS)
def test_border_queries_have_exactly_c_runs(workdir, pattern):
    arr = B.tag_array(workdir, pattern)
    t = arr.oracle()
    assert t.n_runs == B.N_TAG_RUNS
    for c in B.BORDER_C:
        fs = B.border_first_runs(c)
        assert [f % 10 for f in fs] == list(B.BORDER_F_MOD) and len(set(fs)) == 3
        for f in fs:
            st, en = arr.query(f, c)
            rn, pos, over = t.query(st, en)
            exp, eover = arr.expected(f, c)
            assert rn == c and not over and not eover, (c, f)
            assert np.array_equal(np.array(pos, dtype=np.uint64), exp), (c, f)  # pins the first item: f - 1, or f where f % 10 == 0
            if pattern == "equal":
                assert len(pos) == 1
            if pattern == "distinct":
                assert len(pos) == c
            if pattern == "random" and c >= 1024:
                assert 1 < len(pos) < c
    # the first item really differs between f % 10 == 0 and the rest: on distinct values the answer of f holds vals[f + c - 1], not vals[f - 1]
    if pattern == "distinct":
        f = B.border_first_runs(17)[0]
        got = set(t.query(*arr.query(f, 17))[1])
        assert int(arr.vals[f + 16]) in got and int(arr.vals[f - 1]) not in got


def test_overflow_sites_overflow_in_the_oracle(workdir):
    arr = B.tag_array(workdir, "random")
    t = arr.oracle()
    classes = {"single": "single", "small": "small", "big": "wave_lds", "large": "wg_lds", "large_scratch": "wg_scratch", "large_dups": "wg_lds"}
    for name, site in B.OVERFLOW_SITES.items():
        for f, copies in site:
            c = B.N_TAG_RUNS - f + 1
            assert f % 10 == 0 and B.size_class(c) == classes[name]
            rn, pos, over = t.query(*arr.query(f, c))
            assert rn == c and over, name
            exp, eover = arr.expected(f, c)
            assert eover and np.array_equal(np.array(pos, dtype=np.uint64), exp) and exp[0] == 0  # the item beyond the array reads as 0
    assert B.OVERFLOW_SITES["large_dups"][0][1] == 3
    seen = set()
    for f, c in B.OVERFLOW_CONTROLS:
        rn, pos, over = t.query(*arr.query(f, c))
        assert rn == c and not over, (f, c)
        seen.add(B.size_class(c))
    assert seen == {"single", "small", "wave_lds", "wg_lds", "wg_scratch"}
    assert B.OVERFLOW_CONTROLS.count((30000, 5001)) == 2  # a duplicate pair that does not overflow
    assert (69991, 10) in B.OVERFLOW_CONTROLS and 69991 + 10 - 1 == B.N_TAG_RUNS  # ends in the last run, f % 10 != 0
    expect = {"single": 1, "small": 1, "big": 1, "large": 1, "large_scratch": 1, "large_dups": 3}
    for name, k in expect.items():
        st, en = arr.queries(B.overflow_batch([name]))
        assert int(arr.answers(("over", name), st, en)[3].sum()) == k
    st, en = arr.queries(B.overflow_batch(list(B.OVERFLOW_SITES)))
    assert int(arr.answers(("over", "all"), st, en)[3].sum()) == 8


def test_inverted_queries_have_no_runs(workdir):
    arr = B.tag_array(workdir, "random")
    st, en = B.inverted_queries(arr)
    rn, po, pos, over = arr.answers("inverted", st, en)
    assert np.all(en + np.uint64(1) == st) and not rn.any() and not po.any() and not over.any()
    assert sorted((a + 1) % 10 == 0 for a in B.INVERTED_RUNS) == [False, False, True, True]


def test_query_count_batches(workdir):
    """prefixes of one list: one query less than a scan tile, a full tile, one more, two tiles, two tiles and one; the last two queries of
    every prefix have a segment and unique values, so out[n] of both scans differs from out[n - 1]"""
    assert {B.SCAN1_TILE_ITEMS - 1, B.SCAN1_TILE_ITEMS, B.SCAN1_TILE_ITEMS + 1, 2 * B.SCAN1_TILE_ITEMS, 2 * B.SCAN1_TILE_ITEMS + 1} == set(B.QUERY_COUNTS)
    arr = B.tag_array(workdir, "random")
    fc = B.count_queries()
    st, en = arr.queries(fc)
    rn, po, pos, over = arr.answers("counts", st, en)
    assert np.array_equal(rn, np.array([c for _, c in fc], dtype=np.uint64)) and not over.any()
    for n in B.QUERY_COUNTS:
        assert rn[n - 1] > 1 and rn[n - 2] > 1 and po[n] > po[n - 1] > po[n - 2]
        assert {B.size_class(int(c)) for c in rn[:n]} >= {"single", "small", "wave_regs", "wave_lds", "wg_lds"}
    assert "wg_scratch" in {B.size_class(int(c)) for c in rn}


# ---- 3. locate ranges -------------------------------------------------------------------------------------------------------------------------
def test_locate_ranges_have_exactly_c_positions_and_duplicates(workdir):
    case = B.locate_case(workdir)
    for k in (B.SORT_WAVE_REGS, B.SORT_LDS_CAP, B.SORT_WG_LDS_CAP):
        assert {k - 1, k, k + 1} <= set(B.LOCATE_C)
    cs = np.repeat(np.array(B.LOCATE_C, dtype=np.uint64), 3)
    assert np.array_equal(case["last"] - case["first"] + np.uint64(1), cs) and int(case["last"].max()) == case["n"] - 1
    off, vals = B.locate_expected(case, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE)
    uniq = np.diff(off)
    assert int(vals.max()) == 7  # 8 sequences
    for i, c in enumerate(cs):
        if c >= 2 and (i % 3 == 0 or c > 8):
            assert uniq[i] < c, (i, c)  # SEQ_IDS | UNIQUE really removes duplicates
    off, vals = B.locate_expected(case, P.LOCATE_UNIQUE)
    assert np.array_equal(np.diff(off), cs)  # suffix array values are distinct: UNIQUE alone only sorts
    r = O.RIndex(case["ri_path"])
    for i in (0, 3, 6, 15):  # the oracle's literal locate agrees with numpy on its suffix array
        o2, v2 = B.locate_expected(case, P.LOCATE_SEQ_IDS | P.LOCATE_UNIQUE)
        assert np.array_equal(r.locate(int(case["first"][i]), int(case["last"][i]), O.MODE_STRICT), v2[int(o2[i]):int(o2[i + 1])])


# ---- 4. heavy reads ---------------------------------------------------------------------------------------------------------------------------
def test_heavy_cases_pass_their_limits(workdir):
    mid = V.mid_case(workdir)
    ri = O.RIndex(mid["ri_path"])
    cat, offs = B.heavy_cap_reads(mid)
    assert len(offs) - 1 == B.HEAVY_CAP_READS > B.FM_HEAVY_CAP
    # a read is handed on at the first start position it reaches with HEAVY_EXT extensions spent and at least min_len symbols left: every read
    # that needs a second start position after that many extensions qualifies
    n_offered = 0
    for i in range(B.HEAVY_CAP_READS):
        read = bytes(cat[int(offs[i]):int(offs[i + 1])])
        x, ne = 0, 0
        while x < len(read) and len(read) - x >= 20:
            if ne >= B.HEAVY_EXT:
                n_offered += 1
                break
            x, _, e = ri.find_mems_function(read, 20, 1, x)
            ne += e
    assert n_offered > B.FM_HEAVY_CAP + 200, n_offered
    cat, offs = B.heavy_long_reads(mid)
    lens = np.diff(offs)[-len(B.HEAVY_LENGTHS):]
    assert list(lens) == list(B.HEAVY_LENGTHS)
    assert {B.FM_HEAVY_MAXLEN - 1, B.FM_HEAVY_MAXLEN, B.FM_HEAVY_MAXLEN + 1} <= set(B.HEAVY_LENGTHS)
    for k in range(len(B.HEAVY_LENGTHS)):
        i = len(offs) - 1 - len(B.HEAVY_LENGTHS) + k
        read = bytes(cat[int(offs[i]):int(offs[i + 1])])
        assert b"N" not in read
        mems, ne = ri.find_all_mems(read, 20, 1, with_ext=True)
        assert ne > B.HEAVY_EXT and len(mems) >= len(read) // 150  # many start positions, each MEM bounded by the substitutions
        assert max(m[1] - m[0] for m in mems) < 400


# ---- 2. overflow and capacities through pgx_batch_run -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("site", B.OVERFLOW_FILES)
def test_overflow_files_overflow_at_one_site(workdir, site):
    """in the oracle's answer on the shortened tag array the overflowing MEMs are all of the site's class; the large-class file holds one
    such MEM (no copy), the duplicates file the same query three times"""
    case = B.spec_case(workdir)
    key, tags_path, reads = B.overflow_file(case, site)
    cat, offs, ref = case.ref(key, tags_path, reads)
    over = case.mem_overflows(tags_path, ref)
    assert ref["n_tag_overflow"] == int(over.sum()) > 0
    rc = ref["tag_run_counts"][over]
    distinct = {(int(m["bwt_start"]), int(m["size"])) for m in ref["mems"][over]}
    if site == "single":
        assert np.all(rc == 1) and len(rc) > 1000
        assert O.Tags(tags_path, O.TAGS_COMPACT).n_runs % 10 == 0
    elif site == "small":
        assert np.all((rc >= 2) & (rc <= B.TAG_SMALL))
    elif site == "big":
        assert np.all((rc > B.TAG_SMALL) & (rc <= B.SORT_LDS_CAP))
    elif site == "large":
        assert np.all(rc > B.SORT_LDS_CAP) and len(rc) == len(distinct) == 1  # a representative only
    else:
        assert np.all(rc > B.SORT_LDS_CAP) and len(rc) == 3 and len(distinct) == 1  # one representative, two copies
    # MEMs of the other classes are in the batch and do not overflow
    others = {B.size_class(int(c)) for c in ref["tag_run_counts"][~over]}
    assert {"single", "small"} <= others and (site == "single" or "wave_regs" in others or site == "big")
    # the batch that makes the run fall back has far fewer MEMs
    jref = case.ref(key + "_junk", tags_path, B.junk_reads(len(reads)))[2]
    assert B.exceeded(jref, ref) >= {"mems"} and jref["n_tag_overflow"] == 0


def test_capacity_batches_exceed_what_they_claim(workdir):
    case = B.spec_case(workdir)
    batches = B.capacity_batches(case)
    ra = case.ref("cap_A", case.full_tags, batches["A"])[2]
    da = B.demand(ra)
    assert B.SORT_LDS_CAP < da["largest"] <= 4096 and B.capacities(ra)["largest"] == 8192
    assert set(batches) == {"A"} | set(B.CAPACITY_EXCEEDED)
    union = set()
    for name, want in B.CAPACITY_EXCEEDED.items():
        assert len(batches[name]) == len(batches["A"])
        rb = case.ref("cap_" + name, case.full_tags, batches[name])[2]
        assert B.exceeded(ra, rb) == want, name
        assert B.exceeded(rb, ra) == set(), name  # A fits the capacities of a run of B: uploading A again stays speculative
        assert B.demand(rb)["largest"] <= B.SORT_WG_LDS_CAP
        union |= want
    assert union == {"mems", "G", "small", "big", "large", "largest", "P"}
    assert B.CAPACITY_EXCEEDED["largest"] == {"largest"} and B.CAPACITY_EXCEEDED["mems"] == {"mems"}  # each the only capacity exceeded
    rb = case.ref("cap_largest", case.full_tags, batches["largest"])[2]
    assert 8192 < B.demand(rb)["largest"] <= B.SORT_WG_LDS_CAP


def test_query_beyond_the_lds_sort_capacity(workdir):
    case = B.spec_case(workdir)
    ref = case.ref("over16384", case.full_tags, B.over_16384_reads(case))[2]
    assert B.demand(ref)["largest"] > B.SORT_WG_LDS_CAP and ref["n_tag_overflow"] == 0


# ---- 3b. MEMs of exactly 2047 .. 16385 occurrences ---------------------------------------------------------------------------------------------
def test_mem_locate_collection_has_mems_of_the_border_sizes(workdir):
    case = B.mem_locate_case(workdir)
    assert case["n"] <= 1_700_000
    for k in (B.SORT_LDS_CAP, B.SORT_WG_LDS_CAP):
        assert {k, k + 1} <= set(B.MEM_LOCATE_OCC)
    assert B.SORT_LDS_CAP - 1 in B.MEM_LOCATE_OCC
    ref = case["ref"]
    first = ref["mems"][ref["mem_offsets"][:2 * len(B.MEM_LOCATE_OCC)].astype(np.int64)]  # the one MEM of each region read and of its reverse complement
    assert np.all(np.diff(ref["mem_offsets"])[:2 * len(B.MEM_LOCATE_OCC)] == 1)
    assert [int(s) for s in first["size"]] == [occ for occ in B.MEM_LOCATE_OCC for _ in range(2)]
    off, vals = B.mem_locate_expected(case, P.LOCATE_UNIQUE)
    assert np.array_equal(np.diff(off).astype(np.int64), ref["mems"]["size"])
    sizes = set(int(s) for s in ref["mems"]["size"])
    assert {B.size_class(s) for s in sizes} >= {"small", "wave_lds", "wg_lds", "wg_scratch"}
