"""GPU tier of the GAF replay: what pgx_batch_read_align, pgx_batch_read_walk and find_mems --gaf say about every read of tests/replay_cases.py is
replayed by tests/gaf_replay.py -- the CIGAR over the read and the text of Index.text(), the oriented nodes of the case's own graph spelled out
and sliced -- with no read left out and no emulator asked (tests/test_gaf_replay_cpu.py shows that the checker accepts the emulators and
catches every listed mutation).

  a. the bindings on the walk graph: run, locate, read_place, read_verify(1, 4), read_align(band, ALIGN_CIGAR), read_walk(WALK_STEPS) at bands 0, 8
     and 31, and once with read_verify(16, 1, VERIFY_LIST) at band 31; edits never grow with the band and equal verify's mismatches at band 0;
     every mixed, heavy and byte read has a winner; the kept-read bound (replay_cases.check_kept_bound) with at most 10 % of the mixed reads
     left out at band 31; every class of replay_cases.class_counts is reached
  b. the same through one batch that is filled twice, with another number of reads
  c. find_mems --gaf on the walk graph, with the defaults and with small batches, two workers, device formatting and device-parsed reads: as
     many lines as reads, in input order, each replayed from its text alone, both files equal
  d. find_mems --gaf on the golden xy.ri with the node sequences of xy.gbz"""
import os
import subprocess

import pytest

import gaf_replay as G
import gbz_graph_emu as GG
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W
import replay_cases as C

pytestmark = pytest.mark.gpu

K = C.CASES
N = len(K.reads)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pangenome-index_amd", "find_mems")
RUNS = [(0, 1, 4), (8, 1, 4), (31, 1, 4), (31, 16, 1)]  # (band, verify's max_cand, verify's mismatch penalty)


@pytest.fixture(scope="module")
def world(workdir):
    """the walk graph's index with tags made from its path table, and the text the index gives back"""
    g = K.graph
    text = os.path.join(workdir, "replay_graph.txt")
    with open(text, "wb") as f:
        f.write(b"".join(t + b"\n" for t in g["texts"]))
    ri = W.build_index_from_text(text, workdir, "replay_graph", with_tags=False)[0]
    tags = os.path.join(workdir, "replay_graph.graph.tags")
    P.build_tags_paths(ri, g["path_offsets"], g["path_nodes"], g["node_length"], 1, tags, flags=P.BUILD_TAGS_OUT_COMPACT)
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    texts = idx.text()[1].split(b"\n")[:-1]
    idx.close()
    assert len(texts) == len(g["texts"])
    return ri, tags, texts


def _stages(b, band, max_cand, penalty):
    """locate .. walk on a batch that has been run: (verify records, align result, walk result)"""
    b.locate(0)
    b.read_place(P.PLACE_LIST if max_cand > 1 else 0)
    v = b.read_verify(max_cand, penalty, P.VERIFY_LIST if max_cand > 1 else 0)
    a = b.read_align(band, P.ALIGN_CIGAR)
    w = b.read_walk(P.WALK_STEPS)
    return v["reads"], a, w


def _replay(reads, texts, a, w, band, numbers=None):
    n = len(reads)
    assert (a["n_reads"], w["n_reads"], len(a["reads"]), len(w["reads"]), a["band"]) == (n, n, n, n, band)
    assert int(a["op_offsets"][0]) == 0 == int(w["step_offsets"][0]) and int(a["op_offsets"][n]) == len(a["ops"]) and int(w["step_offsets"][n]) == len(w["steps"])
    steps = []
    for r in range(n):
        ops = a["ops"][int(a["op_offsets"][r]):int(a["op_offsets"][r + 1])]
        steps.append(w["steps"][int(w["step_offsets"][r]):int(w["step_offsets"][r + 1])].tolist())
        G.replay_record(reads[r], texts, K.node_seq, a["reads"][r], w["reads"][r], steps[r], ops, band=band, number=r if numbers is None else numbers[r])
    return steps


@pytest.fixture(scope="module")
def device(world):
    """the records of every run of RUNS over all reads, from one batch"""
    ri, tags, texts = world
    cat, offs = O.pack_reads(K.reads)
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    b = P.Batch(idx, cat, offs)
    b.run(C.MIN_LEN, 1, P.RUN_TAGS)
    out = {run: _stages(b, *run) for run in RUNS}
    b.free()
    idx.close()
    return out


@pytest.mark.parametrize("run", RUNS)
def test_every_record_replays(world, device, run):
    v, a, w = device[run]
    steps = _replay(K.reads, world[2], a, w, run[0])
    assert (a["reads"]["seq"] == v["seq"]).all() and (a["reads"]["diag"] == v["diag"]).all() and (w["reads"]["seq"] == v["seq"]).all()
    placed = K.of("mixed", "heavy", "byte_", "end", "node_", "one_bp")
    assert (a["reads"]["seq"][placed] != G.NO_SEQUENCE).all()  # an untouched stretch of 19 bases or more: a MEM, so a winner
    assert (a["reads"]["seq"][K.of("none")] == G.NO_SEQUENCE).all()
    counts = C.class_counts(a["reads"], w["reads"], steps)
    print("band %d, verify(%d, %d): %d reads replayed; %r" % (run + (N, counts)))
    assert all(counts[k] >= 1 for k in counts if run[0] > 0 or k not in ("ins", "dels", "both")), counts
    capped = C.check_kept_bound(K, a["reads"], run[0], K.of("mixed"), capped=run[0] == 31)
    others = C.check_kept_bound(K, a["reads"], run[0], K.of("heavy", "byte_"), capped=False)
    print("band %d, verify(%d, %d): %d of %d mixed reads kept, %d left out (%d kept with the stretch widened by the band); heavy and byte reads: %d kept, %d left out"
          % (run + (capped[0], C.N_MIXED, capped[1], capped[2], others[0], others[1])))


def test_edits_across_the_bands(device):
    for r in range(N):
        G.replay_bands({run[0]: device[run][1]["reads"][r] for run in RUNS[:3]}, device[RUNS[0]][0]["mismatches"][r], number=r)
    wide, narrow = device[RUNS[2]][1]["reads"], device[RUNS[1]][1]["reads"]
    assert (wide["edits"] < narrow["edits"]).any() and (narrow["edits"] < device[RUNS[0]][1]["reads"]["edits"]).any()


def test_a_refilled_batch_replays(world):
    ri, tags, texts = world
    first, second = K.of("end", "byte_"), K.of("mixed")
    idx = P.Index(ri, tags, mode=P.MODE_STRICT)
    b = None
    for numbers in (first, second):
        reads = [K.reads[r] for r in numbers]
        cat, offs = O.pack_reads(reads)
        if b is None:
            b = P.Batch(idx, cat, offs)
        else:
            b.upload(cat, offs)
        b.run(C.MIN_LEN, 1, P.RUN_TAGS)
        v, a, w = _stages(b, 31, 1, 4)
        _replay(reads, texts, a, w, 31, numbers)
        assert (a["reads"]["seq"] != G.NO_SEQUENCE).all()
    b.free()
    idx.close()
    assert len(first) == 68 and len(second) == 300


def _gaf(out, *args):
    r = subprocess.run([CLI] + [str(x) for x in args] + ["--gaf", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    text = open(out, "rb").read().decode()
    assert text.endswith("\n") or text == ""
    return text.split("\n")[:-1]


def test_the_cli_on_the_walk_graph(world, tmp_path):
    ri, tags, texts = world
    reads = [r for r in K.reads if r]  # (a line file cannot hold the empty read)
    path = str(tmp_path / "replay_reads.txt")
    with open(path, "wb") as f:
        f.write(b"".join(r + b"\n" for r in reads))
    plain = _gaf(str(tmp_path / "plain.gaf"), ri, tags, path, C.MIN_LEN, 1, "--mode", "strict", "--align-band", 31)
    small = _gaf(str(tmp_path / "small.gaf"), ri, tags, path, C.MIN_LEN, 1, "--mode", "strict", "--align-band", 31, "--batch", 64, "--streams", 2, "--format", "device",
                 "--device-parse")
    assert len(plain) == len(reads) == N - 1
    stars = 0
    for i, (line, read) in enumerate(zip(plain, reads)):
        stars += G.replay_gaf_line(line, read, K.node_seq, texts=texts, number=i + 1) is None
    assert small == plain
    none = [i for i, kind in enumerate(K.kind[r] for r in range(N) if K.reads[r]) if kind == "none"]
    assert stars >= len(none) and all("*" in plain[i] for i in none) and len(plain) - stars >= 500
    print("%d GAF lines replayed, %d of them * lines" % (len(plain), stars))


@pytest.mark.parametrize("reads_file", ["reads.txt", "test_reads.txt"])
def test_the_cli_on_the_golden_xy(golden, tmp_path, reads_file):
    bt = os.path.join(golden, "bidirectional_test")
    ri, tags = os.path.join(bt, "xy.ri"), os.path.join(bt, "xy_bidirectional_compressed.tags")
    g, seqs, first_id = GG.parse_graph(os.path.join(bt, "xy.gbz"))
    node_seq = {first_id + k: bytes(s) for k, s in enumerate(seqs)}
    reads = [l for l in open(os.path.join(bt, reads_file), "rb").read().split(b"\n") if l]
    idx = P.Index(ri, tags)
    texts = idx.text()[1].split(b"\n")[:-1]
    idx.close()
    placed = 0
    for extra in ([], ["--align-band", 31, "--verify-max", 16, "--verify-mismatch", 1], ["--align-band", 0]):
        lines = _gaf(str(tmp_path / "xy.gaf"), ri, tags, os.path.join(bt, reads_file), 3, 1, *extra)
        assert len(lines) == len(reads)
        for i, (line, read) in enumerate(zip(lines, reads)):
            placed += G.replay_gaf_line(line, read, node_seq, texts=texts, number=i + 1) is not None
    assert placed >= 3
    print("%s: %d lines with a path replayed" % (reads_file, placed))
