"""Case tables of merge_tags (test_merge_cases.py on the CPU, test_gpu_merge_borders.py on the GPU): text collections, sequence -> file maps
and per-file tag streams that put the BWT size, a file's tag count and a stream's run count on the borders of the 256-thread row kernels
(pgx_mt_*_kernel) and of the 4096-item scan tile, that use file ids up to 249 in no order, files without tags, all four stream containers,
tags above 2^44, rows that join the endmarker run, and a merged run of more than 65 536 rows fed by two files.

From first principles, as in test_merge_tags.py: every suffix (sequence s, offset o) gets a tag tagf(s, o, first symbol); file f's stream is
tagf along the suffix array of f's own text, the expectation is tagf along the whole-genome suffix array (0 on the endmarker block).  The CPU
file asserts that every table holds what it claims and that the reference's sequential procedure gives the expectation."""
import hashlib
import os

import numpy as np

import build_device_cases as BC
import oracle_ffi as O
import pgx_ffi as P
import pgx_workload as W

ROW_BLOCK = 256        # threads per block of pgx_mt_file_of / expand / gather / flags / compact
SCAN_TILE = BC.SCAN1_TILE_ITEMS  # PGX_SCAN1_TILE_ITEMS: rows per tile of the one-pass scan (modes 3 and 4)
MAX_PIECE = 511        # longest run of the stream format (length_bits = 9)
CONTAINERS = ("bare", "header", "padded", "zero_runs")
REFERENCE_RUNS = P.MERGE_REFERENCE_RUNS

_U = np.uint64


# ---- tag functions: (global sequence, offset, first symbol of the suffix) -> node << 11 | rev << 10 | offset, all numpy arrays
def fine(seq, off, first):
    """_g of test_merge_tags.py: the node from a coarse offset bucket; short runs"""
    seq, off = seq.astype(_U), off.astype(_U)
    node = _U(1) + off // _U(5) + _U(1000) * (seq // _U(4))
    return (node << _U(11)) | ((seq & _U(1)) << _U(10)) | (off % _U(5))


def coarse(seq, off, first):
    """_by_first_symbol of test_merge_tags.py: the A, C and G ranges of the BWT are one run, whatever file a row belongs to"""
    acg = (first == ord("A")) | (first == ord("C")) | (first == ord("G"))
    return np.where(acg, _U((9 << 11) | 3), _U((17 << 11) | (1 << 10) | 5)).astype(_U)


def wide(seq, off, first):
    """fine with 2^33 added to the node: every tag is above 2^44, so a 32-bit narrowing anywhere loses it"""
    return fine(seq, off, first) + _U(1 << 44)


def zero_first(seq, off, first):
    """0 for every suffix that starts with A (the first rows behind the endmarker block, which carries 0 too), else fine"""
    return np.where(first == ord("A"), _U(0), fine(seq, off, first)).astype(_U)


TAGF = {"fine": fine, "coarse": coarse, "wide": wide, "zero_first": zero_first}


# ---- streams
def bytecode(v):
    out = bytearray()
    while v > 0x7F:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def expected_runs(tags):
    """maximal runs of an array: (values, lengths)"""
    t = np.asarray(tags, dtype=_U)
    if not len(t):
        return np.zeros(0, dtype=_U), np.zeros(0, dtype=_U)
    starts = np.concatenate(([0], np.flatnonzero(t[1:] != t[:-1]) + 1))
    return t[starts], np.diff(np.concatenate((starts, [len(t)]))).astype(_U)


def stream_runs(tags, piece=MAX_PIECE):
    """the runs build_tags' writer emits, as _write_algorithm_tags of test_merge_tags.py cuts them: maximal runs in pieces of at most `piece`"""
    assert 1 <= piece <= MAX_PIECE
    vals, lens = expected_runs(tags)
    out = []
    for v, ln in zip(vals.tolist(), lens.tolist()):
        while ln > piece:
            out.append((v, piece))
            ln -= piece
        out.append((v, ln))
    return out


def encode_run(v, ln):
    """offset:10 | rev:1 | len:9 | node << 20"""
    return bytecode((v & 0x7FF) | (ln << 11) | ((v >> 11) << 20))


# zero-length runs of the zero_runs container: one with a node and an offset, the bare zero byte, one with the rev bit
ZERO_RUNS = (encode_run((77 << 11) | 5, 0), b"\x00", encode_run((12345 << 11) | (1 << 10), 0))


def stream_body(tags, container, piece=MAX_PIECE):
    """the ByteCodes of one file, without header or padding"""
    codes = [encode_run(v, ln) for v, ln in stream_runs(tags, piece)]
    if container == "zero_runs" and codes:
        codes = [ZERO_RUNS[0]] + codes[:len(codes) // 2] + [ZERO_RUNS[1]] + codes[len(codes) // 2:] + [ZERO_RUNS[2]]
    return b"".join(codes)


def stream_file(body, container):
    """the file of a body.  An empty stream is a 0-byte file, under `header` a header of eight zero bytes."""
    assert container in CONTAINERS
    if container == "header" or (container == "padded" and body):
        pad = b"\0" * (-len(body) % 8) if container == "padded" else b""
        return np.uint64(len(body) * 8).tobytes() + body + pad  # int_vector<8> header of sdsl::int_vector_buffer<8>: the bit count
    return body


def tags_start(raw):
    """algorithm_tags_start (pgx_tools.hip) restated: 8 behind a header that states the body's bits, exactly or zero-padded to whole words; else 0"""
    if len(raw) < 8:
        return 0
    bits = int(np.frombuffer(raw[:8], dtype=np.uint64)[0])
    body = len(raw) - 8
    if bits == body * 8:
        return 8
    return 8 if bits % 8 == 0 and bits // 8 < body and (bits // 8 + 7) // 8 * 8 == body else 0


def decode_runs(raw, at=0):
    """(value, length) of every ByteCode from byte `at` on, zero-length ones included"""
    out, i = [], at
    while i < len(raw):
        v, sh = 0, 0
        while True:
            b = raw[i]
            i += 1
            v |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                break
        out.append(((v & 0x7FF) | ((v >> 20) << 11), (v >> 11) & 0x1FF))
    return out


# ---- indexes and suffix arrays (one build per text and session)
_built = {}


def index_of(workdir, text):
    """(path of the r-index, oracle handle, suffix array as int64 sequence * max_length + offset, max_length) of a text, by the CPU builder"""
    key = hashlib.sha1(text).hexdigest()[:16]
    if key not in _built:
        os.makedirs(workdir, exist_ok=True)
        tp = os.path.join(workdir, "t_%s.txt" % key)
        with open(tp, "wb") as f:
            f.write(text)
        ri = os.path.join(workdir, "t_%s.ri" % key)
        P.build_index_from_text(tp, None, ri)
        r = O.RIndex(ri)
        _built[key] = (ri, r, r.decompress_sa().astype(np.int64), int(r.max_length))
    return _built[key]


def sequence_starts(text):
    """text position of the first symbol of every sequence, and the number of sequences"""
    t = np.frombuffer(text, dtype=np.uint8)
    assert len(t) and t[-1] == 10
    nl = np.flatnonzero(t == 10)
    return np.concatenate(([0], nl[:-1] + 1)).astype(np.int64), len(nl)


def tags_along(tagf, sa, ml, n_seq, starts, text, global_of=None):
    """tagf along the non-endmarker rows of a suffix array; global_of maps its sequence numbers to those tagf speaks of"""
    t = np.frombuffer(text, dtype=np.uint8)
    seq, off = sa[n_seq:] // ml, sa[n_seq:] % ml
    first = t[starts[seq] + off]
    assert not (first == 10).any()  # the endmarker block is exactly [0, n_seq)
    return tagf(seq if global_of is None else global_of[seq], off, first)


class Case:
    pass


_made = []  # (one stream directory per make_case call)


def make_case(workdir, text, seq_to_file, n_files, tagf, container, piece=MAX_PIECE):
    """files and expectation of one merge: .ri the whole-genome index, .tag_paths the n_files streams, .seq_to_file, .expected the n tags,
    and what the CPU tier checks: .file_tags (every file's tags in its stream's order), .bodies (its ByteCodes), .sa / .ml / .starts"""
    c = Case()
    c.text, c.n, c.n_files, c.container, c.piece = text, len(text), n_files, container, piece
    c.seq_to_file = np.asarray(seq_to_file, dtype=np.uint32)
    c.starts, c.n_seq = sequence_starts(text)
    assert len(c.seq_to_file) == c.n_seq and int(c.seq_to_file.max()) < n_files
    c.ri, c.rw, c.sa, c.ml = index_of(workdir, text)
    assert len(c.sa) == c.n
    c.expected = np.concatenate((np.zeros(c.n_seq, dtype=_U), tags_along(tagf, c.sa, c.ml, c.n_seq, c.starts, text)))
    ends = np.concatenate((c.starts[1:], [c.n]))
    c.tag_paths, c.file_tags, c.bodies = [], [], []
    _made.append(None)
    tag_dir = os.path.join(workdir, "streams_%d" % len(_made))
    os.makedirs(tag_dir, exist_ok=True)
    for f in range(n_files):
        own = np.flatnonzero(c.seq_to_file == f)  # ascending global ids = the file's local sequence numbers
        tags = np.zeros(0, dtype=_U)
        if len(own) and int((ends[own] - c.starts[own]).sum()) > len(own):  # (only empty sequences: no suffix but the endmarkers, no tag)
            own_text = b"".join(text[c.starts[s]:ends[s]] for s in own)
            _, _, sa_f, ml_f = index_of(workdir, own_text)
            st_f, n_f = sequence_starts(own_text)
            assert n_f == len(own)
            tags = tags_along(tagf, sa_f, ml_f, n_f, st_f, own_text, global_of=own)
        body = stream_body(tags, container, piece)
        p = os.path.join(tag_dir, "file_%03d.algo.tags" % f)
        with open(p, "wb") as fh:
            fh.write(stream_file(body, container))
        c.tag_paths.append(p)
        c.file_tags.append(tags)
        c.bodies.append(body)
    return c


def reference_runs(values, lengths):
    """what MERGE_REFERENCE_RUNS writes: lengths mod 65 536, zeros dropped"""
    l16 = lengths & _U(0xFFFF)
    return values[l16 != 0], l16[l16 != 0]


def split511(values, lengths):
    """the pieces of the compact file (append_compact_run_streamed): 511 while the rest is 512 or more, then the rest"""
    out = []
    for v, ln in zip(values.tolist(), lengths.tolist()):
        while ln >= 512:
            out.append((v, 511))
            ln -= 511
        if ln:
            out.append((v, ln))
    return out


# ---- the tables: name -> dict(text=.., s2f=.., n_files=.., tagf=.., container=.., piece=.., and what lies there)
def collection_from_lengths(lens, seed):
    """newline-terminated sequences over ACGT of exactly these lengths"""
    rng = np.random.default_rng(seed)
    return b"".join(BC._rand(rng, int(ln)) + b"\n" for ln in lens)


# 1. BWT size borders: two files, sequences dealt alternately, containers cycling.  (seed: the text's; chosen so that `padded` bodies are no
# multiple of 8 bytes -- test_merge_cases.py asserts it)
SIZE_N = (255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 65535, 65536, 65537)
SIZE_SEQS = 6
SIZE_SEED = {257: 100257, 8191: 108191}
SIZE_CASES = {}
for _i, _n in enumerate(SIZE_N):
    SIZE_CASES["n_%d" % _n] = dict(n=_n, container=CONTAINERS[_i % 4], seed=SIZE_SEED.get(_n, _n),
                                   what="%d rows: %s" % (_n, "one block of every row kernel" if _n < 4095 else "one tile of the scan, 16 row blocks"
                                                         if _n < 8191 else "two tiles" if _n < 65535 else "16 tiles"))


def _size_case(workdir, name):
    k = SIZE_CASES[name]
    text = BC.random_collection(k["n"], SIZE_SEQS, seed=k["seed"])
    return make_case(workdir, text, np.arange(SIZE_SEQS) % 2, 2, fine, k["container"])


# 2. file 0's tag count on the borders inside about 6000 rows; with piece = 1 its stream's run count (the grid of pgx_mt_expand_kernel) too
TOTAL_T = (255, 256, 257, 4095, 4096, 4097)
TOTAL_ROWS = 6000
TOTAL_SEED = {(257, MAX_PIECE): 107257}
TOTAL_CASES = {}
for _j, _piece in enumerate((MAX_PIECE, 1)):
    for _i, _t in enumerate(TOTAL_T):
        TOTAL_CASES["total_%d_piece_%d" % (_t, _piece)] = dict(total=_t, piece=_piece, container=CONTAINERS[(_i + _j) % 4],
                                                               seed=TOTAL_SEED.get((_t, _piece), 7000 + _t),
                                                               what="file 0 holds %d tags%s" % (_t, " in as many runs" if _piece == 1 else ""))


def total_lengths(t):
    """six sequence lengths: file 0 (even ids) owns t symbols, all six make TOTAL_ROWS rows"""
    rest = TOTAL_ROWS - 6 - t
    a, b = [t // 3, t // 3, t - 2 * (t // 3)], [rest // 3, rest // 3, rest - 2 * (rest // 3)]
    return [a[0], b[0], a[1], b[1], a[2], b[2]]


def _total_case(workdir, name):
    k = TOTAL_CASES[name]
    text = collection_from_lengths(total_lengths(k["total"]), k["seed"])
    return make_case(workdir, text, np.arange(6) % 2, 2, fine, k["container"], k["piece"])


# 3. file counts
MANY_FILES, MANY_SEQS = 250, 300


def many_files_map():
    """300 sequences over 250 files, neither grouped nor ascending: the first 250 reach every file once (7 is prime to 250)"""
    s = np.arange(MANY_SEQS)
    return np.where(s < MANY_FILES, (s * 7 + 3) % MANY_FILES, (s * 13 + 5) % MANY_FILES).astype(np.uint32)


def many_files_text():
    """sequences of 0 to 3 symbols; the first sequence of file 249 is not empty"""
    rng = np.random.default_rng(250)
    lens = rng.integers(0, 4, size=MANY_SEQS)
    lens[int(np.flatnonzero(many_files_map() == MANY_FILES - 1)[0])] = 3
    return collection_from_lengths(lens, 251)


def _idle_text():
    return BC.random_collection(3000, 7, seed=31)


def _empty_only():
    """seven sequences; 1, 3 and 6 are empty and are all that file 1 owns"""
    lens = [700, 0, 512, 0, 300, 900, 0]
    return collection_from_lengths(lens, 33), np.array([0, 1, 2, 1, 2, 0, 1], dtype=np.uint32)


FILE_CASES = {
    "one_file": dict(what="one file owns everything"),
    "files_250": dict(what="250 files, ids 0..249 in a fixed permutation pattern over 300 sequences of 0 to 3 symbols"),
    "idle_file_bare": dict(what="3 files, file 1 owns no sequence: a 0-byte stream"),
    "idle_file_header": dict(what="3 files, file 1 owns no sequence: a header of eight zero bytes"),
    "empty_only_bare": dict(what="3 files, file 1 owns only empty sequences: a 0-byte stream"),
    "empty_only_header": dict(what="3 files, file 1 owns only empty sequences: a header of eight zero bytes"),
}


def _file_case(workdir, name):
    if name == "one_file":
        return make_case(workdir, BC.random_collection(3000, 5, seed=30), np.zeros(5, dtype=np.uint32), 1, fine, "header")
    if name == "files_250":
        return make_case(workdir, many_files_text(), many_files_map(), MANY_FILES, fine, "header")
    container = name.rsplit("_", 1)[1]
    if name.startswith("idle_file"):
        return make_case(workdir, _idle_text(), np.array([0, 2, 2, 0, 2, 0, 0], dtype=np.uint32), 3, fine, container)
    text, s2f = _empty_only()
    return make_case(workdir, text, s2f, 3, fine, container)


# 4. interleaving: 4 files over the 16 sequences of a synthetic pangenome, every tag function once
INTERLEAVE_CASES = {
    "interleave_fine": dict(tagf="fine", container="padded", what="short runs, every file's rows scattered over the BWT"),
    "interleave_coarse": dict(tagf="coarse", container="zero_runs", what="runs that span files"),
    "interleave_wide": dict(tagf="wide", container="header", what="tags above 2^44"),
    "interleave_zero_first": dict(tagf="zero_first", container="bare", what="the first rows behind the endmarker block carry its value"),
}


def _synth(workdir, name, **kw):
    p = os.path.join(workdir, name)
    if not os.path.exists(p):
        os.makedirs(workdir, exist_ok=True)
        W.synth_pangenome_text(p, **kw)
    return open(p, "rb").read()


def interleave_text(workdir):
    return _synth(workdir, "interleave.txt", base_len=2000, n_hap=8, seed=404)


def _interleave_case(workdir, name):
    k = INTERLEAVE_CASES[name]
    return make_case(workdir, interleave_text(workdir), (np.arange(16) * 7) % 4, 4, TAGF[k["tagf"]], k["container"])


# 5. long runs: the `mtl` shape of test_merge_tags.py (two files, two haplotypes in both orientations of about 24 000 symbols each) under
# `coarse`: the A, C and G rows are one run of more than 65 536 rows that both files feed
LONG_CASES = {
    "long_piece_1": dict(piece=1, flags=0, what="every tag its own run in the streams"),
    "long_piece_511": dict(piece=MAX_PIECE, flags=0, what="runs of 511 in the streams"),
    "long_reference_runs": dict(piece=MAX_PIECE, flags=REFERENCE_RUNS, what="MERGE_REFERENCE_RUNS: lengths mod 65 536, zeros dropped"),
}


def long_text(workdir):
    return b"".join(_synth(workdir, "long_%d.txt" % c, base_len=24000 + 700 * c, n_hap=2, seed=200 + c, n_runs=1, n_run_len=(20, 60)) for c in range(2))


def _long_case(workdir, name):
    k = LONG_CASES[name]
    c = make_case(workdir, long_text(workdir), [0] * 4 + [1] * 4, 2, coarse, "bare", k["piece"])
    c.flags = k["flags"]
    return c


TABLES = {"size": (SIZE_CASES, _size_case), "total": (TOTAL_CASES, _total_case), "files": (FILE_CASES, _file_case),
          "interleave": (INTERLEAVE_CASES, _interleave_case), "long": (LONG_CASES, _long_case)}
ALL_CASES = [(t, n) for t, (cases, _) in TABLES.items() for n in cases]


def build_case(workdir, table, name):
    """the case with its name, table and flags; .want_values / .want_lengths are the runs the output file holds"""
    c = TABLES[table][1](os.path.join(workdir, "merge_cases"), name)
    c.name, c.table = name, table
    c.flags = getattr(c, "flags", 0)
    v, ln = expected_runs(c.expected)
    c.want_values, c.want_lengths = reference_runs(v, ln) if c.flags & REFERENCE_RUNS else (v, ln)
    return c
