"""Case tables of build_tags (test_build_tags_cases.py on the CPU, test_gpu_build_tags_borders.py on the GPU): text collections and graphs
stated as pgx_build_tags_paths takes them, that put node starts and sequence ends on the borders of the 1024-position directory
(path_tables in pgx_tools.hip, the search of pgx_bt_tag_kernel), run lengths on the borders of the 511-row piece and of the reference's
16-bit counter, node ids on every border of the ByteCode width up to the 44-bit bound, and the row, sequence and run counts on the
borders of the 256-lane row kernels, the 2048-item scan blocks and the 4096-item one-pass tiles.

pgx_build_tags_paths takes node lengths, not node sequences: a text is random ACGT and the cut into nodes is free, so every border is
placed exactly.  Every path node has an id of its own unless a table says otherwise, ids start at 1 unless a table says otherwise, and
the orientation bit alternates along the node list, so both orientations occur in every table.

From first principles, as in test_gpu_build_tags.py: the oracle's suffix array of the CPU-built index, then gbz_graph_emu.row_tags ->
runs -> encode.  The CPU file asserts that every table holds what its line claims."""
import os

import numpy as np

import build_device_cases as BC
import gbz_graph_emu as E
import merge_cases as M
import pgx_ffi as P

BUCKET = 1024          # text positions per directory entry; also the longest node (10 offset bits)
MAX_PIECE = 511        # longest piece of a run (length_bits = 9)
ROW_BLOCK = 256        # lanes per block of every pgx_bt_* kernel
SCAN_BLOCK = 2048      # items per block of the blocked scans
SCAN_TILE = BC.SCAN1_TILE_ITEMS  # items per tile of the one-pass scan
ID_BITS = 44           # a piece holds node << 20 in 64 bits
REFERENCE_RUNS = P.BUILD_TAGS_REFERENCE_RUNS

_U = np.uint64


class Case:
    """text, path_offsets, path_nodes, node_length, first_node_id, flags, what; build_case adds the index and the truth"""


def graph_from_cuts(cuts, first_node_id=1, holes=()):
    """(path_offsets, path_nodes, node_length): sequence s is cut into nodes of the lengths cuts[s]; every path node gets the next id from
    first_node_id on, except that `holes` ids (counted from first_node_id) stay without a sequence; orientation bits alternate along the list"""
    po, pn, nl, k = [0], [], [], 0
    for cut in cuts:
        for ln in cut:
            while len(nl) in holes:
                nl.append(0)
            pn.append(((first_node_id + len(nl)) << 1) | (k & 1))
            nl.append(int(ln))
            k += 1
        po.append(len(pn))
    return np.array(po, dtype=_U), np.array(pn, dtype=_U), np.array(nl, dtype=np.uint32)


def make_case(text, po, pn, nl, first_node_id, what, flags=0, **claims):
    c = Case()
    c.text, c.path_offsets, c.path_nodes, c.node_length, c.first_node_id, c.flags, c.what = text, po, pn, nl, first_node_id, flags, what
    c.claims = claims
    return c


def node_starts(c):
    """per sequence: the start of every path node within it, and the sequence's length -- a plain loop, no cumsum"""
    out = []
    for s in range(len(c.path_offsets) - 1):
        st, pos = [], 0
        for k in range(int(c.path_offsets[s]), int(c.path_offsets[s + 1])):
            st.append(pos)
            pos += int(c.node_length[(int(c.path_nodes[k]) >> 1) - c.first_node_id])
        out.append((st, pos))
    return out


def naive_row_tags(c):
    """the tag of every row stated naively: walk the path of the row's sequence node by node until the node that covers the offset"""
    out = np.zeros(c.n, dtype=_U)
    for i in range(c.n_seq, c.n):
        s, off = int(c.sa[i]) // c.ml, int(c.sa[i]) % c.ml
        pos = 0
        for k in range(int(c.path_offsets[s]), int(c.path_offsets[s + 1])):
            node = int(c.path_nodes[k])
            ln = int(c.node_length[(node >> 1) - c.first_node_id])
            if off < pos + ln:
                out[i] = ((node >> 1) << 11) | ((node & 1) << 10) | (off - pos)
                break
            pos += ln
        else:
            raise AssertionError("row %d: offset %d beyond the path of sequence %d" % (i, off, s))
    return out


# ---- 1. the directory: one collection that holds every border
LAYOUT_A = [1, 1024, 1024, 1023] + [1] * 1024 + [1023, 1, 1, 1024]  # starts 0 1 1025 2049 3072..4095 4096 5119 5120 5121; 6145 bp
LAYOUT_B = [1024] + [1] * 1024 + [1023, 1024, 1]                    # starts 0 1024..2047 2048 3071 4095; 4096 bp
DIRECTORY_CUTS = [
    [],                  # an empty sequence first
    [1],
    [1023],
    [1024],
    [1024, 1],
    [],                  # ... in the middle
    [1, 1024],
    [1023, 1024],        # a 1024-bp node last, from 1024 - 1 on
    [1024, 1024],
    [1024, 1, 1024],
    [1024, 1024, 1024],
    LAYOUT_A,
    LAYOUT_B,
    [],                  # ... and last
]
DIRECTORY_HOLES = (0, 5, 6, 1040)  # ids without a sequence, the first id among them
DIRECTORY_LENGTHS = (1, 1023, 1024, 1025, 2047, 2048, 2049, 3072)


def _directory(name):
    rng = np.random.default_rng(1024)
    text = b"".join(BC._rand(rng, sum(cut)) + b"\n" for cut in DIRECTORY_CUTS)
    po, pn, nl = graph_from_cuts(DIRECTORY_CUTS, 1, DIRECTORY_HOLES)
    return make_case(text, po, pn, nl, 1, DIRECTORY_CASES[name]["what"])


DIRECTORY_CASES = {"directory": dict(what="sequences of 1, 1023, 1024, 1025, 2047, 2048, 2049 and 3072 bp; node starts on 1024 k - 1, 1024 k and "
                                          "1024 k + 1; a 1024-bp node from offset 1; buckets of 1024 one-bp nodes, one behind a 1024-bp node; a 1024-bp "
                                          "node last; in-node offset 1023 on both orientations; empty sequences first, in the middle and last")}


# ---- 2. run lengths: groups of L identical sequences, every group one node of its own
GROUP_LENGTHS = (1, 2, 510, 511, 512, 1021, 1022, 1023, 1533)
WRAP_LENGTHS = (65535, 65536, 65537)
# the 4-mers of the three groups: in suffix order the runs of the middle group (GTG, TG) lie between runs of the last group (GAT < GTG < T < TG < TGAT)
WRAP_MERS = (b"ACCA", b"CGTG", b"TGAT")
RUN_CASES = {
    "pieces": dict(what="groups of 1, 2, 510, 511, 512, 1021, 1022, 1023 and 1533 identical 6-mers and one empty sequence: the runs have exactly these lengths"),
    "ends_in_long_run": dict(what="512 copies of TTTT behind three other groups: the last 512 rows of the BWT are one run, written as 511 + 1"),
    "wrap": dict(what="groups of 65 535, 65 536 and 65 537 identical 4-mers: reference mode keeps the first, drops the second between two runs that stay, "
                      "leaves 1 of the third", flags=REFERENCE_RUNS),
    "wrap_between_equal": dict(what="65 536 copies of ACG between ACA and ACT, which share their first node: in reference mode the run that vanishes "
                                    "leaves two runs of one value side by side", flags=REFERENCE_RUNS),
}


def _groups(groups, empty_at):
    """groups = [(sequence, copies)]; one node per group; one empty sequence in front of group `empty_at`"""
    text, po, pn = [], [0], []
    for g, (seq, copies) in enumerate(groups):
        if g == empty_at:
            text.append(b"\n")
            po.append(len(pn))
        text.append((seq + b"\n") * copies)
        pn += [((1 + g) << 1) | (g & 1)] * copies
        po += list(range(po[-1] + 1, po[-1] + copies + 1))
    nl = np.array([len(seq) for seq, _ in groups], dtype=np.uint32)
    return b"".join(text), np.array(po, dtype=_U), np.array(pn, dtype=_U), nl


def distinct_mers(count, k, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        m = BC._rand(rng, k)
        if m not in out:
            out.append(m)
    return out


def _run_case(name):
    k = RUN_CASES[name]
    if name == "pieces":
        text, po, pn, nl = _groups(list(zip(distinct_mers(len(GROUP_LENGTHS), 6, 511), GROUP_LENGTHS)), 4)
    elif name == "ends_in_long_run":
        text, po, pn, nl = _groups([(b"ACGTCA", 3), (b"GATC", 600), (b"CCAG", 1), (b"TTTT", 512)], 1)
    elif name == "wrap":
        text, po, pn, nl = _groups(list(zip(WRAP_MERS, WRAP_LENGTHS)), 1)
    else:
        # nodes 1 = AC, 2 = A, 3 = T, 4 = ACG; paths ACA = [1, 2-], ACG = [4] 65 536 times, ACT = [1, 3-]
        text = b"ACA\n" + b"ACG\n" * 65536 + b"ACT\n"
        pn = np.array([1 << 1, (2 << 1) | 1] + [4 << 1] * 65536 + [1 << 1, (3 << 1) | 1], dtype=_U)
        po = np.concatenate(([0], 2 + np.arange(65537), [65540])).astype(_U)
        nl = np.array([2, 1, 1, 3], dtype=np.uint32)
    return make_case(text, po, pn, nl, 1, k["what"], k.get("flags", 0))


# ---- 3. node ids: one 16-symbol sequence of four 4-bp nodes, ids first .. first + 3
ID_BORDERS = (8, 15, 22, 29, 36, 43)  # node << 20 has 20 + k bits below node 2^k, a multiple of 7: (20 + k) / 7 bytes a piece there, one more from 2^k on
NODE_ID_CASES = {"ids_from_1": dict(first=1, bytes=(3, 4), what="ids 1 to 4: a piece takes 3 bytes for node 1 and 4 from node 2 on")}
for _k in ID_BORDERS:
    _b = (20 + _k) // 7
    NODE_ID_CASES["ids_around_2_%d" % _k] = dict(first=(1 << _k) - 2, bytes=(_b, _b + 1),
                                                 what="ids 2^%d - 2 to 2^%d + 1: %d and %d bytes a piece" % (_k, _k, _b, _b + 1))
NODE_ID_CASES["ids_up_to_2_44"] = dict(first=(1 << ID_BITS) - 4, bytes=(10,), what="ids 2^44 - 4 to 2^44 - 1, the largest a piece holds: 10 bytes")
REFUSED_ID = 1 << ID_BITS
REFUSED_FIRST = REFUSED_ID - 3  # the refused id is the last of the four


def node_id_text():
    return BC._rand(np.random.default_rng(44), 16) + b"\n"


def node_id_graph(first):
    po, pn, nl = graph_from_cuts([[4, 4, 4, 4]], first)
    return po, pn, nl


def _node_id_case(name):
    k = NODE_ID_CASES[name]
    po, pn, nl = node_id_graph(k["first"])
    return make_case(node_id_text(), po, pn, nl, k["first"], k["what"], bytes=k["bytes"])


# ---- 4. sizes: every symbol a 1-bp node of its own id, so every row is a run (held twice: every run has two rows)
BORDERS = tuple(b + d for b in (ROW_BLOCK, SCAN_BLOCK, SCAN_TILE) for d in (-1, 0, 1))
SIZE_CASES = {}
for _m in BORDERS:
    SIZE_CASES["runs_%d" % _m] = dict(m=_m, n_seq=3, twice=False, what="%d rows behind the endmarkers, as many runs, 3 sequences" % _m)
for _s in (255, 256, 257):
    SIZE_CASES["seqs_%d" % _s] = dict(m=600, n_seq=_s, twice=False, what="600 symbols in %d sequences, many of them empty" % _s)
for _n, _s in ((2048, 8), (4096, 7)):
    SIZE_CASES["rows_%d" % _n] = dict(m=_n - _s, n_seq=_s, twice=False, what="%d rows in all, %d of them endmarkers" % (_n, _s))
for _r in (255, 256, 257, 2048, 4096, 4097):
    SIZE_CASES["twice_%d" % _r] = dict(m=_r, n_seq=6, twice=True, what="%d runs of two rows: 3 sequences, each held twice on the same nodes" % _r)


def _size_case(name):
    k = SIZE_CASES[name]
    m, n_seq = k["m"], k["n_seq"]
    rng = np.random.default_rng(7 * m + n_seq)
    distinct = n_seq // 2 if k["twice"] else n_seq
    cuts = np.sort(rng.integers(0, m + 1, size=distinct - 1))
    lens = np.diff(np.concatenate(([0], cuts, [m]))).tolist()
    po, pn, nl = graph_from_cuts([[1] * ln for ln in lens], 1)
    seqs = [BC._rand(rng, ln) for ln in lens]
    if k["twice"]:  # the two copies side by side: equal suffixes are ordered by sequence number, so nothing sorts between them
        seqs = [x for x in seqs for _ in range(2)]
        paths = [pn[int(po[s]):int(po[s + 1])] for s in range(distinct) for _ in range(2)]
        pn = np.concatenate(paths)
        po = np.concatenate(([0], np.cumsum([len(p) for p in paths]))).astype(_U)
    return make_case(b"".join(x + b"\n" for x in seqs), po, pn, nl, 1, k["what"])


TABLES = {"directory": (DIRECTORY_CASES, _directory), "runs": (RUN_CASES, _run_case), "node_ids": (NODE_ID_CASES, _node_id_case),
          "sizes": (SIZE_CASES, _size_case)}
ALL_CASES = [(t, n) for t, (cases, _) in TABLES.items() for n in cases]


def build_case(workdir, table, name):
    """the case with its index (.ri, by the CPU builder) and its truth from the oracle's suffix array: .sa, .ml, .n, .n_seq, .tags (one per
    row), .values / .lengths (the maximal runs), .ref_values / .ref_lengths (as PGX_BUILD_TAGS_REFERENCE_RUNS writes them)"""
    c = TABLES[table][1](name)
    c.table, c.name = table, name
    c.ri, c.rw, c.sa, c.ml = M.index_of(os.path.join(workdir, "build_tags_cases"), c.text)
    c.n, c.n_seq = len(c.text), c.text.count(b"\n")
    assert len(c.sa) == c.n and len(c.path_offsets) == c.n_seq + 1
    c.tags = E.row_tags(c.sa, c.n_seq, c.ml, c.path_offsets, c.path_nodes, c.node_length, c.first_node_id)
    c.values, c.lengths = E.runs(c.tags, c.n_seq)
    c.ref_values, c.ref_lengths = E.reference_runs(c.values, c.lengths)
    return c


def pieces(values, lengths):
    """(value, rows) of every piece of the file: 511 while 512 rows or more are left, then the rest -- the rule stated once more, apart
    from gbz_graph_emu.encode, so the CPU tier can hold the two together"""
    out = []
    for v, ln in zip(values.tolist(), lengths.tolist()):
        while ln >= 512:
            out.append((v, MAX_PIECE))
            ln -= MAX_PIECE
        if ln:
            out.append((v, ln))
    return out


def piece_bytes(value, rows):
    """ByteCode bytes of one piece: 7 bits a byte of offset:10 | rev:1 | rows:9 | node << 20"""
    code = (value & 0x7FF) | (rows << 11) | ((value >> 11) << 20)
    return max(1, -(-code.bit_length() // 7))
