"""Pure-Python restatement of the read pack -- TEST INFRASTRUCTURE ONLY.

The definitions of include/pgx.h "read pack" as plain loops over reads, operations and text positions: the node table from the visits, the graph
base under every text position by stepping through the path visit by visit, and the coverage counted base by base.  No difference array, no
prefix sum, no rank: what the kernels do in two atomics a stretch is done here one base at a time.

MUTATIONS names the deliberate mistakes `mut` switches on; tests/test_pack_cpu.py shows a case that trips each."""
import numpy as np

NO_SEQUENCE = 0xFFFFFFFF
OP_I, OP_D, OP_S, OP_EQ, OP_X = 1, 2, 4, 7, 8
MUTATIONS = ("d_counted", "i_consumes", "rev_off_by_one", "base_inclusive", "x_not_counted", "filter_strict")


class FormatError(Exception):
    """two visits of one id with different lengths (PGX_ERR_FORMAT); .node is the smallest such id"""

    def __init__(self, node):
        super().__init__("the tags do not describe whole-node paths: node %d" % node)
        self.node = node


def node_table(path_nodes, visit_length, mut=None):
    """(node_length uint32[n_nodes], node_base uint64[n_nodes + 1]) with n_nodes = max_id + 1, 0 without a visit"""
    if len(path_nodes) == 0:
        return np.zeros(0, np.uint32), np.zeros(1, np.uint64)
    max_id = max(int(v) >> 1 for v in path_nodes)
    length = [0] * (max_id + 1)
    bad = []
    for v, ln in zip(path_nodes, visit_length):
        i = int(v) >> 1
        if length[i] and length[i] != int(ln):
            bad.append(i)
        length[i] = length[i] or int(ln)
    if bad:
        raise FormatError(min(bad))
    base, total = [], 0
    for i in range(max_id + 1):
        if mut == "base_inclusive":
            total += length[i]
            base.append(total)
        else:
            base.append(total)
            total += length[i]
    base.append(total)
    return np.array(length, dtype=np.uint32), np.array(base, dtype=np.uint64)


def graph_bases(nodes, lengths, node_length, node_base, mut=None):
    """the graph base under every offset of a sequence stated as its visits, stepping through the path visit by visit"""
    out = []
    for v, ln in zip(nodes, lengths):
        i, full = int(v) >> 1, int(node_length[int(v) >> 1])
        for d in range(int(ln)):
            o = d if not int(v) & 1 else (full - d if mut == "rev_off_by_one" else full - 1 - d)
            out.append(int(node_base[i]) + o)
    return out


def read_pack(path_offsets, path_nodes, visit_length, seq, text_start, op_offsets, ops, keep=None, mapq=None, min_mapq=0, text_end=None, mut=None):
    """what pgx_read_pack_arrays / pgx_pack_finish return.  keep: the arrays route's filter; mapq + min_mapq: the batch route's; text_end: the batch
    route's align records say where a read ends (None: text_start plus what the operations consume)"""
    node_length, node_base = node_table(path_nodes, visit_length, mut)
    n_nodes, G = len(node_length), int(node_base[-1])
    cov = [0] * (G + (1024 if mut else 0))  # (a mutation may point behind the graph: room to show it instead of an IndexError)
    counted = filtered = added = 0
    bases_of = {}  # sequence -> graph_bases, made once a sequence
    for r in range(len(seq)):
        q = int(seq[r])
        if q == NO_SEQUENCE:
            continue
        words = [int(x) for x in ops[int(op_offsets[r]):int(op_offsets[r + 1])]]
        if text_end is not None:
            placed = int(text_end[r]) > int(text_start[r])
        else:
            placed = sum(w >> 4 for w in words if w & 15 in (OP_D, OP_EQ, OP_X)) > 0
        if not placed:
            continue
        if keep is not None and not int(keep[r]):
            filtered += 1
            continue
        if mapq is not None and min_mapq != 0 and not (int(mapq[r]) > min_mapq if mut == "filter_strict" else int(mapq[r]) >= min_mapq):
            filtered += 1
            continue
        counted += 1
        a, b = int(path_offsets[q]), int(path_offsets[q + 1])
        if q not in bases_of:
            bases_of[q] = graph_bases(path_nodes[a:b], visit_length[a:b], node_length, node_base, mut)
        under = bases_of[q]
        t = int(text_start[r])
        for w in words:
            op, ln = w & 15, w >> 4
            if op in (OP_S, OP_I):
                if op == OP_I and mut == "i_consumes":
                    t += ln
                continue
            adds = op in (OP_EQ, OP_X) if mut != "x_not_counted" else op == OP_EQ
            if op == OP_D and mut == "d_counted":
                adds = True
            for p in range(t, t + ln):
                if adds:
                    cov[under[p]] += 1
            if op in (OP_EQ, OP_X):
                added += ln
            t += ln
        if text_end is not None and mut is None:
            assert t == int(text_end[r]), (r, t, int(text_end[r]))
    cov = [c & 0xFFFFFFFF for c in cov]
    covered, total, most = [], [], []
    for i in range(n_nodes):
        part = cov[int(node_base[i]):int(node_base[i]) + int(node_length[i])]
        covered.append(sum(1 for c in part if c))
        total.append(sum(part))
        most.append(max(part) if part else 0)
    return dict(n_nodes=n_nodes, n_bases=G, node_base=node_base, node_length=node_length, cov=np.array(cov[:G] if not mut else cov, dtype=np.uint32),
                covered=np.array(covered, dtype=np.uint32), sum=np.array(total, dtype=np.uint64), max=np.array(most, dtype=np.uint32),
                reads_counted=counted, reads_filtered=filtered, bases_added=added)


def same(got, exp):
    """byte for byte: the table, the vector, the summary and the counters"""
    assert (got["n_nodes"], got["n_bases"]) == (exp["n_nodes"], exp["n_bases"])
    for k in ("node_base", "node_length", "cov", "covered", "sum", "max"):
        bad = np.flatnonzero(np.asarray(got[k]) != np.asarray(exp[k])) if len(got[k]) == len(exp[k]) else None
        assert got[k].dtype == exp[k].dtype and got[k].tobytes() == exp[k].tobytes(), (k, None if bad is None else (len(bad), int(bad[0]), got[k][bad[0]], exp[k][bad[0]]))
    for k in ("reads_counted", "reads_filtered", "bases_added"):
        assert got[k] == exp[k], (k, got[k], exp[k])


def summary_of(node_base, node_length, cov):
    """(covered, sum, max) per node from a coverage vector: what find_mems does after summing the vectors of several devices"""
    covered, total, most = [], [], []
    for i in range(len(node_length)):
        part = [int(c) for c in cov[int(node_base[i]):int(node_base[i]) + int(node_length[i])]]
        covered.append(sum(1 for c in part if c)); total.append(sum(part)); most.append(max(part) if part else 0)
    return covered, total, most
