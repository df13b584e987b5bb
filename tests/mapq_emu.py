"""Read mapq in plain Python: the definitions of include/pgx.h "read mapq" as loops over reads, entries and classes.

  entries       the list candidates of a read in list order, behind them the extras: the first min(max_extra, 64 - n_list) placements with
                cov == next_score > 0, verified like any candidate (candidates_with_extras, on top of place_emu / verify_emu results)
  chosen        the entry named by the winner's cand_index; none: a record of zeros
  anchor        seg_start of the chosen entry
  locus         of entry i, defined iff span_lo_i <= anchor < span_hi_i: (oriented node, offset in it) of text position diag_i + anchor of seq_i,
                found here by stepping through the visits of the sequence
  classes       equal defined loci; an entry without a locus is a class of its own
  adjacent      a class with an entry within 0 < |diag difference| <= slack of an entry of the chosen's class, on the same sequence
  score         seg_score; PAIRED: + the larger of (best compatible list candidate of the mate, solo_mate - U), 0 where the mate has no candidate
  excess        sum over the competing classes of T[min(49, scale * max(0, S_w - S_X))], plus the rescue terms
  mapq          the largest q in 0 .. 60 with E * K[q] <= (E + 65536) * 65536

T and K are computed here with exact integers (T[k]: the largest t with t^10 * 10^k <= 65536^10; K[q]: the largest v with v^10 <= 65536^10 * 10^q);
tests/test_mapq_cpu.py holds them against the literals of include/pgx.h.  Nothing here is shared with the library: the kernel spreads the entries
over lanes, shuffles and ballots; this file loops.  MUTATIONS are deliberate mistakes (tests/test_mapq_cpu.py says what each trips); the default is none."""
import numpy as np

import verify_emu as V

VERIFY_DTYPE = V.VERIFY_DTYPE
MAPQ_DTYPE = np.dtype([("mapq", "<u4"), ("flags", "<u4"), ("n_entries", "<u4"), ("n_loci", "<u4"), ("n_with", "<u4"), ("n_competing", "<u4"), ("best_other", "<u4"),
                       ("excess", "<u4")])
NO_SEQUENCE = 0xFFFFFFFF
NO_CHOSEN = 0xFFFFFFFF
HAS, LOCUS, PAIRED, RESCUED, CAPPED, OUTSCORED = 1, 2, 4, 8, 16, 32
RESCUE_RESCUED = 2  # the bit of a pgx_read_rescue record
MAX_ENTRIES = 64
U32 = 0xFFFFFFFF
MUTATIONS = ("class_seq_diag", "anchor_zero", "adj_no_seq", "weight_per_entry", "clamp_48", "solo_no_u", "no_rescue", "k_lt", "extras_best")


def _root_floor(target, power=10):
    """the largest v >= 0 with v ** power <= target"""
    lo, hi = 0, 1
    while hi ** power <= target:
        hi *= 2
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mid ** power <= target:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _t(k):
    lo, hi = 0, 65536
    while lo < hi:  # the largest t with t^10 * 10^k <= 65536^10
        mid = (lo + hi + 1) // 2
        if mid ** 10 * 10 ** k <= 65536 ** 10:
            lo = mid
        else:
            hi = mid - 1
    return lo


T = [_t(k) for k in range(50)]
K = [_root_floor(65536 ** 10 * 10 ** q) for q in range(61)]


def quality(excess, mutation=None):
    """mapq of an excess E"""
    q = 0
    for k in range(61):
        lhs, rhs = excess * K[k], (excess + 65536) * 65536
        if (lhs < rhs) if mutation == "k_lt" else (lhs <= rhs):
            q = k
    return q


def weight(scale, d, mutation=None):
    return T[min(48 if mutation == "clamp_48" else 49, scale * d)]


def locus(path_offsets, path_nodes, visit_length, seq, pos):
    """(node << 1 | rev, offset) of position pos of sequence seq, by stepping through its visits; None behind its end"""
    at = 0
    for k in range(int(path_offsets[seq]), int(path_offsets[seq + 1])):
        ln = int(visit_length[k])
        if at <= pos < at + ln:
            return int(path_nodes[k]), pos - at
        at += ln
    return None


def mate_term(seq_lengths, entry, mate_list, frag_min, frag_max, penalty, mutation=None):
    """m_i of an entry from the mate's list candidates"""
    if len(mate_list) == 0:
        return 0
    solo = max(int(c["seg_score"]) for c in mate_list)
    m = solo - (0 if mutation == "solo_no_u" else int(penalty))
    for c in mate_list:
        frag = int(seq_lengths[int(entry["seq"])]) - int(entry["diag"]) - int(c["diag"])
        if int(entry["seq"]) ^ 1 == int(c["seq"]) and frag_min <= frag <= frag_max:
            m = max(m, int(c["seg_score"]))
    return m


def mapq_read(tables, entries, n_list, chosen, scores, scale, slack, rescue=None, capped=False, paired=False, mutation=None):
    """the record of one read as a dict; scores: the score of every entry (seg_score, or the paired sum)"""
    zero = dict(mapq=0, flags=0, n_entries=0, n_loci=0, n_with=0, n_competing=0, best_other=0, excess=0)
    if chosen == NO_CHOSEN:
        return zero
    po, pn, vl = tables
    n = len(entries)
    anchor = 0 if mutation == "anchor_zero" else int(entries[chosen]["seg_start"])
    loci = []
    for e in entries:
        if mutation == "class_seq_diag":
            loci.append((int(e["seq"]), int(e["diag"])))
        elif int(e["span_lo"]) <= anchor < int(e["span_hi"]):
            loci.append(locus(po, pn, vl, int(e["seq"]), int(e["diag"]) + anchor))
        else:
            loci.append(None)
    # classes: lists of entry ordinals, in the order of their first entry
    classes = []
    for i in range(n):
        for c in classes:
            if loci[i] is not None and loci[c[0]] == loci[i]:
                c.append(i)
                break
        else:
            classes.append([i])
    mine = next(c for c in classes if chosen in c)
    s_w = scores[chosen]
    n_with, excess, others = len(mine), 0, []
    for c in classes:
        if c is mine:
            continue
        adjacent = any((mutation == "adj_no_seq" or int(entries[i]["seq"]) == int(entries[j]["seq"])) and 0 < abs(int(entries[i]["diag"]) - int(entries[j]["diag"])) <= slack
                       for i in c for j in mine)
        if adjacent:
            n_with += len(c)
            continue
        s_x = max(scores[i] for i in c)
        others.append(s_x)
        if mutation == "weight_per_entry":
            excess += sum(weight(scale, max(0, s_w - scores[i]), mutation) for i in c)
        else:
            excess += weight(scale, max(0, s_w - s_x), mutation)
    flags = HAS | (LOCUS if loci[chosen] is not None else 0) | (PAIRED if paired else 0) | (CAPPED if capped else 0) | (OUTSCORED if any(s > s_w for s in others) else 0)
    if rescue is not None and int(rescue["flags"]) & RESCUE_RESCUED and chosen == n_list - 1:
        flags |= RESCUED
        if mutation != "no_rescue":
            excess += (max(int(rescue["n_best"]), 1) - 1) * 65536
            if int(rescue["next_score"]) > 0:
                excess += weight(scale, max(0, int(rescue["seg_score"]) - int(rescue["next_score"])), mutation)
    return dict(mapq=quality(excess, mutation), flags=flags, n_entries=n, n_loci=len(classes), n_with=n_with, n_competing=len(others),
                best_other=min(max(max(others), 0), U32) if others else 0, excess=min(excess, U32))


def read_mapq(path_offsets, path_nodes, visit_length, entry_offsets, entries, chosen, list_len=None, rescue=None, paired=None, scale=2, slack=8, max_cand=0, more=None,
              mutation=None):
    """dict(records MAPQ_DTYPE[n_reads], n_has, n_unique, n_capped, sum_mapq).  chosen: an ordinal per read, NO_CHOSEN for none; list_len: None = every
    entry is a list candidate; rescue: None or the pgx_read_rescue records; paired: None or dict(seq_lengths, frag_min, frag_max, penalty); max_cand > 0
    and more (per read, or None): what sets CAPPED"""
    assert mutation is None or mutation in MUTATIONS
    n = len(entry_offsets) - 1
    assert paired is None or n % 2 == 0
    entries = np.asarray(entries, dtype=VERIFY_DTYPE)
    mine = lambda r: entries[int(entry_offsets[r]):int(entry_offsets[r + 1])]
    lists = lambda r: mine(r)[:len(mine(r)) if list_len is None else int(list_len[r])]
    out = np.zeros(n, MAPQ_DTYPE)
    n_unique = 0
    for r in range(n):
        e, n_list = mine(r), len(lists(r))
        assert len(e) <= MAX_ENTRIES and (int(chosen[r]) == NO_CHOSEN or int(chosen[r]) < n_list)
        scores = [int(x["seg_score"]) for x in e]
        used = False
        if paired is not None:
            mate = lists(r ^ 1)
            used = len(mate) > 0
            scores = [s + mate_term(paired["seq_lengths"], x, mate, paired["frag_min"], paired["frag_max"], paired["penalty"], mutation) for s, x in zip(scores, e)]
        capped = bool((max_cand and n_list >= max_cand) or (more is not None and more[r]))
        rec = mapq_read((path_offsets, path_nodes, visit_length), e, n_list, int(chosen[r]), scores, scale, slack, None if rescue is None else rescue[r], capped, used, mutation)
        for f, v in rec.items():
            out[r][f] = v
        n_unique += 1 if rec["flags"] & HAS and rec["excess"] == 0 else 0
    fl = out["flags"]
    return dict(records=out, n_has=int(((fl & HAS) != 0).sum()), n_unique=n_unique, n_capped=int(((fl & CAPPED) != 0).sum()), sum_mapq=int(out["mapq"].sum()))


def chosen_of(winners):
    """the chosen ordinal of every read from its winner record"""
    return np.array([NO_CHOSEN if int(w["seq"]) == NO_SEQUENCE else int(w["cand_index"]) for w in winners], dtype=np.uint32)


def candidates_with_extras(seqs, reads, place, verified, max_extra, penalty=4, mutation=None):
    """the entries of every read from a read-place result (reads, place_offsets, places) and a verify result with its list (cand_offsets, cands): the list, then
    the extras verified by verify_emu.  Returns (entry_offsets, entries, list_len, more); more[r]: more next-level placements exist than extras were taken"""
    n = len(reads)
    offs, flat, list_len, more = [0], [], [], []
    for r in range(n):
        lst = verified["cands"][int(verified["cand_offsets"][r]):int(verified["cand_offsets"][r + 1])]
        flat += [c for c in lst]
        list_len.append(len(lst))
        level = int(place["reads"][r]["best_score" if mutation == "extras_best" else "next_score"]) if max_extra > 0 else 0
        room, over, k = min(max_extra, MAX_ENTRIES - len(lst)), False, 0
        if level > 0:
            for p in place["places"][int(place["place_offsets"][r]):int(place["place_offsets"][r + 1])]:
                if int(p["score"]) != level:
                    continue
                if k >= room:
                    over = True
                    break
                v = V.verify_one(reads[r], seqs[int(p["seq"])], int(p["diag"]), penalty)
                v.update(seq=int(p["seq"]), n_cand=k, cand_index=k, n_tied=0)
                c = np.zeros((), VERIFY_DTYPE)
                for f in VERIFY_DTYPE.names:
                    c[f] = v[f]
                flat.append(c)
                k += 1
        more.append(over)
        offs.append(len(flat))
    ent = np.array(flat, dtype=VERIFY_DTYPE) if flat else np.zeros(0, VERIFY_DTYPE)
    return np.array(offs, np.uint64), ent, np.array(list_len, np.uint32), np.array(more, bool)
