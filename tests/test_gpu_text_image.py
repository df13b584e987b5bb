"""GPU tier of the text image (pgx_index_text): the collection recovered on the device from the index alone equals the text the index was
built from -- on the collections of tests/test_gpu_mem_locate_sets.py (bidirectional, with N), a forward-only text with an odd number of
sequences, a collection that holds a sequence of length 1, and the golden texts; by the locate route (PGX_FM_LCE=0) and from a resident LCE
image; and the handles it refuses."""
import os

import numpy as np
import pytest

import pgx_ffi as P
import pgx_workload as W
from test_gpu_mem_locate_sets import _collection

pytestmark = pytest.mark.gpu


def _expect(raw):
    """(sequence lengths, bytes) of a text file: every sequence followed by one newline"""
    if raw and not raw.endswith(b"\n"):
        raw += b"\n"
    return [len(s) for s in raw.split(b"\n")[:-1]], raw


def _check_text(idx, raw):
    lens, text = idx.text()
    want_lens, want = _expect(raw)
    assert lens.tolist() == want_lens
    assert len(text) == len(want) == int(idx.info().bwt_size)
    if text != want:
        a, b = np.frombuffer(text, np.uint8), np.frombuffer(want, np.uint8)
        at = int(np.flatnonzero(a != b)[0])
        raise AssertionError("first difference at byte %d of %d: %r, want %r" % (at, len(want), text[at:at + 20], want[at:at + 20]))
    lens2, text2 = idx.text()  # the image stays: the same again
    assert text2 == text and lens2.tolist() == want_lens


@pytest.mark.parametrize("n_hap", [32, 33, 65])
def test_text_of_the_collections_by_both_routes(workdir, n_hap, monkeypatch):
    ri, tags, seqs, n_seq = _collection(workdir, "hits_border_%d" % n_hap, n_hap, 2000, 100 + n_hap)
    raw = open(os.path.join(workdir, "hits_border_%d.txt" % n_hap), "rb").read()
    assert b"N" in raw and len(raw) >= 4096 and raw.count(b"\n") == n_seq == 2 * n_hap
    # the LCE image resident first: its suffix array stands in for the locate
    idx = P.Index(ri, tags)
    n = int(idx.info().bwt_size)
    assert idx.lce_view(30, 4 * n).any(), "the LCE image of this index was expected to exist"
    _check_text(idx, raw)
    idx.close()
    # and without one: the whole-range locate
    monkeypatch.setenv("PGX_FM_LCE", "0")
    for mode in (P.MODE_COMPAT, P.MODE_STRICT):
        idx = P.Index(ri, tags, mode=mode)
        assert not idx.lce_view(30, 4 * n).any()
        _check_text(idx, raw)
        idx.close()


def _build(workdir, name, raw, encoded=True):
    path = os.path.join(workdir, name + ".txt")
    with open(path, "wb") as f:
        f.write(raw)
    return W.build_index_from_text(path, workdir, name, encoded=encoded, with_tags=False)[0]


def test_forward_only_text_with_an_odd_number_of_sequences(workdir):
    rng = np.random.default_rng(11)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=int(k), p=[0.24, 0.24, 0.24, 0.24, 0.04])) for k in (700, 1, 333, 2048, 9, 1500, 64)]
    raw = b"".join(s + b"\n" for s in seqs)
    assert len(seqs) % 2 == 1 and len(raw) >= 4096
    for encoded in (True, False):
        idx = P.Index(_build(workdir, "text_fwd_%d" % encoded, raw, encoded), mode=P.MODE_STRICT)
        _check_text(idx, raw)
        idx.close()


def test_collection_with_a_sequence_of_length_one(workdir):
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    fwd = [b"ACGTACGGTTAACCGGTACGATTACA", b"G", b"TTGACCANNNACGT", b"A"]
    seqs = []
    for s in fwd:  # every sequence next to its reverse complement
        seqs += [s, s.translate(comp)[::-1]]
    raw = b"".join(s + b"\n" for s in seqs)
    idx = P.Index(_build(workdir, "text_len1", raw), mode=P.MODE_STRICT)
    _check_text(idx, raw)
    idx.close()


def test_golden_texts(workdir, golden):
    bt = os.path.join(golden, "bidirectional_test")
    committed = [(os.path.join(bt, "contigs_xy"), os.path.join(bt, "xy.ri")),
                 (os.path.join(golden, "two_contig_graph", "contigs_XY.txt"), os.path.join(golden, "two_contig_graph", "xy.ri"))]
    for text_path, ri in committed:  # the .ri files of tests/golden that were built from a text of tests/golden
        raw = open(text_path, "rb").read()
        for mode in (P.MODE_COMPAT, P.MODE_STRICT):
            idx = P.Index(ri, mode=mode)
            info = idx.info()
            if not (mode == P.MODE_COMPAT and info.is_encoded and not info.has_N):
                _check_text(idx, raw)
            idx.close()
    for k, text_path in enumerate([committed[0][0], committed[1][0], os.path.join(golden, "med_test.txt"), os.path.join(golden, "x.newline_separated"),
                                   os.path.join(bt, "contigs_x"), os.path.join(bt, "contigs_y")]):
        raw = open(text_path, "rb").read()
        idx = P.Index(_build(workdir, "text_golden_%d" % k, raw), mode=P.MODE_STRICT)
        _check_text(idx, raw)
        idx.close()


def test_refused_handles(workdir, golden):
    raw = open(os.path.join(golden, "x.newline_separated"), "rb").read()
    assert b"N" not in raw
    ri = _build(workdir, "text_refused", raw, encoded=True)
    idx = P.Index(ri, mode=P.MODE_COMPAT)
    info = idx.info()
    assert info.is_encoded and not info.has_N
    with pytest.raises(P.PgxError) as e:
        idx.text()
    assert e.value.code == P.ERR_UNSUPPORTED and "PGX_MODE_STRICT" in str(e.value)
    # an image file saved without the locate image: the text is recovered through it
    strict = P.Index(ri, mode=P.MODE_STRICT)
    pgi = os.path.join(workdir, "text_refused.pgi")
    strict.save_image(pgi, no_locate=True)
    strict.close()
    img = P.Index.open_image(pgi)
    with pytest.raises(P.PgxError) as e:
        img.text()
    assert e.value.code == P.ERR_UNSUPPORTED and "locate" in str(e.value)
    img.close()
    # too small a buffer: PGX_ERR_ARG with both numbers
    lens = np.zeros(1, np.uint64)
    st = P.lib().pgx_index_text(idx.h, 0, lens.ctypes.data, 1, None, 0)
    assert st == P.ERR_UNSUPPORTED  # (the COMPAT handle is refused before its arguments are looked at)
    idx.close()
    strict = P.Index(ri, mode=P.MODE_STRICT)
    assert P.lib().pgx_index_text(strict.h, 0, lens.ctypes.data, 1, None, 0) == P.ERR_ARG and b"n_seq_cap is 1" in P.lib().pgx_last_error()
    strict.close()
