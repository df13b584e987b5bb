"""GPU tier: the device read parser (pgx_batch_upload_text, csrc/pgx_fastx_kernels.hip) at its tile, line and record borders.  Every text of
tests/fastx_cases.py is uploaded and the reads the batch then holds on its device (pgx_batch_reads: bytes, offsets, longest read) are compared
byte for byte with what the emulator (tests/fastx_emu.py) parses; a refused text gives the emulator's message and leaves the reads of the
upload before it.  One batch serves the whole file, so every upload also meets what larger and smaller ones left in the grow-only buffers.
The other upload forms are read back the same way, and behind the copy-pass and the many-reads cases a search runs, device against device."""
import numpy as np
import pytest

import fastx_cases as FC
import fastx_emu as E
import pgx_ffi as P

pytestmark = pytest.mark.gpu

SMALL = FC.small_cases()
ARRAYS = ("mem_offsets", "pos_offsets", "positions", "tag_run_counts")
KNOWN = b"ACGTACGT\n\nGATTACA\r\nT"  # what a batch holds before a refused upload


@pytest.fixture(scope="module")
def idx(x_index):
    i = P.Index(*x_index)
    yield i
    i.close()


@pytest.fixture(scope="module")
def batch(idx):
    b = idx.batch_empty()
    yield b
    b.free()


def _holds(b, seqs):
    """the batch's reads on the device are exactly seqs"""
    cat, offs, longest = b.reads()
    ecat, eoffs = E.to_batch(seqs)
    assert len(offs) == len(seqs) + 1 and np.array_equal(offs, eoffs)
    assert len(cat) == len(ecat) and cat.tobytes() == ecat.tobytes()
    assert longest == max((len(s) for s in seqs), default=0)


def _upload_and_compare(b, case):
    seqs, _ = E.parse(case.text, case.fmt)
    assert b.upload_text(case.text, case.fmt) == len(seqs)
    _holds(b, seqs)
    return seqs


def _refused(b, case):
    with pytest.raises(E.FastxError) as ee:
        E.parse(case.text, case.fmt)
    known, _ = E.parse(KNOWN, E.LINES)
    assert b.upload_text(KNOWN, P.READS_LINES) == len(known) == 3
    with pytest.raises(P.PgxError) as e:
        b.upload_text(case.text, case.fmt)
    assert e.value.code == P.ERR_FORMAT
    assert ("pgx_batch_upload_text: " + str(ee.value)) in str(e.value), (str(e.value), str(ee.value))
    _holds(b, known)


@pytest.mark.parametrize("case", [c for c in SMALL if c.ok], ids=repr)
def test_accepted_text_read_back(batch, case):
    _upload_and_compare(batch, case)


@pytest.mark.parametrize("case", [c for c in SMALL if not c.ok], ids=repr)
def test_refused_text_leaves_the_reads(batch, case):
    _refused(batch, case)


def test_many_reads_read_back(batch):
    """600 001 reads: the longest-read pass strides over its grid of 2048 blocks, and the longest read is the last"""
    seqs = _upload_and_compare(batch, FC.many_reads_case())
    assert len(seqs) > FC.LONGEST_GRID_READS and batch.reads()[2] == 300


def test_many_tiles_fasta_read_back(batch):
    """4100 tiles, one read of 67 million bytes behind a header of 16 KiB: the copy pass over 16 000 blocks that all read line tables of 4101 lines"""
    seqs = _upload_and_compare(batch, FC.many_tiles_case(E.FASTA))
    assert len(seqs) == 1


def test_long_lived_batch(idx):
    """the largest text, then the smallest, then a refused one, then FASTA: the buffers only grow, and nothing of the 67 MB may show in what follows"""
    by = {c.name: c for c in SMALL}
    b = idx.batch_empty()
    try:
        seqs = _upload_and_compare(b, FC.many_tiles_case(E.LINES))
        assert len(seqs) == FC.MANY_TILES
        assert _upload_and_compare(b, by["one_A-lines"]) == [b"A"]
        with pytest.raises(P.PgxError) as e:
            b.upload_text(by["err_truncated_3_no_plus_issue-fastq"].text, P.READS_FASTQ)
        assert e.value.code == P.ERR_FORMAT and "FASTQ record 1 (byte 0): truncated record (3 of 4 lines)" in str(e.value)
        _holds(b, [b"A"])
        _upload_and_compare(b, by["width_1_crlf_blanks-fasta"])
        _upload_and_compare(b, by["headers_only-fasta"])
        _upload_and_compare(b, by["total_8192-fastq"])
    finally:
        b.free()


# ---- the other upload forms, read back
def _packed_upload(b, reads):
    cat, offs = E.to_batch(reads)
    packed = np.zeros(max((len(cat) + 15) // 16, 1), dtype=np.uint32)
    ids, side = np.zeros(len(offs), dtype=np.uint64), np.zeros(len(cat) + 16, dtype=np.uint8)
    ns, _ = P.pack_reads(cat, offs, packed, ids, side)
    b.upload_packed(packed, offs, ids, side, ns)
    return ns


def _acgt(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def _listed(rng, n, kind):
    """a read of n bytes that pgx_pack_reads lists: lower case, or with a \\0 or an N in it"""
    s = bytearray(_acgt(rng, n))
    if kind == 0:
        return bytes(s).lower()
    s[int(rng.integers(0, n))] = 0 if kind == 1 else ord("N")
    return bytes(s)


def _upload_form_batches():
    rng = np.random.default_rng(700)
    out = {}
    for total in (1, 15, 16, 17, 65537):  # one read, and the same bytes cut at random places
        s = _acgt(rng, total)
        out["total_%d_one_read" % total] = ([s], 0)
        cuts = np.unique(np.concatenate(([0, total], rng.integers(0, total + 1, size=total // 20))))
        out["total_%d_cut" % total] = ([s[int(a):int(b)] for a, b in zip(cuts[:-1], cuts[1:])], 0)
    for n in (1, 63, 64, 65, 129):  # a listed read of n bytes first, last, between others and next to another listed one; neighbours share its packed words
        for kind in range(3):
            plain = [_acgt(rng, int(k)) for k in rng.integers(1, 40, size=6)]
            x, y = _listed(rng, n, kind), _listed(rng, 7, (kind + 1) % 3)
            out["listed_%d_kind%d_first" % (n, kind)] = ([x] + plain, 1)
            out["listed_%d_kind%d_last" % (n, kind)] = (plain + [x], 1)
            out["listed_%d_kind%d_adjacent" % (n, kind)] = (plain[:3] + [x, y] + plain[3:] + [b"", y, x], 4)
    out["every_read_listed"] = ([_listed(rng, int(k), int(k) % 3) for k in rng.integers(1, 70, size=50)], 50)
    out["no_read_listed"] = ([_acgt(rng, int(k)) for k in rng.integers(0, 70, size=50)], 0)
    out["no_reads"] = ([], 0)
    return out


UPLOAD_FORMS = _upload_form_batches()


@pytest.mark.parametrize("name", sorted(UPLOAD_FORMS))
def test_upload_forms_read_back(batch, name):
    """pgx_batch_upload and pgx_batch_upload_packed (pgx_unpack_reads_kernel, then pgx_side_reads_kernel over the listed reads): the device
    holds the caller's bytes either way"""
    reads, n_listed = UPLOAD_FORMS[name]
    cat, offs = E.to_batch(reads)
    batch.upload(cat, offs)
    _holds(batch, reads)
    assert batch.upload_text(KNOWN, P.READS_LINES) == 3  # (something else in between)
    assert _packed_upload(batch, reads) == n_listed
    _holds(batch, reads)


# ---- searches behind the parse
def _same(a, b):
    assert a["n_extensions"] == b["n_extensions"]
    assert a["mems"].tobytes() == b["mems"].tobytes()
    for k in ARRAYS:
        assert np.array_equal(a[k], b[k]), k


def _search_equals_upload(idx, b, case):
    seqs = _upload_and_compare(b, case)
    b.run(10, 1, P.RUN_TAGS)
    got = b.result()
    _holds(b, seqs)  # (a run leaves the reads)
    cat, offs = E.to_batch(seqs)
    b2 = idx.batch_empty()
    try:
        b2.upload(cat, offs)
        b2.run(10, 1, P.RUN_TAGS)
        exp = b2.result()
    finally:
        b2.free()
    _same(got, exp)
    return got


@pytest.mark.parametrize("case", [c for c in SMALL if c.name.startswith(FC.COPY_CASE_PREFIXES)], ids=repr)
def test_search_behind_the_copy_pass(idx, batch, case):
    got = _search_equals_upload(idx, batch, case)
    assert len(got["mems"]) > 0


def test_search_behind_many_reads(idx, batch):
    """the sizes the parse recorded are the ones the search kernels need: the 300-symbol read behind 600 000 one-symbol reads gives its MEMs"""
    got = _search_equals_upload(idx, batch, FC.many_reads_case())
    mo = got["mem_offsets"]
    assert len(mo) == FC.MANY_READS + 2 and int(mo[FC.MANY_READS]) == 0 and int(mo[-1] - mo[-2]) > 0


def test_search_behind_many_tiles(idx, batch):
    got = _search_equals_upload(idx, batch, FC.many_tiles_case(E.LINES))
    assert len(got["mem_offsets"]) == FC.MANY_TILES + 1
