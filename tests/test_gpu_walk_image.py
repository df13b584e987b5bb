"""GPU tier of the walk image (pgx_index_paths): the node list of every sequence, recovered on the device from an index and its tags alone, equals
the path table the tags were made from.

For the `directory` table of tests/build_tags_cases.py (node starts and sequence ends on 1024 k - 1, 1024 k, 1024 k + 1, buckets of 1024 one-bp
nodes, empty sequences first, between and last) and two cases of its `sizes` table, tags by pgx_build_tags_paths in the compact query format:
Index.paths() is (path_offsets, path_nodes) of the case and the lengths of its nodes, in PGX_MODE_STRICT by the locate route, next to the
forced PAIRS layout and through a reopened image file; PGX_MODE_COMPAT refuses, these indexes being encoded without N.  The golden xy.ri with
the reference's own xy_bidirectional_compressed.tags against gbz_graph_emu.graph_tables of xy.gbz, by the locate route (PGX_FM_LCE=0) and
from a resident LCE image (the collection is bidirectional and above 4096 symbols; PGX_MODE_IMAGE_PAIRS as in test_gpu_text_image_borders.py);
which route ran is read off the line PGX_IMAGE_TIMING prints.

These two pin which run holds a row.  A converted build_tags file starts with the runs convert_tags reads out of the 8-byte header, so a row
is neither position i nor i - n_seq of the run starts: the runs END with the last row (csrc/pgx_image.h "WHICH RUN HOLDS ROW i"; xy: i + 15).
On the fixture the reading x = i agrees with the graph on 2 of the 8014 rows and x = i - n_seq on 4.

Then the refused handles: no tags, an image saved without the locate image, and the tags of one case on the index of another."""
import os

import numpy as np
import pytest

import build_tags_cases as B
import gbz_graph_emu as E
import pgx_ffi as P

pytestmark = pytest.mark.gpu
BT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bidirectional_test")
CASES = [("directory", "directory"), ("sizes", "runs_257"), ("sizes", "twice_4097")]
_made = {}


def _case(workdir, table, name):
    """the case with its compact tags, made once"""
    if (table, name) not in _made:
        c = B.build_case(workdir, table, name)
        d = os.path.join(workdir, "walk_image")
        os.makedirs(d, exist_ok=True)
        c.tags_path = os.path.join(d, "%s.compact.tags" % name)
        P.build_tags_paths(c.ri, c.path_offsets, c.path_nodes, c.node_length, c.first_node_id, c.tags_path, flags=P.BUILD_TAGS_OUT_COMPACT)
        _made[table, name] = c
    return _made[table, name]


def _equal(idx, po, pn, lens):
    got_po, got_pn, got_len = idx.paths()
    assert np.array_equal(got_po, po), (got_po[:8], po[:8])
    assert np.array_equal(got_pn, pn) and np.array_equal(got_len, lens)
    again = idx.paths()  # (the image is built once; the second call only reads it)
    assert all(np.array_equal(a, b) for a, b in zip(again, (got_po, got_pn, got_len)))


@pytest.mark.parametrize("table,name", CASES)
def test_paths_are_the_table_the_tags_were_made_from(workdir, table, name, monkeypatch):
    c = _case(workdir, table, name)
    lens = c.node_length[(c.path_nodes >> np.uint64(1)).astype(np.int64) - c.first_node_id]
    monkeypatch.setenv("PGX_FM_LCE", "0")
    for layout in (0, P.MODE_IMAGE_PAIRS):
        try:
            idx = P.Index(c.ri, c.tags_path, mode=P.MODE_STRICT | layout)
        except P.PgxError as e:
            assert layout and e.code == P.ERR_UNSUPPORTED, str(e)
            continue
        _equal(idx, c.path_offsets, c.path_nodes, lens)
        if not layout:
            pgi = os.path.join(workdir, "walk_image", "%s.pgi" % name)
            idx.save_image(pgi)
        idx.close()
    img = P.Index.open_image(pgi)
    _equal(img, c.path_offsets, c.path_nodes, lens)
    img.close()
    compat = P.Index(c.ri, c.tags_path, mode=P.MODE_COMPAT)
    info = compat.info()
    assert info.is_encoded and not info.has_N
    with pytest.raises(P.PgxError) as e:
        compat.paths()
    assert e.value.code == P.ERR_UNSUPPORTED and "PGX_MODE_STRICT" in str(e.value)
    compat.close()


def test_xy_fixture_against_the_graph(monkeypatch, capfd):
    g, seqs, fid = E.parse_graph(os.path.join(BT, "xy.gbz"))
    po, pn, nl, fid = E.graph_tables(g, seqs, fid)
    lens = nl[(pn >> np.uint64(1)).astype(np.int64) - fid]
    ri, tags = os.path.join(BT, "xy.ri"), os.path.join(BT, "xy_bidirectional_compressed.tags")
    monkeypatch.setenv("PGX_IMAGE_TIMING", "1")
    routes = set()
    for lce in (False, True):
        if lce:
            monkeypatch.delenv("PGX_FM_LCE", raising=False)
        else:
            monkeypatch.setenv("PGX_FM_LCE", "0")
        for mode in (P.MODE_STRICT, P.MODE_COMPAT):
            try:
                idx = P.Index(ri, tags, mode=mode | (P.MODE_IMAGE_PAIRS if lce else 0))
            except P.PgxError as e:  # (the forced layout does not exist for every mode of this index)
                assert lce and mode == P.MODE_COMPAT and e.code == P.ERR_UNSUPPORTED, str(e)
                continue
            info = idx.info()
            if mode == P.MODE_COMPAT and info.is_encoded and not info.has_N:
                with pytest.raises(P.PgxError) as e:
                    idx.paths()
                assert e.value.code == P.ERR_UNSUPPORTED
                idx.close()
                continue
            resident = bool(idx.lce_view(30, 4 * int(info.bwt_size)).any())  # (builds the LCE image where the handle qualifies)
            assert resident == lce
            capfd.readouterr()
            _equal(idx, po, pn, lens)
            err = capfd.readouterr().err
            assert ("walk image (lce route)" in err) == lce and ("walk image (locate route)" in err) == (not lce), err
            routes.add((lce, mode))
            idx.close()
    assert (False, P.MODE_STRICT) in routes and (True, P.MODE_STRICT) in routes


def test_refused_handles(workdir):
    c, other = _case(workdir, "directory", "directory"), _case(workdir, "sizes", "runs_257")
    bare = P.Index(c.ri, mode=P.MODE_STRICT)
    with pytest.raises(P.PgxError) as e:
        bare.paths()
    assert e.value.code == P.ERR_UNSUPPORTED and "without a tag array" in str(e.value)
    bare.close()
    idx = P.Index(c.ri, c.tags_path, mode=P.MODE_STRICT)
    pgi = os.path.join(workdir, "walk_image", "no_locate.pgi")
    idx.save_image(pgi, no_locate=True)
    idx.close()
    img = P.Index.open_image(pgi)
    with pytest.raises(P.PgxError) as e:
        img.paths()
    assert e.value.code == P.ERR_UNSUPPORTED and "--no-locate" in str(e.value)
    img.close()
    for ri, tags in ((c.ri, other.tags_path), (other.ri, c.tags_path)):  # runs that cover fewer rows than the index has, and more
        mixed = P.Index(ri, tags, mode=P.MODE_STRICT)
        with pytest.raises(P.PgxError) as e:
            mixed.paths()
        assert e.value.code == P.ERR_FORMAT and "the tags do not belong to this index" in str(e.value), str(e.value)
        mixed.close()
    good = P.Index(c.ri, c.tags_path, mode=P.MODE_STRICT)  # and the next call is served
    assert int(good.paths()[0][-1]) == len(c.path_nodes)
    good.close()
