"""GPU tier of the text image (pgx_index_text) at its borders: on every collection of TEXT_CASES (tests/index_route_cases.py; the CPU tier
tests/test_index_route_cases.py asserts the border each one holds) the text recovered on the device equals the file the index was built
from, byte for byte, and the lengths equal its split -- from the encoded and the legacy .ri, in PGX_MODE_STRICT and, where pgx_index_text is
supported there, in PGX_MODE_COMPAT, by the locate route (PGX_FM_LCE=0) and from a resident LCE image wherever the handle has one (decided
with lce_view, as tests/test_gpu_text_image.py does), and for one case a group from an image file saved with the locate image and reopened.
Collections of at most 20 kB get the 64-byte rank image alone, and an LCE image only exists next to a PAIRS image, so the LCE route runs on
handles opened with PGX_MODE_IMAGE_PAIRS.  A test is a group of the table; it asserts that the locate route ran on every case and the LCE
route on every bidirectional case of 4096 symbols or more whose index qualifies for the PAIRS image, at least one in every group: no
group passes on one route only."""
import os

import pytest

import index_route_cases as C
import pgx_ffi as P
import pgx_workload as W
from test_gpu_text_image import _check_text

pytestmark = pytest.mark.gpu


def _indexes(workdir, name):
    path = os.path.join(workdir, "tib_%s.txt" % name)
    with open(path, "wb") as f:
        f.write(C.TEXT_CASES[name])
    return [W.build_index_from_text(path, workdir, "tib_" + name, encoded=encoded, with_tags=False)[0] for encoded in (True, False)]


def _handles(ri, layout=0):
    """the handles of an .ri that pgx_index_text serves: STRICT always, COMPAT unless the index is encoded without N.  layout: a forced image
    layout; a handle whose index does not qualify for it is left out"""
    for mode in (P.MODE_STRICT, P.MODE_COMPAT):
        try:
            idx = P.Index(ri, mode=mode | layout)
        except P.PgxError as e:
            assert layout and e.code == P.ERR_UNSUPPORTED, str(e)
            continue
        info = idx.info()
        if mode == P.MODE_COMPAT and info.is_encoded and not info.has_N:
            with pytest.raises(P.PgxError) as e:
                idx.text()
            assert e.value.code == P.ERR_UNSUPPORTED
            idx.close()
            continue
        yield mode, idx


@pytest.mark.parametrize("group", list(C.TEXT_GROUPS))
def test_text_of_every_case_by_every_route(workdir, group, monkeypatch):
    ran = {name: set() for name in C.TEXT_GROUPS[group]}
    for name in C.TEXT_GROUPS[group]:
        raw = C.TEXT_CASES[name]
        n = len(raw)
        for ri in _indexes(workdir, name):
            legacy = ri.endswith(".legacy.ri")
            # a resident LCE image first, where the handle has one: its suffix array stands in for the locate.  A collection this small gets the
            # 64-byte rank image alone, and the LCE image only exists next to a PAIRS image, so that layout is forced here
            monkeypatch.delenv("PGX_FM_LCE", raising=False)
            for mode, idx in _handles(ri, P.MODE_IMAGE_PAIRS):
                if idx.lce_view(30, 4 * n).any():
                    _check_text(idx, raw)
                    ran[name].add(("lce", mode, legacy))
                idx.close()
            # and without one: the whole-range locate, next to the default layout and next to the forced one
            monkeypatch.setenv("PGX_FM_LCE", "0")
            for layout in (0, P.MODE_IMAGE_PAIRS):
                for mode, idx in _handles(ri, layout):
                    assert not idx.lce_view(30, 4 * n).any()
                    _check_text(idx, raw)
                    ran[name].add(("locate", mode, legacy) if not layout else ("locate_pairs", mode, legacy))
                    idx.close()
        if name in C.PGI_CASES:  # saved with the locate image and reopened: the text is recovered through it
            monkeypatch.delenv("PGX_FM_LCE", raising=False)
            strict = P.Index(_indexes(workdir, name)[0], mode=P.MODE_STRICT)
            pgi = os.path.join(workdir, "tib_%s.pgi" % name)
            strict.save_image(pgi)
            strict.close()
            img = P.Index.open_image(pgi)
            _check_text(img, raw)
            img.close()
            ran[name].add(("pgi",))
    lce_cases = 0
    for name, routes in ran.items():
        raw = C.TEXT_CASES[name]
        for legacy in (False, True):  # the locate route from both files in STRICT; COMPAT wherever it is served (the legacy file always is)
            assert ("locate", P.MODE_STRICT, legacy) in routes, (name, routes)
        assert ("locate", P.MODE_COMPAT, True) in routes, (name, routes)
        has_lce = ("lce", P.MODE_STRICT, False) in routes
        if C.is_bidirectional(raw) and len(raw) >= C.LCE_MIN:  # an LCE image, unless the index does not qualify for the PAIRS image at all
            assert has_lce or not any(r[0] == "locate_pairs" for r in routes), (name, routes)
        else:
            assert not any(r[0] == "lce" for r in routes), (name, routes)
        lce_cases += has_lce
    assert lce_cases >= 1 and sum(("pgi",) in r for r in ran.values()) == 1, ran
