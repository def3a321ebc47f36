"""The float64 LRSCV restatement of tests/golden/make_golden9.py (no GPU): the literal form (per-sub-region n_bins^2 joint histograms,
lstsq) against the per-bin form the device computes (cell sums keyed by the current bin, closed-form affine fit), the blend order of
LRSCV.cc:249-254 against LSCV's, 1 x 1 LRSCV against make_golden7's RSCV, the once_per_frame early return, the geometry refusal; and the
interface the device path adds (AM_LRSCV, the C-ABI symbols, the Python and C++ entry points)."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden6 as G6  # noqa: E402
import make_golden7 as G7  # noqa: E402
import make_golden9 as G9  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "lk_golden9.npz"))
GOLD7 = np.load(os.path.join(HERE, "golden", "lk_golden7.npz"))
TAGS = [str(t) for t in GOLD["tags"]]


def case(tag):
    for c in G9.CASES:
        if c[0] == tag:
            return c
    raise KeyError(tag)


def sampled(tag):
    _, nb, resx, resy, nx, ny, sx, sy, am, once, lin, affine, corners = case(tag)
    pa = G6.Patch(GOLD["img"].astype(np.float64), nb, resx, resy, affine, corners)
    It_orig, _ = pa.sample(pa.warp(GOLD[tag + "_p"]))
    return pa, It_orig, nb, (resx, resy, nx, ny, sx, sy), am, lin


@pytest.mark.parametrize("tag", TAGS)
def test_literal_equals_per_bin(tag):
    pa, It_orig, nb, geo, am, lin = sampled(tag)
    np.testing.assert_array_equal(It_orig[:16], GOLD[tag + "_It_orig_head"])
    m_lit, a_lit = G9.literal_maps(It_orig, pa.I0o, nb, geo)
    m_bin, a_bin = G9.per_bin_maps(It_orig, pa.I0o, nb, geo)
    np.testing.assert_array_equal(m_lit, m_bin)
    np.testing.assert_allclose(a_bin, a_lit, rtol=1e-12, atol=1e-12)
    w = G9.weights(*geo)
    It_lit = G9.blend(It_orig, m_lit, a_lit, w, geo[2], geo[3], am, lin)
    It_bin = G9.blend(It_orig, m_bin, a_bin, w, geo[2], geo[3], am, lin)
    if am:
        np.testing.assert_allclose(It_bin, It_lit, rtol=0, atol=1e-11)
    else:
        np.testing.assert_array_equal(It_bin, It_lit)
    np.testing.assert_array_equal(m_lit, GOLD[tag + "_maps"])
    np.testing.assert_array_equal(It_lit[:16], GOLD[tag + "_It_head"])
    if tag + "_It" in GOLD:
        np.testing.assert_array_equal(It_lit, GOLD[tag + "_It"])


def test_some_bins_are_empty():
    """the saturated regions leave current bins empty in sub-regions: the map[b] = b rule is exercised"""
    for tag in TAGS:
        nb = int(GOLD[tag + "_cfg"][0])
        assert np.any(GOLD[tag + "_maps"] == np.arange(nb)), tag


def test_blend_order_is_region_id_not_lscv():
    """LRSCV adds the sub-regions in region_id order (idy outer, idx inner); LSCV's order (idx outer, idy inner) rounds differently on
    some pixel of a 3 x 3 case, and the fixture holds the region_id order"""
    differs = 0
    for tag in ("near_50", "lin_50", "n256_60", "aff_40"):
        pa, It_orig, nb, geo, am, lin = sampled(tag)
        m, a = G9.per_bin_maps(It_orig, pa.I0o, nb, geo)
        w = G9.weights(*geo)
        rid = G9.blend(It_orig, m, a, w, geo[2], geo[3], am, lin)
        lscv = G9.blend_lscv_order(It_orig, m, a, w, geo[2], geo[3], am, lin)
        np.testing.assert_allclose(lscv, rid, rtol=0, atol=1e-12)
        np.testing.assert_array_equal(rid, GOLD[tag + "_It"])
        differs += int(np.count_nonzero(rid != lscv))
    assert differs > 0


@pytest.mark.parametrize("tag", ["r64n_50", "r64l_50", "r256n_60", "r64n_aff"])
def test_one_sub_region_equals_rscv(tag):
    """1 x 1 LRSCV is RSCV bit for bit: one map over the whole patch, the weight 1.0, the blend 0 + m 1.0"""
    nb, lin, resx, resy, aff = (int(v) for v in GOLD7[tag + "_cfg"])
    corners = GOLD7[tag + "_corners"]
    pa = G6.Patch(GOLD7["img"].astype(np.float64), nb, resx, resy, bool(aff), corners)
    It_orig, _ = pa.sample(pa.warp(GOLD7[tag + "_p"]))
    geo = (resx, resy, 1, 1, 10, 10)
    w = G9.weights(*geo)
    np.testing.assert_array_equal(w, np.ones((resx * resy, 1)))
    maps, _, It = G9.lrscv_update(It_orig, pa.I0o, nb, geo, w, 0, lin)
    np.testing.assert_array_equal(maps[0], GOLD7[tag + "_map"])
    np.testing.assert_array_equal(maps[0], G7.literal_map(It_orig, pa.I0o, nb))
    np.testing.assert_array_equal(It[:16], GOLD7[tag + "_It_head"])
    if tag + "_It" in GOLD7:
        np.testing.assert_array_equal(It, GOLD7[tag + "_It"])


def test_once_per_frame_early_return_leaves_it_raw():
    """LRSCV.cc:234-235: with once_per_frame and not the first iteration, It is the raw sample -- no map, no blend"""
    pa, It_orig, nb, geo, am, lin = sampled("ship_50")
    w = G9.weights(*geo)
    maps, aff, It = G9.lrscv_update(It_orig, pa.I0o, nb, geo, w, am, lin, first_iter=False, once=True)
    assert maps is None and aff is None
    np.testing.assert_array_equal(It, It_orig)
    maps, aff, It = G9.lrscv_update(It_orig, pa.I0o, nb, geo, w, am, lin, first_iter=True, once=True)
    np.testing.assert_array_equal(maps, GOLD["ship_50_maps"])
    assert np.any(It != It_orig)
    # without once_per_frame every iteration maps
    _, _, It2 = G9.lrscv_update(It_orig, pa.I0o, nb, geo, w, am, lin, first_iter=False, once=False)
    np.testing.assert_array_equal(It2, It)


def test_geometry_refusal():
    with pytest.raises(ValueError, match="not enough to use the specified region spacing"):
        G9.regions(50, 20, 3, 3, 10, 10)   # size_y = 20 - 20 = 0
    G9.regions(50, 21, 3, 3, 10, 10)       # size 1: accepted


def test_fixture_weights_and_size():
    np.testing.assert_array_equal(GOLD["ship_50_w_head"], G9.weights(50, 50, 3, 3, 10, 10)[:16])
    assert os.path.getsize(os.path.join(HERE, "golden", "lk_golden9.npz")) < 512 * 1024
    assert sum(1 for t in TAGS if t + "_esm_dp" in GOLD) >= 2


def test_lrscv_interface_exists():
    """AM_LRSCV = 6 and its entry points: the header declares them, the Python layer binds them"""
    import mtf_amd
    from mtf_amd import _lib as L
    from mtf_amd import host
    assert mtf_amd.AM_LRSCV == L.AM_LRSCV == 6
    text = open(os.path.join(ROOT, "include", "mtfhip.h")).read()
    assert re.search(r"MTFHIP_AM_LRSCV\s*=\s*6", text)
    for sym in ("mtfhip_batch_set_lrscv", "mtfhip_batch_lrscv_intensity_maps"):
        assert sym in L.SYMBOLS
        assert re.search(r"\b%s\s*\(" % sym, text)
    assert callable(mtf_amd.Batch.set_lrscv) and callable(mtf_amd.Batch.lrscv_intensity_maps)
    assert callable(host.CppTracker.lrscv)
