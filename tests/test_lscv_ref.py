"""The float64 LSCV restatement of tests/golden/make_golden8.py (no GPU): the literal form (per-sub-region n_bins^2 joint histograms,
lstsq) against the per-bin form the device computes (cell sums, closed-form affine fit), the weight quirks of LSCV.cc:170-197, the
geometry refusal, 1 x 1 LSCV against SCV, and a spatially varying illumination scene."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import make_golden6 as G6  # noqa: E402
import make_golden8 as G8  # noqa: E402
import numpy_ref as R  # noqa: E402
from mtf_amd import synth  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "lk_golden8.npz"))
TAGS = [str(t) for t in GOLD["tags"]]


def case(tag):
    for c in G8.CASES:
        if c[0] == tag:
            return c
    raise KeyError(tag)


def sampled(tag):
    _, nb, resx, resy, nx, ny, sx, sy, am, once, lin, affine, corners = case(tag)
    pa = G6.Patch(GOLD["img"].astype(np.float64), nb, resx, resy, affine, corners)
    It, _ = pa.sample(pa.warp(GOLD[tag + "_p"]))
    return pa, It, nb, (resx, resy, nx, ny, sx, sy), am, lin


@pytest.mark.parametrize("tag", TAGS)
def test_literal_equals_per_bin(tag):
    pa, It, nb, geo, am, lin = sampled(tag)
    m_lit, a_lit = G8.literal_maps(It, pa.I0o, nb, geo)
    m_bin, a_bin = G8.per_bin_maps(It, pa.I0o, nb, geo)
    np.testing.assert_array_equal(m_lit, m_bin)
    np.testing.assert_allclose(a_bin, a_lit, rtol=1e-12, atol=1e-12)
    w = G8.weights(*geo)
    I0_lit = G8.blend(pa.I0o, m_lit, a_lit, w, geo[2], geo[3], am, lin)
    I0_bin = G8.blend(pa.I0o, m_bin, a_bin, w, geo[2], geo[3], am, lin)
    if am:
        np.testing.assert_allclose(I0_bin, I0_lit, rtol=0, atol=1e-11)
    else:
        np.testing.assert_array_equal(I0_bin, I0_lit)
    np.testing.assert_array_equal(I0_lit[:16], GOLD[tag + "_I0_head"]) if not am else None
    np.testing.assert_array_equal(m_lit, GOLD[tag + "_maps"])


def test_some_bins_are_empty():
    """the saturated regions leave bins empty in every sub-region: the map[b] = b rule is exercised"""
    for tag in TAGS:
        nb = int(GOLD[tag + "_cfg"][0])
        assert np.any(GOLD[tag + "_maps"] == np.arange(nb)), tag


def test_weights_truncate_toward_zero_and_rows_sum_to_one():
    # 50 x 50, 3 x 3, spacing 10: size 30, sub-region 0 spans [0, 29], centre 14.5; pixel 14 gives (int)(-0.5) = 0, pixel 15 (int)0.5 = 0
    w = G8.weights(50, 50, 3, 3, 10, 10)
    assert w.shape == (2500, 9)
    np.testing.assert_allclose(w.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    # pixels (14, 14) and (15, 15): both at diff (0, 0) from sub-region 0's centre -> the same raw weight 1 for that sub-region
    r14, r15 = w[14 * 50 + 14], w[15 * 50 + 15]
    raw = lambda px, py: np.array([1.0 / (1.0 + int(px - cx) ** 2 + int(py - cy) ** 2) for cy in (14.5, 24.5, 34.5) for cx in (14.5, 24.5, 34.5)])
    np.testing.assert_array_equal(r14, raw(14, 14) / sum(raw(14, 14).tolist()))
    np.testing.assert_array_equal(r15, raw(15, 15) / sum(raw(15, 15).tolist()))
    assert raw(14, 14)[0] == 1.0 and raw(15, 15)[0] == 1.0   # (truncation toward zero, not floor: -0.5 -> 0)
    assert int(14 - 24.5) == -10   # (and -10.5 -> -10)
    np.testing.assert_array_equal(GOLD["ship_50_w_head"], w[:16])


def test_geometry_refusal():
    with pytest.raises(ValueError, match="not enough to use the specified region spacing"):
        G8.regions(20, 50, 3, 3, 10, 10)   # size_x = 20 - 20 = 0
    G8.regions(21, 50, 3, 3, 10, 10)       # size 1: accepted
    # the gap case: sub-regions of 12 x 5 px at spacings 25 x 9 leave pixels outside every sub-region
    cx, _, _ = G8.cells(37, 2, 25)
    cy, _, _ = G8.cells(23, 3, 9)
    assert (cx < 0).any() and (cy < 0).any()


@pytest.mark.parametrize("linear", [0, 1])
def test_one_sub_region_is_scv(linear):
    """1 x 1 LSCV: the weight is exactly 1.0 and I0 = 0 + mapped, i.e. SCV's I0 bit for bit"""
    pa, It, nb, _, _, _ = sampled("near_50")
    geo = (50, 50, 1, 1, 10, 10)
    w = G8.weights(*geo)
    assert np.all(w == 1.0)
    _, _, I0 = G8.lscv_update(It, pa.I0o, nb, geo, w, 0, linear)
    m = G6.literal_map(It, pa.I0o, nb, 0)
    np.testing.assert_array_equal(I0, G6.remap(pa.I0o, m, linear))


LO, HI = 0.75, 1.25


def ramp_pair(shape=(256, 256)):
    """frame 1 = frame 0 warped by a known homography, then under a left-to-right gain ramp (LO at the left edge of the target to HI
    at its right edge): an illumination change that varies across the patch"""
    f0 = synth.make_frame(*shape, seed=11).astype(np.float64)
    Wt = np.array([[1.0, -0.02, 3.2], [0.025, 1.0, -2.6], [0.0, 0.0, 1.0]])
    yy, xx = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    q = np.linalg.inv(Wt) @ np.vstack([xx.ravel(), yy.ravel(), np.ones(xx.size)])
    src = R.bilinear(f0, q[0] / q[2], q[1] / q[2]).reshape(shape)
    gain = np.clip(LO + (HI - LO) * (xx - 78.0) / 100.0, LO, HI)
    f1 = np.clip(src * gain, 0, 254)
    c0 = synth.square_corners(128, 128, 100)
    ct = Wt @ np.vstack([c0, np.ones(4)])
    return f0, f1, c0, ct[:2] / ct[2]


def restated_esm(f0, f1, c0, nb, geo, iters=30):
    """the float64 ESM loop (DiffOfJacs + SumOfSelf) on the LSCV re-mapped template, re-mapped at every iteration"""
    resx, resy = geo[0], geo[1]
    pa0 = G6.Patch(f0, nb, resx, resy, False, c0)
    pa1 = G6.Patch(f1, nb, resx, resy, False, c0)
    pa1.I0o, pa1.J0 = pa0.I0o, pa0.J0
    w = G8.weights(*geo)
    W = np.eye(3)
    for _ in range(iters):
        It, Jt = pa1.sample(W)
        I0 = G8.lscv_update(It, pa1.I0o, nb, geo, w, 0, 0, form=G8.per_bin_maps)[2]
        dft = -(It - I0)
        dp = -np.linalg.solve(0.5 * (-Jt.T @ Jt - pa1.J0.T @ pa1.J0), 0.5 * (dft @ (pa1.J0 + Jt)))
        W = R.compose_hom(W, dp)
    return G6.corners_of(W, np.vstack([c0, np.ones(4)]))


def test_lscv_ends_closer_than_scv_under_a_gain_ramp():
    """Under a gain ramp across the patch (0.75 to 1.25), 64 bins, nearest mapping, 30 ESM iterations: 3 x 3 LSCV (spacing 10) ends
    closer to the true corners than SCV (1 x 1 LSCV, which is SCV bit for bit).  The margin is small and neither converges: measured
    with this restatement, LSCV 2.78 px and SCV 3.59 px off.  The test asserts only that ordering, with a 10 % margin."""
    f0, f1, c0, ct = ramp_pair()
    e_lscv = np.abs(restated_esm(f0, f1, c0, 64, (50, 50, 3, 3, 10, 10)) - ct).max()
    e_scv = np.abs(restated_esm(f0, f1, c0, 64, (50, 50, 1, 1, 10, 10)) - ct).max()
    assert 1.1 * e_lscv < e_scv, (e_lscv, e_scv)


def test_exports():
    import mtf_amd
    from mtf_amd import _lib as L
    assert mtf_amd.AM_LSCV == L.AM_LSCV == 5
    for name in ("mtfhip_batch_set_lscv", "mtfhip_batch_lscv_intensity_maps", "mtfhip_batch_set_first_iter", "mtfhip_batch_first_iter"):
        assert name in L.SYMBOLS
    assert hasattr(mtf_amd.Batch, "set_lscv") and hasattr(mtf_amd.Batch, "lscv_intensity_maps") and hasattr(mtf_amd.Batch, "set_first_iter")
