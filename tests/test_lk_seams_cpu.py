"""The seams of the compositional LK path (ESM / FCLK / ICLK, first and second order), no GPU: the conditions the reference alone must
meet on every case of tests/helpers/lk_seam_cases.py so that the device comparison of tests/test_gpu_lk_seams.py is meaningful.

(a) H and g of the first iteration are finite -- except NCC wholly outside the frame, where the reference divides 0 by 0: the table marks
    those cases reference_nan and the oracle must really return NaN there;
(b) the half-outside regions have 20 .. 80 % of their template samples equal to the border constant 128, and from 64 pixels on a run of
    64 consecutive pixels that holds both kinds; every such region also has a shape whose 64-ALIGNED runs (the waves of a kernel that
    takes the pixels in order) mix the two -- not every shape can: at 32 x 33 across the bottom edge the border begins on row 20 of rows of
    32 pixels, so every aligned run is two whole rows of one kind (test_every_edge_has_a_mixed_wave);
(c) second order: the first-pass H is more than 1e-4 (relative) from the sec_ord_hess = 0 oracle's (the device gates are 1e-5 or tighter);
(d) no sample point is within 1e-6 of an integer coordinate.  The current points of the first pass are the template's, and the +-1 / +-2 px
    stencil points of the image Hessian (hess_eps = 1) have their fractional parts, so this one condition covers them all: the 1e-13 px
    between the device's grid and the oracle's cannot move a sample into another bilinear cell or onto the dx == 0 rule;
(e) the jitter floor: corners moved by a seeded +-1e-12 px change the oracle's H and g by less than 1e-6 -- a tenth of the 1e-5 the device
    is held to on its own grid.  A condition on the table, not a tolerance: a case that breaks it gets another region.  One seeded sign
    pattern for the whole table.  The figure is itself a draw from the reference's rounding noise (its grad_eps = 1e-8 central difference
    divides the last bits of two samples by 2e-8): over eight sign patterns the table's maximum was 7.4e-7 .. 1.16e-6, the three patterns
    above 1e-6 all on 4- or 35-pixel patches (2 x 2 NCC 1.03e-6 and 1.10e-6; 5 x 7 ICLK SSD across the top edge 1.16e-6).  So the margin
    under the device gate is ten times for most of the table and never below 8.6 times;

And the oracle's own getImgHess / getWarpedImgHess against the dense float64 restatement at the border and integer-coordinate points."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lk_seam_cases as K   # noqa: E402

JITTER_SEED = 0


def test_table_covers_what_it_claims():
    assert 200 <= len(K.CASES) <= 400 and len(set(K.IDS)) == len(K.CASES)
    names = [K.model_name(m) for m in K.MODELS]
    assert len(set(names)) == len(names) == 34
    for shape in K.SHAPES:                                # every shape on `inside`, first and second order
        kinds = {K.second_order(c) for c in K.CASES if (c.resx, c.resy) == shape and c.region == "inside"}
        assert kinds == {False, True}, shape
    for shape in K.FULL_SHAPES:                           # every region on the three full shapes
        assert {c.region for c in K.CASES if (c.resx, c.resy) == shape} == set(K.REGIONS), shape
    for m in names:                                       # every model on every region
        assert {c.region for c in K.CASES if K.model_name(c.model) == m} == set(K.REGIONS), m
    quad = K.REGIONS["quad"]
    assert np.abs(quad - K.REGIONS["inside"]).max() <= 3.0 and np.abs(quad - K.REGIONS["inside"]).min() > 0.05
    for corners in K.REGIONS.values():
        assert np.all(np.abs(corners - np.round(corners)) > 1e-3)


@pytest.mark.parametrize("cid", K.IDS)
def test_reference_conditions(oracle, frame, frame2, cid):
    c = K.BY_ID[cid]
    ref = K.reference(oracle, frame, frame2, cid)
    rec = ref["rec"]
    N = K.n_pix(c)
    # (a)
    if c.reference_nan:
        assert np.all(ref["I0"] == 128.0)
        assert not np.all(np.isfinite(rec["H"])) or not np.all(np.isfinite(rec["g"]))
        return
    assert np.all(np.isfinite(rec["H"])) and np.all(np.isfinite(rec["g"])) and np.isfinite(rec["f"])
    if c.region == "outside":
        assert rec["f"] == 0.0 and np.all(rec["g"] == 0.0) and np.all(rec["H"] == 0.0)
        return
    # (b)
    if c.region in K.HALF_OUTSIDE:
        border = ref["I0"] == 128.0
        assert 0.2 <= border.mean() <= 0.8, border.mean()
        if N >= 64:
            assert any(0 < border[s:s + 64].sum() < 64 for s in range(N - 63))
    # (c)
    if K.second_order(c):
        first = K.first_pass(oracle, frame, frame2, c.model, c.resx, c.resy, K.REGIONS[c.region], with_arrays=False, sec_ord_hess=0)["rec"]
        assert K.rel(first["H"], rec["H"]) > 1e-4
    # (d)
    pts = ref["init_pts"]
    assert np.abs(pts - np.round(pts)).min() > 1e-6
    # (e)
    moved = K.REGIONS[c.region] + np.random.default_rng(JITTER_SEED).choice([-1e-12, 1e-12], size=(2, 4))
    jit = K.first_pass(oracle, frame, frame2, c.model, c.resx, c.resy, moved, with_arrays=False)["rec"]
    assert K.rel(jit["H"], rec["H"]) < 1e-6
    assert np.linalg.norm(jit["g"] - rec["g"]) < 1e-6 * max(np.linalg.norm(rec["g"]), K.g_scale(rec, c.model.am))


def test_every_edge_has_a_mixed_wave(oracle, frame, frame2):
    for region in K.HALF_OUTSIDE:
        mixed = []
        for c in K.CASES:
            if c.region == region and K.n_pix(c) >= 64:
                border = K.reference(oracle, frame, frame2, c.id)["I0"] == 128.0
                mixed.append(any(0 < border[s:s + 64].sum() < 64 for s in range(0, K.n_pix(c), 64)))
        assert mixed and any(mixed), region


def test_quad_region_is_projective(oracle):
    """the rectangle -> quad warp of the `quad` region has a projective row (the library clears its batch-wide unit_z for it), the one of
    `inside` has none"""
    for name, projective in (("inside", False), ("quad", True)):
        ssm = oracle.SSM(K.HOM, 5, 7)
        ssm.set_corners(K.REGIONS[name])
        z = ssm.get("init_pts_hm").reshape(-1, 3)[:, 2]
        assert (np.ptp(z) > 1e-6) == projective, (name, np.ptp(z))


def test_oracle_image_hessians_at_the_border(oracle, frame):
    """mtfo_get_img_hess / mtfo_get_warped_img_hess (utils::getImgHess, getWarpedImgHess) against numpy_ref.image_hessian_stencil on the
    border / integer-coordinate point list.

    Exactly equal, not merely within an ulp: numpy_ref.bilinear restates the reference's sampler expression for expression -- the same
    in-range test, the same upper neighbour (taken only when the fractional part is non-zero), the four products
    ((I * (1 - dx)) * (1 - dy) ...) summed left to right -- and image_hessian_stencil the stencil's (inc + dec - 2 c) / 4 and
    ((a + b) - (c + d)) / 4 (the division by 4 = (2 eps)^2 is exact, like the reference's multiplication by its reciprocal 0.25); NumPy
    does not contract to FMA and the oracle is compiled for the baseline x86-64 instruction set, which has none, so every intermediate
    rounds alike."""
    import numpy_ref as R
    h, w = frame.shape
    pts = K.hess_border_points(h, w)
    flat = np.ascontiguousarray(pts.T.ravel())
    want = R.image_hessian_stencil(frame.astype(np.float64), pts[0], pts[1])
    got = oracle.get_img_hess(frame, flat).reshape(-1, 2, 2)
    assert np.array_equal(got, want)
    assert np.abs(want).max() > 10.0                         # the list is not all flat border
    # the warped form on the same stencil: hess_pts = (+xx, -xx, +yy, -yy, +xy, -xy, +yx, -yx) of the identity warp at hess_eps = 1
    off = np.array([[2, 0], [-2, 0], [0, 2], [0, -2], [1, 1], [-1, -1], [1, -1], [-1, 1]], dtype=np.float64)
    hp = (pts.T[:, None, :] + off[None]).reshape(-1)
    got_w = oracle.get_warped_img_hess(frame, flat, np.ascontiguousarray(hp)).reshape(-1, 2, 2)
    assert np.array_equal(got_w, got)                        # the two overloads take the same samples in the same order


def test_long_double_solve():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(8, 8)); A = A + A.T
    x = rng.normal(size=8)
    got = K.long_double_solve(A, A @ x)
    assert np.abs(np.asarray(got, dtype=np.float64) - x).max() < 1e-12
    assert K.long_double_solve(np.zeros((3, 3)), np.ones(3)) is None
