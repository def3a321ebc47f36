"""CPU: the reference side of the frame-layout tests (tests/test_gpu_frame_layout.py) on a NON-SQUARE frame, and the layout fixture those
tests borrow their padded, offset views from.

The oracle's samples and central-difference gradients on a 96 x 160 frame are pinned to an independent float64 NumPy restatement of
getPixVal<Linear, Constant> (imgUtils.h:91-113), written from the header's text with vectorised selects instead of early returns: the
`x >= w`, `ux >= w` -> 128 rules and the `dx == 0 ? lx : lx + 1` rule included.  An h / w mix-up in the oracle would pass every test on
the square 512 x 512 frame of the suite; it cannot pass here."""
import numpy as np
import pytest

from mtf_amd import _lib as L
from mtf_amd import synth

# ---------------------------------------------------------------- the layout fixture (shared with the GPU file)
H, W = 96, 160                  # the logical frame: h != w
H_SMALL = 48                    # a frame lower than the 64 x 64 LDS window of k_iclk_track / k_grid_fb
PH, PW = 256, 203               # the parent allocation: odd row pitch
R0, C0 = 64, 21                 # the view's origin inside it: an odd float offset (64 * 203 + 21 = 13013)
POISON = 1.0e6                  # finite: a leak shows as a wrong number, not as NaN
RES = [(17, 13), (40, 40)]      # N = 221: below one workgroup and kTemplateInitMaxPix, ragged; N = 1600: several workgroups, above it
B = 5


def views():
    """name -> logical frame: a / b the 96 x 160 frame and its successor (a small known homography about the centre), sa / sb the same
    at 48 x 160"""
    p_true = synth.random_small_homography(np.random.default_rng(2027)) * 0.5
    a = synth.make_frame(H, W)
    sa = synth.make_frame(H_SMALL, W, seed=synth.DEFAULT_SEED + 5)
    return dict(a=a, b=synth.warp_frame(a, p_true, (W / 2.0, H / 2.0)), sa=sa, sb=synth.warp_frame(sa, p_true, (W / 2.0, H_SMALL / 2.0)))


def place(view):
    """the view in the middle of a poisoned parent: any plausible mis-addressing (y * w + x, swapped w / h, a row above 0 or below h)
    still lands inside the allocation"""
    parent = np.full((PH, PW), POISON, dtype=np.float32)
    parent[R0:R0 + view.shape[0], C0:C0 + view.shape[1]] = view
    return parent


def targets(h=H):
    """(B, 2, 4) corners: one patch well inside, one across each of the left, top, right and bottom borders.  The right-border patch is
    centred at x = 140: inside the frame only if w and h are not swapped."""
    if h == H:
        t = [synth.square_corners(80, 48, 40), synth.square_corners(8, 50, 40), synth.square_corners(70, 6, 40),
             synth.square_corners(140, 48, 50), synth.square_corners(60, 90, 40)]
    else:
        t = [synth.square_corners(80, 24, 30), synth.square_corners(8, 24, 30), synth.square_corners(70, 5, 30),
             synth.square_corners(140, 24, 44), synth.square_corners(60, 42, 30)]
    return np.stack(t)


def small_states(ssm, n=B, seed=9, scale=0.5):
    rng = np.random.default_rng(seed)
    if ssm == L.SSM_HOMOGRAPHY:
        return np.stack([synth.random_small_homography(rng, scale) for _ in range(n)])
    return rng.uniform(-1, 1, (n, 6)) * np.array([2, 2, .02, .02, .02, .02]) * scale


def layout_is_discriminating(view, origin=0):
    """fraction of view pixels for which the packed address y * w + x, applied to the parent from `origin` (floats), does NOT give the
    pixel.  origin 0: from the allocation's start; R0 * PW + C0: from the view's base pointer, which is where a sampler that took w for
    the pitch would read"""
    parent = place(view).ravel()
    h, w = view.shape
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return float((parent[origin + yy * w + xx] != view).mean())


# ---------------------------------------------------------------- float64 restatement of getPixVal<Linear, Constant>
def pix_val_np(img, x, y):
    h, w = img.shape
    im = img.astype(np.float64)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out0 = (x < 0) | (x >= w) | (y < 0) | (y >= h)
    xs, ys = np.where(out0, 0.0, x), np.where(out0, 0.0, y)
    lx, ly = np.trunc(xs).astype(np.int64), np.trunc(ys).astype(np.int64)
    dx, dy = xs - lx, ys - ly
    ux, uy = np.where(dx == 0, lx, lx + 1), np.where(dy == 0, ly, ly + 1)
    out1 = (ux >= w) | (uy >= h)
    uxc, uyc = np.where(out1, lx, ux), np.where(out1, ly, uy)
    v = im[ly, lx] * (1 - dx) * (1 - dy) + im[ly, uxc] * dx * (1 - dy) + im[uyc, lx] * (1 - dx) * dy + im[uyc, uxc] * dx * dy
    return np.where(out0 | out1, 128.0, v)


def img_grad_np(img, x, y, eps=1e-8):
    mult = 1.0 / (2 * eps)
    return np.stack([(pix_val_np(img, x + eps, y) - pix_val_np(img, x - eps, y)) * mult,
                     (pix_val_np(img, x, y + eps) - pix_val_np(img, x, y - eps)) * mult], axis=1)


def test_restatement_rules():
    """the restatement itself on hand-made coordinates: outside, the last row / column (ux == w), exact integers (dx == 0)"""
    img = np.arange(12, dtype=np.float32).reshape(3, 4) * 10      # h = 3, w = 4
    x = np.array([-1e-9, 0.0, 3.0, 3.0 + 1e-9, 2.5, 1.0, 1.5, 3.9, 0.0, 3.0])
    y = np.array([1.0, 0.0, 2.0, 1.0, 2.5, 2.0, 1.5, 0.0, 2.9, 2.0 + 1e-9])
    want = np.array([128.0, 0.0, 110.0, 128.0, 128.0, 90.0, 0.25 * (50 + 60 + 90 + 100), 128.0, 128.0, 128.0])
    np.testing.assert_allclose(pix_val_np(img, x, y), want, rtol=0, atol=1e-12)
    # (the last column and the last row each answer to their own extent)
    assert pix_val_np(img, 3.5, 1.0) == 128.0 and pix_val_np(img.T.copy(), 1.0, 3.5) == 128.0
    assert pix_val_np(img, 2.5, 1.0) == 65.0


@pytest.mark.parametrize("name", ["a", "sa"])
def test_layout_fixture_is_discriminating(name):
    view = views()[name]
    assert view.shape == ((H, W) if name == "a" else (H_SMALL, W))
    assert layout_is_discriminating(view) >= 0.95
    assert layout_is_discriminating(view, R0 * PW + C0) >= 0.95      # (row 0 is right under either pitch: 1 row of 96, or of 48)
    parent = place(view)
    assert (R0 * PW + C0) % 2 == 1 and PW % 2 == 1
    assert np.array_equal(parent[R0:R0 + view.shape[0], C0:C0 + view.shape[1]], view)
    assert (parent == POISON).sum() == PH * PW - view.size
    assert view.max() < 1e3      # (poison is far from every pixel)


@pytest.mark.parametrize("ssm", [L.SSM_HOMOGRAPHY, L.SSM_AFFINE], ids=["hom", "aff"])
@pytest.mark.parametrize("res", RES, ids=lambda r: "%dx%d" % r)
@pytest.mark.parametrize("name", ["b", "sb"])
def test_oracle_samples_on_the_non_square_frame(oracle, name, res, ssm):
    """the oracle's updatePixVals / updatePixGrad at the five targets' warped grids against the restatement.  Samples: 1e-12 absolute
    (the same float64 expression; at most the order of the four products' sum differs).  Gradients: the difference of two such samples
    times 1 / (2 grad_eps), so 2 x 1e-12 / (2 x 1e-8) = 1e-4 absolute."""
    img = views()[name]
    h = img.shape[0]
    states = small_states(ssm)
    n_border = 0
    for t, corners in enumerate(targets(h)):
        o_ssm = oracle.SSM(ssm, res[0], res[1]); o_am = oracle.AM(L.AM_SSD, res[0], res[1])
        o_am.set_curr_img(img)
        o_ssm.set_corners(corners)
        o_am.initialize_pix_vals(o_ssm.get("curr_pts")); o_am.initialize_pix_grad_pts(o_ssm.get("curr_pts"))   # (they size It, dIt_dx)
        o_ssm.set_state(states[t])
        pts = o_ssm.get("curr_pts")
        x, y = pts.reshape(-1, 2)[:, 0], pts.reshape(-1, 2)[:, 1]
        o_am.update_pix_vals(pts); o_am.update_pix_grad_pts(pts)
        want = pix_val_np(img, x, y)
        np.testing.assert_allclose(o_am.get("It"), want, rtol=0, atol=1e-12, err_msg="target %d" % t)
        np.testing.assert_allclose(o_am.get("dIt_dx").reshape(2, -1).T, img_grad_np(img, x, y), rtol=0, atol=2 * 1e-12 / (2 * 1e-8),
                                   err_msg="target %d" % t)
        border = int((want == 128.0).sum())
        assert (border == 0) == (t == 0), (t, border)      # the inside patch never leaves the frame, every other one does
        n_border += border
        if t == 3:     # the right-border patch: most of it is INSIDE a frame 160 wide (it would be all border in one 96 wide)
            assert border < 0.5 * want.size
    assert n_border > 0
