#!/usr/bin/env python
"""Generates tests/golden/lk_golden5.npz: MI at the shipped configuration (10 bins, partition of unity, Config/modules.cfg:115-117) and at
the other bin counts the ten-class kernels serve, from the independent NumPy definitions of oracle/numpy_ref.py.

lk_golden.npz / lk_golden2.npz pin MI at 8 bins without partition of unity only.  The cases here are chosen for the edges of the
ten-class pass-2 kernels: an image region saturated at 0 and 255 (a flat 0 samples to exactly 0, so the stored value is exactly 1.0
with partition of unity -- phi = 0 at a class boundary -- and exactly 0.0 without, the truncated window at bin 0), a ramp that
occupies only two or three classes (the class sort meets empty classes), ordinary texture, ragged pixel counts (37 x 23) and a
100 x 100 patch that spans several workgroups.  The image is stored in the file, so that every test loads exactly what was used here.

Per case: corners, p, heads of I0n / Itn, f, the head of df/dIt, g_curr = df_dIt . Jt, H_curr (cmptCurrHessian(Jt)),
H_init (cmptInitHessian(J0) at p), H_init0 (the same at the template state, It = I0: the constant Hessian init_template keeps) and
H_self1 (first-order cmptSelfHessian(Jt)).

Run from the repo root:  python tests/golden/make_golden5.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy_ref as R  # noqa: E402
from mtf_amd import synth  # noqa: E402

SEED = 20261015
IMG_SEED = 515
IMG_SHAPE = (256, 256)
HEAD = 16

# (tag, n_bins, pou, resx, resy, affine, corners): the rows of the issue's table plus two more 10-bin / pou / 40 x 40 cases, so that one
# batch can hold three targets of the shipped configuration on three different regions
def _rect(x0, y0, x1, y1, jitter=0.37):
    return np.array([[x0, x1, x1, x0], [y0, y0, y1, y1]], dtype=np.float64) + jitter


CASES = (
    ("b10p_sat", 10, 1, 40, 40, False, synth.square_corners(64, 64, 70)),
    ("b10p_low", 10, 1, 40, 40, False, synth.square_corners(192, 64, 64)),
    ("b10p_tex", 10, 1, 40, 40, False, synth.square_corners(70, 190, 72)),
    ("b10n_sat", 10, 0, 40, 40, False, synth.square_corners(64, 64, 70)),
    ("b9p_low", 9, 1, 37, 23, False, _rect(164, 40, 222, 86)),
    ("b5n_tex", 5, 0, 37, 23, True, _rect(160, 170, 226, 214)),
    ("b10p_big", 10, 1, 100, 100, False, synth.square_corners(128, 128, 150)),
)


def make_image():
    """synth.make_frame with a saturated block pair, a ramp of a few classes and the texture elsewhere (float32)"""
    img = synth.make_frame(*IMG_SHAPE, seed=IMG_SEED).astype(np.float64)
    img[20:62, 20:58] = 0.0                                 # saturated low: top-left of the b10*_sat patches
    img[66:110, 70:110] = 255.0                             # saturated high: bottom-right of them
    yy, xx = np.meshgrid(np.arange(IMG_SHAPE[0], dtype=np.float64), np.arange(IMG_SHAPE[1], dtype=np.float64), indexing="ij")
    ramp = 80.0 + 0.8 * (xx - 140.0) + 0.3 * (yy - 10.0) + 3.0 * np.sin(xx / 5.0) * np.cos(yy / 7.0)
    sel = (yy >= 10) & (yy < 120) & (xx >= 140) & (xx < 250)
    img[sel] = ramp[sel]                                    # low contrast: ~70 levels over the b*_low patches, two or three classes
    return np.clip(img, 0.0, 255.0).astype(np.float32)


def mi_case(img, nb, pou, resx, resy, affine, corners, p):
    mult, add = R.mi_pix_norm(nb, pou)
    init_pts, init_hm = R.grid_from_corners(corners, resx, resy, affine=affine)
    x, y = init_pts
    I0n = mult * R.bilinear(img, x, y) + add
    g0 = R.img_grad(img, init_pts, mult=mult)
    if affine:
        P = R.aff_param_jacobian(x, y)
        A = R.aff_matrix(p)
        wpts = (A @ np.vstack([x, y, np.ones_like(x)]))[:2]
        J0 = R.sd_rows_direct(g0, P)
        Jt = R.sd_rows_chained(R.img_grad(img, wpts, mult=mult), np.broadcast_to(A[:2, :2], (x.size, 2, 2)), P)
    else:
        Pj = R.hom_param_jacobian(x, y)
        J0 = R.sd_rows_chained(g0, R.hom_spatial_jacobian(np.eye(3), init_pts, init_hm[2]), Pj)
        W = R.hom_matrix(p)
        wpts, q = R.warp_pts(W, init_hm)
        Jt = R.sd_rows_chained(R.img_grad(img, wpts, mult=mult), R.hom_spatial_jacobian(W, wpts, q[2]), Pj)
    Itn = mult * R.bilinear(img, wpts[0], wpts[1]) + add
    f = R.mi_similarity(I0n, Itn, nb)
    dft = R.mi_curr_grad(I0n, Itn, nb)
    g = dft @ Jt
    S = Jt.shape[1]
    # the analytic gradient against a directional central difference of the definition.  Only with partition of unity: without it the
    # windows truncated at the edge bins no longer sum to one, the template's marginal is no longer the row sum of the joint histogram,
    # and the reference's 1 + log h - log h_c (MI.cc:426-442) is not the exact derivative of f -- it is still what the fixture pins
    for s_ in range(S if pou else 0):
        h = 1e-4 / np.abs(Jt[:, s_]).max()
        fd = (R.mi_similarity(I0n, Itn + h * Jt[:, s_], nb) - R.mi_similarity(I0n, Itn - h * Jt[:, s_], nb)) / (2 * h)
        assert abs(fd - g[s_]) <= 1e-6 * max(abs(g[s_]), np.abs(g).max() * 1e-3), (s_, fd, g[s_])
    H_init0 = R.mi_init_hessian(I0n, I0n, J0, nb)
    # at It = I0 the init and the self Hessian are one quantity, written two ways (template roles / current roles)
    H_s0 = R.mi_self_hessian2(I0n, J0, np.zeros((x.size, S, S)), nb)
    assert np.linalg.norm(H_init0 - H_s0) <= 1e-12 * np.linalg.norm(H_s0)
    return dict(I0n=I0n, Itn=Itn, f=f, dft=dft, g=g, J0=J0, Jt=Jt,
                H_curr=R.mi_curr_hessian(I0n, Itn, Jt, nb), H_init=R.mi_init_hessian(I0n, Itn, J0, nb), H_init0=H_init0,
                H_self1=R.mi_self_hessian2(Itn, Jt, np.zeros((x.size, S, S)), nb))


def main():
    rng = np.random.default_rng(SEED)
    img = make_image()
    out = {"img": img, "tags": np.array([c[0] for c in CASES])}
    for tag, nb, pou, resx, resy, affine, corners in CASES:
        if affine:
            p = rng.uniform(-1, 1, 6) * [1.2, 1.2, 0.02, 0.02, 0.02, 0.02]
        else:
            p = synth.random_small_homography(rng, 0.4)
        m = mi_case(img, nb, pou, resx, resy, affine, corners, p)
        out.update({
            tag + "_cfg": np.array([nb, pou, resx, resy, int(affine)]), tag + "_corners": corners, tag + "_p": p,
            tag + "_I0n_head": m["I0n"][:HEAD], tag + "_Itn_head": m["Itn"][:HEAD],
            tag + "_f": m["f"], tag + "_df_dIt_head": m["dft"][:HEAD], tag + "_g_curr": m["g"],
            tag + "_H_curr": m["H_curr"], tag + "_H_init": m["H_init"], tag + "_H_init0": m["H_init0"], tag + "_H_self1": m["H_self1"],
        })
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lk_golden5.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
