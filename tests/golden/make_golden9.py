#!/usr/bin/env python
"""Generates tests/golden/lk_golden9.npz: the Localized Reversed SCV appearance model (LRSCV, AM/src/LRSCV.cc) from an independent float64
NumPy restatement of its definition, written from the maths below (the C++ oracle has no SCV family).

LRSCV normalises pixels as SCV does: v -> (n_bins - 1) / 255 * v; I0 is the normalised template.  The sub-regions and the per-pixel
weights are LSCV's (make_golden8.py: regions, weights -- the centre (start + end) / 2.0, the difference truncated toward zero,
1 / (1 + dx^2 + dy^2), each pixel's row divided by its sum taken idy outer, idx inner; a sub-region size <= 0 is refused).  Every
updatePixVals (LRSCV.cc:224-261):
  1. It_orig is sampled at the current warp; with once_per_frame and not the first iteration of a frame, It = It_orig and that is all;
  2. per sub-region r: the Dirac joint histogram of ((int)It_orig, (int)I0) over r's pixels, pre-seeds 0, and curr_hist_r, its rows' sums;
     map_r[b] = sum_j j joint_r(b, j) / curr_hist_r(b), and b where curr_hist_r(b) == 0;
  3. mapped_r = the WHOLE It_orig through map_r: affine_mapping: a_r It_orig + c_r with (a_r, c_r) the least-squares line
     map_r[k] ~ a k + c over k = 0 .. n_bins - 1; else nearest map_r[(int)rint(x)] or linear (make_golden6.remap);
  4. It = 0; It += mapped_r * w(pix, r) for r = idy n_x + idx in order (idy outer, idx inner -- not LSCV's idx-outer order), each product
     and each sum rounded;
then SSD on It: r = It - I0, f = -|r|^2 / 2, df/dIt = -r; the gradients (dIt/dx, Jt, J0) are those of the unmapped images.
`literal_maps` builds each sub-region's n_bins^2 histogram and fits with lstsq; `per_bin_maps` is the form the device computes (u32 sums of
(int)I0 and counts per (cell, current bin), the cells of each sub-region added, the closed-form affine fit); tests/test_lrscv_ref.py holds
them to each other.

Per case: config, corners, p, the weights (head rows), the maps, the affine parameters, heads (and for patches of at most FULL_MAX pixels
the whole) of It_orig, the blended It and df/dIt, f, g = df/dIt . Jt, H = -Jt^T Jt, and for the well-conditioned homography cases of at
least 2500 pixels the state update and the corners after 5 chained ESM (DiffOfJacs, SumOfSelf), 5 chained FCLK (CurrentSelf) and 5 ICLK
(InitialSelf) iterations from p, with the case's once_per_frame (the first iteration maps, the later ones run on the raw patch).
Well-conditioned: every method's fifth step below 0.5 in every parameter.  The image is make_golden7.py's (every non-zero texel moved by
+0.29, so that no flat region puts (int)It_orig on the rounding of the warp).

Run from the repo root:  python tests/golden/make_golden9.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import numpy_ref as R  # noqa: E402
from mtf_amd import synth  # noqa: E402
import make_golden5  # noqa: E402
import make_golden6  # noqa: E402
import make_golden7  # noqa: E402
import make_golden8  # noqa: E402

SEED = 20261018
HEAD = 16
FULL_MAX = 3600
N_ITERS = 5

# (tag, n_bins, resx, resy, n_x, n_y, s_x, s_y, affine_mapping, once_per_frame, weighted_mapping, affine SSM, corners)
CASES = (
    ("ship_50", 64, 50, 50, 3, 3, 10, 10, 1, 1, 0, False, synth.square_corners(64, 64, 70)),
    ("ship_200", 64, 200, 200, 3, 3, 10, 10, 1, 1, 0, False, synth.square_corners(128, 128, 150)),
    ("near_50", 64, 50, 50, 3, 3, 10, 10, 0, 0, 0, False, synth.square_corners(64, 64, 70)),
    ("lin_50", 64, 50, 50, 3, 3, 10, 10, 0, 0, 1, False, synth.square_corners(64, 64, 70)),
    ("n256_60", 256, 60, 60, 3, 3, 10, 10, 0, 0, 0, False, synth.square_corners(70, 190, 72)),
    ("gap_37x23", 64, 37, 23, 2, 3, 25, 9, 0, 0, 0, False, make_golden5._rect(164, 40, 222, 86)),
    ("aff_40", 64, 40, 40, 3, 3, 5, 5, 0, 0, 0, True, make_golden5._rect(160, 170, 226, 214)),
)

regions = make_golden8.regions
weights = make_golden8.weights
cells = make_golden8.cells
remap = make_golden6.remap


def _bins(v, nb):
    return np.clip(v.astype(np.int64), 0, nb - 1)


def _affine_fit_lstsq(maps):
    nb = maps.shape[1]
    A = np.column_stack([np.arange(nb, dtype=np.float64), np.ones(nb)])
    return np.array([np.linalg.lstsq(A, m, rcond=None)[0] for m in maps])


def literal_maps(It_orig, I0, nb, geo):
    """per sub-region (index idy nx + idx): the n_bins^2 Dirac joint histogram joint[(int)It_orig, (int)I0] over its pixels, curr_hist,
    the map, literally; the affine fits by lstsq"""
    resx, resy, nx, ny, sx, sy = geo
    rx, ry = regions(resx, resy, nx, ny, sx, sy)
    px, py = np.arange(resx * resy) % resx, np.arange(resx * resy) // resx
    maps = np.empty((nx * ny, nb))
    for idx in range(nx):
        for idy in range(ny):
            m = (px >= rx[idx][0]) & (px <= rx[idx][1]) & (py >= ry[idy][0]) & (py <= ry[idy][1])
            joint = np.zeros((nb, nb))
            np.add.at(joint, (_bins(It_orig[m], nb), _bins(I0[m], nb)), 1.0)
            curr_hist = joint.sum(axis=1)
            out = np.arange(nb, dtype=np.float64)
            for b in range(nb):
                if curr_hist[b] != 0:
                    wt_sum = 0.0
                    for j in range(nb):
                        wt_sum += j * joint[b, j]
                    out[b] = wt_sum / curr_hist[b]
            maps[idy * nx + idx] = out
    return maps, _affine_fit_lstsq(maps)


def per_bin_maps(It_orig, I0, nb, geo):
    """the device's form: integer sums of (int)I0 and counts per (cell, current bin), the cells of each sub-region added, the
    closed-form affine fit by the normal equations"""
    resx, resy, nx, ny, sx, sy = geo
    cx, rx, ncx = cells(resx, nx, sx)
    cy, ry, ncy = cells(resy, ny, sy)
    i = np.arange(resx * resy)
    c = np.where((cx[i % resx] >= 0) & (cy[i // resx] >= 0), cy[i // resx] * ncx + cx[i % resx], -1)
    ok = c >= 0
    s = np.zeros((ncx * ncy, nb), dtype=np.int64)
    n = np.zeros((ncx * ncy, nb), dtype=np.int64)
    np.add.at(s, (c[ok], _bins(It_orig[ok], nb)), _bins(I0[ok], nb))
    np.add.at(n, (c[ok], _bins(It_orig[ok], nb)), 1)
    s, n = s.reshape(ncy, ncx, nb), n.reshape(ncy, ncx, nb)
    maps, aff = np.empty((nx * ny, nb)), np.empty((nx * ny, 2))
    k = np.arange(nb, dtype=np.float64)
    N, Sk, Skk = float(nb), float(nb * (nb - 1) // 2), float((nb - 1) * nb * (2 * nb - 1) // 6)
    for idx in range(nx):
        for idy in range(ny):
            ss = s[ry[idy][0]:ry[idy][1] + 1, rx[idx][0]:rx[idx][1] + 1].sum(axis=(0, 1))
            nn = n[ry[idy][0]:ry[idy][1] + 1, rx[idx][0]:rx[idx][1] + 1].sum(axis=(0, 1))
            r = idy * nx + idx
            maps[r] = np.where(nn == 0, k, ss.astype(np.float64) / np.where(nn == 0, 1, nn).astype(np.float64))
            Sm, Skm = maps[r].sum(), (k * maps[r]).sum()
            det = N * Skk - Sk * Sk
            aff[r] = [(N * Skm - Sk * Sm) / det, (Skk * Sm - Sk * Skm) / det]
    return maps, aff


def mapped(It_orig, maps, aff, r, affine, linear):
    return aff[r][0] * It_orig + aff[r][1] if affine else remap(It_orig, maps[r], linear)


def blend(It_orig, maps, aff, w, nx, ny, affine, linear):
    """It = 0; It += mapped_r * w(pix, r) for r = idy nx + idx in order (LRSCV.cc:249-254)"""
    It = np.zeros_like(It_orig)
    for r in range(nx * ny):
        It = It + mapped(It_orig, maps, aff, r, affine, linear) * w[:, r]
    return It


def blend_lscv_order(It_orig, maps, aff, w, nx, ny, affine, linear):
    """the same sum in LSCV's order (idx outer, idy inner, LSCV.cc:268-299): NOT what LRSCV computes"""
    It = np.zeros_like(It_orig)
    for idx in range(nx):
        for idy in range(ny):
            It = It + mapped(It_orig, maps, aff, idy * nx + idx, affine, linear) * w[:, idy * nx + idx]
    return It


def lrscv_update(It_orig, I0, nb, geo, w, affine, linear, first_iter=True, once=False, form=literal_maps):
    """LRSCV::updatePixVals after the sampling: (maps, aff, It); maps and aff are None on the early return"""
    if once and not first_iter:
        return None, None, It_orig.copy()
    maps, aff = form(It_orig, I0, nb, geo)
    return maps, aff, blend(It_orig, maps, aff, w, geo[2], geo[3], affine, linear)


def lk_run(pa, W, nb, geo, w, affine, linear, once, method):
    """N_ITERS chained ESM (DiffOfJacs + SumOfSelf), FCLK (CurrentSelf) or ICLK (InitialSelf) SSD steps on the blended current patch;
    once_per_frame: the first iteration maps, the later ones run on the raw patch; the last dp and W"""
    for it in range(N_ITERS):
        It_orig, Jt = pa.sample(W)
        It = lrscv_update(It_orig, pa.I0o, nb, geo, w, affine, linear, first_iter=it == 0, once=once)[2]
        dft = -(It - pa.I0o)
        if method == "esm":
            g = 0.5 * (dft @ (pa.J0 + Jt))
            H = 0.5 * (-Jt.T @ Jt - pa.J0.T @ pa.J0)
        elif method == "fclk":
            g = dft @ Jt
            H = -Jt.T @ Jt
        else:
            g = (-dft) @ pa.J0
            H = -pa.J0.T @ pa.J0
        dp = -np.linalg.solve(H, g)
        W = make_golden7.inv_compose(W, dp) if method == "iclk" else R.compose_hom(W, dp)
    return dp, W


def main():
    rng = np.random.default_rng(SEED)
    img = make_golden7.make_image()
    out = {"img": img, "tags": np.array([c[0] for c in CASES])}
    n_track = 0
    for tag, nb, resx, resy, nx, ny, sx, sy, am, once, lin, affine, corners in CASES:
        if affine:
            p = rng.uniform(-1, 1, 6) * [1.2, 1.2, 0.02, 0.02, 0.02, 0.02]
        else:
            p = synth.random_small_homography(rng, 0.4)
        geo = (resx, resy, nx, ny, sx, sy)
        pa = make_golden6.Patch(img.astype(np.float64), nb, resx, resy, affine, corners)
        w = weights(*geo)
        W = pa.warp(p)
        It_orig, Jt = pa.sample(W)
        maps, aff, It = lrscv_update(It_orig, pa.I0o, nb, geo, w, am, lin)
        dft = -(It - pa.I0o)
        full = resx * resy <= FULL_MAX
        rec = {
            tag + "_cfg": np.array([nb, resx, resy, nx, ny, sx, sy, am, once, lin, int(affine)]), tag + "_corners": corners, tag + "_p": p,
            tag + "_w_head": w[:HEAD], tag + "_maps": maps, tag + "_aff": aff, tag + "_It_orig_head": It_orig[:HEAD],
            tag + "_It_head": It[:HEAD], tag + "_df_dIt_head": dft[:HEAD], tag + "_f": -0.5 * float(dft @ dft), tag + "_g": dft @ Jt,
            tag + "_H": -Jt.T @ Jt,
        }
        if full:
            rec[tag + "_It"] = It
            rec[tag + "_df_dIt"] = dft
        if not affine and resx * resy >= 2500:
            chm = np.vstack([corners, np.ones(4)])
            runs = {method: lk_run(pa, W, nb, geo, w, am, lin, once, method) for method in ("esm", "fclk", "iclk")}
            if all(np.abs(dp).max() < 0.5 for dp, _ in runs.values()):
                n_track += 1
                for method, (dp, Wn) in runs.items():
                    rec[tag + "_" + method + "_dp"] = dp
                    rec[tag + "_" + method + "_corners"] = make_golden6.corners_of(Wn, chm)
            else:
                print("no track record for", tag, [float(np.abs(dp).max()) for dp, _ in runs.values()])
        out.update(rec)
    assert n_track >= 2, "too few well-conditioned track cases"
    path = os.path.join(HERE, "lk_golden9.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
