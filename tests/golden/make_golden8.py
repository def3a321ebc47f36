#!/usr/bin/env python
"""Generates tests/golden/lk_golden8.npz: the Localized SCV appearance model (LSCV, AM/src/LSCV.cc) from an independent float64 NumPy
restatement of its definition, written from the maths below (the C++ oracle has no SCV family).

LSCV normalises pixels as SCV does: v -> (n_bins - 1) / 255 * v; I0_orig is the normalised template.  The patch (pixel i at
(i % resx, i / resx)) has n_x x n_y overlapping sub-regions: sub-region (idx, idy) covers x in [idx s_x, idx s_x + size_x - 1] with
size_x = resx - (n_x - 1) s_x (the same in y); size <= 0 is refused.  Per-pixel weights (LSCV.cc:170-197): the centre (start + end) / 2.0,
diff = (int)(pix - centre) truncated toward zero, w = 1 / (1 + diff_x^2 + diff_y^2), each pixel's row divided by its sum (taken idy outer,
idx inner).  Every updateSimilarity that runs (once_per_frame: the first iteration of a frame only):
  I0 = 0; for idx outer, idy inner: the Dirac joint histogram of ((int)It, (int)I0_orig) over the sub-region, map[b] = sum_i i joint(i, b)
  / init_hist(b) (b where init_hist(b) == 0), I0_mapped through it (affine_mapping: the least-squares line map[k] ~ a k + c over
  k = 0 .. n_bins - 1, I0_mapped = a I0_orig + c; else nearest map[(int)rint(x)] or linear), I0 += I0_mapped * w(pix, region);
then SSD on the re-mapped I0: r = It - I0, f = -|r|^2 / 2, df/dIt = -r.  J0 and dI0/dx stay the original template's.
`literal_maps` builds each sub-region's n_bins^2 histogram and fits with lstsq; `per_bin_maps` is the form the device computes (u32
sums per (cell, bin), cells added per sub-region, the closed-form affine fit); tests/test_lscv_ref.py holds them to each other.

Per case: config, corners, p, the weights (head rows), the maps, the affine parameters, heads (and for small patches the whole) of the
re-mapped I0 and df/dIt, f, g = df/dIt . Jt, H = -Jt^T Jt, and for the homography cases the state update and the corners after 5 chained
ESM (DiffOfJacs, SumOfSelf) and 5 chained FCLK (CurrentSelf) iterations from p, with the case's once_per_frame (not for the
37 x 23 gap case, whose first steps move 8 px: the 5-iteration run is ill-conditioned).  The image is
make_golden6.py's (make_golden5.py's with the high saturated block at 254).

Run from the repo root:  python tests/golden/make_golden8.py
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

SEED = 20261017
HEAD = 16
FULL_MAX = 3600
N_ITERS = 5

# (tag, n_bins, resx, resy, n_x, n_y, s_x, s_y, affine_mapping, once_per_frame, weighted_mapping, affine SSM, corners)
CASES = (
    ("ship_50", 64, 50, 50, 3, 3, 10, 10, 1, 1, 0, False, make_golden5._rect(40, 40, 104, 104)),
    ("ship_200", 64, 200, 200, 3, 3, 10, 10, 1, 1, 0, False, synth.square_corners(128, 128, 150)),
    ("near_50", 64, 50, 50, 3, 3, 10, 10, 0, 0, 0, False, synth.square_corners(64, 64, 70)),
    ("lin_50", 64, 50, 50, 3, 3, 10, 10, 0, 0, 1, False, synth.square_corners(64, 64, 70)),
    ("n256_60", 256, 60, 60, 3, 3, 10, 10, 0, 0, 0, False, synth.square_corners(70, 190, 72)),
    ("gap_37x23", 64, 37, 23, 2, 3, 25, 9, 0, 0, 0, False, make_golden5._rect(164, 40, 222, 86)),
    ("aff_40", 64, 40, 40, 3, 3, 5, 5, 0, 0, 0, True, make_golden5._rect(160, 170, 226, 214)),
)


def regions(resx, resy, nx, ny, sx, sy):
    """[(x0, x1)] * nx, [(y0, y1)] * ny, inclusive (LSCV.cc:146-167); ValueError where the reference throws"""
    size_x, size_y = resx - (nx - 1) * sx, resy - (ny - 1) * sy
    if size_x <= 0 or size_y <= 0:
        raise ValueError("LSCV :: Patch size : %dx%d is not enough to use the specified region spacing and / or count" % (resx, resy))
    return [(i * sx, i * sx + size_x - 1) for i in range(nx)], [(j * sy, j * sy + size_y - 1) for j in range(ny)]


def weights(resx, resy, nx, ny, sx, sy):
    """sub_region_wts: [n_pix, nx ny], column idy nx + idx"""
    rx, ry = regions(resx, resy, nx, ny, sx, sy)
    n = resx * resy
    px = (np.arange(n) % resx).astype(np.float64)
    py = (np.arange(n) // resx).astype(np.float64)
    w = np.empty((n, nx * ny))
    s = np.zeros(n)
    for idy in range(ny):
        cy = float(ry[idy][0] + ry[idy][1]) / 2.0
        for idx in range(nx):
            cx = float(rx[idx][0] + rx[idx][1]) / 2.0
            dx = np.trunc(px - cx).astype(np.int64)
            dy = np.trunc(py - cy).astype(np.int64)
            pw = 1.0 / (1.0 + dx * dx + dy * dy)
            w[:, idy * nx + idx] = pw
            s = s + pw
    return w / s[:, None]


def _region_mask(resx, resy, x, y):
    px, py = np.arange(resx * resy) % resx, np.arange(resx * resy) // resx
    return (px >= x[0]) & (px <= x[1]) & (py >= y[0]) & (py <= y[1])


def _bins(v, nb):
    return np.clip(v.astype(np.int64), 0, nb - 1)


def literal_maps(It, I0o, nb, geo):
    """per sub-region (index idy nx + idx): the n_bins^2 Dirac joint histogram, init_hist and the map; the affine fits by lstsq"""
    resx, resy, nx, ny, sx, sy = geo
    rx, ry = regions(resx, resy, nx, ny, sx, sy)
    maps, aff = np.empty((nx * ny, nb)), np.empty((nx * ny, 2))
    A = np.column_stack([np.arange(nb, dtype=np.float64), np.ones(nb)])
    for idx in range(nx):
        for idy in range(ny):
            m = _region_mask(resx, resy, rx[idx], ry[idy])
            joint = np.zeros((nb, nb))
            np.add.at(joint, (_bins(It[m], nb), _bins(I0o[m], nb)), 1.0)
            init_hist = joint.sum(axis=0)
            wt = np.arange(nb, dtype=np.float64) @ joint
            r = idy * nx + idx
            maps[r] = np.where(init_hist == 0, np.arange(nb, dtype=np.float64), wt / np.where(init_hist == 0, 1, init_hist))
            aff[r] = np.linalg.lstsq(A, maps[r], rcond=None)[0]
    return maps, aff


def cells(res, n, spacing):
    """the cell of every coordinate of one axis (-1 outside every sub-region) and the cell range of every sub-region"""
    size = res - (n - 1) * spacing
    cell, rng, key, nc = np.full(res, -1), np.full((n, 2), -1), None, 0
    for v in range(res):
        inside = [k for k in range(n) if k * spacing <= v <= k * spacing + size - 1]
        if not inside:
            continue
        if (inside[0], inside[-1]) != key:
            key, nc = (inside[0], inside[-1]), nc + 1
        cell[v] = nc - 1
        for k in inside:
            rng[k] = [nc - 1 if rng[k][0] < 0 else rng[k][0], nc - 1]
    return cell, rng, nc


def per_bin_maps(It, I0o, nb, geo):
    """the device's form: integer sums of (int)It and counts per (cell, template bin), the cells of each sub-region added, the
    closed-form affine fit by the normal equations"""
    resx, resy, nx, ny, sx, sy = geo
    cx, rx, ncx = cells(resx, nx, sx)
    cy, ry, ncy = cells(resy, ny, sy)
    i = np.arange(resx * resy)
    c = np.where((cx[i % resx] >= 0) & (cy[i // resx] >= 0), cy[i // resx] * ncx + cx[i % resx], -1)
    ok = c >= 0
    s = np.zeros((ncx * ncy, nb), dtype=np.int64)
    n = np.zeros((ncx * ncy, nb), dtype=np.int64)
    np.add.at(s, (c[ok], _bins(I0o[ok], nb)), _bins(It[ok], nb))
    np.add.at(n, (c[ok], _bins(I0o[ok], nb)), 1)
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


def blend(I0o, maps, aff, w, nx, ny, affine, linear):
    """I0 = sum over idx (outer), idy (inner) of I0_mapped * w, each product rounded"""
    I0 = np.zeros_like(I0o)
    for idx in range(nx):
        for idy in range(ny):
            r = idy * nx + idx
            mapped = aff[r][0] * I0o + aff[r][1] if affine else make_golden6.remap(I0o, maps[r], linear)
            I0 = I0 + mapped * w[:, r]
    return I0


def lscv_update(It, I0o, nb, geo, w, affine, linear, form=literal_maps):
    maps, aff = form(It, I0o, nb, geo)
    I0 = blend(I0o, maps, aff, w, geo[2], geo[3], affine, linear)
    return maps, aff, I0


def lk_run(pa, W, nb, geo, w, affine, linear, once, method):
    """N_ITERS chained ESM (DiffOfJacs + SumOfSelf) or FCLK (CurrentSelf) SSD steps on the re-mapped template; once_per_frame: the
    template re-mapped at the first iteration only"""
    I0 = None
    for it in range(N_ITERS):
        It, Jt = pa.sample(W)
        if I0 is None or not once:
            I0 = lscv_update(It, pa.I0o, nb, geo, w, affine, linear)[2]
        dft = -(It - I0)
        if method == "esm":
            g = 0.5 * (dft @ (pa.J0 + Jt))
            H = 0.5 * (-Jt.T @ Jt - pa.J0.T @ pa.J0)
        else:
            g = dft @ Jt
            H = -Jt.T @ Jt
        dp = -np.linalg.solve(H, g)
        W = R.compose_hom(W, dp)
    return dp, W


def golden_image():
    img = make_golden5.make_image()
    img[img == 255.0] = 254.0   # (make_golden6.py's fixture image: see its main())
    return img


def main():
    rng = np.random.default_rng(SEED)
    img = golden_image()
    out = {"img": img, "tags": np.array([c[0] for c in CASES])}
    for tag, nb, resx, resy, nx, ny, sx, sy, am, once, lin, affine, corners in CASES:
        if affine:
            p = rng.uniform(-1, 1, 6) * [1.2, 1.2, 0.02, 0.02, 0.02, 0.02]
        else:
            p = synth.random_small_homography(rng, 0.4)
        geo = (resx, resy, nx, ny, sx, sy)
        pa = make_golden6.Patch(img.astype(np.float64), nb, resx, resy, affine, corners)
        w = weights(*geo)
        W = pa.warp(p)
        It, Jt = pa.sample(W)
        maps, aff, I0 = lscv_update(It, pa.I0o, nb, geo, w, am, lin)
        dft = -(It - I0)
        full = resx * resy <= FULL_MAX
        rec = {
            tag + "_cfg": np.array([nb, resx, resy, nx, ny, sx, sy, am, once, lin, int(affine)]), tag + "_corners": corners, tag + "_p": p,
            tag + "_w_head": w[:HEAD], tag + "_maps": maps, tag + "_aff": aff, tag + "_I0o_head": pa.I0o[:HEAD], tag + "_I0_head": I0[:HEAD],
            tag + "_df_dIt_head": dft[:HEAD], tag + "_f": -0.5 * float(dft @ dft), tag + "_g": dft @ Jt, tag + "_H": -Jt.T @ Jt,
        }
        if full:
            rec[tag + "_I0"] = I0
            rec[tag + "_df_dIt"] = dft
        if not affine and resx * resy >= 2500:   # (37 x 23: its first steps move 8 px; the 5-iteration run is ill-conditioned)
            chm = np.vstack([corners, np.ones(4)])
            for method in ("esm", "fclk"):
                dp, Wn = lk_run(pa, W, nb, geo, w, am, lin, once, method)
                rec[tag + "_" + method + "_dp"] = dp
                rec[tag + "_" + method + "_corners"] = make_golden6.corners_of(Wn, chm)
        out.update(rec)
    path = os.path.join(HERE, "lk_golden8.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
