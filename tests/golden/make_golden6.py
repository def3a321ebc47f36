#!/usr/bin/env python
"""Generates tests/golden/lk_golden6.npz: the Sum of Conditional Variance appearance model (SCV, AM/src/SCV.cc) from an independent
float64 NumPy restatement of its definition, written from the maths below (the C++ oracle has no SCV).

SCV normalises pixels as MI does but over PIX_MAX - PIX_MIN = 255: v -> (n_bins - 1) / 255 * v.  I0_orig is the normalised template.
Every updateSimilarity:
  1. the joint histogram of (It, I0_orig), n_bins x n_bins, no pre-seed -- Dirac: joint((int)It, (int)I0_orig) += 1; Bilinear: the
     four-cell split of getBilinearJointHist with its r_wt != 0 / b_wt != 0 guards -- and init_hist, the histogram of I0_orig;
  2. map[b] = sum_i i joint(i, b) / init_hist(b), and map[b] = b where init_hist(b) == 0;
  3. I0 = map(I0_orig): nearest map[(int)rint(x)], or linear (1 - dx) map[lx] + dx map[lx + 1] (dx == 0: map[lx]);
  4. SSD on the re-mapped I0: r = It - I0, f = -|r|^2 / 2, df/dIt = -r; J0 and dI0/dx stay the original template's.
`literal_map` builds the n_bins^2 histogram itself; `per_bin_map` is the two-sums-per-bin form the device computes (tests/test_scv_ref.py
holds them to each other).

Per case: config, corners, p, the map, heads (and for small patches the whole) of I0_orig, re-mapped I0 and df/dIt, f, g = df/dIt . Jt,
H_curr = H_self = -Jt^T Jt (SSD's current and first-order self Hessians), and for the homography cases of 64 bins and more the state update and the corners
after 5 chained ESM (DiffOfJacs, SumOfSelf) and 5 chained FCLK (CurrentSelf) iterations from p.  The image is make_golden5.py's (regions
saturated at 0 and 255 -- the latter moved to 254, see main() -- so that bins are empty and the map[b] = b rule is hit, a low-contrast ramp
and texture) and is stored in the file.

Run from the repo root:  python tests/golden/make_golden6.py
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

SEED = 20261016
HEAD = 16
FULL_MAX = 3600      # patches up to this many pixels store their whole I0 and df/dIt
N_ITERS = 5

# (tag, hist_type 0 Dirac / 1 Bilinear, n_bins, weighted_mapping, resx, resy, affine, corners)
CASES = (
    ("d64n_50", 0, 64, 0, 50, 50, False, synth.square_corners(64, 64, 70)),
    ("d64n_200", 0, 64, 0, 200, 200, False, synth.square_corners(128, 128, 150)),
    ("d256n_60", 0, 256, 0, 60, 60, False, synth.square_corners(70, 190, 72)),
    ("d7n_37x23", 0, 7, 0, 37, 23, False, make_golden5._rect(164, 40, 222, 86)),
    ("b64n_50", 1, 64, 0, 50, 50, False, synth.square_corners(64, 64, 70)),
    ("b64l_50", 1, 64, 1, 50, 50, False, synth.square_corners(64, 64, 70)),
    ("d64n_aff", 0, 64, 0, 40, 40, True, make_golden5._rect(160, 170, 226, 214)),
)


def pix_mult(n_bins):
    """SCV's pixel normalisation (hist types Dirac / Bilinear): [0, 255] -> [0, n_bins - 1]"""
    return (n_bins - 1.0) / 255.0


def literal_map(It, I0o, n_bins, hist_type):
    """the joint histogram joint[i_t, i_0] and init_hist, then the map, literally"""
    joint = np.zeros((n_bins, n_bins))
    init_hist = np.zeros(n_bins)
    for k in range(It.size):
        pt, p0 = int(It[k]), int(I0o[k])
        if hist_type == 0:
            joint[pt, p0] += 1
            init_hist[p0] += 1
            continue
        r_wt = It[k] - pt
        l_wt = 1.0 - r_wt
        b_wt = I0o[k] - p0
        t_wt = 1 - b_wt
        init_hist[p0] += t_wt
        joint[pt, p0] += l_wt * t_wt
        # (a bilinear sample of a region saturated at 255 can come out a few ulps above 255, i.e. above n_bins - 1 once normalised: the
        # reference's guards then index one past its histograms; the cells past the last bin are dropped here, as on the device)
        up_t, up_0 = r_wt != 0 and pt + 1 < n_bins, b_wt != 0 and p0 + 1 < n_bins
        if up_t:
            joint[pt + 1, p0] += r_wt * t_wt
            if up_0:
                joint[pt + 1, p0 + 1] += r_wt * b_wt
        if up_0:
            init_hist[p0 + 1] += b_wt
            joint[pt, p0 + 1] += l_wt * b_wt
    out = np.arange(n_bins, dtype=np.float64)
    for b in range(n_bins):
        if init_hist[b] != 0:
            wt_sum = 0.0
            for i in range(n_bins):
                wt_sum += i * joint[i, b]
            out[b] = wt_sum / init_hist[b]
    return out


def per_bin_map(It, I0o, n_bins, hist_type):
    """the same map from two sums per template bin: sum of (int)It (Dirac) or of the bin weight times It (Bilinear), and the weight"""
    s = np.zeros(n_bins)
    w = np.zeros(n_bins)
    b0 = I0o.astype(np.int64)
    if hist_type == 0:
        np.add.at(s, b0, np.trunc(It))
        np.add.at(w, b0, 1.0)
    else:
        b_wt = I0o - b0
        t_wt = 1 - b_wt
        np.add.at(s, b0, t_wt * It)
        np.add.at(w, b0, t_wt)
        nz = (b_wt != 0) & (b0 + 1 < n_bins)
        np.add.at(s, b0[nz] + 1, b_wt[nz] * It[nz])
        np.add.at(w, b0[nz] + 1, b_wt[nz])
    out = np.arange(n_bins, dtype=np.float64)
    ok = w != 0
    out[ok] = s[ok] / w[ok]
    return out


def remap(I0o, m, linear):
    if not linear:
        return m[np.rint(I0o).astype(np.int64)]
    lx = I0o.astype(np.int64)
    dx = I0o - lx
    hi = np.minimum(lx + 1, m.size - 1)
    return np.where(dx == 0, m[lx], (1 - dx) * m[lx] + dx * m[hi])


class Patch:
    """the sample grid of one target and its template quantities"""

    def __init__(self, img, n_bins, resx, resy, affine, corners):
        self.img, self.affine, self.mult = img, affine, pix_mult(n_bins)
        self.init_pts, self.init_hm = R.grid_from_corners(corners, resx, resy, affine=affine)
        x, y = self.init_pts
        self.I0o = self.mult * R.bilinear(img, x, y)
        g0 = R.img_grad(img, self.init_pts, mult=self.mult)
        if affine:
            self.P = R.aff_param_jacobian(x, y)
            self.J0 = R.sd_rows_direct(g0, self.P)
        else:
            self.P = R.hom_param_jacobian(x, y)
            self.J0 = R.sd_rows_chained(g0, R.hom_spatial_jacobian(np.eye(3), self.init_pts, self.init_hm[2]), self.P)

    def warp(self, p):
        return R.aff_matrix(p) if self.affine else R.hom_matrix(p)

    def sample(self, W):
        """It and Jt at the warp W (chained: the image gradient at the warped points through dW/dx)"""
        if self.affine:
            x, y = self.init_pts
            wpts = (W @ np.vstack([x, y, np.ones_like(x)]))[:2]
            sj = np.broadcast_to(W[:2, :2], (x.size, 2, 2))
        else:
            wpts, q = R.warp_pts(W, self.init_hm)
            sj = R.hom_spatial_jacobian(W, wpts, q[2])
        It = self.mult * R.bilinear(self.img, wpts[0], wpts[1])
        Jt = R.sd_rows_chained(R.img_grad(self.img, wpts, mult=self.mult), sj, self.P)
        return It, Jt


def scv_update(It, I0o, n_bins, hist_type, linear):
    m = literal_map(It, I0o, n_bins, hist_type)
    I0 = remap(I0o, m, linear)
    r = It - I0
    return m, I0, -0.5 * float(r @ r), -r


def lk_run(pa, W, n_bins, hist_type, linear, method):
    """N_ITERS chained ESM (DiffOfJacs + SumOfSelf) or FCLK (CurrentSelf) SSD steps on the re-mapped template; the last dp and W"""
    for _ in range(N_ITERS):
        It, Jt = pa.sample(W)
        _, _, _, dft = scv_update(It, pa.I0o, n_bins, hist_type, linear)
        if method == "esm":
            g = 0.5 * (dft @ (pa.J0 + Jt))
            H = 0.5 * (-Jt.T @ Jt - pa.J0.T @ pa.J0)
        else:
            g = dft @ Jt
            H = -Jt.T @ Jt
        dp = -np.linalg.solve(H, g)
        W = R.compose_hom(W, dp)
    return dp, W


def corners_of(W, corners_hm):
    q = W @ corners_hm
    return q[:2] / q[2]


def main():
    rng = np.random.default_rng(SEED)
    img = make_golden5.make_image()
    # The high saturated block is put at 254, not 255.  The bilinear interpolant of a region at exactly 255 lands a few ulps either side
    # of 255, i.e. of n_bins - 1 once normalised, so (int)It there is decided by the rounding of the warp (in the reference as well) and no
    # independent restatement can pin it.  The block at 0 stays: a flat 0 samples to exactly 0.
    img[img == 255.0] = 254.0
    out = {"img": img, "tags": np.array([c[0] for c in CASES])}
    for tag, ht, nb, lin, resx, resy, affine, corners in CASES:
        if affine:
            p = rng.uniform(-1, 1, 6) * [1.2, 1.2, 0.02, 0.02, 0.02, 0.02]
        else:
            p = synth.random_small_homography(rng, 0.4)
        pa = Patch(img.astype(np.float64), nb, resx, resy, affine, corners)
        W = pa.warp(p)
        It, Jt = pa.sample(W)
        m, I0, f, dft = scv_update(It, pa.I0o, nb, ht, lin)
        assert np.any(m == np.arange(nb)), tag   # (an empty bin or a fixed point: the saturated regions leave most bins empty)
        full = resx * resy <= FULL_MAX
        rec = {
            tag + "_cfg": np.array([ht, nb, lin, resx, resy, int(affine)]), tag + "_corners": corners, tag + "_p": p,
            tag + "_map": m, tag + "_I0o_head": pa.I0o[:HEAD], tag + "_I0_head": I0[:HEAD], tag + "_df_dIt_head": dft[:HEAD],
            tag + "_f": f, tag + "_g": dft @ Jt, tag + "_H_curr": -Jt.T @ Jt, tag + "_H_self": -Jt.T @ Jt,
        }
        if full:
            rec[tag + "_I0"] = I0
            rec[tag + "_df_dIt"] = dft
        if not affine and nb >= 64:   # (7 bins on the ramp: the first ESM step moves 26 px; the 5-iteration run is ill-conditioned)
            chm = np.vstack([corners, np.ones(4)])
            for method in ("esm", "fclk"):
                dp, Wn = lk_run(pa, W, nb, ht, lin, method)
                rec[tag + "_" + method + "_dp"] = dp
                rec[tag + "_" + method + "_corners"] = corners_of(Wn, chm)
        out.update(rec)
    path = os.path.join(HERE, "lk_golden6.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
