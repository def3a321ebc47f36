#!/usr/bin/env python
"""Generates tests/golden/lk_golden7.npz: the Reversed SCV appearance model (RSCV, AM/src/RSCV.cc) from an independent float64 NumPy
restatement of its definition, written from the maths below (the C++ oracle has no RSCV).

RSCV normalises pixels as SCV does: v -> (n_bins - 1) / 255 * v.  I0 is the normalised template.  Every updatePixVals:
  1. It_orig is sampled at the current warp;
  2. the Dirac joint histogram of (It_orig, I0), n_bins x n_bins, no pre-seed: joint((int)It_orig, (int)I0) += 1, and curr_hist, the
     histogram of It_orig (histUtils.cc:370-394);
  3. map[b] = sum_j j joint(b, j) / curr_hist(b), and map[b] = b where curr_hist(b) == 0 (RSCV.cc:211-229);
  4. It = map(It_orig): nearest map[(int)rint(x)], or linear (1 - dx) map[lx] + dx map[lx + 1] (dx == 0: map[lx]) (imgUtils.h:682-703);
  5. SSD on the mapped It: r = It - I0, f = -|r|^2 / 2, df/dIt = -r; the gradients (dIt/dx, Jt, J0) are those of the unmapped images.
`literal_map` builds the n_bins^2 histogram itself; `per_bin_map` is the two-sums-per-current-bin form the device computes
(tests/test_rscv_ref.py holds them to each other).

Per case: config, corners, p, the map, the head of It_orig, heads (and for patches of at most FULL_MAX pixels the whole) of the
mapped It and df/dIt, f, g = df/dIt . Jt, H_curr = H_self = -Jt^T Jt, and for the well-conditioned homography cases the state update
and the corners after 5 chained ESM (DiffOfJacs, SumOfSelf), 5 chained FCLK (CurrentSelf) and 5 ICLK (InitialSelf) iterations from p.
Well-conditioned: 64 bins or more, and every method's fifth step below 0.5 in every parameter (with nearest mapping at 64 bins the
50 x 50 patch, whose map jumps across the saturated blocks, still takes steps of 0.8 - 5 at the fifth iteration).

The image is make_golden5.py's (regions saturated at 0 and 255, a low-contrast ramp and texture) with every non-zero texel moved by a
fraction (+0.29, the saturated block to 254.71): a flat region, or a sample on integer coordinates, that normalised to a whole number
would put (int)It_orig on the rounding of the warp (at 256 bins every integer texel does, at 64 bins every multiple of 85).  The flat 0
block samples to exactly 0, which is safe.  The image is stored in the file.

Run from the repo root:  python tests/golden/make_golden7.py
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
import make_golden6  # noqa: E402  (its Patch: the sample grid, the normalised samples and the steepest-descent rows)

SEED = 20261017
HEAD = 16
FULL_MAX = 3600      # patches up to this many pixels store their whole It and df/dIt
N_ITERS = 5

# (tag, n_bins, weighted_mapping, resx, resy, affine, corners)
CASES = (
    ("r64n_50", 64, 0, 50, 50, False, synth.square_corners(64, 64, 70)),
    ("r64l_50", 64, 1, 50, 50, False, synth.square_corners(64, 64, 70)),
    ("r256n_60", 256, 0, 60, 60, False, synth.square_corners(70, 190, 72)),
    ("r7n_37x23", 7, 0, 37, 23, False, make_golden5._rect(164, 40, 222, 86)),
    ("r64n_aff", 64, 0, 40, 40, True, make_golden5._rect(160, 170, 226, 214)),
    ("r64n_200", 64, 0, 200, 200, False, synth.square_corners(128, 128, 150)),
)


def make_image():
    img = make_golden5.make_image().astype(np.float64)
    nz = img > 0
    img[nz] = np.minimum(img[nz] + 0.29, 254.71)
    return img.astype(np.float32)


def literal_map(It_orig, I0, n_bins):
    """the joint histogram joint[(int)It_orig, (int)I0] and curr_hist, then the map, literally"""
    joint = np.zeros((n_bins, n_bins))
    curr_hist = np.zeros(n_bins)
    for k in range(It_orig.size):
        pt, p0 = int(It_orig[k]), int(I0[k])
        curr_hist[pt] += 1
        joint[pt, p0] += 1
    out = np.arange(n_bins, dtype=np.float64)
    for b in range(n_bins):
        if curr_hist[b] != 0:
            wt_sum = 0.0
            for j in range(n_bins):
                wt_sum += j * joint[b, j]
            out[b] = wt_sum / curr_hist[b]
    return out


def per_bin_map(It_orig, I0, n_bins):
    """the same map from two integer sums per current bin: the sum of (int)I0 over the pixels of bin (int)It_orig, and their count"""
    bt = np.clip(It_orig.astype(np.int64), 0, n_bins - 1)
    s = np.zeros(n_bins, dtype=np.int64)
    c = np.zeros(n_bins, dtype=np.int64)
    np.add.at(s, bt, np.clip(I0.astype(np.int64), 0, n_bins - 1))
    np.add.at(c, bt, 1)
    out = np.arange(n_bins, dtype=np.float64)
    ok = c != 0
    out[ok] = s[ok].astype(np.float64) / c[ok].astype(np.float64)
    return out


remap = make_golden6.remap      # nearest map[(int)rint(x)] / linear, the indices clamped to [0, n_bins - 1]
Patch = make_golden6.Patch


def rscv_update(It_orig, I0, n_bins, linear):
    m = literal_map(It_orig, I0, n_bins)
    It = remap(It_orig, m, linear)
    r = It - I0
    return m, It, -0.5 * float(r @ r), -r


def inv_compose(W, dp):
    """ICLK's update: the inverse of the step composed onto the warp (invertState + compositionalUpdate)"""
    Wn = W @ np.linalg.inv(R.hom_matrix(dp))
    return Wn / Wn[2, 2]


def lk_run(pa, W, n_bins, linear, method):
    """N_ITERS chained ESM (DiffOfJacs + SumOfSelf), FCLK (CurrentSelf) or ICLK (InitialSelf) SSD steps on the mapped current patch;
    the last dp and W"""
    for _ in range(N_ITERS):
        It_orig, Jt = pa.sample(W)
        _, It, _, dft = rscv_update(It_orig, pa.I0o, n_bins, linear)
        if method == "esm":
            g = 0.5 * (dft @ (pa.J0 + Jt))
            H = 0.5 * (-Jt.T @ Jt - pa.J0.T @ pa.J0)
        elif method == "fclk":
            g = dft @ Jt
            H = -Jt.T @ Jt
        else:
            g = (-dft) @ pa.J0          # df/dI0 = It - I0 (SSDBase::updateInitGrad)
            H = -pa.J0.T @ pa.J0
        dp = -np.linalg.solve(H, g)
        W = inv_compose(W, dp) if method == "iclk" else R.compose_hom(W, dp)
    return dp, W


def corners_of(W, corners_hm):
    q = W @ corners_hm
    return q[:2] / q[2]


def main():
    rng = np.random.default_rng(SEED)
    img = make_image()
    out = {"img": img, "tags": np.array([c[0] for c in CASES])}
    empty_hit = False
    for tag, nb, lin, resx, resy, affine, corners in CASES:
        if affine:
            p = rng.uniform(-1, 1, 6) * [1.2, 1.2, 0.02, 0.02, 0.02, 0.02]
        else:
            p = synth.random_small_homography(rng, 0.4)
        pa = Patch(img.astype(np.float64), nb, resx, resy, affine, corners)   # (pa.I0o: the normalised template, RSCV's I0)
        W = pa.warp(p)
        It_orig, Jt = pa.sample(W)
        m, It, f, dft = rscv_update(It_orig, pa.I0o, nb, lin)
        empty_hit = empty_hit or bool(np.any(np.bincount(It_orig.astype(np.int64), minlength=nb)[:nb] == 0))
        full = resx * resy <= FULL_MAX
        rec = {
            tag + "_cfg": np.array([nb, lin, resx, resy, int(affine)]), tag + "_corners": corners, tag + "_p": p,
            tag + "_map": m, tag + "_It_orig_head": It_orig[:HEAD], tag + "_It_head": It[:HEAD], tag + "_df_dIt_head": dft[:HEAD],
            tag + "_f": f, tag + "_g": dft @ Jt, tag + "_H_curr": -Jt.T @ Jt, tag + "_H_self": -Jt.T @ Jt,
        }
        if full:
            rec[tag + "_It"] = It
            rec[tag + "_df_dIt"] = dft
        if not affine and nb >= 64:   # (7 bins on the ramp: a coarse map, the 5-iteration run is not a meaningful fixture)
            chm = np.vstack([corners, np.ones(4)])
            runs = {method: lk_run(pa, W, nb, lin, method) for method in ("esm", "fclk", "iclk")}
            if all(np.abs(dp).max() < 0.5 for dp, _ in runs.values()):
                for method, (dp, Wn) in runs.items():
                    rec[tag + "_" + method + "_dp"] = dp
                    rec[tag + "_" + method + "_corners"] = corners_of(Wn, chm)
        out.update(rec)
    assert empty_hit, "no case exercises the empty-bin rule"
    path = os.path.join(HERE, "lk_golden7.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
