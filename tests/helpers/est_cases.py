"""Synthetic point sets and hypothesis lists for the estimator tests (tests/test_est_ref.py, tests/test_gpu_est.py): an s x s lattice of
input points, a known warp, Gaussian noise, a fraction of points displaced grossly, all rounded to float32."""
import numpy as np

import est_ref as R

H_TRUE = np.array([[1.03, 0.02, 4.0], [-0.015, 0.98, -3.0], [2e-5, -1.5e-5, 1.0]])
A_TRUE = np.array([[1.03, 0.02, 4.0], [-0.015, 0.98, -3.0], [0.0, 0.0, 1.0]])


def apply(H, pts):
    q = np.c_[pts, np.ones(len(pts))] @ H.T
    return q[:, :2] / q[:, 2:]


def make_points(ssm, s, seed, outlier_frac, noise=0.3, n=None):
    """(in_pts, out_pts, clean): float32 (n, 2) pairs and the boolean mask of the points that were NOT displaced.  n < s * s keeps the
    first n lattice points (for counts that are no square)."""
    rng = np.random.default_rng(seed)
    g = np.linspace(120.0, 390.0, s)
    pts = np.array([(x, y) for y in g for x in g])
    if n is not None:
        pts = pts[:n]
    n = len(pts)
    out = apply(H_TRUE if ssm == R.HOMOGRAPHY else A_TRUE, pts) + rng.normal(0.0, noise, size=(n, 2)) if noise > 0 else \
        apply(H_TRUE if ssm == R.HOMOGRAPHY else A_TRUE, pts)
    clean = np.ones(n, dtype=bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = rng.choice(n, n_out, replace=False)
        d = rng.uniform(15.0, 40.0, size=(n_out, 2)) * rng.choice([-1.0, 1.0], size=(n_out, 2))   # gross: up to +-40 px, never small
        out[bad] += d
        clean[bad] = False
    return pts.astype(np.float32), out.astype(np.float32), clean


def draw_subsets(seed, in_pts, out_pts, n_hyp, mp):
    """n_hyp rows of mp distinct indices that pass the reference's checkSubset on both sides; no subset twice, in any order"""
    rng = np.random.default_rng(seed)
    M, m = in_pts.astype(np.float64), out_pts.astype(np.float64)
    rows, seen = [], set()
    n = len(M)
    while len(rows) < n_hyp:
        r = rng.choice(n, mp, replace=False)
        key = tuple(sorted(r.tolist()))
        if key in seen or not R.check_subset(M[r]) or not R.check_subset(m[r]):
            continue
        seen.add(key)
        rows.append(r)
    return np.array(rows, dtype=np.int32)
