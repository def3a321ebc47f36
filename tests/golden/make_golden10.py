#!/usr/bin/env python
"""Generates tests/golden/lk_golden10.npz: the Sum of Pixelwise Structural Similarity appearance model (SPSS, AM/src/SPSS.cc) from an
independent float64 NumPy restatement of its definition, written from the table below (the C++ oracle has no SPSS).

With a = I0 and b = It the raw pixel values of one pixel (no normalisation, no pixel mapper) and c = (255 k)^2:
  den     = a^2 + b^2 + c
  fv      = (2 a b + c) / den                         f = sum fv, at most N
  df_dIt  = 2 (a - fv b) / den                        the derivative of f in It
  df_dI0  = 2 (b (b^2 - a^2) + c (b - 2 a)) / den^2   NOT the derivative of f in I0 (that has c (b - a)): the reference's form, kept
  w_self  = -2 / (2 b^2 + c)
  w_curr  = -2 (fv + 3 df_dIt b) / den
  w_init  = -2 (fv + a df_dI0) / den
  g_curr(J) = sum df_dIt J_row      g_init(J0) = sum df_dI0 J0_row      H_x(J) = sum w_x J_row J_row^T
H0 = H_self(J0) at It = I0 (the constant Hessian of InitialSelf).  Search-method algebra (NT/ESM.cc, NT/FCLK.cc, NT/ICLK.cc):
  FCLK  g_curr(Jt);  H0 | H_self(Jt) | H_curr(Jt)
  ICLK  g_init(J0);  H0 | H_self(Jt) | H_init(J0)
  ESM   g_curr(Jm) (Original) or (g_curr(Jt) - g_init(J0)) / 2 (DiffOfJacs), Jm = (J0 + Jt) / 2;
        H0 | H_self(Jt) | (H_self(Jt) + H0) / 2 | H_curr(Jm) | (H_init(J0) + H_curr(Jt)) / 2 | H_curr(Jt)

Per case: cfg (resx, resy, affine), k, corners, the state p, It, df_dIt, df_dI0, f, g_curr, g_init, H_self, H_curr, H_init (over Jt, Jt, J0),
g_mean and H_mean (g_curr and H_curr over Jm), H0, the updates dp of ESM (DiffOfJacs + SumOfSelf: esm_ds; Original + Original: esm_oo), FCLK (CurrentSelf: fclk_cs; Std: fclk_std) and
ICLK (InitialSelf: iclk_is; Std: iclk_std), and for every summed quantity err_floor_*: the largest difference between the float64
evaluation and the same sums in np.longdouble, relative to the quantity's largest entry.  For the well-conditioned cases (the last solved step of
every run moves the corners by less than CONTRACTED, squared and summed: the loop is contracting when it ends) the loop of each method --
esm_ds, fclk_cs, iclk_is -- from p, at most N_ITERS iterations, without and with Levenberg-Marquardt (delta 0.01, update 10): passes
done, state and corners.  The corner-change test's epsilon is one per GROUP of cases (the cases of one group share a batch in the loop
tests, and a batch has one search-method configuration): of EPS_CANDIDATES the one no run's corner change comes closer to than any other,
and never within a factor of 2, so the pass counts do not hang on rounding (corners that agree to 2e-4 px move a squared change of 1e-4
px^2 by a few per cent); it is stored as <tag>_eps.

The image is the top-left 176 x 176 of make_golden5.py's (a block saturated at 0, one at 255, texture) and is stored in the file.
Three 50 x 50 homography cases share a batch in the loop tests; the third has a corner outside the frame (samples there take 128).

Run from the repo root:  python tests/golden/make_golden10.py
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

SEED = 20261019
IMG_SIDE = 176
N_ITERS = 5
EPS_CANDIDATES = (1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 3e-6, 1e-6, 3e-7, 1e-7)
CONTRACTED = 1e-2
LM_DELTA, LM_UPDATE = 0.01, 10.0
K_DEFAULT = 0.01

_rect = make_golden5._rect
# (tag, k, resx, resy, affine, corners, scale of p)
CASES = (
    ("h50a", 0.01, 50, 50, False, synth.square_corners(112, 60, 64), 0.15),
    ("h50b", 0.01, 50, 50, False, synth.square_corners(60, 128, 70), 0.08),
    ("h50c", 0.01, 50, 50, False, _rect(118, 96, 181, 160), 0.04),    # right edge past the frame (176 columns)
    ("h37x23", 0.01, 37, 23, False, _rect(96, 20, 154, 66), 0.1),
    ("a7x5", 0.01, 7, 5, True, _rect(100, 120, 121, 135), 1.0),
    ("a40", 0.01, 40, 40, True, _rect(30, 100, 96, 144), 1.0),
    ("a40k3", 0.03, 40, 40, True, _rect(30, 100, 96, 144), 1.0),      # a40 at k = 0.03 (the same p: drawn once)
)
METHODS = ("esm_ds", "esm_oo", "fclk_cs", "fclk_std", "iclk_is", "iclk_std")
LOOPS = ("esm_ds", "fclk_cs", "iclk_is")


def rect_to_quad(lo_x, lo_y, hi_x, hi_y, corners):
    """the map of the rectangle [lo, hi] onto the quadrilateral TL, TR, BR, BL (2 x 4), row-major 3 x 3 with the last entry 1: the closed form
    of the four-point homography (affine when the quadrilateral is a parallelogram), scalar by scalar"""
    (x0, x1, x2, x3), (y0, y1, y2, y3) = (float(v) for v in corners[0]), (float(v) for v in corners[1])
    dx1, dx2, sx = x1 - x2, x3 - x2, x0 - x1 + x2 - x3
    dy1, dy2, sy = y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    if sx == 0 and sy == 0:
        a, b, c, d, e, f, g, h = x1 - x0, x3 - x0, x0, y1 - y0, y3 - y0, y0, 0.0, 0.0
    else:
        den = dx1 * dy2 - dy1 * dx2
        g, h = (sx * dy2 - dx2 * sy) / den, (dx1 * sy - sx * dy1) / den
        a, b, c = x1 - x0 + g * x1, x3 - x0 + h * x3, x0
        d, e, f = y1 - y0 + g * y1, y3 - y0 + h * y3, y0
    wx, wy = hi_x - lo_x, hi_y - lo_y
    m = []
    for r in ((a, b, c), (d, e, f), (g, h, 1.0)):
        m += [r[0] / wx, r[1] / wy, r[2] - r[0] * lo_x / wx - r[1] * lo_y / wy]
    if m[8] != 1.0:
        m = [v / m[8] for v in m]
    m[8] = 1.0
    return m


def lin_spaced(n, lo, hi):
    """Eigen's LinSpaced: lo + i step, the last entry hi itself"""
    v = lo + np.arange(n, dtype=np.float64) * ((hi - lo) / (n - 1))
    v[-1] = hi
    return v


class Patch:
    """The sample grid of one target, its template quantities and its samples at a warp, with every expression written out element by
    element in the reference's operation order (ProjectiveBase / Homography.cc:66,86-90,231-294, Affine.cc:104,213-242, imgUtils.cc:233-254):
    the 1e-8-step central differences amplify the last bit of a sample point to ~1e-7 of a gradient, so a reference whose points came out of
    a matrix product in another order would not pin g and H beyond that.  Raw pixel values (SPSS has no normalisation)."""

    def __init__(self, img, resx, resy, affine, corners):
        self.img, self.affine = img, affine
        lo_x, lo_y, hi_x, hi_y = (1 - resx / 2.0, 1 - resy / 2.0, resx / 2.0, resy / 2.0) if affine else (-0.5, -0.5, 0.5, 0.5)
        w0 = rect_to_quad(lo_x, lo_y, hi_x, hi_y, corners)
        nx = np.tile(lin_spaced(resx, lo_x, hi_x), resy)
        ny = np.repeat(lin_spaced(resy, lo_y, hi_y), resx)
        X = w0[0] * nx + w0[1] * ny + w0[2] * 1.0
        Y = w0[3] * nx + w0[4] * ny + w0[5] * 1.0
        Z = w0[6] * nx + w0[7] * ny + w0[8] * 1.0
        x, y = X / Z, Y / Z
        self.init_pts = np.stack([x, y])
        # the homogeneous points the warp multiplies: affine re-homogenises (x, y, 1), homography keeps (X, Y, Z)
        self.init_hm = np.stack([x, y, np.ones_like(x)]) if affine else np.stack([X, Y, Z])
        self.I0o = R.bilinear(img, x, y)
        g0 = R.img_grad(img, self.init_pts)
        self.J0 = self.rows(np.eye(3), np.zeros(8), g0, x, y, self.init_hm[2])

    def warp(self, p):
        return R.aff_matrix(p) if self.affine else R.hom_matrix(p)

    def rows(self, W, state, grad, cx, cy, cz):
        """cmptWarpedPixJacobian: the steepest-descent rows of the gradient `grad` taken at the warped points (cx, cy), third homogeneous
        coordinate cz, under the warp W (affine: its state)"""
        x, y = self.init_pts
        gx, gy = grad[:, 0], grad[:, 1]
        if self.affine:
            a, b, c, d = state[2] + 1, state[3], state[4], state[5] + 1
            Ixx, Ixy, Iyy, Iyx = gx * x, gx * y, gy * y, gy * x
            return np.stack([gx * a + gy * c, gx * b + gy * d, Ixx * a + Iyx * c, Ixy * a + Iyy * c, Ixx * b + Iyx * d, Ixy * b + Iyy * d], axis=1)
        inv_det = 1.0 / cz
        dwx_dx, dwx_dy = W[0, 0] - W[2, 0] * cx, W[0, 1] - W[2, 1] * cx
        dwy_dx, dwy_dy = W[1, 0] - W[2, 0] * cy, W[1, 1] - W[2, 1] * cy
        Ix = (dwx_dx * gx + dwy_dx * gy) * inv_det
        Iy = (dwx_dy * gx + dwy_dy * gy) * inv_det
        Ixx, Iyy, Ixy, Iyx = Ix * x, Iy * y, Ix * y, Iy * x
        return np.stack([Ixx, Ixy, Ix, Iyx, Iyy, Iy, -x * Ixx - y * Iyx, -x * Ixy - y * Iyy], axis=1)

    def sample(self, W, state=None):
        """It and Jt at the warp W (chained: the image gradient at the warped points through dW/dx); state: the affine state the warp was
        built from (its own state otherwise)"""
        hx, hy, z = self.init_hm
        cx = W[0, 0] * hx + W[0, 1] * hy + W[0, 2] * z
        cy = W[1, 0] * hx + W[1, 1] * hy + W[1, 2] * z
        if self.affine:
            wx, wy, D = cx, cy, np.ones_like(cx)
            if state is None:
                state = state_of(W, True)
        else:
            D = W[2, 0] * hx + W[2, 1] * hy + W[2, 2] * z
            wx, wy = cx / D, cy / D
        It = R.bilinear(self.img, wx, wy)
        Jt = self.rows(W, state, R.img_grad(self.img, np.stack([wx, wy])), wx, wy, D)
        return It, Jt


def make_image():
    return np.ascontiguousarray(make_golden5.make_image()[:IMG_SIDE, :IMG_SIDE])


def spss_c(k):
    c = k * 255.0
    return c * c


def per_pixel(a, b, c):
    """fv, df_dIt, df_dI0, w_self, w_curr, w_init of the table, in the dtype of the inputs"""
    den = a * a + b * b + c
    fv = (2 * a * b + c) / den
    dft = 2 * (a - fv * b) / den
    df0 = 2 * (b * (b * b - a * a) + c * (b - 2 * a)) / (den * den)
    return fv, dft, df0, -2 / (2 * b * b + c), -2 * (fv + 3 * dft * b) / den, -2 * (fv + a * df0) / den


def wgram(w, J):
    return (J * w[:, None]).T @ J


def quantities(I0, It, J0, Jt, c, dtype=np.float64):
    """every summed quantity of one pass, evaluated in dtype from the float64 inputs"""
    a, b, J0, Jt = (np.asarray(v, dtype=dtype) for v in (I0, It, J0, Jt))
    c = dtype(c)
    fv, dft, df0, ws, wc, wi = per_pixel(a, b, c)
    Jm = (J0 + Jt) / 2
    return {"fv": fv, "df_dIt": dft, "df_dI0": df0, "f": fv.sum(), "g_curr": dft @ Jt, "g_init": df0 @ J0, "g_mean": dft @ Jm,
            "H_self": wgram(ws, Jt), "H_curr": wgram(wc, Jt), "H_init": wgram(wi, J0), "H_mean": wgram(wc, Jm)}


def self_hessian0(I0, J0, c):
    return wgram(-2 / (2 * I0 * I0 + c), J0)


def g_and_H(q, H0, method):
    if method == "esm_ds":
        return 0.5 * (q["g_curr"] - q["g_init"]), 0.5 * (q["H_self"] + H0)
    if method == "esm_oo":
        return q["g_mean"], q["H_mean"]
    if method == "fclk_cs":
        return q["g_curr"], q["H_self"]
    if method == "fclk_std":
        return q["g_curr"], q["H_curr"]
    if method == "iclk_is":
        return q["g_init"], H0
    return q["g_init"], q["H_init"]


def step_matrix(dp, affine):
    return R.aff_matrix(dp) if affine else R.hom_matrix(dp)


def compose(W, dp, affine, inverse):
    M = step_matrix(dp, affine)
    Wn = W @ (np.linalg.inv(M) if inverse else M)
    return Wn / Wn[2, 2]


def state_of(W, affine):
    if affine:
        return np.array([W[0, 2], W[1, 2], W[0, 0] - 1, W[0, 1], W[1, 0], W[1, 1] - 1])
    return np.array([W[0, 0] - 1, W[0, 1], W[0, 2], W[1, 0], W[1, 1] - 1, W[1, 2], W[2, 0], W[2, 1]])


def corners_of(W, corners_hm):
    q = W @ corners_hm
    return q[:2] / q[2]


def run_loop(pa, W, c, H0, affine, corners, method, leven_marq, eps):
    """the search method's update() from the warp W with the corner-change test at eps: passes done, final warp, and the corner changes of
    the solved steps.  Levenberg-Marquardt as NT/ESM.cc:186-232, NT/FCLK.cc:205-250, NT/ICLK.cc:181-199: f is
    compared with the last accepted one; a worse f multiplies delta, takes the previous update back and skips the convergence test; the
    pass after an undo skips the comparison; an undo consumes an iteration of ESM's and ICLK's for loops but not of FCLK's while loop."""
    chm = np.vstack([corners, np.ones(4)])
    iclk, fclk = method.startswith("iclk"), method.startswith("fclk")
    prev_f, delta, state_reset, it_id, last_dp = 0.0, LM_DELTA, False, 0, None
    passes, changes = 0, []
    max_passes = 2 * N_ITERS if (leven_marq and fclk) else N_ITERS
    while passes < max_passes:
        It, Jt = pa.sample(W)
        q = quantities(pa.I0o, It, pa.J0, Jt, c)
        undo = False
        if leven_marq:
            if not state_reset and it_id > 0:
                if q["f"] < prev_f:
                    delta *= LM_UPDATE
                    undo = True
                elif q["f"] > prev_f:
                    delta /= LM_UPDATE
            if not undo and not state_reset:
                prev_f = q["f"]
            state_reset = undo
        if undo:
            dp = last_dp
        else:
            g, H = g_and_H(q, H0, method)
            if leven_marq:
                H = H + delta * np.diag(np.diag(H))
            dp = -np.linalg.solve(H, g)
            last_dp = dp
        before = corners_of(W, chm)
        W = compose(W, dp, affine, inverse=(iclk != undo))
        change = float(((before - corners_of(W, chm)) ** 2).sum())
        passes += 1
        it_id += 0 if (undo and fclk) else 1
        if not undo:
            changes.append(change)
        if (not undo and change < eps) or it_id >= N_ITERS:
            break
    return passes, W, changes


def eps_margin(changes, eps):
    """how close a corner change comes to eps, as a ratio >= 1"""
    return min(max(ch / eps, eps / max(ch, 1e-300)) for ch in changes)


def rel_floor(x64, xld):
    xld = np.asarray(xld, dtype=np.longdouble)
    return float(np.abs(np.asarray(x64, dtype=np.longdouble) - xld).max() / np.abs(xld).max())


def main():
    rng = np.random.default_rng(SEED)
    img = make_image()
    out = {"img": img, "tags": np.array([c[0] for c in CASES]), "loop_cfg": np.array([N_ITERS, LM_DELTA, LM_UPDATE])}
    drawn = {}
    outside = False
    loops = {}     # group (resx, resy, affine, k) -> [(tag, pa, W, c, H0, affine, corners)]
    for tag, k, resx, resy, affine, corners, scale in CASES:
        key = (resx, resy, affine, corners.tobytes())
        if key not in drawn:
            drawn[key] = (rng.uniform(-1, 1, 6) * [1.2, 1.2, 0.02, 0.02, 0.02, 0.02] * scale if affine
                          else synth.random_small_homography(rng, scale))
        p = drawn[key]
        c = spss_c(k)
        pa = Patch(img.astype(np.float64), resx, resy, affine, corners)
        W = pa.warp(p)
        It, Jt = pa.sample(W, p)
        q = quantities(pa.I0o, It, pa.J0, Jt, c)
        ql = quantities(pa.I0o, It, pa.J0, Jt, c, dtype=np.longdouble)
        H0 = self_hessian0(pa.I0o, pa.J0, c)
        wp = W @ pa.init_hm
        wp = wp[:2] / wp[2]
        outside = outside or bool((wp[0] >= IMG_SIDE).any() or (wp[1] >= IMG_SIDE).any() or (wp < 0).any())
        rec = {tag + "_cfg": np.array([resx, resy, int(affine)]), tag + "_k": k, tag + "_corners": corners, tag + "_p": p,
               tag + "_It": It, tag + "_df_dIt": q["df_dIt"], tag + "_df_dI0": q["df_dI0"], tag + "_H0": H0}
        for name in ("f", "g_curr", "g_init", "g_mean", "H_self", "H_curr", "H_init", "H_mean"):
            rec[tag + "_" + name] = np.asarray(q[name], dtype=np.float64)
            rec[tag + "_err_floor_" + name] = rel_floor(q[name], ql[name])
        for method in METHODS:
            g, H = g_and_H(q, H0, method)
            rec[tag + "_" + method + "_dp"] = -np.linalg.solve(H, g)
        free = [run_loop(pa, W, c, H0, affine, corners, m, lm, 0.0) for m in LOOPS for lm in (False, True)]
        if all(r[2][-1] < CONTRACTED for r in free):
            loops.setdefault((resx, resy, affine, k), []).append((tag, pa, W, c, H0, affine, corners))
        out.update(rec)
    assert outside, "no case samples past the frame"
    for group in loops.values():
        best = None
        for eps in EPS_CANDIDATES:
            runs = {(g[0], m, lm): run_loop(*g[1:], m, lm, eps) for g in group for m in LOOPS for lm in (False, True)}
            margin = min(eps_margin(r[2], eps) for r in runs.values())
            if best is None or margin > best[0]:
                best = (margin, eps, runs)
        margin, eps, runs = best
        assert margin > 2, "%s: a corner change within a factor %.2f of every candidate epsilon" % (group[0][0], margin)
        for tag, pa, W, c, H0, affine, corners in group:
            out[tag + "_eps"] = eps
            chm = np.vstack([corners, np.ones(4)])
            for m in LOOPS:
                for lm in (False, True):
                    passes, Wn, _ = runs[(tag, m, lm)]
                    pre = tag + "_" + m + ("_lm" if lm else "") + "_loop"
                    out[pre + "_n"] = passes
                    out[pre + "_state"] = state_of(Wn, affine)
                    out[pre + "_corners"] = corners_of(Wn, chm)
    path = os.path.join(HERE, "lk_golden10.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
