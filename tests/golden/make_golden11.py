#!/usr/bin/env python
"""Generates tests/golden/lk_golden11.npz: the Structural Similarity appearance model (SSIM, AM/src/SSIM.cc) from an independent float64
NumPy restatement of it, written from the CENTRED vectors the reference forms -- not from the raw moments the device reduces (the C++
oracle has no SSIM).

With N the patch size, m0 / mt the means of I0 / It, x0 = I0 - m0, xt = It - mt, c1 = (255 k1)^2, c2 = (255 k2)^2 (SSIM.cc:36-39, 98-111):
  v0 = x0.x0 / (N - 1)    vt = xt.xt / (N - 1)    cross = x0.xt / (N - 1)
  a = 2 mt m0 + c1    b = 2 cross + c2    c = mt^2 + m0^2 + c1    d = vt + v0 + c2    f = a b / (c d)
Gradients (SSIM.cc:113-142), mu = 2 / (N c d):
  gv_t = mu (a x0 - f c xt)    gs_t = 2 (m0 b - mt f d) / (c d (N - 1))    df_dIt = gv_t + gs_t
  gv_0 = mu (a xt - f c x0)    gs_0 = 2 (mt b - m0 f d) / (c d (N - 1))    df_dI0 = gv_0 + gs_0
(the N against N - 1 in mu and gs is the reference's: the vectors are not the derivatives of f, and are kept).
Hessians over a pixel Jacobian X (N x S), sX its column sums (SSIM.cc:144-287); for cmptCurrHessian, with a_diff = 2 m0 / N,
c_diff = 2 mt / N, m1 = 2 / (N c d), m2 = 2 / ((N - 1) c d), QI = 2 / (N - 1) as the INTEGER quotient the reference writes (0 for N >= 4)
and w = QI xt / d + c_diff / c:
  H_curr = m1 (a_diff (X^T x0) sX^T - (X^T xt) ((c df_dIt + f c_diff)^T X) - f c (X^T X - sX sX^T / N))
           - (X^T gv_t) (w^T X)
           + (X^T (m2 (x0 2 m0 / (N - 1) - ((d df_dIt + (2.0 / (N - 1)) f xt) mt + f d / N)) - gs_t w)) sX^T
cmptInitHessian is the same with I0 and It exchanged (x0 <-> xt, m0 <-> mt, df_dI0, gv_0, gs_0).  (In the second line the reference multiplies
X^T gv^T, a column, by the column w -- a product Eigen only evaluates with its assertions compiled out; w is taken as the row that makes the
product conform, which is the outer product the surrounding terms are.)  Neither matrix is symmetric.
  H_self = cs (2 / (N cs ds)) (sX sX^T / N - X^T X) - (2 ds / ((N - 1) cs ds N)) sX sX^T    cs = 2 mt^2 + c1, ds = 2 vt + c2
cmptSelfHessian overwrites the members c and d until the next updateSimilarity (SSIM.cc:273-274); nothing here carries such state: every
Hessian is taken with the c and d of the similarity.  H0 = H_self(J0) at It = I0.  Likelihood exp(-alpha (1 / f - 1)^2) (SSIM.cc:45-48).

Search-method algebra (NT/ESM.cc, NT/FCLK.cc, NT/ICLK.cc), as for NCC:
  FCLK  g_curr(Jt);  H0 | H_self(Jt) | H_curr(Jt)
  ICLK  g_init(J0);  H0 | - | H_init(J0)
  ESM   g_curr(Jm) (Original) or (g_curr(Jt) - g_init(J0)) / 2 (DiffOfJacs), Jm = (J0 + Jt) / 2;
        H0 | H_self(Jt) | (H_self(Jt) + H0) / 2 | H_curr(Jm) | (H_init(J0) + H_curr(Jt)) / 2 | H_curr(Jt)

Per case: cfg (resx, resy, ssm), k1, k2, corners, the state p, It, f, g_curr, g_init, g_mean, H_self, H_curr, H_init (over Jt,
Jt, J0), H_mean (H_curr over Jm), H0, the updates dp of METHODS, dp_jitter (below), H_curr_fq (H_curr with the quotient in floating point)
and for every summed quantity err_floor_*: the largest difference between the float64 evaluation and the same expressions in np.longdouble, relative to
the quantity's largest entry.  dp_jitter is the floor of the UPDATE under arithmetic that is not the reference's own (dp_jitter()): how far
the reference's updates move when the corners move by 1e-12 px.  Loops as in make_golden10.py, per method: where a method's free runs end
contracting (the last solved step moves the corners by less than CONTRACTED; <tag>_well, one flag per method of LOOPS) its loop from p, at
most N_ITERS iterations, without and with Levenberg-Marquardt, with one epsilon per group of cases that share a batch, chosen so that no
corner change comes within a factor 2 of it.  The generator fails unless a homography, an affine and a low-order case are
well-conditioned for every method.

Cases, on the 176 x 176 image of make_golden5.py: 7 x 9 homography (N = 63, under one wave), 25 x 25 affine (N = 625), 16 x 16 homography
(N = 256), three 50 x 50 homography cases that share a batch (one with a corner outside the frame), and a 20 x 20 case for each of
Similitude, Isometry and Translation (the models of tests/helpers/lowdof_ref.py).

Run from the repo root:  python tests/golden/make_golden11.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, HERE)
import numpy_ref as R  # noqa: E402
from mtf_amd import synth  # noqa: E402
import make_golden5  # noqa: E402
import make_golden10 as M10  # noqa: E402
import lowdof_ref as LD  # noqa: E402

SEED = 20261020
IMG_SIDE = 176
N_ITERS = 5
EPS_CANDIDATES = M10.EPS_CANDIDATES
CONTRACTED = 1e-2
LM_DELTA, LM_UPDATE = 0.01, 10.0
K1_DEFAULT, K2_DEFAULT = 0.01, 0.03
HOM, AFF, SIM, ISO, TRA = 0, 1, 2, 3, 4     # MTFHIP_SSM_*

_rect = make_golden5._rect
# (tag, k1, k2, resx, resy, ssm, corners, scale of p)
CASES = (
    ("h50a", 0.01, 0.03, 50, 50, HOM, synth.square_corners(112, 60, 64), 0.15),
    ("h50b", 0.01, 0.03, 50, 50, HOM, synth.square_corners(60, 128, 70), 0.08),
    ("h50c", 0.01, 0.03, 50, 50, HOM, _rect(118, 96, 181, 160), 0.04),    # right edge past the frame (176 columns)
    ("h7x9", 0.01, 0.03, 7, 9, HOM, _rect(100, 120, 121, 147), 0.05),
    ("h16", 0.01, 0.03, 16, 16, HOM, _rect(96, 20, 144, 68), 0.1),
    ("a25", 0.01, 0.03, 25, 25, AFF, _rect(30, 100, 96, 144), 1.0),
    ("a25k", 0.05, 0.1, 25, 25, AFF, _rect(30, 100, 96, 144), 1.0),       # a25 at other constants (the same p: drawn once)
    ("sim20", 0.01, 0.03, 20, 20, SIM, _rect(40, 96, 100, 150), 1.0),
    ("iso20", 0.01, 0.03, 20, 20, ISO, _rect(40, 96, 100, 150), 1.0),
    ("tra20", 0.01, 0.03, 20, 20, TRA, _rect(40, 96, 100, 150), 1.0),
)
# key -> (search method 0 ESM / 1 FCLK / 2 ICLK, jac_type, hess_type)
METHODS = {"esm_ds": (0, 1, 2), "esm_oo": (0, 0, 3), "esm_ss": (0, 1, 4), "esm_std": (0, 1, 5), "fclk_cs": (1, 1, 1), "fclk_std": (1, 1, 2),
           "iclk_is": (2, 1, 0), "iclk_std": (2, 1, 2)}
LOOPS = ("esm_ds", "fclk_cs", "iclk_is")


def make_image():
    return M10.make_image()


def ssim_c(k):
    c = k * 255.0
    return c * c


class LowPatch:
    """a Similitude / Isometry / Translation target: the grid, the warp and the pixel Jacobians of tests/helpers/lowdof_ref.py's SSM, sampled
    as Patch samples (raw pixel values, chained gradients)"""

    def __init__(self, img, resx, resy, kind, corners):
        self.img, self.kind, self.affine = img, kind, False
        self.ssm = LD.SSM(kind, resx, resy)
        self.ssm.set_corners(corners)
        self.init_pts = self.ssm.init_pts.copy()
        self.I0o = R.bilinear(img, self.init_pts[0], self.init_pts[1])
        g0 = R.img_grad(img, self.init_pts)
        self.J0, self.J0_aff = self._rows(g0), self.aff_rows(g0)

    def _rows(self, grad):
        S = self.ssm.S
        return np.ascontiguousarray(self.ssm.cmpt_warped_pix_jacobian(np.concatenate([grad[:, 0], grad[:, 1]])).reshape(S, -1).T)

    def aff_rows(self, grad):
        """the six affine-coordinate columns [Ix, Iy, Ix x, Ix y, Iy x, Iy y] of the warped gradient at the model's current warp: the rows of
        the model are combinations of them, J_S = J_aff M (lowdof_ref.M), with the same products and sums"""
        ssm, g0, g1 = self.ssm, grad[:, 0], grad[:, 1]
        if self.kind == TRA:
            Ix, Iy = g0, g1
        elif self.kind == SIM:
            a, b, c, d = ssm.state[2] + 1, -ssm.state[3], ssm.state[3], ssm.state[2] + 1
            Ix, Iy = a * g0 + c * g1, b * g0 + d * g1
        else:
            cos_t, sin_t = ssm.warp[0, 0], ssm.warp[1, 0]
            Ix, Iy = cos_t * g0 + sin_t * g1, cos_t * g1 - sin_t * g0
        x, y = self.init_pts
        return np.stack([Ix, Iy, Ix * x, Ix * y, Iy * x, Iy * y], axis=1)

    def warp(self, p):
        return self.ssm.warp_from_state(p)

    def sample(self, W, state=None, affine_rows=False):
        self.ssm.set_warp(W)
        x, y = self.ssm.curr_pts
        It = R.bilinear(self.img, x, y)
        grad = R.img_grad(self.img, np.stack([x, y]))
        return It, (self.aff_rows(grad) if affine_rows else self._rows(grad))

    def compose(self, W, dp, inverse):
        self.ssm.set_warp(W)
        self.ssm.compositional_update(self.ssm.invert_state(dp) if inverse else dp)
        return self.ssm.warp.copy()

    def state_of(self, W):
        return self.ssm.state_from_warp(W)


class Model:
    """what the loops need of a case, homography / affine (make_golden10.Patch) or low-order (LowPatch)"""

    def __init__(self, img, resx, resy, ssm, corners):
        self.ssm_id, self.corners = ssm, corners
        self.low = ssm >= SIM
        self.pa = LowPatch(img, resx, resy, ssm, corners) if self.low else M10.Patch(img, resx, resy, ssm == AFF, corners)
        self.chm = np.vstack([corners, np.ones(4)])
        self.I0, self.J0 = self.pa.I0o, self.pa.J0

    def draw(self, rng, scale):
        if self.ssm_id == HOM:
            return synth.random_small_homography(rng, scale)
        if self.ssm_id == AFF:
            return rng.uniform(-1, 1, 6) * [1.2, 1.2, 0.02, 0.02, 0.02, 0.02] * scale
        return (rng.uniform(-1, 1, 4) * [1.2, 1.2, 0.02, 0.02] * scale)[:LD.STATE_SIZE[self.ssm_id]]

    def warp(self, p):
        return self.pa.warp(p)

    def sample(self, W, p=None):
        return self.pa.sample(W, p)

    def compose(self, W, dp, inverse):
        return self.pa.compose(W, dp, inverse) if self.low else M10.compose(W, dp, self.ssm_id == AFF, inverse)

    def state_of(self, W):
        return self.pa.state_of(W) if self.low else M10.state_of(W, self.ssm_id == AFF)

    def corners_of(self, W):
        return M10.corners_of(W, self.chm)


def scalars(I0, It, c1, c2):
    """SSIM.cc:50-111 on the centred vectors, in the dtype of the inputs"""
    N = I0.size
    m0, mt = I0.sum() / N, It.sum() / N
    x0, xt = I0 - m0, It - mt
    v0, vt = (x0 * x0).sum() / (N - 1), (xt * xt).sum() / (N - 1)
    a = 2 * mt * m0 + c1
    cross = (x0 * xt).sum() / (N - 1)
    b = 2 * cross + c2
    c = mt * mt + m0 * m0 + c1
    d = vt + v0 + c2
    cd = c * d
    f = (a * b) / cd
    mu = 2.0 / (N * cd)
    gs_t = 2 * (m0 * b - mt * f * d) / (cd * (N - 1))
    gs_0 = 2 * (mt * b - m0 * f * d) / (cd * (N - 1))
    gv_t, gv_0 = mu * (a * x0 - f * c * xt), mu * (a * xt - f * c * x0)
    return dict(N=N, m0=m0, mt=mt, x0=x0, xt=xt, v0=v0, vt=vt, a=a, b=b, c=c, d=d, cd=cd, f=f, gs_t=gs_t, gs_0=gs_0, gv_t=gv_t, gv_0=gv_0,
                df_dIt=gv_t + gs_t, df_dI0=gv_0 + gs_0, c1=c1, c2=c2)


def hess_std(s, X, curr, int_quot=True):
    """cmptCurrHessian (curr) / cmptInitHessian over X, SSIM.cc:144-254; int_quot: (2 / (patch_size - 1)) as the integer quotient it is"""
    N, c, d, cd, f = s["N"], s["c"], s["d"], s["cd"], s["f"]
    if curr:
        mo, mu_, xo, xu, df, gv, gs = s["m0"], s["mt"], s["x0"], s["xt"], s["df_dIt"], s["gv_t"], s["gs_t"]
    else:
        mo, mu_, xo, xu, df, gv, gs = s["mt"], s["m0"], s["xt"], s["x0"], s["df_dI0"], s["gv_0"], s["gs_0"]
    a_diff, c_diff = 2.0 * mo / N, 2.0 * mu_ / N
    m1, m2 = 2.0 / (N * cd), 2.0 / ((N - 1) * cd)
    qi = (2 // (N - 1)) if int_quot else 2.0 / (N - 1)
    sX = X.sum(axis=0)
    w = qi * xu / d + (c_diff / c)
    u = m2 * (xo * (2 * mo / (N - 1)) - ((df * d + (2.0 / (N - 1)) * xu * f) * mu_ + f * d / N)) - gs * w
    return (m1 * (a_diff * np.outer(X.T @ xo, sX) - np.outer(X.T @ xu, (df * c + f * c_diff) @ X) - f * c * (X.T @ X - np.outer(sX, sX) / N))
            - np.outer(X.T @ gv, w @ X) + np.outer(X.T @ u, sX))


def hess_self(mt, vt, N, c1, c2, X):
    """cmptSelfHessian, SSIM.cc:270-287"""
    cs, ds = 2 * mt * mt + c1, 2 * vt + c2
    cds = cs * ds
    m1, m2 = 2.0 / (N * cds), 2.0 / ((N - 1) * cds)
    sX = X.sum(axis=0)
    return cs * m1 * (np.outer(sX, sX) / N - X.T @ X) - (m2 * ds / N) * np.outer(sX, sX)


def quantities(I0, It, J0, Jt, c1, c2, dtype=np.float64, int_quot=True):
    """every summed quantity of one pass, evaluated in dtype from the float64 inputs"""
    I0, It, J0, Jt = (np.asarray(v, dtype=dtype) for v in (I0, It, J0, Jt))
    s = scalars(I0, It, dtype(c1), dtype(c2))
    Jm = (J0 + Jt) / 2
    return {"f": s["f"], "df_dIt": s["df_dIt"], "df_dI0": s["df_dI0"], "g_curr": s["df_dIt"] @ Jt, "g_init": s["df_dI0"] @ J0,
            "g_mean": s["df_dIt"] @ Jm, "H_self": hess_self(s["mt"], s["vt"], s["N"], s["c1"], s["c2"], Jt),
            "H_curr": hess_std(s, Jt, True, int_quot), "H_init": hess_std(s, J0, False, int_quot), "H_mean": hess_std(s, Jm, True, int_quot),
            "scalars": s}


def self_hessian0(I0, J0, c1, c2, dtype=np.float64):
    I0, J0 = np.asarray(I0, dtype=dtype), np.asarray(J0, dtype=dtype)
    s = scalars(I0, I0, dtype(c1), dtype(c2))
    return hess_self(s["m0"], s["v0"], s["N"], s["c1"], s["c2"], J0)


def likelihood(f, alpha=1.0):
    d = (1.0 / f) - 1
    return np.exp(-alpha * d * d)


def g_and_H(q, H0, method):
    sm, jac, ht = METHODS[method] if isinstance(method, str) else method
    if sm == 1:
        return q["g_curr"], (H0 if ht == 0 else (q["H_self"] if ht == 1 else q["H_curr"]))
    if sm == 2:
        return q["g_init"], (H0 if ht == 0 else (q["H_self"] if ht == 1 else q["H_init"]))
    g = q["g_mean"] if jac == 0 else 0.5 * (q["g_curr"] - q["g_init"])
    H = {0: H0, 1: q["H_self"], 2: 0.5 * (q["H_self"] + H0), 3: q["H_mean"], 4: 0.5 * (q["H_init"] + q["H_curr"]), 5: q["H_curr"]}[ht]
    return g, H


def run_loop(mo, W, c1, c2, H0, method, leven_marq, eps):
    """make_golden10.run_loop over a Model: passes done, final warp, and the corner changes of the solved steps"""
    iclk, fclk = method.startswith("iclk"), method.startswith("fclk")
    prev_f, delta, state_reset, it_id, last_dp = 0.0, LM_DELTA, False, 0, None
    passes, changes = 0, []
    max_passes = 2 * N_ITERS if (leven_marq and fclk) else N_ITERS
    while passes < max_passes:
        It, Jt = mo.sample(W)
        q = quantities(mo.I0, It, mo.J0, Jt, c1, c2)
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
        before = mo.corners_of(W)
        W = mo.compose(W, dp, inverse=(iclk != undo))
        change = float(((before - mo.corners_of(W)) ** 2).sum())
        passes += 1
        it_id += 0 if (undo and fclk) else 1
        if not undo:
            changes.append(change)
        if (not undo and change < eps) or it_id >= N_ITERS:
            break
    return passes, W, changes


def rel_floor(x64, xld):
    xld = np.asarray(xld, dtype=np.longdouble)
    return float(np.abs(np.asarray(x64, dtype=np.longdouble) - xld).max() / np.abs(xld).max())


JITTER_PX = 1e-12
JITTER_SHIFTS = (np.array([[JITTER_PX], [JITTER_PX]]), np.array([[-JITTER_PX], [-JITTER_PX]]), np.array([[JITTER_PX], [-JITTER_PX]]))


def updates(img, resx, resy, ssm, corners, p, c1, c2):
    """the eight stored updates dp of a case laid out on `corners`"""
    mo = Model(img, resx, resy, ssm, corners)
    It, Jt = mo.sample(mo.warp(p), p)
    q, H0 = quantities(mo.I0, It, mo.J0, Jt, c1, c2), self_hessian0(mo.I0, mo.J0, c1, c2)
    return {m: -np.linalg.solve(g_and_H(q, H0, m)[1], g_and_H(q, H0, m)[0]) for m in METHODS}


def dp_jitter(img, resx, resy, ssm, corners, p, c1, c2):
    """how far the reference's OWN updates move, relative to their largest entry, when the region's corners move by 1e-12 px (three shifts; the
    largest over the eight methods): every sample point then changes in its last bits, which the 1e-8-step central difference of the image
    gradient amplifies -- the floor under any comparison of an update with one computed in other arithmetic from the same region"""
    base = updates(img, resx, resy, ssm, corners, p, c1, c2)
    worst = 0.0
    for sh in JITTER_SHIFTS:
        moved = updates(img, resx, resy, ssm, corners + sh, p, c1, c2)
        worst = max(worst, max(float(np.abs(moved[m] - base[m]).max() / np.abs(base[m]).max()) for m in METHODS))
    return worst


def build():
    rng = np.random.default_rng(SEED)
    img = make_image()
    out = {"img": img, "tags": np.array([c[0] for c in CASES]), "loop_cfg": np.array([N_ITERS, LM_DELTA, LM_UPDATE])}
    drawn = {}
    outside = False
    loops = {}     # group (resx, resy, ssm, k1, k2) -> [(tag, model, W, c1, c2, H0)]
    for tag, k1, k2, resx, resy, ssm, corners, scale in CASES:
        mo = Model(img.astype(np.float64), resx, resy, ssm, corners)
        key = (resx, resy, ssm, corners.tobytes())
        if key not in drawn:
            drawn[key] = mo.draw(rng, scale)
        p = drawn[key]
        c1, c2 = ssim_c(k1), ssim_c(k2)
        W = mo.warp(p)
        It, Jt = mo.sample(W, p)
        q = quantities(mo.I0, It, mo.J0, Jt, c1, c2)
        ql = quantities(mo.I0, It, mo.J0, Jt, c1, c2, dtype=np.longdouble)
        qf = quantities(mo.I0, It, mo.J0, Jt, c1, c2, int_quot=False)
        H0 = self_hessian0(mo.I0, mo.J0, c1, c2)
        H0l = self_hessian0(mo.I0, mo.J0, c1, c2, dtype=np.longdouble)
        if not mo.low:
            wp = W @ mo.pa.init_hm
            wp = wp[:2] / wp[2]
            outside = outside or bool((wp[0] >= IMG_SIDE).any() or (wp[1] >= IMG_SIDE).any() or (wp < 0).any())
        rec = {tag + "_cfg": np.array([resx, resy, ssm]), tag + "_k": np.array([k1, k2]), tag + "_corners": corners, tag + "_p": p,
               tag + "_It": It, tag + "_H0": H0,
               tag + "_err_floor_H0": rel_floor(H0, H0l), tag + "_H_curr_fq": qf["H_curr"]}
        for name in ("f", "g_curr", "g_init", "g_mean", "H_self", "H_curr", "H_init", "H_mean"):
            rec[tag + "_" + name] = np.asarray(q[name], dtype=np.float64)
            rec[tag + "_err_floor_" + name] = rel_floor(q[name], ql[name])
        for method in METHODS:
            g, H = g_and_H(q, H0, method)
            gl, Hl = g_and_H(ql, H0l, method)
            rec[tag + "_" + method + "_dp"] = -np.linalg.solve(H, g)
            rec[tag + "_err_floor_" + method + "_H"] = rel_floor(H, Hl)
            rec[tag + "_err_floor_" + method + "_g"] = rel_floor(g, gl)
        rec[tag + "_dp_jitter"] = dp_jitter(img.astype(np.float64), resx, resy, ssm, corners, p, c1, c2)
        free = {m: [run_loop(mo, W, c1, c2, H0, m, lm, 0.0) for lm in (False, True)] for m in LOOPS}
        ok = {m: all(r[2][-1] < CONTRACTED for r in free[m]) for m in LOOPS}
        rec[tag + "_well"] = np.array([int(ok[m]) for m in LOOPS])
        if any(ok.values()):
            loops.setdefault((resx, resy, ssm, k1, k2), []).append((tag, mo, W, c1, c2, H0))
        out.update(rec)
    assert outside, "no case samples past the frame"
    for k, m in enumerate(LOOPS):
        kinds = {int(out[g[0] + "_cfg"][2]) for grp in loops.values() for g in grp if out[g[0] + "_well"][k]}
        assert HOM in kinds, "%s: no well-conditioned homography case" % m
        assert AFF in kinds, "%s: no well-conditioned affine case" % m
        assert kinds & {SIM, ISO, TRA}, "%s: no well-conditioned low-order case" % m
    for group in loops.values():
        best = None
        for eps in EPS_CANDIDATES:
            runs = {(g[0], m, lm): run_loop(*g[1:], m, lm, eps) for g in group for k, m in enumerate(LOOPS) if out[g[0] + "_well"][k]
                    for lm in (False, True)}
            margin = min(M10.eps_margin(r[2], eps) for r in runs.values())
            if best is None or margin > best[0]:
                best = (margin, eps, runs)
        margin, eps, runs = best
        assert margin > 2, "%s: a corner change within a factor %.2f of every candidate epsilon" % (group[0][0], margin)
        for tag, mo, W, c1, c2, H0 in group:
            out[tag + "_eps"] = eps
            for k, m in enumerate(LOOPS):
                if not out[tag + "_well"][k]:
                    continue
                for lm in (False, True):
                    passes, Wn, _ = runs[(tag, m, lm)]
                    pre = tag + "_" + m + ("_lm" if lm else "") + "_loop"
                    out[pre + "_n"] = passes
                    out[pre + "_state"] = mo.state_of(Wn)
                    out[pre + "_corners"] = mo.corners_of(Wn)
    return out


def main():
    out = build()
    path = os.path.join(HERE, "lk_golden11.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for t in out["tags"]:
        t = str(t)
        print(t, "well", out[t + "_well"].tolist(), "eps", out.get(t + "_eps"), "f %.6f" % float(out[t + "_f"]),
              {m: int(out[t + "_" + m + "_loop_n"]) for m in LOOPS if t + "_" + m + "_loop_n" in out}, "dp_jitter %.1e" % float(out[t + "_dp_jitter"]))


if __name__ == "__main__":
    main()
