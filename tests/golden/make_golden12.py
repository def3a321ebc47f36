#!/usr/bin/env python
"""Generates tests/golden/lk_golden12.npz: the Cross Cumulative Residual Entropy appearance model (CCRE, AM/src/CCRE.cc; first order,
symmetrical_grad = 0, true cumulative histograms) from an independent float64 NumPy restatement of its definition, written from the table
below (the C++ oracle has no CCRE).

Pixel values: v = add + mult raw, mult = (hi - lo) / 255, (lo, hi) = (0, nb - 1), or (1, nb - 2) with partition of unity; add = lo.
norm = 1 / (N + nb^2 pre_seed).  A pixel's window is [max(0, floor(v) - 1), min(nb - 1, floor(v) + 2)]; tap k of it sits at
x_k = (first bin - v) + k, accumulated by +1 as the reference does.  With b3 the cubic B-spline and c3 its cumulative form (1 at x <= -2,
0 from 2 on; the piecewise forms and the truncated constants 0.33333333333 / 0.66666666666 of the reference's *WithGrad functions):
  beta_j(p)  = b3(x)            beta'_j = -norm b3'(x)          beta''_j = norm b3''(x)        over the window of I0(p), else 0
  C_i(p)     = 1 below the window of It(p), c3(x) inside it, 0 ABOVE it (the reference leaves stale values there: not kept)
  C'_i       = -norm c3'(x)     C''_i = norm c3''(x)            inside the window, else 0
  cum_joint(i, j) = norm (pre_seed + sum_p C_i beta_j)     cum_hist(i) = norm (nb pre_seed + sum_p C_i)     hist_0(j) = norm (nb pre_seed + sum_p beta_j)
  L(i, j) = log cum_joint - log cum_hist(i) - log hist_0(j)            f = sum cum_joint L
  df_dIt(p) = sum_ij C'_i beta_j L(i, j)
  df_dI0(p) = sum_j beta'_j [ sum_i C_i (1 + L(i, j)) - colsum(j) / hist_0(j) ],   colsum(j) = sum_i cum_joint(i, j)
  H_curr(J)  = sum_p [sum_ij C''_i beta_j L] J_p^T J_p + sum_ij (1 / cum_joint - 1 / cum_hist(i)) r_ij^T r_ij,   r_ij = sum_p C'_i beta_j J_p
  H_self(J)  = the same with beta(It), hist_t(j) = norm (nb pre_seed + sum_p beta_j(It)) and the self joint / log term
  H_init(J0) = sum_ij r_ij^T (r_ij / cum_joint - 2 G_j) + sum_j colsum(j) G_j^T G_j
               + sum_p [sum_j beta''_j (sum_i C_i (1 + L(i, j)) - colsum(j) / hist_0(j))] J0_p^T J0_p,
               r_ij = sum_p C_i beta'_j J0_p,  G_j = sum_p (beta'_j / hist_0(j)) J0_p          (not symmetric: kept as written)
initializeSimilarity / initializeGrad are the same with It = I0.  H0 = H_self(J0) at It = I0.  Search-method algebra as make_golden10.py's,
plus esm_std (ESM, SumOfStd): g = (g_curr - g_init) / 2, H = (H_init(J0) + H_curr(Jt)) / 2.

Per case: cfg (resx, resy, affine, n_bins, partition_of_unity), pre_seed, corners, the state p, I0 and It (normalised), f and f_init, df_dIt,
df_dI0, df_init, the raw sums and tables (for the shared tables header), g_curr, g_init, g_mean, H_self, H_curr, H_init, H_mean, H0, dp of
every method, and err_floor_*: the float64 evaluation against the same sums in np.longdouble, relative to the largest entry.  For the
loops of esm_ds, fclk_cs, iclk_is without and with Levenberg-Marquardt (0.01, 10), every case: passes, state, corners, and what to run
(<run>_loop_iters, _loop_eps).  A run that contracts (its last solved step moves the corners by less than CONTRACTED) is the whole
10-iteration loop with a corner-change test.  CCRE does not contract on every patch -- with 63 or 143 pixels the seeding, nb^2 pre_seed, outweighs
the pixels and the objective is nearly flat; from the identity such runs wander as well -- and a wandering loop amplifies the last bit of its start
by a factor per pass: such a run is stored without a test (epsilon 0) up to the last iteration at which the same loop with its first update shifted by
STATE_SHIFT stays within SHIFT_PX of it in its corners and in its state, which is as far as it pins a second implementation;
the epsilon of a group as make_golden10.py chooses it, with no corner change within a factor 1.5 of it (the device's corners agree with
these to 1e-6 px or better, which moves a squared change of 1e-4 px^2 by a few per cent at most).

The image is make_golden10.py's (a block at 0, one at 255, texture) with one region quantised to multiples of 17: with 16 bins the scaling
is 1 / 17, so every normalised value sampled there ON the pixel lattice is an exact integer -- on the branch boundaries of both splines.

Run from the repo root:  python tests/golden/make_golden12.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
from mtf_amd import synth  # noqa: E402
import make_golden10 as G10  # noqa: E402  (the sample grid and the warps: geometry only)

SEED = 20261020
N_ITERS = 10
EPS_CANDIDATES = G10.EPS_CANDIDATES
CONTRACTED = 1e-2
STATE_SHIFT, SHIFT_PX = 1e-11, 2e-4 / 16      # (2e-4 px: the bound the device loops are held to)
LM_DELTA, LM_UPDATE = 0.01, 10.0
PRE_SEED = 10.0
Q_ROWS, Q_COLS, Q_STEP = slice(120, 176), slice(100, 176), 17.0

_rect = G10._rect
# (tag, n_bins, pou, pre_seed, resx, resy, affine, corners, scale of p | an explicit state | (tag, factor): that case's state times factor)
CASES = (
    ("h50a", 8, 0, PRE_SEED, 50, 50, False, synth.square_corners(64, 64, 70), 0.10),       # pixels at exactly 0 and 255
    ("h50b", 8, 0, PRE_SEED, 50, 50, False, synth.square_corners(64, 64, 70), ("h50a", 0.5)),    # the same template from half h50a's state
    ("h50c", 8, 0, PRE_SEED, 50, 50, False, synth.square_corners(64, 64, 70), ("h50a", 0.0)),    # ... and from the identity
    ("h50p10", 10, 1, PRE_SEED, 50, 50, False, synth.square_corners(64, 64, 70), 0.10),    # h50a's region and state
    ("h50s0", 8, 0, 0.5, 50, 50, False, synth.square_corners(64, 64, 70), 0.10),           # ... at another pre_seed
    ("a25x20", 16, 0, PRE_SEED, 25, 20, True, _rect(20, 110, 68, 148), 0.2),
    ("a25x20i", 16, 0, PRE_SEED, 25, 20, True, _rect(110, 125, 134, 144, jitter=0.0), np.array([1.0, 0, 0, 0, 0, 0])),   # integers
    ("h7x9p4", 4, 1, PRE_SEED, 7, 9, False, _rect(100, 20, 121, 47), 0.1),
    ("h13x11b2", 2, 0, PRE_SEED, 13, 11, False, _rect(30, 100, 69, 133), 0.05),
    ("h13x11", 8, 0, 1.0, 13, 11, False, _rect(30, 100, 69, 133), 0.05),        # (pre_seed 1: at 10 the 640 seeds outweigh the 143 pixels)
)
METHODS = ("esm_ds", "esm_oo", "esm_std", "fclk_cs", "fclk_std", "iclk_is", "iclk_std")
LOOPS = ("esm_ds", "fclk_cs", "iclk_is")
SUMMED = ("f", "g_curr", "g_init", "g_mean", "H_self", "H_curr", "H_init", "H_mean")


def make_image():
    img = G10.make_image().astype(np.float64)
    img[Q_ROWS, Q_COLS] = np.clip(np.rint(img[Q_ROWS, Q_COLS] / Q_STEP) * Q_STEP, 0.0, 255.0)
    return img.astype(np.float32)


def pix_norm(nb, pou):
    lo, hi = (1.0, nb - 2.0) if pou else (0.0, nb - 1.0)
    return (hi - lo) / 255.0, lo


# ---- the splines, piece by piece with the reference's boundaries (x <= -1, x <= 0, ...) ----
K13, K23 = 0.33333333333, 0.66666666666


def _pieces(x, p0, p1, p2, p3, below, above):
    """the value per piece: (-2, -1], (-1, 0], (0, 1], (1, 2); `below` at x <= -2, `above` from 2 on"""
    out = np.full(x.shape, above, dtype=x.dtype)
    out = np.where(x < 2, p3, out)
    out = np.where(x <= 1, p2, out)
    out = np.where(x <= 0, p1, out)
    out = np.where(x <= -1, p0, out)
    return np.where(x <= -2, x.dtype.type(below), out)


def b3(x):
    t0, t3 = 2 + x, 2 - x
    return _pieces(x, (t0 * t0 / 2) * t0 / 3, K23 - x * x * (1 + x / 2), K23 - x * x * (1 - x / 2), (t3 * t3 / 2) * t3 / 3, 0, 0)


def b3_d(x):
    t0, t3 = 2 + x, 2 - x
    return _pieces(x, t0 * t0 / 2, -x * (x / 2 + x + 2), x * (x / 2 + x - 2), -(t3 * t3) / 2, 0, 0)


def b3_dd(x):
    return _pieces(x, 2 + x, -(3 * x + 2), 3 * x - 2, 2 - x, 0, 0)


def c3(x):
    t0, t3 = 2 + x, x - 2
    x2 = x * x
    return _pieces(x, 1 + (-(t0 * t0 * t0) / 6 * t0) / 4, 0.5 + x * (x2 * (K13 + x / 8) - K23), 0.5 + x * (x2 * (K13 - x / 8) - K23),
                   ((t3 * t3 * t3) / 6 * t3) / 4, 1, 0)


def c3_d(x):
    t0, t3 = 2 + x, x - 2
    x2 = x * x
    return _pieces(x, -(t0 * t0 * t0) / 6, x2 * (1 + x / 2) - K23, x2 * (1 - x / 2) - K23, (t3 * t3 * t3) / 6, 0, 0)


def c3_dd(x):
    t0, t3 = 2 + x, 2 - x
    return _pieces(x, -(t0 * t0) / 2, x * (3 * x + 4) / 2, -x * (3 * x - 4) / 2, (t3 * t3) / 2, 0, 0)


def window_rows(v, nb, funcs, dtype):
    """dense [len(funcs)][nb][N] rows of the functions over every pixel's window, zero elsewhere; and the window's first bin"""
    v = np.asarray(v, dtype=dtype)
    fl = np.trunc(np.asarray(v, dtype=np.float64)).astype(np.int64)
    lo, hi = np.maximum(0, fl - 1), np.minimum(nb - 1, fl + 2)
    out = np.zeros((len(funcs), nb, v.size), dtype=dtype)
    x = lo.astype(dtype) - v
    cols = np.arange(v.size)
    for k in range(4):
        sel = lo + k <= hi
        for m, fn in enumerate(funcs):
            out[m, (lo + k)[sel], cols[sel]] = fn(x)[sel]
        x = x + 1
    return out, lo


def weights(I0, It, nb, norm, dtype):
    """beta, beta', beta'' of I0 ; C, C', C'' of It ; beta of It (the self histogram)"""
    (B, dB, ddB), _ = window_rows(I0, nb, (b3, b3_d, b3_dd), dtype)
    (Cw, dC, ddC), lo = window_rows(It, nb, (c3, c3_d, c3_dd), dtype)
    (Bt,), _ = window_rows(It, nb, (b3,), dtype)
    below = np.arange(nb)[:, None] < lo[None, :]
    C = np.where(below, dtype(1), Cw)
    return B, -norm * dB, norm * ddB, C, -norm * dC, norm * ddC, Bt


def tables(C, B, nb, pre_seed, norm, hist_b=None):
    """cum_hist, cum_joint, hist of the plain side (hist_b: its own weights when they are not B's), L, f, colsum"""
    raw_cum, raw_joint, raw_hist = C.sum(axis=1), C @ B.T, (B if hist_b is None else hist_b).sum(axis=1)
    cum_hist, cum_joint, hist = norm * (nb * pre_seed + raw_cum), norm * (pre_seed + raw_joint), norm * (nb * pre_seed + raw_hist)
    L = np.log(cum_joint) - np.log(cum_hist)[:, None] - np.log(hist)[None, :]
    return dict(raw_cum=raw_cum, raw_joint=raw_joint, raw_hist=raw_hist, cum_hist=cum_hist, cum_joint=cum_joint, hist=hist, L=L,
                f=(cum_joint * L).sum(), colsum=cum_joint.sum(axis=0))


def pair_hessian(dC, ddC, B, L, joint, cum_hist, J):
    """H_curr / H_self: the per-pixel term plus the bin-pair terms"""
    term = np.einsum("ip,jp,ij->p", ddC, B, L)
    r = np.einsum("ip,jp,ps->ijs", dC, B, J)
    fac = 1 / joint - 1 / cum_hist[:, None]
    return (J * term[:, None]).T @ J + np.einsum("ijs,ijt,ij->st", r, r, fac)


def init_hessian(C, dB, ddB, t, J0):
    """H_init(J0) as written in CCRE.cc:521-560 (not symmetric)"""
    r = np.einsum("ip,jp,ps->ijs", C, dB, J0)
    G = (dB / t["hist"][:, None]) @ J0
    H = np.einsum("ijs,ijt->st", r, r / t["cum_joint"][:, :, None] - 2 * G[None, :, :]) + np.einsum("j,js,jt->st", t["colsum"], G, G)
    inner = np.einsum("ip,ij->jp", C, t["L"] + 1) - (t["colsum"] / t["hist"])[:, None]
    term = (ddB * inner).sum(axis=0)
    return H + (J0 * term[:, None]).T @ J0


def quantities(I0, It, J0, Jt, nb, pre_seed, dtype=np.float64):
    """every quantity of one pass, evaluated in dtype from the float64 inputs"""
    I0, It, J0, Jt = (np.asarray(v, dtype=dtype) for v in (I0, It, J0, Jt))
    pre_seed = dtype(pre_seed)
    norm = 1 / (dtype(I0.size) + nb * nb * pre_seed)
    B, dB, ddB, C, dC, ddC, Bt = weights(I0, It, nb, norm, dtype)
    t = tables(C, B, nb, pre_seed, norm)
    ts = tables(C, Bt, nb, pre_seed, norm)
    dft = np.einsum("ip,jp,ij->p", dC, B, t["L"])
    inner = np.einsum("ip,ij->jp", C, t["L"] + 1) - (t["colsum"] / t["hist"])[:, None]
    df0 = (dB * inner).sum(axis=0)
    Jm = (J0 + Jt) / 2
    return {"f": t["f"], "df_dIt": dft, "df_dI0": df0, "g_curr": dft @ Jt, "g_init": df0 @ J0, "g_mean": dft @ Jm,
            "H_curr": pair_hessian(dC, ddC, B, t["L"], t["cum_joint"], t["cum_hist"], Jt),
            "H_mean": pair_hessian(dC, ddC, B, t["L"], t["cum_joint"], t["cum_hist"], Jm),
            "H_self": pair_hessian(dC, ddC, Bt, ts["L"], ts["cum_joint"], t["cum_hist"], Jt),
            "H_init": init_hessian(C, dB, ddB, t, J0), "tables": t, "self_tables": ts}


def self_hessian_on(I0, It, J, nb, pre_seed, dtype=np.float64):
    """cmptSelfHessian(J) of a patch It (the template enters only through updateSimilarity's tables, which the self Hessian does not read)"""
    q = quantities(I0, It, J, J, nb, pre_seed, dtype)
    return q["H_self"]


def g_and_H(q, H0, method):
    if method == "esm_std":
        return 0.5 * (q["g_curr"] - q["g_init"]), 0.5 * (q["H_init"] + q["H_curr"])
    return G10.g_and_H(q, H0, method)


def run_loop(pa, mult, add, W, nb, pre_seed, H0, affine, corners, method, leven_marq, first_dp_shift=0.0):
    """the search method's update() from the warp W WITHOUT a convergence test, pass by pass (make_golden10.run_loop's Levenberg-Marquardt):
    [(undo, corner change, warp after the pass, iteration counter after it)] -- a test at any epsilon stops a prefix of this (stop_at)"""
    chm = np.vstack([corners, np.ones(4)])
    iclk, fclk = method.startswith("iclk"), method.startswith("fclk")
    prev_f, delta, state_reset, it_id, last_dp = 0.0, LM_DELTA, False, 0, None
    rec = []
    max_passes = 2 * N_ITERS if (leven_marq and fclk) else N_ITERS
    while len(rec) < max_passes and it_id < N_ITERS:
        It, Jt = pa.sample(W)
        q = quantities(mult * pa.I0o + add, mult * It + add, mult * pa.J0, mult * Jt, nb, pre_seed)
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
            if not rec:
                dp = dp + first_dp_shift      # (the sensitivity probe of main: what the rounding of the first solve does to the rest)
            last_dp = dp
        before = G10.corners_of(W, chm)
        W = G10.compose(W, dp, affine, inverse=(iclk != undo))
        change = float(((before - G10.corners_of(W, chm)) ** 2).sum())
        it_id += 0 if (undo and fclk) else 1
        rec.append((undo, change, W, it_id))
    return rec


def stop_at(rec, eps):
    """passes done with the corner-change test at eps, and the solved steps' changes up to there"""
    changes = []
    for k, (undo, change, _, it_id) in enumerate(rec):
        if not undo:
            changes.append(change)
        if (not undo and change < eps) or it_id >= N_ITERS:
            return k + 1, changes
    return len(rec), changes


def main():
    rng = np.random.default_rng(SEED)
    img = make_image()
    img64 = img.astype(np.float64)
    out = {"img": img, "tags": np.array([c[0] for c in CASES]), "loop_cfg": np.array([N_ITERS, LM_DELTA, LM_UPDATE])}
    drawn, loops = {}, {}
    for tag, nb, pou, pre_seed, resx, resy, affine, corners, scale in CASES:
        key = (resx, resy, affine, corners.tobytes())
        if isinstance(scale, np.ndarray):
            p = scale
        elif isinstance(scale, tuple):
            p = scale[1] * out[scale[0] + "_p"]
        else:
            if key not in drawn:
                drawn[key] = (rng.uniform(-1, 1, 6) * [1.2, 1.2, 0.02, 0.02, 0.02, 0.02] * scale if affine
                              else synth.random_small_homography(rng, scale))
            p = drawn[key]
        mult, add = pix_norm(nb, pou)
        pa = G10.Patch(img64, resx, resy, affine, corners)
        W = pa.warp(p)
        It_raw, Jt_raw = pa.sample(W, p)
        I0, It, J0, Jt = mult * pa.I0o + add, mult * It_raw + add, mult * pa.J0, mult * Jt_raw
        q = quantities(I0, It, J0, Jt, nb, pre_seed)
        ql = quantities(I0, It, J0, Jt, nb, pre_seed, dtype=np.longdouble)
        q0 = quantities(I0, I0, J0, J0, nb, pre_seed)
        H0 = q0["H_self"]
        if tag == "h50a":
            assert (I0 == 0).sum() > 20 and (I0 == nb - 1).sum() > 20 and (It == nb - 1).sum() > 20, "no pixels at exactly 0 / 255"
        if tag == "a25x20i":
            n_int = int((I0 == np.rint(I0)).sum()), int((It == np.rint(It)).sum())
            assert min(n_int) > I0.size // 2, "the quantised region gives %s integer values" % (n_int,)
            out["n_integer"] = np.array(n_int)
        t, ts = q["tables"], q["self_tables"]
        rec = {tag + "_cfg": np.array([resx, resy, int(affine), nb, pou]), tag + "_pre_seed": pre_seed, tag + "_corners": corners, tag + "_p": p,
               tag + "_I0": I0, tag + "_It": It, tag + "_df_dIt": q["df_dIt"], tag + "_df_dI0": q["df_dI0"], tag + "_df_init": q0["df_dIt"],
               tag + "_f_init": q0["f"], tag + "_H0": H0,
               tag + "_err_floor_df_dIt": G10.rel_floor(q["df_dIt"], ql["df_dIt"]), tag + "_err_floor_df_dI0": G10.rel_floor(q["df_dI0"], ql["df_dI0"]),
               # the raw sums a histogram pass hands the tables kernel, and what it makes of them
               tag + "_raw": np.concatenate([t["raw_cum"], t["raw_joint"].ravel(), ts["raw_cum"], ts["raw_joint"].ravel(), ts["raw_hist"]]),
               tag + "_raw_hist0": t["raw_hist"], tag + "_cum_hist": t["cum_hist"], tag + "_cum_joint": t["cum_joint"], tag + "_hist0": t["hist"],
               tag + "_L": t["L"], tag + "_colsum": t["colsum"], tag + "_self_joint": ts["cum_joint"], tag + "_self_L": ts["L"], tag + "_hist_t": ts["hist"]}
        for name in SUMMED:
            rec[tag + "_" + name] = np.asarray(q[name], dtype=np.float64)
            rec[tag + "_err_floor_" + name] = G10.rel_floor(q[name], ql[name])
        for method in METHODS:
            g, H = g_and_H(q, H0, method)
            gl, Hl = g_and_H(ql, np.asarray(H0, dtype=np.longdouble), method)
            rec[tag + "_" + method + "_dp"] = -np.linalg.solve(H, g)
            rec[tag + "_err_floor_" + method + "_dp"] = G10.rel_floor(rec[tag + "_" + method + "_dp"],
                                                                      -np.linalg.solve(np.asarray(Hl, dtype=np.float64), np.asarray(gl, dtype=np.float64)))
        out.update(rec)
        free = {(m, lm): run_loop(pa, mult, add, W, nb, pre_seed, H0, affine, corners, m, lm) for m in LOOPS for lm in (False, True)}
        # a run is kept whole when it is contracting as it ends: its last solved step moves the corners by less than CONTRACTED (squared, summed)
        kept = {k: r for k, r in free.items() if [c for u, c, _, _ in r if not u][-1] < CONTRACTED}
        if kept:
            loops.setdefault((resx, resy, affine, nb, pou, pre_seed), []).append((tag, affine, corners, kept))
        # every other run is kept as far as it pins anything: the same loop with its FIRST update shifted by STATE_SHIFT (about what the rounding of
        # one solve moves it by; the start itself is the same bits everywhere) -- the record ends with the last iteration up to which the two runs'
        # corners and states stay within SHIFT_PX of each other
        chm = np.vstack([corners, np.ones(4)])
        for (m, lm), r in free.items():
            if (m, lm) in kept:
                continue
            r2 = run_loop(pa, mult, add, W, nb, pre_seed, H0, affine, corners, m, lm, first_dp_shift=STATE_SHIFT)
            iters = 0
            for k in range(min(len(r), len(r2))):
                same = (r[k][0] == r2[k][0] and np.abs(G10.corners_of(r[k][2], chm) - G10.corners_of(r2[k][2], chm)).max() < SHIFT_PX and
                        np.abs(G10.state_of(r[k][2], affine) - G10.state_of(r2[k][2], affine)).max() < SHIFT_PX)
                if not same:
                    break
                iters = r[k][3]
            # (a pass that takes an update back does not advance FCLK's counter: the prefix ends where the counter first reaches `iters`)
            passes = next(k + 1 for k in range(len(r)) if r[k][3] >= iters) if iters else 0
            assert iters >= 1, "%s %s lm %d: not one pass survives the shifted start" % (tag, m, lm)
            pre = tag + "_" + m + ("_lm" if lm else "") + "_loop"
            Wn = r[passes - 1][2]
            out[pre + "_n"], out[pre + "_iters"], out[pre + "_eps"] = passes, iters, 0.0
            out[pre + "_state"], out[pre + "_corners"] = G10.state_of(Wn, affine), G10.corners_of(Wn, chm)
        print(tag, "f %.6g" % q["f"], "whole loops:", sorted(kept), "cut:", {k: int(out[tag + "_" + k[0] + ("_lm" if k[1] else "") + "_loop_iters"])
                                                                            for k in free if k not in kept})
    for group in loops.values():
        best = None
        for eps in EPS_CANDIDATES:
            margin = min(G10.eps_margin(stop_at(r, eps)[1], eps) for g in group for r in g[3].values())
            if best is None or margin > best[0]:
                best = (margin, eps)
        margin, eps = best
        assert margin > 1.5, "%s: a corner change within a factor %.2f of every candidate epsilon" % (group[0][0], margin)
        for tag, affine, corners, free in group:
            out[tag + "_eps"] = eps
            chm = np.vstack([corners, np.ones(4)])
            for (m, lm), r in free.items():
                passes, _ = stop_at(r, eps)
                Wn = r[passes - 1][2]
                pre = tag + "_" + m + ("_lm" if lm else "") + "_loop"
                out[pre + "_n"], out[pre + "_iters"], out[pre + "_eps"] = passes, N_ITERS, eps
                out[pre + "_state"] = G10.state_of(Wn, affine)
                out[pre + "_corners"] = G10.corners_of(Wn, chm)
    batch3 = [int(out["h50%s_esm_ds_loop_n" % s]) for s in "abc"]
    assert len(set(batch3)) > 1, "the three 50 x 50 targets stop at the same pass: %s" % batch3
    path = os.path.join(HERE, "lk_golden12.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
