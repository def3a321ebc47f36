"""NumPy float64 restatement of NCC::estimateOpticalFlow (AM/src/NCC.cc:412-526) and of nt::GridTrackerFlow
(SM/src/NT/GridTrackerFlow.cc:74-126), written from the cited lines.  Test infrastructure: PARITY UNPINNED -- the reference itself cannot be
built here (no Eigen, no OpenCV), so nothing pins this file to its bits; it is the operation order of the cited lines in IEEE double.

What is restated, and how:
  * the lattice: VectorXd::LinSpaced(n, lo, hi) as Eigen forms it (lo + i * ((hi - lo) / (n - 1)), the last element hi), NCC.cc:427-433;
  * the sampler: utils::sc::PixVal<Linear, Constant>::get (imgUtils.h:91-113, overflow value 128) -- `pix_val` is the scalar routine,
    `pix_vals` evaluates the same expression in the same order for every element of an array (elementwise IEEE operations: the same
    bits; tests/test_flow_cpu.py checks the two against each other); raw pixel values, no norm_mult / norm_add;
  * getPixValsWithGrad (imgUtils.h:337-366): central differences at x +- grad_eps, y +- grad_eps times 1 / (2 grad_eps);
  * the explicit loops of NCC.cc:457-460, 478-482, 489-494, 498-501 as serial left-to-right sums; Eigen's own reductions (mean(),
    colwise().mean(), the matrix products of :503-505) as serial sums as well -- Eigen's vectorised order is not knowable from the source,
    and the difference is one of summation order only;
  * colPivHouseholderQr().solve for the 2 x 2 system: the column-pivoted Householder QR of the project's checker (mtfo_colpiv_qr_solve),
    written out for n = 2; a system with a non-finite entry gives a non-finite step (the checker's routine would call it rank 0);
  * curr_pts accumulates in float32 (cv::Point2f, :516-517), win_x / win_y in double, element by element, every pass (:518-519);
  * the break (:520) comes after the update.
A non-finite step ends the point: the reference goes on sampling at NaN coordinates, which is undefined behaviour; the record says so
(status 0) and the point is NaN, as the device reports it.
"""
import math

import numpy as np

NONFINITE, CONVERGED, MAX_ITERS = 0, 1, 2


def lin_spaced(n, lo, hi):
    out = np.empty(n)
    step = (hi - lo) / (n - 1) if n > 1 else 0.0
    for i in range(n):
        out[i] = hi if (n == 1 or i == n - 1) else lo + i * step
    return out


def pix_val(img, x, y):
    """the scalar sampler, imgUtils.h:91-113"""
    h, w = img.shape
    if x < 0 or x >= w or y < 0 or y >= h or not (math.isfinite(x) and math.isfinite(y)):
        return 128.0
    lx, ly = int(x), int(y)
    dx, dy = x - lx, y - ly
    ux = lx if dx == 0 else lx + 1
    uy = ly if dy == 0 else ly + 1
    if ux >= w or uy >= h:
        return 128.0
    t00, t01, t10, t11 = float(img[ly, lx]), float(img[ly, ux]), float(img[uy, lx]), float(img[uy, ux])
    return t00 * (1 - dx) * (1 - dy) + t01 * dx * (1 - dy) + t10 * (1 - dx) * dy + t11 * dx * dy


def pix_vals(img, x, y):
    """pix_val for arrays of coordinates: the same expression, the same order, per element"""
    h, w = img.shape
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    fin = np.isfinite(x) & np.isfinite(y)
    with np.errstate(invalid="ignore"):
        inside = fin & ~((x < 0) | (x >= w) | (y < 0) | (y >= h))
    xs, ys = np.where(inside, x, 0.0), np.where(inside, y, 0.0)
    lx, ly = xs.astype(np.int64), ys.astype(np.int64)
    dx, dy = xs - lx, ys - ly
    ux, uy = np.where(dx == 0, lx, lx + 1), np.where(dy == 0, ly, ly + 1)
    inside &= ~((ux >= w) | (uy >= h))
    ux, uy = np.minimum(ux, w - 1), np.minimum(uy, h - 1)
    t00, t01 = img[ly, lx].astype(np.float64), img[ly, ux].astype(np.float64)
    t10, t11 = img[uy, lx].astype(np.float64), img[uy, ux].astype(np.float64)
    v = t00 * (1 - dx) * (1 - dy) + t01 * dx * (1 - dy) + t10 * (1 - dx) * dy + t11 * dx * dy
    return np.where(inside, v, 128.0)


def get_pix_vals(img, win_x, win_y):
    """sc::getPixVals, imgUtils.h:319-334: row-major, y outer, x inner"""
    X, Y = np.meshgrid(win_x, win_y)
    return pix_vals(img, X.ravel(), Y.ravel())


def get_pix_vals_with_grad(img, win_x, win_y, grad_eps, grad_mult_factor):
    """sc::getPixValsWithGrad, imgUtils.h:337-366"""
    X, Y = np.meshgrid(win_x, win_y)
    x, y = X.ravel(), Y.ravel()
    val = pix_vals(img, x, y)
    grad = np.empty((len(x), 2))
    grad[:, 0] = (pix_vals(img, x + grad_eps, y) - pix_vals(img, x - grad_eps, y)) * grad_mult_factor
    grad[:, 1] = (pix_vals(img, x, y + grad_eps) - pix_vals(img, x, y - grad_eps)) * grad_mult_factor
    return val, grad


def ssum(v):
    """serial left-to-right sum in double"""
    v = np.asarray(v, dtype=np.float64)
    return float(np.cumsum(v)[-1]) if len(v) else 0.0


def colpiv_qr_solve2(A, b):
    """x = A^-1 b for a 2 x 2 A: the column-pivoted Householder QR of mtfo_colpiv_qr_solve, n = 2"""
    if not (np.all(np.isfinite(A)) and np.all(np.isfinite(b))):
        return np.array([np.nan, np.nan])
    a00, a10, a01, a11 = float(A[0, 0]), float(A[1, 0]), float(A[0, 1]), float(A[1, 1])
    cn0, cn1 = a00 * a00 + a10 * a10, a01 * a01 + a11 * a11
    max_norm0 = max(0.0, cn0, cn1)
    best, swapped = -1.0, False
    if cn0 > best:
        best = cn0
    if cn1 > best:
        best, swapped = cn1, True
    if best <= max_norm0 * 1e-300 or best == 0:
        return np.zeros(2)
    p0, p1, q0, q1 = (a01, a11, a00, a10) if swapped else (a00, a10, a01, a11)
    r0, r1 = float(b[0]), float(b[1])
    norm = math.sqrt(best)
    alpha = -norm if p0 > 0 else norm
    v0, v1 = p0 - alpha, p1
    vnorm2 = v0 * v0 + v1 * v1
    if vnorm2 > 0:
        f = 2 * (v0 * p0 + v1 * p1) / vnorm2
        p0, p1 = p0 - f * v0, p1 - f * v1
        f = 2 * (v0 * q0 + v1 * q1) / vnorm2
        q0, q1 = q0 - f * v0, q1 - f * v1
        f = 2 * (v0 * r0 + v1 * r1) / vnorm2
        r0, r1 = r0 - f * v0, r1 - f * v1
    best = q1 * q1
    full = not (best <= max_norm0 * 1e-300 or best == 0)
    if full:
        norm = math.sqrt(best)
        alpha = -norm if q1 > 0 else norm
        v1 = q1 - alpha
        vnorm2 = v1 * v1
        if vnorm2 > 0:
            f = 2 * (v1 * q1) / vnorm2
            q1 = q1 - f * v1
            f = 2 * (v1 * r1) / vnorm2
            r1 = r1 - f * v1
    y1 = r1 / q1 if full else 0.0
    y0 = ((r0 - q0 * y1) if full else r0) / p0
    return np.array([y1, y0]) if swapped else np.array([y0, y1])


def estimate_optical_flow(prev_img, curr_img, prev_pts, win=(10, 10), max_iters=30, term_eps=0.01, const_grad=False, grad_eps=1e-8):
    """NCC::estimateOpticalFlow.  Returns curr_pts (n, 2) float32, n_iters (n,), status (n,), and per point the list of per-pass records
    dict(opt_flow, f, df_dx, H, sq_norm)."""
    prev_img, curr_img = np.asarray(prev_img), np.asarray(curr_img)
    prev_pts = np.asarray(prev_pts, dtype=np.float32).reshape(-1, 2)
    win_w, win_h = (win, win) if isinstance(win, int) else win
    srch_size = win_w * win_h
    half_width, half_height = win_w / 2.0, win_h / 2.0
    grad_mult_factor = 1.0 / (2 * grad_eps)
    n_pts = len(prev_pts)
    curr_pts = np.zeros((n_pts, 2), dtype=np.float32)
    n_iters, status, logs = np.zeros(n_pts, dtype=np.int32), np.zeros(n_pts, dtype=np.int32), []
    err = dict(invalid="ignore", divide="ignore", over="ignore")
    for pt_id in range(n_pts):
        log = []
        logs.append(log)
        px, py = float(prev_pts[pt_id, 0]), float(prev_pts[pt_id, 1])
        if not (math.isfinite(px) and math.isfinite(py)):
            curr_pts[pt_id] = np.nan
            continue
        win_x = lin_spaced(win_w, px - half_width, px + half_width)
        win_y = lin_spaced(win_h, py - half_height, py + half_height)
        with np.errstate(**err):
            if const_grad:
                I0, dIt_dx = get_pix_vals_with_grad(prev_img, win_x, win_y, grad_eps, grad_mult_factor)
                dIt_dx_mean = np.array([ssum(dIt_dx[:, 0]) / srch_size, ssum(dIt_dx[:, 1]) / srch_size])
            else:
                I0 = get_pix_vals(prev_img, win_x, win_y)
            I0_mean = ssum(I0) / srch_size
            I0_cntr = I0 - I0_mean
            c = math.sqrt(ssum(I0_cntr * I0_cntr))
            I0_cntr_c = I0_cntr / c
            cur = prev_pts[pt_id].copy()       # float32
            st, n_it = MAX_ITERS, max_iters
            for iter_id in range(max_iters):
                if const_grad:
                    It = get_pix_vals(curr_img, win_x, win_y)
                else:
                    It, dIt_dx = get_pix_vals_with_grad(curr_img, win_x, win_y, grad_eps, grad_mult_factor)
                    dIt_dx_mean = np.array([ssum(dIt_dx[:, 0]) / srch_size, ssum(dIt_dx[:, 1]) / srch_size])
                It_mean = ssum(It) / srch_size
                It_cntr = It - It_mean
                a = ssum(I0_cntr * It_cntr)
                b = ssum(It_cntr * It_cntr)
                b = math.sqrt(b) if b >= 0 else float("nan")
                f = a / (b * c) if (b * c) != 0 else (float("nan") if a == 0 or a != a else math.copysign(float("inf"), a))
                It_cntr_b = It_cntr / b
                df_dIt_ncntr = (I0_cntr_c - f * It_cntr_b) / b
                df_dIt_ncntr_mean = ssum(df_dIt_ncntr) / srch_size
                wgt = df_dIt_ncntr - df_dIt_ncntr_mean
                df_dx = np.array([ssum(wgt * dIt_dx[:, 0]), ssum(wgt * dIt_dx[:, 1])])
                gcx, gcy = (dIt_dx[:, 0] - dIt_dx_mean[0]) / b, (dIt_dx[:, 1] - dIt_dx_mean[1]) / b
                sxx, sxy, syy = ssum(gcx * gcx), ssum(gcx * gcy), ssum(gcy * gcy)
                v0, v1 = ssum(gcx * It_cntr_b), ssum(gcy * It_cntr_b)
                H = np.array([[-sxx + v0 * v0, -sxy + v0 * v1], [-sxy + v0 * v1, -syy + v1 * v1]])
                opt_flow = -colpiv_qr_solve2(H, df_dx)
                sq = float(opt_flow[0] * opt_flow[0] + opt_flow[1] * opt_flow[1])
                log.append(dict(opt_flow=opt_flow.copy(), f=f, df_dx=df_dx, H=H, sq_norm=sq))
                if not np.all(np.isfinite(opt_flow)):
                    st, n_it = NONFINITE, iter_id + 1
                    break
                cur[0] = np.float32(cur[0] + np.float32(opt_flow[0]))
                cur[1] = np.float32(cur[1] + np.float32(opt_flow[1]))
                win_x = win_x + opt_flow[0]
                win_y = win_y + opt_flow[1]
                if sq < term_eps:
                    st, n_it = CONVERGED, iter_id + 1
                    break
        curr_pts[pt_id] = np.nan if st == NONFINITE else cur
        n_iters[pt_id], status[pt_id] = n_it, st
    return curr_pts, n_iters, status, logs


def warp_matrix(ssm_affine, p):
    """getWarpFromState: Homography.cc:94-107, Affine.cc:116-130"""
    p = np.asarray(p, dtype=np.float64)
    if ssm_affine:
        return np.array([[1 + p[2], p[3], p[0]], [p[4], 1 + p[5], p[1]], [0, 0, 1.0]])
    return np.array([[1 + p[0], p[1], p[2]], [p[3], 1 + p[4], p[5]], [p[6], p[7], 1.0]])


class GridTrackerFlowRef:
    """nt::GridTrackerFlow with `estimator(prev_pts, curr_pts) -> state update` standing in for ssm.estimateWarpFromPts and
    `grid_pts(region) -> (n, 2)` for ssm.getPts() of the grid SSM"""

    def __init__(self, grid_pts, estimator, ssm_affine, win=(10, 10), max_iters=30, epsilon=0.01, use_const_grad=False):
        self.grid_pts, self.estimator, self.ssm_affine = grid_pts, estimator, ssm_affine
        self.win, self.max_iters, self.epsilon, self.use_const_grad = win, max_iters, epsilon, use_const_grad
        self.curr_img = self.prev_img = None

    def set_image(self, img):
        self.curr_img = np.asarray(img)

    def initialize(self, corners):          # :74-86
        self.set_region(corners)
        self.prev_img = self.curr_img.copy()

    def set_region(self, corners):          # :119-126
        self.region = np.asarray(corners, dtype=np.float64).reshape(2, 4).copy()
        self.prev_pts = np.asarray(self.grid_pts(self.region), dtype=np.float64).astype(np.float32)

    def update(self):                       # :88-105
        self.curr_pts, self.n_iters, self.status, self.logs = estimate_optical_flow(
            self.prev_img, self.curr_img, self.prev_pts, self.win, self.max_iters, self.epsilon, self.use_const_grad)
        self.ssm_update = np.asarray(self.estimator(self.prev_pts.astype(np.float64), self.curr_pts.astype(np.float64)), dtype=np.float64)
        W = warp_matrix(self.ssm_affine, self.ssm_update)
        hm = W @ np.vstack([self.region, np.ones(4)])
        self.region = hm[:2] / hm[2]
        self.prev_pts = self.curr_pts.copy()
        self.prev_img = self.curr_img.copy()
        return self.region.copy()
