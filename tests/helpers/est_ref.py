"""NumPy float64 restatement of the reference's grid-SSM estimator, written from its source:
SSM/src/SSMEstimator.cc (runRANSAC :73-139, cvRANSACUpdateNumIters :50-71, runLMeDS :143-216, checkSubset :262-296, LevMarq::updateAlt /
step :427-516), HomographyEstimator.cc (runKernel :16-81, computeReprojError :84-98, refine :100-144, estimateHomography :166-228),
AffineEstimator.cc (:17-46, :49-62, :64-105, :127-190), Homography.cc:885-897 and Affine.cc:359-369.

It does not sample: the hypothesis sequence is an input (`subsets`, one row of point indices per hypothesis; a row holding -1 is a
hypothesis whose getSubset found nothing).  solver selects the linear algebra of runKernel -- "eigh": numpy.linalg.eigh of LtL as the
reference (cvEigenVV) / lstsq for the affine system; "alt": an SVD of L itself / normal equations -- so that the distance between two
legitimate solvers can be measured.
"""
import math

import numpy as np

RANSAC, LMEDS, LEAST_SQUARES = 0, 1, 2
HOMOGRAPHY, AFFINE = 0, 1
DBL_EPSILON = np.finfo(np.float64).eps
FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_MAX = np.finfo(np.float64).max
DBL_MIN = np.finfo(np.float64).tiny


class Params:
    """SSMEstimatorParams with the class defaults (SSMEstimatorParams.cc:5-13)"""

    def __init__(self, method=RANSAC, ransac_reproj_thresh=10.0, n_model_pts=4, refine=True, max_iters=2000, max_subset_attempts=300,
                 confidence=0.995, lm_max_iters=10):
        self.method, self.n_model_pts, self.refine, self.max_iters = method, n_model_pts, bool(refine), max_iters
        self.ransac_reproj_thresh = 3.0 if ransac_reproj_thresh <= 0 else float(ransac_reproj_thresh)   # :54-56
        self.max_subset_attempts, self.confidence, self.lm_max_iters = max_subset_attempts, confidence, lm_max_iters


def cv_round(v):
    return int(round(v))    # Python rounds half to even, as cvRound does


def ransac_update_num_iters(p, ep, model_points, max_iters):   # SSMEstimator.cc:50-71
    p = min(max(p, 0.), 1.)
    ep = min(max(ep, 0.), 1.)
    num = max(1. - p, DBL_MIN)
    denom = 1. - math.pow(1. - ep, model_points)
    if denom < DBL_MIN:
        return 0
    num, denom = math.log(num), math.log(denom)
    return max_iters if (denom >= 0 or -num >= max_iters * (-denom)) else cv_round(num / denom)


def lmeds_num_iters(confidence, model_points, max_iters):     # :145, 172-173
    n = cv_round(math.log(1 - confidence) / math.log(1 - math.pow(1 - 0.45, model_points)))
    return min(max(n, 3), max_iters)


def check_subset(pts):   # :262-296 with checkPartialSubsets == false: i0 = 0, i1 = count - 1
    count = len(pts)
    if count <= 2:
        return True
    for i in range(count):
        for j in range(i):
            dx1, dy1 = pts[j][0] - pts[i][0], pts[j][1] - pts[i][1]
            for k in range(j):
                dx2, dy2 = pts[k][0] - pts[i][0], pts[k][1] - pts[i][1]
                if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                    return False
    return True


def run_kernel(ssm, M, m, solver="eigh"):
    """runKernel: M the input ("object") points, m the output ("image") points, (n, 2) float64.  Returns the 3 x 3 matrix or None."""
    count = len(M)
    if ssm == AFFINE:   # AffineEstimator.cc:17-46 -> utils::computeAffineDLT warpUtils.cc:344-377
        A = np.zeros((2 * count, 6))
        A[0::2, 0:2], A[0::2, 2] = M, 1
        A[1::2, 3:5], A[1::2, 5] = M, 1
        b = m.reshape(-1)
        x = np.linalg.lstsq(A, b, rcond=None)[0] if solver == "eigh" else np.linalg.solve(A.T @ A, A.T @ b)
        return np.array([[x[0], x[1], x[2]], [x[3], x[4], x[5]], [0, 0, 1.0]])
    cm, cM = m.sum(axis=0) / count, M.sum(axis=0) / count                  # HomographyEstimator.cc:29-39
    sm, sM = np.abs(m - cm).sum(axis=0), np.abs(M - cM).sum(axis=0)        # :41-46
    if min(abs(sm[0]), abs(sm[1]), abs(sM[0]), abs(sM[1])) < DBL_EPSILON:  # :48-50
        return None
    sm, sM = count / sm, count / sM
    inv_hnorm = np.array([[1. / sm[0], 0, cm[0]], [0, 1. / sm[1], cm[1]], [0, 0, 1]])
    hnorm2 = np.array([[sM[0], 0, -cM[0] * sM[0]], [0, sM[1], -cM[1] * sM[1]], [0, 0, 1]])
    xy, XY = (m - cm) * sm, (M - cM) * sM
    L = np.zeros((2 * count, 9))
    L[0::2, 0:2], L[0::2, 2] = XY, 1
    L[0::2, 6:8], L[0::2, 8] = -xy[:, :1] * XY, -xy[:, 0]
    L[1::2, 3:5], L[1::2, 5] = XY, 1
    L[1::2, 6:8], L[1::2, 8] = -xy[:, 1:] * XY, -xy[:, 1]
    if solver == "eigh":
        w, v = np.linalg.eigh(L.T @ L)      # ascending: the smallest eigenvalue's vector is column 0 (cvEigenVV descending: V[8])
        h0 = v[:, 0].reshape(3, 3)
    else:
        Lp = L if len(L) >= 9 else np.vstack([L, np.zeros((9 - len(L), 9))])
        h0 = np.linalg.svd(Lp)[2][-1].reshape(3, 3)
    H = inv_hnorm @ h0 @ hnorm2
    return H / H[2, 2]


def reproj_err(ssm, H, M, m):   # :84-98 / AffineEstimator.cc:49-62: double arithmetic, stored as float
    with np.errstate(all="ignore"):
        if ssm == HOMOGRAPHY:
            ww = 1. / (H[2, 0] * M[:, 0] + H[2, 1] * M[:, 1] + 1.)
            dx = (H[0, 0] * M[:, 0] + H[0, 1] * M[:, 1] + H[0, 2]) * ww - m[:, 0]
            dy = (H[1, 0] * M[:, 0] + H[1, 1] * M[:, 1] + H[1, 2]) * ww - m[:, 1]
        else:
            dx = (H[0, 0] * M[:, 0] + H[0, 1] * M[:, 1] + H[0, 2]) - m[:, 0]
            dy = (H[1, 0] * M[:, 0] + H[1, 1] * M[:, 1] + H[1, 2]) - m[:, 1]
        return (dx * dx + dy * dy).astype(np.float32)


def median_of(err):   # SSMEstimator.cc:193-196
    s = np.sort(err)
    count = len(s)
    if count % 2:
        return float(s[count // 2])
    return float(np.float32(s[count // 2 - 1] + s[count // 2])) * 0.5


def sq_error(ssm, H, M, m):
    """the refinement's errNorm at H (double, unrounded)"""
    return lm_terms(ssm, H.reshape(-1)[:8 if ssm == HOMOGRAPHY else 6], M, m, False)[2]


def lm_terms(ssm, h, M, m, with_j=True):   # HomographyEstimator.cc:117-139, AffineEstimator.cc:81-100
    Mx, My = M[:, 0], M[:, 1]
    n = len(M)
    if ssm == HOMOGRAPHY:
        ww = h[6] * Mx + h[7] * My + 1.
        ww = np.where(np.abs(ww) > DBL_EPSILON, 1. / np.where(ww == 0, 1, ww), 0.)
        xi, yi = (h[0] * Mx + h[1] * My + h[2]) * ww, (h[3] * Mx + h[4] * My + h[5]) * ww
        z = np.zeros(n)
        J0 = np.stack([Mx * ww, My * ww, ww, z, z, z, -Mx * ww * xi, -My * ww * xi], axis=1)
        J1 = np.stack([z, z, z, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi], axis=1)
    else:
        xi, yi = h[0] * Mx + h[1] * My + h[2], h[3] * Mx + h[4] * My + h[5]
        z, o = np.zeros(n), np.ones(n)
        J0 = np.stack([Mx, My, o, z, z, z], axis=1)
        J1 = np.stack([z, z, z, Mx, My, o], axis=1)
    e0, e1 = xi - m[:, 0], yi - m[:, 1]
    err_norm = float((e0 * e0 + e1 * e1).sum())
    if not with_j:
        return None, None, err_norm
    return J0.T @ J0 + J1.T @ J1, J0.T @ e0 + J1.T @ e1, err_norm


def refine(ssm, H, M, m, max_iters):
    """refine(): LevMarq(nparams, 0, ITER + EPS (max_iters, DBL_EPSILON)) driven through updateAlt"""
    npar = 8 if ssm == HOMOGRAPHY else 6
    max_iter = min(max(max_iters, 1), 1000)        # SSMEstimator.cc:348-349
    param = H.reshape(-1)[:npar].copy()
    lambda_lg10, iters = -3, 0                     # :346

    def step(JtJ, JtErr, prev):                    # :489-516 (JtJ arrives complete: the mirrored upper triangle)
        lam = math.exp(lambda_lg10 * math.log(10.))
        N = JtJ.copy()
        N[np.diag_indices(npar)] *= 1. + lam
        return prev - np.linalg.lstsq(N, JtErr, rcond=None)[0]

    JtJ, JtErr, err_norm = lm_terms(ssm, param, M, m)      # STARTED -> CALC_J
    while True:
        prev = param.copy()                                # CALC_J :448-457
        param = step(JtJ, JtErr, prev)
        prev_err_norm = err_norm
        err_norm = lm_terms(ssm, param, M, m, False)[2]
        while err_norm > prev_err_norm:                    # CHECK_ERR :459-469
            lambda_lg10 += 1
            if lambda_lg10 > 16:
                break
            param = step(JtJ, JtErr, prev)
            err_norm = lm_terms(ssm, param, M, m, False)[2]
        lambda_lg10 = max(lambda_lg10 - 1, -16)            # :471
        iters += 1
        if iters >= max_iter or np.linalg.norm(param - prev) / (np.linalg.norm(prev) + DBL_EPSILON) < DBL_EPSILON:
            break
        JtJ, JtErr, _ = lm_terms(ssm, param, M, m)        # :479-486 (errNorm is kept)
    out = H.copy().reshape(-1)
    out[:npar] = param
    return out.reshape(3, 3)


def state_from_mat(ssm, H):   # Homography.cc:889-896, Affine.cc:363-368
    if ssm == HOMOGRAPHY:
        return np.array([H[0, 0] - 1, H[0, 1], H[0, 2], H[1, 0], H[1, 1] - 1, H[1, 2], H[2, 0], H[2, 1]])
    return np.array([H[0, 2], H[1, 2], H[0, 0] - 1, H[0, 1], H[1, 0], H[1, 1] - 1])


def estimate(ssm, in_pts, out_pts, p, subsets=None, solver="eigh"):
    """estimateHomography / estimateAffine + estimateWarpFromPts.  Returns a dict with everything the device returns and, under
    "margins", how close the run came to a tie: the smallest relative distance of a squared error to the squared threshold over every
    hypothesis the rule walked and the final mask pass, and the smallest relative gap between a walked median and the running minimum."""
    M = np.asarray(in_pts, dtype=np.float32).astype(np.float64).reshape(-1, 2)     # cvConvertPointsHomogeneous :179-183
    m = np.asarray(out_pts, dtype=np.float32).astype(np.float64).reshape(-1, 2)
    n, mp = len(M), p.n_model_pts
    if n < mp:
        raise ValueError("n_pts < n_model_pts")
    mask = np.ones(n, dtype=np.uint8)
    method = LEAST_SQUARES if n == mp else p.method          # :196
    H, result, winner, walked, min_median, sigma = None, False, -1, 0, DBL_MAX, 0.0
    thr_margin, med_margin = np.inf, np.inf

    def margin(err, thr2):
        with np.errstate(all="ignore"):
            d = np.abs(err.astype(np.float64) - thr2) / thr2
        return float(np.nanmin(d)) if len(d) else np.inf

    if method == LEAST_SQUARES:
        H = run_kernel(ssm, M, m, solver)
        result = H is not None
    else:
        subsets = np.asarray(subsets, dtype=np.int64).reshape(-1, mp)
        niters = p.max_iters if method == RANSAC else lmeds_num_iters(p.confidence, mp, p.max_iters)
        niters = min(niters, len(subsets))
        max_good, failed, it = 0, False, 0
        thr2 = p.ransac_reproj_thresh ** 2
        while it < niters:                                    # :101 / :175
            row = subsets[it]
            if (row < 0).any():                               # getSubset found nothing :104-109
                failed = it == 0
                break
            Hk = run_kernel(ssm, M[row], m[row], solver)
            if Hk is None:
                it += 1
                continue
            err = reproj_err(ssm, Hk, M, m)
            if method == RANSAC:
                thr_margin = min(thr_margin, margin(err, thr2))
                good = int((err <= thr2).sum())               # findInliers :43-45
                if good > max(max_good, mp - 1):              # :120-126
                    H, max_good, winner = Hk, good, it
                    mask = (err <= thr2).astype(np.uint8)
                    niters = ransac_update_num_iters(p.confidence, (n - good) / n, mp, niters)
            else:
                med = median_of(err)
                if np.isfinite(med) and min_median < DBL_MAX:
                    med_margin = min(med_margin, abs(med - min_median) / min_median if min_median > 0 else np.inf)
                if med < min_median:                          # :198-201
                    min_median, H, winner = med, Hk, it
            it += 1
        walked = it
        if method == RANSAC:
            result = (not failed) and max_good > 0            # :132-136
            if not result:
                mask[:] = 1
        elif (not failed) and min_median < DBL_MAX:           # :207-213
            sigma = max(2.5 * 1.4826 * (1 + 5. / (n - mp)) * math.sqrt(min_median), 0.001)
            err = reproj_err(ssm, H, M, m)
            thr_margin = min(thr_margin, margin(err, sigma * sigma))
            mask = (err <= sigma * sigma).astype(np.uint8)
            result = int(mask.sum()) >= mp
    if result and n > mp:                                     # HomographyEstimator.cc:206-215
        keep = mask.astype(bool)
        Mi, mi = M[keep], m[keep]
        if method == RANSAC:
            H2 = run_kernel(ssm, Mi, mi, solver)
            if H2 is not None:
                H = H2
        if p.refine:
            H = refine(ssm, H, Mi, mi, p.lm_max_iters)
    if not result:
        H = np.zeros((3, 3))                                  # :161-162
    return dict(state_update=state_from_mat(ssm, H), mask=mask, ok=bool(result), winner=winner, n_walked=walked, n_inliers=int(mask.sum()),
                min_median=min_median if min_median < DBL_MAX else 0.0, sigma=sigma, H=H,
                margins=dict(threshold=thr_margin, median=med_margin))
