"""The three low-order state space models -- Similitude, Isometry, Translation (SSM/src/Similitude.cc, Isometry.cc, Translation.cc, with
normalized_init = 0) -- restated in NumPy float64 from their formulas, and nt::ESM / nt::FCLK / nt::ICLK::initialize / update
(SM/src/NT/{ESM,FCLK,ICLK}.cc) restated over an appearance-model object and a state-space-model object, call for call in the reference's
order.  `SSM` has the method names and the array layouts of oracle_py.SSM, so either can stand behind `LKRef`; the appearance model is
oracle_py.AM, whose Jacobian and Hessian calls take any state size.

Layouts (oracle_py's): points (2 N,) x, y interleaved; corners (8,) x, y per corner TL TR BR BL; a pixel gradient (2 N,) N x then N y; a
pixel Jacobian (N S,) S columns of N; warps (9,) row-major; set_corners / apply_warp_to_pts take 2 x n arrays."""
import numpy as np

SIM, ISO, TRANS = 2, 3, 4              # MTFHIP_SSM_SIMILITUDE / _ISOMETRY / _TRANSLATION
AFFINE = 1
STATE_SIZE = {SIM: 4, ISO: 3, TRANS: 2}
NAMES = {SIM: "similitude", ISO: "isometry", TRANS: "translation"}
ESM, FCLK, ICLK = 0, 1, 2              # MTFHIP_SM_*

# J_S = J_aff M: the constant 6 x S matrices (affine columns [Ix, Iy, Ix x, Ix y, Iy x, Iy y])
M = {
    TRANS: np.array([[1, 0], [0, 1], [0, 0], [0, 0], [0, 0], [0, 0]], dtype=np.float64),
    ISO: np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, -1], [0, 0, 1], [0, 0, 0]], dtype=np.float64),
    SIM: np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, -1], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=np.float64),
}


def lin_spaced(n, lo, hi):
    """Eigen's LinSpaced as utils::getNormUnitSquarePts uses it (warpUtils.cc:15-34): lo + i step, the last element hi"""
    v = lo + np.arange(n) * ((hi - lo) / (n - 1))
    v[-1] = hi
    return v


def homography_dlt(src_2x4, dst_2x4):
    """the homography through four point pairs, (2, 2) = 1: what computeHomographyDLT's SVD returns for four pairs (warpUtils.cc:171-224)"""
    A, b = np.zeros((8, 8)), np.zeros(8)
    for q in range(4):
        x, y = src_2x4[:, q]
        u, v = dst_2x4[:, q]
        A[2 * q] = [x, y, 1, 0, 0, 0, -u * x, -u * y]
        A[2 * q + 1] = [0, 0, 0, x, y, 1, -v * x, -v * y]
        b[2 * q], b[2 * q + 1] = u, v
    h = np.linalg.solve(A, b)
    return np.append(h, 1.0).reshape(3, 3)


def similitude_dlt(in_2x4, out_2x4):
    """utils::computeSimilitudeDLT (warpUtils.cc:494-535): least-squares [tx, ty, a, b] of out - in = [1 0 x -y; 0 1 y x] p"""
    A, d = np.zeros((8, 4)), np.zeros(8)
    for q in range(4):
        x, y = in_2x4[:, q]
        A[2 * q] = [1, 0, x, -y]
        A[2 * q + 1] = [0, 1, y, x]
        d[2 * q], d[2 * q + 1] = out_2x4[0, q] - x, out_2x4[1, q] - y
    p = np.linalg.lstsq(A, d, rcond=None)[0]
    return np.array([[1 + p[2], -p[3], p[0]], [p[3], 1 + p[2], p[1]], [0, 0, 1.0]])


class SSM:
    def __init__(self, kind, resx, resy):
        assert kind in STATE_SIZE
        self.kind, self.resx, self.resy = kind, resx, resy
        self.n, self.S = resx * resy, STATE_SIZE[kind]
        # Similitude.cc:66-67: the pixel-sized square; Isometry and Translation keep ProjectiveBase's unit square (ProjectiveBase.cc:15)
        if kind == SIM:
            lo_x, lo_y, hi_x, hi_y = 1 - resx / 2.0, 1 - resy / 2.0, resx / 2.0, resy / 2.0
        else:
            lo_x, lo_y, hi_x, hi_y = -0.5, -0.5, 0.5, 0.5
        xs, ys = lin_spaced(resx, lo_x, hi_x), lin_spaced(resy, lo_y, hi_y)
        self.norm_pts = np.stack([np.tile(xs, resy), np.repeat(ys, resx)])           # point id = row resx + col
        self.norm_corners = np.array([[lo_x, hi_x, hi_x, lo_x], [lo_y, lo_y, hi_y, hi_y]])
        self.warp = np.eye(3)
        self.state = np.zeros(self.S)
        self.init_pts = self.curr_pts = self.norm_pts.copy()
        self.init_corners = self.curr_corners = self.norm_corners.copy()
        self.grad_pts = None

    # ---- getWarpFromState / getStateFromWarp: Similitude.cc:123-153, Isometry.cc:68-97, Translation.cc:86-101
    def warp_from_state(self, p):
        p = np.asarray(p, dtype=np.float64)
        if self.kind == TRANS:
            return np.array([[1, 0, p[0]], [0, 1, p[1]], [0, 0, 1.0]])
        if self.kind == SIM:
            return np.array([[1 + p[2], -p[3], p[0]], [p[3], 1 + p[2], p[1]], [0, 0, 1.0]])
        c, s = np.cos(p[2]), np.sin(p[2])
        return np.array([[c, -s, p[0]], [s, c, p[1]], [0, 0, 1.0]])

    def state_from_warp(self, W):
        if self.kind == TRANS:
            return np.array([W[0, 2], W[1, 2]])
        if self.kind == SIM:
            return np.array([W[0, 2], W[1, 2], W[0, 0] - 1, W[1, 0]])
        return np.array([W[0, 2], W[1, 2], np.arctan2(W[1, 0], W[0, 0])])

    def affine_state(self):
        """the affine state [tx, ty, a - 1, b, c, d - 1] (Affine.cc:132-143) of the current warp"""
        W = self.warp
        return np.array([W[0, 2], W[1, 2], W[0, 0] - 1, W[0, 1], W[1, 0], W[1, 1] - 1])

    def get(self, what):
        if what in ("curr_pts", "init_pts"):
            return np.ascontiguousarray(getattr(self, what).T.ravel())
        if what in ("curr_corners", "init_corners"):
            return np.ascontiguousarray(getattr(self, what).T.ravel())
        if what == "state":
            return self.state.copy()
        if what == "curr_warp":
            return self.warp.ravel().copy()
        if what == "grad_pts":
            return self.grad_pts.copy()
        raise KeyError(what)

    # ---- setCorners with normalized_init = 0: ProjectiveBase.cc:20-39, Translation.cc:55-64, Similitude.cc:87-100
    def set_corners(self, corners):
        c = np.asarray(corners, dtype=np.float64).reshape(2, 4)
        H = homography_dlt(self.norm_corners, c)
        ph = H @ np.vstack([self.norm_pts, np.ones(self.n)])
        self.init_pts = ph[:2] / ph[2]
        self.curr_pts = self.init_pts.copy()
        self.init_corners, self.curr_corners = c.copy(), c.copy()
        self.warp, self.state = np.eye(3), np.zeros(self.S)

    def _apply(self):
        """curr_pts = curr_warp.topRows<2>() * init_pts_hm, every product and sum rounded on its own and in Eigen's order (no BLAS: a fused
        multiply-add would move a point by an ulp, which the 1e-8 central difference of the image gradient turns into 1e-5 of a gradient)"""
        W = self.warp

        def go(p):
            return np.stack([W[0, 0] * p[0] + W[0, 1] * p[1] + W[0, 2], W[1, 0] * p[0] + W[1, 1] * p[1] + W[1, 2]])
        self.curr_pts, self.curr_corners = go(self.init_pts), go(self.init_corners)

    def set_warp(self, W):
        """the state and the points of a given warp matrix (tests hand over the device's own matrix, so that both sides sample the image at
        the same bits whatever cos / sin the two maths libraries return)"""
        self.warp = np.asarray(W, dtype=np.float64).reshape(3, 3).copy()
        self.state = self.state_from_warp(self.warp)
        self._apply()

    def set_state(self, p):
        self.state = np.asarray(p, dtype=np.float64).copy()
        self.warp = self.warp_from_state(self.state)
        if self.kind == TRANS:   # Translation.cc:66-73
            self.curr_pts = self.init_pts + self.state[:, None]
            self.curr_corners = self.init_corners + self.state[:, None]
        else:
            self._apply()

    def compositional_update(self, dp):
        dp = np.asarray(dp, dtype=np.float64)
        if self.kind == TRANS:   # Translation.cc:75-84
            self.state = self.state + dp
            self.warp[0, 2], self.warp[1, 2] = self.state
            self.curr_pts = self.curr_pts + dp[:, None]
            self.curr_corners = self.curr_corners + dp[:, None]
            return
        self.warp = self.warp @ self.warp_from_state(dp)   # Similitude.cc:111-121, Isometry.cc:56-66
        self.state = self.state_from_warp(self.warp)
        self._apply()

    def invert_state(self, p):
        p = np.asarray(p, dtype=np.float64)
        if self.kind == TRANS:   # Translation.cc:103-105
            return -p
        Wi = np.linalg.inv(self.warp_from_state(p))   # ProjectiveBase.cc:57-62
        return self.state_from_warp(Wi / Wi[2, 2])

    def update_grad_pts(self, eps):
        """Similitude.cc:314-333, Isometry.cc:348-367, Translation.cc:107-122 -> (8 N,) per point x+ y+ | x- y- of the x step, then the y step"""
        dx, dy = self.warp[:2, 0] * eps, self.warp[:2, 1] * eps
        if self.kind == TRANS:
            dx, dy = np.array([eps, 0.0]), np.array([0.0, eps])
        p = self.curr_pts
        g = np.stack([p[0] + dx[0], p[1] + dx[1], p[0] - dx[0], p[1] - dx[1], p[0] + dy[0], p[1] + dy[1], p[0] - dy[0], p[1] - dy[1]], axis=1)
        self.grad_pts = np.ascontiguousarray(g.ravel())

    def apply_warp_to_pts(self, pts, p):
        W = self.warp_from_state(p)
        q = np.asarray(pts, dtype=np.float64)
        return W[:2, :2] @ q + W[:2, 2:3]

    def apply_warp_to_corners(self, corners, p):
        return self.apply_warp_to_pts(np.asarray(corners, dtype=np.float64).reshape(2, 4), p)

    def compose_warps(self, p1, p2):
        return self.state_from_warp(self.warp_from_state(p2) @ self.warp_from_state(p1))   # ProjectiveBase.cc:324-331

    def estimate_warp_from_corners(self, in_corners, out_corners):
        a, b = np.asarray(in_corners, dtype=np.float64).reshape(2, 4), np.asarray(out_corners, dtype=np.float64).reshape(2, 4)
        if self.kind == TRANS:   # Translation.cc:164-171
            return b.mean(axis=1) - a.mean(axis=1)
        W = similitude_dlt(a, b)
        if self.kind == SIM:     # Similitude.cc:295-301
            return self.state_from_warp(W)
        s = np.sqrt(W[0, 0] ** 2 + W[1, 0] ** 2)   # Isometry.cc:296-322
        return np.array([W[0, 2], W[1, 2], np.arctan2(W[1, 0] / s, W[0, 0] / s)])

    # ---- pixel Jacobians: Translation.h:45-63, Isometry.cc:115-135,162-185, Similitude.cc:163-210
    def _rows(self, Ix, Iy):
        x, y = self.init_pts
        cols = [Ix, Iy]
        if self.kind == SIM:
            cols += [Ix * x + Iy * y, Iy * x - Ix * y]
        elif self.kind == ISO:
            cols += [Iy * x - Ix * y]
        return np.ascontiguousarray(np.concatenate(cols))

    def cmpt_init_pix_jacobian(self, grad):
        g = np.asarray(grad, dtype=np.float64).reshape(2, self.n)
        return self._rows(g[0], g[1])

    def cmpt_warped_pix_jacobian(self, grad):
        g = np.asarray(grad, dtype=np.float64).reshape(2, self.n)
        if self.kind == TRANS:
            return self._rows(g[0], g[1])
        if self.kind == SIM:
            a, b, c, d = self.state[2] + 1, -self.state[3], self.state[3], self.state[2] + 1
            return self._rows(a * g[0] + c * g[1], b * g[0] + d * g[1])
        cos_t, sin_t = self.warp[0, 0], self.warp[1, 0]
        return self._rows(cos_t * g[0] + sin_t * g[1], cos_t * g[1] - sin_t * g[0])


# ------------------------------------------------------------------ nt::ESM / FCLK / ICLK
# ESM hess_type: 0 InitialSelf 1 CurrentSelf 2 SumOfSelf 3 Original 4 SumOfStd 5 Std; FCLK / ICLK: 0 InitialSelf 1 CurrentSelf 2 Std
DEFAULTS = dict(max_iters=30, epsilon=1e-4, jac_type=1, hess_type=0, chained_warp=1, leven_marq=0, lm_delta_init=0.01, lm_delta_update=10.0,
                grad_eps=1e-8)


class LKRef:
    def __init__(self, method, o_am, o_ssm, **params):
        assert method in (ESM, FCLK, ICLK)
        self.method, self.am, self.ssm = method, o_am, o_ssm
        self.p = dict(DEFAULTS)
        self.p.update(params)
        self.J0 = self.H0 = None

    def _pix_jacobian(self, init):
        """initializePixJacobian / updatePixJacobian (NT/ESM.cc:376-404), the same two routes in FCLK.cc:115-134,223-235 and ICLK.cc:79-93"""
        am, ssm = self.am, self.ssm
        if self.p["chained_warp"]:
            (am.initialize_pix_grad_pts if init else am.update_pix_grad_pts)(ssm.get("curr_pts"))
            return ssm.cmpt_warped_pix_jacobian(am.get("dI0_dx" if init else "dIt_dx"))
        ssm.update_grad_pts(self.p["grad_eps"])
        (am.initialize_pix_grad_warped if init else am.update_pix_grad_warped)(ssm.get("grad_pts"))
        return ssm.cmpt_init_pix_jacobian(am.get("dI0_dx" if init else "dIt_dx"))

    def initialize(self, corners):
        """NT/ESM.cc:110-148, NT/FCLK.cc:102-169, NT/ICLK.cc:71-129 (first-order Hessians)"""
        am, ssm, p = self.am, self.ssm, self.p
        ssm.set_corners(corners)
        am.initialize_pix_vals(ssm.get("curr_pts"))
        if self.method == FCLK:
            am.initialize_similarity(); am.initialize_grad(); am.initialize_hess()
            self.J0 = self._pix_jacobian(True)
        else:
            self.J0 = self._pix_jacobian(True)
            am.initialize_similarity(); am.initialize_grad(); am.initialize_hess()
        self.H0 = am.cmpt_self_hessian(self.J0)

    def set_region(self, corners):
        """NT/ESM.cc:150-168; FCLK.cc:360-376 and ICLK.cc:131-157 (update_ssm off) reset the SSM alone"""
        self.ssm.set_corners(corners)
        if self.method == ESM:
            self.J0 = self.ssm.cmpt_init_pix_jacobian(self.am.get("dI0_dx"))
            self.H0 = self.am.cmpt_self_hessian(self.J0)

    def _g_H(self, Jt):
        am, p, J0, H0 = self.am, self.p, self.J0, self.H0
        ht = p["hess_type"]
        if self.method == FCLK:     # FCLK.cc:259-288
            g = am.cmpt_curr_jacobian(Jt)
            H = H0 if ht == 0 else (am.cmpt_self_hessian(Jt) if ht == 1 else am.cmpt_curr_hessian(Jt))
            return g, H
        if self.method == ICLK:     # ICLK.cc:200-254
            g = am.cmpt_init_jacobian(J0)
            H = H0 if ht == 0 else (am.cmpt_self_hessian(Jt) if ht == 1 else am.cmpt_init_hessian(J0))
            return g, H
        Jm = (np.asarray(J0) + np.asarray(Jt)) / 2.0 if (p["jac_type"] == 0 or ht == 3) else None   # ESM.cc:238-241
        g = am.cmpt_curr_jacobian(Jm) if p["jac_type"] == 0 else 0.5 * am.cmpt_difference_of_jacobians(J0, Jt)   # ESM.cc:299-314
        if ht == 0:
            H = H0
        elif ht == 1:
            H = am.cmpt_self_hessian(Jt)
        elif ht == 2:
            H = (am.cmpt_self_hessian(Jt) + H0) * 0.5
        elif ht == 3:
            H = am.cmpt_curr_hessian(Jm)
        elif ht == 4:
            H = am.cmpt_sum_of_hessians(J0, Jt) * 0.5
        else:
            H = am.cmpt_curr_hessian(Jt)
        return g, H

    def update(self, max_passes=None):
        """-> dict(n_iters, corners (8,), state, log).  n_iters counts the passes the reference's loop ran (a rejected Levenberg-Marquardt
        step of ESM / ICLK consumes an iteration of their for loops, of FCLK's while loop it does not: iters of the loop variable differ,
        passes do not); log: one dict per pass with f, undo, lm_delta and -- unless the step was rejected -- g, H (before damping), dp,
        It, dIt_dx, Jt (None where the method does not form them) and the state and corners after the pass.  max_passes: stop early."""
        import oracle_py
        am, ssm, p = self.am, self.ssm, self.p
        prev_f, lm_delta, state_reset = 0.0, p["lm_delta_init"], False
        ssm_update = np.zeros(ssm.S)
        log = []
        iter_id = 0
        while iter_id < p["max_iters"]:
            if max_passes is not None and len(log) >= max_passes:
                break
            am.update_pix_vals(ssm.get("curr_pts"))
            am.update_similarity(False)
            f = am.similarity
            if p["leven_marq"] and not state_reset:
                if iter_id > 0:
                    if f < prev_f:
                        lm_delta *= p["lm_delta_update"]
                        # ESM.cc:213-214, FCLK.cc:199-200: the inverse of the last update; ICLK.cc:184: the update itself
                        ssm.compositional_update(ssm_update if self.method == ICLK else ssm.invert_state(ssm_update))
                        state_reset = True
                        log.append(dict(f=f, undo=True, lm_delta=lm_delta, dp=ssm_update.copy(), state=ssm.get("state").copy(),
                                        corners=ssm.get("curr_corners").copy()))
                        if self.method != FCLK:
                            iter_id += 1      # `continue` in a for loop
                        continue
                    if f > prev_f:
                        lm_delta /= p["lm_delta_update"]
                prev_f = f
            state_reset = False
            Jt = None
            if self.method == FCLK:
                am.update_curr_grad()
                Jt = self._pix_jacobian(False)
            elif self.method == ESM:
                Jt = self._pix_jacobian(False)
                am.update_curr_grad()
                am.update_init_grad()
            else:
                am.update_init_grad()
                if p["hess_type"] == 1:
                    Jt = self._pix_jacobian(False)
            g, H = self._g_H(Jt)
            Hs = np.array(H, dtype=np.float64)
            if p["leven_marq"]:
                Hs[np.diag_indices(ssm.S)] += lm_delta * np.diag(Hs)
            ssm_update = -oracle_py.colpiv_qr_solve(Hs, g)
            prev_corners = ssm.get("curr_corners").copy()
            ssm.compositional_update(ssm.invert_state(ssm_update) if self.method == ICLK else ssm_update)
            corners = ssm.get("curr_corners").copy()
            update_norm = float(((prev_corners - corners) ** 2).sum())
            log.append(dict(f=f, undo=False, lm_delta=lm_delta, g=np.array(g), H=np.array(H), dp=ssm_update.copy(), state=ssm.get("state").copy(),
                            corners=corners, update_norm=update_norm, It=am.get("It").copy(),
                            Jt=None if Jt is None else np.array(Jt), dIt_dx=None if Jt is None else am.get("dIt_dx").copy()))
            if update_norm < p["epsilon"]:
                break
            iter_id += 1
        return dict(n_iters=len(log), corners=ssm.get("curr_corners").copy(), state=ssm.get("state").copy(), log=log)


def track(oracle, method, am_kind, ssm_obj, frame0, frame1, corners, **params):
    """a fresh oracle appearance model over `ssm_obj`, initialised on frame0 at `corners` and updated once on frame1 -> (LKRef, result)"""
    o_am = oracle.AM(am_kind, ssm_obj.resx, ssm_obj.resy)
    o_am.set_curr_img(frame0)
    ref = LKRef(method, o_am, ssm_obj, **params)
    ref.initialize(corners)
    o_am.set_curr_img(frame1)
    return ref, ref.update()


def corner_error(corners8, truth_2x4):
    """mean corner distance (pixels) between an (8,) x, y per corner vector and 2 x 4 ground-truth corners"""
    c = np.asarray(corners8).reshape(4, 2).T
    return float(np.sqrt(((c - truth_2x4) ** 2).sum(axis=0)).mean())
