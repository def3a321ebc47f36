"""nt::FALK::initialize / update (SM/src/NT/FALK.cc:93-257) and nt::IALK::initialize / update (SM/src/NT/IALK.cc:55-199) restated over the
oracle's appearance model and state space model (oracle_py.AM / oracle_py.SSM), call for call in the reference's order: the three Hessian
types, Levenberg-Marquardt with its undo through additiveUpdate(-ssm_update), the corner-change convergence test.  The solve is the
oracle's colPivHouseholderQr.  Every executed pass is logged, a rejected one included."""
import numpy as np

FALK, IALK = 3, 4                      # MTFHIP_SM_FALK / MTFHIP_SM_IALK
INITIAL_SELF, CURRENT_SELF, STD = 0, 1, 2   # FALKParams.h:9, IALKParams.h:9

# SM/src/FALKParams.cc:3-15, IALKParams.cc:4-11
DEFAULTS = dict(max_iters=10, epsilon=0.01, hess_type=INITIAL_SELF, leven_marq=0, lm_delta_init=0.01, lm_delta_update=10.0)


class AlkRef:
    def __init__(self, method, o_am, o_ssm, **params):
        assert method in (FALK, IALK)
        self.method, self.am, self.ssm = method, o_am, o_ssm
        self.p = dict(DEFAULTS)
        self.p.update(params)
        self.H0 = None
        self.J0 = None

    def initialize(self, corners):
        """FALK.cc:96-122 / IALK.cc:58-82 (first-order Hessians)"""
        am, ssm = self.am, self.ssm
        ssm.set_corners(corners)
        pts = ssm.get("curr_pts")
        am.initialize_pix_vals(pts)
        am.initialize_pix_grad_pts(pts)
        am.initialize_similarity()
        am.initialize_grad()
        am.initialize_hess()
        if self.p["hess_type"] == INITIAL_SELF:
            self.J0 = ssm.cmpt_pix_jacobian(am.get("dI0_dx"))
            self.H0 = am.cmpt_self_hessian(self.J0)

    def update(self):
        """FALK.cc:132-257 / IALK.cc:90-199 -> dict(n_iters, corners (8,) x, y per corner, state, log); log: one dict per executed pass
        with f, undo, lm_delta and -- unless the pass was a rejected step -- g, H (before damping), dp, and state / corners after the pass"""
        import oracle_py
        am, ssm, p = self.am, self.ssm, self.p
        prev_f, lm_delta, state_reset = 0.0, p["lm_delta_init"], False
        ssm_update = np.zeros(ssm.S)
        log = []
        for iter_id in range(p["max_iters"]):
            am.update_pix_vals(ssm.get("curr_pts"))
            am.update_similarity(False)
            f = am.similarity
            if p["leven_marq"] and not state_reset:
                if iter_id > 0:
                    if f < prev_f:
                        lm_delta *= p["lm_delta_update"]
                        ssm.additive_update(-ssm_update)   # undo the last update
                        state_reset = True
                        log.append(dict(f=f, undo=True, lm_delta=lm_delta, dp=ssm_update.copy(), state=ssm.get("state").copy(),
                                        corners=ssm.get("curr_corners").copy()))
                        continue
                    if f > prev_f:
                        lm_delta /= p["lm_delta_update"]
                prev_f = f
            state_reset = False
            if self.method == FALK:
                am.update_pix_grad_pts(ssm.get("curr_pts"))
                Jt = ssm.cmpt_pix_jacobian(am.get("dIt_dx"))
            else:
                Jt = ssm.cmpt_approx_pix_jacobian(am.get("dI0_dx"))
            am.update_curr_grad()
            g = am.cmpt_curr_jacobian(Jt)
            if p["hess_type"] == INITIAL_SELF:
                H = self.H0
            elif p["hess_type"] == CURRENT_SELF:
                H = am.cmpt_self_hessian(Jt)
            else:
                H = am.cmpt_curr_hessian(Jt)
            Hs = np.array(H, dtype=np.float64)
            if p["leven_marq"]:
                Hs[np.diag_indices(ssm.S)] += lm_delta * np.diag(Hs)
            ssm_update = -oracle_py.colpiv_qr_solve(Hs, g)
            prev_corners = ssm.get("curr_corners").copy()
            ssm.additive_update(ssm_update)
            corners = ssm.get("curr_corners").copy()
            update_norm = float(((prev_corners - corners) ** 2).sum())
            log.append(dict(f=f, undo=False, lm_delta=lm_delta, g=g.copy(), H=np.array(H), dp=ssm_update.copy(), state=ssm.get("state").copy(),
                            corners=corners, update_norm=update_norm, It=am.get("It").copy(), Jt=Jt.copy(),
                            dIt_dx=am.get("dIt_dx").copy() if self.method == FALK else None))
            if update_norm < p["epsilon"]:
                break
        return dict(n_iters=len(log), corners=ssm.get("curr_corners").copy(), state=ssm.get("state").copy(), log=log)


def track(oracle, method, am_kind, ssm_kind, resx, resy, frame0, frame1, corners, **params):
    """a fresh pair of oracle objects initialised on frame0 at `corners` and updated once on frame1 -> (AlkRef, result of update())"""
    o_ssm = oracle.SSM(ssm_kind, resx, resy)
    o_am = oracle.AM(am_kind, resx, resy)
    o_am.set_curr_img(frame0)
    ref = AlkRef(method, o_am, o_ssm, **params)
    ref.initialize(corners)
    o_am.set_curr_img(frame1)
    return ref, ref.update()


def corner_error(corners8, truth_2x4):
    """mean corner distance (pixels) between an (8,) x, y per corner vector and 2 x 4 ground-truth corners"""
    c = np.asarray(corners8).reshape(4, 2).T
    return float(np.sqrt(((c - truth_2x4) ** 2).sum(axis=0)).mean())


def warped_corners(corners_2x4, p_true, centre):
    """where synth.warp_frame(frame, p_true, centre) moves the corners of a region"""
    W = np.array([[1 + p_true[0], p_true[1], p_true[2]], [p_true[3], 1 + p_true[4], p_true[5]], [p_true[6], p_true[7], 1.0]])
    q = W @ np.vstack([corners_2x4 - np.array(centre)[:, None], np.ones(4)])
    return q[:2] / q[2] + np.array(centre)[:, None]
