"""CPU: tests/helpers/lowdof_ref.py held to what it restates.  LKRef -- nt::ESM / FCLK / ICLK over an AM and an SSM object -- reproduces the
oracle's own trackers where both exist (the affine SSM); the three low-order SSMs satisfy their defining relations (the inverse undoes the
update, the Jacobian rows are the derivative of the warp, J_S = J_aff M); and on the shared cases the reference converges, which is the
condition the device comparisons of tests/test_gpu_lowdof.py rest on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import alk_cases as AC       # noqa: E402
import lowdof_cases as LC    # noqa: E402
import lowdof_ref as R       # noqa: E402


# ------------------------------------------------------------------ LKRef against the oracle's trackers
@pytest.mark.parametrize("am", [LC.SSD, LC.NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("method", LC.METHODS, ids=LC.METHOD_IDS)
def test_lkref_reproduces_the_oracle_tracker_on_affine(oracle, method, am):
    """Over oracle_py.SSM(AFFINE) and oracle_py.AM at 37 x 23, LKRef runs the float64 expressions of oracle_py.Tracker: the same n_iters, and
    per pass and at the end the same corners to 1e-10 px (measured: 0.0 -- both call the same oracle functions in the same order)"""
    size = (37, 23)
    frame0, frame1 = AC.frame0(), AC.warped(AC.P_AFF)
    params = dict(max_iters=30, epsilon=1e-4, jac_type=1, hess_type=LC.default_hess(method), chained_warp=1, leven_marq=0)
    o_ssm = oracle.SSM(AC.AFF, *size); o_am = oracle.AM(am, *size); o_am.set_curr_img(frame0)
    trk = oracle.Tracker(method, o_am, o_ssm, **params)
    trk.initialize(AC.REGION)
    o_am.set_curr_img(frame1)
    n_it = trk.update()
    trace = trk.trace()
    ref, res = R.track(oracle, method, am, oracle.SSM(AC.AFF, *size), frame0, frame1, AC.REGION, **params)
    gap = float(np.abs(res["corners"].reshape(4, 2).T - trk.get_region()).max())
    print("lkref vs tracker method %d am %d: n_iters %d / %d, corner gap %.3e" % (method, am, res["n_iters"], n_it, gap))
    assert res["n_iters"] == n_it == len(trace)
    assert 2 <= n_it < 30
    assert gap < 1e-10
    for k, (a, r) in enumerate(zip(res["log"], trace)):
        assert np.abs(a["corners"].reshape(4, 2).T - r["corners"]).max() < 1e-10, k
        assert np.abs(a["dp"] - r["dp"]).max() <= 1e-10 * max(1.0, np.abs(r["dp"]).max()), k


# ------------------------------------------------------------------ the three SSMs
STATES = {R.TRANS: np.array([1.7, -2.3]), R.ISO: np.array([1.7, -2.3, 0.04]), R.SIM: np.array([1.7, -2.3, 0.03, -0.02])}
UPDATES = {R.TRANS: np.array([-0.4, 0.6]), R.ISO: np.array([-0.4, 0.6, -0.015]), R.SIM: np.array([-0.4, 0.6, -0.01, 0.012])}


@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_inverse_undoes_the_compositional_update(ssm):
    s = R.SSM(ssm, 9, 7)
    s.set_corners(LC.REGION)
    s.set_state(STATES[ssm])
    pts, corners, state = s.curr_pts.copy(), s.curr_corners.copy(), s.state.copy()
    s.compositional_update(UPDATES[ssm])
    assert np.abs(s.curr_corners - corners).max() > 0.1
    s.compositional_update(s.invert_state(UPDATES[ssm]))
    assert np.abs(s.curr_pts - pts).max() < 1e-11
    assert np.abs(s.curr_corners - corners).max() < 1e-11
    assert np.abs(s.state - state).max() < 1e-12


@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_jacobian_rows_are_the_derivative_of_the_warp(ssm):
    """cmptInitPixJacobian's row k is grad . d(warp of the grid point)/dp_k at the identity, cmptWarpedPixJacobian's the same for the
    update composed behind the current warp with the gradient taken in the warped frame: against a central difference"""
    s = R.SSM(ssm, 9, 7)
    s.set_corners(LC.REGION)
    rng = np.random.default_rng(3)
    grad = rng.standard_normal(2 * s.n)
    g = grad.reshape(2, s.n)
    h = 1e-6
    for warped in (False, True):
        s.set_state(STATES[ssm] if warped else np.zeros(s.S))
        J = (s.cmpt_warped_pix_jacobian(grad) if warped else s.cmpt_init_pix_jacobian(grad)).reshape(s.S, s.n)
        A = s.warp[:2, :2] if warped else np.eye(2)
        for k in range(s.S):
            e = np.zeros(s.S); e[k] = h
            d = (s.apply_warp_to_pts(s.init_pts, e) - s.apply_warp_to_pts(s.init_pts, -e)) / (2 * h)   # dw/dp_k at the identity, (2, n)
            num = ((A.T @ g) * d).sum(axis=0)   # the chain rule through the current warp's 2 x 2 block
            assert np.abs(J[k] - num).max() < 1e-8 * max(1.0, np.abs(num).max()), (warped, k)


@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_rows_are_the_affine_rows_times_m(oracle, ssm):
    """J_S == J_aff M with J_aff from oracle_py.SSM(AFFINE) at the embedded state, both Jacobian variants, to 1e-12 of the rows' scale"""
    size = (9, 7)
    s = R.SSM(ssm, *size)
    s.set_corners(LC.REGION)
    a = oracle.SSM(AC.AFF, *size)
    a.set_corners(LC.REGION)
    # the same grid up to rounding (both are the 4-corner map of a uniform lattice)
    assert np.abs(a.get("init_pts") - s.get("init_pts")).max() < 1e-10
    grad = np.random.default_rng(4).standard_normal(2 * s.n)
    for warped in (False, True):
        s.set_state(STATES[ssm] if warped else np.zeros(s.S))
        a.set_state(s.affine_state())
        Js = (s.cmpt_warped_pix_jacobian(grad) if warped else s.cmpt_init_pix_jacobian(grad)).reshape(s.S, s.n).T
        Ja = (a.cmpt_warped_pix_jacobian(grad) if warped else a.cmpt_init_pix_jacobian(grad)).reshape(6, s.n).T
        err = np.abs(Js - Ja @ R.M[ssm]).max() / np.abs(Ja).max()
        print("J_S = J_aff M, ssm %d warped %d: %.3e" % (ssm, warped, err))
        assert err < 1e-12


@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_estimate_warp_from_corners_recovers_a_model_warp(ssm):
    s = R.SSM(ssm, 5, 5)
    out = s.apply_warp_to_corners(LC.REGION, STATES[ssm])
    est = s.estimate_warp_from_corners(LC.REGION, out)
    assert np.abs(est - STATES[ssm]).max() < 1e-11
    # compose_warps: W(p2) W(p1)
    c = s.compose_warps(STATES[ssm], UPDATES[ssm])
    both = s.apply_warp_to_pts(s.apply_warp_to_pts(LC.REGION, STATES[ssm]), UPDATES[ssm])
    assert np.abs(s.apply_warp_to_pts(LC.REGION, c) - both).max() < 1e-11


# ------------------------------------------------------------------ the condition on the shared inputs
@pytest.mark.parametrize("size", LC.SIZES, ids=LC.SIZE_IDS)
@pytest.mark.parametrize("chained", [1, 0], ids=["chained", "nonchained"])
@pytest.mark.parametrize("method", LC.METHODS, ids=LC.METHOD_IDS)
@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_reference_converges_on_the_shared_cases(oracle, ssm, method, chained, size):
    """on every shared case the reference stops by epsilon after at least two passes, within 0.05 px of where the frame was warped to (SSD)"""
    res = LC.reference(ssm, method, LC.SSD, size, chained)
    err = R.corner_error(res["corners"], LC.true_corners(ssm))
    print("reference ssm %d method %d chained %d %s: n_iters %d, corner error %.4f px" % (ssm, method, chained, size, res["n_iters"], err))
    assert 2 <= res["n_iters"] < LC.PARAMS["max_iters"]
    assert err < 0.05
