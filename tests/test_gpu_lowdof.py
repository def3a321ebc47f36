"""GPU: the Similitude, Isometry and Translation state space models on the device -- the StateSpaceModel entry points and k_pix_jacobian
against tests/helpers/lowdof_ref.py, one fused pass (the affine pixel pass + the projection) and the device loop against LKRef, the
projection identity against an affine batch, the loop against its own single passes and against itself, and the refusals.

Tolerances: one pass on the reference's grid, replay arithmetic: those of tests/test_gpu_alk.py::test_one_pass_parity (f 1e-12, H 1e-9,
g 1e-10 of its scale, the update 1e-6 relative or 1e-12 absolute; the difference is the order of the N-wide sums); tolerance arithmetic:
tests/test_gpu_parity.py's 2e-6 for H and g, 1e-5 for the update; device loops: TOL_CORNERS = 2e-4 px (tests/test_gpu_alk.py:27)."""
import os
import sys

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import alk_cases as AC       # noqa: E402
import lowdof_cases as LC    # noqa: E402
import lowdof_ref as R       # noqa: E402

pytestmark = pytest.mark.gpu
TOL_CORNERS = 2e-4
STATES = {R.TRANS: np.array([1.7, -2.3]), R.ISO: np.array([1.7, -2.3, 0.04]), R.SIM: np.array([1.7, -2.3, 0.03, -0.02])}
UPDATES = {R.TRANS: np.array([-0.4, 0.6]), R.ISO: np.array([-0.4, 0.6, -0.015]), R.SIM: np.array([-0.4, 0.6, -0.01, 0.012])}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d, n = np.linalg.norm(a - b), np.linalg.norm(b)
    return d / n if n > 0 else d


def c24(c8):
    return np.asarray(c8).reshape(4, 2).T


def pts2n(flat):
    return np.asarray(flat).reshape(-1, 2).T


def ref_grid(b, r):
    """the device gets the reference's sample grid verbatim (as tests/test_gpu_alk.py::oracle_grid): every per-pixel quantity is then
    computed from identical inputs"""
    b.write(L.BUF_INIT_PTS, r.init_pts[None])
    b.write(L.BUF_INIT_HXY, r.init_pts[None])
    b.write(L.BUF_INIT_Z, np.ones((1, r.n)))
    b.set_state(np.zeros((1, b.S)))


# ------------------------------------------------------------------ per-function parity
@pytest.mark.parametrize("size", LC.SIZES, ids=LC.SIZE_IDS)
@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_ssm_entry_points_follow_the_reference(gpu_ctx, ssm, size):
    """set_corners' grid, set_state, compositional_update, invert_state, update_grad_pts and both pixel Jacobians, per-pixel arrays to 1e-12
    of their scale (a coordinate's scale is the frame's 320 px)"""
    r = R.SSM(ssm, *size)
    r.set_corners(LC.REGION)
    gpu_ctx.set_image(LC.frame0())
    b = mtf_amd.Batch(gpu_ctx, LC.SSD, ssm, size[0], size[1], 1)
    try:
        assert b.S == r.S == L.lib().mtfhip_batch_state_size(b._h)
        b.set_corners(LC.REGION[None])
        tol = 1e-12 * 320
        assert np.abs(b.read(L.BUF_INIT_PTS)[0] - r.init_pts).max() < tol
        assert np.abs(b.read(L.BUF_CURR_PTS)[0] - r.curr_pts).max() < tol
        assert np.array_equal(b.read(L.BUF_INIT_Z)[0], np.ones(r.n))
        assert not b.get_state().any() and np.array_equal(b.get_warp()[0].ravel(), np.eye(3).ravel())
        ref_grid(b, r)
        grad = np.random.default_rng(5).standard_normal((r.n, 2))
        b.write(L.BUF_DI0_DX, grad[None])
        gflat = np.ascontiguousarray(grad.T.ravel())
        for step in ("set_state", "compositional_update"):
            if step == "set_state":
                r.set_state(STATES[ssm]); b.set_state(STATES[ssm][None])
            else:
                r.compositional_update(UPDATES[ssm]); b.compositional_update(UPDATES[ssm][None])
            assert np.abs(b.get_state()[0] - r.state).max() < 1e-12, step
            assert np.abs(b.get_warp()[0].ravel() - r.warp.ravel()).max() < 1e-12, step
            assert np.abs(b.get_corners()[0] - r.curr_corners).max() < tol, step
            assert np.abs(b.read(L.BUF_CURR_PTS)[0] - r.curr_pts).max() < tol, step
            b.update_grad_pts(1e-8); r.update_grad_pts(1e-8)
            assert np.abs(b.read(L.BUF_GRAD_PTS)[0] - r.grad_pts.reshape(r.n, 8)).max() < tol, step
            for variant, fn in ((L.JAC_INIT, r.cmpt_init_pix_jacobian), (L.JAC_WARPED, r.cmpt_warped_pix_jacobian)):
                b.cmpt_pix_jacobian(variant, L.BUF_DI0_DX, L.BUF_JM)
                want = fn(gflat).reshape(r.S, r.n).T
                got = b.read(L.BUF_JM)[0]
                assert got.shape == want.shape == (r.n, r.S)
                assert np.abs(got - want).max() < 1e-12 * np.abs(want).max(), (step, variant)
        inv = b.invert_state(UPDATES[ssm][None])[0]
        assert np.abs(inv - r.invert_state(UPDATES[ssm])).max() < 1e-12
        out = b.apply_warp_to_corners(LC.REGION[None], STATES[ssm][None])[0]
        assert np.abs(out - r.apply_warp_to_corners(LC.REGION, STATES[ssm])).max() < tol
    finally:
        b.close()


# ------------------------------------------------------------------ one fused pass against LKRef
def _one_pass(oracle, gpu_ctx, ssm, am, method, chained, size, start):
    frame0, frame1 = LC.frame0(), LC.warped(ssm)
    r = R.SSM(ssm, *size)
    o_am = oracle.AM(am, *size); o_am.set_curr_img(frame0)
    hts = {LC.ESM: (2, 0, 1, 3, 4, 5), LC.FCLK: (1, 0, 2), LC.ICLK: (0, 2)}[method]
    ref = R.LKRef(method, o_am, r, hess_type=hts[0], chained_warp=chained, max_iters=1)
    ref.initialize(LC.REGION)
    gpu_ctx.set_image(frame0)
    b = mtf_amd.Batch(gpu_ctx, am, ssm, size[0], size[1], 1)
    worst = dict(f=0.0, H=0.0, g=0.0, dp=0.0, fast_H=0.0, fast_g=0.0, fast_dp=0.0)
    try:
        b.set_corners(LC.REGION[None])
        ref_grid(b, r)
        first = True
        for ht in hts:
            for jt in ((0, 1) if method == LC.ESM and ht == hts[0] else (1,)):
                ref.p["hess_type"], ref.p["jac_type"] = ht, jt
                sm = mtf_amd.sm_desc(method, materialize=1, hess_type=ht, jac_type=jt, chained_warp=chained, max_iters=1)
                if first:
                    b.init_template(sm)
                    assert np.array_equal(b.read(L.BUF_I0)[0], o_am.get("I0"))
                    J0 = b.read(L.BUF_J0)[0]
                    assert J0.shape == (r.n, r.S)
                    want_J0 = np.asarray(ref.J0).reshape(r.S, r.n).T
                    assert np.abs(J0 - want_J0).max() <= 1e-12 * np.abs(want_J0).max()
                    o_am.set_curr_img(frame1); gpu_ctx.set_image(frame1)
                    first = False
                b.set_state(start[None]); r.set_warp(b.get_warp()[0])
                rec = ref.update()["log"][0]
                b.set_math_mode(L.MATH_REPLAY)
                f, g, H = b.iterate(sm)
                assert g.shape == (1, r.S) and H.shape == (1, r.S, r.S)
                assert np.array_equal(b.read(L.BUF_IT)[0], rec["It"]), ht
                if rec["Jt"] is not None and method != LC.ICLK:
                    assert np.array_equal(b.read(L.BUF_DIT_DX)[0], rec["dIt_dx"].reshape(2, -1).T), ht
                    Jt, want = b.read(L.BUF_JT)[0], rec["Jt"].reshape(r.S, -1).T
                    assert Jt.shape == want.shape
                    assert np.abs(Jt - want).max() <= 1e-12 * np.abs(want).max(), ht
                    if method == LC.ESM and (jt == 0 or ht == 3):
                        Jm = (np.asarray(ref.J0).reshape(r.S, -1).T + want) / 2.0
                        assert np.abs(b.read(L.BUF_JM)[0] - Jm).max() <= 1e-12 * np.abs(Jm).max(), ht
                dp = -oracle.colpiv_qr_solve(H[0], g[0])
                g_scale = np.sqrt(abs(np.trace(rec["H"]))) * (np.sqrt(abs(2 * rec["f"])) if am == LC.SSD else 1.0)
                e = dict(f=rel(f[0], rec["f"]), H=rel(H[0], rec["H"]), g=float(np.linalg.norm(g[0] - rec["g"]) / max(np.linalg.norm(rec["g"]), g_scale)),
                         dp=rel(dp, rec["dp"]), dp_abs=float(np.abs(dp - rec["dp"]).max()))
                assert e["f"] < 1e-12, (ht, jt, e)
                assert e["H"] < 1e-9, (ht, jt, e)
                assert e["g"] < 1e-10, (ht, jt, e)
                assert e["dp"] < 1e-6 or e["dp_abs"] < 1e-12, (ht, jt, e)
                # tolerance arithmetic: the lean launch of the same pass
                b.set_math_mode(L.MATH_FAST)
                sm0 = mtf_amd.sm_desc(method, materialize=0, hess_type=ht, jac_type=jt, chained_warp=chained, max_iters=1)
                f2, g2, H2 = b.iterate(sm0)
                dp2 = -oracle.colpiv_qr_solve(H2[0], g2[0])
                e2 = dict(fast_H=rel(H2[0], rec["H"]), fast_g=float(np.linalg.norm(g2[0] - rec["g"]) / max(np.linalg.norm(rec["g"]), g_scale)),
                          fast_dp=rel(dp2, rec["dp"]))
                assert e2["fast_H"] < 2e-6 and e2["fast_g"] < 2e-6 and e2["fast_dp"] < 1e-5, (ht, jt, e2)
                for k in worst:
                    worst[k] = max(worst[k], e.get(k, e2.get(k, 0.0)))
    finally:
        b.close()
    return worst


@pytest.mark.parametrize("size", LC.SIZES, ids=LC.SIZE_IDS)
@pytest.mark.parametrize("chained", [1, 0], ids=["chained", "nonchained"])
@pytest.mark.parametrize("method", LC.METHODS, ids=LC.METHOD_IDS)
@pytest.mark.parametrize("am", [LC.SSD, LC.NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_one_pass_parity(oracle, gpu_ctx, ssm, am, method, chained, size):
    """mtfhip_batch_iterate -- the affine pixel pass, its assembly in affine coordinates, the projection -- against LKRef's first pass away
    from the identity, on the reference's grid, for every hess_type (and both of ESM's jac_type): f, g, H, the update, and the materialised
    It, dIt_dx (bit for bit), JT and ESM's JM as N x S"""
    w = _one_pass(oracle, gpu_ctx, ssm, am, method, chained, size, LC.PASS_START[ssm])
    print("one_pass ssm %d am %d method %d chained %d %s: %s" % (ssm, am, method, chained, size, {k: "%.2e" % v for k, v in w.items()}))


# ------------------------------------------------------------------ the projection identity
@pytest.mark.parametrize("am", [LC.SSD, LC.NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("method", LC.METHODS, ids=LC.METHOD_IDS)
@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_projection_identity(gpu_ctx, ssm, am, method):
    """on the same frame and the same grid, H and g of a low-order batch are M^T H M and g M of an AFFINE batch at the state
    [W02, W12, W00 - 1, W01, W10, W11 - 1] of the low-order batch's warp: to 1e-12 of max |H_aff| (both derive from the same reduced rows)"""
    size = (37, 23)
    frame0, frame1 = LC.frame0(), LC.warped(ssm)
    out = {}
    for kind in (ssm, AC.AFF):
        gpu_ctx.set_image(frame0)
        b = mtf_amd.Batch(gpu_ctx, am, kind, size[0], size[1], 1)
        try:
            b.set_math_mode(L.MATH_REPLAY)
            b.set_corners(LC.REGION[None])
            if kind == ssm:
                grid = b.read(L.BUF_INIT_PTS)
            else:
                b.write(L.BUF_INIT_PTS, grid); b.write(L.BUF_INIT_HXY, grid); b.write(L.BUF_INIT_Z, np.ones((1, size[0] * size[1])))
                b.set_state(np.zeros((1, 6)))
            res = []
            for ht in ({LC.ESM: (2, 5), LC.FCLK: (1, 2), LC.ICLK: (0, 2)}[method]):
                sm = mtf_amd.sm_desc(method, materialize=1, hess_type=ht, max_iters=1)
                gpu_ctx.set_image(frame0)
                b.set_state(np.zeros((1, b.S)))
                b.init_template(sm)
                gpu_ctx.set_image(frame1)
                if kind == ssm:
                    b.set_state(LC.PASS_START[ssm][None])
                    W = b.get_warp()[0].reshape(3, 3)
                    out["aff_state"] = np.array([W[0, 2], W[1, 2], W[0, 0] - 1, W[0, 1], W[1, 0], W[1, 1] - 1])
                else:
                    b.set_state(out["aff_state"][None])
                f, g, H = b.iterate(sm)
                res.append((f[0], g[0].copy(), H[0].copy()))
            out[kind] = res
        finally:
            b.close()
    Mx = R.M[ssm]
    for (f_s, g_s, H_s), (f_a, g_a, H_a) in zip(out[ssm], out[AC.AFF]):
        scale = np.abs(H_a).max()
        eH = np.abs(H_s - Mx.T @ H_a @ Mx).max() / scale
        eg = np.abs(g_s - g_a @ Mx).max() / max(np.abs(g_a).max(), 1e-300)
        print("projection ssm %d am %d method %d: H %.2e g %.2e" % (ssm, am, method, eH, eg))
        assert abs(f_s - f_a) <= 1e-12 * max(1.0, abs(f_a))   # (NCC: the affine batch's template scalars come from its one-launch initialisation)
        assert eH < 1e-12 and eg < 1e-12


# ------------------------------------------------------------------ the device loop against LKRef
def run_loop(ctx, ssm, am, method, size, regions, starts, frame1, trace=0, **params):
    B = len(regions)
    ctx.set_image(LC.frame0())
    b = mtf_amd.Batch(ctx, am, ssm, size[0], size[1], B)
    try:
        b.set_corners(np.asarray(regions))
        sm = mtf_amd.sm_desc(method, **params)
        b.init_template(sm)
        if starts is not None:
            b.set_state(np.asarray(starts))
        ctx.set_image(frame1)
        if trace:
            b.track_trace(trace)
        n_it, corners = b.track(sm)
        recs = b.read_track_trace(n_it) if trace else None
        return n_it.copy(), corners.copy(), b.get_state().copy(), b.get_warp().copy(), recs
    finally:
        b.close()


@pytest.mark.parametrize("size", LC.SIZES, ids=LC.SIZE_IDS)
@pytest.mark.parametrize("lm", [0, 1], ids=["gn", "lm"])
@pytest.mark.parametrize("method", LC.METHODS, ids=LC.METHOD_IDS)
@pytest.mark.parametrize("am", [LC.SSD, LC.NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_device_loop_follows_reference(oracle, gpu_ctx, ssm, am, method, lm, size):
    """mtfhip_batch_track against LKRef.update() on the shared case: the same n_iters, every pass's and the final corners within
    TOL_CORNERS, the state the loop leaves mapped to corners likewise; with and without Levenberg-Marquardt"""
    res = LC.reference(ssm, method, am, size, 1, lm)
    params = dict(hess_type=LC.default_hess(method), leven_marq=lm, materialize=1, **LC.PARAMS)
    n_it, corners, state, warp, recs = run_loop(gpu_ctx, ssm, am, method, size, LC.REGION[None], None, LC.warped(ssm), trace=LC.PARAMS["max_iters"], **params)
    print("device_loop ssm %d am %d method %d lm %d %s: n_iters %d (ref %d), final corner diff %.3e" % (
        ssm, am, method, lm, size, n_it[0], res["n_iters"], np.abs(corners[0] - c24(res["corners"])).max()))
    assert n_it[0] == res["n_iters"]
    np.testing.assert_allclose(corners[0], c24(res["corners"]), rtol=0, atol=TOL_CORNERS)
    for k, (d, r) in enumerate(zip(recs[0], res["log"])):
        assert d["undo"] == r["undo"], k
        np.testing.assert_allclose(d["corners"], c24(r["corners"]), rtol=0, atol=TOL_CORNERS, err_msg="pass %d" % k)
    o = R.SSM(ssm, *size)
    assert state.shape == (1, o.S)
    np.testing.assert_allclose(o.apply_warp_to_corners(LC.REGION, state[0]), c24(res["corners"]), rtol=0, atol=TOL_CORNERS)
    assert np.abs(o.warp_from_state(state[0]) - warp[0].reshape(3, 3)).max() < 1e-12


def _batch_of_three(gpu_ctx, ssm, am, method, ref, distinct=True, **params):
    """the batch of three through mtfhip_batch_track; n_iters and corners against `ref` (distinct: the targets stop behind different
    passes), and the arrays the loop materialises, per target:
    JT is the model's N x S Jacobian of the target's own dIt_dx at the warp ITS last pass ran at -- W_last = W_final U(dp_last)^-1 from
    the trace, exact to rounding: 1e-9 of the rows' scale (rows taken from another target's gradient are a different image; rows taken
    at the warp AFTER the last update differ by the size of that update, printed as `margin`) -- and, where ESM keeps a mean Jacobian,
    JM == (J0 + JT) / 2 bit for bit"""
    size = (37, 23)
    n = size[0] * size[1]
    starts = np.stack([LC.batch_start(ssm, t) for t in range(3)])
    gpu_ctx.set_image(LC.frame0())
    b = mtf_amd.Batch(gpu_ctx, am, ssm, size[0], size[1], 3)
    try:
        b.set_corners(LC.BATCH_REGIONS)
        sm = mtf_amd.sm_desc(method, leven_marq=0, materialize=1, max_iters=15, epsilon=1e-4, **params)
        b.init_template(sm)
        b.set_state(starts)
        gpu_ctx.set_image(LC.warped(ssm))
        b.track_trace(15)
        n_it, corners = b.track(sm)
        recs = b.read_track_trace(n_it)
        print("batch ssm %d am %d method %d %s: n_iters %s (ref %s)" % (ssm, am, method, params, n_it, [r["n_iters"] for r in ref]))
        assert LC.BATCH_REGIONS[2][0].max() > AC.W
        assert [int(v) for v in n_it] == [r["n_iters"] for r in ref]
        if distinct:
            assert len(set(int(v) for v in n_it)) > 1
        for t in range(3):
            np.testing.assert_allclose(corners[t], c24(ref[t]["corners"]), rtol=0, atol=TOL_CORNERS, err_msg="target %d" % t)
        if method == LC.ICLK:
            return
        JT, J0, dIt, grid, W = b.read(L.BUF_JT), b.read(L.BUF_J0), b.read(L.BUF_DIT_DX), b.read(L.BUF_INIT_PTS), b.get_warp()
        assert JT.shape == (3, n, b.S)
        errs, margin = [], []
        for t in range(3):
            r = R.SSM(ssm, *size)
            r.init_pts = grid[t]
            U = r.warp_from_state(recs[t][-1]["dp"])
            r.set_warp(W[t].reshape(3, 3) @ np.linalg.inv(U))
            want = r.cmpt_warped_pix_jacobian(np.ascontiguousarray(dIt[t].T.ravel())).reshape(r.S, n).T
            errs.append(float(np.abs(JT[t] - want).max() / np.abs(want).max()))
            if ssm != R.TRANS:   # (Translation's rows do not depend on the warp)
                r.set_warp(W[t].reshape(3, 3))
                off = r.cmpt_warped_pix_jacobian(np.ascontiguousarray(dIt[t].T.ravel())).reshape(r.S, n).T
                margin.append(float(np.abs(JT[t] - off).max() / np.abs(want).max()))
        print("  JT per target against its own last pass: %s (margin to the final warp: %s)" % (["%.2e" % e for e in errs], ["%.2e" % e for e in margin]))
        assert max(errs) < 1e-9, errs
        if method == LC.ESM and (params.get("jac_type", 1) == 0 or params.get("hess_type") == 3):
            assert np.array_equal(b.read(L.BUF_JM), (J0 + JT) / 2.0)
    finally:
        b.close()


@pytest.mark.parametrize("method", LC.METHODS, ids=LC.METHOD_IDS)
@pytest.mark.parametrize("am", [LC.SSD, LC.NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_device_loop_batch_of_three(oracle, gpu_ctx, ssm, am, method):
    """three targets at three places (the third region reaches past the frame's edge) from three start states: each follows its own
    reference, they stop behind different passes, and the materialised JT of every target is the model's N x S Jacobian at ITS last pass"""
    _batch_of_three(gpu_ctx, ssm, am, method, LC.batch_reference(ssm, method, am, (37, 23)), hess_type=LC.default_hess(method))


@pytest.mark.parametrize("jt,ht", [(0, 2), (1, 3), (0, 3)], ids=["jac_original", "hess_original", "both_original"])
@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_device_loop_leaves_esm_mean_jacobian(oracle, gpu_ctx, ssm, jt, ht):
    """ESM with the Original Jacobian and / or Hessian keeps mean_pix_jacobian (NT/ESM.cc:238-241): behind mtfhip_batch_track JM is the
    N x S mean of J0 and of every target's own JT, and the loop follows LKRef with these types (that the three targets stop behind
    different passes is test_device_loop_batch_of_three's condition, not this test's: with the Original Hessian Translation's do not)"""
    _batch_of_three(gpu_ctx, ssm, LC.SSD, LC.ESM, LC.batch_reference(ssm, LC.ESM, LC.SSD, (37, 23), 0, ht, jt), distinct=False, hess_type=ht,
                    jac_type=jt)


# ------------------------------------------------------------------ the loop against itself
@pytest.mark.parametrize("ssm,am,method,size", [(R.TRANS, LC.SSD, LC.ESM, (50, 50)), (R.ISO, LC.NCC, LC.FCLK, (37, 23)), (R.SIM, LC.SSD, LC.ICLK, (7, 5)),
                                                (R.SIM, LC.NCC, LC.ESM, (37, 23))], ids=["trans_ssd_esm_50", "iso_ncc_fclk_37x23", "sim_ssd_iclk_7x5", "sim_ncc_esm_37x23"])
def test_device_loop_equals_single_passes_and_itself(gpu_ctx, ssm, am, method, size):
    """mtfhip_batch_track with max_iters = n against n calls of one pass each (max_iters = 1), the reduced system of every pass against
    mtfhip_batch_iterate at the state the pass ran at, and two identical calls against each other: bit for bit.  The arrays the loop
    materialises (It, dIt_dx, JT as N x S) are those of the last single pass."""
    params = dict(hess_type=LC.default_hess(method), leven_marq=0, epsilon=1e-4, materialize=1)
    a = run_loop(gpu_ctx, ssm, am, method, size, LC.REGION[None], None, LC.warped(ssm), trace=12, max_iters=12, **params)
    a2 = run_loop(gpu_ctx, ssm, am, method, size, LC.REGION[None], None, LC.warped(ssm), trace=12, max_iters=12, **params)
    n_it, corners, state, warp, recs = a
    assert 2 <= n_it[0] < 12
    assert np.array_equal(n_it, a2[0]) and np.array_equal(corners, a2[1]) and np.array_equal(state, a2[2]) and np.array_equal(warp, a2[3])
    gpu_ctx.set_image(LC.frame0())
    b = mtf_amd.Batch(gpu_ctx, am, ssm, size[0], size[1], 1)
    try:
        b.set_math_mode(L.MATH_REPLAY)
        b.set_corners(LC.REGION[None])
        one = mtf_amd.sm_desc(method, max_iters=1, **params)
        b.init_template(one)
        gpu_ctx.set_image(LC.warped(ssm))
        for k in range(int(n_it[0])):
            f, g, H = b.iterate(one)
            assert rel(g[0], recs[0][k]["g"]) < 1e-12 and rel(H[0], recs[0][k]["H"]) < 1e-12, k   # (the host's and the finish's row sums)
            it_k = b.read(L.BUF_IT).copy()
            jt_k = b.read(L.BUF_JT).copy() if method != LC.ICLK else None
            n1, c1 = b.track(one)
            assert n1[0] == 1
            assert np.array_equal(c1[0], recs[0][k]["corners"]), k
            assert np.array_equal(b.read(L.BUF_IT), it_k), k
            if jt_k is not None:
                assert np.array_equal(b.read(L.BUF_JT), jt_k), k
        assert np.array_equal(c1, corners) and np.array_equal(b.get_state(), state)
    finally:
        b.close()
    # the loop's own materialised arrays: those of its last pass
    gpu_ctx.set_image(LC.frame0())
    b = mtf_amd.Batch(gpu_ctx, am, ssm, size[0], size[1], 1)
    try:
        b.set_corners(LC.REGION[None])
        sm = mtf_amd.sm_desc(method, max_iters=12, **params)
        b.init_template(sm)
        gpu_ctx.set_image(LC.warped(ssm))
        b.track(sm)
        assert np.array_equal(b.read(L.BUF_IT), it_k)
        if jt_k is not None:
            assert b.read(L.BUF_JT).shape == (1, size[0] * size[1], b.S)
            assert np.array_equal(b.read(L.BUF_JT), jt_k)
    finally:
        b.close()


@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_lk_tracker_device_loop_equals_host_solve(gpu_ctx, ssm):
    """sm.LKTracker: the device loop and the host-driven loop (iterate + the host's solve + compositional_update) end within TOL_CORNERS
    of each other and of where the frame was warped to (0.05 px); set_region / update_region serve the three models too"""
    from mtf_amd import sm as SM
    size = (37, 23)
    out = []
    for host_solve in (True, False):
        gpu_ctx.set_image(LC.frame0())
        trk = SM.LKTracker(gpu_ctx, L.SM_ESM, ssm, size[0], size[1], 1, host_solve=host_solve, am=LC.NCC, materialize=1, **LC.PARAMS)
        try:
            trk.initialize(LC.REGION)
            gpu_ctx.set_image(LC.warped(ssm))
            c = trk.update()[0].copy()
            assert R.corner_error(c.T.ravel(), LC.true_corners(ssm)) < 0.05
            c2 = trk.update_region(LC.REGION)[0].copy()
            np.testing.assert_allclose(c2, c, rtol=0, atol=TOL_CORNERS)
            out.append(c)
        finally:
            trk.batch.close()
    np.testing.assert_allclose(out[0], out[1], rtol=0, atol=TOL_CORNERS)


@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_nt_search_method_over_the_per_function_entry_points(oracle, gpu_ctx, ssm):
    """sm.NTSearchMethod -- nt::ESM / FCLK / ICLK written against the AM / SSM entry points, one C-ABI call per reference virtual --
    over a low-order batch: the same n_iters as LKRef and its corners within TOL_CORNERS"""
    from mtf_amd import sm as SM
    size = (37, 23)
    for method in LC.METHODS:
        res = LC.reference(ssm, method, LC.SSD, size, 1, 0)
        gpu_ctx.set_image(LC.frame0())
        nt = SM.NTSearchMethod(gpu_ctx, method, LC.SSD, ssm, size[0], size[1], 1, hess_type=LC.default_hess(method), **LC.PARAMS)
        try:
            nt.initialize(LC.REGION)
            gpu_ctx.set_image(LC.warped(ssm))
            c = nt.update()[0]
            assert len(nt.trace) == res["n_iters"], method
            np.testing.assert_allclose(c, c24(res["corners"]), rtol=0, atol=TOL_CORNERS)
        finally:
            nt.batch.close()


@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_cpp_host_layer(gpu_ctx, ssm):
    """the C++ layer: nt::ESM / FCLK / ICLK of the harness over HipAM + HipSSM of a low-order kind (the per-function entry points) and
    mtf::hip::LK (one mtfhip_batch_track call per update()) run the three models -- the same n_iters as LKRef and as each other, corners
    within TOL_CORNERS; hip::LK against sm.LKTracker's device loop with the same parameters: the same n_iters and corners -- and what the
    ABI refuses arrives as the reference's FunctonNotImplemented"""
    from mtf_amd import sm as SM
    from mtf_amd.host import CppTracker, CppParticleFilter, HostError
    size = (37, 23)
    for method in LC.METHODS:
        res = LC.reference(ssm, method, LC.SSD, size, 1, 0)
        gpu_ctx.set_image(LC.frame0())
        # (materialize = 0 as mtf::hip::LK asks: the two are then the same mtfhip_batch_track call on the same inputs)
        py = SM.LKTracker(gpu_ctx, method, ssm, size[0], size[1], 1, host_solve=False, am=LC.SSD, hess_type=LC.default_hess(method), leven_marq=0,
                          materialize=0, **LC.PARAMS)
        try:
            py.initialize(LC.REGION)
            gpu_ctx.set_image(LC.warped(ssm))
            py_c, py_n = py.update()[0].copy(), int(np.asarray(py.n_iters).ravel()[0])
        finally:
            py.batch.close()
        got = []
        for device_loop in (False, True):
            trk = CppTracker(method, am=LC.SSD, ssm=ssm, resx=size[0], resy=size[1], hess_type=LC.default_hess(method), leven_marq=0,
                             device_loop=device_loop, **LC.PARAMS)
            trk.set_image(LC.frame0())
            trk.initialize(LC.REGION)
            trk.set_image(LC.warped(ssm))
            c = np.asarray(trk.update()).reshape(2, 4)
            assert trk.iters == res["n_iters"], (method, device_loop)
            np.testing.assert_allclose(c, c24(res["corners"]), rtol=0, atol=TOL_CORNERS)
            got.append(c)
        np.testing.assert_allclose(got[0], got[1], rtol=0, atol=TOL_CORNERS)
        # hip::LK == sm.LKTracker: both are one mtfhip_batch_track call on the same inputs
        assert py_n == res["n_iters"]
        print("hip::LK vs sm.LKTracker ssm %d method %d: corner diff %.3e" % (ssm, method, np.abs(got[1] - py_c).max()))
        assert np.array_equal(got[1], py_c), (ssm, method)
    falk = CppTracker(L.SM_FALK, am=LC.SSD, ssm=ssm, resx=10, resy=10, leven_marq=0)
    falk.set_image(LC.frame0())
    with pytest.raises(HostError) as e:     # nt::FALK's initialize reaches cmptPixJacobian, which the ABI refuses for these models
        falk.initialize(LC.REGION)
    assert str(e.value).startswith("FunctonNotImplemented: "), str(e.value)   # (the C wrapper reports "<exception type>: <what>")
    with pytest.raises(HostError):
        CppParticleFilter(ssm=ssm, resx=10, resy=10)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_refusals(gpu_ctx, ssm):
    """what the three models are not served with returns MTFHIP_ERR_NOT_IMPLEMENTED with a reason, before anything is launched"""
    def refused(fn, *a, **k):
        with pytest.raises(L.FunctionNotImplemented) as e:
            fn(*a, **k)
        assert e.value.code == -2 and len(str(e.value)) > 30
    gpu_ctx.set_image(LC.frame0())
    for am in (L.AM_MI, L.AM_SCV, L.AM_RSCV, L.AM_LSCV, L.AM_LRSCV):
        refused(mtf_amd.Batch, gpu_ctx, am, ssm, 10, 10, 1)
    refused(mtf_amd.Batch, gpu_ctx, LC.SSD, ssm, 10, 10, 1, n_channels=3)
    b = mtf_amd.Batch(gpu_ctx, LC.SSD, ssm, 10, 10, 1)
    try:
        S = b.S
        b.set_corners(LC.REGION[None])
        for variant in (L.JAC_PIX, L.JAC_APPROX):
            refused(b.cmpt_pix_jacobian, variant, L.BUF_DI0_DX, L.BUF_J0)
        refused(b.update_hess_pts)
        refused(b.initialize_pix_hess)
        refused(b.update_pix_hess)
        refused(b.cmpt_pix_hessian, L.JAC_INIT, L.BUF_D2I0_DX2, L.BUF_DI0_DX, L.BUF_D2I0_DP2)
        refused(b.mean_pix_hessian)
        refused(b.cmpt_init_hessian2); refused(b.cmpt_curr_hessian2); refused(b.cmpt_self_hessian2); refused(b.cmpt_sum_of_hessians2)
        refused(b.additive_update, np.zeros((1, S)))
        refused(b.estimate_state_sigma, 1.0)
        for sm_kind in (L.SM_FALK, L.SM_IALK):
            sm = mtf_amd.sm_desc(sm_kind)
            refused(b.init_template, sm); refused(b.iterate, sm); refused(b.track, sm)
        so = mtf_amd.sm_desc(L.SM_ESM, sec_ord_hess=1)
        refused(b.init_template, so); refused(b.iterate, so); refused(b.track, so); refused(b.set_region, LC.REGION[None], so)
        sm = mtf_amd.sm_desc(L.SM_ICLK)
        refused(b.grid_update, LC.REGION[None], sm)
        gd = L.GridDesc(1, 1, 10, 10, 1, 0, 1)
        refused(b.grid_frame, gd, sm, LC.REGION)
        refused(b.grid_reset, gd, sm, LC.REGION, 1)
        fb = L.GridFbDesc(2.0, 1, 4)
        refused(b.grid_backward, gd, sm, fb)
        refused(b.grid_frame_fb, gd, sm, fb, np.zeros((1, 2), dtype=np.float32), LC.REGION)
        refused(b.score_candidates, np.zeros((4, S)))
        refused(b.sample_candidates, np.zeros((4, S)))
        refused(b.nn_dataset, 8, np.full(S, 0.01))
        # the device-pointer forms: any buffer of the batch serves as the address (nothing may be read or written before the refusal)
        dev = b.device_ptr(L.BUF_I0)
        refused(b.score_candidates_dev, dev, 4, dev)
        refused(lambda: L.check(L.lib().mtfhip_sample_candidates_dev(b._h, L.C.c_void_p(dev), 4, L.C.c_void_p(dev))))
        refused(b.nn_dataset_dev, b.nn_desc(8, np.full(S, 0.01)), dev, 0, 8)
        refused(b.nn_create, 8)
        refused(gpu_ctx.estimate_warp_from_pts, ssm, np.zeros((8, 2), dtype=np.float32), np.zeros((8, 2), dtype=np.float32))
        from mtf_amd import sm as SM
        refused(SM.ParticleFilter, gpu_ctx, ssm=ssm)
        # the batch is still good for what it does serve
        b.init_template(mtf_amd.sm_desc(L.SM_ESM))
        f, g, H = b.iterate(mtf_amd.sm_desc(L.SM_ESM))
        assert g.shape == (1, S) and np.isfinite(H).all()
    finally:
        b.close()
