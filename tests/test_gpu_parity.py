"""GPU parity: every C-ABI entry point of the hot path against the CPU oracle on the same seeded
inputs (sizes the oracle finishes in seconds).  Tolerances: bit-exact where the device replays the
reference's per-pixel arithmetic (samples, gradients, Jacobian rows), 1e-5 relative (north_star)
on H / g / parameter updates, 1e-9 relative on PF scores."""
import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.linalg.norm(a - b)
    n = np.linalg.norm(b)
    return d / n if n > 0 else d


def make_pair(oracle, ctx, img, am, ssm, res, corners, **kw):
    o_ssm = oracle.SSM(ssm, res, res)
    o_names = {"mi_pou": "pou", "mi_n_bins": "n_bins", "mi_pre_seed": "pre_seed"}   # (the C ABI's field names -> the oracle's)
    o_am = oracle.AM(am, res, res, **{o_names.get(k, k): v for k, v in kw.items()})
    o_am.set_curr_img(img)
    ctx.set_image(img)
    b = mtf_amd.Batch(ctx, am, ssm, res, res, 1, **{k: v for k, v in kw.items()})
    o_ssm.set_corners(corners)
    b.set_corners(corners[None])
    return o_am, o_ssm, b


CORNER_SETS = {
    "square": lambda rng: synth.square_corners(256, 256, 100),
    "quad": lambda rng: synth.square_corners(256, 256, 100) + rng.uniform(-4, 4, size=(2, 4)),
}


@pytest.mark.parametrize("ssm", [L.SSM_HOMOGRAPHY, L.SSM_AFFINE])
@pytest.mark.parametrize("shape", ["square", "quad"])
def test_ssm_grid_and_warp(oracle, gpu_ctx, frame, ssm, shape):
    rng = np.random.default_rng(11)
    corners = CORNER_SETS[shape](rng)
    o_am, o_ssm, b = make_pair(oracle, gpu_ctx, frame, L.AM_SSD, ssm, 50, corners)
    S = b.S
    np.testing.assert_allclose(b.read(L.BUF_INIT_PTS)[0], o_ssm.get("init_pts").reshape(-1, 2).T, rtol=0, atol=1e-9)
    p = synth.random_small_homography(rng)[:S] if ssm == L.SSM_HOMOGRAPHY else rng.uniform(-1, 1, 6) * [2, 2, .02, .02, .02, .02]
    o_ssm.set_state(p)
    b.set_state(p[None])
    np.testing.assert_allclose(b.get_pts()[0], o_ssm.get("curr_pts").reshape(-1, 2).T, rtol=0, atol=1e-9)
    np.testing.assert_allclose(b.get_corners()[0], o_ssm.get("curr_corners").reshape(4, 2).T, rtol=0, atol=1e-9)
    dp = p * 0.1
    o_ssm.compositional_update(dp)
    b.compositional_update(dp[None])
    np.testing.assert_allclose(b.get_state()[0], o_ssm.get("state"), rtol=0, atol=1e-12)
    np.testing.assert_allclose(b.get_pts()[0], o_ssm.get("curr_pts").reshape(-1, 2).T, rtol=0, atol=1e-9)
    np.testing.assert_allclose(b.invert_state(p[None])[0], o_ssm.invert_state(p), rtol=1e-12, atol=1e-14)
    o_ssm.update_grad_pts(1e-8)
    b.update_grad_pts(1e-8)
    np.testing.assert_allclose(b.read(L.BUF_GRAD_PTS)[0].ravel(), o_ssm.get("grad_pts"), rtol=0, atol=1e-9)


@pytest.mark.parametrize("ssm", [L.SSM_HOMOGRAPHY, L.SSM_AFFINE])
def test_unfused_interface_chain(oracle, gpu_ctx, frame, ssm):
    """updatePixVals -> updateSimilarity -> updateCurrGrad -> updatePixGrad -> cmpt*PixJacobian ->
    cmptCurrJacobian / cmpt*Hessian, each as its own C-ABI call, fed with the oracle's points."""
    rng = np.random.default_rng(5)
    corners = synth.square_corners(250, 260, 90)
    o_am, o_ssm, b = make_pair(oracle, gpu_ctx, frame, L.AM_SSD, ssm, 40, corners)
    S = b.S
    pts0 = o_ssm.get("curr_pts")
    o_am.initialize_pix_vals(pts0); o_am.initialize_pix_grad_pts(pts0)
    o_am.initialize_similarity(); o_am.initialize_grad(); o_am.initialize_hess()
    # fed with the oracle's own points the device replays the reference's arithmetic bit for bit
    pts0_np = pts0.reshape(1, -1, 2).transpose(0, 2, 1)
    b.initialize_pix_vals(pts0_np); b.initialize_pix_grad(pts0_np)
    b.initialize_similarity(); b.initialize_grad(); b.initialize_hess()
    assert np.array_equal(b.read(L.BUF_I0)[0], o_am.get("I0"))
    assert np.array_equal(b.read(L.BUF_DI0_DX)[0], o_am.get("dI0_dx").reshape(2, -1).T)
    J0_o = o_ssm.cmpt_warped_pix_jacobian(o_am.get("dI0_dx"))
    b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DI0_DX, L.BUF_J0)
    np.testing.assert_allclose(b.read(L.BUF_J0)[0], J0_o.reshape(S, -1).T, rtol=1e-9, atol=1e-7)

    p = (synth.random_small_homography(rng) if ssm == L.SSM_HOMOGRAPHY else
         rng.uniform(-1, 1, 6) * [2, 2, .02, .02, .02, .02])
    o_ssm.set_state(p); b.set_state(p[None])
    pts = o_ssm.get("curr_pts")
    # explicit host points (upload path) must equal the device-resident fast path
    o_am.update_pix_vals(pts)
    b.update_pix_vals()
    it_dev = b.read(L.BUF_IT)[0].copy()
    b.update_pix_vals(pts.reshape(1, -1, 2).transpose(0, 2, 1))
    it_host = b.read(L.BUF_IT)[0].copy()
    np.testing.assert_allclose(it_dev, it_host, rtol=0, atol=1e-9)
    assert np.array_equal(it_host, o_am.get("It"))

    o_am.update_similarity(False); b.update_similarity(False)
    assert rel(b.get_similarity()[0], o_am.similarity) < 1e-12
    assert rel(b.get_likelihood()[0], o_am.likelihood) < 1e-12
    o_am.update_curr_grad(); b.update_curr_grad()
    o_am.update_init_grad(); b.update_init_grad()
    np.testing.assert_allclose(b.read(L.BUF_DF_DIT)[0], o_am.get("df_dIt"), rtol=0, atol=1e-9)

    # chained: gradient at the warped points + warped Jacobian
    o_am.update_pix_grad_pts(pts); b.update_pix_grad(pts.reshape(1, -1, 2).transpose(0, 2, 1))
    assert np.array_equal(b.read(L.BUF_DIT_DX)[0], o_am.get("dIt_dx").reshape(2, -1).T)
    for variant, fn in ((L.JAC_WARPED, o_ssm.cmpt_warped_pix_jacobian), (L.JAC_INIT, o_ssm.cmpt_init_pix_jacobian),
                        (L.JAC_PIX, o_ssm.cmpt_pix_jacobian), (L.JAC_APPROX, o_ssm.cmpt_approx_pix_jacobian)):
        Jo = fn(o_am.get("dIt_dx"))
        b.cmpt_pix_jacobian(variant, L.BUF_DIT_DX, L.BUF_JT)
        assert rel(b.read(L.BUF_JT)[0], Jo.reshape(S, -1).T) < 1e-6, variant
    Jt_o = o_ssm.cmpt_warped_pix_jacobian(o_am.get("dIt_dx"))
    b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DIT_DX, L.BUF_JT)
    assert rel(b.cmpt_curr_jacobian()[0], o_am.cmpt_curr_jacobian(Jt_o)) < 1e-5
    assert rel(b.cmpt_init_jacobian()[0], o_am.cmpt_init_jacobian(J0_o)) < 1e-5
    assert rel(b.cmpt_difference_of_jacobians()[0], o_am.cmpt_difference_of_jacobians(J0_o, Jt_o)) < 1e-5
    assert rel(b.cmpt_self_hessian()[0], o_am.cmpt_self_hessian(Jt_o)) < 1e-5
    assert rel(b.cmpt_curr_hessian()[0], o_am.cmpt_curr_hessian(Jt_o)) < 1e-5
    assert rel(b.cmpt_init_hessian()[0], o_am.cmpt_init_hessian(J0_o)) < 1e-5
    assert rel(b.cmpt_sum_of_hessians()[0], o_am.cmpt_sum_of_hessians(J0_o, Jt_o)) < 1e-5
    b.mean_jacobian()
    np.testing.assert_allclose(b.read(L.BUF_JM)[0], ((J0_o + Jt_o) / 2).reshape(S, -1).T, rtol=1e-6, atol=1e-6)

    # non-chained: gradient of the warped image through the offset points
    o_ssm.update_grad_pts(1e-8); b.update_grad_pts()
    o_am.update_pix_grad_warped(o_ssm.get("grad_pts")); b.update_pix_grad(o_ssm.get("grad_pts").reshape(1, -1, 8), warped=True)
    assert np.array_equal(b.read(L.BUF_DIT_DX)[0], o_am.get("dIt_dx").reshape(2, -1).T)
    b.update_pix_grad(warped=True)   # device-resident offset points: same up to the grid's 1e-13 jitter
    np.testing.assert_allclose(b.read(L.BUF_DIT_DX)[0], o_am.get("dIt_dx").reshape(2, -1).T, rtol=0, atol=5e-5)


SM_CASES = [
    # sm, ssm, res, extra
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 50, dict()),                                  # config 1
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 50, dict(chained_warp=0)),
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(jac_type=0, hess_type=3)),           # Original + Original
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(hess_type=5)),
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(hess_type=0)),
    (L.SM_FCLK, L.SSM_HOMOGRAPHY, 100, dict()),                                # config 2 shape, reduced
    (L.SM_FCLK, L.SSM_HOMOGRAPHY, 60, dict(chained_warp=0)),
    (L.SM_FCLK, L.SSM_AFFINE, 50, dict()),
    (L.SM_FCLK, L.SSM_AFFINE, 50, dict(chained_warp=0)),
    (L.SM_ICLK, L.SSM_HOMOGRAPHY, 50, dict()),
    (L.SM_ICLK, L.SSM_AFFINE, 25, dict()),                                     # config 3 patch shape
    (L.SM_ESM, L.SSM_AFFINE, 40, dict()),
    # second-order Hessians through the fused path (k_second_order_ssd keeps the S x S pixel-Hessian blocks in registers)
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(sec_ord_hess=1, hess_type=5)),
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(sec_ord_hess=1, hess_type=4, chained_warp=0)),
    (L.SM_ESM, L.SSM_AFFINE, 40, dict(sec_ord_hess=1, hess_type=3, jac_type=0)),
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(sec_ord_hess=1)),                    # SumOfSelf: SSD's self Hessian stays first order
    (L.SM_FCLK, L.SSM_HOMOGRAPHY, 50, dict(sec_ord_hess=1, hess_type=2)),
    (L.SM_FCLK, L.SSM_AFFINE, 40, dict(sec_ord_hess=1, hess_type=2, chained_warp=0)),
    (L.SM_ICLK, L.SSM_HOMOGRAPHY, 40, dict(sec_ord_hess=1, hess_type=2)),
    (L.SM_ICLK, L.SSM_AFFINE, 25, dict(sec_ord_hess=1, hess_type=2, chained_warp=0)),
]


def _case_id(c):
    return "sm%d-ssm%d-res%d-%s" % (c[0], c[1], c[2], "_".join("%s%s" % kv for kv in c[3].items()))


NCC_CASES = [
    # the fused kernel accumulates raw moments for NCC; f, g and every first-order Hessian type are assembled from them
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 50, dict()),                                  # DiffOfJacs + SumOfSelf (class defaults)
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(jac_type=0, hess_type=3)),           # Original + Original (mean Jacobian)
    (L.SM_ESM, L.SSM_AFFINE, 40, dict(hess_type=4, chained_warp=0)),           # SumOfStd
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(hess_type=5, jac_type=0)),           # Original Jacobian + Std Hessian
    (L.SM_ESM, L.SSM_AFFINE, 40, dict(hess_type=1)),
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(hess_type=0)),
    (L.SM_FCLK, L.SSM_HOMOGRAPHY, 60, dict()),                                 # CurrentSelf
    (L.SM_FCLK, L.SSM_AFFINE, 50, dict(hess_type=2, chained_warp=0)),
    (L.SM_FCLK, L.SSM_HOMOGRAPHY, 40, dict(hess_type=0)),
    (L.SM_ICLK, L.SSM_HOMOGRAPHY, 50, dict()),
    (L.SM_ICLK, L.SSM_AFFINE, 25, dict(hess_type=2)),                          # Std: cmptInitHessian depends on the frame
    # second order (NCC.cc:391-410): the weighted pixel-Hessian sums with NCC's own gradients as weights
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(sec_ord_hess=1, hess_type=5)),
    (L.SM_ESM, L.SSM_AFFINE, 40, dict(sec_ord_hess=1, hess_type=4, chained_warp=0)),
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(sec_ord_hess=1, hess_type=3, jac_type=0)),
    (L.SM_FCLK, L.SSM_HOMOGRAPHY, 40, dict(sec_ord_hess=1, hess_type=2)),
    (L.SM_FCLK, L.SSM_AFFINE, 40, dict(sec_ord_hess=1, hess_type=2, chained_warp=0)),
    (L.SM_ICLK, L.SSM_HOMOGRAPHY, 40, dict(sec_ord_hess=1, hess_type=2)),
    (L.SM_ICLK, L.SSM_AFFINE, 25, dict(sec_ord_hess=1, hess_type=2, chained_warp=0)),
]


@pytest.mark.parametrize("grid", ["oracle_grid", "device_grid"])
@pytest.mark.parametrize("materialize", [1, 0])
@pytest.mark.parametrize("case", NCC_CASES, ids=_case_id)
def test_fused_ncc_iterations_follow_oracle(oracle, gpu_ctx, frame, case, materialize, grid):
    """NCC through the fused kernel (k_fused_ncc: one pass, raw moments) against the oracle's nt:: trackers, iteration by
    iteration, as test_fused_iterations_follow_oracle does for SSD."""
    _fused_follow(oracle, gpu_ctx, frame, L.AM_NCC, case, materialize, grid)


MI_CASES = [
    # fused MI iteration: pass 0 = the fused LK kernel materialising It / dIt_dx / Jt, then one histogram pass and
    # one gradient + Hessian pass; the class-default (self-type) Hessians
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 50, dict()),                                  # config 5 shape (DiffOfJacs + SumOfSelf), reduced
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(hess_type=1, chained_warp=0)),
    (L.SM_ESM, L.SSM_AFFINE, 40, dict(hess_type=0)),
    (L.SM_FCLK, L.SSM_HOMOGRAPHY, 50, dict()),                                 # CurrentSelf
    (L.SM_FCLK, L.SSM_AFFINE, 40, dict(hess_type=0, chained_warp=0)),
    (L.SM_ICLK, L.SSM_HOMOGRAPHY, 40, dict()),
    # the other first-order types: cmptCurrHessian / cmptInitHessian / cmptSumOfHessians, the mean Jacobian
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(hess_type=5)),                       # Std
    (L.SM_ESM, L.SSM_AFFINE, 40, dict(hess_type=4, chained_warp=0)),           # SumOfStd
    (L.SM_ESM, L.SSM_HOMOGRAPHY, 40, dict(hess_type=3, jac_type=0)),           # Original + Original
    (L.SM_ESM, L.SSM_AFFINE, 36, dict(jac_type=0)),                            # Original Jacobian, SumOfSelf
    (L.SM_FCLK, L.SSM_HOMOGRAPHY, 40, dict(hess_type=2)),                      # Std
    (L.SM_ICLK, L.SSM_AFFINE, 30, dict(hess_type=2)),                          # Std: cmptInitHessian(J0)
    (L.SM_ICLK, L.SSM_HOMOGRAPHY, 36, dict(hess_type=1)),                      # CurrentSelf: needs the current Jacobian
]


@pytest.mark.parametrize("grid", ["oracle_grid", "device_grid"])
@pytest.mark.parametrize("materialize", [1, 0])
@pytest.mark.parametrize("case", MI_CASES, ids=_case_id)
def test_fused_mi_iterations_follow_oracle(oracle, gpu_ctx, frame, case, materialize, grid):
    _fused_follow(oracle, gpu_ctx, frame, L.AM_MI, case, materialize, grid)


@pytest.mark.parametrize("rowsum", ["1", "0"])
@pytest.mark.parametrize("materialize", [1, 0])
@pytest.mark.parametrize("case", [MI_CASES[0], MI_CASES[1], MI_CASES[4], MI_CASES[5], MI_CASES[6]], ids=_case_id)
def test_fused_mi_partition_of_unity(oracle, gpu_ctx, frame, case, materialize, rowsum, monkeypatch):
    """mi_pou = 1, what the shipped Config/modules.cfg:117 sets (MI.cc:80-94: pixel values mapped to [1, n_bins - 2], every B-spline window
    inside the bins).  There the recompute pass takes the histogram of It as the row sums of the joint histogram (the windows of I0 sum to
    one) instead of a block product of its own; MTFHIP_MI_HIST_ROWSUM=0 keeps the product: both held to the oracle like every other case"""
    monkeypatch.setenv("MTFHIP_MI_HIST_ROWSUM", rowsum)
    _fused_follow(oracle, gpu_ctx, frame, L.AM_MI, case, materialize, "device_grid", am_kw=dict(mi_pou=1))


@pytest.mark.parametrize("pou", [0, 1])
@pytest.mark.parametrize("n_bins", [10, 9, 5])
@pytest.mark.parametrize("case", [MI_CASES[0], MI_CASES[1], MI_CASES[2], MI_CASES[3], MI_CASES[5], MI_CASES[12]], ids=_case_id)
def test_fused_mi_other_bin_counts(oracle, gpu_ctx, frame, case, n_bins, pou):
    """r06: the recompute passes with other bin counts than 8 -- the shipped configuration is mi_n_bins 10 with the partition of unity
    (Config/modules.cfg:115-117) -- for the constant and the self Hessian forms of the three search methods: ten-class sort, 3 x 3 tiles of
    the histograms' block products, the waves' moment tables (k_mi_pass_hist / k_mi_pass_grad_hess <.., NB = 10>).  Held to the
    oracle exactly as the 8-bin cases are (_fused_follow: both arithmetic modes, every iteration).  9 and 5 bins: ragged last tiles."""
    if pou and n_bins < 4:
        pytest.skip("MI::Too few bins to enforce the partition of unity constraint (MI.cc:83-87)")
    dp_tol = 1e-5
    if n_bins != 10 and case[3].get("chained_warp") == 0:
        # (measured before: dp 1.1e-5 / 1.25e-5 at 9 bins + pou and 5 bins -- MI's update is ill-conditioned there and the reference's own
        # update moves by as much when its finite-difference step or its gradient route changes.)  The bound is that floor, measured here
        # for this case: 4 x the floor, never above 1e-4 absolute -- and never below the 1e-5 budget the other cases are held to
        floor = _mi_dp_noise_floor(oracle, frame, case, n_bins, pou)
        dp_tol = min(max(4.0 * floor, 1e-5), 1e-4)
    _fused_follow(oracle, gpu_ctx, frame, L.AM_MI, case, 0, "device_grid", am_kw=dict(mi_n_bins=n_bins, mi_pou=pou), dp_tol=dp_tol)


def _mi_dp_noise_floor(oracle, frame, case, n_bins, pou):
    """How far the oracle's own MI parameter update moves for this case's search method, bin count and pou (as test_oracle_relations.py::test_mi_update_noise_floor does for 8 bins): the relative dp between the oracle at
    grad_eps 1e-8 and at 2e-8, and between the non-chained and the chained route, over the first two iterations (where dp is held
    plain relative; later ones go to zero); each run follows its own trajectory from _fused_follow's start."""
    sm_kind, ssm, res, extra = case
    rng = np.random.default_rng(17)
    centre = (250.0, 262.0)
    corners = synth.square_corners(centre[0], centre[1], 2.0 * res if res <= 60 else float(res))
    frame2 = synth.warp_frame(frame, synth.random_small_homography(rng, 0.6), centre)

    def run(eps, chained):
        o_ssm = oracle.SSM(ssm, res, res)
        o_am = oracle.AM(L.AM_MI, res, res, grad_eps=eps, n_bins=n_bins, pou=pou)
        o_am.set_curr_img(frame)
        params = dict(leven_marq=0, max_iters=8)
        params.update(extra)
        params["chained_warp"] = chained
        trk = oracle.Tracker(sm_kind, o_am, o_ssm, **params)
        trk.initialize(corners); o_am.set_curr_img(frame2); trk.update()
        return trk.trace()

    a, b, c = run(1e-8, 0), run(2e-8, 0), run(1e-8, 1)
    return max(max(rel(a[k]["dp"], b[k]["dp"]), rel(a[k]["dp"], c[k]["dp"])) for k in range(2))


@pytest.mark.parametrize("grid", ["oracle_grid", "device_grid"])
@pytest.mark.parametrize("materialize", [1, 0])
@pytest.mark.parametrize("case", SM_CASES, ids=_case_id)
def test_fused_iterations_follow_oracle(oracle, gpu_ctx, frame, case, materialize, grid):
    _fused_follow(oracle, gpu_ctx, frame, L.AM_SSD, case, materialize, grid)


# _fused_follow's bounds on (f, H, g), by grid and arithmetic (the seam suites take them from here); the update: DP_TOL relative, or
# DP_CORNER_PX at the corners; LOOP_CORNER_PX: the corners after a device-side loop (_device_loop)
FOLLOW_BOUNDS = dict(oracle_grid=(1e-12, 1e-9, 1e-10), device_grid=(1e-8, 1e-5, 1e-5), fast=(1e-8, 2e-6, 2e-6))
DP_TOL, DP_CORNER_PX, LOOP_CORNER_PX = 1e-5, 1e-6, 2e-4


def _fused_follow(oracle, gpu_ctx, frame, am, case, materialize, grid, am_kw=None, dp_tol=DP_TOL):
    """Drive the SM loop on the host exactly as the reference does (solve + compositional update on the
    CPU), with the device producing f, g, H per iteration; compare every iteration with the oracle's
    trace of nt::ESM / nt::FCLK / nt::ICLK::update.

    oracle_grid: the device gets the oracle's sample grid verbatim, so every per-pixel quantity is
      bit-identical and only the summation order differs -> 1e-9.
    device_grid: the device builds its own grid from the corners (its 4-point DLT differs from the
      oracle's by ~1e-13 px).  The reference's grad_eps = 1e-8 finite difference turns that jitter into
      ~5e-6 absolute noise on every image-gradient component (the reference's own noise floor), so H and
      the parameter update are held to the north-star 1e-5, and g to 1e-5 of its Cauchy-Schwarz scale
      ||J||_F ||r|| (g itself cancels to ~0 at convergence).
    dp_tol: the relative bound on the parameter update where north_star's 1e-5 holds it (a caller passes a measured noise floor
      where the reference's own update moves by more; H, g and f keep their bounds)."""
    sm_kind, ssm, res, extra = case
    rng = np.random.default_rng(17)
    centre = (250.0, 262.0)
    corners = synth.square_corners(centre[0], centre[1], 2.0 * res if res <= 60 else float(res))
    p_true = synth.random_small_homography(rng, 0.6)
    frame2 = synth.warp_frame(frame, p_true, centre)

    params = dict(leven_marq=0, max_iters=8)
    params.update(extra)
    o_am, o_ssm, b = make_pair(oracle, gpu_ctx, frame, am, ssm, res, corners, **(am_kw or {}))
    ncc = am == L.AM_NCC
    if grid == "oracle_grid":
        hm = o_ssm.get("init_pts_hm").reshape(-1, 3)
        b.write(L.BUF_INIT_PTS, o_ssm.get("init_pts").reshape(1, -1, 2).transpose(0, 2, 1))
        b.write(L.BUF_INIT_HXY, hm[:, :2].T[None])
        b.write(L.BUF_INIT_Z, hm[:, 2][None])
        b.set_state(np.zeros((1, b.S)))
    trk = oracle.Tracker(sm_kind, o_am, o_ssm, **params)
    trk.initialize(corners)
    sm = mtf_amd.sm_desc(sm_kind, materialize=materialize, **params)
    b.init_template(sm)

    o_am.set_curr_img(frame2)
    gpu_ctx.set_image(frame2)
    trk.update()
    trace = trk.trace()
    assert len(trace) >= 2
    tight = grid == "oracle_grid"
    b.set_math_mode(mtf_amd.MATH_REPLAY)
    # Tolerance-mode arithmetic (the lean launch: FMA, one reciprocal per point, the CLOSED-FORM slope of the bilinear cell times the
    # ROUNDED step of the reference's central difference -- fd_step, mtfhip_device.h) is held to the reference-parameter oracle
    # (grad_eps = 1e-8): the step 1e-8 is quantised by the coordinates it is added to (175 921.86 ulps of a coordinate in [256, 512)
    # become 175 922: a systematic ~1e-6 .. 1e-5 on every gradient), r03's closed form did not carry that factor and sat 1e-5 from
    # the oracle in H; r04's does: (ii) H and g within 2e-6, dp within north_star's 1e-5.  (i) The same restatement run with
    # grad_eps = 1e-6 (a hundred times less quantisation) is now the farther one: its distance is bounded by the quantisation itself
    # and recorded.
    o_kw = {{"mi_pou": "pou", "mi_n_bins": "n_bins", "mi_pre_seed": "pre_seed"}.get(k, k): v for k, v in (am_kw or {}).items()}
    o_am6 = oracle.AM(am, res, res, grad_eps=1e-6, **o_kw); o_ssm6 = oracle.SSM(ssm, res, res)
    o_am6.set_curr_img(frame); o_ssm6.set_corners(corners)
    trk6 = oracle.Tracker(sm_kind, o_am6, o_ssm6, **dict(params, max_iters=1))
    trk6.initialize(corners); o_am6.set_curr_img(frame2)
    fast_vs_6 = dict(H=0.0, g=0.0, dp=0.0); fast_vs_8 = dict(H=0.0, g=0.0, dp=0.0)
    for it, rec in enumerate(trace):
        if not materialize and not tight:
            b.set_math_mode(mtf_amd.MATH_FAST)
            ff, gf, Hf = b.iterate(sm)
            b.set_math_mode(mtf_amd.MATH_REPLAY)
            dpf = -oracle.colpiv_qr_solve(Hf[0], gf[0])
            gs = np.sqrt(abs(np.trace(rec["H"]))) * (np.sqrt(abs(2 * rec["f"])) if am == L.AM_SSD else 1.0)
            # (i) against the low-noise oracle at the device's current state
            o_ssm6.set_state(b.get_state()[0]); trk6.update(); r6 = trk6.trace()[0]
            assert rel(ff[0], r6["f"]) < 1e-8, it
            assert rel(Hf[0], r6["H"]) < 2e-5, it
            assert np.linalg.norm(gf[0] - r6["g"]) < 2e-5 * max(np.linalg.norm(r6["g"]), gs), it
            # measured, not just bounded: the distances of this case go to the parity record (profiles/r04_parity_record.jsonl)
            fast_vs_6["H"] = max(fast_vs_6["H"], rel(Hf[0], r6["H"])); fast_vs_8["H"] = max(fast_vs_8["H"], rel(Hf[0], rec["H"]))
            fast_vs_6["g"] = max(fast_vs_6["g"], float(np.linalg.norm(gf[0] - r6["g"]) / max(np.linalg.norm(r6["g"]), gs)))
            fast_vs_8["g"] = max(fast_vs_8["g"], float(np.linalg.norm(gf[0] - rec["g"]) / max(np.linalg.norm(rec["g"]), gs)))
            if it <= 1:
                fast_vs_6["dp"] = max(fast_vs_6["dp"], rel(dpf, r6["dp"])); fast_vs_8["dp"] = max(fast_vs_8["dp"], rel(dpf, rec["dp"]))
            if it <= 1:
                # plain relative while g, dp are far from zero -- MI included since r05: its pass 2 takes the non-chained route's own
                # rounded steps (mi_finish, NONCH) instead of running both routes through the chained form (r04: H 4.9e-6, dp 2.3e-5 on
                # ESM + MI chained_warp = 0; now 1.6e-7 / 1.9e-6, profiles/r05_parity_record.jsonl)
                if am != L.AM_MI:   # (MI's update moves by 1.5e-5 .. 2.8e-5 between the 1e-8 and the 1e-6 oracle: test_mi_update_noise_floor)
                    assert rel(gf[0], r6["g"]) < 2e-5 and rel(dpf, r6["dp"]) < 2e-5, it
                assert rel(gf[0], rec["g"]) < 1e-5 and rel(dpf, rec["dp"]) < dp_tol, it
            # (ii) against the reference's own arithmetic: one set of bounds for SSD, NCC and MI
            tol_f, tol_H, tol_g = FOLLOW_BOUNDS["fast"]
            assert rel(ff[0], rec["f"]) < tol_f, it
            assert rel(Hf[0], rec["H"]) < tol_H, it
            assert np.linalg.norm(gf[0] - rec["g"]) < tol_g * max(np.linalg.norm(rec["g"]), gs), it
            cf = b.apply_warp_to_corners(corners[None], dpf[None])[0]
            cr = b.apply_warp_to_corners(corners[None], rec["dp"][None])[0]
            # (later passes: dp itself goes to zero, so either its relative error or what it does to the corners)
            assert rel(dpf, rec["dp"]) < dp_tol or np.abs(cf - cr).max() < DP_CORNER_PX, it
        f, g, H = b.iterate(sm)
        dp = -oracle.colpiv_qr_solve(H[0], g[0])
        if it <= 1 and not tight:    # plain relative errors while g and dp are far from zero (north_star's literal wording)
            assert rel(g[0], rec["g"]) < 1e-5, it
            assert rel(dp, rec["dp"]) < dp_tol, it
        # scale of g: Cauchy-Schwarz ||J|| ||r|| for SSD; for NCC the gradient vectors have norm <= 2 / b, so ||Jc|| ~ sqrt(|tr H|)
        g_scale = np.sqrt(abs(np.trace(rec["H"]))) * (np.sqrt(abs(2 * rec["f"])) if am == L.AM_SSD else 1.0)
        tol_f, tol_H, tol_g = FOLLOW_BOUNDS[grid]
        if tight:
            assert rel(f[0], rec["f"]) < tol_f, it
            assert rel(H[0], rec["H"]) < tol_H, it
            assert np.linalg.norm(g[0] - rec["g"]) < tol_g * max(np.linalg.norm(rec["g"]), g_scale), it
            assert rel(dp, rec["dp"]) < 1e-6 or np.abs(dp - rec["dp"]).max() < 1e-12, it
        else:
            assert rel(f[0], rec["f"]) < tol_f, it
            assert rel(H[0], rec["H"]) < tol_H, it
            assert np.linalg.norm(g[0] - rec["g"]) < tol_g * max(np.linalg.norm(rec["g"]), g_scale), it
            c_gpu = b.apply_warp_to_corners(corners[None], dp[None])[0]
            c_ref = b.apply_warp_to_corners(corners[None], rec["dp"][None])[0]
            assert rel(dp, rec["dp"]) < dp_tol or np.abs(c_gpu - c_ref).max() < DP_CORNER_PX, it
        # follow the oracle's trajectory so that every iteration is compared on identical inputs
        dp = rec["dp"]
        if sm_kind == L.SM_ICLK:
            dp = b.invert_state(dp[None])[0]
        b.compositional_update(dp[None])
        np.testing.assert_allclose(b.get_corners()[0], rec["corners"], rtol=0, atol=1e-9)
    if not materialize and not tight:
        import conftest
        conftest.PARITY_RECORD.append(dict(test="fused_iterate_fast_math", case="%s+%s+%s %dx%d %s" % (
            {0: "ESM", 1: "FCLK", 2: "ICLK"}[sm_kind], {0: "SSD", 1: "NCC", 2: "MI"}[am], "hom" if ssm == 0 else "aff", res, res,
            " ".join("%s=%s" % kv for kv in sorted(extra.items()))), iterations=len(trace),
            fast_vs_oracle_grad_eps_1e6=fast_vs_6, fast_vs_oracle_grad_eps_1e8=fast_vs_8,
            note="dp over the first two iterations (plain relative), H and g over all"))
    if materialize and sm_kind != L.SM_ICLK:
        assert b.read(L.BUF_JT).shape == (1, res * res, b.S)
    if not materialize and am != L.AM_MI:   # (the fused MI iteration always materialises It / Jt: its second pass reads them)
        with pytest.raises(mtf_amd.LogicError):
            b.read(L.BUF_IT)


@pytest.mark.parametrize("extra", [dict(), dict(hess_type=5, jac_type=0), dict(hess_type=2)], ids=["default", "std", "ht2"])
@pytest.mark.parametrize("sm_kind,ssm", [(L.SM_ESM, L.SSM_HOMOGRAPHY), (L.SM_FCLK, L.SSM_AFFINE), (L.SM_ICLK, L.SSM_HOMOGRAPHY)])
def test_device_side_loop_ncc(oracle, gpu_ctx, frame, sm_kind, ssm, extra, parity_record):
    """the device-side loop with NCC: k_fused_ncc + the moment assembly and solve inside k_finish_track"""
    if sm_kind != L.SM_ESM and extra.get("hess_type") == 5:
        pytest.skip("ESM-only Hessian type")
    _device_loop(oracle, gpu_ctx, frame, sm_kind, ssm, L.AM_NCC, 100, extra, parity_record)   # > kIclkTrackMaxPix: not the one-launch kernel


@pytest.mark.parametrize("sm_kind,ssm,extra", [
    (L.SM_ESM, L.SSM_HOMOGRAPHY, dict()), (L.SM_ESM, L.SSM_AFFINE, dict(hess_type=4)), (L.SM_ESM, L.SSM_HOMOGRAPHY, dict(hess_type=3, jac_type=0)),
    (L.SM_ESM, L.SSM_AFFINE, dict(hess_type=0, jac_type=0)), (L.SM_FCLK, L.SSM_HOMOGRAPHY, dict()), (L.SM_FCLK, L.SSM_AFFINE, dict(hess_type=2)),
    (L.SM_ICLK, L.SSM_HOMOGRAPHY, dict()), (L.SM_ICLK, L.SSM_AFFINE, dict(hess_type=2)), (L.SM_ICLK, L.SSM_HOMOGRAPHY, dict(hess_type=1))],
    ids=lambda v: "_".join("%s%s" % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_device_side_loop_mi(oracle, gpu_ctx, frame, sm_kind, ssm, extra, parity_record):
    """mtfhip_batch_track with MI: the fused MI passes leave g and H on the device, k_finish_track_mi hands them to the same
    finish kernel (solve, compositional update, convergence test) -- every first-order type, against the oracle's trackers."""
    _device_loop(oracle, gpu_ctx, frame, sm_kind, ssm, L.AM_MI, 36, extra, parity_record)


@pytest.mark.parametrize("sm_kind,ssm", [(L.SM_ESM, L.SSM_HOMOGRAPHY), (L.SM_FCLK, L.SSM_HOMOGRAPHY),
                                         (L.SM_ICLK, L.SSM_AFFINE), (L.SM_ICLK, L.SSM_HOMOGRAPHY)])
def test_device_side_loop_matches_oracle_tracker(oracle, gpu_ctx, frame, sm_kind, ssm, parity_record):
    _device_loop(oracle, gpu_ctx, frame, sm_kind, ssm, L.AM_SSD, 40, dict(), parity_record)


@pytest.mark.parametrize("sm_kind,ssm,am,res", [(L.SM_ICLK, L.SSM_AFFINE, L.AM_NCC, 25), (L.SM_ICLK, L.SSM_HOMOGRAPHY, L.AM_SSD, 30)])
def test_device_side_loop_one_launch_grid_kernel(oracle, gpu_ctx, frame, sm_kind, ssm, am, res, parity_record):
    """the one-launch ICLK loop of the grid (k_iclk_track: config 3's patch tracker), iteration by iteration"""
    _device_loop(oracle, gpu_ctx, frame, sm_kind, ssm, am, res, dict(hess_type=0), parity_record)


def _trace_errors(tr, ref, am):
    """per-iteration errors of one device-loop record against one oracle record: H and dp plain relative, g relative to the larger
    of its own norm and its Cauchy-Schwarz scale (g cancels to ~0 at convergence)"""
    gs = np.sqrt(abs(np.trace(ref["H"]))) * (np.sqrt(abs(2 * ref["f"])) if am == L.AM_SSD else 1.0)
    return dict(H=rel(tr["H"], ref["H"]) if tr["has_H"] else 0.0,
                g=float(np.linalg.norm(tr["g"] - ref["g"]) / max(np.linalg.norm(ref["g"]), gs)),
                dp=rel(tr["dp"], ref["dp"]), f=rel(tr["f"], ref["f"]))


def _device_loop_per_iteration(oracle, gpu_ctx, frame, frame2, corners, sm_kind, ssm, am, res, params, record, case):
    """The device-side loop against the CPU trackers ITERATION BY ITERATION (mtfhip_batch_track_trace).
    (a) injected: every oracle iteration k is replayed as ONE pass of the device loop (the loop's own kernels: fused pass + finish,
        or the one-launch grid kernel) started from the oracle's state before k -- identical inputs, so H_k, g_k, dp_k compare
        directly: replay AND tolerance-mode arithmetic against the reference-parameter oracle (grad_eps 1e-8) within north_star's
        1e-5 (r04: the tolerance mode carries the reference's rounded finite-difference step, fd_step); its distance to the low-noise
        oracle (grad_eps 1e-6) is RECORDED per case (profiles/r04_parity_record.jsonl).
    (b) free running: the whole loop in one call, every pass compared with the oracle's own trajectory relative to the size of
        the first update (later updates shrink towards zero, so their plain relative error measures nothing)."""
    B = corners.shape[0]
    mi = am == L.AM_MI
    tol_dp = 5e-5 if mi else 1e-5   # MI: the oracle's own dp moves by 1.5e-5 .. 2.8e-5 under a one-ulp grid change (test_mi_update_noise_floor)
    sm1 = mtf_amd.sm_desc(sm_kind, materialize=0, **dict(params, max_iters=1, epsilon=-1.0))
    smN = mtf_amd.sm_desc(sm_kind, materialize=0, **params)
    traces = {}
    for eps in (1e-8, 1e-6):
        traces[eps] = []
        for t in range(B):
            o_ssm = oracle.SSM(ssm, res, res); o_am = oracle.AM(am, res, res, grad_eps=eps); o_am.set_curr_img(frame)
            trk = oracle.Tracker(sm_kind, o_am, o_ssm, **params)
            trk.initialize(corners[t]); o_am.set_curr_img(frame2); trk.update()
            traces[eps].append(trk.trace())
    fresh = []   # per target a single-iteration grad_eps = 1e-7 tracker that can be started from any state
    for t in range(B):
        o_ssm = oracle.SSM(ssm, res, res); o_am = oracle.AM(am, res, res, grad_eps=1e-7); o_am.set_curr_img(frame)
        trk = oracle.Tracker(sm_kind, o_am, o_ssm, **dict(params, max_iters=1))
        trk.initialize(corners[t]); o_am.set_curr_img(frame2)
        fresh.append((trk, o_ssm, o_am))
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, am, ssm, res, res, B)
    b.set_corners(corners); b.init_template(smN)
    gpu_ctx.set_image(frame2)
    b.track_trace(params["max_iters"])
    worst = {}
    for mode, name, eps_ref in ((mtf_amd.MATH_REPLAY, "replay", 1e-8), (mtf_amd.MATH_FAST, "fast", 1e-8)):
        b.set_math_mode(mode)
        # ---- (a) injected single passes along the oracle's trajectory
        ref = traces[eps_ref]
        b.set_corners(corners)
        n_max = max(len(tr) for tr in ref)
        w = dict(H=0.0, g=0.0, dp=0.0, f=0.0); w8 = dict(H=0.0, g=0.0, dp=0.0, f=0.0)
        for k in range(n_max):
            st_k = b.get_state().copy()
            n_it, _ = b.track(sm1)
            assert np.all(n_it == 1)
            recs = b.read_track_trace(n_it)
            dp_next = np.zeros((B, b.S))
            for t in range(B):
                if k >= len(ref[t]):
                    continue
                e = _trace_errors(recs[t][0], ref[t][k], am)
                # the corners the two updates produce from the same state (pixels): what the update is FOR -- near convergence g has
                # cancelled to ~0 and dp = -H^-1 g inherits the relative error of that remainder, not of the kernels
                e["corners_px"] = float(np.abs(recs[t][0]["corners"] - ref[t][k]["corners"]).max())
                big = np.linalg.norm(ref[t][k]["dp"]) >= 1e-3 * np.linalg.norm(ref[t][0]["dp"])
                ok = (e["dp"] < tol_dp or e["corners_px"] < 1e-6) and e["H"] < 1e-5 and e["g"] < 1e-5 and e["f"] < 1e-8 and (mi or not big or e["dp"] < 3 * tol_dp)
                if not ok and name == "fast":
                    # The low-noise oracle is not always a clean limit: a grad_eps = 1e-6 step straddles a texel edge when a sample lies
                    # within 1e-6 of it -- 4 N eps = 4 % of the iterations at 100 x 100 -- and that one pixel's mixed slope is a 1e-5
                    # change of H (found on FCLK+NCC+Affine: y = 231.99999989; the 1e-8 oracle and the closed form agree there); and
                    # MI's Std Hessians are ill-conditioned enough that dp moves by 1e-4 between two oracles (test_mi_update_noise_floor).
                    # Such a record is judged against the same restatement with grad_eps = 1e-7 at the same state as well, and against
                    # the disagreement of the two oracles with each other: the reference's own sensitivity at this state.
                    o7 = fresh[t]
                    o7[1].set_state(st_k[t]); o7[0].update(); r7 = o7[0].trace()[0]
                    e7 = _trace_errors(recs[t][0], r7, am)
                    e7["corners_px"] = float(np.abs(recs[t][0]["corners"] - r7["corners"]).max())
                    spread = dict(H=rel(r7["H"], ref[t][k]["H"]), dp=rel(r7["dp"], ref[t][k]["dp"]), corners_px=float(np.abs(r7["corners"] - ref[t][k]["corners"]).max()))
                    e = {q: min(e[q], e7[q]) for q in e}
                    worst["fast_records_judged_against_two_oracles"] = worst.get("fast_records_judged_against_two_oracles", 0) + 1
                    worst["oracle_1e-6_vs_1e-7_spread"] = {q: max(worst.get("oracle_1e-6_vs_1e-7_spread", {}).get(q, 0.0), spread[q]) for q in spread}
                    ok = (e["dp"] < max(tol_dp, 4 * spread["dp"]) or e["corners_px"] < max(1e-6, 4 * spread["corners_px"])) and \
                        e["H"] < max(1e-5, 4 * spread["H"]) and e["g"] < 1e-5 and e["f"] < 1e-8
                for q in w:
                    if q != "dp" or big:
                        w[q] = max(w[q], e[q])
                w["corners_px"] = max(w.get("corners_px", 0.0), e["corners_px"])
                assert ok, (name, t, k, e)
                if name == "fast" and k < len(traces[1e-6][t]) and k <= 1:
                    # the two oracles share a trajectory only while their own difference is small: the first iterations
                    e8 = _trace_errors(recs[t][0], traces[1e-6][t][k], am)
                    for q in w8:
                        w8[q] = max(w8[q], e8[q])
                dp = ref[t][k]["dp"]
                dp_next[t] = dp
            # back to the state before the pass, then the ORACLE's update (ICLK: its inverse, NT/ICLK.cc:266-267)
            b.set_state(st_k)
            upd = dp_next if sm_kind != L.SM_ICLK else b.invert_state(dp_next)
            b.compositional_update(upd)
        worst[name] = w
        if name == "fast":
            worst["fast_vs_grad_eps_1e-6_first_two_iterations"] = w8
        # ---- (b) the free-running loop
        b.set_corners(corners)
        n_it, final = b.track(smN)
        recs = b.read_track_trace(n_it)
        wf = 0.0
        for t in range(B):
            o = ref[t]
            assert abs(int(n_it[t]) - len(o)) <= 1
            scale = np.linalg.norm(o[0]["dp"])
            for k in range(min(len(o), len(recs[t]))):
                d = float(np.linalg.norm(recs[t][k]["dp"] - o[k]["dp"]) / scale)
                wf = max(wf, d)
                # (the two oracles' own trajectories differ from each other: an update is not asked to be closer to one of them than
                # four times that -- MI's Std Hessians put it at 1e-4 of the first update)
                oa, ob = traces[1e-8][t], traces[1e-6][t]
                sp = float(np.linalg.norm(oa[k]["dp"] - ob[k]["dp"]) / scale) if k < min(len(oa), len(ob)) else 0.0
                assert d < max(2 * tol_dp, 4 * sp), (name, t, k, d, sp)
                spc = float(np.abs(oa[k]["corners"] - ob[k]["corners"]).max()) if k < min(len(oa), len(ob)) else 0.0
                np.testing.assert_allclose(recs[t][k]["corners"], o[k]["corners"], rtol=0, atol=max(2e-4, 4 * spc))
        worst[name + "_free_running_dp_over_first_update"] = wf
    b.track_trace(0)
    b.close()
    record.append(dict(test="device_loop_per_iteration", case=case, targets=B, **worst))


def _device_loop(oracle, gpu_ctx, frame, sm_kind, ssm, am, res, extra, record=None):
    """mtfhip_batch_track (solve + update + convergence test on the device) lands on the oracle's
    final corners and iteration count, for several independent targets in one batch -- and follows the oracle's trace iteration
    by iteration (_device_loop_per_iteration)."""
    rng = np.random.default_rng(23)
    B = 5
    centres = [(150.0 + 60 * i, 200.0 + 25 * i) for i in range(B)]
    p_true = synth.random_small_homography(rng, 0.4)
    frame2 = synth.warp_frame(frame, p_true, (256.0, 256.0))
    corners = np.stack([synth.square_corners(cx, cy, 70) for cx, cy in centres])
    params = dict(leven_marq=0, max_iters=25, epsilon=1e-4)
    params.update(extra)
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, am, ssm, res, res, B)
    b.set_corners(corners)
    sm = mtf_amd.sm_desc(sm_kind, materialize=0, **params)
    b.init_template(sm)
    gpu_ctx.set_image(frame2)
    n_it, final = b.track(sm)
    for t in range(B):
        o_ssm = oracle.SSM(ssm, res, res)
        o_am = oracle.AM(am, res, res)
        o_am.set_curr_img(frame)
        trk = oracle.Tracker(sm_kind, o_am, o_ssm, **params)
        trk.initialize(corners[t])
        o_am.set_curr_img(frame2)
        iters = trk.update()
        np.testing.assert_allclose(final[t], trk.get_region(), rtol=0, atol=LOOP_CORNER_PX)
        assert abs(int(n_it[t]) - iters) <= 1
    # target chunking (all iterations of 2 targets, then the next 2, ...) changes the schedule, not the result
    import os
    os.environ["MTFHIP_TRACK_CHUNK_PX"] = str(2 * res * res)
    try:
        gpu_ctx.set_image(frame); b.set_corners(corners); b.init_template(sm); gpu_ctx.set_image(frame2)
        n_it2, final2 = b.track(sm)
    finally:
        del os.environ["MTFHIP_TRACK_CHUNK_PX"]
    np.testing.assert_allclose(final2, final, rtol=0, atol=1e-7)
    assert np.array_equal(n_it2, n_it)
    b.close()
    if record is not None:
        case = "%s+%s+%s %dx%d %s" % ({0: "ESM", 1: "FCLK", 2: "ICLK"}[sm_kind], {0: "SSD", 1: "NCC", 2: "MI"}[am], "hom" if ssm == 0 else "aff", res, res,
                                      " ".join("%s=%s" % kv for kv in sorted(extra.items())))
        _device_loop_per_iteration(oracle, gpu_ctx, frame, frame2, corners[:3], sm_kind, ssm, am, res, params, record, case)


@pytest.mark.parametrize("am", [L.AM_SSD, L.AM_NCC, L.AM_MI])
def test_pf_candidate_scores(oracle, gpu_ctx, frame, am):
    """setState -> updatePixVals -> updateSimilarity -> getLikelihood per candidate (PF.cc:247-262) for all three appearance
    models (MI: the histogram pass over the candidate axis, MI.cc:346-387)"""
    rng = np.random.default_rng(31)
    corners = synth.square_corners(256, 256, 100)
    o_am, o_ssm, b = make_pair(oracle, gpu_ctx, frame, am, L.SSM_HOMOGRAPHY, 50, corners)
    pts0 = o_ssm.get("curr_pts")
    o_am.initialize_pix_vals(pts0); o_am.initialize_similarity()
    b.initialize_pix_vals(); b.initialize_similarity()
    states = synth.pf_candidate_states(rng, 300)
    lik_o, sim_o = oracle.pf_score(o_am, o_ssm, states)
    lik, sim = b.score_candidates(states, want_similarity=True)
    np.testing.assert_allclose(sim, sim_o, rtol=1e-9)
    np.testing.assert_allclose(lik, lik_o, rtol=1e-9 if am != L.AM_MI else 1e-7)   # (MI: exp(-alpha (1 / f - 1)^2) amplifies f's 1e-12)


@pytest.mark.parametrize("am,ssm", [(L.AM_SSD, L.SSM_HOMOGRAPHY), (L.AM_NCC, L.SSM_HOMOGRAPHY), (L.AM_SSD, L.SSM_AFFINE)])
def test_pf_candidate_scores_at_the_frame_border(oracle, gpu_ctx, frame, am, ssm):
    """The scorer skips the per-sample border test for a workgroup whose four candidates have their warped template corners inside
    the frame (PfScoreArgs::hull): candidates that sit well inside, that touch the border, that straddle it and that lie mostly
    outside, mixed so that workgroups of every kind occur -- all against the oracle (constant border 128, imgUtils.h:91-113), in both
    arithmetic modes; and a projective candidate whose denominator changes sign over the template (no fast path for it)."""
    h, w = frame.shape
    corners = synth.square_corners(60.0, 58.0, 100)                      # 10 .. 110: ten pixels from the left / top border
    o_am, o_ssm, b = make_pair(oracle, gpu_ctx, frame, am, ssm, 50, corners)
    pts0 = o_ssm.get("curr_pts")
    o_am.initialize_pix_vals(pts0); o_am.initialize_similarity()
    b.initialize_pix_vals(); b.initialize_similarity()
    rng = np.random.default_rng(5)
    S = 8 if ssm == L.SSM_HOMOGRAPHY else 6
    n = 240
    states = np.zeros((n, S))
    tx, ty = (2, 5) if ssm == L.SSM_HOMOGRAPHY else (0, 1)
    shift = np.concatenate([rng.uniform(-9.9, 5.0, n // 4), rng.uniform(-10.5, -9.5, n // 4), rng.uniform(-60.0, -10.0, n // 4), rng.uniform(-140.0, 20.0, n // 4)])
    states[:, tx] = rng.permutation(shift)
    states[:, ty] = rng.permutation(shift) * 0.7
    if ssm == L.SSM_HOMOGRAPHY:
        states[:, [0, 1, 3, 4]] = rng.normal(0, 0.01, (n, 4))
        states[:, 6:8] = rng.normal(0, 1e-5, (n, 2))
        states[7, 6] = -1.0 / 60.0                                          # the denominator 1 + p6 x crosses zero inside the template
    else:
        states[:, 2:6] = rng.normal(0, 0.01, (n, 4))
    lik_o, sim_o = oracle.pf_score(o_am, o_ssm, states)
    for mode in (L.MATH_FAST, L.MATH_REPLAY):
        b.set_math_mode(mode)
        lik, sim = b.score_candidates(states, want_similarity=True)
        keep = np.isfinite(sim_o)
        if ssm == L.SSM_HOMOGRAPHY:
            keep[7] = False      # (samples next to the pole are ill-conditioned in any arithmetic: scored, not compared)
        np.testing.assert_allclose(sim[keep], sim_o[keep], rtol=1e-9, err_msg="mode %d" % mode)
        np.testing.assert_allclose(lik[keep], lik_o[keep], rtol=1e-9, atol=1e-300)


@pytest.mark.parametrize("via", ["write", "device_ptr"])
def test_pf_candidate_scores_with_a_caller_supplied_grid(oracle, gpu_ctx, frame, via):
    """r04 advisor: a caller that replaces INIT_PTS (mtfhip_batch_write, or a raw device pointer) must not leave the scorer trusting
    the corners set_corners saw as the hull of the sample points -- here the corners are a 20 px square well inside the frame while
    the grid that is actually sampled spans 100 px and crosses the border under the candidates' shifts.  Against the oracle, which
    samples the same big grid."""
    small = synth.square_corners(60.0, 58.0, 20)
    big = synth.square_corners(60.0, 58.0, 100)
    o_am, o_ssm, b = make_pair(oracle, gpu_ctx, frame, L.AM_SSD, L.SSM_AFFINE, 50, big)
    b.set_corners(small[None])
    grid = o_ssm.get("init_pts").reshape(-1, 2).T          # the oracle's SSM holds the big grid
    if via == "write":
        b.write(L.BUF_INIT_PTS, grid[None])
    else:
        import torch
        ptr = b.device_ptr(L.BUF_INIT_PTS)
        host = np.ascontiguousarray(grid.T)                # (x, y) interleaved
        t = torch.from_numpy(host).to("cuda:0")
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(ctypes.c_void_p(ptr), ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(host.nbytes), 3) == 0   # device to device
        torch.cuda.synchronize()
    o_am.initialize_pix_vals(o_ssm.get("curr_pts")); o_am.initialize_similarity()
    b.initialize_pix_vals(grid[None]); b.initialize_similarity()
    rng = np.random.default_rng(6)
    n = 64
    states = np.zeros((n, 6))
    states[:, 0] = rng.uniform(-30.0, -5.0, n)      # the small square stays inside (50 - 30 > 0), the big grid (10 .. 110) does not
    states[:, 1] = rng.uniform(-30.0, -5.0, n)
    lik_o, sim_o = oracle.pf_score(o_am, o_ssm, states)
    for mode in (L.MATH_FAST, L.MATH_REPLAY):
        b.set_math_mode(mode)
        lik, sim = b.score_candidates(states, want_similarity=True)
        np.testing.assert_allclose(sim, sim_o, rtol=1e-9, err_msg="mode %d" % mode)
        np.testing.assert_allclose(lik, lik_o, rtol=1e-9, atol=1e-300)


def test_border_and_integer_coordinate_cases(oracle, gpu_ctx, frame):
    """Constant border (128) outside the image and at the last row/column, and the dx == 0 branch at
    exact integer coordinates (imgUtils.h:96-108) -- samples and both gradient flavours."""
    h, w = frame.shape
    xs = np.array([-3.0, -1e-9, 0.0, 0.5, 10.0, 10.0 + 1e-8, w - 1.0, w - 1.0 + 1e-9, w - 0.5, w + 2.0, 37.25, 64.0])
    ys = np.array([5.0, 5.0, 0.0, 0.0, 20.0, 20.0, 30.0, 30.0, h - 1.0, 7.0, h - 1.0, 64.0])
    n = 16 * 16
    X = np.resize(xs, n); Y = np.resize(ys, n)
    pts = np.stack([X, Y])
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, 16, 16, 1)
    b.set_corners(synth.square_corners(100, 100, 16)[None])
    b.update_pix_vals(pts[None])
    flat = np.ascontiguousarray(pts.T.ravel())
    assert np.array_equal(b.read(L.BUF_IT)[0], oracle.get_pix_vals(frame, flat))
    b.update_pix_grad(pts[None])
    assert np.array_equal(b.read(L.BUF_DIT_DX)[0], oracle.get_img_grad(frame, flat).reshape(2, -1).T)


def test_error_behaviour(gpu_ctx, frame):
    with pytest.raises(mtf_amd.InvalidArgument):
        mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, 0, 10, 1)   # ImageBase.cc:33-35
    b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, 10, 10, 1)
    with pytest.raises(mtf_amd.LogicError):
        b.set_state(np.zeros((1, 8)))
    with pytest.raises(mtf_amd.InvalidArgument):
        gpu_ctx.set_image(np.zeros((8, 8), dtype=np.uint8))             # ImageBase.cc:49-54
    bn = mtf_amd.Batch(gpu_ctx, L.AM_NCC, L.SSM_AFFINE, 10, 10, 1)
    bn.set_corners(synth.square_corners(50, 50, 10)[None])


@pytest.mark.parametrize("am", [L.AM_SSD, L.AM_NCC])
def test_nn_dataset_rows(oracle, gpu_ctx, frame, am):
    """NN-SM dataset generation (NT/NN.cc:131-191): per sample, invert the perturbation, compose, sample,
    updateDistFeat -- rows of the feature matrix against the oracle's setState + updatePixVals."""
    rng = np.random.default_rng(53)
    corners = synth.square_corners(256, 240, 80)
    o_am, o_ssm, b = make_pair(oracle, gpu_ctx, frame, am, L.SSM_HOMOGRAPHY, 32, corners)
    o_am.initialize_pix_vals(o_ssm.get("init_pts"))
    b.initialize_pix_vals()
    perts = synth.pf_candidate_states(rng, 40)
    states = np.stack([o_ssm.invert_state(p) for p in perts])      # identity o inverse(perturbation)
    np.testing.assert_allclose(b.invert_state(perts[:1])[0], states[0], rtol=1e-12, atol=1e-15)
    feats = b.sample_candidates(states)
    assert feats.shape == (40, 32 * 32)
    for c in range(0, 40, 7):
        o_ssm.set_state(states[c])
        o_am.update_pix_vals(o_ssm.get("curr_pts"))
        It = o_am.get("It")
        want = It if am == L.AM_SSD else (It - It.mean()) / np.linalg.norm(It - It.mean())
        np.testing.assert_allclose(feats[c], want, rtol=1e-10, atol=1e-9)


# ------------------------------------------------------------------ second-order Hessians (sec_ord_hess)
@pytest.mark.parametrize("ssm", [L.SSM_HOMOGRAPHY, L.SSM_AFFINE])
@pytest.mark.parametrize("am", [L.AM_SSD, L.AM_NCC, L.AM_MI])
def test_second_order_interface(oracle, gpu_ctx, frame, frame2, am, ssm):
    """hess_pts, image Hessians (both overloads), the four SSM pixel Hessians and the AM's second-order Hessians
    against the oracle, call by call (NT/ESM.cc:406-432, Homography.cc:360-801, SSDBase.cc:313-415, NCC.cc:391-410,
    MI.cc:659-733)."""
    rng = np.random.default_rng(71)
    res = 24
    corners = synth.square_corners(256, 250, 70) + rng.uniform(-2, 2, size=(2, 4))
    o_am, o_ssm, b = make_pair(oracle, gpu_ctx, frame, am, ssm, res, corners)
    S, N = b.S, b.N
    # template side
    pts0 = o_ssm.get("curr_pts")
    o_am.initialize_pix_vals(pts0); o_am.initialize_pix_grad_pts(pts0); o_am.initialize_pix_hess_pts(pts0)
    b.initialize_pix_vals(); b.initialize_pix_grad(); b.initialize_pix_hess()
    scale = np.abs(o_am.get("d2I0_dx2")).max()
    np.testing.assert_allclose(b.read(L.BUF_D2I0_DX2)[0].reshape(-1), o_am.get("d2I0_dx2"), rtol=0, atol=1e-9 * scale)
    o_am.initialize_similarity(); o_am.initialize_grad(); o_am.initialize_hess()
    b.initialize_similarity(); b.initialize_grad(); b.initialize_hess()
    J0_o = o_ssm.cmpt_warped_pix_jacobian(o_am.get("dI0_dx"))
    b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DI0_DX, L.BUF_J0)
    D0_o = o_ssm.cmpt_warped_pix_hessian(o_am.get("d2I0_dx2"), o_am.get("dI0_dx"))
    b.cmpt_pix_hessian(L.JAC_WARPED, L.BUF_D2I0_DX2, L.BUF_DI0_DX, L.BUF_D2I0_DP2)
    # current side: a warped state on the second frame
    p = (synth.random_small_homography(rng) if ssm == L.SSM_HOMOGRAPHY else
         rng.uniform(-1, 1, 6) * [2, 2, .02, .02, .02, .02])
    o_ssm.set_state(p); b.set_state(p[None])
    o_am.set_curr_img(frame2); gpu_ctx.set_image(frame2)
    pts = o_ssm.get("curr_pts")
    o_am.update_pix_vals(pts); o_am.update_pix_grad_pts(pts)
    b.update_pix_vals(); b.update_pix_grad()
    # hess_pts + warped-image Hessian (non-chained route), device-resident and host-upload forms
    o_ssm.update_hess_pts(1.0); b.update_hess_pts()
    hp_o = o_ssm.get("hess_pts").reshape(N, 16)
    np.testing.assert_allclose(b.read(L.BUF_HESS_PTS)[0], hp_o, rtol=0, atol=1e-9)
    o_am.update_pix_hess_warped(pts, hp_o)
    b.update_pix_hess(warped=True)
    dev_res = b.read(L.BUF_D2IT_DX2)[0].reshape(-1).copy()
    np.testing.assert_allclose(dev_res, o_am.get("d2It_dx2"), rtol=0, atol=1e-9 * scale)
    b.update_pix_hess(pts=pts.reshape(1, N, 2).transpose(0, 2, 1), hess_pts=hp_o[None], warped=True)
    np.testing.assert_allclose(b.read(L.BUF_D2IT_DX2)[0].reshape(-1), dev_res, rtol=0, atol=1e-9 * scale)
    # chained route
    o_am.update_pix_hess_pts(pts); b.update_pix_hess()
    np.testing.assert_allclose(b.read(L.BUF_D2IT_DX2)[0].reshape(-1), o_am.get("d2It_dx2"), rtol=0, atol=1e-9 * scale)
    ph, g = o_am.get("d2It_dx2"), o_am.get("dIt_dx")
    for variant, name in ((L.JAC_INIT, "init_pix"), (L.JAC_PIX, "pix"), (L.JAC_WARPED, "warped_pix"), (L.JAC_APPROX, "approx_pix")):
        want = getattr(o_ssm, "cmpt_%s_hessian" % name)(ph, g)
        if want is None:        # Affine: cmptPixHessian / cmptApproxPixHessian are not implemented in the reference
            with pytest.raises(mtf_amd.FunctionNotImplemented):
                b.cmpt_pix_hessian(variant, L.BUF_D2IT_DX2, L.BUF_DIT_DX, L.BUF_D2IT_DP2)
            continue
        b.cmpt_pix_hessian(variant, L.BUF_D2IT_DX2, L.BUF_DIT_DX, L.BUF_D2IT_DP2)
        got = b.read(L.BUF_D2IT_DP2)[0]
        # the third-order terms multiply the FD gradient (5e-6 absolute jitter between the two grids) by x^2 ~ 6e4
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6 * np.abs(want).max(), err_msg=name)
    # fed the oracle's own gradient and image Hessian the kernels agree to round-off (same expressions, same order)
    b.write(L.BUF_DIT_DX, g.reshape(1, 2, N).transpose(0, 2, 1)); b.write(L.BUF_D2IT_DX2, ph[None])
    for variant, name in ((L.JAC_INIT, "init_pix"), (L.JAC_WARPED, "warped_pix")):
        want = getattr(o_ssm, "cmpt_%s_hessian" % name)(ph, g)
        b.cmpt_pix_hessian(variant, L.BUF_D2IT_DX2, L.BUF_DIT_DX, L.BUF_D2IT_DP2)
        got = b.read(L.BUF_D2IT_DP2)[0]
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-11 * np.abs(want).max(), err_msg=name + " (oracle-fed)")
    if ssm == L.SSM_HOMOGRAPHY:     # the reference's partial mirroring: (6,5) / (7,5) differ from (5,6) / (5,7)
        assert np.abs(got[:, 6, 5] - got[:, 5, 6]).max() > 0
    # second-order AM Hessians on (J0, D0) / (Jt, Dt)
    Jt_o = o_ssm.cmpt_warped_pix_jacobian(g)
    Dt_o = o_ssm.cmpt_warped_pix_hessian(ph, g)
    b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DIT_DX, L.BUF_JT)
    b.cmpt_pix_hessian(L.JAC_WARPED, L.BUF_D2IT_DX2, L.BUF_DIT_DX, L.BUF_D2IT_DP2)
    o_am.update_similarity(False); o_am.update_curr_grad(); o_am.update_init_grad()
    b.update_similarity(False); b.update_curr_grad(); b.update_init_grad()

    def close(got, want, what):
        # device grid vs oracle grid: the 1e-8-step FD gradients inside J carry ~5e-6 absolute jitter,
        # so H agrees to the 1e-5 budget of SURVEY.md 8(d), not to round-off
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6 * np.abs(want).max(), err_msg=what)
    close(b.cmpt_init_hessian2()[0], o_am.cmpt_init_hessian2(J0_o, D0_o), "init2")
    close(b.cmpt_curr_hessian2()[0], o_am.cmpt_curr_hessian2(Jt_o, Dt_o), "curr2")
    close(b.cmpt_sum_of_hessians2()[0], o_am.cmpt_sum_of_hessians2(J0_o, Jt_o, D0_o, Dt_o), "sum2")
    want_self = o_am.cmpt_self_hessian2(Jt_o, Dt_o)
    if want_self is None:
        with pytest.raises(mtf_amd.FunctionNotImplemented):
            b.cmpt_self_hessian2()
    else:
        close(b.cmpt_self_hessian2()[0], want_self, "self2")
    b.mean_pix_hessian()
    np.testing.assert_allclose(b.read(L.BUF_D2IM_DP2)[0], (D0_o + Dt_o) / 2.0, rtol=1e-5, atol=1e-6 * np.abs(D0_o).max())


@pytest.mark.parametrize("shape", ["square", "quad"])
@pytest.mark.parametrize("sm_kind,extra", [(L.SM_ESM, dict()), (L.SM_ESM, dict(chained_warp=0, hess_type=0)),
                                           (L.SM_FCLK, dict(hess_type=0)), (L.SM_ICLK, dict())])
def test_set_region_follows_the_search_method(oracle, gpu_ctx, frame, frame2, sm_kind, extra, shape):
    """nt::ESM / FCLK / ICLK::setRegion (NT/ESM.cc:148-168, NT/FCLK.cc:360-376, NT/ICLK.cc:131-157) between frames, to a
    DIFFERENT region: ESM (and FCLK / InitialSelf) refresh init_pix_jacobian and the constant Hessian on the new grid, ICLK
    keeps its template Jacobian.  The fused kernel rebuilds J0's rows from dI0_dx (or reads them back with
    MTFHIP_J0_RECOMPUTE=0): both must give the oracle's g and H, bit-identical to each other."""
    import os
    rng = np.random.default_rng(61)
    res = 30
    c0 = CORNER_SETS[shape](rng)
    c1 = c0 + np.array([[3.3], [-2.1]]) + rng.uniform(-1.5, 1.5, size=(2, 4)) * (shape == "quad")
    params = dict(leven_marq=0, max_iters=1, epsilon=-1.0)
    params.update(extra)
    o_am, o_ssm, b = make_pair(oracle, gpu_ctx, frame, L.AM_SSD, L.SSM_HOMOGRAPHY, res, c0)
    trk = oracle.Tracker(sm_kind, o_am, o_ssm, **params)
    trk.initialize(c0)
    o_am.set_curr_img(frame2)
    trk.set_region(c1)
    trk.update()
    rec = trk.trace()[0]
    results = []
    for env in ("1", "0"):
        os.environ["MTFHIP_J0_RECOMPUTE"] = env
        try:
            gpu_ctx.set_image(frame)
            bb = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, res, res, 1)
            bb.set_corners(c0[None])
            bb.set_math_mode(mtf_amd.MATH_REPLAY)   # the bit-for-bit comparison below is a statement about the replay arithmetic
            sm = mtf_amd.sm_desc(sm_kind, materialize=0, **params)
            bb.init_template(sm)
            gpu_ctx.set_image(frame2)
            bb.set_region(c1[None], sm)
            f, g, H = bb.iterate(sm)
        finally:
            del os.environ["MTFHIP_J0_RECOMPUTE"]
        assert rel(f[0], rec["f"]) < 1e-8
        assert rel(H[0], rec["H"]) < 1e-5
        gs = max(np.linalg.norm(rec["g"]), np.sqrt(abs(np.trace(rec["H"])) * abs(2 * rec["f"])))
        assert np.linalg.norm(g[0] - rec["g"]) < 1e-5 * gs
        results.append((f.copy(), g.copy(), H.copy()))
        bb.close()
    for x, y in zip(results[0], results[1]):
        assert np.array_equal(x, y)           # rebuilt rows == stored rows, bit for bit


def _lazy_batch(gpu_ctx, frame, ssm, res, corners, lazy, monkeypatch, am=L.AM_SSD):
    monkeypatch.setenv("MTFHIP_LAZY", "1" if lazy else "0")   # read when the batch is created
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, am, ssm, res, res, 1)
    b.set_corners(corners[None])
    b.initialize_pix_vals(); b.initialize_pix_grad()
    b.initialize_similarity(); b.initialize_grad(); b.initialize_hess()
    b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DI0_DX, L.BUF_J0)
    return b


@pytest.mark.parametrize("am", [L.AM_SSD, L.AM_NCC, L.AM_MI])
@pytest.mark.parametrize("ssm", [L.SSM_HOMOGRAPHY, L.SSM_AFFINE])
@pytest.mark.parametrize("flow", ["esm", "esm_original", "fclk", "fclk_unchained", "iclk", "lm", "odd_order", "flush_only"])
def test_deferred_fusion_equals_call_by_call(gpu_ctx, frame, frame2, ssm, flow, am, monkeypatch):
    """The per-function entry points only record the pixel-level calls of an iteration and serve the ESM / FCLK / ICLK
    sequences with one fused launch (mtfhip_batch::Lazy).  Whatever the call pattern, buffers and results must be those
    of the call-by-call execution (MTFHIP_LAZY=0): per-pixel arrays bit for bit, the N-wide sums to summation order.
    NCC: the fused launch derives the scalars from raw moments instead of two passes, so everything that depends on them
    (f, g, H, and the gradient vectors df_dI re-derived afterwards) agrees to rounding, not to the bit.
    flush_only: no Jacobian is asked for, so nothing fuses and the flush replays every recorded call -- updateInitGrad
    included -- through the un-fused kernels in the recorded order: every array bit for bit, no tolerance."""
    rng = np.random.default_rng(11)
    corners = synth.square_corners(250, 260, 70) + rng.uniform(-3, 3, size=(2, 4))
    p = (synth.random_small_homography(rng) if ssm == L.SSM_HOMOGRAPHY else rng.uniform(-1, 1, 6) * [2, 2, .02, .02, .02, .02])
    S = 8 if ssm == L.SSM_HOMOGRAPHY else 6
    out = {}
    for lazy in (0, 1):
        b = _lazy_batch(gpu_ctx, frame, ssm, 40, corners, lazy, monkeypatch, am)
        gpu_ctx.set_image(frame2)
        gpu_ctx.timing(1); gpu_ctx.timing_reset()
        res = []
        state = p.copy()
        for it in range(3):
            b.set_state(state[None])
            b.update_pix_vals()
            b.update_similarity(False)
            if flow == "lm":
                res.append(b.get_similarity().copy())       # Levenberg-Marquardt reads f in the middle of the iteration
            if flow == "flush_only":
                b.update_init_grad(); b.update_curr_grad()
                res += [b.read(buf).copy() for buf in (L.BUF_IT, L.BUF_DF_DI0, L.BUF_DF_DIT)] + [b.get_similarity().copy()]
                state = state + 0.02 * (it + 1) * p
                continue
            if flow in ("esm", "esm_original", "lm"):
                b.update_pix_grad(); b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DIT_DX, L.BUF_JT)
                if flow == "esm_original": b.mean_jacobian()
                b.update_curr_grad(); b.update_init_grad()
                g = b.cmpt_curr_jacobian(L.BUF_JM) if flow == "esm_original" else b.cmpt_difference_of_jacobians()
                H = b.cmpt_curr_hessian(L.BUF_JM) if flow == "esm_original" else b.cmpt_sum_of_hessians()
            elif flow == "fclk":
                b.update_curr_grad()
                b.update_pix_grad(); b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DIT_DX, L.BUF_JT)
                g = b.cmpt_curr_jacobian(L.BUF_JT); H = b.cmpt_self_hessian(L.BUF_JT)
            elif flow == "fclk_unchained":
                b.update_curr_grad()
                b.update_grad_pts(); b.update_pix_grad(warped=True); b.cmpt_pix_jacobian(L.JAC_INIT, L.BUF_DIT_DX, L.BUF_JT)
                g = b.cmpt_curr_jacobian(L.BUF_JT); H = b.cmpt_curr_hessian(L.BUF_JT)
            elif flow == "iclk":
                b.update_init_grad()
                g = b.cmpt_init_jacobian(L.BUF_J0); H = b.cmpt_init_hessian(L.BUF_J0)
            else:   # a pattern no search method uses: Approx Jacobian, gradient before the sample, results read in between
                b.update_pix_grad()
                dit = b.read(L.BUF_DIT_DX).copy()
                b.cmpt_pix_jacobian(L.JAC_APPROX, L.BUF_DIT_DX, L.BUF_JT)
                b.update_curr_grad()
                g = b.cmpt_curr_jacobian(L.BUF_JT); H = b.cmpt_self_hessian(L.BUF_JT)
                res.append(dit)
            res += [g.copy(), H.copy(), b.get_similarity().copy()]
            # everything the interface exposes, read after the fact
            for buf in (L.BUF_IT, L.BUF_DF_DI0, L.BUF_DF_DIT) + (() if flow == "iclk" else (L.BUF_DIT_DX, L.BUF_JT)):
                res.append(b.read(buf).copy())
            if flow == "esm_original": res.append(b.read(L.BUF_JM).copy())
            state = state + 0.02 * (it + 1) * p
        _, n_fused = gpu_ctx.timing_get("fused_lk")
        gpu_ctx.timing(False)
        out[lazy] = (res, n_fused)
        b.close()
    direct, fused = out[0][0], out[1][0]
    assert out[0][1] == 0
    # one fused launch per iteration; with the LM pattern a lean one behind getSimilarity() and the full one afterwards
    # (MI: the fused LK kernel is its materialising pass; df_dIt . Jm of the Original Jacobian is not accumulated there)
    expect = {"odd_order": 0, "flush_only": 0, "lm": 6}.get(flow, 3)
    if am == L.AM_MI and flow == "esm_original": expect = 0
    assert out[1][1] == expect, "the deferred path did not take the fused launch"
    assert len(direct) == len(fused)
    if flow == "flush_only":
        for k, (a, c) in enumerate(zip(direct, fused)):
            assert np.array_equal(a, c), k
        return
    ncc = am != L.AM_SSD    # NCC and MI: values that pass through the scalars / tables agree to rounding
    for k, (a, c) in enumerate(zip(direct, fused)):
        if a.size <= 64:                       # g, H, f: sums over the pixels
            np.testing.assert_allclose(c, a, rtol=1e-9 if ncc else 1e-11, atol=1e-9 * max(1.0, np.abs(a).max()), err_msg=str(k))
        elif ncc and not np.array_equal(a, c):  # df_dI0 / df_dIt of NCC: functions of the scalars
            assert a.shape[-1] != b_S(ssm) and a.ndim == 2, k
            np.testing.assert_allclose(c, a, rtol=0, atol=1e-11 * np.abs(a).max(), err_msg=str(k))
        else:                                  # per-pixel arrays
            assert np.array_equal(a, c), k


def b_S(ssm):
    return 8 if ssm == L.SSM_HOMOGRAPHY else 6


def test_deferred_calls_survive_an_image_change(gpu_ctx, frame, frame2, monkeypatch):
    """a recorded updatePixVals refers to the image that was current when it was called"""
    corners = synth.square_corners(250, 260, 60)
    vals = {}
    for lazy in (0, 1):
        b = _lazy_batch(gpu_ctx, frame, L.SSM_HOMOGRAPHY, 30, corners, lazy, monkeypatch)
        b.update_pix_vals()                  # deferred ...
        gpu_ctx.set_image(frame2)            # ... and flushed here, against `frame`
        vals[lazy] = b.read(L.BUF_IT).copy()
        b.close()
    assert np.array_equal(vals[0], vals[1])


@pytest.mark.gpu
@pytest.mark.parametrize("am", [L.AM_SSD, L.AM_NCC])
@pytest.mark.parametrize("ssm", [L.SSM_HOMOGRAPHY, L.SSM_AFFINE])
def test_inline_warp_probe_and_equivalence(gpu_ctx, frame, frame2, ssm, am, monkeypatch):
    """Single-target launches read the warp / state from the kernel-argument segment (fused_lk_body, `inline_warp`): the library
    probes once per process that the runtime lays the segment out as the kernels assume (k_kernarg_probe) -- on gfx950 the probe
    must succeed -- and the path gives the bits of the upload-first path (MTFHIP_INLINE_WARP=0), through iterate and through
    the device loop."""
    rng = np.random.default_rng(5)
    corners = (synth.square_corners(250, 260, 70) + rng.uniform(-2, 2, size=(2, 4)))[None]
    out = {}
    for inline in ("1", "0"):
        monkeypatch.setenv("MTFHIP_INLINE_WARP", inline)
        gpu_ctx.set_image(frame)
        b = mtf_amd.Batch(gpu_ctx, am, ssm, 40, 40, 1)
        assert b.inline_warp == (inline == "1")
        b.set_math_mode(mtf_amd.MATH_REPLAY)
        b.set_corners(corners)
        sm = mtf_amd.sm_desc(L.SM_ESM, materialize=1, leven_marq=0, max_iters=6, epsilon=-1.0)
        b.init_template(sm)
        gpu_ctx.set_image(frame2)
        f, g, H = b.iterate(sm)
        n_it, final = b.track(sm)
        out[inline] = (f.copy(), g.copy(), H.copy(), final.copy(), b.read(L.BUF_IT).copy())
        b.close()
    for a, r in zip(out["1"], out["0"]):
        assert np.array_equal(a, r)


@pytest.mark.gpu
@pytest.mark.parametrize("sm_kind,am,extra", [(L.SM_ESM, L.AM_SSD, dict()), (L.SM_FCLK, L.AM_SSD, dict()), (L.SM_ESM, L.AM_NCC, dict()),
                                              (L.SM_ESM, L.AM_SSD, dict(leven_marq=1)), (L.SM_FCLK, L.AM_SSD, dict(leven_marq=1)),
                                              (L.SM_FCLK, L.AM_SSD, dict(sec_ord_hess=1, hess_type=2)), (L.SM_ESM, L.AM_NCC, dict(sec_ord_hess=1, hess_type=5))],
                         ids=lambda v: "_".join("%s%s" % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_two_queue_device_loop_equals_single_queue(oracle, gpu_ctx, frame, frame2, sm_kind, am, extra, monkeypatch):
    """The device-side loop keeps two chunks of independent targets in flight on two queues when the launches materialise the
    interface arrays (track_queues in api_track.hip): same per-target arithmetic, another cut of the pixel pass (half the resident
    workgroups per chunk), so the results agree with the single-queue loop to summation order -- iteration counts, final corners,
    and the arrays the last pass materialised -- and with the oracle's tracker."""
    rng = np.random.default_rng(23)
    B, res = 14, 200          # 14 x 40 000 rows: above the two-queue threshold, odd split (7 + 7)
    monkeypatch.setenv("MTFHIP_TRACK_STREAMS_MIN_ROWS", "0")
    corners = np.stack([synth.square_corners(140 + 17 * (t % 7), 150 + 23 * (t // 7) + 5 * (t % 3), 200.0) for t in range(B)])
    out = {}
    for q in ("1", "2"):
        monkeypatch.setenv("MTFHIP_TRACK_STREAMS", q)
        gpu_ctx.set_image(frame)
        b = mtf_amd.Batch(gpu_ctx, am, L.SSM_HOMOGRAPHY, res, res, B)
        b.set_corners(corners)
        params = dict(leven_marq=0, max_iters=12, epsilon=1e-4)
        params.update(extra)
        sm = mtf_amd.sm_desc(sm_kind, materialize=1, **params)
        b.init_template(sm)
        assert b.track_queues(sm) == int(q)
        gpu_ctx.set_image(frame2)
        n_it, final = b.track(sm)
        out[q] = (n_it.copy(), final.copy(), b.read(L.BUF_IT).copy(), b.read(L.BUF_JT).copy())
        b.close()
    assert np.array_equal(out["1"][0], out["2"][0])
    np.testing.assert_allclose(out["2"][1], out["1"][1], rtol=0, atol=1e-8)
    np.testing.assert_allclose(out["2"][2], out["1"][2], rtol=0, atol=1e-7)
    np.testing.assert_allclose(out["2"][3], out["1"][3], rtol=0, atol=1e-5 * np.abs(out["1"][3]).max())
    o_ssm = oracle.SSM(L.SSM_HOMOGRAPHY, res, res); o_am = oracle.AM(am, res, res); o_am.set_curr_img(frame)
    trk = oracle.Tracker(sm_kind, o_am, o_ssm, **params)
    trk.initialize(corners[B - 1]); o_am.set_curr_img(frame2); trk.update()
    np.testing.assert_allclose(out["2"][1][B - 1], trk.get_region(), rtol=0, atol=2e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("ssm,res", [(L.SSM_HOMOGRAPHY, 60), (L.SSM_AFFINE, 40), (L.SSM_HOMOGRAPHY, 200)])
@pytest.mark.parametrize("sm_kind,extra", [(L.SM_ESM, dict()), (L.SM_ESM, dict(leven_marq=1)), (L.SM_FCLK, dict(leven_marq=1)), (L.SM_FCLK, dict(hess_type=0)),
                                           (L.SM_ICLK, dict()), (L.SM_ICLK, dict(leven_marq=1)), (L.SM_ESM, dict(hess_type=2, jac_type=1))],
                         ids=lambda v: "_".join("%s%s" % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_register_resident_finish_equals_reference_finish(gpu_ctx, frame, frame2, ssm, res, sm_kind, extra, monkeypatch):
    """finish_track_fast_body (tolerance mode, SSD: the system solved by L D L^T in the registers of every lane, reciprocals, no LDS
    elimination) against finish_track_body (the reference's expressions, IEEE divisions, Gauss-Jordan in LDS) on the same reduced
    rows: per-pass trace records -- H as the search method holds it, g, the state update, corners, the Levenberg-Marquardt
    decisions -- and the final state, for one target (157 block rows at 200 x 200: the three-run row sum) and a batch."""
    for B in (1, 5):
        corners = np.stack([synth.square_corners(250 + 9 * t, 240 - 7 * t, float(res) * 1.2) for t in range(B)])
        out = {}
        for ff in ("0", "1"):
            monkeypatch.setenv("MTFHIP_FAST_FINISH", ff)
            gpu_ctx.set_image(frame)
            b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, ssm, res, res, B)
            b.set_corners(corners)
            params = dict(leven_marq=0, max_iters=8, epsilon=1e-6)
            params.update(extra)
            sm = mtf_amd.sm_desc(sm_kind, materialize=0, **params)
            b.init_template(sm)
            gpu_ctx.set_image(frame2)
            b.track_trace(8)
            n_it, final = b.track(sm)
            out[ff] = (n_it.copy(), final.copy(), b.read_track_trace(n_it), b.get_state().copy())
            b.close()
        assert np.array_equal(out["0"][0], out["1"][0])
        np.testing.assert_allclose(out["1"][1], out["0"][1], rtol=0, atol=1e-6)
        np.testing.assert_allclose(out["1"][3], out["0"][3], rtol=1e-5, atol=1e-9)
        t0, t1 = out["0"][2], out["1"][2]
        for t in range(B):
            assert len(t0[t]) == len(t1[t]) > 0
            for k, (r0, r1) in enumerate(zip(t0[t], t1[t])):
                # pass 0 starts from the same reduced row: H and g are the same numbers, dp differs by the solver's rounding (condition
                # number x eps); later passes start from states that differ by that much, and g = H dp amplifies it
                tol = 0.0 if k == 0 else 1e-6
                np.testing.assert_allclose(r1["H"], r0["H"], rtol=0, atol=tol * np.abs(r0["H"]).max())
                np.testing.assert_allclose(r1["g"], r0["g"], rtol=0, atol=tol * np.abs(t0[t][0]["g"]).max())   # (g -> 0 with convergence)
                np.testing.assert_allclose(r1["dp"], r0["dp"], rtol=0, atol=(1e-7 if k == 0 else 1e-5) * np.abs(r0["dp"]).max())
                np.testing.assert_allclose(r1["corners"], r0["corners"], rtol=0, atol=1e-7 if k == 0 else 1e-6)
                assert r1["undo"] == r0["undo"] and np.isclose(r1["lm_delta"], r0["lm_delta"], rtol=1e-12)
