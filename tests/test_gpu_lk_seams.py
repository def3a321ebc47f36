"""GPU: the compositional LK path -- homography and affine, first and second order (sec_ord_hess) -- at the seams of its kernels'
decompositions and of the frame, against the oracle.  The cases are tests/helpers/lk_seam_cases.py's; tests/test_lk_seams_cpu.py holds the
reference alone to the conditions that make these comparisons meaningful (finite, not vacuous, off the integer grid, a jitter floor a
tenth of the device-grid bound).

Part A  one fused iteration (Batch.iterate: the fused kernel and k_second_order_ssd reading CURR_PTS), single targets and batches of three;
Part B  the first pass of the device-side loop (Batch.track: k_second_order_ssd building its own points from INIT_PTS, or from INIT_HXY /
        INIT_Z when one region of the batch is projective), its solve held to the reference's solver on the device's own system;
Part C  the image-Hessian kernels at the frame border and on integer coordinates, the SSM pixel-Hessian kernel and the weighted plane sum
        fed the oracle's arrays at ragged pixel counts.

Bounds are those of tests/test_gpu_parity.py::_fused_follow (oracle grid: f 1e-12, H 1e-9, g 1e-10 of max(|g|, g_scale), dp 1e-6 or 1e-12
absolute; device grid: f 1e-8, H 1e-5, g 1e-5; tolerance-mode arithmetic 2e-6), of tests/test_gpu_trackers.py::
test_device_loop_second_order_hessians (1e-5, final corners 2e-4 px) and of test_second_order_interface (oracle-fed: 1e-10 relative, 1e-11
of the maximum)."""
import os
import sys

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lk_seam_cases as K   # noqa: E402
from lk_seam_cases import dp_ulp_sensitivity as _dp_ulp_sensitivity   # noqa: E402

pytestmark = pytest.mark.gpu

AM_KW = {K.MI: dict(mi_n_bins=8)}


def _batch(gpu_ctx, frame, model, resx, resy, corners, grid_from=None):
    """a batch on `frame` inside `corners` (B x 2 x 4); grid_from: the oracle reference whose grid is written over the device's"""
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, model.am, model.ssm, resx, resy, corners.shape[0], **AM_KW.get(model.am, {}))
    b.set_math_mode(mtf_amd.MATH_REPLAY)
    b.set_corners(corners)
    if grid_from is not None:
        hm = grid_from["init_pts_hm"].reshape(-1, 3)
        b.write(L.BUF_INIT_PTS, grid_from["init_pts"].reshape(1, -1, 2).transpose(0, 2, 1))
        b.write(L.BUF_INIT_HXY, hm[:, :2].T[None])
        b.write(L.BUF_INIT_Z, hm[:, 2][None])
        b.set_state(np.zeros((1, b.S)))
    return b


def _sm(model, materialize, **kw):
    params = dict(leven_marq=0)
    params.update(model.extra)
    params.update(kw)
    return mtf_amd.sm_desc(model.sm, materialize=materialize, **params)


def _check(f, g, H, rec, am, tol_f, tol_H, tol_g, what):
    gs = K.g_scale(rec, am)
    ef, eH = K.rel(f, rec["f"]), K.rel(H, rec["H"])
    eg = float(np.linalg.norm(g - rec["g"]) / max(np.linalg.norm(rec["g"]), gs, 1e-300))
    print("%s: f %.3e H %.3e g %.3e" % (what, ef, eH, eg))
    assert ef < tol_f, what
    assert eH < tol_H, what
    assert eg < tol_g, what
    return dict(f=ef, H=eH, g=eg)


# ================================================================================================ Part A
@pytest.mark.parametrize("cid", K.IDS)
def test_fused_iteration_at_the_seams(oracle, gpu_ctx, frame, frame2, cid, parity_record):
    """One Batch.iterate from the identity on the next frame against the oracle's first iteration, materialised and lean, in the replay
    arithmetic, on the oracle's grid (per-pixel quantities bit-identical, only the order of the sums differs: the tight bounds, the
    materialised It and dIt_dx bit for bit, and -- inside the frame from 35 pixels on -- the update solved from the device's H, g: 1e-6, or
    1e-12 absolute; where that misses with H and g inside their tight bounds, ten times the reference's own dp under one-ulp changes of its
    own H and g, both figures recorded: 23x37 ICLK NCC homography, cond(H) 1e16, device H 3.6e-16 off, dp 1.3e-6, reference 1.2e-6) and on
    the device's own grid (the 1e-5 bounds); first-order cases also in the tolerance arithmetic (lean, device grid, 2e-6).

    Wholly outside the frame every sample is the border constant: SSD must give f = 0, g = 0, H = 0 exactly, with and without the
    second-order term.  NCC divides 0 by 0 there and the reference itself returns NaN (asserted on the oracle in
    tests/test_lk_seams_cpu.py), so for those cases nothing is asserted of the device beyond that the call returns."""
    c = K.BY_ID[cid]
    m = c.model
    ref = K.reference(oracle, frame, frame2, cid)
    rec = ref["rec"]
    corners = K.REGIONS[c.region][None]
    worst = {}
    for grid in ("oracle_grid", "device_grid"):
        for materialize in (1, 0):
            b = _batch(gpu_ctx, frame, m, c.resx, c.resy, corners, ref if grid == "oracle_grid" else None)
            sm = _sm(m, materialize)
            b.init_template(sm)
            gpu_ctx.set_image(frame2)
            f, g, H = b.iterate(sm)
            what = "%s %s materialize=%d" % (cid, grid, materialize)
            if c.region == "outside":
                if m.am == K.SSD:
                    assert f[0] == 0.0 and np.all(g[0] == 0.0) and np.all(H[0] == 0.0), what
                b.close()
                continue
            tight = grid == "oracle_grid"
            e = _check(f[0], g[0], H[0], rec, m.am, *((1e-12, 1e-9, 1e-10) if tight else (1e-8, 1e-5, 1e-5)), what)
            worst[what] = e
            if tight and materialize:
                assert np.array_equal(b.read(L.BUF_IT)[0], ref["It"]), what
                if m.sm != K.ICLK:
                    assert np.array_equal(b.read(L.BUF_DIT_DX)[0], ref["dIt_dx"]), what
            if tight and c.region in ("inside", "quad") and K.n_pix(c) >= 35:
                dp = -oracle.colpiv_qr_solve(H[0], g[0])
                e_dp = K.rel(dp, rec["dp"])
                if not (e_dp < 1e-6 or np.abs(dp - rec["dp"]).max() < 1e-12):
                    # H and g have just passed the tight bounds (and, materialised, It / dIt_dx are the oracle's bits): what is left is the
                    # order of the sums, a few ulps of H, through a solve whose condition number is 1e16 on the homography.  No guessed
                    # number: the case's bound is ten times what the REFERENCE's solve does with one-ulp changes of its own H and g
                    floor = _dp_ulp_sensitivity(oracle, rec)
                    parity_record.append(dict(test="lk_seams_dp_order_sensitivity", case=what, device_dp_error=e_dp,
                                              reference_dp_under_one_ulp=floor, device_H_error=e["H"], device_g_error=e["g"]))
                    print("%s: dp %.3e, the reference's own dp under one-ulp changes of H, g %.3e" % (what, e_dp, floor))
                    assert e_dp < 10.0 * floor, (what, e_dp, floor)
            if not tight and not materialize and not K.second_order(c):
                b.set_math_mode(mtf_amd.MATH_FAST)
                ff, gf, Hf = b.iterate(sm)
                worst[what + " fast"] = _check(ff[0], gf[0], Hf[0], rec, m.am, 1e-8, 2e-6, 2e-6, what + " MATH_FAST")
            b.close()
    if worst:
        parity_record.append(dict(test="lk_seams_fused_iteration", case=cid, **{k.split(" ", 1)[1]: v for k, v in worst.items()}))


BATCH_SHAPES = [(5, 7), (7, 9), (33, 31), (32, 33)]      # N = 35, 63, 1023, 1056
BATCH_REGIONS = ("inside", "right", "quad")


@pytest.mark.parametrize("shape", BATCH_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", K.MODELS, ids=K.model_name)
def test_fused_iteration_in_a_batch_of_three(oracle, gpu_ctx, frame, frame2, model, shape):
    """`inside`, `right` and `quad` as three targets of one batch -- odd pixel counts against the target-major strides of every per-pixel
    array, and a projective region next to a square one -- each against its own single-target oracle, at the device-grid bounds"""
    resx, resy = shape
    corners = np.stack([K.REGIONS[r] for r in BATCH_REGIONS])
    for materialize in (1, 0):
        b = _batch(gpu_ctx, frame, model, resx, resy, corners)
        sm = _sm(model, materialize)
        b.init_template(sm)
        gpu_ctx.set_image(frame2)
        f, g, H = b.iterate(sm)
        for t, region in enumerate(BATCH_REGIONS):
            rec = K.region_reference(oracle, frame, frame2, model, resx, resy, region)["rec"]
            _check(f[t], g[t], H[t], rec, model.am, 1e-8, 1e-5, 1e-5, "%s %dx%d target %d (%s) materialize=%d" % (
                K.model_name(model), resx, resy, t, region, materialize))
        b.close()


# ================================================================================================ Part B
LOOP_SHAPES = [(5, 7), (16, 17), (32, 33), (37, 23)]
LOOP_MODELS = [m for m in K.MODELS if m.ssm == K.HOM]
LOOP = dict(max_iters=12, epsilon=1e-5)


def _track(gpu_ctx, frame, frame2, model, resx, resy, regions):
    corners = np.stack([K.REGIONS[r] for r in regions])
    b = _batch(gpu_ctx, frame, model, resx, resy, corners)
    sm = _sm(model, 0, **LOOP)
    b.init_template(sm)
    gpu_ctx.set_image(frame2)
    b.track_trace(2 * LOOP["max_iters"])
    n_it, final = b.track(sm)
    recs = b.read_track_trace(n_it)
    b.track_trace(0)
    b.close()
    return n_it, final, recs


def _first_pass_of_the_loop(oracle, frame, frame2, model, resx, resy, region, recs, final, parity_record, what):
    """the first non-undo record of one target against the oracle's first iteration, its solve against the reference's solver on the
    same system, and -- where the oracle converged inside the frame -- the final corners"""
    run = K.full_run(oracle, frame, frame2, model, resx, resy, region, **LOOP)
    o = run["trace"][0]
    d0 = [r for r in recs if not r["undo"]][0]
    # the one-launch loop of first-order ICLK works from the constant template Hessian and records none (include/mtfhip.h): every other
    # model must have recorded the H it solved
    if not (model.sm == K.ICLK and not model.extra.get("sec_ord_hess")):
        assert d0["has_H"], what
    eH = K.rel(d0["H"], o["H"]) if d0["has_H"] else 0.0
    eg = K.rel(d0["g"], o["g"])
    print("%s: H %.3e g %.3e" % (what, eH, eg))
    assert eH < 1e-5 and eg < 1e-5, (what, eH, eg)
    if d0["has_H"]:
        # dp is not compared with the oracle's (at the borders |dp| is 1e2 .. 1e3 and the oracle's own dp moves by up to 8e-5 under the
        # 1e-12 px between the two grids): the device's solve is held to the reference's SOLVER on the device's own system, both measured
        # against an extended-precision solution; ten times the reference solver's error is the room for another backward-stable
        # elimination order
        exact = K.long_double_solve(d0["H"], -d0["g"])
        assert exact is not None, what
        err_ref = float(np.linalg.norm(np.asarray(-oracle.colpiv_qr_solve(d0["H"], d0["g"]) - exact, dtype=np.float64)))
        err_dev = float(np.linalg.norm(np.asarray(d0["dp"] - exact, dtype=np.float64)))
        parity_record.append(dict(test="lk_seams_loop_solve", case=what, reference_solver_error=err_ref, device_solver_error=err_dev,
                                  dp_norm=float(np.linalg.norm(d0["dp"]))))
        print("%s: solve error device %.3e reference %.3e |dp| %.3e" % (what, err_dev, err_ref, np.linalg.norm(d0["dp"])))
        assert err_dev <= 10.0 * err_ref + 1e-12, (what, err_dev, err_ref)
    if run["iters"] < LOOP["max_iters"] and region in ("inside", "quad"):
        np.testing.assert_allclose(final, run["region"], rtol=0, atol=2e-4, err_msg=what)


@pytest.mark.parametrize("shape", LOOP_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", LOOP_MODELS, ids=K.model_name)
def test_device_loop_first_pass_on_a_projective_region(oracle, gpu_ctx, frame, frame2, model, shape, parity_record):
    """(i) one `quad` target: the loop's own points come from INIT_HXY / INIT_Z (unit_z = 0); (ii) [inside, quad, right]: the projective
    region clears the batch-wide unit_z, so the square target runs the general branch too, next to a target across the frame edge"""
    resx, resy = shape
    for regions in (("quad",), ("inside", "quad", "right")):
        n_it, final, recs = _track(gpu_ctx, frame, frame2, model, resx, resy, regions)
        assert np.all(np.isfinite(final))
        for t, region in enumerate(regions):
            _first_pass_of_the_loop(oracle, frame, frame2, model, resx, resy, region, recs[t], final[t], parity_record,
                                    "%s %dx%d B=%d target %d (%s)" % (K.model_name(model), resx, resy, len(regions), t, region))


@pytest.mark.parametrize("shape", LOOP_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", [m for m in LOOP_MODELS if m.am == K.SSD], ids=K.model_name)
def test_device_loop_next_to_a_region_outside_the_frame(oracle, gpu_ctx, frame, frame2, model, shape, parity_record):
    """(iii) [inside, outside], SSD: the outside target's system is H = 0, g = 0 -- its corners stay where they are, nothing is NaN -- and
    its neighbour's first pass has the bits of the same target tracked alone"""
    resx, resy = shape
    n_it, final, recs = _track(gpu_ctx, frame, frame2, model, resx, resy, ("inside", "outside"))
    assert np.all(np.isfinite(final))
    for r in recs[1]:
        assert np.all(np.isfinite(r["g"])) and np.all(np.isfinite(r["dp"])) and np.all(np.isfinite(r["H"]))
    assert np.array_equal(final[1], K.REGIONS["outside"])
    n1, final1, recs1 = _track(gpu_ctx, frame, frame2, model, resx, resy, ("inside",))
    a, a1 = [r for r in recs[0] if not r["undo"]][0], [r for r in recs1[0] if not r["undo"]][0]
    for q in ("H", "g", "dp", "corners"):
        assert np.array_equal(a[q], a1[q]), q
    assert a["f"] == a1["f"] and a["has_H"] == a1["has_H"]
    _first_pass_of_the_loop(oracle, frame, frame2, model, resx, resy, "inside", recs[0], final[0], parity_record,
                            "%s %dx%d B=2 target 0 (inside, next to outside)" % (K.model_name(model), resx, resy))


# ================================================================================================ Part C
def test_image_hessians_at_the_border_and_on_integer_coordinates(oracle, gpu_ctx, frame):
    """k_img_hess and k_warped_img_hess where the constant border, the last row / column and the dx == 0 rule (imgUtils.h:96-108) switch for
    the sample or for one of its stencil points two pixels away: bit for bit the oracle's getImgHess / getWarpedImgHess -- the same
    expressions in the same order without contraction, as for the samples and the gradients
    (test_gpu_parity.py::test_border_and_integer_coordinate_cases).  272 points: one workgroup and a quarter of a wave."""
    h, w = frame.shape
    pts = K.hess_border_points(h, w, 272)
    flat = np.ascontiguousarray(pts.T.ravel())
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, 16, 17, 1)
    b.set_corners(K.REGIONS["inside"][None])
    want = oracle.get_img_hess(frame, flat).reshape(-1, 2, 2)
    assert np.abs(want).max() > 10.0 and (want == 0).any()
    b.update_pix_hess(pts=pts[None])
    assert np.array_equal(b.read(L.BUF_D2IT_DX2)[0], want)
    b.initialize_pix_hess(pts=pts[None])
    assert np.array_equal(b.read(L.BUF_D2I0_DX2)[0], want)
    # warped form: the oracle's hess_pts of a projective state at these points would leave the list; the stencil of a small affine-like
    # offset set is enough to tell every sample apart: (+xx, -xx, +yy, -yy, +xy, -xy, +yx, -yx), each pair with its own step
    off = np.array([[2, 0.25], [-2, -0.25], [0.5, 2], [-0.5, -2], [1, 1.25], [-1, -1.25], [1.5, -1], [-1.5, 1]], dtype=np.float64)
    for o in (np.array([[2, 0], [-2, 0], [0, 2], [0, -2], [1, 1], [-1, -1], [1, -1], [-1, 1]], dtype=np.float64), off):
        hp = np.ascontiguousarray((pts.T[:, None, :] + o[None]).reshape(-1, 16))
        want_w = oracle.get_warped_img_hess(frame, flat, hp.ravel()).reshape(-1, 2, 2)
        b.update_pix_hess(pts=pts[None], hess_pts=hp[None], warped=True)
        assert np.array_equal(b.read(L.BUF_D2IT_DX2)[0], want_w)
    assert not np.array_equal(want_w, want)
    b.close()


@pytest.mark.parametrize("ssm", [L.SSM_HOMOGRAPHY, L.SSM_AFFINE])
def test_warped_image_hessian_with_the_oracles_hess_pts(oracle, gpu_ctx, frame, ssm):
    """k_hess_pts on a projective homography state (p[6], p[7] != 0) and on an affine state, across the right edge of the frame, within
    the 1e-9 px of test_second_order_interface; k_warped_img_hess fed the ORACLE's hess_pts: bit for bit"""
    resx, resy = 16, 17
    o_ssm = oracle.SSM(ssm, resx, resy)
    o_ssm.set_corners(K.REGIONS["right"])
    p = np.array([0.011, -0.007, 1.3, 0.005, -0.012, -0.8, 6e-5, -4e-5]) if ssm == L.SSM_HOMOGRAPHY else np.array([1.3, -0.8, 0.011, -0.007, 0.005, -0.012])
    o_ssm.set_state(p)
    o_ssm.update_hess_pts(1.0)
    pts, hp = o_ssm.get("curr_pts"), o_ssm.get("hess_pts").reshape(-1, 16)
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, ssm, resx, resy, 1)
    b.set_corners(K.REGIONS["right"][None])
    b.set_state(p[None])
    b.update_hess_pts()
    np.testing.assert_allclose(b.read(L.BUF_HESS_PTS)[0], hp, rtol=0, atol=1e-9)
    want = oracle.get_warped_img_hess(frame, pts, hp.ravel()).reshape(-1, 2, 2)
    assert (want == 0).any() and np.abs(want).max() > 1.0          # border and image
    b.update_pix_hess(pts=pts.reshape(1, -1, 2).transpose(0, 2, 1), hess_pts=hp[None], warped=True)
    assert np.array_equal(b.read(L.BUF_D2IT_DX2)[0], want)
    b.close()


def test_multichannel_image_hessian_at_the_border(oracle, gpu_ctx):
    """k_img_hess_mc on a three-channel frame at the same points, both forms: bit for bit the oracle's multi-channel getImgHess /
    getWarpedImgHess (mc::getImgHess, imgUtils.cc:1127-1168, :1036-1075).  The reference's multi-channel sampler multiplies each texel by
    the product of its two weights where the single-channel one multiplies texel, weight, weight in turn, so per channel the result is the
    single-channel oracle's on that channel's plane only to the last bits of a sample (held here to 4 ulps of 255: three samples and a
    doubling), not to the bit -- the branch each stencil point takes (border constant or image) is what that comparison pins"""
    from mtf_amd import synth
    img3 = synth.make_frame_mc(512, 512)
    h, w = img3.shape[:2]
    pts = K.hess_border_points(h, w, 272)
    flat = np.ascontiguousarray(pts.T.ravel())
    off = np.array([[2, 0.25], [-2, -0.25], [0.5, 2], [-0.5, -2], [1, 1.25], [-1, -1.25], [1.5, -1], [-1.5, 1]], dtype=np.float64)
    hp = np.ascontiguousarray((pts.T[:, None, :] + off[None]).reshape(-1, 16))
    o_am = oracle.AM(L.AM_SSD, 16, 17); o_am.set_channels(3); o_am.set_curr_img(img3)
    o_am.initialize_pix_hess_pts(flat)
    o_am.update_pix_hess_pts(flat)
    want = o_am.get("d2It_dx2").reshape(272, 3, 2, 2).copy()
    o_am.update_pix_hess_warped(flat, hp.ravel())
    want_w = o_am.get("d2It_dx2").reshape(272, 3, 2, 2).copy()
    gpu_ctx.set_image(img3)
    b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, 16, 17, 1, n_channels=3)
    b.set_corners(K.REGIONS["inside"][None])
    b.update_pix_hess(pts=pts[None])
    plain = b.read(L.BUF_D2IT_DX2)[0].reshape(272, 3, 2, 2).copy()
    b.update_pix_hess(pts=pts[None], hess_pts=hp[None], warped=True)
    warped = b.read(L.BUF_D2IT_DX2)[0].reshape(272, 3, 2, 2).copy()
    assert np.array_equal(plain, want)
    assert np.array_equal(warped, want_w)
    tol = 4 * np.spacing(255.0)
    for ch in range(3):
        plane = np.ascontiguousarray(img3[:, :, ch])
        assert np.abs(plain[:, ch] - oracle.get_img_hess(plane, flat).reshape(-1, 2, 2)).max() <= tol, ch
        assert np.abs(warped[:, ch] - oracle.get_warped_img_hess(plane, flat, hp.ravel()).reshape(-1, 2, 2)).max() <= tol, ch
    assert not np.array_equal(plain[:, 0], plain[:, 1])
    b.close()


@pytest.mark.parametrize("shape", [(5, 7), (33, 31), (32, 33)], ids=lambda s: "%dx%d" % s)      # N = 35, 1023, 1056
@pytest.mark.parametrize("ssm", [L.SSM_HOMOGRAPHY, L.SSM_AFFINE])
def test_pixel_hessian_and_weighted_plane_sum_fed_the_oracles_arrays(oracle, gpu_ctx, frame, frame2, ssm, shape):
    """k_pix_hessian and k_weighted_plane_sum + k_plane_sum_finish with B = 3 (inside, right, quad) at pixel counts that leave a partial
    wave in the last workgroup, every input the oracle's own (Batch.write): the Init and Warped pixel Hessians within 1e-10 relative /
    1e-11 of the maximum, and -- with a zero Jacobian, so that H is the weighted sum alone -- cmptCurrHessian, cmptInitHessian and
    cmptSumOfHessians (second order) against the oracle's on the same arrays, at the same bounds"""
    resx, resy = shape
    N = resx * resy
    regions = ("inside", "right", "quad")
    corners = np.stack([K.REGIONS[r] for r in regions])
    S = 8 if ssm == L.SSM_HOMOGRAPHY else 6
    p = np.array([0.011, -0.007, 1.3, 0.005, -0.012, -0.8, 6e-5, -4e-5]) if ssm == L.SSM_HOMOGRAPHY else np.array([1.3, -0.8, 0.011, -0.007, 0.005, -0.012])
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, ssm, resx, resy, 3)
    b.set_corners(corners)
    b.initialize_pix_vals(); b.initialize_pix_grad(); b.initialize_pix_hess()
    b.initialize_similarity(); b.initialize_grad(); b.initialize_hess()
    b.set_state(np.stack([p, 0.5 * p, -p]))
    gpu_ctx.set_image(frame2)
    b.update_pix_vals(); b.update_pix_grad(); b.update_pix_hess()
    b.update_similarity(False); b.update_curr_grad(); b.update_init_grad()
    o = []
    for t, region in enumerate(regions):
        o_ssm = oracle.SSM(ssm, resx, resy); o_am = oracle.AM(L.AM_SSD, resx, resy); o_am.set_curr_img(frame)
        o_ssm.set_corners(K.REGIONS[region])
        pts0 = o_ssm.get("curr_pts")
        o_am.initialize_pix_vals(pts0); o_am.initialize_pix_grad_pts(pts0); o_am.initialize_pix_hess_pts(pts0)
        o_am.initialize_similarity(); o_am.initialize_grad(); o_am.initialize_hess()
        D0 = o_ssm.cmpt_warped_pix_hessian(o_am.get("d2I0_dx2"), o_am.get("dI0_dx"))
        o_ssm.set_state((p, 0.5 * p, -p)[t])
        o_am.set_curr_img(frame2)
        pts = o_ssm.get("curr_pts")
        o_am.update_pix_vals(pts); o_am.update_pix_grad_pts(pts); o_am.update_pix_hess_pts(pts)
        o_am.update_similarity(False); o_am.update_curr_grad(); o_am.update_init_grad()
        ph, gr = o_am.get("d2It_dx2").copy(), o_am.get("dIt_dx").copy()
        o.append(dict(ssm=o_ssm, am=o_am, ph=ph, gr=gr, D0=np.asarray(D0).reshape(N, S, S), df_dIt=o_am.get("df_dIt").copy(), df_dI0=o_am.get("df_dI0").copy()))
    b.write(L.BUF_DIT_DX, np.stack([x["gr"].reshape(2, N).T for x in o]))
    b.write(L.BUF_D2IT_DX2, np.stack([x["ph"] for x in o]))
    for variant, name in ((L.JAC_INIT, "init_pix"), (L.JAC_WARPED, "warped_pix")):
        b.cmpt_pix_hessian(variant, L.BUF_D2IT_DX2, L.BUF_DIT_DX, L.BUF_D2IT_DP2)
        got = b.read(L.BUF_D2IT_DP2)
        for t in range(3):
            want = np.asarray(getattr(o[t]["ssm"], "cmpt_%s_hessian" % name)(o[t]["ph"], o[t]["gr"])).reshape(N, S, S)
            np.testing.assert_allclose(got[t], want, rtol=1e-10, atol=1e-11 * np.abs(want).max(), err_msg="%s target %d" % (name, t))
    Dt = [np.asarray(x["ssm"].cmpt_warped_pix_hessian(x["ph"], x["gr"])).reshape(N, S, S) for x in o]
    # D2*_DP2 on the device: planes [c][r][N] per target
    b.write(L.BUF_D2IT_DP2, np.stack([d.transpose(2, 1, 0) for d in Dt]))
    b.write(L.BUF_D2I0_DP2, np.stack([x["D0"].transpose(2, 1, 0) for x in o]))
    b.write(L.BUF_DF_DIT, np.stack([x["df_dIt"] for x in o]))
    b.write(L.BUF_DF_DI0, np.stack([x["df_dI0"] for x in o]))
    zero = np.zeros((3, N, S))
    b.write(L.BUF_JT, zero); b.write(L.BUF_J0, zero)
    Jz = np.zeros(N * S)
    got_c, got_i, got_s = b.cmpt_curr_hessian2(), b.cmpt_init_hessian2(), b.cmpt_sum_of_hessians2()
    for t in range(3):
        am = o[t]["am"]
        for got, want, what in ((got_c[t], am.cmpt_curr_hessian2(Jz, Dt[t]), "curr2"), (got_i[t], am.cmpt_init_hessian2(Jz, o[t]["D0"]), "init2"),
                                (got_s[t], am.cmpt_sum_of_hessians2(Jz, Jz, o[t]["D0"], Dt[t]), "sum2")):
            assert np.abs(want).max() > 0
            np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-11 * np.abs(want).max(), err_msg="%s target %d" % (what, t))
    b.close()
