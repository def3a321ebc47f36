"""GPU: the additive search methods FALK / IALK (k_alk_pass, k_alk_finish) and the Similitude / Isometry / Translation state space models
(the affine pixel pass + the projection, k_finish_track_lo) at the seams of their kernels' decompositions and of the frame, against
alk_ref.AlkRef and lowdof_ref.LKRef.  The cases are tests/helpers/addlow_seam_cases.py's; tests/test_alk_lowdof_seams_cpu.py holds the
references alone to the conditions that make these comparisons meaningful (finite, not vacuous, off the integer grid, a jitter floor a
tenth of the device-grid bound, the projective region really projective, the loops' references converged).

Part A  one pass (Batch.iterate) away from the identity per case of the table, every variant of its model, materialised and lean, in the
        replay arithmetic: on the reference's grid and on the device's own (set_corners alone: on `quad` the homography's unit_z = 0
        branch of k_alk_pass, and k_init_grid's re-homogenised projective lattice for the affine and the low-order models);
Part B  batches of three -- a square region, one across the frame's edge and the projective one -- each target against its own
        single-target reference, at the small batch shapes and at 91 x 91 (nine partial rows per target, three targets);
Part C  the device loop (Batch.track): the first pass against the reference's, the solve against the reference's solver on the device's
        own recorded system, final corners where the reference converged; next to a region outside the frame; and on the four BIG
        shapes (9, 9, 17 and 25 partial rows: the finish kernels' 256-thread, three-run row sum) the loop against its own single passes
        and against Batch.iterate's host assembly of the same partial rows.

Bounds are the project's: on the reference's grid f 1e-12, H 1e-9, g 1e-10 of max(|g|, g_scale), the update 1e-6 or 1e-12 absolute
(tests/test_gpu_alk.py::test_one_pass_parity, tests/test_gpu_lowdof.py::test_one_pass_parity), low-order JT / JM 1e-12 of their scale; on
the device's grid f 1e-8, H 1e-5, g 1e-5 (tests/test_gpu_lk_seams.py), the low-order lean pass in MATH_FAST 2e-6
(tests/test_gpu_lowdof.py::test_one_pass_parity); loops 1e-5 on the first pass and 2e-4 px on final corners (tests/test_gpu_lk_seams.py
Part B)."""
import os
import sys

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import addlow_seam_cases as K   # noqa: E402

pytestmark = pytest.mark.gpu

TIGHT = (1e-12, 1e-9, 1e-10)
LOOSE = (1e-8, 1e-5, 1e-5)


def _batch(gpu_ctx, frame, m, resx, resy, corners):
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, m.am, m.ssm, resx, resy, corners.shape[0])
    b.set_math_mode(mtf_amd.MATH_REPLAY)
    b.set_corners(corners)
    return b


def _write_grid(b, ref):
    """the device gets the reference's sample grid verbatim (tests/test_gpu_alk.py::oracle_grid, tests/test_gpu_lowdof.py::ref_grid)"""
    hm = ref["init_pts_hm"]
    b.write(L.BUF_INIT_PTS, ref["init_pts"][None])
    b.write(L.BUF_INIT_HXY, hm[:2][None])
    b.write(L.BUF_INIT_Z, hm[2][None])
    b.set_state(np.zeros((1, b.S)))


def _sm(m, params, materialize, **kw):
    p = dict(leven_marq=0, max_iters=1)
    p.update(params)
    p.update(kw)
    return mtf_amd.sm_desc(m.sm, materialize=materialize, **p)


def _errors(f, g, H, rec, am):
    gs = K.g_scale(rec, am)
    return dict(f=K.rel(f, rec["f"]), H=K.rel(H, rec["H"]), g=float(np.linalg.norm(g - rec["g"]) / max(np.linalg.norm(rec["g"]), gs, 1e-300)))


def _check(f, g, H, rec, am, tol, what):
    e = _errors(f, g, H, rec, am)
    print("%s: f %.3e H %.3e g %.3e" % (what, e["f"], e["H"], e["g"]))
    assert e["f"] < tol[0], (what, e)
    assert e["H"] < tol[1], (what, e)
    assert e["g"] < tol[2], (what, e)
    return e


def _runs(m):
    """ALK: one batch serves the three hess_type (the template is initialised once, with InitialSelf's constant Hessian); low order:
    chained_warp decides how the template's Jacobian is taken, so each variant initialises its own batch"""
    v = K.variants(m)
    return [v] if m.family == K.ALK else [[x] for x in v]


# ================================================================================================ Part A
@pytest.mark.parametrize("cid", K.IDS)
def test_one_pass_at_the_seams(oracle, gpu_ctx, frame, frame2, cid, parity_record):
    """One Batch.iterate at the case's start state on the next frame against the reference's pass there.

    On the reference's grid every per-pixel quantity has identical inputs and only the order of the sums differs: materialised It,
    dIt_dx (FALK, low-order non-ICLK) and ALK's JT bit for bit, low-order JT / JM 1e-12 of their scale; f, H, g at the tight bounds; and --
    inside the frame from 35 pixels on -- the update solved from the device's H, g within 1e-6, or 1e-12 absolute; where that misses with H
    and g inside their bounds, ten times the reference's own dp under one-ulp changes of its H and g, both figures recorded.
    On the device's own grid: the 1e-5 bounds, the low-order lean pass also in MATH_FAST at 2e-6; on `quad` INIT_PTS within 1e-12 of the
    frame size of the reference's, and INIT_Z exactly 1 for the affine and the low-order models.

    Wholly outside the frame SSD gives f = 0, g = 0, H = 0 exactly; NCC divides 0 by 0 in the reference (asserted there), so for those
    cases nothing is asserted beyond that the call returns."""
    c = K.BY_ID[cid]
    m = c.model
    N = K.n_pix(c)
    corners = K.REGIONS[c.region][None]
    base = K.reference(oracle, frame, frame2, cid)
    start = base["start"]
    worst = {}
    for grid in ("oracle_grid", "device_grid"):
        tight = grid == "oracle_grid"
        for materialize in (1, 0):
            for run in _runs(m):
                b = _batch(gpu_ctx, frame, m, c.resx, c.resy, corners)
                try:
                    if tight:
                        _write_grid(b, base)
                    elif c.region == "quad":
                        assert np.abs(b.read(L.BUF_INIT_PTS)[0] - base["init_pts"]).max() < 1e-12 * K.FRAME_SIZE, cid
                        if not (m.family == K.ALK and m.ssm == K.HOM):
                            assert np.all(b.read(L.BUF_INIT_Z)[0] == 1.0), cid
                    for k, (label, p) in enumerate(run):
                        sm = _sm(m, p, materialize)
                        if k == 0:
                            gpu_ctx.set_image(frame)
                            b.init_template(sm)
                            gpu_ctx.set_image(frame2)
                        b.set_state(start[None])
                        ref = base if m.family == K.ALK else K.reference(oracle, frame, frame2, cid, warp=b.get_warp()[0])
                        rec = ref["recs"][label]
                        f, g, H = b.iterate(sm)
                        what = "%s %s %s materialize=%d" % (cid, grid, label, materialize)
                        if c.region == "outside":
                            if m.am == K.SSD:
                                assert f[0] == 0.0 and np.all(g[0] == 0.0) and np.all(H[0] == 0.0), what
                            continue
                        e = _check(f[0], g[0], H[0], rec, m.am, TIGHT if tight else LOOSE, what)
                        worst[what.split(" ", 1)[1]] = e
                        if tight and materialize:
                            S = b.S
                            assert np.array_equal(b.read(L.BUF_IT)[0], rec["It"]), what
                            if m.family == K.ALK:
                                assert np.array_equal(b.read(L.BUF_JT)[0], rec["Jt"].reshape(S, -1).T), what
                                if m.sm == K.FALK:
                                    assert np.array_equal(b.read(L.BUF_DIT_DX)[0], rec["dIt_dx"].reshape(2, -1).T), what
                            elif rec["Jt"] is not None and m.sm != K.ICLK:
                                assert np.array_equal(b.read(L.BUF_DIT_DX)[0], rec["dIt_dx"].reshape(2, -1).T), what
                                want = rec["Jt"].reshape(S, -1).T
                                assert np.abs(b.read(L.BUF_JT)[0] - want).max() <= 1e-12 * np.abs(want).max(), what
                                if m.sm == K.ESM and (p["jac_type"] == 0 or p["hess_type"] == 3):
                                    Jm = (ref["J0"][label].reshape(S, -1).T + want) / 2.0
                                    assert np.abs(b.read(L.BUF_JM)[0] - Jm).max() <= 1e-12 * np.abs(Jm).max(), what
                        if tight and c.region in ("inside", "quad") and N >= 35:
                            dp = -oracle.colpiv_qr_solve(H[0], g[0])
                            e_dp = K.rel(dp, rec["dp"])
                            if not (e_dp < 1e-6 or np.abs(dp - rec["dp"]).max() < 1e-12):
                                # H and g have just passed the tight bounds: what is left is the order of the sums through the solve.  The
                                # case's bound is ten times what the REFERENCE's solve does with one-ulp changes of its own H and g
                                floor = K.dp_ulp_sensitivity(oracle, rec)
                                parity_record.append(dict(test="alk_lowdof_seams_dp_order_sensitivity", case=what, device_dp_error=e_dp,
                                                          reference_dp_under_one_ulp=floor, device_H_error=e["H"], device_g_error=e["g"]))
                                print("%s: dp %.3e, the reference's own dp under one-ulp changes of H, g %.3e" % (what, e_dp, floor))
                                assert e_dp < 10.0 * floor, (what, e_dp, floor)
                        if not tight and not materialize and m.family == K.LOW:
                            b.set_math_mode(mtf_amd.MATH_FAST)
                            ff, gf, Hf = b.iterate(sm)
                            b.set_math_mode(mtf_amd.MATH_REPLAY)
                            worst[what.split(" ", 1)[1] + " fast"] = _check(ff[0], gf[0], Hf[0], rec, m.am, (1e-8, 2e-6, 2e-6), what + " MATH_FAST")
                finally:
                    b.close()
    if worst:
        parity_record.append(dict(test="alk_lowdof_seams_one_pass", case=cid, nblk=c.nblk, **worst))


# ================================================================================================ Part B
BATCH_SHAPES = [(5, 7), (7, 9), (33, 31), (32, 33), (91, 91)]      # N = 35, 63, 1023, 1056; 8281: nine partial rows per target
BATCH_REGIONS = ("inside", "right", "quad")


@pytest.mark.parametrize("shape", BATCH_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", K.MODELS, ids=K.model_name)
def test_one_pass_in_a_batch_of_three(oracle, gpu_ctx, frame, frame2, model, shape):
    """`inside`, `right` and `quad` as three targets of one batch -- odd pixel counts against the target-major strides of every per-pixel
    array and of the partial rows (at 91 x 91 target t's nine rows start at row 9 t), and a projective region next to a square one: on the
    homography it clears the batch-wide unit_z, so the square target runs k_alk_pass's general branch too -- each against its own
    single-target reference, at the device-grid bounds"""
    resx, resy = shape
    if shape == (91, 91):
        assert K.fused_decomposition(resx * resy, 3)[0] == K.fused_decomposition(resx * resy, 1)[0] == 9
    corners = np.stack([K.REGIONS[r] for r in BATCH_REGIONS])
    start = K.start_state(model)
    for materialize in (1, 0):
        for run in _runs(model):
            b = _batch(gpu_ctx, frame, model, resx, resy, corners)
            try:
                for k, (label, p) in enumerate(run):
                    sm = _sm(model, p, materialize)
                    if k == 0:
                        gpu_ctx.set_image(frame)
                        b.init_template(sm)
                        gpu_ctx.set_image(frame2)
                    b.set_state(np.tile(start, (3, 1)))
                    W = b.get_warp()
                    f, g, H = b.iterate(sm)
                    for t, region in enumerate(BATCH_REGIONS):
                        ref = K.region_reference(oracle, frame, frame2, model, resx, resy, region, warp=None if model.family == K.ALK else W[t])
                        _check(f[t], g[t], H[t], ref["recs"][label], model.am, LOOSE, "%s %dx%d target %d (%s) %s materialize=%d" % (
                            K.model_name(model), resx, resy, t, region, label, materialize))
            finally:
                b.close()


# ================================================================================================ Part C
def _track(gpu_ctx, frame, frame2, m, resx, resy, regions, materialize=0, **kw):
    corners = np.stack([K.REGIONS[r] for r in regions])
    b = _batch(gpu_ctx, frame, m, resx, resy, corners)
    try:
        sm = _sm(m, K.loop_params(m), materialize, **kw)
        b.init_template(sm)
        gpu_ctx.set_image(frame2)
        b.track_trace(2 * K.LOOP["max_iters"])
        n_it, final = b.track(sm)
        recs = b.read_track_trace(n_it)
        state = b.get_state().copy()
        b.track_trace(0)
        return n_it, final, recs, state
    finally:
        b.close()


def _first_pass_of_the_loop(oracle, frame, frame2, m, resx, resy, region, recs, final, parity_record, what):
    """the first non-undo record of one target against the reference's first pass, its solve against the reference's solver on the same
    system, and -- where the reference converged inside the frame -- the final corners"""
    run = K.full_run(oracle, frame, frame2, m, resx, resy, region)
    o = run["log"][0]
    assert not o["undo"]
    d0 = [r for r in recs if not r["undo"]][0]
    # the one-launch loop of first-order ICLK works from the constant template Hessian and may record none (include/mtfhip.h)
    if m.sm != K.ICLK or m.family == K.ALK:
        assert d0["has_H"], what
    eH = K.rel(d0["H"], o["H"]) if d0["has_H"] else 0.0
    eg = K.rel(d0["g"], o["g"])
    print("%s: H %.3e g %.3e" % (what, eH, eg))
    assert eH < 1e-5 and eg < 1e-5, (what, eH, eg)
    lm = bool(m.extra.get("leven_marq"))
    if d0["has_H"]:
        # the device's solve is held to the reference's SOLVER on the device's own system (damped as the search method damps it), both
        # measured against an extended-precision solution; ten times the reference solver's error is the room for another
        # backward-stable elimination order
        Hs = np.array(d0["H"], dtype=np.float64)
        if lm:
            Hs[np.diag_indices(Hs.shape[0])] += d0["lm_delta"] * np.diag(Hs)
        exact = K.long_double_solve(Hs, -d0["g"])
        assert exact is not None, what
        err_ref = float(np.linalg.norm(np.asarray(-oracle.colpiv_qr_solve(Hs, d0["g"]) - exact, dtype=np.float64)))
        err_dev = float(np.linalg.norm(np.asarray(d0["dp"] - exact, dtype=np.float64)))
        parity_record.append(dict(test="alk_lowdof_seams_loop_solve", case=what, reference_solver_error=err_ref, device_solver_error=err_dev,
                                  dp_norm=float(np.linalg.norm(d0["dp"]))))
        print("%s: solve error device %.3e reference %.3e |dp| %.3e" % (what, err_dev, err_ref, np.linalg.norm(d0["dp"])))
        assert err_dev <= 10.0 * err_ref + 1e-12, (what, err_dev, err_ref)
    if K.corners_compared(m) and region in K.CORNER_REGIONS:
        assert K.converged(run), what
        np.testing.assert_allclose(final, np.asarray(run["corners"]).reshape(4, 2).T, rtol=0, atol=2e-4, err_msg=what)


def _loop_equals_its_single_passes(gpu_ctx, frame, frame2, m, resx, resy, region, parity_record):
    """Batch.track with max_iters = n against n calls of one pass each (max_iters = 1): corners and state bit for bit; every pass's
    recorded H and g against Batch.iterate at the state the pass ran at, 1e-12 (the finish kernel's three-run sum of the partial rows
    against the host's assembly of the same rows, which adds them in row order) -- tests/test_gpu_alk.py::
    test_device_loop_equals_single_passes_from_the_host, tests/test_gpu_lowdof.py::test_device_loop_equals_single_passes_and_itself.

    g is held against max(|g|, g_scale), the scale it cancels at (lk_seam_cases.g_scale, as in Part A): the two orders of the same nine
    to twenty-five rows differ in the last bits of the sums, and NCC's g is a difference of quotients of those sums that shrinks with
    every pass of a converging loop -- against |g| alone the same last bits measured up to 7.7e-10 at the third pass (ESM NCC isometry,
    91 x 91; SSD 1e-15), while a row left out or added twice is an error of a ninth to a twenty-fifth at either scale.  Both figures are
    recorded."""
    n_it, final, recs, state = _track(gpu_ctx, frame, frame2, m, resx, resy, (region,), materialize=1)
    n = int(n_it[0])
    assert 1 <= n <= K.LOOP["max_iters"] and len(recs[0]) == n
    b = _batch(gpu_ctx, frame, m, resx, resy, K.REGIONS[region][None])
    try:
        one = _sm(m, K.loop_params(m), 1, max_iters=1)
        b.init_template(one)
        gpu_ctx.set_image(frame2)
        for k in range(n):
            f, g, H = b.iterate(one)
            r = recs[0][k]
            dg = float(np.linalg.norm(g[0] - r["g"]))
            eg_own = dg / max(float(np.linalg.norm(r["g"])), 1e-300)
            eg = dg / max(float(np.linalg.norm(r["g"])), K.g_scale(dict(H=H[0], f=f[0]), m.am), 1e-300)
            eH = K.rel(H[0], r["H"]) if r["has_H"] else 0.0
            what = "%s %dx%d %s pass %d" % (K.model_name(m), resx, resy, region, k)
            print("%s: loop against iterate H %.3e g %.3e (of |g| alone %.3e)" % (what, eH, eg, eg_own))
            parity_record.append(dict(test="alk_lowdof_seams_loop_vs_iterate", case=what, H=eH, g=eg, g_of_its_own_norm=eg_own))
            assert eg < 1e-12 and eH < 1e-12, (what, eg, eH, eg_own)
            n1, c1 = b.track(one)
            assert int(n1[0]) == 1
            assert np.array_equal(c1[0], recs[0][k]["corners"]), k
        assert np.array_equal(c1[0], final[0]) and np.array_equal(b.get_state()[0], state[0])
    finally:
        b.close()


@pytest.mark.parametrize("shape", K.LOOP_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", K.LOOP_MODELS, ids=K.model_name)
def test_device_loop_on_a_projective_region(oracle, gpu_ctx, frame, frame2, model, shape, parity_record):
    """(i) one `quad` target: on the homography k_alk_pass takes its points from INIT_HXY / INIT_Z (unit_z = 0), the low-order models run
    on the re-homogenised projective lattice; (ii) [inside, quad, right]: the projective region clears the batch-wide unit_z, next to a
    target across the frame edge, which is held to the first pass and to the solve alone.  On the BIG shapes the finish kernels sum 9, 9, 17 and 25 partial rows per target with 256 threads in
    three runs: there the loop is also held to its own single passes (Levenberg-Marquardt keeps its state across the passes of one call
    only, so its cases are not)"""
    resx, resy = shape
    for regions in K.LOOP_REGION_SETS:
        n_it, final, recs, state = _track(gpu_ctx, frame, frame2, model, resx, resy, regions)
        for t, region in enumerate(regions):
            # (nothing is asserted of where the target across the edge ends: under NCC the additive methods diverge there in the reference
            # itself -- |dp| 1e10 from the fifth pass on -- and a region that leaves the frame altogether is NCC's 0 / 0)
            if region in K.CORNER_REGIONS:
                assert np.all(np.isfinite(final[t])) and np.all(np.isfinite(state[t])), (regions, t)
            _first_pass_of_the_loop(oracle, frame, frame2, model, resx, resy, region, recs[t], final[t], parity_record,
                                    "%s %dx%d B=%d target %d (%s)" % (K.model_name(model), resx, resy, len(regions), t, region))
    if shape in K.BIG_SHAPES and not model.extra.get("leven_marq"):
        assert K.fused_decomposition(resx * resy, 1)[0] > 8
        _loop_equals_its_single_passes(gpu_ctx, frame, frame2, model, resx, resy, "quad", parity_record)


@pytest.mark.parametrize("shape", K.LOOP_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", [m for m in K.LOOP_MODELS if m.am == K.SSD], ids=K.model_name)
def test_device_loop_next_to_a_region_outside_the_frame(oracle, gpu_ctx, frame, frame2, model, shape, parity_record):
    """(iii) [inside, outside], SSD: the outside target's system is H = 0, g = 0 -- its records are finite and its corners stay, bit for
    bit, where they started -- and its neighbour's first pass has the bits of the same target tracked alone"""
    resx, resy = shape
    n_it, final, recs, state = _track(gpu_ctx, frame, frame2, model, resx, resy, K.LOOP_OUTSIDE_SET)
    assert np.all(np.isfinite(final)) and np.all(np.isfinite(state))
    assert len(recs[1]) >= 1
    for r in recs[1]:
        assert np.all(np.isfinite(r["g"])) and np.all(np.isfinite(r["dp"])) and np.all(np.isfinite(r["H"])) and np.isfinite(r["f"])
    assert np.array_equal(final[1], K.REGIONS["outside"])
    n1, final1, recs1, state1 = _track(gpu_ctx, frame, frame2, model, resx, resy, ("inside",))
    a, a1 = [r for r in recs[0] if not r["undo"]][0], [r for r in recs1[0] if not r["undo"]][0]
    for q in ("H", "g", "dp", "corners"):
        assert np.array_equal(a[q], a1[q]), q
    assert a["f"] == a1["f"] and a["has_H"] == a1["has_H"]
    _first_pass_of_the_loop(oracle, frame, frame2, model, resx, resy, "inside", recs[0], final[0], parity_record,
                            "%s %dx%d B=2 target 0 (inside, next to outside)" % (K.model_name(model), resx, resy))
