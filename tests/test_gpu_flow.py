"""GPU: the device optical flow (k_ncc_flow, mtfhip_ncc_estimate_optical_flow[_dev|_trace]) and sm.GridTrackerFlow against the NumPy restatement of
NCC::estimateOpticalFlow / nt::GridTrackerFlow (tests/helpers/flow_ref.py), at the smallest shapes where the kernel can go wrong."""
import os
import sys

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import host, synth
from mtf_amd.sm import GridTrackerFlow, least_squares_estimator

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import flow_cases as FC   # noqa: E402
import flow_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 0.01
# replay mode, a pass that starts from the reference's own lattice (the first): the bounds and relative definitions of
# tests/test_gpu_alk.py::test_one_pass_parity -- only the order of the N-wide sums differs
F_REL, H_REL, G_REL, STEP_REL, STEP_ABS = 1e-12, 1e-9, 1e-10, 1e-6, 1e-12
# replay mode, later passes: see test_trace_parity's docstring
# (measured maxima: f 6.6e-8, H 5.0e-6, g 2.9e-7, step 3.5e-6 px, all at 2 x 2; from 7 x 5 up f 9.3e-10, H 2.3e-7, g 3.0e-8, step 6.8e-8 px)
LATER_F_REL, LATER_H_REL, LATER_G_REL, LATER_STEP_PX = 2.5e-7, 1e-5, 1e-6, 1e-5
PT_ULP, REGION_ATOL = 4e-5, 1e-4          # tests/test_gpu_grid.py
FAST_STEP_PX = 1e-5                       # the project's tolerance-mode bound (tests/test_gpu_lowdof.py)
MODES = [L.MATH_REPLAY, L.MATH_FAST]
MODE_IDS = ["replay", "fast"]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / n) if n > 0 else float(np.linalg.norm(a - b))


def set_frames(ctx):
    f0, f1 = FC.frames()
    ctx.set_image(f0); ctx.keep_prev(); ctx.set_image(f1)


def compare(tag, dev, ref, math, worst):
    """a device result (curr_pts, n_iters, status, trace) against the reference's; every figure goes into `worst`, what misses a bound into
    worst["failed"], which the caller asserts empty after it has printed and recorded the figures"""
    cp, ni, st, tr = dev
    rcp, rni, rst, logs = ref
    FC.assert_valid(logs, EPS)
    assert np.array_equal(ni, rni), (tag, ni, rni)
    assert np.array_equal(st, rst), (tag, st, rst)
    for p, log in enumerate(logs):
        for k, rec in enumerate(log):
            t = tr[p, k]
            flow, f, g, H = t[0:2], t[2], t[3:5], np.array([[t[5], t[6]], [t[6], t[7]]])
            if not np.all(np.isfinite(rec["opt_flow"])):
                assert not np.all(np.isfinite(flow)), (tag, p, k)
                continue
            g_scale = max(np.linalg.norm(rec["df_dx"]), np.sqrt(abs(np.trace(rec["H"]))))
            e = dict(f=rel(f, rec["f"]), H=rel(H, rec["H"]), g=float(np.linalg.norm(g - rec["df_dx"]) / g_scale), step=rel(flow, rec["opt_flow"]),
                     step_px=float(np.abs(flow - rec["opt_flow"]).max()))
            which = "first" if k == 0 else "later"
            for name, v in e.items():
                worst[which][name] = max(worst[which].get(name, 0.0), v)
            if math == L.MATH_FAST:
                good = e["step_px"] < FAST_STEP_PX
            elif k == 0:
                good = e["f"] < F_REL and e["H"] < H_REL and e["g"] < G_REL and (e["step"] < STEP_REL or e["step_px"] < STEP_ABS)
            else:
                good = e["f"] < LATER_F_REL and e["H"] < LATER_H_REL and e["g"] < LATER_G_REL and e["step_px"] < LATER_STEP_PX
            if not good:
                worst["failed"].append((tag, p, k, e))
        assert not tr[p, len(log):].any(), (tag, p)          # passes the point did not run stay zero
    nan = np.isnan(rcp)
    assert np.array_equal(np.isnan(cp), nan), tag
    d = float(np.abs(cp[~nan].astype(np.float64) - rcp[~nan].astype(np.float64)).max()) if (~nan).any() else 0.0
    worst["pts"] = max(worst.get("pts", 0.0), d)
    if not d <= (PT_ULP if math == L.MATH_REPLAY else REGION_ATOL):
        worst["failed"].append((tag, "final points", d))


@pytest.mark.parametrize("math", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("const_grad", [False, True], ids=["grad_curr", "const_grad"])
@pytest.mark.parametrize("win", FC.WINDOWS, ids=["%dx%d" % w for w in FC.WINDOWS])
def test_trace_parity(gpu_ctx, parity_record, win, const_grad, math):
    """Every pass of every point against the reference's record: interior points (and the point wholly outside) through their whole trajectory,
    the border points with max_iters 1 and 2 (their full trajectories do not converge on the CPU either: a comparison of final points would
    measure chaos, not the kernel).
    Replay mode.  The first pass samples the reference's own lattice, bit for bit, and meets test_one_pass_parity's bounds.  A later pass
    cannot: its lattice is the first one plus a step that differs from the reference's in the last bits (the order of the N-wide sums), a
    coordinate that moves by one ulp (5.7e-14 at x = 300) changes where x +- 1e-8 round to, and the central difference divides that by 2e-8 -- a
    relative change of up to ~3e-6 of that pixel's gradient, random from pixel to pixel.  H, g and the step of later passes therefore agree to
    about 1e-6 / sqrt(N) relative, not to 1e-9, and f follows the lattice.  Measured maxima over all cases (all at the four-sample window,
    whose 2 x 2 system amplifies most): f 6.6e-8, H 5.0e-6, g 2.9e-7, step 3.5e-6 px; the bounds are at most 4 x those and the step's is
    tolerance mode's 1e-5 px.  From 7 x 5 up: f 9.3e-10, H 2.3e-7, g 3.0e-8, step 6.8e-8 px.
    Tolerance mode: every step within 1e-5 px, final points within 1e-4 px.  n_iters and status are equal in both modes."""
    set_frames(gpu_ctx)
    worst = dict(first={}, later={}, failed=[])
    pts = np.asarray(FC.interior_points(win, const_grad) + [FC.OUTSIDE], dtype=np.float32)
    dev = gpu_ctx.estimate_optical_flow(pts, win, 30, EPS, const_grad, math, trace=True)
    compare("interior", dev, FC.ref_flow(FC.key(pts), win, 30, const_grad), math, worst)
    bpts = np.asarray(FC.border_points(win, const_grad), dtype=np.float32).reshape(-1, 2)
    for mi in ((1, 2) if len(bpts) else ()):
        dev = gpu_ctx.estimate_optical_flow(bpts, win, mi, EPS, const_grad, math, trace=True)
        compare("border max_iters %d" % mi, dev, FC.ref_flow(FC.key(bpts), win, mi, const_grad), math, worst)
    # the trace form and the plain form are one kernel
    plain = gpu_ctx.estimate_optical_flow(pts, win, 30, EPS, const_grad, math)
    dev = gpu_ctx.estimate_optical_flow(pts, win, 30, EPS, const_grad, math, trace=True)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(plain, dev[:3]))
    print("flow parity win %s const_grad %d %s: %s" % (win, const_grad, MODE_IDS[math], worst))
    parity_record.append(dict(test="flow_trace_parity", win=list(win), const_grad=int(const_grad), math=MODE_IDS[math], **{
        "%s_%s" % (w, k): v for w in ("first", "later") for k, v in worst[w].items()}, pts=worst["pts"]))
    assert not worst["failed"], worst["failed"]


@pytest.mark.parametrize("math", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n", [1, 3, 100])
def test_batches(gpu_ctx, n, math):
    """members of a batch stop at different passes, one of them (the second) is wholly outside: every workgroup is on its own"""
    set_frames(gpu_ctx)
    pts = FC.batch_points(n)
    rcp, rni, rst, logs = FC.ref_flow(FC.key(pts), (10, 10), 30, False)
    FC.assert_valid(logs, EPS)
    cp, ni, st = gpu_ctx.estimate_optical_flow(pts, (10, 10), 30, EPS, False, math)
    assert np.array_equal(ni, rni) and np.array_equal(st, rst)
    if n > 1:
        assert st[1] == L.FLOW_NONFINITE and ni[1] == 1 and np.isnan(cp[1]).all() and len(set(ni.tolist())) > 1
    nan = np.isnan(rcp)
    assert np.array_equal(np.isnan(cp), nan)
    d = float(np.abs(cp[~nan].astype(np.float64) - rcp[~nan]).max())
    print("flow batch %d %s: final points %.3e px" % (n, MODE_IDS[math], d))
    assert d <= (PT_ULP if math == L.MATH_REPLAY else REGION_ATOL)


def test_non_finite_start_point(gpu_ctx):
    set_frames(gpu_ctx)
    pts = np.array([[np.nan, 100.0], FC.INTERIOR[0], [100.0, np.inf], [3e38, -3e38]], dtype=np.float32)
    for math in MODES:
        cp, ni, st = gpu_ctx.estimate_optical_flow(pts, (10, 10), 30, EPS, False, math)
        assert st[0] == 0 and ni[0] == 0 and st[2] == 0 and ni[2] == 0 and np.isnan(cp[[0, 2]]).all()
        assert st[1] == L.FLOW_CONVERGED and st[3] == 0 and ni[3] == 1       # a finite point far off the frame: a flat window, pass 1


# ------------------------------------------------------------------ frame layouts
PW, R0, C0 = 640, 5, 7          # the parent's pitch, the view's origin in it


@pytest.mark.parametrize("math", MODES, ids=MODE_IDS)
def test_frame_layouts(gpu_ctx, math):
    """the same batch on a packed frame, a padded host frame (row stride != width) and borrowed device views with an origin and a pitch:
    the current image as a view, and -- through swap_prev -- the previous image as a view.  Equal arrays."""
    import torch
    f0, f1 = FC.frames()
    pts = np.vstack([FC.batch_points(3), np.asarray(FC.BORDER, dtype=np.float32)])
    args = ((7, 5), 4, EPS, False, math)
    set_frames(gpu_ctx)
    want = gpu_ctx.estimate_optical_flow(pts, *args)
    set_frames(gpu_ctx)
    cg = gpu_ctx.estimate_optical_flow(pts, (7, 5), 4, EPS, True, math)

    def padded(f):
        big = np.full((f.shape[0], PW), 77.0, dtype=np.float32)
        big[:, :f.shape[1]] = f
        return big[:, :f.shape[1]]
    gpu_ctx.set_image(padded(f0)); gpu_ctx.keep_prev(); gpu_ctx.set_image(padded(f1))
    got = gpu_ctx.estimate_optical_flow(pts, *args)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(want, got))

    def parent(f):
        big = np.full((f.shape[0] + 2 * R0, PW), 33.0, dtype=np.float32)
        big[R0:R0 + f.shape[0], C0:C0 + f.shape[1]] = f
        return torch.from_numpy(big).to("cuda:0")
    t0, t1 = parent(f0), parent(f1)
    torch.cuda.synchronize()

    def borrow(t):
        gpu_ctx.set_image_device(t.data_ptr() + 4 * (R0 * PW + C0), f0.shape[0], f0.shape[1], PW, keep=t)
    try:
        # the current image a borrowed view, the previous one the context's packed clone of a borrowed view
        borrow(t0); gpu_ctx.keep_prev(); borrow(t1)
        got = gpu_ctx.estimate_optical_flow(pts, *args)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(want, got))
        # the previous image a borrowed view (pitch 640, origin (5, 7)), the current one the swapped clone
        borrow(t1); gpu_ctx.keep_prev(); borrow(t0); gpu_ctx.swap_prev()
        got = gpu_ctx.estimate_optical_flow(pts, *args)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(want, got))
        got = gpu_ctx.estimate_optical_flow(pts, (7, 5), 4, EPS, True, math)      # const_grad: the gradient comes from that view
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(cg, got))
    finally:
        gpu_ctx.set_image(f1)      # nothing of the context points into the parents any more
        gpu_ctx.keep_prev(); gpu_ctx.set_image(f1)


# ------------------------------------------------------------------ the tracker
QUAD = synth.square_corners(256.0, 256.0, 280) + np.array([[3.0, -2.0, 5.0, -4.0], [-1.5, 2.5, 4.0, -3.0]])   # REGIONS["quad"], tests/test_gpu_grid.py


def tracker_frames():
    """(seed 82: with the restatement on the CPU, no pass of any point of either sequence below comes within 11 % of epsilon; the seeds
    77 .. 81 each have one within 4 %, which assert_valid refuses)"""
    f0, _ = FC.frames()
    rng = np.random.default_rng(82)
    out, cur = [], f0
    for _ in range(3):
        cur = synth.warp_frame(cur, synth.random_small_homography(rng, 0.15), FC.CENTRE)
        out.append(cur)
    return f0, out


def ref_grid_pts(gs):
    import numpy_ref as NR
    return lambda region: NR.grid_layout(region, gs, gs, 1, 1, 0, 0)[0]


@pytest.mark.parametrize("grid_ssm", [L.SSM_HOMOGRAPHY, L.SSM_AFFINE], ids=["homography", "affine"])
def test_tracker_follows_reference(gpu_ctx, grid_ssm):
    """grid 5, window 10, an interior region: three frames, a set_region, one more frame; bounds of test_python_grid_tracker_follows_oracle"""
    gs = 5
    est = least_squares_estimator(grid_ssm)
    f0, frames = tracker_frames()
    o = R.GridTrackerFlowRef(ref_grid_pts(gs), est, grid_ssm == L.SSM_AFFINE, (10, 10), 30, EPS, False)
    o.set_image(f0); o.initialize(QUAD)
    gpu_ctx.set_image(f0)
    g = GridTrackerFlow(gpu_ctx, grid_size=gs, search_window=10, grid_ssm=grid_ssm, estimator=est, math=L.MATH_REPLAY)
    g.initialize(QUAD)
    np.testing.assert_allclose(g.prev_pts, o.prev_pts, rtol=0, atol=PT_ULP)

    def step(k, f):
        gpu_ctx.set_image(f); o.set_image(f)
        before = g.prev_pts.copy()
        g.update(); o.update()
        FC.assert_valid(o.logs, EPS)
        assert np.array_equal(g.n_iters, o.n_iters) and np.array_equal(g.status, o.status), k
        np.testing.assert_allclose(g.curr_pts, o.curr_pts, rtol=0, atol=PT_ULP, err_msg="curr_pts, frame %d" % k)
        np.testing.assert_allclose(g.prev_pts, o.prev_pts, rtol=0, atol=PT_ULP, err_msg="prev_pts, frame %d" % k)
        np.testing.assert_allclose(g.ssm_update, o.ssm_update, rtol=0, atol=2e-5, err_msg="ssm_update, frame %d" % k)
        np.testing.assert_allclose(g.get_region(), o.region, rtol=0, atol=REGION_ATOL, err_msg="region, frame %d" % k)
        assert np.array_equal(g.prev_pts, g.curr_pts) and not np.array_equal(before, g.prev_pts)      # the points drift
    for k, f in enumerate(frames):
        step(k + 1, f)
    moved = g.get_region() + np.array([[1.5], [-0.75]])
    g.set_region(moved); o.set_region(moved)
    np.testing.assert_allclose(g.prev_pts, o.prev_pts, rtol=0, atol=PT_ULP)
    np.testing.assert_allclose(g.prev_pts, g.grid_pts(moved), rtol=0, atol=PT_ULP)       # back on the grid
    step(9, frames[0])


@pytest.mark.parametrize("grid_ssm", [L.SSM_HOMOGRAPHY, L.SSM_AFFINE], ids=["homography", "affine"])
def test_cpp_driver_equals_python_driver(gpu_ctx, grid_ssm):
    """mtf::hip::GridFlow (libmtfhost.so) through the same sequence with the same estimator callback: the Python driver's arrays"""
    est = least_squares_estimator(grid_ssm)
    f0, frames = tracker_frames()
    gpu_ctx.set_image(f0)
    g = GridTrackerFlow(gpu_ctx, grid_size=5, search_window=10, grid_ssm=grid_ssm, estimator=est)
    h = host.CppGridTrackerFlow(grid_size=5, search_window=10, grid_ssm=grid_ssm, estimator=est)
    h.set_image(f0)
    g.initialize(QUAD); h.initialize(QUAD)
    assert np.array_equal(g.prev_pts, h.prev_pts()) and h.pix_mask().all()

    def step(f):
        gpu_ctx.set_image(f); h.set_image(f)
        g.update(); h.update()
        assert np.array_equal(g.curr_pts, h.curr_pts()) and np.array_equal(g.prev_pts, h.prev_pts())
        assert np.array_equal(g.n_iters, h.n_iters()) and np.array_equal(g.status, h.status())
        assert np.array_equal(g.ssm_update, h.ssm_update()) and np.array_equal(g.get_region(), h.get_region())
    for f in frames:
        step(f)
    moved = g.get_region() + np.array([[1.5], [-0.75]])
    g.set_region(moved); h.set_region(moved)
    assert np.array_equal(g.prev_pts, h.prev_pts())
    step(frames[0])
    # the device estimator behind the C++ driver
    p = L.est_params(L.EST_RANSAC, 10.0, 4, True, 200)
    h2 = host.CppGridTrackerFlow(grid_size=5, search_window=10, grid_ssm=grid_ssm, est_params=p, est_seed=5)
    g2 = GridTrackerFlow(gpu_ctx, grid_size=5, search_window=10, grid_ssm=grid_ssm, est_params=p, est_seed=5)
    gpu_ctx.set_image(f0); h2.set_image(f0)
    g2.initialize(QUAD); h2.initialize(QUAD)
    gpu_ctx.set_image(frames[0]); h2.set_image(frames[0])
    g2.update(); h2.update()
    assert np.array_equal(g2.curr_pts, h2.curr_pts()) and np.array_equal(g2.ssm_update, h2.ssm_update())
    assert np.array_equal(g2.pix_mask, h2.pix_mask()) and h2.est_ok == g2.est_ok


def test_cpp_appearance_model_mirror(gpu_ctx):
    """HipAM::estimateOpticalFlow: NCC gives the C ABI's arrays, every other model throws FunctonNotImplemented (AppearanceModel.h:221-226)"""
    f0, f1 = FC.frames()
    pts = FC.batch_points(3)
    set_frames(gpu_ctx)
    want = gpu_ctx.estimate_optical_flow(pts, (7, 5), 30, EPS, False, L.MATH_REPLAY)
    got = host.am_optical_flow(L.AM_NCC, np.ascontiguousarray(f0), np.ascontiguousarray(f1), pts, (7, 5), 30, EPS, False, L.MATH_REPLAY)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(want, got))
    for am in (L.AM_SSD, L.AM_MI, L.AM_SCV):
        with pytest.raises(host.HostError, match="FunctonNotImplemented"):
            host.am_optical_flow(am, np.ascontiguousarray(f0), np.ascontiguousarray(f1), pts)


@pytest.mark.parametrize("method", [L.EST_LEAST_SQUARES, L.EST_RANSAC], ids=["least_squares", "ransac"])
def test_tracker_chained_device_estimator(gpu_ctx, method):
    """with est_params the flow's and the estimator's device-pointer forms run back to back: exactly what the two host-pointer calls give"""
    f0, frames = tracker_frames()
    p = L.est_params(method, 10.0, 4, True, 200)
    gpu_ctx.set_image(f0)
    g = GridTrackerFlow(gpu_ctx, grid_size=5, search_window=10, est_params=p, est_seed=5)
    g.initialize(QUAD)
    for k, f in enumerate(frames[:2]):
        gpu_ctx.set_image(f)
        prev = g.prev_pts.copy()
        region = g.get_region()
        cp, ni, st = gpu_ctx.estimate_optical_flow(prev, (10, 10), 30, EPS, False, L.MATH_FAST)
        e = gpu_ctx.estimate_warp_from_pts(L.SSM_HOMOGRAPHY, prev, cp, p, seed=5 + k)
        g.update()
        assert np.array_equal(g.curr_pts, cp) and np.array_equal(g.n_iters, ni) and np.array_equal(g.status, st)
        assert np.array_equal(g.ssm_update, e.state_update) and np.array_equal(g.pix_mask, e.mask) and g.est_ok == e.ok
        assert g.est_ok and g.pix_mask.shape == (25,) and g.pix_mask.dtype == np.uint8 and g.pix_mask.sum() >= 4
        assert np.array_equal(g.get_region(), mtf_amd.apply_warp_to_pts(L.SSM_HOMOGRAPHY, region, e.state_update))


def test_tracker_non_finite_point_raises(gpu_ctx):
    f0, f1 = FC.frames()
    gpu_ctx.set_image(f0)
    g = GridTrackerFlow(gpu_ctx, grid_size=3, search_window=10)
    region = np.array([[-80.0, 200, 200, -80], [60, 60, 300, 300]])      # the left column of the grid: windows wholly outside
    g.initialize(region)
    gpu_ctx.set_image(f1)
    before = g.prev_pts.copy()
    with pytest.raises(L.LogicError, match="point 0"):
        g.update()
    assert np.array_equal(g.prev_pts, before) and np.array_equal(g.get_region(), region)      # a lost frame changes nothing


def test_refusals(gpu_ctx):
    f0, f1 = FC.frames()
    pts = np.asarray(FC.INTERIOR, dtype=np.float32)
    set_frames(gpu_ctx)
    for win in ((1, 10), (10, 1)):
        with pytest.raises(L.InvalidArgument):
            gpu_ctx.estimate_optical_flow(pts, win)
    with pytest.raises(L.FunctionNotImplemented, match="1024"):
        gpu_ctx.estimate_optical_flow(pts, (33, 32))
    with pytest.raises(L.InvalidArgument):
        gpu_ctx.estimate_optical_flow(pts, max_iters=0)
    with pytest.raises(L.InvalidArgument):
        gpu_ctx.estimate_optical_flow(np.zeros((0, 2), dtype=np.float32))
    gpu_ctx.set_image(np.ascontiguousarray(f1[:400, :480]))              # mismatched shapes
    with pytest.raises(L.InvalidArgument, match="512 x 512"):
        gpu_ctx.estimate_optical_flow(pts)
    mc = synth.make_frame_mc(64, 64)
    gpu_ctx.set_image(mc); gpu_ctx.keep_prev(); gpu_ctx.set_image(mc)   # a 3-channel image
    with pytest.raises(L.FunctionNotImplemented):
        gpu_ctx.estimate_optical_flow(pts)
    c2 = mtf_amd.Context(0)
    try:
        c2.set_image(f0)
        with pytest.raises(L.LogicError, match="previous image"):      # no previous image
            c2.estimate_optical_flow(pts)
    finally:
        c2.close()
    set_frames(gpu_ctx)
    assert gpu_ctx.estimate_optical_flow(pts)[2].tolist() == [1, 1]     # and the context still serves
