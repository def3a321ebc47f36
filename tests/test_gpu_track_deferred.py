"""Deferred materialisation of the device-side LK loop (track_loop_chunked, api_track.hip): with MTFHIP_TRACK_DEFER_MAT unset / 1 the passes before a target's
last run the non-materialising kernel and the interface arrays are written once -- by the pass the host knows to be the last, or by one
trailing launch for the targets the finish stopped earlier; with 0 every pass materialises.  Both loops take the same cut of the pixel
pass and the same arithmetic, so everything a caller can see after the call is the same BITS."""
import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth

pytestmark = pytest.mark.gpu

MODELS = [
    (L.SM_ESM, L.AM_SSD, L.SSM_HOMOGRAPHY, dict()),
    (L.SM_FCLK, L.AM_SSD, L.SSM_AFFINE, dict(chained_warp=0)),
    (L.SM_ESM, L.AM_NCC, L.SSM_HOMOGRAPHY, dict()),
    (L.SM_FCLK, L.AM_NCC, L.SSM_AFFINE, dict()),
]
MODEL_IDS = ["esm_ssd_hom", "fclk_ssd_aff_unchained", "esm_ncc_hom", "fclk_ncc_aff"]
NAMES = ("n_iters", "corners", "state", "It", "dIt_dx", "Jt", "n_iters_2", "corners_2", "state_2", "It_2", "dIt_dx_2", "Jt_2")


def _corners(B, size):
    return np.stack([synth.square_corners(200 + 31 * t, 230 + 17 * t, float(size)) for t in range(B)])


def _arrays(b):
    return [b.read(L.BUF_IT).copy(), b.read(L.BUF_DIT_DX).copy(), b.read(L.BUF_JT).copy()]


def _run(gpu_ctx, frame, frame2, am, ssm, sm_kind, params, resx, resy, corners, start=None, batch_kw=None, trace=0):
    """template on `frame`, two calls of the device-side loop on `frame2` (the second behind set_region(c1 + 0.4)); -> what a caller sees"""
    B = len(corners)
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, am, ssm, resx, resy, B, **(batch_kw or {}))
    try:
        b.set_corners(corners)
        sm = mtf_amd.sm_desc(sm_kind, materialize=1, **params)
        b.init_template(sm)
        gpu_ctx.set_image(frame2)
        if trace:
            b.track_trace(trace)
        if start is not None:
            b.set_region(start, sm)
        n1, c1 = b.track(sm)
        out = [n1.copy(), c1.copy(), b.get_state().copy()] + _arrays(b)
        b.set_region(c1 + 0.4, sm)
        n2, c2 = b.track(sm)
        out += [n2.copy(), c2.copy(), b.get_state().copy()] + _arrays(b)
        return out, (b.track_queues(sm), b.track_targets_per_launch(sm))
    finally:
        b.close()


def _both_arms_equal(monkeypatch, *args, **kw):
    res = {}
    for arm in ("0", "1"):
        monkeypatch.setenv("MTFHIP_TRACK_DEFER_MAT", arm)
        res[arm], plan = _run(*args, **kw)
    print("n_iters", res["0"][0].tolist(), res["1"][0].tolist(), "second call", res["0"][6].tolist(), res["1"][6].tolist(), "queues, targets per launch", plan)
    for name, a, c in zip(NAMES, res["0"], res["1"]):
        assert a.shape == c.shape and np.array_equal(a, c), name
    return res["0"], plan


@pytest.mark.parametrize("sm_kind,am,ssm,extra", MODELS, ids=MODEL_IDS)
@pytest.mark.parametrize("max_iters", [1, 2, 3, 9])
def test_runs_out_of_passes(gpu_ctx, frame, frame2, monkeypatch, sm_kind, am, ssm, extra, max_iters):
    """an unreachable epsilon: the pass the host knows to be the last is the only one that materialises; the gate opens at three passes (one
    and two keep the loop that materialises every pass)"""
    params = dict(leven_marq=0, max_iters=max_iters, epsilon=-1.0)
    params.update(extra)
    out, _ = _both_arms_equal(monkeypatch, gpu_ctx, frame, frame2, am, ssm, sm_kind, params, 40, 40, _corners(3, 60))
    assert (out[0] == max_iters).all() and (out[6] == max_iters).all()


def _mixed_start(gpu_ctx, frame, frame2, monkeypatch, am, ssm, sm_kind, params, res, corners):
    """start regions whose targets stop at different passes: target 0 on its converged region (found with the loop that materialises every
    pass), the others displaced by growing amounts, the last far enough to use every pass"""
    monkeypatch.setenv("MTFHIP_TRACK_DEFER_MAT", "0")
    B = len(corners)
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, am, ssm, res, res, B)
    try:
        b.set_corners(corners)
        sm = mtf_amd.sm_desc(sm_kind, materialize=1, **dict(params, max_iters=40, epsilon=1e-12))
        b.init_template(sm)
        gpu_ctx.set_image(frame2)
        c0 = corners.copy()
        for _ in range(6):   # (set_region refreshes the template Jacobian on the new grid: the fixed point is found on that grid)
            b.set_region(c0, sm)
            n, c = b.track(sm)
            c0 = c.reshape(corners.shape).copy()
            if n[0] == 1:
                break
        start = corners.copy()
        start[0] = c0[0]
        for t, d in zip(range(1, B - 1), (0.35, 2.0)):
            start[t] = c0[t] + d
        # the last target: the smallest of these displacements from which the loop that materialises every pass uses all of them
        sm_run = mtf_amd.sm_desc(sm_kind, materialize=1, **params)
        for d in (9.0, 13.0, 18.0, 25.0, 35.0, 50.0):
            start[B - 1] = c0[B - 1] + d
            b.set_region(start, sm_run)
            n, _ = b.track(sm_run)
            if n[B - 1] == params["max_iters"]:
                break
    finally:
        b.close()
    return start


@pytest.mark.parametrize("sm_kind,am,ssm,extra", MODELS, ids=MODEL_IDS)
def test_targets_stop_at_different_passes(gpu_ctx, frame, frame2, monkeypatch, sm_kind, am, ssm, extra):
    """a reachable epsilon: the targets the finish stops behind a lean pass get their arrays from the trailing launch, at the warp of
    their own last pass; the one that runs out of passes from the last pass itself"""
    params = dict(leven_marq=0, max_iters=9, epsilon=1e-5)
    params.update(extra)
    corners = _corners(4, 60)
    start = _mixed_start(gpu_ctx, frame, frame2, monkeypatch, am, ssm, sm_kind, params, 40, corners)
    out, _ = _both_arms_equal(monkeypatch, gpu_ctx, frame, frame2, am, ssm, sm_kind, params, 40, 40, corners, start=start)
    n = out[0].tolist()
    # (the arm that materialises every pass shows the spread; without it the trailing launch is not under test)
    assert len(set(n)) >= 3 and 1 in n and 9 in n, n


@pytest.mark.parametrize("sm_kind,am,ssm,extra", MODELS, ids=MODEL_IDS)
@pytest.mark.parametrize("epsilon", [-1.0, 1e-5])
def test_chunk_and_queue_seams(gpu_ctx, frame, frame2, monkeypatch, sm_kind, am, ssm, extra, epsilon):
    """chunks of two targets with a ragged last one, on two queues: every chunk has its own lean / full pair and its own trailing launch"""
    monkeypatch.setenv("MTFHIP_TRACK_CHUNK_PX", str(2 * 24 * 24 + 10))
    monkeypatch.setenv("MTFHIP_TRACK_STREAMS", "12")
    params = dict(leven_marq=0, max_iters=9, epsilon=epsilon)
    params.update(extra)
    corners = _corners(5, 40)
    start = corners + np.array([0.0, 0.3, 0.8, 1.5, 4.0])[:, None, None]
    _, plan = _both_arms_equal(monkeypatch, gpu_ctx, frame, frame2, am, ssm, sm_kind, params, 24, 24, corners, start=start)
    assert plan == (2, 2), plan


@pytest.mark.parametrize("epsilon", [-1.0, 1e-5])
def test_row_that_is_not_a_whole_workgroup(gpu_ctx, frame, frame2, monkeypatch, epsilon):
    """50 x 30 = 1500 points: five full rows of 256 and a partial one, a non-square lattice"""
    params = dict(leven_marq=0, max_iters=9, epsilon=epsilon)
    corners = synth.square_corners(256, 240, 70.0)[None]
    _both_arms_equal(monkeypatch, gpu_ctx, frame, frame2, L.AM_SSD, L.SSM_HOMOGRAPHY, L.SM_ESM, params, 50, 30, corners, start=corners + 0.6)


@pytest.mark.parametrize("am,params,batch_kw,trace", [
    (L.AM_SSD, dict(leven_marq=1, max_iters=9, epsilon=1e-5), dict(), 0),
    (L.AM_SSD, dict(leven_marq=0, max_iters=9, epsilon=1e-5), dict(), 12),
    (L.AM_SCV, dict(leven_marq=0, max_iters=9, epsilon=1e-5), dict(mi_n_bins=64), 0),
], ids=["leven_marq", "track_trace", "scv"])
def test_outside_the_gate_the_knob_changes_nothing(gpu_ctx, frame, frame2, monkeypatch, am, params, batch_kw, trace):
    """Levenberg-Marquardt, a batch with the debug trace on and SCV keep the loop that materialises every pass whatever the knob says"""
    corners = _corners(3, 60)
    _both_arms_equal(monkeypatch, gpu_ctx, frame, frame2, am, L.SSM_HOMOGRAPHY, L.SM_ESM, params, 40, 40, corners, start=corners + 0.5,
                     batch_kw=batch_kw, trace=trace)
