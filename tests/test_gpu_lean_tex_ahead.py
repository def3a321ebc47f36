"""The lean replay SSD pass with a row's texels requested one row ahead (fused_lk_body's TEX_AHEAD loop, mtfhip_fused_device.h) against the
materialising pass, which keeps the loop that requests and uses a row's texels in the same iteration.  With MTFHIP_TRACK_DEFER_MAT=1 the
device-side loop runs the lean kernel on every pass but a target's last, with 0 the materialising kernel on every pass; each pixel's
operations and each thread's order of accumulation are the same in both, so everything a caller can see is the same BITS.  The shapes are
the ones at which a reordered row loop can go wrong: no, one and two full 256-pixel rows per workgroup with and without a partial last
row, several workgroups per target with a short last one, waves that change between the interior and the general sampler from one row to
the next, targets that are switched off behind the first row's loads."""
import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth

pytestmark = pytest.mark.gpu

NAMES = ("n_iters", "corners", "state", "warp", "It", "dIt_dx", "Jt")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _run(gpu_ctx, tmpl_frame, run_frame, ssm, sm_kind, params, resx, resy, corners, start):
    B = len(corners)
    gpu_ctx.set_image(tmpl_frame)
    b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, ssm, resx, resy, B)
    try:
        b.set_corners(corners)
        sm = mtf_amd.sm_desc(sm_kind, materialize=1, **params)
        b.init_template(sm)
        gpu_ctx.set_image(run_frame)
        if start is not None:
            b.set_region(start, sm)
        n, c = b.track(sm)
        out = [n.copy(), c.copy(), b.get_state().copy(), b.get_warp().copy(),
               b.read(L.BUF_IT).copy(), b.read(L.BUF_DIT_DX).copy(), b.read(L.BUF_JT).copy()]
        return out, (b.track_queues(sm), b.track_targets_per_launch(sm))
    finally:
        b.close()


def _both_arms_equal(monkeypatch, *args):
    res = {}
    for arm in ("0", "1"):
        monkeypatch.setenv("MTFHIP_TRACK_DEFER_MAT", arm)
        res[arm], plan = _run(*args)
    print("n_iters every-pass", res["0"][0].tolist(), "deferred", res["1"][0].tolist(), "queues, targets per launch", plan)
    for name, a, c in zip(NAMES, res["0"], res["1"]):
        assert a.shape == c.shape and np.array_equal(_bits(a), _bits(c)), name
    return res["0"], plan


def _params(max_iters, epsilon=-1.0, **extra):
    return dict(leven_marq=0, max_iters=max_iters, epsilon=epsilon, **extra)


# pixels per target: 255 (no full row), 256 (one), 257 does not factor -> 23 x 11 = 253 beside it, 511 (one full + partial), 512 (two full),
# 513 (two + partial); 70 x 70 = five workgroups of four rows, the last one with three full rows and a partial one; 200 x 200 = the
# headline's target, four rows per workgroup
SHAPES = [(15, 17), (16, 16), (23, 11), (7, 73), (16, 32), (19, 27), (70, 70), (200, 200)]


def _rows_per_workgroup(monkeypatch, gpu_ctx, frame, frame2, resx, resy):
    corners = synth.square_corners(250, 240, 90.0)[None]
    out, _ = _both_arms_equal(monkeypatch, gpu_ctx, frame, frame2, L.SSM_HOMOGRAPHY, L.SM_ESM, _params(5), resx, resy, corners, corners + 0.6)
    assert (out[0] == 5).all()


# a 60-pixel region over each edge of the 512 x 512 frame: its rows inside take the interior path, those across the edge the general sampler
EDGES = {"left": (10, 250), "right": (500, 250), "top": (250, 10), "bottom": (250, 500), "corner": (495, 498), "outside": (700, -200)}


def _region_over_the_frame_edge(monkeypatch, gpu_ctx, frame, frame2, where, resx, resy):
    cx, cy = EDGES[where]
    corners = synth.square_corners(cx, cy, 60.0)[None]
    _both_arms_equal(monkeypatch, gpu_ctx, frame, frame2, L.SSM_HOMOGRAPHY, L.SM_ESM, _params(4), resx, resy, corners, corners + 0.3)


def _identity_warp_on_an_integer_lattice(monkeypatch, gpu_ctx, frame, sm_kind, resx, resy):
    """every sample on integer coordinates of the frame the template was taken from: the residual is zero, the warp stays the identity,
    and no wave of any pass takes the interior path"""
    x0, y0 = 100.0, 140.0
    corners = np.array([[x0, x0 + (resx - 1), x0 + (resx - 1), x0], [y0, y0, y0 + (resy - 1), y0 + (resy - 1)]])[None]
    out, _ = _both_arms_equal(monkeypatch, gpu_ctx, frame, frame, L.SSM_HOMOGRAPHY, sm_kind, _params(4), resx, resy, corners, None)
    assert np.array_equal(out[1].reshape(corners.shape), corners)


def _middle_target_stops_early(monkeypatch, gpu_ctx, frame):
    """three targets tracked on the template's own frame: the middle one starts on its template region and stops behind its first pass
    (its workgroups then return behind the first row's loads, and its arrays come from the trailing launch), the others start displaced"""
    corners = np.stack([synth.square_corners(150 + 90 * t, 200 + 40 * t, 60.0) for t in range(3)])
    start = corners + np.array([1.5, 0.0, 2.5])[:, None, None]
    out, _ = _both_arms_equal(monkeypatch, gpu_ctx, frame, frame, L.SSM_HOMOGRAPHY, L.SM_ESM, _params(9, epsilon=1e-5), 19, 27, corners, start)
    n = out[0].tolist()
    assert n[1] < n[0] and n[1] < n[2], n


def _two_chunks_on_two_queues(monkeypatch, gpu_ctx, frame, frame2):
    """65 targets as chunks of 33 and 32 on two queues (a batch this small keeps one launch on one queue unless told otherwise)"""
    B = 65
    monkeypatch.setenv("MTFHIP_TRACK_CHUNK_PX", str(33 * 19 * 27 + 10))
    monkeypatch.setenv("MTFHIP_TRACK_STREAMS", "12")
    corners = np.stack([synth.square_corners(60 + 45 * (t % 9), 60 + 50 * (t // 9), 40.0) for t in range(B)])
    start = corners + (0.1 + 0.02 * np.arange(B))[:, None, None]
    _, plan = _both_arms_equal(monkeypatch, gpu_ctx, frame, frame2, L.SSM_HOMOGRAPHY, L.SM_ESM, _params(4), 19, 27, corners, start)
    assert plan == (2, 33), plan


def _models(monkeypatch, gpu_ctx, frame, frame2, sm_kind, ssm, chained, max_iters):
    """every instantiation the lean replay SSD pass has (the homography kernels with the non-chained gradient and the affine chained
    FCLK kernel keep the one loop: no room for a row ahead in their registers), two targets of two full rows and a partial one"""
    corners = np.stack([synth.square_corners(200 + 60 * t, 230 + 30 * t, 70.0) for t in range(2)])
    out, _ = _both_arms_equal(monkeypatch, gpu_ctx, frame, frame2, ssm, sm_kind, _params(max_iters, chained_warp=chained), 19, 27, corners, corners + 0.5)
    assert (out[0] == max_iters).all()


def _cases(frame, frame2):
    """-> (id, function of monkeypatch and the context) for every case; each function asserts for itself"""
    out = []
    for resx, resy in SHAPES:
        out.append(("rows_per_workgroup[%dx%d]" % (resx, resy), lambda mp, ctx, resx=resx, resy=resy: _rows_per_workgroup(mp, ctx, frame, frame2, resx, resy)))
    for resx, resy in ((19, 27), (40, 40)):
        for where in EDGES:
            out.append(("region_over_the_frame_edge[%dx%d-%s]" % (resx, resy, where),
                        lambda mp, ctx, resx=resx, resy=resy, where=where: _region_over_the_frame_edge(mp, ctx, frame, frame2, where, resx, resy)))
    for resx, resy in ((16, 16), (16, 32)):
        for name, sm_kind in (("esm", L.SM_ESM), ("fclk", L.SM_FCLK)):
            out.append(("identity_warp_on_an_integer_lattice[%dx%d-%s]" % (resx, resy, name),
                        lambda mp, ctx, resx=resx, resy=resy, sm_kind=sm_kind: _identity_warp_on_an_integer_lattice(mp, ctx, frame, sm_kind, resx, resy)))
    out.append(("middle_target_stops_early", lambda mp, ctx: _middle_target_stops_early(mp, ctx, frame)))
    out.append(("two_chunks_on_two_queues", lambda mp, ctx: _two_chunks_on_two_queues(mp, ctx, frame, frame2)))
    for sname, sm_kind in (("esm", L.SM_ESM), ("fclk", L.SM_FCLK)):
        for mname, ssm in (("hom", L.SSM_HOMOGRAPHY), ("aff", L.SSM_AFFINE)):
            for chained in (0, 1):
                for max_iters in (3, 7):
                    out.append(("models[%s-%s-%s-%d]" % (sname, mname, "chained" if chained else "unchained", max_iters),
                                lambda mp, ctx, sm_kind=sm_kind, ssm=ssm, chained=chained, max_iters=max_iters:
                                _models(mp, ctx, frame, frame2, sm_kind, ssm, chained, max_iters)))
    return out


def test_lean_pass_equals_materialising_pass_at_every_seam(gpu_ctx, frame, frame2, monkeypatch):
    """Every case below in one test item (42 cases, about a second together): a case that fails its comparison is recorded and the others
    still run, and the assertion at the end names every one that failed; any other error ends the test where it happens."""
    failed = []
    for cid, run in _cases(frame, frame2):
        with monkeypatch.context() as mp:
            try:
                run(mp, gpu_ctx)
                print("ok  ", cid)
            except AssertionError as e:
                print("FAIL", cid, e)
                failed.append("%s: %s" % (cid, str(e).splitlines()[0] if str(e) else "assertion"))
    assert not failed, "%d case(s) differ:\n%s" % (len(failed), "\n".join(failed))


