"""The call path of the chunked device-side LK loop (track_core / track_loop_chunked, api_track.hip): one prologue launch in front of the loop
(slab ingest + the loop's words + the Levenberg-Marquardt start state, k_track_prologue), the results delivered by the finish that stops a
target or by the last one enqueued (k_finish_track's HostPublish), and the finish waves' raised issue priority.
MTFHIP_TRACK_FUSED_IO=0 keeps the separate ingest, memsets, copy and k_publish_host launch; MTFHIP_FINISH_PRIO=0 leaves the priority alone.
None of this re-orders arithmetic, so everything a caller can see after a call is the same BITS in all three arms."""
import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth

pytestmark = pytest.mark.gpu

MODELS = [
    (L.SM_ESM, L.AM_SSD, L.SSM_HOMOGRAPHY, dict()),
    (L.SM_FCLK, L.AM_SSD, L.SSM_AFFINE, dict()),
    (L.SM_ESM, L.AM_NCC, L.SSM_AFFINE, dict()),
    (L.SM_FCLK, L.AM_NCC, L.SSM_HOMOGRAPHY, dict()),
]
MODEL_IDS = ["esm_ssd_hom", "fclk_ssd_aff", "esm_ncc_aff", "fclk_ncc_hom"]
# (fused head and tail, finish priority): the new path, the old head and tail, the new path without the priority
ARMS = {"new": ("1", "1"), "old_io": ("0", "1"), "no_prio": ("1", "0")}
NAMES = ("It", "n_iters", "corners", "state", "warp", "dIt_dx", "Jt")


def _corners(B, size):
    return np.stack([synth.square_corners(200 + 31 * t, 230 + 17 * t, float(size)) for t in range(B)])


def _seen(b, n, c):
    """what a caller sees behind a call; It is read first: a stream-ordered read right behind the call, which the join has to order behind both queues"""
    it = b.read(L.BUF_IT).copy()
    return [it, n.copy(), c.copy(), b.get_state().copy(), b.get_warp().copy(), b.read(L.BUF_DIT_DX).copy(), b.read(L.BUF_JT).copy()]


def _two_queues(monkeypatch, resx, resy, per_chunk=2):
    monkeypatch.setenv("MTFHIP_TRACK_STREAMS", "12")
    monkeypatch.setenv("MTFHIP_TRACK_CHUNK_PX", str(per_chunk * resx * resy + 10))


def _set_image(gpu_ctx, img, borrow):
    """upload (the context owns its copy), or adopt a device tensor (borrowed: the caller's to rewrite behind a call that returns results)"""
    if not borrow:
        gpu_ctx.set_image(img)
        return
    import torch
    gpu_ctx.synchronize()   # (mtfhip.h: the image borrowed so far stays unchanged and alive until a call that synchronises with the context's stream)
    t = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to("cuda:0")
    torch.cuda.synchronize()
    gpu_ctx.set_image_device(t.data_ptr(), t.shape[0], t.shape[1], keep=t)


def _launches(gpu_ctx):
    """launches per kernel family since timing_reset(): the prologue, k_publish_host, the chunked driver's finish"""
    return {k: gpu_ctx.timing_get(k)[1] for k in ("track_prologue", "publish_host", "finish_track")}


def _run(gpu_ctx, frame, frame2, am, ssm, sm_kind, params, resx, resy, corners, start=None, trace=0, region=False, borrow=False, counts=None):
    """template on `frame`, two calls of the device-side loop on `frame2`, the second right behind the first at a shifted region;
    counts (a dict): filled with the launches of the two calls per kernel family"""
    B = len(corners)
    _set_image(gpu_ctx, frame, borrow)
    b = mtf_amd.Batch(gpu_ctx, am, ssm, resx, resy, B)
    try:
        b.set_corners(corners)
        sm = mtf_amd.sm_desc(sm_kind, materialize=1, **params)
        b.init_template(sm)
        _set_image(gpu_ctx, frame2, borrow)
        if trace:
            b.track_trace(trace)
        s0 = corners if start is None else start
        if counts is not None:
            gpu_ctx.timing(True)
            gpu_ctx.timing_reset()
        if region:
            n1, c1 = b.track_region(s0, sm)
        else:
            b.set_region(s0, sm)
            n1, c1 = b.track(sm)
        out = _seen(b, n1, c1)
        if region:
            n2, c2 = b.track_region(c1 + 0.4, sm)
        else:
            b.set_region(c1 + 0.4, sm)
            n2, c2 = b.track(sm)
        out += _seen(b, n2, c2)
        if counts is not None:
            counts.update(_launches(gpu_ctx))
        return out, (b.track_queues(sm), b.track_targets_per_launch(sm))
    finally:
        if counts is not None:
            gpu_ctx.timing(False)
        b.close()
        if borrow:
            gpu_ctx.set_image(frame2)   # (the session's context goes on with an image of its own)


def _assert_same(res, ref="old_io"):
    for arm, out in res.items():
        for k, (a, c) in enumerate(zip(res[ref], out)):
            name = "%s of call %d, arm %s against %s" % (NAMES[k % len(NAMES)], k // len(NAMES) + 1, arm, ref)
            assert a.shape == c.shape and np.array_equal(a, c), name


def _arms_equal(monkeypatch, *args, counts=None, **kw):
    """counts (a dict): per arm the launches of the two calls per kernel family"""
    res, plan = {}, None
    for arm, (io, prio) in ARMS.items():
        monkeypatch.setenv("MTFHIP_TRACK_FUSED_IO", io)
        monkeypatch.setenv("MTFHIP_FINISH_PRIO", prio)
        if counts is not None:
            counts[arm] = {}
        res[arm], plan = _run(*args, counts=None if counts is None else counts[arm], **kw)
    print("n_iters", res["new"][1].tolist(), "second call", res["new"][1 + len(NAMES)].tolist(), "queues, targets per launch", plan)
    _assert_same(res)
    return res["old_io"], plan


@pytest.mark.parametrize("sm_kind,am,ssm,extra", MODELS, ids=MODEL_IDS)
@pytest.mark.parametrize("max_iters", [1, 2, 3, 7])
def test_runs_out_of_passes(gpu_ctx, frame, frame2, monkeypatch, sm_kind, am, ssm, extra, max_iters):
    """an unreachable epsilon on two queues, chunks of 2 + 2 + 1 targets (two groups of chunks): every target is delivered by the last pass -- one
    and two passes materialise every pass, three is the boundary of the deferred loop, seven runs it"""
    _two_queues(monkeypatch, 40, 30)
    params = dict(leven_marq=0, max_iters=max_iters, epsilon=-1.0)
    params.update(extra)
    corners = _corners(5, 50)
    out, plan = _arms_equal(monkeypatch, gpu_ctx, frame, frame2, am, ssm, sm_kind, params, 40, 30, corners, start=corners + 0.7)
    assert plan == (2, 3 if max_iters == 1 else 2), plan   # (a single pass is not chunked: one launch per queue)
    assert (out[1] == max_iters).all() and (out[1 + len(NAMES)] == max_iters).all()


@pytest.mark.parametrize("B", [1, 2])
def test_small_batches(gpu_ctx, frame, frame2, monkeypatch, B):
    """one target (one queue, one chunk) and two (a target per queue)"""
    _two_queues(monkeypatch, 32, 32, per_chunk=1)
    params = dict(leven_marq=0, max_iters=7, epsilon=-1.0)
    corners = _corners(B, 44)
    _, plan = _arms_equal(monkeypatch, gpu_ctx, frame, frame2, L.AM_SSD, L.SSM_HOMOGRAPHY, L.SM_ESM, params, 32, 32, corners, start=corners + 0.5)
    assert plan == (B, 1), plan


def _mixed_start(gpu_ctx, frame, frame2, am, ssm, sm_kind, params, res, corners):
    """start regions whose targets stop behind different passes: target 0 on its converged region, the last displaced until it uses every
    pass, the ones in between by growing small amounts"""
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
        for t in range(1, B - 1):
            start[t] = c0[t] + 0.35 * t
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


@pytest.mark.parametrize("sm_kind,am,ssm,extra", [MODELS[0], MODELS[3]], ids=[MODEL_IDS[0], MODEL_IDS[3]])
def test_targets_stop_at_different_passes(gpu_ctx, frame, frame2, monkeypatch, sm_kind, am, ssm, extra):
    """a reachable epsilon: a target converged at pass 1, one that never converges, others in between -- each is delivered once, by the pass
    that stops it, and the trailing materialising launches run behind the delivery"""
    _two_queues(monkeypatch, 32, 32)
    monkeypatch.setenv("MTFHIP_TRACK_FUSED_IO", "0")
    params = dict(leven_marq=0, max_iters=7, epsilon=1e-5)
    params.update(extra)
    corners = _corners(5, 44)
    start = _mixed_start(gpu_ctx, frame, frame2, am, ssm, sm_kind, params, 32, corners)
    out, plan = _arms_equal(monkeypatch, gpu_ctx, frame, frame2, am, ssm, sm_kind, params, 32, 32, corners, start=start)
    n = out[1].tolist()
    assert plan == (2, 2), plan
    assert 1 in n and 7 in n and len(set(n)) >= 3, n


@pytest.mark.parametrize("sm_kind", [L.SM_ESM, L.SM_FCLK], ids=["esm", "fclk"])
def test_levenberg_marquardt_state_comes_from_the_prologue(gpu_ctx, frame, frame2, monkeypatch, sm_kind):
    """Levenberg-Marquardt (FCLK: 2 x max_iters passes): the start state of every target is written by the prologue launch instead of a copy"""
    _two_queues(monkeypatch, 40, 30)
    params = dict(leven_marq=1, max_iters=5, epsilon=1e-5)
    corners = _corners(5, 50)
    start = corners + np.array([0.0, 0.3, 0.8, 1.5, 4.0])[:, None, None]
    _, plan = _arms_equal(monkeypatch, gpu_ctx, frame, frame2, L.AM_SSD, L.SSM_HOMOGRAPHY, sm_kind, params, 40, 30, corners, start=start)
    assert plan == (2, 2), plan


@pytest.mark.parametrize("leven_marq", [0, 1])
def test_folded_track_region(gpu_ctx, frame, frame2, monkeypatch, leven_marq):
    """FCLK 40 x 40 through track_region: the reset travels with the slab (no upload in track_core), so the prologue runs without the ingest"""
    _two_queues(monkeypatch, 40, 40, per_chunk=1)
    params = dict(leven_marq=leven_marq, max_iters=6, epsilon=1e-5)
    corners = _corners(2, 56)
    counts = {}
    _, plan = _arms_equal(monkeypatch, gpu_ctx, frame, frame2, L.AM_SSD, L.SSM_HOMOGRAPHY, L.SM_FCLK, params, 40, 40, corners, start=corners + 0.6, region=True,
                          counts=counts)
    assert plan == (2, 1), plan
    # the chunked driver ran (its finish launches), behind one prologue per call, and delivered from the loop; the old arm published by launch
    print(counts)
    assert counts["new"]["finish_track"] > 0 and counts["new"]["track_prologue"] == 2 and counts["new"]["publish_host"] == 0, counts
    assert counts["old_io"]["track_prologue"] == 0 and counts["old_io"]["publish_host"] == 2, counts


@pytest.mark.parametrize("epsilon", [-1.0, 1e-5])
def test_the_fused_head_and_delivery_run(gpu_ctx, frame, frame2, monkeypatch, epsilon):
    """what the arms launch, by the context's per-family launch counts: one prologue per call and no k_publish_host on the new path (also with a
    reachable epsilon: the context owns its image), the reverse with MTFHIP_TRACK_FUSED_IO=0"""
    _two_queues(monkeypatch, 40, 30)
    params = dict(leven_marq=0, max_iters=7, epsilon=epsilon)
    corners = _corners(5, 50)
    counts = {}
    _arms_equal(monkeypatch, gpu_ctx, frame, frame2, L.AM_SSD, L.SSM_HOMOGRAPHY, L.SM_ESM, params, 40, 30, corners, start=corners + 0.7, counts=counts)
    print(counts)
    for arm in ("new", "no_prio"):
        assert counts[arm]["track_prologue"] == 2 and counts[arm]["publish_host"] == 0 and counts[arm]["finish_track"] > 0, counts
    assert counts["old_io"]["track_prologue"] == 0 and counts["old_io"]["publish_host"] == 2, counts


@pytest.mark.parametrize("epsilon", [-1.0, 1e-5])
def test_borrowed_image(gpu_ctx, frame, frame2, monkeypatch, epsilon):
    """an image the caller owns may be rewritten once the call has returned.  With a reachable epsilon, pixel passes follow the in-loop delivery
    (the trailing materialising launches sample the image), so such a call keeps the delivery behind the queues' join: k_publish_host runs;
    with an unreachable one nothing samples the image behind the last finish and the loop delivers.  Same bits either way."""
    _two_queues(monkeypatch, 40, 30)
    params = dict(leven_marq=0, max_iters=7, epsilon=epsilon)
    corners = _corners(5, 50)
    start = corners + np.array([0.0, 0.3, 0.8, 1.5, 4.0])[:, None, None]
    counts = {}
    _arms_equal(monkeypatch, gpu_ctx, frame, frame2, L.AM_SSD, L.SSM_HOMOGRAPHY, L.SM_ESM, params, 40, 30, corners, start=start, borrow=True, counts=counts)
    print(counts)
    assert counts["new"]["track_prologue"] == 2, counts
    assert counts["new"]["publish_host"] == (2 if epsilon > 0 else 0), counts


@pytest.mark.parametrize("epsilon", [-1.0, 1e-5])
def test_one_large_target(gpu_ctx, frame, frame2, monkeypatch, epsilon):
    """100 x 96 points of one target are ten block rows: the finish runs with 256 threads (three groups of lanes sum the rows), of which the first
    wave alone delivers"""
    params = dict(leven_marq=0, max_iters=5, epsilon=epsilon)
    corners = synth.square_corners(256, 250, 130.0)[None]
    counts = {}
    _arms_equal(monkeypatch, gpu_ctx, frame, frame2, L.AM_SSD, L.SSM_HOMOGRAPHY, L.SM_ESM, params, 100, 96, corners, start=corners + 0.6, counts=counts)
    assert counts["new"]["track_prologue"] == 2 and counts["new"]["publish_host"] == 0, counts


def test_with_a_trace_set(gpu_ctx, frame, frame2, monkeypatch):
    """the debug trace keeps one queue and the delivery by k_publish_host; the head is the prologue launch"""
    _two_queues(monkeypatch, 32, 32)
    params = dict(leven_marq=0, max_iters=6, epsilon=1e-5)
    corners = _corners(3, 44)
    _, plan = _arms_equal(monkeypatch, gpu_ctx, frame, frame2, L.AM_SSD, L.SSM_HOMOGRAPHY, L.SM_ESM, params, 32, 32, corners, start=corners + 0.5, trace=8)
    assert plan[0] == 1, plan


def test_two_batches_alternate_on_one_context(gpu_ctx, frame, frame2, monkeypatch):
    """two batches of different size take turns on one context: their sequence numbers and arrival counters are their own, the phase stamps
    are the context's"""
    _two_queues(monkeypatch, 32, 32)
    params = dict(leven_marq=0, max_iters=7, epsilon=1e-5)
    res = {}
    for arm, (io, prio) in ARMS.items():
        monkeypatch.setenv("MTFHIP_TRACK_FUSED_IO", io)
        monkeypatch.setenv("MTFHIP_FINISH_PRIO", prio)
        gpu_ctx.set_image(frame)
        batches = [mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, 32, 32, B) for B in (5, 2)]
        try:
            sm = mtf_amd.sm_desc(L.SM_ESM, materialize=1, **params)
            cs = [_corners(5, 44), _corners(2, 40) + 60.0]
            for b, c in zip(batches, cs):
                b.set_corners(c)
                b.init_template(sm)
            gpu_ctx.set_image(frame2)
            out = []
            for shift in (0.5, 1.1, 0.2):
                for b, c in zip(batches, cs):
                    b.set_region(c + shift, sm)
                    n, cr = b.track(sm)
                    out += _seen(b, n, cr)
            res[arm] = out
        finally:
            for b in batches:
                b.close()
    _assert_same(res)


def test_without_host_coherent_mirrors(gpu_ctx, frame, frame2, monkeypatch):
    """a batch created under MTFHIP_ZERO_COPY=0 (read at batch creation) uploads with a copy and reads back with a copy + synchronisation: the
    prologue then only sets the words; same bits as the zero-copy batch"""
    _two_queues(monkeypatch, 40, 30)
    params = dict(leven_marq=1, max_iters=5, epsilon=1e-5)
    corners = _corners(5, 50)
    args = (gpu_ctx, frame, frame2, L.AM_SSD, L.SSM_HOMOGRAPHY, L.SM_ESM, params, 40, 30, corners)
    monkeypatch.setenv("MTFHIP_ZERO_COPY", "0")
    out_copy, _ = _arms_equal(monkeypatch, *args, start=corners + 0.7)
    monkeypatch.delenv("MTFHIP_ZERO_COPY")
    monkeypatch.setenv("MTFHIP_TRACK_FUSED_IO", "1")
    monkeypatch.setenv("MTFHIP_FINISH_PRIO", "1")
    out_zc, _ = _run(*args, start=corners + 0.7)
    _assert_same({"zero_copy": out_zc, "old_io": out_copy})
