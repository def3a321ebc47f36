"""nt::NN's update loop on the device (mtfhip_nn_update, mtf_amd.sm.NNTracker, mtf::hip::NN) against tests/helpers/nn_ref.nn_update, which
drives the oracle's appearance and state space models: the dataset is the oracle's own (handed over through set_dataset), so the only
difference between the two sides' distances is the query feature, which tests/test_gpu_nn.py holds to 1e-9 (SSD) / 1e-12 (NCC) of the
oracle.  best_idx of every iteration must be equal (the reference's gap asserted first), best_dist within 1e-8 relative (SSD) / 1e-9
absolute (NCC), the corners within 1e-9 px, n_iters equal.  The device loop and the host-stepped loop, and a built and a handed-over
dataset, must agree bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd.sm import NNTracker

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import nn_cases as NC   # noqa: E402
import nn_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
_REF = {}


def _reference(oracle, frame, frame2, case):
    """the oracle's dataset and NN::update for a case: computed once, shared, never changed"""
    if case[0] not in _REF:
        _, am, ssm, res, ch, kind, max_iters, eps, seed = case
        img0, img1 = NC.track_frames(kind, frame, frame2)
        o_ssm = oracle.SSM(ssm, res, res); o_am = oracle.AM(am, res, res)
        if ch > 1:
            o_am.set_channels(ch); o_ssm.set_channels(ch)
        o_am.set_curr_img(img0)
        corners = NC.track_corners_for(kind, res)
        o_ssm.set_corners(corners)
        o_am.initialize_pix_vals(o_ssm.get("curr_pts"))
        perts = NC.track_perturbations(ssm, seed)
        feats = oracle.nn_generate_dataset(o_am, o_ssm, perts)
        o_am.set_curr_img(img1)
        r = R.nn_update(o_am, o_ssm, feats, perts, max_iters, eps)
        for a in (feats, perts, r["log"], r["corners"]):
            a.setflags(write=False)
        _REF[case[0]] = dict(img0=img0, img1=img1, corners=corners, perts=perts, feats=feats, ref=r)
    return _REF[case[0]]


def _tracker(ctx, case, host_stepped=False, **kw):
    _, am, ssm, res, ch, kind, max_iters, eps, seed = case
    old = os.environ.get("MTFHIP_NN_HOST_STEPPED")
    os.environ["MTFHIP_NN_HOST_STEPPED"] = "1" if host_stepped else "0"
    try:
        return NNTracker(ctx, am=am, ssm=ssm, resx=res, resy=res, n_samples=NC.N_SAMPLES, max_iters=max_iters, epsilon=eps,
                         am_params=dict(n_channels=ch) if ch > 1 else None, **kw)
    finally:
        if old is None:
            del os.environ["MTFHIP_NN_HOST_STEPPED"]
        else:
            os.environ["MTFHIP_NN_HOST_STEPPED"] = old


def _corners8(c24):
    """(2, 4) -> x0 y0 x1 y1 ... as the oracle lays corners out"""
    return np.asarray(c24).T.reshape(-1)


@pytest.mark.parametrize("case", NC.TRACK_CASES, ids=lambda c: c[0])
def test_update_follows_reference_and_forms_agree(oracle, gpu_ctx, frame, frame2, case):
    d = _reference(oracle, frame, frame2, case)
    am, ref = case[1], d["ref"]
    for row in ref["log"]:
        assert R.gap_ok(row[1], row[2])
    out = {}
    for stepped in (False, True):
        gpu_ctx.set_image(d["img0"])
        t = _tracker(gpu_ctx, case, host_stepped=stepped)
        t.initialize(d["corners"], features=d["feats"], perturbations=d["perts"])
        gpu_ctx.set_image(d["img1"])
        c = t.update()
        out[stepped] = (c.copy(), t.n_iters, t.log.copy(), t.get_region().copy(), t.batch.get_state().copy())
        t.close()
    c, n_iters, log, region, state = out[False]
    assert n_iters == ref["n_iters"] and log.shape == (n_iters, 3)
    assert np.array_equal(log[:, 0], ref["log"][:, 0])
    for i in range(n_iters):
        want = ref["log"][i, 1]
        err = abs(log[i, 1] - want)
        print("%s it=%d idx=%d dist err=%.3e" % (case[0], i, int(log[i, 0]), err))
        assert err <= (1e-8 * abs(want) if am == R.SSD else 1e-9)
    print("%s corners err=%.3e" % (case[0], np.abs(_corners8(c) - ref["corners"]).max()))
    np.testing.assert_allclose(_corners8(c), ref["corners"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(log[:, 2], ref["log"][:, 3], rtol=1e-6, atol=1e-9)
    assert np.array_equal(region, c)                  # the batch's SSM followed
    # the host-stepped loop: the same kernels one iteration per call -- the same bits
    for a, b in zip(out[False], out[True]):
        assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("case", [NC.TRACK_CASES[1], NC.TRACK_CASES[3], NC.TRACK_CASES[4]], ids=lambda c: c[0])
def test_built_dataset_equals_handed_over_dataset(gpu_ctx, frame, frame2, case):
    """a tracker that builds its dataset on the device (two sampler distributions: consecutive row blocks) and one handed the same rows
    through set_dataset return identical results; the built rows are NNDataset.initialize's"""
    _, am, ssm, res, ch, kind, max_iters, eps, seed = case
    sg = NC.SIGMA_H if ssm == 0 else NC.SIGMA_A
    kw = dict(ssm_sigma=(sg * 0.3, sg), distr_n_samples=[63, NC.N_SAMPLES - 63], seed=seed)
    corners = NC.track_corners(res)
    gpu_ctx.set_image(frame)
    t1 = _tracker(gpu_ctx, case, **kw)
    t1.initialize(corners)
    feats, perts = t1.get_dataset()
    ds = mtf_amd.sm.NNDataset(gpu_ctx, am=am, ssm=ssm, resx=res, resy=res, n_samples=NC.N_SAMPLES, **kw)
    assert np.array_equal(ds.initialize(corners), feats) and np.array_equal(ds.perturbations, perts)
    ds.batch.close()
    t2 = _tracker(gpu_ctx, case)
    t2.initialize(corners, features=feats, perturbations=perts)
    gpu_ctx.set_image(frame2)
    c1, c2 = t1.update(), t2.update()
    assert np.array_equal(c1, c2) and t1.n_iters == t2.n_iters and np.array_equal(t1.log, t2.log)
    assert t1.n_iters == max_iters and np.abs(c1 - corners).max() > 1e-3       # it did move
    # search() on the resident rows: a stored row finds itself
    idx, dist = t1.search(feats[[5, 150]])
    assert list(idx) == [5, 150] and (dist[0] == 0.0 if am == L.AM_SSD else abs(dist[0] + 1) < 1e-12)
    t1.close(); t2.close()


@pytest.mark.parametrize("am", [L.AM_SSD, L.AM_NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("ssm", [L.SSM_HOMOGRAPHY, L.SSM_AFFINE], ids=["hom", "aff"])
def test_zero_motion(gpu_ctx, frame, am, ssm):
    """the image unchanged and the zero perturbation as row 0: row 0 at distance 0 (SSD) / -1 (NCC), the corners unchanged, and the loop
    stops after its first iteration for any positive epsilon"""
    case = ("zero", am, ssm, 24, 1, "frame2", 5, 1e-12, 11)
    corners = NC.track_corners(24)
    perts = NC.track_perturbations(ssm, 11)
    gpu_ctx.set_image(frame)
    t = _tracker(gpu_ctx, case)
    t.initialize(corners)            # (its own draws ...)
    feats, _ = t.get_dataset()
    b = mtf_amd.Batch(gpu_ctx, am, ssm, 24, 24, 1)
    b.set_corners(corners[None]); b.initialize_pix_vals()
    _, feats = b.nn_dataset(NC.N_SAMPLES, np.zeros(8), perturbations=perts)      # (... replaced by rows of known perturbations, row 0 zero)
    b.close()
    t.set_dataset(feats, perts)
    c = t.update()
    assert t.n_iters == 1 and t.log[0, 0] == 0 and t.log[0, 2] == 0.0
    assert t.log[0, 1] == 0.0 if am == L.AM_SSD else abs(t.log[0, 1] + 1.0) < 1e-12
    assert np.array_equal(c, corners) and np.array_equal(t.get_region(), corners)
    t.close()


def test_cpp_driver_equals_python_driver(gpu_ctx, frame, frame2):
    """mtf::hip::NN (one mtfhip_nn_update per update()) against sm.NNTracker: the same draws, the same corners"""
    from mtf_amd import host
    lib = host.lib()
    res, n, iters, seed = 24, NC.N_SAMPLES, 5, 21
    sg = np.zeros((2, 8)); sg[0] = NC.SIGMA_H * 0.3; sg[1] = NC.SIGMA_H
    cnt = np.array([63, n - 63], dtype=np.int32)
    corners = NC.track_corners(res)
    t = lib.mtfhost_nn_create(L.AM_SSD, L.SSM_HOMOGRAPHY, res, res, n, iters, 0.0, 2, sg.ctypes.data, None, cnt.ctypes.data, seed, 0, 1)
    assert t, lib.mtfhost_last_error()
    c8 = np.ascontiguousarray(corners.T).reshape(-1)
    for img, first in ((frame, True), (frame2, False)):
        assert lib.mtfhost_set_image(t, img.ctypes.data, img.shape[0], img.shape[1], img.shape[1]) == 0, lib.mtfhost_last_error()
        if first:
            assert lib.mtfhost_initialize(t, c8.ctypes.data) == 0, lib.mtfhost_last_error()
    it = ctypes.c_int()
    assert lib.mtfhost_update(t, ctypes.byref(it)) == 0, lib.mtfhost_last_error()
    out, log = np.empty(8), np.zeros((iters, 3))
    assert lib.mtfhost_get_region(t, out.ctypes.data) == 0 and lib.mtfhost_nn_log(t, log.ctypes.data, iters) == it.value == iters
    lib.mtfhost_destroy(t)
    gpu_ctx.set_image(frame)
    p = NNTracker(gpu_ctx, n_samples=n, resx=res, resy=res, ssm_sigma=(sg[0], sg[1]), distr_n_samples=[63, n - 63], max_iters=iters, epsilon=0.0, seed=seed)
    p.initialize(corners)
    gpu_ctx.set_image(frame2)
    c = p.update()
    assert np.array_equal(out.reshape(4, 2).T, c) and np.array_equal(log, p.log)
    p.close()
