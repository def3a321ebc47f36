"""CPU: the NumPy restatement of the reference's RANSAC / LMedS estimator (tests/helpers/est_ref.py) held to facts that do not come from
it, and the C ABI of the device estimator (declared, exported, loud without a device)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import est_cases as EC   # noqa: E402
import est_ref as R      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_iteration_counts_by_hand():
    # log(0.005) / log(1 - 0.7^4) = -5.2983 / -0.27457 = 19.30
    assert R.ransac_update_num_iters(0.995, 0.3, 4, 2000) == 19
    # log(0.005) / log(1 - 0.55^4) = -5.2983 / -0.095967 = 55.21 (the shipped est_confidence 0.995, est_n_model_pts 4)
    assert R.lmeds_num_iters(0.995, 4, 10000) == 55
    assert R.lmeds_num_iters(0.995, 4, 20) == 20 and R.lmeds_num_iters(0.5, 8, 100) >= 3
    assert R.ransac_update_num_iters(0.995, 0.0, 4, 2000) == 0          # no outliers: denom = 0
    assert R.ransac_update_num_iters(0.995, 1.0, 4, 2000) == 2000       # no inliers
    assert R.cv_round(2.5) == 2 and R.cv_round(3.5) == 4                # half to even


@pytest.mark.parametrize("ssm", [R.HOMOGRAPHY, R.AFFINE], ids=["homography", "affine"])
@pytest.mark.parametrize("method", [R.RANSAC, R.LMEDS], ids=["ransac", "lmeds"])
def test_exact_map_with_gross_outliers_is_recovered(ssm, method):
    a, b, clean = EC.make_points(ssm, 10, 5, 0.30, noise=0.0)
    p = R.Params(method=method, ransac_reproj_thresh=1.0, n_model_pts=4 if ssm == R.HOMOGRAPHY else 3, max_iters=500)
    sub = EC.draw_subsets(17, a, b, 60, p.n_model_pts)
    r = R.estimate(ssm, a, b, p, sub)
    assert r["ok"] and np.array_equal(r["mask"].astype(bool), clean)
    # the recovered map sends every clean point onto its partner (the points are float32: 400 px * 2^-24 = 2.4e-5 px of rounding)
    np.testing.assert_allclose(EC.apply(r["H"], a[clean].astype(np.float64)), b[clean].astype(np.float64), rtol=0, atol=1e-3)


def test_collinear_subset_is_rejected():
    line = np.array([[0.0, 0.0], [1.0, 1.0], [5.0, 5.0], [3.0, -2.0]])
    assert not R.check_subset(line)
    assert R.check_subset(line[[0, 1, 3]]) and R.check_subset(np.array([[0.0, 0], [4, 0], [4, 3], [0, 3]]))
    assert not R.check_subset(np.array([[0.0, 0], [4, 0], [4, 3], [2, 0]]))
    # a hypothesis whose subset search failed ends the walk; at index 0 the fit fails with the zero matrix and an all-ones mask
    a, b, _ = EC.make_points(R.HOMOGRAPHY, 5, 1, 0.2)
    r = R.estimate(R.HOMOGRAPHY, a, b, R.Params(), np.full((3, 4), -1))
    assert not r["ok"] and r["mask"].all() and np.array_equal(r["state_update"], [-1, 0, 0, 0, -1, 0, 0, 0]) and r["n_walked"] == 0


@pytest.mark.parametrize("ssm", [R.HOMOGRAPHY, R.AFFINE], ids=["homography", "affine"])
def test_refinement_does_not_increase_the_error(ssm):
    a, b, _ = EC.make_points(ssm, 8, 3, 0.0)
    M, m = a.astype(np.float64), b.astype(np.float64)
    H = R.run_kernel(ssm, M, m)
    H0 = H.copy()
    H0[0, 2] += 0.4
    H0[1, 0] += 1e-3                                     # a start away from the optimum
    for start in (H, H0):
        assert R.sq_error(ssm, R.refine(ssm, start, M, m, 10), M, m) <= R.sq_error(ssm, start, M, m)
    assert R.sq_error(ssm, R.refine(ssm, H0, M, m, 10), M, m) < 0.5 * R.sq_error(ssm, H0, M, m)


def test_the_two_solvers_agree():
    a, b, _ = EC.make_points(R.HOMOGRAPHY, 6, 2, 0.0)
    M, m = a.astype(np.float64), b.astype(np.float64)
    for ssm in (R.HOMOGRAPHY, R.AFFINE):
        np.testing.assert_allclose(R.run_kernel(ssm, M, m, "eigh"), R.run_kernel(ssm, M, m, "alt"), rtol=1e-7, atol=1e-9)
        q = [0, 5, 30, 34]                               # a minimal subset: LtL has rank 8
        np.testing.assert_allclose(R.run_kernel(ssm, M[q], m[q], "eigh"), R.run_kernel(ssm, M[q], m[q], "alt"), rtol=1e-7, atol=1e-9)
    assert R.run_kernel(R.HOMOGRAPHY, M[:4], m[:4]) is None   # four points of one lattice row: no spread in y (HomographyEstimator.cc:48-50)


def test_abi_declares_exports_and_fails_loudly():
    import mtf_amd
    from mtf_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "mtfhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    lib.mtfhip_last_error.restype = ctypes.c_char_p
    for fn in ("mtfhip_ssm_estimate_from_pts", "mtfhip_ssm_estimate_from_pts_dev"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, text), fn
        assert hasattr(lib, fn) and fn in L.SYMBOLS
    assert "mtfhip_est_params" in text
    # no context (what a machine without a device is left with: mtfhip_ctx_create fails there): an error with a message, no CPU path
    p = L.est_params()
    n = np.array([4], dtype=np.int32)
    pts = np.zeros((4, 2), dtype=np.float32)
    upd, mask, info, stats = np.zeros(8), np.zeros(4, dtype=np.uint8), np.zeros(4, dtype=np.int32), np.zeros(2)
    lib.mtfhip_ssm_estimate_from_pts.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + \
        [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_ulonglong] + [ctypes.c_void_p] * 5
    rc = lib.mtfhip_ssm_estimate_from_pts(None, 0, ctypes.byref(p), 1, n.ctypes.data, 4, pts.ctypes.data, pts.ctypes.data, None, 1, 0,
                                          upd.ctypes.data, mask.ctypes.data, info.ctypes.data, stats.ctypes.data, None)
    assert rc == -1 and b"ssm_estimate_from_pts" in lib.mtfhip_last_error()
    lib.mtfhip_ssm_estimate_from_pts_dev.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + \
        [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong] + [ctypes.c_void_p] * 4
    rc = lib.mtfhip_ssm_estimate_from_pts_dev(None, 0, ctypes.byref(p), 1, None, None, 4, None, None, None, 0, 1, 0, None, None, None, None)
    assert rc == -1 and b"ssm_estimate_from_pts_dev" in lib.mtfhip_last_error()
    if lib.mtfhip_device_count() == 0:
        with pytest.raises(mtf_amd.MtfHipError):
            mtf_amd.Context(0)
