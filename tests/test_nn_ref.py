"""CPU: the float64 restatement of nt::NN's search and update (tests/helpers/nn_ref.py) held to planted cases, the gap condition of every
shared case (tests/helpers/nn_cases.py) on the reference alone, and the C ABI of the device tracker (declared, exported, loud without a
device, argument checks that need none)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import nn_cases as NC   # noqa: E402
import nn_ref as R      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NN_SYMBOLS = ["mtfhip_nn_create", "mtfhip_nn_destroy", "mtfhip_nn_build", "mtfhip_nn_set_dataset", "mtfhip_nn_set_dataset_dev", "mtfhip_nn_get_dataset",
              "mtfhip_nn_get_dataset_dev", "mtfhip_nn_search", "mtfhip_nn_search_dev", "mtfhip_nn_update"]


@pytest.mark.parametrize("am", [R.SSD, R.NCC], ids=["ssd", "ncc"])
def test_planted_rows(am):
    rng = np.random.default_rng(1)
    m = rng.uniform(0, 255, size=(40, 49))
    if am == R.NCC:
        m = NC.unit_rows(m)
    dist = R.ssd_dist if am == R.SSD else R.ncc_dist
    # a stored row is its own nearest neighbour, at distance 0 (SSD) / -1 (NCC: minus the correlation of a unit row with itself)
    k, best, second = R.nearest(m, m[17], am)
    assert k == 17 and second > best
    assert best == 0.0 if am == R.SSD else abs(best + 1.0) < 1e-15
    assert abs(dist(m[17], m[3]) - R.distances(m, m[17], am)[3]) <= 1e-12 * abs(dist(m[17], m[3]))
    # a query nearer to row j than to any other finds j
    q = m[29] + 1e-3 * (m[5] - m[29])
    q = NC.unit_rows(q) if am == R.NCC else q
    assert R.nearest(m, q, am)[0] == 29
    # duplicated rows: the first index, and no gap
    m2 = m.copy(); m2[31] = m2[8]
    k, best, second = R.nearest(m2, m2[31], am)
    assert k == 8 and second == best and not R.gap_ok(best, second)
    # one row: no runner-up
    assert R.nearest(m[:1], q, am)[2] == float("inf")


def test_distances_by_hand():
    assert R.ssd_dist([1.0, 2.0, 3.0], [1.5, 2.0, 1.0]) == 4.25 and R.ncc_dist([0.6, 0.8], [0.8, 0.6]) == pytest.approx(-0.96, abs=1e-16)
    # extended precision: three terms of 2^-54 behind a 1 are not lost one by one (a float64 running sum would stay at 1)
    assert R.ssd_dist([1.0] + [2.0 ** -27] * 3, [0.0] * 4) == 1.0 + 2.0 ** -52


@pytest.mark.parametrize("am", [R.SSD, R.NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("shape", NC.SEARCH_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_search_cases_have_a_gap(shape, am):
    F = shape[0] * shape[1] * shape[2]
    m = NC.search_matrix(F, am)
    for n in NC.SEARCH_N:
        for pos in NC.planted_positions(n):
            qs = NC.search_queries(m, n, pos, am, seed=n + pos)
            for j, q in enumerate(qs):
                k, best, second = R.nearest(m[:n], q, am)
                assert n == 1 or R.gap_ok(best, second), (F, n, pos, j, best, second)
                if j == 0:
                    assert k == pos


@pytest.mark.parametrize("case", NC.TRACK_CASES, ids=lambda c: c[0])
def test_tracker_cases_have_a_gap(oracle, frame, frame2, case):
    _, am, ssm, res, ch, kind, max_iters, eps, seed = case
    img0, img1 = NC.track_frames(kind, frame, frame2)
    o_ssm = oracle.SSM(ssm, res, res); o_am = oracle.AM(am, res, res)
    if ch > 1:
        o_am.set_channels(ch); o_ssm.set_channels(ch)
    o_am.set_curr_img(img0)
    o_ssm.set_corners(NC.track_corners_for(kind, res))
    o_am.initialize_pix_vals(o_ssm.get("curr_pts"))
    perts = NC.track_perturbations(ssm, seed)
    feats = oracle.nn_generate_dataset(o_am, o_ssm, perts)
    o_am.set_curr_img(img1)
    r = R.nn_update(o_am, o_ssm, feats, perts, max_iters, eps)
    assert 1 <= r["n_iters"] <= max_iters and (r["n_iters"] == 1 if eps > 1 else r["n_iters"] == max_iters)
    for k, best, second, un in r["log"]:
        assert R.gap_ok(best, second), (case[0], k, best, second)


def test_abi_declares_exports_and_fails_loudly():
    import mtf_amd
    from mtf_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "mtfhip.h")).read()
    assert "stays with FLANN" not in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    lib.mtfhip_last_error.restype = ctypes.c_char_p
    for fn in NN_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % fn, text), fn
        assert hasattr(lib, fn) and fn in L.SYMBOLS
    assert sorted(set(re.findall(r"\b(mtfhip_[a-z_0-9]+)\s*\(", text))) == sorted(L.SYMBOLS)
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.mtfhip_nn_create.argtypes = [vp, ci, vp]
    lib.mtfhip_nn_build.argtypes = [vp, vp, ci]
    lib.mtfhip_nn_search.argtypes = [vp, vp, ci, vp, vp]
    lib.mtfhip_nn_search_dev.argtypes = [vp, vp, ci, vp, vp]
    lib.mtfhip_nn_update.argtypes = [vp, ci, cd, vp, vp, vp]
    for fn in ("mtfhip_nn_set_dataset", "mtfhip_nn_set_dataset_dev", "mtfhip_nn_get_dataset", "mtfhip_nn_get_dataset_dev"):
        getattr(lib, fn).argtypes = [vp, vp, vp]
    lib.mtfhip_nn_destroy.argtypes = [vp]
    # no batch (what a machine without a device is left with: mtfhip_ctx_create fails there): an error with a message, no CPU path
    h = ctypes.c_void_p()
    assert lib.mtfhip_nn_create(None, 100, ctypes.byref(h)) == -1 and b"nn_create" in lib.mtfhip_last_error() and not h.value
    buf = np.zeros(16)
    idx = np.zeros(4, dtype=np.int32)
    p = buf.ctypes.data
    calls = [("nn_build", lambda: lib.mtfhip_nn_build(None, p, 1)), ("nn_set_dataset", lambda: lib.mtfhip_nn_set_dataset(None, p, p)),
             ("nn_set_dataset_dev", lambda: lib.mtfhip_nn_set_dataset_dev(None, p, p)), ("nn_get_dataset", lambda: lib.mtfhip_nn_get_dataset(None, p, p)),
             ("nn_get_dataset_dev", lambda: lib.mtfhip_nn_get_dataset_dev(None, p, p)),
             ("nn_search", lambda: lib.mtfhip_nn_search(None, p, 1, idx.ctypes.data, p)),
             ("nn_search_dev", lambda: lib.mtfhip_nn_search_dev(None, p, 1, idx.ctypes.data, p)),
             ("nn_update", lambda: lib.mtfhip_nn_update(None, 1, 0.01, p, idx.ctypes.data, None)), ("nn_destroy", lambda: lib.mtfhip_nn_destroy(None))]
    for name, call in calls:
        assert call() == -1 and name.encode() in lib.mtfhip_last_error(), name
    if lib.mtfhip_device_count() == 0:
        with pytest.raises(mtf_amd.MtfHipError):
            mtf_amd.Context(0)


def test_argument_checks_need_no_device():
    """n_samples <= 0, Q <= 0 and max_iters <= 0 are refused in front of anything that touches a device: a handle that is only an address
    is enough to reach them"""
    from mtf_amd import _lib as L
    L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    lib.mtfhip_last_error.restype = ctypes.c_char_p
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.mtfhip_nn_create.argtypes = [vp, ci, vp]
    lib.mtfhip_nn_search.argtypes = [vp, vp, ci, vp, vp]
    lib.mtfhip_nn_search_dev.argtypes = [vp, vp, ci, vp, vp]
    lib.mtfhip_nn_update.argtypes = [vp, ci, cd, vp, vp, vp]
    fake = np.zeros(4096, dtype=np.uint8)      # stands in for a handle; the checks below return before reading it
    buf, idx, h = np.zeros(16), np.zeros(4, dtype=np.int32), ctypes.c_void_p()
    f, p, ip = fake.ctypes.data, buf.ctypes.data, idx.ctypes.data
    for n in (0, -5):
        assert lib.mtfhip_nn_create(f, n, ctypes.byref(h)) == -1 and b"n_samples must be positive" in lib.mtfhip_last_error()
        assert lib.mtfhip_nn_search(f, p, n, ip, p) == -1 and b"n_queries must be positive" in lib.mtfhip_last_error()
        assert lib.mtfhip_nn_search_dev(f, p, n, ip, p) == -1 and b"n_queries must be positive" in lib.mtfhip_last_error()
        assert lib.mtfhip_nn_update(f, n, 0.01, p, ip, None) == -1 and b"max_iters must be positive" in lib.mtfhip_last_error()
