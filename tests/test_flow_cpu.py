"""CPU: the NumPy restatement of NCC::estimateOpticalFlow / nt::GridTrackerFlow (tests/helpers/flow_ref.py) held to facts that do not come
from it, and the C ABI of the device flow (declared, exported, descriptor layout, the refusals that need no device)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import flow_cases as FC   # noqa: E402
import flow_ref as R      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scalar_and_array_sampler_agree_bit_for_bit():
    f0, _ = FC.frames()
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-3, 515, 400), [0.0, 300.0, 511.0, 510.999, 511.5, -1e-9, 17.0, 17.0 + 1e-8, 17.0 - 1e-8]])
    y = np.concatenate([rng.uniform(-3, 515, 400), [0.0, 256.0, 511.0, 3.25, 100.0, 5.0, 511.0, 44.0, 44.0]])
    assert np.array_equal(R.pix_vals(f0, x, y), np.array([R.pix_val(f0, a, b) for a, b in zip(x, y)]))
    # the lattice: LinSpaced with the step w / (w - 1), the last element exactly hi
    w = R.lin_spaced(10, 95.0, 105.0)
    assert w[0] == 95.0 and w[-1] == 105.0 and w[1] - w[0] == pytest.approx(10.0 / 9.0, rel=1e-15)
    assert np.array_equal(R.lin_spaced(2, 299.0, 301.0), [299.0, 301.0])


def test_qr_solve_2x2():
    rng = np.random.default_rng(3)
    for _ in range(20):
        A, b = rng.normal(size=(2, 2)), rng.normal(size=2)
        np.testing.assert_allclose(R.colpiv_qr_solve2(A, b), np.linalg.solve(A, b), rtol=1e-10, atol=1e-13)
    assert np.array_equal(R.colpiv_qr_solve2(np.zeros((2, 2)), np.ones(2)), [0, 0])
    assert np.isnan(R.colpiv_qr_solve2(np.array([[np.nan, 0], [0, 1.0]]), np.ones(2))).all()


@pytest.mark.parametrize("win,tol,passes", [((10, 10), 0.05, 3), ((25, 25), 0.02, 2)], ids=["10x10", "25x25"])
@pytest.mark.parametrize("const_grad", [False, True], ids=["grad_curr", "const_grad"])
def test_known_shift_is_recovered(win, tol, passes, const_grad):
    """a frame shifted by (1.3, -0.8): the flow of interior points is the shift (properties of the reference, measured with the restatement:
    25 x 25 within 0.01 px in 2 passes, 10 x 10 within 0.04 px in 3)"""
    pts = np.asarray(FC.INTERIOR, dtype=np.float32)
    cp, ni, st, logs = FC.ref_flow(FC.key(pts), win, 30, const_grad)
    d = cp.astype(np.float64) - pts.astype(np.float64)
    print("known shift", win, const_grad, d.tolist(), ni.tolist(), st.tolist())
    assert (st == R.CONVERGED).all()
    assert np.abs(d - np.asarray(FC.SHIFT)).max() < tol
    for p, log in enumerate(logs):          # ... and already after `passes` passes
        moved = np.sum([rec["opt_flow"] for rec in log[:passes]], axis=0)
        assert np.abs(moved - np.asarray(FC.SHIFT)).max() < tol, (p, moved)


def test_window_off_the_frame_is_not_finite():
    cp, ni, st, logs = FC.ref_flow(FC.key([FC.OUTSIDE]), (10, 10), 30, False)
    assert np.isnan(cp).all() and st[0] == R.NONFINITE and ni[0] == 1 and len(logs[0]) == 1
    # and it does not disturb its neighbours in a batch
    pts = FC.batch_points(3)
    cp3, ni3, st3, _ = FC.ref_flow(FC.key(pts), (10, 10), 30, False)
    one = FC.ref_flow(FC.key(pts[:1]), (10, 10), 30, False)
    assert np.array_equal(cp3[0], one[0][0]) and st3[1] == R.NONFINITE and np.isnan(cp3[1]).all() and st3[0] == R.CONVERGED


def test_tracker_restatement_follows_a_shift():
    f0, f1 = FC.frames()
    from mtf_amd.sm import least_squares_estimator
    from mtf_amd import _lib as L
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy_ref as NR
    region = np.array([[150.0, 350, 350, 150], [160, 160, 340, 340]])
    t = R.GridTrackerFlowRef(lambda r: NR.grid_layout(r, 4, 4, 1, 1, 0, 0)[0], least_squares_estimator(L.SSM_AFFINE), True, (25, 25))
    t.set_image(f0); t.initialize(region)
    assert t.prev_pts.dtype == np.float32 and np.allclose(t.prev_pts[0], region[:, 0]) and np.allclose(t.prev_pts[-1], region[:, 2])
    t.set_image(f1)
    out = t.update()
    np.testing.assert_allclose(out - region, np.tile(np.asarray(FC.SHIFT)[:, None], (1, 4)), atol=0.05)
    assert np.array_equal(t.prev_pts, t.curr_pts)          # the points drift: not put back on the grid


def test_abi_declares_exports_layout_and_refusals():
    import mtf_amd
    from mtf_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "mtfhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    lib.mtfhip_last_error.restype = ctypes.c_char_p
    fns = ("mtfhip_ncc_estimate_optical_flow", "mtfhip_ncc_estimate_optical_flow_dev", "mtfhip_ncc_estimate_optical_flow_trace")
    for fn in fns:
        assert re.search(r"\bint\s+%s\s*\(" % fn, text), fn
        assert hasattr(lib, fn) and fn in L.SYMBOLS
    # the documented layout of mtfhip_flow_desc: the fields in the header's order, natural alignment
    m = re.search(r"typedef struct mtfhip_flow_desc \{(.*?)\} mtfhip_flow_desc;", text, flags=re.S)
    names = re.findall(r"(?:int|double)\s+([^;]+);", m.group(1))
    names = [n.strip() for part in names for n in part.split(",")]
    assert names == ["win_w", "win_h", "max_iters", "epsilon", "const_grad", "grad_eps", "math_mode"] == [f[0] for f in L.FlowDesc._fields_]
    assert [getattr(L.FlowDesc, n).offset for n in names] == [0, 4, 8, 16, 24, 32, 40] and ctypes.sizeof(L.FlowDesc) == 48
    d = L.flow_desc()
    assert (d.win_w, d.win_h, d.max_iters, d.epsilon, d.const_grad, d.grad_eps) == (10, 10, 30, 0.01, 0, 1e-8)   # GridTrackerFlowParams.h:6-17
    # refusals that need no device
    for fn in fns[:2]:
        getattr(lib, fn).argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    lib.mtfhip_ncc_estimate_optical_flow_trace.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int]
    pp, cp = np.zeros((4, 2), dtype=np.float32), np.zeros((4, 2), dtype=np.float32)
    ni, st, tr = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32), np.zeros((4, 30, 8))
    arrs = (pp.ctypes.data, cp.ctypes.data, ni.ctypes.data, st.ctypes.data)

    def call(desc, n=4, which=0, a=arrs):
        if which == 2:
            return lib.mtfhip_ncc_estimate_optical_flow_trace(None, ctypes.byref(desc) if desc is not None else None, n, *a, tr.ctypes.data, 30)
        return getattr(lib, fns[which])(None, ctypes.byref(desc) if desc is not None else None, n, *a)
    for which in (0, 1, 2):
        assert call(L.flow_desc(), which=which) == -1 and fns[which][7:].encode() in lib.mtfhip_last_error()   # no context
        assert call(None, which=which) == -1
        assert call(L.flow_desc(), which=which, a=(None,) * 4) == -1                                           # NULL arrays
        assert call(L.flow_desc(win=(1, 10)), which=which) == -1 and call(L.flow_desc(win=(10, 1)), which=which) == -1
        assert call(L.flow_desc(), n=0, which=which) == -1 and call(L.flow_desc(max_iters=0), which=which) == -1
        assert call(L.flow_desc(math=7), which=which) == -1
        assert call(L.flow_desc(win=(33, 32)), which=which) == -2 and b"1024" in lib.mtfhip_last_error()        # 1056 samples
        assert call(L.flow_desc(win=(33, 31)), which=which) == -1                                              # 1023: only the context is missing
    if lib.mtfhip_device_count() == 0:
        with pytest.raises(mtf_amd.MtfHipError):
            mtf_amd.Context(0)


def test_python_driver_refuses_low_order_grid_ssms():
    from mtf_amd import _lib as L
    from mtf_amd.sm import GridTrackerFlow
    for ssm in (L.SSM_TRANSLATION, L.SSM_ISOMETRY, L.SSM_SIMILITUDE):
        with pytest.raises(L.FunctionNotImplemented):
            GridTrackerFlow(None, grid_ssm=ssm)
    g = GridTrackerFlow(None, grid_size=4, search_window=7, pyramid_levels=3, min_eig_thresh=0.5)      # carried, ignored
    assert g.n == 16 and g.win == (7, 7) and (g.pyramid_levels, g.min_eig_thresh) == (3, 0.5) and g.pix_mask.all()
