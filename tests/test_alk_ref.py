"""CPU: the search-method values of the additive Lucas-Kanade methods (MTFHIP_SM_FALK / _IALK) in the header, the Python mirror and the built
library; the restatement of nt::FALK / nt::IALK over the oracle (tests/helpers/alk_ref.py) on a known homography and a known affine warp; the
affine identity cmptPixJacobian == cmptInitPixJacobian and what it means for FALK's InitialSelf Hessian; and the Levenberg-Marquardt cases
the GPU tests reuse, which must reject steps on the reference itself."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import alk_cases as AC   # noqa: E402
import alk_ref as R      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_search_method_values_agree():
    from mtf_amd import _lib as L
    import mtf_amd
    assert L.SM_FALK == 3 and L.SM_IALK == 4
    assert mtf_amd.SM_FALK == 3 and mtf_amd.SM_IALK == 4
    hdr = open(os.path.join(ROOT, "include", "mtfhip.h")).read()
    assert int(re.search(r"MTFHIP_SM_FALK\s*=\s*(\d+)", hdr).group(1)) == L.SM_FALK
    assert int(re.search(r"MTFHIP_SM_IALK\s*=\s*(\d+)", hdr).group(1)) == L.SM_IALK
    assert (R.FALK, R.IALK) == (L.SM_FALK, L.SM_IALK)
    # the class default of FALKParams.cc:5 / IALKParams.cc:6
    assert mtf_amd.sm_desc(L.SM_FALK).hess_type == 0 and mtf_amd.sm_desc(L.SM_IALK).hess_type == 0


def test_library_argument_check_knows_the_methods():
    """mtfhip_batch_init_template's argument check needs no device: with FALK / IALK an out-of-range hess_type is reported as such (the
    value was recognised and FALKParams' range applied), where a value the library does not know never gets that far"""
    from mtf_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail("libmtfhip.so is missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(L.LIB_PATH)
    lib.mtfhip_last_error.restype = ctypes.c_char_p
    for sm_kind in (L.SM_FALK, L.SM_IALK):
        sm = L.SMDesc(sm=sm_kind, hess_type=3, max_iters=1)
        rc = lib.mtfhip_batch_init_template(None, ctypes.byref(sm))
        assert rc == -1
        assert ("hess_type 3 invalid for search method %d" % sm_kind) in lib.mtfhip_last_error().decode()
        sm.hess_type = 0
        assert lib.mtfhip_batch_init_template(None, ctypes.byref(sm)) == -1
        assert "NULL argument" in lib.mtfhip_last_error().decode()
    sm = L.SMDesc(sm=7, hess_type=3, max_iters=1)
    assert lib.mtfhip_batch_init_template(None, ctypes.byref(sm)) == -1
    assert "hess_type" not in lib.mtfhip_last_error().decode()


# the reference's own mean corner error (pixels) behind update() on the 50 x 50 patch, InitialSelf, max_iters 10, epsilon 1e-4, and its
# n_iters, as computed by tests/helpers/alk_ref.py when the cases were written:
#   (method, am, ssm)          n_iters  start    pass 1   pass 2   final
#   FALK SSD homography        3        0.5140   0.0214   0.0061   0.0058
#   FALK NCC homography        3        0.5140   0.0199   0.0064   0.0055
#   IALK SSD homography        3        0.5140   0.0262   0.0074   0.0068
#   IALK NCC homography        3        0.5140   0.0246   0.0065   0.0055
#   FALK SSD affine            4        1.3771   0.0958   0.0045   0.0039
#   FALK NCC affine            3        1.3771   0.0792   0.0040   0.0018
#   IALK SSD affine            3        1.3771   0.0895   0.0057   0.0051
#   IALK NCC affine            3        1.3771   0.0807   0.0036   0.0029
RECORDED_FINAL = {
    (AC.FALK, AC.SSD, AC.HOM): 0.0058, (AC.FALK, AC.NCC, AC.HOM): 0.0055, (AC.IALK, AC.SSD, AC.HOM): 0.0068, (AC.IALK, AC.NCC, AC.HOM): 0.0055,
    (AC.FALK, AC.SSD, AC.AFF): 0.0039, (AC.FALK, AC.NCC, AC.AFF): 0.0018, (AC.IALK, AC.SSD, AC.AFF): 0.0051, (AC.IALK, AC.NCC, AC.AFF): 0.0029,
}


@pytest.mark.parametrize("ssm", [AC.HOM, AC.AFF], ids=["hom", "aff"])
@pytest.mark.parametrize("am", [AC.SSD, AC.NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("method", [AC.FALK, AC.IALK], ids=AC.name)
def test_reference_converges_on_a_known_warp(oracle, method, am, ssm):
    p = AC.warp_of(ssm)
    truth = R.warped_corners(AC.REGION, p, AC.CENTRE)
    ref, res = R.track(oracle, method, am, ssm, 50, 50, AC.frame0(), AC.warped(p), AC.REGION, max_iters=10, epsilon=1e-4)
    errs = [R.corner_error(AC.REGION.T.ravel(), truth)] + [R.corner_error(rec["corners"], truth) for rec in res["log"]]
    assert errs[0] > errs[1] > errs[2], errs          # monotonic over the first passes
    assert res["n_iters"] < 10                          # stopped by epsilon
    assert res["log"][-1]["update_norm"] < 1e-4
    assert errs[-1] <= 10 * RECORDED_FINAL[(method, am, ssm)], errs
    # the log is what the GPU tests compare with: the state is the sum of the updates (additiveUpdate), the corners its image
    np.testing.assert_allclose(res["state"], sum(rec["dp"] for rec in res["log"]), rtol=0, atol=1e-13)
    np.testing.assert_array_equal(res["corners"], res["log"][-1]["corners"])


@pytest.mark.parametrize("size", AC.SIZES, ids=lambda s: "%dx%d" % s)
def test_affine_pix_jacobian_is_the_init_pix_jacobian(oracle, size):
    """Affine.h:35-37: cmptPixJacobian forwards to cmptInitPixJacobian -- bit for bit, at any state"""
    o_ssm = oracle.SSM(AC.AFF, *size)
    o_ssm.set_corners(AC.REGION)
    o_ssm.set_state(AC.batch_start(AC.AFF, 2))
    grad = np.random.default_rng(3).normal(0, 20, size=2 * size[0] * size[1])
    assert np.array_equal(o_ssm.cmpt_pix_jacobian(grad), o_ssm.cmpt_init_pix_jacobian(grad))


@pytest.mark.parametrize("am", [AC.SSD, AC.NCC], ids=["ssd", "ncc"])
def test_affine_falk_initial_self_hessian_is_fclks(oracle, am):
    """... so FALK's InitialSelf Hessian (FALK.cc:110-118) is the one nt::FCLK keeps (FCLK.cc:120-128) at initialisation: the chained FCLK
    builds its template Jacobian with cmptWarpedPixJacobian at the identity state, whose affine rows are Ix * 1 + Iy * 0 -- the same bits"""
    res = 37, 23
    o_ssm = oracle.SSM(AC.AFF, *res); o_am = oracle.AM(am, *res); o_am.set_curr_img(AC.frame0())
    ref = R.AlkRef(R.FALK, o_am, o_ssm, hess_type=0)
    ref.initialize(AC.REGION)
    f_ssm = oracle.SSM(AC.AFF, *res); f_am = oracle.AM(am, *res); f_am.set_curr_img(AC.frame0())
    trk = oracle.Tracker(oracle.SM_FCLK, f_am, f_ssm, hess_type=0, chained_warp=1, leven_marq=0, max_iters=1)
    trk.initialize(AC.REGION)
    trk.update()
    assert np.array_equal(np.asarray(ref.H0), np.asarray(trk.trace()[0]["H"]))


@pytest.mark.parametrize("method", [AC.FALK, AC.IALK], ids=AC.name)
def test_reference_rejects_steps_under_levenberg_marquardt(oracle, method):
    """the Levenberg-Marquardt cases of the GPU tests exercise the reject path: on the reference alone at least one step is taken back, the
    pass after a rejected one is never rejected (state_reset), the damping grows with every rejection, and the loop still stops by epsilon"""
    res = AC.lm_reference(method)
    log = res["log"]
    undo = [rec["undo"] for rec in log]
    assert sum(undo) >= 1
    assert not any(a and b for a, b in zip(undo, undo[1:]))
    assert not undo[0]
    for k in range(1, len(log)):
        if undo[k]:
            assert log[k]["lm_delta"] == pytest.approx(10.0 * log[k - 1]["lm_delta"])
            assert log[k]["f"] < log[k - 1]["f"]          # (the pass before a rejected one was accepted: its f is prev_f)
    assert res["n_iters"] < AC.LM_CASES[method]["max_iters"]
    assert not undo[-1] and log[-1]["update_norm"] < AC.LM_CASES[method]["epsilon"]
    # a rejected step is taken back exactly: the state behind it is the state before the step it undoes, up to the rounding of s + u - u
    for k in range(2, len(log)):
        if undo[k]:
            np.testing.assert_allclose(log[k]["state"], log[k - 2]["state"], rtol=0, atol=1e-12)


def test_batch_targets_stop_at_different_passes(oracle):
    """the three targets of the GPU batch test stop behind different passes on the reference"""
    for method, am, ssm in ((AC.FALK, AC.SSD, AC.HOM), (AC.IALK, AC.NCC, AC.AFF)):
        n = [r["n_iters"] for r in AC.batch_reference(method, am, ssm, (50, 50))]
        assert len(set(n)) == 3, n
