"""CPU: the batch-free StateSpaceModel entry points of the C ABI -- mtfhip_ssm_identity_warp, _compose_warps, _apply_warp_to_pts,
_estimate_warp_from_corners: host algebra, callable without a device -- for MTFHIP_SSM_SIMILITUDE / _ISOMETRY / _TRANSLATION against
tests/helpers/lowdof_ref.py, to 1e-12.  Before the three models were added every one of these calls returned MTFHIP_ERR_INVALID_ARG
("unknown state space model")."""
import os
import sys

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lowdof_cases as LC    # noqa: E402
import lowdof_ref as R       # noqa: E402

STATES = {R.TRANS: [np.array([1.7, -2.3]), np.array([-0.4, 0.6])],
          R.ISO: [np.array([1.7, -2.3, 0.04]), np.array([-0.4, 0.6, -0.015])],
          R.SIM: [np.array([1.7, -2.3, 0.03, -0.02]), np.array([-0.4, 0.6, -0.01, 0.012])]}


def test_constants_follow_the_header():
    assert (L.SSM_SIMILITUDE, L.SSM_ISOMETRY, L.SSM_TRANSLATION) == (2, 3, 4) == (R.SIM, R.ISO, R.TRANS)
    assert (mtf_amd.SSM_SIMILITUDE, mtf_amd.SSM_ISOMETRY, mtf_amd.SSM_TRANSLATION) == (2, 3, 4)
    assert [L.ssm_state_size(s) for s in (0, 1, 2, 3, 4)] == [8, 6, 4, 3, 2]
    with pytest.raises(L.InvalidArgument):
        L.ssm_state_size(5)


@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_identity_warp(ssm):
    out = mtf_amd.identity_warp(ssm)
    assert out.shape == (R.STATE_SIZE[ssm],) and not out.any()


@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_compose_warps(ssm):
    ref = R.SSM(ssm, 5, 5)
    p1, p2 = STATES[ssm]
    got = mtf_amd.compose_warps(ssm, p1, p2)
    assert got.shape == (ref.S,)
    assert np.abs(got - ref.compose_warps(p1, p2)).max() < 1e-12


@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_apply_warp_to_pts(ssm):
    ref = R.SSM(ssm, 5, 5)
    pts = np.random.default_rng(7).uniform(0, 300, size=(2, 11))
    for p in STATES[ssm]:
        got = mtf_amd.apply_warp_to_pts(ssm, pts, p)
        assert np.abs(got - ref.apply_warp_to_pts(pts, p)).max() < 1e-12 * 300


@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_estimate_warp_from_corners(ssm):
    """the model's own fit (Translation: centroid difference; Similitude: computeSimilitudeDLT; Isometry: its rotation) of corners moved by
    a model warp -- recovered -- and of corners moved by a general homography, where the fit is a genuine least-squares answer"""
    ref = R.SSM(ssm, 5, 5)
    rng = np.random.default_rng(8)
    outs = [ref.apply_warp_to_corners(LC.REGION, STATES[ssm][0]), LC.REGION + rng.uniform(-3, 3, size=(2, 4))]
    for k, out in enumerate(outs):
        got = mtf_amd.estimate_warp_from_corners(ssm, LC.REGION, out)
        want = ref.estimate_warp_from_corners(LC.REGION, out)
        print("estimate_warp_from_corners ssm %d case %d: %.3e" % (ssm, k, np.abs(got - want).max()))
        assert got.shape == (ref.S,)
        assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    assert np.abs(mtf_amd.estimate_warp_from_corners(ssm, LC.REGION, outs[0]) - STATES[ssm][0]).max() < 1e-11


def test_unknown_model_is_still_refused():
    with pytest.raises(L.InvalidArgument):
        out = np.empty(8)
        L.check(L.lib().mtfhip_ssm_identity_warp(5, out.ctypes.data_as(L.C.POINTER(L.C.c_double))))


@pytest.mark.parametrize("ssm", LC.SSMS, ids=LC.SSM_IDS)
def test_trackers_that_are_not_served_say_so_before_any_device_call(ssm):
    """GridTracker, ParticleFilter, NNDataset and NNTracker raise for the three models without touching the context (None here)"""
    from mtf_amd import sm
    with pytest.raises(L.FunctionNotImplemented):
        sm.GridTracker(None, ssm=ssm)
    with pytest.raises(L.FunctionNotImplemented):
        sm.GridTracker(None, grid_ssm=ssm)
    with pytest.raises(L.FunctionNotImplemented):
        sm.ParticleFilter(None, ssm=ssm)
    with pytest.raises(L.FunctionNotImplemented):
        sm.NNDataset(None, ssm=ssm)
    with pytest.raises(L.FunctionNotImplemented):
        sm.NNTracker(None, ssm=ssm)
