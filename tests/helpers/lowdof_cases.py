"""The cases the CPU and the GPU tests of the Similitude / Isometry / Translation state space models share: the frame, the region and the
patch sizes of alk_cases.py, and the frames the frame becomes under one known small warp per model.  Reference results are computed once
per process and cached; nobody modifies them."""
import functools

import numpy as np

import alk_cases as AC
import alk_ref
import lowdof_ref as R

SIM, ISO, TRANS = R.SIM, R.ISO, R.TRANS
SSMS = [TRANS, ISO, SIM]
SSM_IDS = ["trans", "iso", "sim"]
SSD, NCC = 0, 1
ESM, FCLK, ICLK = R.ESM, R.FCLK, R.ICLK
METHODS = [ESM, FCLK, ICLK]
METHOD_IDS = ["esm", "fclk", "iclk"]
SIZES = AC.SIZES            # (50, 50) several workgroups per target, (37, 23) 851 pixels, (7, 5) fewer than a wave
SIZE_IDS = ["%dx%d" % s for s in SIZES]
REGION = AC.REGION
CENTRE = AC.CENTRE
frame0 = AC.frame0


def _hom_state(a00, a01, tx, a10, a11, ty):
    """the warp [[a00, a01, tx], [a10, a11, ty]] in synth.warp_frame's homography parameterisation"""
    return np.array([a00 - 1, a01, tx, a10, a11 - 1, ty, 0.0, 0.0])


_TH = 0.012
# translation (1.9, -1.4); rotation 0.012 rad with translation (1.1, -0.8); similitude a = 0.012, b = 0.008 with translation (0.9, -0.7):
# all about the frame's centre
P_TRUE = {
    TRANS: _hom_state(1.0, 0.0, 1.9, 0.0, 1.0, -1.4),
    ISO: _hom_state(np.cos(_TH), -np.sin(_TH), 1.1, np.sin(_TH), np.cos(_TH), -0.8),
    SIM: _hom_state(1.012, -0.008, 0.9, 0.008, 1.012, -0.7),
}
PARAMS = dict(max_iters=30, epsilon=1e-4)


def warped(ssm):
    return AC.warped(P_TRUE[ssm])


def true_corners(ssm, region=None):
    return alk_ref.warped_corners(REGION if region is None else region, P_TRUE[ssm], CENTRE)


def default_hess(method):
    """the reference's class defaults: ESM SumOfSelf, FCLK CurrentSelf, ICLK InitialSelf (ESMParams.cc, FCLKParams.cc, ICLKParams.cc)"""
    return {ESM: 2, FCLK: 1, ICLK: 0}[method]


@functools.lru_cache(maxsize=None)
def reference(ssm, method, am, size, chained=1, leven_marq=0, hess_type=None):
    """LKRef over lowdof_ref.SSM and oracle_py.AM: initialize on the frame at REGION, update() on the model's warped frame"""
    import oracle_py
    ht = default_hess(method) if hess_type is None else hess_type
    ref, res = R.track(oracle_py, method, am, R.SSM(ssm, *size), frame0(), warped(ssm), REGION, chained_warp=chained, leven_marq=leven_marq,
                       hess_type=ht, **PARAMS)
    return res


# the batch of three: regions at three places of the frame -- the third reaches past the frame's right edge (x up to 320.37 of 320) -- started
# from states of different size so that they stop behind different passes (asserted on the reference in the GPU test).  The isometry
# contracts fastest: its second target starts further out.
BATCH_REGIONS = np.stack([AC.BATCH_REGIONS[0], AC.BATCH_REGIONS[1], AC.synth.square_corners(281, 150, 78)])
_STARTS = {
    TRANS: np.array([[0.0, 0.0], [4.5, -3.5], [-0.6, 0.5]]),
    ISO: np.array([[0.0, 0.0, 0.0], [7.0, -5.5, 0.06], [-0.6, 0.5, -0.002]]),
    SIM: np.array([[0.0, 0.0, 0.0, 0.0], [4.5, -3.5, 0.02, -0.012], [-0.6, 0.5, -0.002, 0.002]]),
}
# the state one fused pass is compared at: away from the identity, inside the basin
PASS_START = {TRANS: np.array([1.6, -1.2]), ISO: np.array([1.6, -1.2, 0.006]), SIM: np.array([1.6, -1.2, 0.006, -0.004])}


def batch_start(ssm, t):
    """[tx, ty] | [tx, ty, theta] | [tx, ty, a, b] of target t"""
    return _STARTS[ssm][t].copy()


@functools.lru_cache(maxsize=None)
def batch_reference(ssm, method, am, size, leven_marq=0, hess_type=None, jac_type=1):
    import oracle_py
    out = []
    for t in range(3):
        o_ssm = R.SSM(ssm, *size)
        o_am = oracle_py.AM(am, *size)
        o_am.set_curr_img(frame0())
        ref = R.LKRef(method, o_am, o_ssm, hess_type=default_hess(method) if hess_type is None else hess_type, jac_type=jac_type,
                      leven_marq=leven_marq, max_iters=15, epsilon=1e-4)
        ref.initialize(BATCH_REGIONS[t])
        o_ssm.set_state(batch_start(ssm, t))
        o_am.set_curr_img(warped(ssm))
        out.append(ref.update())
    return out
