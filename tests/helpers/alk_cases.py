"""The cases the CPU and the GPU tests of nt::FALK / nt::IALK share: one 320 x 240 synthetic frame, the frames it becomes under a known small
homography and a known small affine warp, the patch sizes, the Levenberg-Marquardt cases in which the reference rejects steps, and the three
targets of the batch test.  Reference results are computed once per process and cached; nobody modifies them."""
import functools

import numpy as np

import alk_ref as R
from mtf_amd import synth

FALK, IALK = R.FALK, R.IALK
SSD, NCC = 0, 1
HOM, AFF = 0, 1
H, W = 240, 320
CENTRE = (160.0, 120.0)
# 50 x 50: the shipped NN / PF size (several workgroups per target); 37 x 23: 851 pixels, no multiple of 64 or 256; 7 x 5: fewer than a wave
SIZES = [(50, 50), (37, 23), (7, 5)]
REGION = synth.square_corners(160, 120, 90)

# homography state [h00-1, h01, h02, h10, h11-1, h12, h20, h21]; the affine warp in the same parameterisation
P_HOM = synth.random_small_homography(np.random.default_rng(5), 0.5)
P_AFF = np.array([0.012, -0.008, 0.9, 0.006, -0.01, -0.7, 0.0, 0.0])


def name(method):
    return "FALK" if method == FALK else "IALK"


@functools.lru_cache(maxsize=None)
def frame0():
    f = synth.make_frame(H, W, seed=11)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _warped(key):
    f = synth.warp_frame(frame0(), np.array(key), CENTRE)
    f.setflags(write=False)
    return f


def warped(p):
    return _warped(tuple(float(v) for v in p))


def warp_of(ssm):
    """the known warp a state space model is tested on: the homography for the homography, the affine one for the affine"""
    return P_HOM if ssm == HOM else P_AFF


# Levenberg-Marquardt: warps and lm_delta_init under which the reference itself takes steps back (found by search over seeds; asserted on
# the reference alone in test_alk_ref.py), 37 x 23, SSD, homography, InitialSelf
LM_CASES = {
    FALK: dict(p=synth.random_small_homography(np.random.default_rng(4), 3.0), lm_delta_init=1.0, max_iters=20, epsilon=1e-3),
    IALK: dict(p=synth.random_small_homography(np.random.default_rng(5), 3.0), lm_delta_init=1.0, max_iters=20, epsilon=1e-3),
}


@functools.lru_cache(maxsize=None)
def lm_reference(method):
    import oracle_py
    c = LM_CASES[method]
    ref, res = R.track(oracle_py, method, SSD, HOM, 37, 23, frame0(), warped(c["p"]), REGION, hess_type=0, leven_marq=1,
                       lm_delta_init=c["lm_delta_init"], lm_delta_update=10.0, max_iters=c["max_iters"], epsilon=c["epsilon"])
    return res


# the batch of three: regions at three places of the frame, tracked on the homography-warped frame from start states of growing size, so
# that the targets stop behind different passes
BATCH_REGIONS = np.stack([synth.square_corners(110, 95, 70), synth.square_corners(160, 120, 90), synth.square_corners(215, 150, 64)])
BATCH_STARTS = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                         [0.012, -0.009, 2.4, 0.006, 0.015, -1.8, 3e-5, -3e-5],
                         [-0.012, 0.009, -2.2, 0.01, -0.011, 1.9, 4e-5, 3e-5]])
BATCH_PARAMS = dict(hess_type=1, max_iters=15, epsilon=1e-4, leven_marq=0)


@functools.lru_cache(maxsize=None)
def batch_reference(method, am, ssm, size):
    """per target: the reference's update() on the warped frame from BATCH_STARTS[t] (the first S components)"""
    import oracle_py
    out = []
    for t in range(3):
        o_ssm = oracle_py.SSM(ssm, size[0], size[1])
        o_am = oracle_py.AM(am, size[0], size[1])
        o_am.set_curr_img(frame0())
        ref = R.AlkRef(method, o_am, o_ssm, **BATCH_PARAMS)
        ref.initialize(BATCH_REGIONS[t])
        o_ssm.set_state(batch_start(ssm, t))
        o_am.set_curr_img(warped(P_HOM))
        out.append(ref.update())
    return out


def batch_start(ssm, t):
    s = BATCH_STARTS[t]
    if ssm == HOM:
        return s.copy()
    return np.array([s[2], s[5], s[0], s[1], s[3], s[4]])   # affine state [tx, ty, a-1, b, c, d-1]
