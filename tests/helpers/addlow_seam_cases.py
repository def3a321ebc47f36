"""The cases tests/test_alk_lowdof_seams_cpu.py (the references alone) and tests/test_gpu_alk_lowdof_seams.py (the device against them) share:
the additive search methods FALK / IALK (reference: alk_ref.AlkRef over oracle_py) and the Similitude / Isometry / Translation state space
models under ESM / FCLK / ICLK (reference: lowdof_ref.LKRef over lowdof_ref.SSM), at the pixel counts where the kernels' decompositions
have a seam, on regions that are projective, cross a frame edge or lie outside the frame (the regions, frames and yardsticks of
lk_seam_cases.py), and on single targets large enough for the finish kernels' 256-thread, three-run row sum.  Importable without a GPU.

A model of the table is (method, appearance model, state space model[, ESM's Original Jacobian + Hessian]); a case runs every variant of
its model -- the three hess_type of an additive method, both chained_warp values of a low-order one -- so the 8 + 24 models of the table
stand for 24 + 48 parameter sets.  The table is not the cross product: each of the 36 (shape, region) pairs takes every third model,
shifted by the pair's index.  The three FULL_SHAPES of a region, and the BIG_SHAPES of `inside` and of `quad`, are consecutive pairs, so
every model meets every region, every model meets a BIG shape, and every model meets `quad` on a BIG shape.

Reference results are computed once per process and cached; nobody modifies them."""
import collections

import numpy as np

import alk_cases as AC
import alk_ref
import lowdof_cases as LC
import lowdof_ref as LR
from lk_seam_cases import REGIONS, HALF_OUTSIDE, rel, g_scale, long_double_solve, dp_ulp_sensitivity   # noqa: F401
from lk_seam_cases import SHAPES as _LK_SHAPES

FALK, IALK = alk_ref.FALK, alk_ref.IALK
ESM, FCLK, ICLK = LR.ESM, LR.FCLK, LR.ICLK
SSD, NCC = 0, 1
HOM, AFF = 0, 1
SIM, ISO, TRANS = LR.SIM, LR.ISO, LR.TRANS
ALK, LOW = "alk", "low"

SHAPES = list(_LK_SHAPES)
FULL_SHAPES = [(5, 7), (32, 33), (37, 23)]
# one target of N = 8281, 9215, 16512, 24964 pixels: 9, 9, 17, 25 partial rows (the finish kernels take 256 threads and three runs above
# eight: runs [0,8) [8,9) [16,9) -- the third starts past the end --, a one-row last run at 17, a one-row last run of the 16-row cut at 25);
# 95 x 97 leaves 255 pixels in the last 256-pixel row
BIG_SHAPES = [(91, 91), (95, 97), (129, 128), (158, 158)]
FRAME_SIZE = 512


def fused_decomposition(N, B, slots=512, min_rows=4, block=256):
    """fused_decomposition of mtf_amd/csrc/mtfhip_internal.h restated: (nblk, rows) -- a target's ceil(N / block) pixel rows are cut into
    nblk chunks of `rows` rows, at least min_rows each, the cut with the least rounds of `slots` resident workgroups x (rows + 1.5)"""
    total_rows = (N + block - 1) // block
    nb_max = max((total_rows + min_rows - 1) // min_rows, 1)
    B = max(B, 1)
    best, best_nb = 1e300, 1
    for nb in range(1, nb_max + 1):
        r = (total_rows + nb - 1) // nb
        real_nb = (total_rows + r - 1) // r
        rounds = (B * real_nb + slots - 1) // slots
        cost = float(rounds) * (r + 1.5)
        if cost < best - 1e-9:
            best, best_nb = cost, real_nb
    rows = (total_rows + best_nb - 1) // best_nb
    return (total_rows + rows - 1) // rows, rows


# extra: what is fixed for the model (low order: ESM's jac_type / hess_type when not the class default; loop models: hess_type, leven_marq)
Model = collections.namedtuple("Model", "family sm ssm am extra")
Case = collections.namedtuple("Case", "id resx resy region model reference_nan nblk alt_start")

_SM_NAME = {(ALK, FALK): "FALK", (ALK, IALK): "IALK", (LOW, ESM): "ESM", (LOW, FCLK): "FCLK", (LOW, ICLK): "ICLK"}
_SSM_NAME = {(ALK, HOM): "hom", (ALK, AFF): "aff", (LOW, SIM): "sim", (LOW, ISO): "iso", (LOW, TRANS): "trans"}


def model_name(m):
    return "%s-%s-%s%s" % (_SM_NAME[m.family, m.sm], ("SSD", "NCC")[m.am], _SSM_NAME[m.family, m.ssm],
                           "".join("-%s%s" % kv for kv in sorted(m.extra.items())))


def _models():
    alk = [Model(ALK, sm, ssm, am, {}) for sm in (FALK, IALK) for am in (SSD, NCC) for ssm in (HOM, AFF)]
    low = []
    for ssm in (TRANS, ISO, SIM):
        for am in (SSD, NCC):
            for sm in (ESM, FCLK, ICLK):
                low.append(Model(LOW, sm, ssm, am, {}))
            low.append(Model(LOW, ESM, ssm, am, dict(jac_type=0, hess_type=3)))     # Original + Original: the mean pixel Jacobian
    return alk, low


ALK_MODELS, LOW_MODELS = _models()
MODELS = ALK_MODELS + LOW_MODELS
STRIDE = 3


def variants(m):
    """the parameter sets one case of a model runs: (label, sm_desc / reference parameters)"""
    if m.family == ALK:
        return [("ht%d" % ht, dict(hess_type=ht)) for ht in (0, 1, 2)]
    base = dict(hess_type=LC.default_hess(m.sm), jac_type=1)
    base.update(m.extra)
    return [("chained" if ch else "nonchained", dict(base, chained_warp=ch)) for ch in (1, 0)]


def start_state(m, alt=False):
    """the state the compared pass runs at: away from the identity, inside the basin (alt: the additive cases of ALT_START)"""
    return AC.batch_start(m.ssm, 2 if alt else 1) if m.family == ALK else LC.PASS_START[m.ssm].copy()


# Cases whose reference breaks the jitter floor at the usual start state (condition (e) of tests/test_alk_lowdof_seams_cpu.py: corners moved
# by 1e-12 px move H by 1.2e-6 .. 1.6e-6 -- four and six pixels under NCC, and IALK's NCC Std Hessian, in which the 1e-6 noise of the
# stored template gradient's 1e-8 central difference survives a cancellation): they run at alk_cases.batch_start(ssm, 2) instead, where
# six seeded sign patterns stay below 7.7e-7
ALT_START = {"2x2-inside-FALK-NCC-aff", "2x3-inside-FALK-NCC-hom", "7x9-inside-IALK-NCC-hom", "37x23-quad-IALK-NCC-hom"}


PAIRS = ([(s, "inside") for s in SHAPES] + [(s, r) for r in list(REGIONS)[1:] for s in FULL_SHAPES] +
         [(s, "inside") for s in BIG_SHAPES] + [(s, "quad") for s in BIG_SHAPES])


def _build_cases():
    out = []
    for ci, ((resx, resy), region) in enumerate(PAIRS):
        for mi, m in enumerate(MODELS):
            if (ci + mi) % STRIDE:
                continue
            cid = "%dx%d-%s-%s" % (resx, resy, region, model_name(m))
            out.append(Case(cid, resx, resy, region, m, m.am == NCC and region == "outside", fused_decomposition(resx * resy, 1)[0],
                            cid in ALT_START))
    return out


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]


def n_pix(c):
    return c.resx * c.resy


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)
    return x


# ---------------------------------------------------------------- one pass away from the identity
def alk_first_pass(oracle, frame, frame2, m, resx, resy, corners, alt=False):
    """AlkRef initialised on `frame` inside `corners`, one pass on `frame2` at start_state(m) for every hess_type: the grid, the template
    arrays, the points the pass samples, and per variant the pass's record (f, g, H, dp, It, Jt, dIt_dx)"""
    o_ssm = oracle.SSM(m.ssm, resx, resy)
    o_am = oracle.AM(m.am, resx, resy)
    o_am.set_curr_img(frame)
    ref = alk_ref.AlkRef(m.sm, o_am, o_ssm, hess_type=0, max_iters=1, leven_marq=0)
    ref.initialize(corners)
    out = dict(init_pts=o_ssm.get("init_pts").reshape(-1, 2).T.copy(), init_pts_hm=o_ssm.get("init_pts_hm").reshape(-1, 3).T.copy(),
               I0=o_am.get("I0").copy(), start=start_state(m, alt), recs={})
    o_am.set_curr_img(frame2)
    for label, p in variants(m):
        ref.p["hess_type"] = p["hess_type"]
        o_ssm.set_state(out["start"])
        out["curr_pts"] = o_ssm.get("curr_pts").reshape(-1, 2).T.copy()
        out["recs"][label] = ref.update()["log"][0]
    return out


def low_first_pass(oracle, frame, frame2, m, resx, resy, corners, warp=None):
    """LKRef over lowdof_ref.SSM, as alk_first_pass; warp: the 3 x 3 matrix of start_state(m) where the caller has one of its own (the
    device's, so that both sides sample at the same bits whatever cos / sin the two maths libraries return)"""
    out = dict(start=start_state(m), recs={}, J0={})
    for label, p in variants(m):
        r = LR.SSM(m.ssm, resx, resy)
        o_am = oracle.AM(m.am, resx, resy)
        o_am.set_curr_img(frame)
        ref = LR.LKRef(m.sm, o_am, r, max_iters=1, leven_marq=0, **p)
        ref.initialize(corners)
        out["init_pts"] = r.init_pts.copy()
        out["init_pts_hm"] = np.vstack([r.init_pts, np.ones(r.n)])
        out["I0"] = o_am.get("I0").copy()
        out["J0"][label] = np.array(ref.J0)
        o_am.set_curr_img(frame2)
        r.set_warp(r.warp_from_state(out["start"]) if warp is None else warp)
        out["warp"] = r.warp.copy()
        out["curr_pts"] = r.curr_pts.copy()
        out["recs"][label] = ref.update()["log"][0]
    return out


def first_pass(oracle, frame, frame2, m, resx, resy, corners, warp=None, alt=False):
    if m.family == ALK:
        return alk_first_pass(oracle, frame, frame2, m, resx, resy, corners, alt)
    return low_first_pass(oracle, frame, frame2, m, resx, resy, corners, warp)


_REF = {}


def region_reference(oracle, frame, frame2, m, resx, resy, region, warp=None, alt=False):
    """first_pass of a model at a shape on a named region, cached"""
    key = (model_name(m), resx, resy, region, None if warp is None else np.asarray(warp, dtype=np.float64).tobytes(), bool(alt))
    if key not in _REF:
        if warp is not None and m.family == LOW:
            plain = region_reference(oracle, frame, frame2, m, resx, resy, region)
            if np.array_equal(plain["warp"], np.asarray(warp).reshape(3, 3)):
                _REF[key] = plain
                return plain
        _REF[key] = _freeze(first_pass(oracle, frame, frame2, m, resx, resy, REGIONS[region], warp, alt))
    return _REF[key]


def reference(oracle, frame, frame2, cid, warp=None):
    """first_pass of a case of the table, cached"""
    c = BY_ID[cid]
    return region_reference(oracle, frame, frame2, c.model, c.resx, c.resy, c.region, warp, c.alt_start)


# ---------------------------------------------------------------- the device loop (Part C of the GPU test)
LOOP = dict(max_iters=12, epsilon=1e-5)
LOOP_SHAPES = [(5, 7), (16, 17), (32, 33), (37, 23)] + BIG_SHAPES
LOOP_MODELS = ([Model(ALK, sm, HOM, am, dict(hess_type=ht)) for sm in (FALK, IALK) for am in (SSD, NCC) for ht in (0, 1)] +
               [Model(LOW, sm, ssm, am, dict(hess_type=LC.default_hess(sm))) for ssm in (TRANS, ISO, SIM) for am in (SSD, NCC)
                for sm in (ESM, FCLK, ICLK)] +
               # Levenberg-Marquardt, one per family
               [Model(ALK, FALK, HOM, SSD, dict(hess_type=1, leven_marq=1)), Model(LOW, ESM, SIM, SSD, dict(hess_type=2, leven_marq=1))])
LOOP_REGION_SETS = [("quad",), ("inside", "quad", "right")]
LOOP_OUTSIDE_SET = ("inside", "outside")
CORNER_REGIONS = ("inside", "quad")     # where the final corners are compared, if the reference converged


def loop_params(m):
    p = dict(leven_marq=0)
    p.update(m.extra)
    p.update(LOOP)
    return p


_RUN = {}


def full_run(oracle, frame, frame2, m, resx, resy, region):
    """the reference's whole update() from the identity: dict(n_iters, corners (8,), state, log), cached"""
    key = (model_name(m), resx, resy, region)
    if key not in _RUN:
        if m.family == ALK:
            _, res = alk_ref.track(oracle, m.sm, m.am, m.ssm, resx, resy, frame, frame2, REGIONS[region], **loop_params(m))
        else:
            _, res = LR.track(oracle, m.sm, m.am, LR.SSM(m.ssm, resx, resy), frame, frame2, REGIONS[region], **loop_params(m))
        _RUN[key] = _freeze(res)
    return _RUN[key]


def converged(run):
    """the reference stopped by epsilon, not by max_iters"""
    last = run["log"][-1]
    return (not last["undo"]) and last["update_norm"] < LOOP["epsilon"]



def corners_compared(m):
    """(g) of tests/test_alk_lowdof_seams_cpu.py: undamped Gauss-Newton with the InitialSelf Hessian of an additive method on the
    homography runs into max_iters on every shape and region of the loop table (a loop that does not contract keeps no fixed distance
    between two trajectories that start 1e-13 px apart, tests/test_gpu_alk.py::test_device_loop_follows_reference_ssd); every other loop
    model's reference stops by epsilon everywhere, and there the device's final corners are compared"""
    return not (m.family == ALK and m.extra.get("hess_type") == 0 and not m.extra.get("leven_marq"))
