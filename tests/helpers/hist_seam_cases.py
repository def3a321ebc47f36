"""The cases tests/test_hist_seams_cpu.py (the references alone) and tests/test_gpu_hist_seams.py (the device against them) share: the
histogram appearance models -- MI (the materialising passes of kernels_mi.hip and the recompute passes k_mi_pass_hist / k_mi_pass_grad_hess of
kernels_mi_fused.hip) and CCRE (kernels_ccre.hip) -- at the pixel counts, bin counts and frame positions where their decompositions have a
seam.  Importable without a GPU.

The table is not a cross product.  A (shape, region, bins) triple is a `pair`; an MI pair takes every STEP-th row of
tests/test_gpu_parity.py::MI_CASES (every MiPlan Hessian kind and gradient mode, chained and not), shifted by the pair's index, on the SSM the
sum of the two indices picks -- so every row meets every region, on both SSMs.  A CCRE case is a pair alone: the reference is evaluated on the
arrays the device sampled, one evaluation serves every served (search method, jac_type, hess_type), and the device test runs them all.

References.  MI: the C++ oracle (first_pass: one update() from the identity on the second frame).  At FCLK numpy_mi restates
tests/golden/make_golden5.py::mi_case for two frames and the identity -- an independent float64 second reference.  CCRE: the oracle has none;
tests/golden/make_golden12.py::quantities on a tests/golden/make_golden10.py::Patch here, on the device's own samples there.

Reference results are computed once per process and cached; nobody modifies them."""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.join(TESTS, "golden"))
sys.path.insert(0, os.path.join(os.path.dirname(TESTS), "oracle"))

from mtf_amd import _lib as L  # noqa: E402
from mtf_amd import synth  # noqa: E402
import make_golden5 as G5  # noqa: E402
import make_golden12 as G12  # noqa: E402
import numpy_ref as R  # noqa: E402
import test_gpu_ccre as TC  # noqa: E402  (SERVED, FIXTURE_METHODS, the bounds, ref_g_H)
import test_gpu_parity as TP  # noqa: E402  (MI_CASES, FOLLOW_BOUNDS)

G10 = G12.G10
ESM, FCLK, ICLK = L.SM_ESM, L.SM_FCLK, L.SM_ICLK
HOM, AFF = L.SSM_HOMOGRAPHY, L.SSM_AFFINE
MI, CCRE = L.AM_MI, L.AM_CCRE
PRE_SEED = 10.0
FRAME2_SEED = 20261021
JITTER_SEED = 0

# ---------------------------------------------------------------- the frames
_FRAMES = {}


def frames():
    """make_golden5.make_image() (256 x 256: a block at exactly 0, one at exactly 255, a ramp of two or three classes, texture) and the next
    frame: the same image seen through a seeded small homography about its centre"""
    if not _FRAMES:
        img = G5.make_image()
        p_true = synth.random_small_homography(np.random.default_rng(FRAME2_SEED)) * 0.5
        img2 = synth.warp_frame(img, p_true, (128.0, 128.0)).astype(np.float32)
        img.setflags(write=False); img2.setflags(write=False)
        _FRAMES["f"] = (img, img2)
    return _FRAMES["f"]


def frames_mc():
    """three channels: the frame, its transpose and its vertical flip (every channel keeps the exact blocks), and the same next-frame warp"""
    if "mc" not in _FRAMES:
        img, _ = frames()
        img3 = np.ascontiguousarray(np.stack([img, img.T, img[::-1]], axis=2))
        p_true = synth.random_small_homography(np.random.default_rng(FRAME2_SEED)) * 0.5
        img3b = synth.warp_frame(img3, p_true, (128.0, 128.0)).astype(np.float32)
        _FRAMES["mc"] = (img3, img3b)
    return _FRAMES["mc"]


# ---------------------------------------------------------------- regions (the frame is 256 x 256; the zero block is rows 20..61, columns 20..57)
REGIONS = collections.OrderedDict([
    ("inside", synth.square_corners(128.3, 190.7, 40)),                   # texture
    ("h50a", synth.square_corners(64, 64, 70)),                           # make_golden12's h50a: pixels at exactly 0 and exactly 255
    ("right", synth.square_corners(245.7, 180.4, 60)),
    ("bottom", synth.square_corners(100.3, 248.4, 50)),
    ("top", synth.square_corners(100.3, 1.7, 40)),
    ("outside", synth.square_corners(-300, -300, 60)),
    ("flat0", G5._rect(26, 27, 50, 54)),                                  # wholly inside the exact-zero block, six pixels from its edges
])
HALF_OUTSIDE = ("right", "bottom", "top")
FLAT = ("outside", "flat0")
EDGE_REGIONS = HALF_OUTSIDE + FLAT
# four distinct in-frame texture regions the targets of a large batch cycle through
CYCLE = [synth.square_corners(128.3, 190.7, 40), synth.square_corners(60.6, 200.2, 44), synth.square_corners(190.4, 170.9, 36),
         synth.square_corners(140.8, 215.3, 42)]

# (resx, resy).  4: fewer pixels than parameters; 63, 64, 65: one wave +- 1; 255, 256, 258: one workgroup, then a second wave-chunk with two
# pixels; 1023, 1024, 1025: simple_blocks_per_target 1 -> 2, the second workgroup holds one pixel in one wave and three empty waves; 2048,
# 2050: 2 -> 3; 851 both ways: resx != resy
PIXEL_SHAPES = [(2, 2), (7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (6, 43), (33, 31), (32, 32), (25, 41), (32, 64), (41, 50), (37, 23),
                (23, 37)]
EDGE_SHAPES = [(5, 7), (32, 33), (37, 23)]
CAP_SHAPE = (257, 256)            # 65 792 px: 65 block rows, past the 64 of ccre_grad_blocks / mi_grad_blocks -- k_ccre_grad_gemv and k_mi_grad_gemv stride
BIN_SHAPE = (50, 50)
BINS_DENSE = [2, 3, 9, 11, 12, 13, 14, 15, 16]          # CCRE and the materialising MI passes; kMiPairs' pairs per lane step at 8|9, 11|12, 13|14
BINS_RECOMPUTE = [(2, 0), (3, 0), (4, 0), (6, 0), (7, 0), (4, 1), (6, 1), (7, 1)]      # (bins, pou): what the suite does not have yet

# ---------------------------------------------------------------- models
MI_ROWS = [(sm, dict(extra)) for sm, _, _, extra in TP.MI_CASES]
assert len(MI_ROWS) == 13
# the rows mi_fast_ok admits at other than 8 bins: the constant and the self Hessian (tests/test_gpu_parity.py::test_fused_mi_other_bin_counts)
RECOMPUTE_ROWS = [0, 1, 2, 3, 4, 5, 9, 12]
CCRE_METHODS = list(TC.SERVED)
assert {m[1:] for m in TC.FIXTURE_METHODS} <= set(CCRE_METHODS)

Case = collections.namedtuple("Case", "id group am resx resy region nb pou ssm sm extra row")


def sm_name(sm):
    return {ESM: "ESM", FCLK: "FCLK", ICLK: "ICLK"}[sm]


def row_name(row):
    sm, extra = MI_ROWS[row]
    return sm_name(sm) + "".join("-%s%s" % kv for kv in sorted(extra.items()))


def _cfg_name(am, nb, pou):
    return "%s%d%s" % ("mi" if am == MI else "ccre", nb, "p" if pou else "")


def _build_cases():
    out = []
    pair, n_ccre = [0], [0]

    def mi_pair(group, shape, region, nb, pou, rows, step, ssm_rule=None):
        ci = pair[0]; pair[0] += 1
        for k, row in enumerate(rows):
            if (ci + k) % step:
                continue
            ssm = ssm_rule if ssm_rule is not None else (HOM, AFF)[(ci + k // step) % 2]
            sm, extra = MI_ROWS[row]
            out.append(Case("%s-%dx%d-%s-%s-%s-%s" % (group, shape[0], shape[1], region, _cfg_name(MI, nb, pou), row_name(row), ("hom", "aff")[ssm]),
                            group, MI, shape[0], shape[1], region, nb, pou, ssm, sm, extra, row))

    def ccre_pair(group, shape, region, nb, pou, ssm_rule=None):
        ci = n_ccre[0]; n_ccre[0] += 1                  # (its own counter: SSM by its parity, chained or not by the next bit)
        ssm = ssm_rule if ssm_rule is not None else (HOM, AFF)[ci % 2]
        chained = (ci // 2 + 1) % 2
        out.append(Case("%s-%dx%d-%s-%s-%s-chained%d" % (group, shape[0], shape[1], region, _cfg_name(CCRE, nb, pou), ("hom", "aff")[ssm], chained),
                        group, CCRE, shape[0], shape[1], region, nb, pou, ssm, None, dict(chained_warp=chained), None))

    all_rows = list(range(13))
    # 1. pixel count, on `inside`; below 400 pixels the affine SSM (too few pixels for a conditioned 8-parameter solve)
    for shape in PIXEL_SHAPES:
        small = AFF if shape[0] * shape[1] < 400 else None
        mi_pair("px", shape, "inside", 8, 0, all_rows, 6, small)
        mi_pair("px", shape, "inside", 10, 1, all_rows, 6, small)
        ccre_pair("px", shape, "inside", 8, 0, small)
    # the cap case, one iterate each
    out.append(Case("cap-257x256-inside-mi8-FCLK-hom", "cap", MI, CAP_SHAPE[0], CAP_SHAPE[1], "inside", 8, 0, HOM, FCLK, dict(), 3))
    out.append(Case("cap-257x256-inside-ccre8-hom-chained1", "cap", CCRE, CAP_SHAPE[0], CAP_SHAPE[1], "inside", 8, 0, HOM, None, dict(chained_warp=1), None))
    # 2. bin count, 50 x 50 on h50a's region
    for nb in BINS_DENSE:
        ccre_pair("bins", BIN_SHAPE, "h50a", nb, 0)
        mi_pair("bins", BIN_SHAPE, "h50a", nb, 0, all_rows, 6)
    for nb, pou in BINS_RECOMPUTE:
        mi_pair("bins_rc", BIN_SHAPE, "h50a", nb, pou, RECOMPUTE_ROWS, 4)
    # 3. frame edge
    for region in EDGE_REGIONS:
        for shape in EDGE_SHAPES:
            mi_pair("edge", shape, region, 8, 0, all_rows, 6)
            mi_pair("edge", shape, region, 10, 1, all_rows, 6)
            ccre_pair("edge", shape, region, 8, 0)
            ccre_pair("edge", shape, region, 16, 0)
    return out


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
MI_IDS = [c.id for c in CASES if c.am == MI]
CCRE_IDS = [c.id for c in CASES if c.am == CCRE]

# 6. three channels (MI only): NP sample points -> 3 NP (pixel, channel) rows = 63, 66, 255, 258: a 64-row chunk ends inside a pixel
MC_SHAPES = [(3, 7), (2, 11), (5, 17), (2, 43)]
# 5. candidates: N = 63, 65, 1025
CAND_SHAPES = [(7, 9), (5, 13), (25, 41)]
N_CAND = 37


def n_pix(c):
    return c.resx * c.resy


def am_kw(c):
    """the device's keyword arguments of a case's appearance model"""
    kw = dict(mi_n_bins=c.nb, mi_pou=c.pou)
    if c.am == CCRE:
        kw["mi_pre_seed"] = PRE_SEED
    return kw


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = np.linalg.norm(b)
    d = np.linalg.norm(a - b)
    return float(d / n) if n > 0 else float(d)


def g_scale(rec):
    """the scale g is held against where it cancels (tests/test_gpu_parity.py::_fused_follow, for MI: sqrt |tr H|)"""
    return float(np.sqrt(abs(np.trace(rec["H"]))))


def g_err(g, rec):
    return float(np.linalg.norm(g - rec["g"]) / max(np.linalg.norm(rec["g"]), g_scale(rec), 1e-300))


# ---------------------------------------------------------------- MI: the oracle
def first_pass(oracle, frame, frame2, sm, ssm, extra, resx, resy, corners, am_kw=None, channels=1, with_arrays=True, **override):
    """the oracle's MI tracker initialised on `frame` inside `corners`, one update() on `frame2` from the identity: the first trace record and
    (with_arrays) the per-pixel arrays of that one iteration.  am_kw: the oracle's own names (n_bins, pou, grad_eps, pre_seed)"""
    o_ssm = oracle.SSM(ssm, resx, resy)
    o_am = oracle.AM(MI, resx, resy, **(am_kw or {}))
    if channels != 1:
        o_am.set_channels(channels); o_ssm.set_channels(channels)
    o_am.set_curr_img(frame)
    params = dict(leven_marq=0, max_iters=1, epsilon=-1.0)
    params.update(extra)
    params.update(override)
    trk = oracle.Tracker(sm, o_am, o_ssm, **params)
    trk.initialize(corners)
    out = {}
    if with_arrays:
        out["init_pts"] = o_ssm.get("init_pts").copy()
        out["init_pts_hm"] = o_ssm.get("init_pts_hm").copy()
        out["I0"] = o_am.get("I0").copy()
    o_am.set_curr_img(frame2)
    trk.update()
    out["rec"] = trk.trace()[0]
    if with_arrays:
        out["It"] = o_am.get("It").copy()
        out["dIt_dx"] = o_am.get("dIt_dx").copy()
    return out


def _freeze(r):
    for v in list(r.values()) + [x for v in r.values() if isinstance(v, dict) for x in v.values()]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


_REF = {}


def mi_reference(oracle, sm, ssm, extra, resx, resy, corners, nb, pou, channels=1, jitter=False):
    """first_pass on the suite's frames, cached; jitter: the corners moved by the seeded +-1e-12 px of tests/test_lk_seams_cpu.py (e)"""
    key = (sm, ssm, tuple(sorted(extra.items())), resx, resy, corners.tobytes(), nb, pou, channels, jitter)
    if key not in _REF:
        f1, f2 = frames() if channels == 1 else frames_mc()
        if jitter:
            corners = corners + np.random.default_rng(JITTER_SEED).choice([-1e-12, 1e-12], size=(2, 4))
        _REF[key] = _freeze(first_pass(oracle, f1, f2, sm, ssm, extra, resx, resy, corners, am_kw=dict(n_bins=nb, pou=pou), channels=channels,
                                       with_arrays=not jitter))
    return _REF[key]


def reference(oracle, cid):
    c = BY_ID[cid]
    return mi_reference(oracle, c.sm, c.ssm, c.extra, c.resx, c.resy, REGIONS[c.region], c.nb, c.pou)


def mi_floor(oracle, sm, ssm, extra, resx, resy, corners, nb, pou, channels=1):
    """the reference's own floor: how far the oracle's f, H, g and dp move under the seeded +-1e-12 px corner jitter"""
    a = mi_reference(oracle, sm, ssm, extra, resx, resy, corners, nb, pou, channels)["rec"]
    b = mi_reference(oracle, sm, ssm, extra, resx, resy, corners, nb, pou, channels, jitter=True)["rec"]
    return dict(f=rel(b["f"], a["f"]), H=rel(b["H"], a["H"]), g=g_err(b["g"], a), dp=rel(b["dp"], a["dp"]))


def case_floor(oracle, cid):
    c = BY_ID[cid]
    return mi_floor(oracle, c.sm, c.ssm, c.extra, c.resx, c.resy, REGIONS[c.region], c.nb, c.pou)


_RUN = {}
MAX_ITERS = 8
EPS_CANDIDATES = (1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5)


def mi_trace(oracle, sm, ssm, extra, resx, resy, corners, nb, pou):
    """the oracle's update() of MAX_ITERS iterations without a convergence test: the squared corner change and the corners after each; cached.
    The loop with a test at any epsilon is a prefix of it (stop_at)."""
    key = (sm, ssm, tuple(sorted(extra.items())), resx, resy, corners.tobytes(), nb, pou)
    if key not in _RUN:
        f1, f2 = frames()
        o_ssm = oracle.SSM(ssm, resx, resy)
        o_am = oracle.AM(MI, resx, resy, n_bins=nb, pou=pou)
        o_am.set_curr_img(f1)
        params = dict(leven_marq=0, max_iters=MAX_ITERS, epsilon=-1.0)
        params.update(extra)
        trk = oracle.Tracker(sm, o_am, o_ssm, **params)
        trk.initialize(corners)
        o_am.set_curr_img(f2)
        trk.update()
        cs = [corners] + [t["corners"].copy() for t in trk.trace()]
        _RUN[key] = dict(changes=[float(((cs[i + 1] - cs[i]) ** 2).sum()) for i in range(len(cs) - 1)], corners=cs[1:])
    return _RUN[key]


def stop_at(changes, eps):
    """iterations of the loop with the corner-change test at eps"""
    for k, ch in enumerate(changes):
        if ch < eps:
            return k + 1
    return len(changes)


def pick_eps(runs):
    """the candidate epsilon no corner change of the runs (up to where each stops) comes close to: (eps, margin), margin a ratio >= 1"""
    best = None
    for eps in EPS_CANDIDATES:
        margin = min(G10.eps_margin(r["changes"][:stop_at(r["changes"], eps)], eps) for r in runs)
        if best is None or margin > best[1]:
            best = (eps, margin)
    return best


# ---------------------------------------------------------------- MI: the NumPy second reference (FCLK)
def numpy_mi(nb, pou, resx, resy, affine, corners):
    """make_golden5.mi_case for two frames and the identity warp, through numpy_ref's functions directly (mi_case's finite-difference
    self-check divides by max |Jt|, which is zero on a flat region): f, g_curr, H_curr, H_init, H_init0, H_self1"""
    f1, f2 = (v.astype(np.float64) for v in frames())
    mult, add = R.mi_pix_norm(nb, pou)
    init_pts, init_hm = R.grid_from_corners(corners, resx, resy, affine=affine)
    x, y = init_pts
    I0n = mult * R.bilinear(f1, x, y) + add
    Itn = mult * R.bilinear(f2, x, y) + add
    g0, gt = R.img_grad(f1, init_pts, mult=mult), R.img_grad(f2, init_pts, mult=mult)
    if affine:
        P = R.aff_param_jacobian(x, y)
        J0 = R.sd_rows_direct(g0, P)
        Jt = R.sd_rows_chained(gt, np.broadcast_to(np.eye(2), (x.size, 2, 2)), P)
    else:
        Pj = R.hom_param_jacobian(x, y)
        sj = R.hom_spatial_jacobian(np.eye(3), init_pts, init_hm[2])
        J0, Jt = R.sd_rows_chained(g0, sj, Pj), R.sd_rows_chained(gt, sj, Pj)
    S = Jt.shape[1]
    dft = R.mi_curr_grad(I0n, Itn, nb)
    return dict(I0n=I0n, Itn=Itn, f=R.mi_similarity(I0n, Itn, nb), g=dft @ Jt, Jt=Jt, J0=J0,
                H_curr=R.mi_curr_hessian(I0n, Itn, Jt, nb), H_init=R.mi_init_hessian(I0n, Itn, J0, nb),
                H_init0=R.mi_init_hessian(I0n, I0n, J0, nb), H_self1=R.mi_self_hessian2(Itn, Jt, np.zeros((x.size, S, S)), nb))


# ---------------------------------------------------------------- CCRE: the generator on a Patch (CPU) / on the device's samples (GPU)
_PATCH = {}


def ccre_arrays(resx, resy, affine, corners, nb, pou):
    """I0, It, J0, Jt (normalised) of one pass from the identity on the second frame, sampled as make_golden10.Patch samples"""
    key = (resx, resy, affine, corners.tobytes(), nb, pou)
    if key not in _PATCH:
        f1, f2 = (v.astype(np.float64) for v in frames())
        mult, add = G12.pix_norm(nb, pou)
        p1, p2 = G10.Patch(f1, resx, resy, affine, corners), G10.Patch(f2, resx, resy, affine, corners)
        # (the identity warp samples the second frame at the template's own points: Patch's template quantities of that frame)
        _PATCH[key] = _freeze(dict(I0=mult * p1.I0o + add, It=mult * p2.I0o + add, J0=mult * p1.J0, Jt=mult * p2.J0, pts=p1.init_pts))
    return _PATCH[key]


def ccre_quantities(a, nb, dtype=np.float64):
    """(q, q0): the pass and the template's own (It = I0), as tests/test_gpu_ccre.py::device_reference"""
    return (G12.quantities(a["I0"], a["It"], a["J0"], a["Jt"], nb, PRE_SEED, dtype),
            G12.quantities(a["I0"], a["I0"], a["J0"], a["J0"], nb, PRE_SEED, dtype))


def ccre_floors(a, nb):
    """float64 against long double on the same arrays, per method: {(sm, jac, ht): dict(f, g, H)}, relative to the largest entry"""
    q, q0 = ccre_quantities(a, nb)
    ql, q0l = ccre_quantities(a, nb, np.longdouble)
    out = {}
    for sm, jac, ht in CCRE_METHODS:
        g, H = TC.ref_g_H(q, q0["H_self"], sm, jac, ht)
        gl, Hl = TC.ref_g_H(ql, q0l["H_self"], sm, jac, ht)
        out[(sm, jac, ht)] = dict(f=_floor(q["f"], ql["f"]), g=_floor(g, gl), H=_floor(H, Hl))
    return out


def _floor(x64, xld):
    xld = np.asarray(xld, dtype=np.longdouble)
    top = np.abs(xld).max()
    return float(np.abs(np.asarray(x64, dtype=np.longdouble) - xld).max() / top) if top > 0 else 0.0


def widened(base, floor):
    """max(project bound, 16 x the reference's own floor): tests/test_gpu_ccre.py::floor16's factor"""
    return max(base, 16.0 * floor)


# ---------------------------------------------------------------- Part B: the device loop
LOOP_SHAPES = [(32, 33), (37, 23)]
LOOP_REGIONS = ("inside", "right", "flat0")
BATCH3_SHAPE = (32, 33)
BATCH3 = ("inside", "right", "flat0")      # one region past the right edge; the flat one stops after its first pass (H = 0, g = 0: no update)
# MI: (sm, extra, bins, pou) per loop; the recompute passes serve both (the self and the constant Hessian)
MI_LOOP_MODELS = [(ESM, dict(), 10, 1), (ICLK, dict(), 8, 0)]
CCRE_LOOP_KEYS = ("esm_ds", "fclk_cs")
CCRE_LOOP_BINS = 16
CCRE_BATCH_KEY = "fclk_cs"           # (the method whose reference loop pins more than one iteration on every region of the batch)
CCRE_BATCH_EPS = 1e-12          # a test only the flat target's zero update passes


class TwoFramePatch(G10.Patch):
    """make_golden10.Patch with the template taken on one frame and every later sample on the next"""

    def __init__(self, f1, f2, resx, resy, affine, corners):
        super().__init__(f1, resx, resy, affine, corners)
        self.img = f2


_CCRE_LOOP = {}


def _ccre_run(pa, mult, add, nb, H0, corners, key, shift):
    flat = not pa.J0.any()
    if flat:        # H = 0 and g = 0: the rank-revealing solve of a zero system is zero (asserted on the oracle's solver), no update
        return [(False, 0.0, np.eye(3), k + 1) for k in range(G12.N_ITERS)]
    return G12.run_loop(pa, mult, add, np.eye(3), nb, PRE_SEED, H0, False, corners, key, False, first_dp_shift=shift)


def ccre_loop(resx, resy, region, nb, key):
    """make_golden12's loop of one method from the identity on the second frame, kept as make_golden12 keeps a run that does not contract: up
    to the last iteration at which the same loop with its first update shifted by STATE_SHIFT stays within SHIFT_PX of it (as far as the run
    pins a second implementation), without a convergence test.  dict(iters, corners)"""
    k_ = (resx, resy, region, nb, key)
    if k_ not in _CCRE_LOOP:
        f1, f2 = (v.astype(np.float64) for v in frames())
        corners = REGIONS[region]
        pa = TwoFramePatch(f1, f2, resx, resy, False, corners)
        mult, add = G12.pix_norm(nb, 0)
        I0, J0 = mult * pa.I0o + add, mult * pa.J0
        H0 = G12.quantities(I0, I0, J0, J0, nb, PRE_SEED)["H_self"]
        r, r2 = _ccre_run(pa, mult, add, nb, H0, corners, key, 0.0), _ccre_run(pa, mult, add, nb, H0, corners, key, G12.STATE_SHIFT)
        chm = np.vstack([corners, np.ones(4)])
        iters = 0
        for k in range(min(len(r), len(r2))):
            if not (np.abs(G10.corners_of(r[k][2], chm) - G10.corners_of(r2[k][2], chm)).max() < G12.SHIFT_PX and
                    np.abs(G10.state_of(r[k][2], False) - G10.state_of(r2[k][2], False)).max() < G12.SHIFT_PX):
                break
            iters = k + 1
        _CCRE_LOOP[k_] = dict(iters=iters, corners=[G10.corners_of(r[k][2], chm) for k in range(iters)])
    return _CCRE_LOOP[k_]
