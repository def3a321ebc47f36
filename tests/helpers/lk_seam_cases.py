"""The cases tests/test_lk_seams_cpu.py (the reference alone) and tests/test_gpu_lk_seams.py (the device against it) share: the compositional
LK methods ESM / FCLK / ICLK, first and second order (sec_ord_hess), at the pixel counts where the kernels' decompositions have a seam and on
regions that are projective, cross a frame edge or lie outside the frame.  Importable without a GPU.

The table is not the cross product (13 shapes x 6 regions x 34 models): every shape runs on `inside`, every region runs on FULL_SHAPES, and
each of those 28 (shape, region) pairs takes every third model, shifted by the pair's index -- so every model meets every region (the three
FULL_SHAPES of one region fall in the three residues) and four or five of the thirteen shapes.

Reference results are computed once per process and cached; nobody modifies them."""
import collections

import numpy as np

from mtf_amd import synth

ESM, FCLK, ICLK = 0, 1, 2
SSD, NCC, MI = 0, 1, 2
HOM, AFF = 0, 1

# (resx, resy): N = 4, 6: fewer pixels than parameters; 35: below a wave; 63, 64, 65: around one wave; 256, 272: one workgroup (+ 16);
# 1023, 1024: just under / exactly the pixels of one workgroup of the simple decomposition (ceil(N / 1024) workgroups of 256, stride
# nblk * 256); 1056: its second workgroup holds half a wave, and the fused kernel's decomposition goes to 5 rows; 851 both ways: resx != resy
SHAPES = [(2, 2), (2, 3), (5, 7), (7, 9), (8, 8), (5, 13), (16, 16), (16, 17), (33, 31), (32, 32), (32, 33), (37, 23), (23, 37)]
FULL_SHAPES = [(5, 7), (32, 33), (37, 23)]
MI_SHAPES = [(16, 17), (32, 33), (37, 23)]

_INSIDE = synth.square_corners(250.3, 244.7, 40)
REGIONS = collections.OrderedDict([
    ("inside", _INSIDE),
    # every corner moved by a seeded +-3 px: a projective region (the rectangle -> quad warp has W0[6], W0[7] != 0)
    ("quad", _INSIDE + np.random.default_rng(20261018).uniform(-3.0, 3.0, size=(2, 4))),
    ("right", synth.square_corners(501.7, 200.4, 60)),
    ("bottom", synth.square_corners(203.3, 504.4, 50)),
    ("top", synth.square_corners(200.3, 1.7, 40)),
    ("outside", synth.square_corners(-300, -300, 60)),
])
HALF_OUTSIDE = ("right", "bottom", "top")

# second order: every branch of SM_CASES / NCC_CASES in tests/test_gpu_parity.py; (sm, extra)
SECOND_ORDER = [
    (ESM, dict(hess_type=5)),                       # Std
    (ESM, dict(hess_type=4, chained_warp=0)),       # SumOfStd, non-chained
    (ESM, dict(hess_type=3, jac_type=0)),           # Original + Original: the mean pixel Hessian
    (FCLK, dict(hess_type=2)),
    (FCLK, dict(hess_type=2, chained_warp=0)),
    (ICLK, dict(hess_type=2)),
    (ICLK, dict(hess_type=2, chained_warp=0)),
]

Model = collections.namedtuple("Model", "sm ssm am extra")
Case = collections.namedtuple("Case", "id resx resy region model reference_nan")


def _models():
    out = []
    for am in (SSD, NCC):
        for ssm in (HOM, AFF):
            for sm, extra in SECOND_ORDER:
                out.append(Model(sm, ssm, am, dict(extra, sec_ord_hess=1)))
        for sm in (ESM, FCLK, ICLK):                # the class defaults, first order, on the homography
            out.append(Model(sm, HOM, am, dict()))
    return out


MODELS = _models()
MI_MODELS = [Model(sm, ssm, MI, dict(hess_type=ht, sec_ord_hess=1)) for sm, ht in ((ESM, 5), (ICLK, 2)) for ssm in (HOM, AFF)]
PAIRS = [(s, "inside") for s in SHAPES] + [(s, r) for r in list(REGIONS)[1:] for s in FULL_SHAPES]


def model_name(m):
    return "%s-%s-%s%s" % (("ESM", "FCLK", "ICLK")[m.sm], ("SSD", "NCC", "MI")[m.am], ("hom", "aff")[m.ssm],
                           "".join("-%s%s" % kv for kv in sorted(m.extra.items())))


def _build_cases():
    out = []
    for ci, ((resx, resy), region) in enumerate(PAIRS):
        for mi, m in enumerate(MODELS):
            if (ci + mi) % 3:
                continue
            out.append(Case("%dx%d-%s-%s" % (resx, resy, region, model_name(m)), resx, resy, region, m,
                            m.am == NCC and region == "outside"))
    for resx, resy in MI_SHAPES:
        for m in MI_MODELS:
            out.append(Case("%dx%d-inside-%s" % (resx, resy, model_name(m)), resx, resy, "inside", m, False))
    return out


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]


def second_order(c):
    return bool(c.model.extra.get("sec_ord_hess"))


def n_pix(c):
    return c.resx * c.resy


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = np.linalg.norm(b)
    d = np.linalg.norm(a - b)
    return float(d / n) if n > 0 else float(d)


def g_scale(rec, am):
    """the scale g is held against where it cancels (as tests/test_gpu_parity.py::_fused_follow): Cauchy-Schwarz ||J|| ||r|| for SSD"""
    return float(np.sqrt(abs(np.trace(rec["H"]))) * (np.sqrt(abs(2 * rec["f"])) if am == SSD else 1.0))


def first_pass(oracle, frame, frame2, model, resx, resy, corners, with_arrays=True, **override):
    """the oracle's tracker initialised on `frame` inside `corners`, one update() on `frame2` from the identity: the first trace record and
    (with_arrays) the per-pixel arrays of that one iteration"""
    o_ssm = oracle.SSM(model.ssm, resx, resy)
    o_am = oracle.AM(model.am, resx, resy)
    o_am.set_curr_img(frame)
    params = dict(leven_marq=0, max_iters=1, epsilon=-1.0)
    params.update(model.extra)
    params.update(override)
    trk = oracle.Tracker(model.sm, o_am, o_ssm, **params)
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
        out["dIt_dx"] = o_am.get("dIt_dx").reshape(2, -1).T.copy()
    return out


_REF = {}


def region_reference(oracle, frame, frame2, model, resx, resy, region):
    """first_pass of a model at a shape on a named region, cached"""
    key = (model_name(model), resx, resy, region)
    if key not in _REF:
        r = first_pass(oracle, frame, frame2, model, resx, resy, REGIONS[region])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def reference(oracle, frame, frame2, cid):
    """first_pass of a case of the table, cached"""
    c = BY_ID[cid]
    return region_reference(oracle, frame, frame2, c.model, c.resx, c.resy, c.region)


_RUN = {}


def full_run(oracle, frame, frame2, model, resx, resy, region, max_iters=12, epsilon=1e-5):
    """the oracle's whole update() (device-loop tests): trace, iteration count, final region; cached"""
    key = (model_name(model), resx, resy, region)
    if key not in _RUN:
        o_ssm = oracle.SSM(model.ssm, resx, resy)
        o_am = oracle.AM(model.am, resx, resy)
        o_am.set_curr_img(frame)
        params = dict(leven_marq=0, max_iters=max_iters, epsilon=epsilon)
        params.update(model.extra)
        trk = oracle.Tracker(model.sm, o_am, o_ssm, **params)
        trk.initialize(REGIONS[region])
        o_am.set_curr_img(frame2)
        iters = trk.update()
        _RUN[key] = dict(trace=trk.trace(), iters=iters, region=trk.get_region().copy(), max_iters=max_iters, epsilon=epsilon)
    return _RUN[key]


# ---------------------------------------------------------------- the image-Hessian point list (border and integer coordinates)
def hess_border_points(h, w, n=272):
    """x (and, transposed, y) at the coordinates where the constant-128 border rule, the last row / column and the dx == 0 rule of the
    bilinear sampler switch for a sample or for one of its +-1 / +-2 px stencil points, against an interior ordinate; a few exact-integer
    interior points; replicated to n.  (2, n)."""
    def edge(s):
        return [-3.0, -2.0, -1.0 - 1e-9, -1.0, -1e-9, 0.0, 0.5, 1.0, 2.0, 2.0 + 1e-8, s - 3.0, s - 2.0, s - 1.0, s - 1.0 + 1e-9, s - 0.5,
                float(s), s + 2.0]
    xs, ys = [], []
    for k, x in enumerate(edge(w)):
        xs.append(x); ys.append(37.25 + 11.0 * k)
    for k, y in enumerate(edge(h)):
        xs.append(41.75 + 9.0 * k); ys.append(y)
    for x, y in ((64.0, 64.0), (100.0, 37.25), (37.25, 100.0), (255.0, 256.0)):
        xs.append(x); ys.append(y)
    return np.stack([np.resize(np.array(xs), n), np.resize(np.array(ys), n)])


def dp_ulp_sensitivity(oracle, rec):
    """How far the reference's own update moves when every entry of its own H and g moves by one ulp (eight seeded sign patterns, the
    largest relative change of colpiv_qr_solve's dp): the least any other order of the same sums can do to it.  (The sums themselves move
    by more than one ulp under a reordering -- about sqrt(N) -- so this under-states the reference's order sensitivity and the bound built
    on it is the stricter one.)"""
    H, g = rec["H"], rec["g"]
    worst = 0.0
    for seed in range(8):
        rng = np.random.default_rng(seed)
        Hp = H * (1.0 + rng.choice([-1.0, 1.0], size=H.shape) * 2.0 ** -52)
        gp = g * (1.0 + rng.choice([-1.0, 1.0], size=g.shape) * 2.0 ** -52)
        worst = max(worst, rel(-oracle.colpiv_qr_solve(Hp, gp), rec["dp"]))
    return worst


def long_double_solve(A, b):
    """A x = b by Gaussian elimination with complete pivoting in numpy.longdouble (the extended-precision yardstick the device's and the
    reference's solves are both measured against); None where a pivot vanishes"""
    A = np.array(A, dtype=np.longdouble)
    x = np.array(b, dtype=np.longdouble)
    n = A.shape[0]
    perm = np.arange(n)
    for k in range(n):
        sub = np.abs(A[k:, k:])
        i, j = np.unravel_index(int(np.argmax(sub)), sub.shape)
        if sub[i, j] == 0:
            return None
        i += k; j += k
        A[[k, i]] = A[[i, k]]; x[[k, i]] = x[[i, k]]
        A[:, [k, j]] = A[:, [j, k]]; perm[[k, j]] = perm[[j, k]]
        for r in range(k + 1, n):
            m = A[r, k] / A[k, k]
            A[r, k:] -= m * A[k, k:]
            x[r] -= m * x[k]
    for k in range(n - 1, -1, -1):
        x[k] = (x[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    out = np.empty(n, dtype=np.longdouble)
    out[perm] = x
    return out
