"""The seams of the SCV family's pass-1 kernels (SCV, RSCV, LSCV, LRSCV), no GPU: one table of cases -- shared with
tests/test_gpu_scv_seams.py, which runs the device on the same inputs -- and, for every case,

(a) the two forms of each float64 restatement (tests/golden/make_golden6.py .. make_golden9.py) agree at the new shapes: the literal
    n_bins^2 joint histogram against the per-bin sums the device computes (exact for Dirac sums; Bilinear maps and the affine fits
    within the tolerances of tests/test_*_ref.py).  The two over-cap cases take the per-bin form only (`literal=False` in the table:
    131 406 and 262 656 pixels through a per-pixel Python loop);
(b) conditions on the inputs that the reference alone must meet, so that the device comparison is meaningful: every normalised sample
    of the template and of the current patch is exactly reproducible (the out-of-frame constant 128 mult, or exactly 0 from the flat
    zero block) or at least 1e-9 from every integer; every map has an empty bin (the map[b] = b rule) and a non-identity entry; the
    half-outside cases have at least 20 % of either kind of sample and a 64-pixel wave that holds both.

Two kinds of case cannot have a non-identity Dirac entry and are exempt from that one condition (`identity_ok`): at 2 bins every
admissible sample normalises into [0, 1), i.e. bin 0, and map[0] is a mean of zeros; wholly outside the frame every sample is
128 mult, so the only populated bin maps to itself.  Their Bilinear maps are not identities and are held to the condition.  At 2 bins
a Bilinear histogram has no empty bin either (every sample in (0, 1) weighs into both), so that case is exempt from the empty-bin one.

The image is make_golden7.py's (every non-zero texel moved by +0.29: no flat block normalises to a whole number)."""
import collections
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import make_golden5 as G5  # noqa: E402
import make_golden6 as G6  # noqa: E402
import make_golden7 as G7  # noqa: E402
import make_golden8 as G8  # noqa: E402
import make_golden9 as G9  # noqa: E402
import numpy_ref as R  # noqa: E402
from mtf_amd import synth  # noqa: E402

IMG = G7.make_image()
IMG64 = IMG.astype(np.float64)
MODELS = ("scv_d", "scv_b", "rscv", "lscv", "lrscv")
# kLscvLdsBudget - 64 (mtf_amd/csrc/mtfhip_internal.h; imap_geometry in api_imap.hip refuses 2 * sizeof(unsigned) * cells * n_bins above it).  A
# copy: if the constant changes, the GPU test's accepted / refused pair stops matching the device and fails
LDS_HIST_BUDGET = 64 * 1024 - 64

# geo: (n_x, n_y, spacing_x, spacing_y); mapping: 0 nearest, 1 linear, 2 affine (LSCV / LRSCV; SCV Bilinear uses `linear`, SCV Dirac and
# RSCV nearest unless `linear`); track: a 5-iteration track is checked; literal: the literal form is evaluated on the CPU
Case = collections.namedtuple("Case", "id group resx resy nb affine corners p models geo mapping linear track literal identity_ok edge")


def _rect(x0, y0, w, h):
    return G5._rect(x0, y0, x0 + w, y0 + h)


def _state(rng, affine, scale=1.0):
    if affine:
        return rng.uniform(-1, 1, 6) * np.array([1.2, 1.2, 0.02, 0.02, 0.02, 0.02]) * scale
    return synth.random_small_homography(rng, 0.4 * scale)


def _build_cases():
    rng = np.random.default_rng(20261101)
    out = []

    def add(id, group, resx, resy, nb=64, affine=False, corners=None, models=MODELS, geo=(2, 2, 1, 1), mapping=0, linear=0, track=False,
            literal=True, identity_ok=False, edge=None, scale=1.0):
        out.append(Case(id, group, resx, resy, nb, affine, corners, _state(rng, affine, scale), tuple(models), geo, mapping, linear, track,
                        literal, identity_ok, edge))

    # pixel-count seams: 64 bins; below 400 pixels the affine SSM (too few pixels for a conditioned 8-parameter solve) and no track
    for resx, resy in ((3, 3), (7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (6, 43), (32, 64), (41, 50), (64, 64), (64, 65)):
        n = resx * resy
        add("px_%dx%d" % (resx, resy), "pixels", resx, resy, affine=n < 400, corners=_rect(30, 135, max(1.3 * resx, 14), max(1.3 * resy, 14)),
            track=n >= 2048, scale=0.5 if n >= 2048 else 1.0)
    # past the cap of 64 workgroups per target: one target, iterate only, the region inside the image
    add("cap_362x363", "cap", 362, 363, corners=_rect(8, 8, 238, 238), models=("scv_d", "scv_b", "rscv"), literal=False)
    add("cap_512x513", "cap", 512, 513, corners=_rect(8, 8, 238, 238), models=("lscv", "lrscv"), geo=(3, 3, 10, 10), literal=False)
    # bin-count seams at 50 x 50: the bin slots per lane of the Bilinear path (nk = 1 .. 4) and their edges.  The region is on the
    # texture, off the saturated blocks: across their edges the Bilinear maps are not conditioned against coordinate rounding
    # (test_bilinear_maps_are_conditioned_against_coordinate_rounding)
    for nb in (2, 63, 64, 65, 128, 129, 192, 193, 255, 256):
        add("bins_%d" % nb, "bins", 50, 50, nb=nb, corners=_rect(40, 160, 60, 60), geo=(3, 3, 10, 10), linear=nb % 2,
            identity_ok=nb == 2)
    # the frame edge (the image is 256 x 256): half across the right edge, half across the bottom edge, wholly outside
    for resx, resy in ((30, 30), (37, 23)):
        for edge, c in (("right", _rect(226, 100, 60, 50)), ("bottom", _rect(90, 224, 70, 64)), ("outside", _rect(300, 290, 60, 50))):
            add("edge_%s_%dx%d" % (edge, resx, resy), "edge", resx, resy, corners=c, geo=(3, 3, 5, 5), identity_ok=edge == "outside", edge=edge)
    # sub-region decompositions (LSCV / LRSCV), each with nearest, linear and affine mapping
    for tag, resx, resy, geo in (("coincide", 21, 21, (3, 3, 0, 0)), ("one_px", 21, 21, (3, 3, 10, 10)), ("touch", 30, 30, (3, 3, 10, 10)),
                                 ("1x4", 41, 23, (1, 4, 10, 5)), ("4x1", 41, 23, (4, 1, 10, 5))):
        for mapping in (0, 1, 2):
            add("geo_%s_m%d" % (tag, mapping), "geo", resx, resy, corners=_rect(40, 140, 1.5 * resx, 1.5 * resy), models=("lscv", "lrscv"), geo=geo,
                mapping=mapping)
    return out


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}
PAIRS = [(c.id, m) for c in CASES for m in c.models]


def geo6(c):
    return (c.resx, c.resy) + tuple(c.geo)


@functools.lru_cache(maxsize=None)
def patch(cid):
    c = BY_ID[cid]
    return G6.Patch(IMG64, c.nb, c.resx, c.resy, c.affine, c.corners)


@functools.lru_cache(maxsize=None)
def sampled(cid):
    pa = patch(cid)
    return pa.sample(pa.warp(BY_ID[cid].p))


@functools.lru_cache(maxsize=None)
def weights(cid):
    return G8.weights(*geo6(BY_ID[cid]))


def model_linear(c, model):
    return 1 if (model == "scv_b" or c.linear) else 0


def maps_of(c, model, It, I0o, literal=False):
    """(maps, aff) of one model: aff is None for SCV / RSCV"""
    if model in ("scv_d", "scv_b"):
        ht = 1 if model == "scv_b" else 0
        return (G6.literal_map if literal else G6.per_bin_map)(It, I0o, c.nb, ht), None
    if model == "rscv":
        return (G7.literal_map if literal else G7.per_bin_map)(It, I0o, c.nb), None
    if model == "lscv":
        return (G8.literal_maps if literal else G8.per_bin_maps)(It, I0o, c.nb, geo6(c))
    return (G9.literal_maps if literal else G9.per_bin_maps)(It, I0o, c.nb, geo6(c))


def mapped_pair(c, model, It, I0o, maps, aff, w):
    """(current patch, template) as the SSD behind the map sees them"""
    if model in ("scv_d", "scv_b"):
        return It, G6.remap(I0o, maps, model_linear(c, model))
    if model == "rscv":
        return G6.remap(It, maps, model_linear(c, model)), I0o
    if model == "lscv":
        return It, G8.blend(I0o, maps, aff, w, c.geo[0], c.geo[1], c.mapping == 2, c.mapping == 1)
    return G9.blend(It, maps, aff, w, c.geo[0], c.geo[1], c.mapping == 2, c.mapping == 1), I0o


def evaluate(c, model, pa, W, w=None, maps=None, aff=None):
    """one similarity update at the warp W: a dict of maps, aff, cur, tmpl, f, dft, g, H, Jt, It_orig; with `maps` given (once_per_frame
    after the first iteration) LSCV keeps its template and LRSCV runs on the raw patch"""
    It, Jt = pa.sample(W)
    if maps is None:
        maps, aff = maps_of(c, model, It, pa.I0o)
        cur, tmpl = mapped_pair(c, model, It, pa.I0o, maps, aff, w)
    elif model == "lscv":
        cur, tmpl = It, mapped_pair(c, model, It, pa.I0o, maps, aff, w)[1]
    else:
        cur, tmpl = It, pa.I0o
    r = cur - tmpl
    return dict(maps=maps, aff=aff, cur=cur, tmpl=tmpl, f=-0.5 * float(r @ r), dft=-r, g=(-r) @ Jt, H=-Jt.T @ Jt, Jt=Jt, It_orig=It)


@functools.lru_cache(maxsize=None)
def ref(cid, model):
    c = BY_ID[cid]
    pa = patch(cid)
    return evaluate(c, model, pa, pa.warp(c.p), weights(cid) if model in ("lscv", "lrscv") else None)


def solve_step(H, g):
    """the SSD Hessians are negated Gram matrices: a zero pivot (a flat or out-of-frame patch) leaves its unknown at zero"""
    if not np.any(H):
        return np.zeros_like(g)
    return -np.linalg.solve(H, g)


def lk_run(c, model, pa, p, method, max_iters, epsilon, once=0, w=None, corners=None):
    """chained ESM (DiffOfJacs + SumOfSelf) or FCLK (CurrentSelf) steps from the state p with the device loop's stopping rule: the sum
    of the squared corner displacements of a step below epsilon, or max_iters.  Returns the number of steps, the steps, the corners and
    the stopping margins |change - epsilon| / epsilon"""
    corners = c.corners if corners is None else corners
    chm = np.vstack([corners, np.ones(4)])
    W = pa.warp(p)
    kept = None
    dps, margins = [], []
    cr = G6.corners_of(W, chm) if not c.affine else (W @ chm)[:2]
    for it in range(max_iters):
        e = evaluate(c, model, pa, W, w, *(kept if (once and it > 0) else (None, None)))
        if once and it == 0:
            kept = (e["maps"], e["aff"])
        if method == "esm":
            g, H = 0.5 * (e["dft"] @ (pa.J0 + e["Jt"])), 0.5 * (e["H"] - pa.J0.T @ pa.J0)
        else:
            g, H = e["g"], e["H"]
        dp = solve_step(H, g)
        W = W @ R.aff_matrix(dp) if c.affine else R.compose_hom(W, dp)
        new = G6.corners_of(W, chm) if not c.affine else (W @ chm)[:2]
        change = float(((new - cr) ** 2).sum())
        cr = new
        dps.append(dp)
        if epsilon > 0:
            margins.append(abs(change - epsilon) / epsilon)
        if change < epsilon:
            break
    return len(dps), dps, cr, margins


@functools.lru_cache(maxsize=None)
def ref_track(cid, model, method):
    c = BY_ID[cid]
    return lk_run(c, model, patch(cid), c.p, method, 5, 0.0, w=weights(cid) if model in ("lscv", "lrscv") else None)


# --------------------------------------------------------------------------------------------------------------- batch seams
BATCH_RES = (12, 11)
BATCH_EPS = 0.1      # (the sum of the squared corner displacements of a step: about 0.16 px per corner)
BATCH_MAX_ITERS = 8


def batch_case(affine):
    return Case("batch_aff" if affine else "batch_hom", "batch", BATCH_RES[0], BATCH_RES[1], 64, affine, None, None, MODELS, (2, 2, 3, 3), 0, 0,
                False, True, False, None)


def batch_targets(affine, B):
    """B targets on distinct regions and states: k % 3 == 0 already at the solution, the others displaced by 1 to 3 px; the middle one
    (B >= 3) wholly outside the frame.  (corners, states, kinds)"""
    S = 6 if affine else 8
    cs, ps, kinds = [], [], []
    for k in range(B):
        rng = np.random.default_rng(7700 + k)
        if B >= 3 and k == B // 2:
            cs.append(_rect(300 + k, 280, 30, 28)); ps.append(np.zeros(S)); kinds.append("outside")
            continue
        cs.append(_rect(24 + 17 * (k % 6), 132 + 19 * (k // 6), 30, 28))
        p = np.zeros(S)
        if k % 3:
            d = (1.0 if k % 3 == 1 else 3.0) * rng.choice([-1.0, 1.0]) * np.ones(2) / np.sqrt(2.0)   # (1 px, 3 px, along the diagonal)
            p[[0, 1] if affine else [2, 5]] = d
        ps.append(p); kinds.append("moved" if k % 3 else "solved")
    return np.stack(cs), np.stack(ps), kinds


@functools.lru_cache(maxsize=None)
def batch_ref(affine, model, once, corners_key, p_key):
    c = batch_case(affine)
    corners, p = np.array(corners_key).reshape(2, 4), np.array(p_key)
    pa = G6.Patch(IMG64, 64, c.resx, c.resy, affine, corners)
    w = G8.weights(*geo6(c)) if model in ("lscv", "lrscv") else None
    return lk_run(c, model, pa, p, "esm", BATCH_MAX_ITERS, BATCH_EPS, once=once, w=w, corners=corners)


def batch_ref_iters(affine, model, once, B):
    cs, ps, _ = batch_targets(affine, B)
    runs = [batch_ref(affine, model, once, tuple(cs[k].ravel()), tuple(ps[k])) for k in range(B)]
    return np.array([r[0] for r in runs]), runs


# --------------------------------------------------------------------------------------------------------------- LDS budget
def lds_limit_counts(nb, res=130):
    """the largest n for which 1 x n sub-regions at spacing 1 on `res` rows fit the histogram LDS budget at nb bins, from
    make_golden8.cells: (n accepted, its cell count, the cell count of n + 1)"""
    n = 1
    while 8 * G8.cells(res, n + 1, 1)[2] * nb <= LDS_HIST_BUDGET:
        n += 1
    return n, G8.cells(res, n, 1)[2], G8.cells(res, n + 1, 1)[2]


def lds_case(nb, n):
    rng = np.random.default_rng(31 + nb)
    return Case("lds_%d_%d" % (nb, n), "lds", 8, 130, nb, False, _rect(40, 20, 24, 200), _state(rng, False, 0.5), ("lscv", "lrscv"), (1, n, 0, 1), 0, 0,
                False, True, False, None)


# --------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("cid,model", [(c, m) for c, m in PAIRS if BY_ID[c].literal])
def test_literal_equals_per_bin(cid, model):
    c = BY_ID[cid]
    It, _ = sampled(cid)
    I0o = patch(cid).I0o
    m_lit, a_lit = maps_of(c, model, It, I0o, literal=True)
    m_bin, a_bin = maps_of(c, model, It, I0o)
    if model == "scv_b":
        np.testing.assert_allclose(m_bin, m_lit, rtol=1e-12, atol=1e-12)
    else:
        np.testing.assert_array_equal(m_bin, m_lit)
    if a_lit is not None:
        np.testing.assert_allclose(a_bin, a_lit, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_samples_are_reproducible_or_off_the_integers(cid):
    c = BY_ID[cid]
    border = 128.0 * G6.pix_mult(c.nb)
    for v in (patch(cid).I0o, sampled(cid)[0]):
        ok = (v == border) | (v == 0.0) | (np.abs(v - np.rint(v)) >= 1e-9)
        assert ok.all(), (cid, v[~ok][:4])
        assert v.min() >= 0 and v.max() < c.nb - 1 + (c.nb == 256)


def warped_pts(pa, W):
    if pa.affine:
        x, y = pa.init_pts
        return (W @ np.vstack([x, y, np.ones_like(x)]))[:2]
    return R.warp_pts(W, pa.init_hm)[0]


def bilinear_map_coordinate_sensitivity(cid):
    """The largest change of the Bilinear SCV map, relative to the 1e-12 (1 + |map|) the device is held to, when every sample point of
    the template and / or of the current patch moves by one unit in the last place of its coordinates (the same way for all points:
    the nine combinations of -1, 0, +1 ulp in x and y, for either image).  Two correct float64 evaluations of the sample grid differ
    by that much, and across a step of the image -- the edge of a saturated block, 250 grey levels in one pixel -- a sample then
    moves by 1e-12: a bin whose sum rests on a weight of a few hundredths next to such a step is not pinned to 1e-12 by any
    restatement.  This is a condition on the inputs, like the distance from the integers."""
    c = BY_ID[cid]
    pa = patch(cid)
    pts0, pts1 = pa.init_pts, warped_pts(pa, pa.warp(c.p))
    shifts = [(sx, sy) for sx in (-1, 0, 1) for sy in (-1, 0, 1)]

    def samples(pts):
        x, y = pts
        return [pa.mult * R.bilinear(IMG64, x + sx * np.spacing(x), y + sy * np.spacing(y)) for sx, sy in shifts]

    s0, s1 = samples(pts0), samples(pts1)
    base = G6.per_bin_map(s1[4], s0[4], c.nb, 1)
    worst = 0.0
    for a in s0:
        for b in s1:
            m = G6.per_bin_map(b, a, c.nb, 1)
            worst = max(worst, float((np.abs(m - base) / (1e-12 * (1 + np.abs(base)))).max()))
    return worst


@pytest.mark.parametrize("cid", [c.id for c in CASES if "scv_b" in c.models and c.literal])
def test_bilinear_maps_are_conditioned_against_coordinate_rounding(cid):
    assert bilinear_map_coordinate_sensitivity(cid) <= 0.1, cid   # (a tenth of the bound: the device's grid may be off by more than one ulp)


@pytest.mark.parametrize("cid,model", PAIRS)
def test_maps_have_an_empty_bin_and_a_non_identity_entry(cid, model):
    c = BY_ID[cid]
    r = ref(cid, model)
    maps = np.atleast_2d(r["maps"])
    ident = np.arange(c.nb, dtype=np.float64)
    It, I0o = r["It_orig"], patch(cid).I0o
    keyed = It if model in ("rscv", "lrscv") else I0o          # the image whose bins key the map
    counts = np.bincount(np.clip(keyed.astype(np.int64), 0, c.nb - 1), minlength=c.nb)
    if model == "scv_b":   # (a Bilinear sample also weighs into the bin above)
        counts = counts + np.bincount(np.clip(keyed.astype(np.int64) + 1, 0, c.nb - 1), minlength=c.nb)
    if not (c.nb == 2 and model == "scv_b"):   # (2 bins, Bilinear: every sample in (0, 1) weighs into both bins -- none can be empty)
        assert (counts == 0).any(), cid
    assert all((m[counts == 0] == ident[counts == 0]).all() for m in maps), cid
    if c.identity_ok and model != "scv_b":   # (see the module docstring: no Dirac map of these cases can leave the identity)
        return
    assert any((m != ident).any() for m in maps), cid


@pytest.mark.parametrize("cid", [c.id for c in CASES if c.group == "edge"])
def test_edge_cases_mix_border_and_image_samples(cid):
    c = BY_ID[cid]
    border = 128.0 * G6.pix_mult(c.nb)
    for v in (patch(cid).I0o, sampled(cid)[0]):
        out = v == border
        if c.edge == "outside":
            assert out.all()
            continue
        assert 0.2 <= out.mean() <= 0.8, (cid, out.mean())
        waves = [out[k:k + 64] for k in range(0, v.size, 64)]
        assert any(wv.any() and not wv.all() for wv in waves), cid
    assert c.resx * c.resy % 64 != 0   # (900 and 851 pixels: the last wave is ragged)


def test_case_table_covers_the_seams():
    n = {c.id: c.resx * c.resy for c in CASES}
    assert [n[i] for i in n if i.startswith("px_")] == [9, 63, 64, 65, 255, 256, 258, 2048, 2050, 4096, 4160]
    assert n["cap_362x363"] > 64 * 8 * 256 >= 362 * 362 and n["cap_512x513"] > 64 * 16 * 256 >= 512 * 512
    assert sorted({(c.nb + 63) >> 6 for c in CASES if c.group == "bins"}) == [1, 2, 3, 4]
    # the sub-region decompositions: coinciding sub-regions are one cell; one-pixel-wide and touching ones do not overlap
    assert G8.cells(21, 3, 0)[2] == 1 and G8.cells(21, 3, 10)[2] == 3 and G8.cells(30, 3, 10)[2] == 3
    assert G8.regions(21, 21, 3, 3, 10, 10)[0] == [(0, 0), (10, 10), (20, 20)]
    assert G8.regions(30, 30, 3, 3, 10, 10)[0] == [(0, 9), (10, 19), (20, 29)]


@pytest.mark.parametrize("model", ["lscv", "lrscv"])
@pytest.mark.parametrize("mapping", [0, 1, 2])
def test_coinciding_sub_regions_give_the_one_region_map(model, mapping):
    c = BY_ID["geo_coincide_m%d" % mapping]
    r = ref(c.id, model)
    one = c._replace(geo=(1, 1, 0, 0))
    m1, _ = maps_of(one, model, r["It_orig"], patch(c.id).I0o)
    for m in r["maps"]:
        np.testing.assert_array_equal(m, m1[0])


@pytest.mark.parametrize("cid,model", [(c, m) for c, m in PAIRS if BY_ID[c].track])
def test_track_cases_are_well_conditioned(cid, model):
    """the 5-iteration tracks the device is held to (1e-6 px): make_golden7.py's rule, every method's fifth step below 0.5 in every
    parameter"""
    for method in ("esm", "fclk"):
        n, dps, _, _ = ref_track(cid, model, method)
        assert n == 5 and np.abs(dps[-1]).max() < 0.5, (cid, model, method, [float(np.abs(d).max()) for d in dps])


# (model, once_per_frame, affine SSM)
BATCH_CONFIGS = [(m, 0, a) for m in MODELS for a in (True, False)] + [(m, 1, a) for m in ("lscv", "lrscv") for a in (True, False)]


@pytest.mark.parametrize("model,once,affine", BATCH_CONFIGS)
def test_batch_premise_three_distinct_iteration_counts(model, once, affine):
    """the mixed batch of the device test stops its targets at three or more different iterations in the reference's own loop, and no
    stopping decision is within 0.1 % of epsilon (so the device's count is the reference's)"""
    n, runs = batch_ref_iters(affine, model, once, 11)
    assert len(set(n.tolist())) >= 3, n
    _, _, kinds = batch_targets(affine, 11)
    assert all(n[k] == 1 for k in range(11) if kinds[k] != "moved"), (n, kinds)
    assert all(m > 1e-3 for r in runs for m in r[3]), [min(r[3]) for r in runs]


def test_lds_budget_counts():
    assert lds_limit_counts(64) == (64, 127, 129)
    assert lds_limit_counts(256) == (16, 31, 33)
