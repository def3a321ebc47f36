"""The seams of the additive search methods (FALK / IALK) and of the low-order state space models (Similitude / Isometry / Translation
under ESM / FCLK / ICLK), no GPU: the conditions the references alone must meet on every case of tests/helpers/addlow_seam_cases.py so
that the device comparison of tests/test_gpu_alk_lowdof_seams.py is meaningful.  384 cases (36 (shape, region) pairs x every third of 32 models), 72 parameter sets.

(a) H, g and f of the compared pass are finite -- except NCC wholly outside the frame, where the reference divides 0 by 0: the table marks
    those cases reference_nan, I0 is all 128 there and the reference must really return a non-finite H or g;
(b) SSD wholly outside the frame: f = 0, g = 0, H = 0 exactly;
(c) the half-outside regions have 20 .. 80 % of their template samples equal to the border constant 128 and, from 64 pixels on, a run of
    64 consecutive pixels that holds both kinds;
(d) no sample point of the compared pass is within 1e-6 of an integer coordinate (FALK's +-grad_eps = 1e-8 stencil included);
(e) the jitter floor: corners moved by a seeded +-1e-12 px (one sign pattern for the whole table) change the reference's H and g by less
    than 1e-6, a tenth of the 1e-5 the device is held to on its own grid.  Measured maximum over the table: 6.8e-7 (2 x 3 FALK NCC homography; the next are 2 x 3 too: from 35 pixels on the maximum is 5.1e-7).  Four cases
    broke the floor at the usual start state (1.2e-6 .. 1.6e-6) and run at another one: addlow_seam_cases.ALT_START;
(f) `quad` on the homography gives an init_pts_hm whose third row is more than 1e-6 from 1 somewhere (the unit_z = 0 branch is what
    runs); on the affine and the three low-order models the third row is exactly 1;
(g) the device-loop cases: the reference stops by epsilon before max_iters on `inside` and `quad` at every loop shape for every model
    the GPU test compares final corners on (addlow_seam_cases.corners_compared: all but undamped FALK / IALK with InitialSelf)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import addlow_seam_cases as K   # noqa: E402

JITTER_SEED = 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_covers_what_it_claims():
    assert 250 <= len(K.CASES) <= 450 and len(set(K.IDS)) == len(K.CASES)
    names = [K.model_name(m) for m in K.MODELS]
    assert len(set(names)) == len(names) == 32
    assert sum(len(K.variants(m)) for m in K.ALK_MODELS) == 24 and sum(len(K.variants(m)) for m in K.LOW_MODELS) == 48
    for shape in K.SHAPES:                                # every small shape on `inside`, both families
        fams = {c.model.family for c in K.CASES if (c.resx, c.resy) == shape and c.region == "inside"}
        assert fams == {K.ALK, K.LOW}, shape
    for shape in K.FULL_SHAPES:                           # every region on the three full shapes
        assert {c.region for c in K.CASES if (c.resx, c.resy) == shape} == set(K.REGIONS), shape
    for shape in K.BIG_SHAPES:
        assert {c.region for c in K.CASES if (c.resx, c.resy) == shape} == {"inside", "quad"}, shape
    for m in K.MODELS:
        mine = [c for c in K.CASES if c.model is m]
        assert {c.region for c in mine} == set(K.REGIONS), K.model_name(m)                      # every model on every region
        assert any((c.resx, c.resy) in K.BIG_SHAPES for c in mine), K.model_name(m)             # ... and on a BIG shape
        assert any((c.resx, c.resy) in K.BIG_SHAPES and c.region == "quad" for c in mine), K.model_name(m)   # ... on `quad` (ALK: the issue's claim)
    for fam in (K.ALK, K.LOW):
        assert {1, 2, 9, 17, 25} <= {c.nblk for c in K.CASES if c.model.family == fam}, fam
        for am in (K.SSD, K.NCC):                          # each edge under each appearance model
            assert set(K.HALF_OUTSIDE) <= {c.region for c in K.CASES if c.model.family == fam and c.model.am == am}
    assert {(m.ssm) for m in K.LOW_MODELS} == {K.TRANS, K.ISO, K.SIM}
    # a homography additive case with unit_z = 0 from set_corners itself
    assert any(c.model.family == K.ALK and c.model.ssm == K.HOM and c.region == "quad" for c in K.CASES)


def test_expected_partial_rows():
    """the table's nblk at the shapes the issue names, for one target and for a batch of three"""
    want = {(2, 2): 1, (33, 31): 1, (32, 32): 1, (32, 33): 2, (37, 23): 1, (91, 91): 9, (95, 97): 9, (129, 128): 17, (158, 158): 25}
    for (resx, resy), nblk in want.items():
        assert K.fused_decomposition(resx * resy, 1)[0] == nblk, (resx, resy)
    assert K.fused_decomposition(91 * 91, 3) == (9, 4)
    assert 95 * 97 % 256 == 255
    for c in K.CASES:
        assert c.nblk == K.fused_decomposition(c.resx * c.resy, 1)[0]


def test_decomposition_constants_are_the_librarys():
    """MTFHIP_SLOTS, MTFHIP_MIN_ROWS and kBlock as mtfhip_internal.h defines them are the restatement's defaults: a change of the
    decomposition fails here instead of silently moving the seams"""
    import inspect
    src = open(os.path.join(ROOT, "mtf_amd", "csrc", "mtfhip_internal.h")).read()
    slots = int(re.search(r"#define\s+MTFHIP_SLOTS\s+(\d+)", src).group(1))
    min_rows = int(re.search(r"#define\s+MTFHIP_MIN_ROWS\s+(\d+)", src).group(1))
    block = int(re.search(r"constexpr\s+int\s+kBlock\s*=\s*(\d+)\s*;", src).group(1))
    d = {k: v.default for k, v in inspect.signature(K.fused_decomposition).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(slots=slots, min_rows=min_rows, block=block)


def _jittered(region):
    return K.REGIONS[region] + np.random.default_rng(JITTER_SEED).choice([-1e-12, 1e-12], size=(2, 4))


def jitter_of(oracle, frame, frame2, c, ref):
    """the largest relative change of H and of g (against max(|g|, g_scale)) over the case's variants under the seeded corner jitter"""
    jit = K.first_pass(oracle, frame, frame2, c.model, c.resx, c.resy, _jittered(c.region), alt=c.alt_start)
    worst = 0.0
    for label, _ in K.variants(c.model):
        rec, j = ref["recs"][label], jit["recs"][label]
        eH = K.rel(j["H"], rec["H"])
        eg = float(np.linalg.norm(j["g"] - rec["g"]) / max(np.linalg.norm(rec["g"]), K.g_scale(rec, c.model.am)))
        worst = max(worst, eH, eg)
    return worst


@pytest.mark.parametrize("cid", K.IDS)
def test_reference_conditions(oracle, frame, frame2, cid):
    c = K.BY_ID[cid]
    m = c.model
    ref = K.reference(oracle, frame, frame2, cid)
    N = K.n_pix(c)
    recs = [ref["recs"][label] for label, _ in K.variants(m)]
    assert ref["I0"].shape == (N,)
    # (a)
    if c.reference_nan:
        assert np.all(ref["I0"] == 128.0)
        for rec in recs:
            assert not np.all(np.isfinite(rec["H"])) or not np.all(np.isfinite(rec["g"]))
        return
    for rec in recs:
        assert np.all(np.isfinite(rec["H"])) and np.all(np.isfinite(rec["g"])) and np.isfinite(rec["f"])
    # (b)
    if c.region == "outside":
        for rec in recs:
            assert rec["f"] == 0.0 and np.all(rec["g"] == 0.0) and np.all(rec["H"] == 0.0)
        return
    # (c)
    if c.region in K.HALF_OUTSIDE:
        border = ref["I0"] == 128.0
        assert 0.2 <= border.mean() <= 0.8, border.mean()
        if N >= 64:
            assert any(0 < border[s:s + 64].sum() < 64 for s in range(N - 63))
    # (d)
    pts = ref["curr_pts"]
    assert np.abs(pts - np.round(pts)).min() > 1e-6
    # (f)
    if c.region == "quad":
        z = ref["init_pts_hm"][2]
        if m.family == K.ALK and m.ssm == K.HOM:
            assert np.abs(z - 1.0).max() > 1e-6
        else:
            assert np.all(z == 1.0)
    # (e)
    j = jitter_of(oracle, frame, frame2, c, ref)
    print("jitter %s %.3e" % (cid, j))
    assert j < 1e-6


@pytest.mark.parametrize("model", K.LOOP_MODELS, ids=K.model_name)
def test_loop_references_converge(oracle, frame, frame2, model):
    """(g): on `inside` and `quad` at every loop shape the reference stops by epsilon before max_iters wherever the GPU test compares
    final corners (corners_compared); the models it does not compare them on really run into max_iters everywhere"""
    for shape in K.LOOP_SHAPES:
        for region in K.CORNER_REGIONS:
            run = K.full_run(oracle, frame, frame2, model, shape[0], shape[1], region)
            assert np.all(np.isfinite(run["corners"]))
            assert K.converged(run) == K.corners_compared(model), (shape, region, run["n_iters"])


def test_long_double_solve_small_systems():
    """the yardstick serves the 2-, 3- and 4-parameter systems of the low-order models"""
    rng = np.random.default_rng(3)
    for n in (2, 3, 4, 6):
        A = rng.normal(size=(n, n)); A = A + A.T
        x = rng.normal(size=n)
        assert np.abs(np.asarray(K.long_double_solve(A, A @ x), dtype=np.float64) - x).max() < 1e-12
