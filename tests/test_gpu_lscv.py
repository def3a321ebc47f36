"""The HIP LSCV path (am = MTFHIP_AM_LSCV: SSD on the template re-mapped through one E[It | I0_orig] per sub-region, blended with
per-pixel weights) against the independent float64 definitions of tests/golden/make_golden8.py (fixture lk_golden8.npz), in both math
modes:

- the maps (bit for bit), the re-mapped I0 (bit for bit with nearest mapping, 1e-12 with linear mapping and the affine fit), f and df/dIt (the
  SCV tolerances: f 1e-10 relative, df/dIt 1e-8), g and H (1e-5 relative) -- through the per-function entry points and Batch.iterate;
- the state update and the corners after 5 ESM / FCLK iterations of Batch.track (1e-6 px), once_per_frame 0 and 1, one and many targets;
- 1 x 1 LSCV with once_per_frame 0 against AM_SCV Dirac over a whole track, bit for bit; the first-iteration flag; reproducibility; the
  refused configurations; HipAM("lscv") through the harness."""
import ctypes
import os

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "lk_golden8.npz"))
TAGS = [str(t) for t in G["tags"]]
TRACK_TAGS = [t for t in TAGS if t + "_esm_dp" in G]
MATHS = [mtf_amd.MATH_REPLAY, mtf_amd.MATH_FAST]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def cfg(tag):
    return tuple(int(v) for v in G[tag + "_cfg"])   # nb, resx, resy, nx, ny, sx, sy, affine_mapping, once, linear, affine SSM


def lscv_batch(ctx, tags, math, once=None):
    nb, resx, resy, nx, ny, sx, sy, am, o, lin, aff = cfg(tags[0])
    ctx.set_image(G["img"])
    b = mtf_amd.Batch(ctx, L.AM_LSCV, L.SSM_AFFINE if aff else L.SSM_HOMOGRAPHY, resx, resy, len(tags), mi_n_bins=nb)
    b.set_lscv(nx, ny, sx, sy, am, o if once is None else once, lin)
    b.set_math_mode(math)
    b.set_corners(np.stack([G[t + "_corners"] for t in tags]))
    return b


def check_template(b, k, tag):
    """the re-mapped I0: bit for bit with nearest mapping (a function of the template's bins, the maps and the weights); 1e-12 with the
    affine fit (the device's closed form against lstsq) and with linear mapping (it reads I0_orig itself, and the device's template
    samples are not pinned to the last bit against the float64 sampler of the fixture: 16 of 2500 pixels differ by an ulp)"""
    I0 = b.read(L.BUF_I0)[k]
    if cfg(tag)[7] or cfg(tag)[9]:
        np.testing.assert_allclose(I0[:16], G[tag + "_I0_head"], rtol=0, atol=1e-12)
        if tag + "_I0" in G:
            np.testing.assert_allclose(I0, G[tag + "_I0"], rtol=0, atol=1e-12)
    else:
        np.testing.assert_array_equal(I0[:16], G[tag + "_I0_head"])
        if tag + "_I0" in G:
            np.testing.assert_array_equal(I0, G[tag + "_I0"])


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("tag", TAGS)
def test_lscv_golden8_interface(gpu_ctx, tag, math):
    b = lscv_batch(gpu_ctx, [tag], math)
    b.initialize_pix_vals(); b.initialize_pix_grad(); b.initialize_similarity(); b.initialize_grad(); b.initialize_hess()
    nb, nsub = cfg(tag)[0], cfg(tag)[3] * cfg(tag)[4]
    np.testing.assert_array_equal(b.lscv_intensity_maps()[0], np.tile(np.arange(nb, dtype=np.float64), (nsub, 1)))
    b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DI0_DX, L.BUF_J0)
    b.set_state(G[tag + "_p"][None])
    b.set_first_iter(True)   # (once_per_frame: the re-map runs on the first iteration only)
    b.update_pix_vals(); b.update_similarity(False); b.update_curr_grad(); b.update_init_grad(); b.update_pix_grad()
    np.testing.assert_array_equal(b.lscv_intensity_maps()[0], G[tag + "_maps"])
    check_template(b, 0, tag)
    f = float(G[tag + "_f"])
    assert abs(b.get_similarity()[0] - f) <= 1e-10 * abs(f)
    dft = b.read(L.BUF_DF_DIT)[0]
    np.testing.assert_allclose(dft[:16], G[tag + "_df_dIt_head"], rtol=1e-8, atol=1e-12)
    if tag + "_df_dIt" in G:
        np.testing.assert_allclose(dft, G[tag + "_df_dIt"], rtol=1e-8, atol=1e-12)
    b.cmpt_warped_pix_jacobian()
    assert rel(b.cmpt_curr_jacobian()[0], G[tag + "_g"]) < 1e-5
    assert rel(b.cmpt_curr_hessian()[0], G[tag + "_H"]) < 1e-5
    b.close()


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("materialize", [0, 1])
@pytest.mark.parametrize("tag", TAGS)
def test_lscv_golden8_fused(gpu_ctx, tag, materialize, math):
    """Batch.iterate (FCLK, CurrentSelf) from the fixture state: the re-map, then the fused SSD pass on it"""
    b = lscv_batch(gpu_ctx, [tag], math)
    sm = mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, materialize=materialize, leven_marq=0)
    b.init_template(sm)
    b.set_state(G[tag + "_p"][None])
    b.set_first_iter(True)
    f, g, H = b.iterate(sm)
    np.testing.assert_array_equal(b.lscv_intensity_maps()[0], G[tag + "_maps"])
    check_template(b, 0, tag)
    ft = float(G[tag + "_f"])
    assert abs(f[0] - ft) <= 1e-10 * abs(ft)
    assert rel(g[0], G[tag + "_g"]) < 1e-5
    assert rel(H[0], G[tag + "_H"]) < 1e-5
    b.close()


def test_lscv_first_iter_flag(gpu_ctx):
    """a fresh batch has the flag clear: with once_per_frame 1 the per-function update_similarity then does not re-map; with it set it
    does; with once_per_frame 0 it re-maps either way"""
    tag = "ship_50"
    b = lscv_batch(gpu_ctx, [tag], mtf_amd.MATH_REPLAY)
    assert not b.first_iter()
    b.initialize_pix_vals(); b.initialize_pix_grad(); b.initialize_similarity()
    I0_orig = b.read(L.BUF_I0)[0].copy()
    b.set_state(G[tag + "_p"][None])
    b.update_pix_vals(); b.update_similarity(False)
    np.testing.assert_array_equal(b.read(L.BUF_I0)[0], I0_orig)
    b.set_first_iter(True)
    assert b.first_iter()
    b.update_similarity(False)
    check_template(b, 0, tag)
    b.close()


def track_sm(method, materialize=0):
    if method == "esm":
        return mtf_amd.sm_desc(L.SM_ESM, jac_type=1, hess_type=2, max_iters=5, epsilon=0.0, materialize=materialize, leven_marq=0)
    return mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, max_iters=5, epsilon=0.0, materialize=materialize, leven_marq=0)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("method", ["esm", "fclk"])
@pytest.mark.parametrize("tag", TRACK_TAGS)
def test_lscv_golden8_track(gpu_ctx, tag, method, math):
    """5 iterations of the device loop from the fixture state, with the case's once_per_frame: the last state update and the corners"""
    b = lscv_batch(gpu_ctx, [tag], math)
    sm = track_sm(method)
    b.init_template(sm)
    b.set_state(G[tag + "_p"][None])
    b.track_trace(5)
    n, corners = b.track(sm)
    assert int(n[0]) == 5
    assert not b.first_iter()
    recs = b.read_track_trace(n)[0]
    np.testing.assert_allclose(recs[-1]["dp"], G[tag + "_" + method + "_dp"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(corners[0], G[tag + "_" + method + "_corners"], rtol=0, atol=1e-6)
    b.track_trace(0)
    b.close()


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("tag", ["ship_200", "near_50"])
def test_lscv_track_many_targets_matches_single(gpu_ctx, tag, math):
    """the chunked / multi-queue device loop on 6 copies of a case: every target lands on the fixture's corners"""
    tags = [tag] * 6
    b = lscv_batch(gpu_ctx, tags, math)
    for method in ("esm", "fclk"):
        sm = track_sm(method, materialize=1 if method == "esm" else 0)
        b.set_corners(np.stack([G[t + "_corners"] for t in tags]))
        b.init_template(sm)
        b.set_state(np.stack([G[t + "_p"] for t in tags]))
        _, corners = b.track(sm)
        for k in range(len(tags)):
            np.testing.assert_allclose(corners[k], G[tag + "_" + method + "_corners"], rtol=0, atol=1e-6)
    b.close()


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("lin", [0, 1])
@pytest.mark.parametrize("method", ["esm", "fclk"])
def test_lscv_one_sub_region_equals_scv(gpu_ctx, lin, method, math):
    """1 x 1 LSCV, once_per_frame 0: I0, the state updates and the corners of a whole track bit for bit those of AM_SCV Dirac"""
    tag = "near_50"
    res = {}
    for am in (L.AM_SCV, L.AM_LSCV):
        gpu_ctx.set_image(G["img"])
        b = mtf_amd.Batch(gpu_ctx, am, L.SSM_HOMOGRAPHY, 50, 50, 3, mi_n_bins=64)
        if am == L.AM_SCV:
            b.set_scv(0, lin, 0)
        else:
            b.set_lscv(1, 1, 10, 10, 0, 0, lin)
        b.set_math_mode(math)
        b.set_corners(np.stack([G[tag + "_corners"] + d for d in (0.0, 1.5, -2.0)]))
        sm = track_sm(method)
        b.init_template(sm)
        b.set_state(np.stack([G[tag + "_p"] * s for s in (1.0, 0.5, -0.7)]))
        b.track_trace(5)
        n, corners = b.track(sm)
        res[am] = (corners.copy(), b.read(L.BUF_I0).copy(), [r["dp"] for r in b.read_track_trace(n)[0]])
        b.track_trace(0)
        b.close()
    np.testing.assert_array_equal(res[L.AM_SCV][0], res[L.AM_LSCV][0])
    np.testing.assert_array_equal(res[L.AM_SCV][1], res[L.AM_LSCV][1])
    np.testing.assert_array_equal(np.array(res[L.AM_SCV][2]), np.array(res[L.AM_LSCV][2]))


@pytest.mark.parametrize("once", [0, 1])
def test_lscv_reproducible(gpu_ctx, once):
    """ten iterate calls and two track calls, 8 targets of 200 x 200, the shipped configuration: identical bits"""
    tag = "ship_200"
    gpu_ctx.set_image(G["img"])
    B = 8
    b = mtf_amd.Batch(gpu_ctx, L.AM_LSCV, L.SSM_HOMOGRAPHY, 200, 200, B, mi_n_bins=64)
    b.set_lscv(3, 3, 10, 10, 1, once, 0)
    rng = np.random.default_rng(5)
    from mtf_amd import synth
    cs = np.stack([G[tag + "_corners"] + rng.uniform(-3, 3, (1, 1)) for _ in range(B)])
    ps = np.stack([synth.random_small_homography(rng, 0.4) for _ in range(B)])
    b.set_corners(cs)
    sm = mtf_amd.sm_desc(L.SM_ESM, materialize=0, leven_marq=0)
    b.init_template(sm)
    first = None
    for _ in range(10):
        b.set_state(ps)
        b.set_first_iter(True)
        f, g, H = b.iterate(sm)
        cur = (f.copy(), g.copy(), H.copy(), b.lscv_intensity_maps().copy(), b.read(L.BUF_I0).copy())
        if first is None:
            first = cur
        for a, c in zip(first, cur):
            np.testing.assert_array_equal(a, c)
    smt = mtf_amd.sm_desc(L.SM_ESM, max_iters=10, epsilon=0.0, materialize=0, leven_marq=0)
    runs = []
    for _ in range(2):
        b.set_corners(cs)
        b.init_template(smt)
        b.set_state(ps)
        _, corners = b.track(smt)
        runs.append((corners.copy(), b.lscv_intensity_maps().copy()))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    b.close()


def test_lscv_refusals(gpu_ctx):
    gpu_ctx.set_image(G["img"])
    tag = "near_50"

    def fresh(resx=50, resy=50, nb=64):
        b = mtf_amd.Batch(gpu_ctx, L.AM_LSCV, L.SSM_HOMOGRAPHY, resx, resy, 1, mi_n_bins=nb)
        b.set_corners(G[tag + "_corners"][None])
        return b

    b = fresh()
    with pytest.raises(mtf_amd.InvalidArgument, match="not enough to use the specified region spacing"):
        b.set_lscv(3, 3, 25, 10, 0, 0, 0)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="second-order"):
        b.init_template(mtf_amd.sm_desc(L.SM_ESM, sec_ord_hess=1))
    sm = mtf_amd.sm_desc(L.SM_ESM, leven_marq=0)
    b.init_template(sm)
    with pytest.raises(mtf_amd.LogicError, match="before init_template"):
        b.set_lscv()
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="second-order"):
        b.iterate(mtf_amd.sm_desc(L.SM_ESM, sec_ord_hess=1))
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="LSCVDist"):
        b.score_candidates(np.zeros((4, 8)))
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="LSCVDist"):
        b.nn_dataset(4, np.full(8, 0.01))
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="grid tracker"):
        b.grid_update(G[tag + "_corners"][None], sm)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="updateModel"):
        b.update_model()
    lib = L.lib()
    pf = ctypes.c_void_p()
    desc = ctypes.create_string_buffer(4096)
    assert lib.mtfhip_pf_create(b._h, ctypes.addressof(desc), ctypes.addressof(pf)) == -2
    assert "particle filter" in lib.mtfhip_last_error().decode()
    b.close()
    b = fresh()
    b.set_lscv(3, 3, 10, 10, 0, 1, 0)
    b.init_template(sm)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="Levenberg-Marquardt"):
        b.track(mtf_amd.sm_desc(L.SM_FCLK, leven_marq=1))
    b.close()
    b = fresh(100, 100, 256)   # 9 x 9 sub-regions: 289 cells x 256 bins x 8 B of histograms
    b.set_lscv(9, 9, 5, 5, 0, 0, 0)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="LDS"):
        b.init_template(sm)
    b.close()
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="MCLSCV"):
        mtf_amd.Batch(gpu_ctx, L.AM_LSCV, L.SSM_HOMOGRAPHY, 50, 50, 1, mi_n_bins=64, n_channels=3)


@pytest.mark.parametrize("once,affine", [(1, 1), (0, 0)])
def test_lscv_cpp_harness_matches_python(gpu_ctx, once, affine):
    """HipAM("lscv") built from its LSCVParams through the harness: under mtf::hip::LK (the device loop) the same corners as Batch.track
    bit for bit; under nt::ESM (the reference's loop over the AM / SSM virtuals, setFirstIter / clearFirstIter included) within 1e-6 px"""
    from mtf_amd import host
    import test_gpu_scv
    f0, f1, c0, _ = test_gpu_scv.gamma_pair()
    kw = dict(max_iters=10, epsilon=1e-6, leven_marq=0)
    gpu_ctx.set_image(f0)
    b = mtf_amd.Batch(gpu_ctx, L.AM_LSCV, L.SSM_HOMOGRAPHY, 50, 50, 1, mi_n_bins=64)
    b.set_lscv(3, 3, 10, 10, affine, once, 0)
    sm = mtf_amd.sm_desc(L.SM_ESM, materialize=0, **kw)
    b.set_corners(c0[None])
    b.init_template(sm)
    gpu_ctx.set_image(f1)
    _, corners = b.track(sm)
    b.close()
    for device_loop in (True, False):
        t = host.CppTracker.lscv(L.SM_ESM, L.SSM_HOMOGRAPHY, 50, 50, n_bins=64, affine_mapping=affine, once_per_frame=once,
                                 device_loop=device_loop, **kw)
        t.set_image(f0)
        t.initialize(c0)
        t.set_image(f1)
        t.update()
        cpp = np.asarray(t.get_region()).reshape(2, 4)
        if device_loop:
            np.testing.assert_array_equal(cpp, corners[0])
        else:
            np.testing.assert_allclose(cpp, corners[0], rtol=0, atol=1e-6)
