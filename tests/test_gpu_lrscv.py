"""The HIP LRSCV path (am = MTFHIP_AM_LRSCV: SSD on the current patch mapped through one E[I0 | It] per sub-region and blended with
per-pixel weights, inside the fused pass) against the independent float64 definitions of tests/golden/make_golden9.py (fixture
lk_golden9.npz), in both math modes unless noted:

- the maps (bit for bit), the blended It (bit for bit with nearest mapping in replay mode; 1e-12 otherwise), f (1e-10 relative), df/dIt
  (1e-8), g and H (1e-5 relative) through the per-function entry points and Batch.iterate (materialise 0 and 1); the materialised It
  bit for bit the per-function route's;
- the state update and the corners after 5 ESM / FCLK / ICLK iterations of Batch.track (1e-6 px); 64 targets on the bits each gives alone;
- 1 x 1 LRSCV against AM_RSCV over whole tracks, bit for bit; once_per_frame 1 against one LRSCV pass followed by SSD passes, bit for bit;
- reproducibility, the refused configurations and HipAM("lrscv") through the harness."""
import ctypes
import os

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "lk_golden9.npz"))
G7 = np.load(os.path.join(HERE, "golden", "lk_golden7.npz"))
TAGS = [str(t) for t in G["tags"]]
TRACK_TAGS = [t for t in TAGS if t + "_esm_dp" in G]
MATHS = [mtf_amd.MATH_REPLAY, mtf_amd.MATH_FAST]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def cfg(tag):
    return tuple(int(v) for v in G[tag + "_cfg"])   # nb, resx, resy, nx, ny, sx, sy, affine_mapping, once, linear, affine SSM


def lrscv_batch(ctx, tags, math, once=None):
    nb, resx, resy, nx, ny, sx, sy, am, o, lin, aff = cfg(tags[0])
    ctx.set_image(G["img"])
    b = mtf_amd.Batch(ctx, L.AM_LRSCV, L.SSM_AFFINE if aff else L.SSM_HOMOGRAPHY, resx, resy, len(tags), mi_n_bins=nb)
    b.set_lrscv(nx, ny, sx, sy, am, o if once is None else once, lin)
    b.set_math_mode(math)
    b.set_corners(np.stack([G[t + "_corners"] for t in tags]))
    return b


def check_it(It, tag, math):
    """the blended current patch: bit for bit with nearest mapping in replay mode (a function of the current bins, the maps and the
    weights); 1e-12 with the affine fit (closed form against lstsq), linear mapping (it reads It_orig itself) and in tolerance mode"""
    exact = not (cfg(tag)[7] or cfg(tag)[9]) and math == mtf_amd.MATH_REPLAY
    check = np.testing.assert_array_equal if exact else (lambda a, b: np.testing.assert_allclose(a, b, rtol=0, atol=1e-12))
    check(It[:16], G[tag + "_It_head"])
    if tag + "_It" in G:
        check(It, G[tag + "_It"])


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("tag", TAGS)
def test_lrscv_golden9_interface(gpu_ctx, tag, math):
    b = lrscv_batch(gpu_ctx, [tag], math)
    b.initialize_pix_vals(); b.initialize_pix_grad(); b.initialize_similarity(); b.initialize_grad(); b.initialize_hess()
    nb, nsub = cfg(tag)[0], cfg(tag)[3] * cfg(tag)[4]
    np.testing.assert_array_equal(b.lrscv_intensity_maps()[0], np.tile(np.arange(nb, dtype=np.float64), (nsub, 1)))
    b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DI0_DX, L.BUF_J0)
    b.set_state(G[tag + "_p"][None])
    b.set_first_iter(True)   # (once_per_frame: the map is built on the first iteration only)
    b.update_pix_vals(); b.update_similarity(False); b.update_curr_grad(); b.update_init_grad(); b.update_pix_grad()
    np.testing.assert_array_equal(b.lrscv_intensity_maps()[0], G[tag + "_maps"])
    check_it(b.read(L.BUF_IT)[0], tag, math)
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


def test_lrscv_once_per_frame_per_function_leaves_it_raw(gpu_ctx):
    """once_per_frame 1 and the flag clear: update_pix_vals writes the raw patch (LRSCV.cc:234-235) and leaves the maps alone"""
    tag = "ship_50"
    nb = cfg(tag)[0]
    b = lrscv_batch(gpu_ctx, [tag], mtf_amd.MATH_REPLAY)
    assert not b.first_iter()
    b.initialize_pix_vals(); b.initialize_pix_grad(); b.initialize_similarity()
    b.set_state(G[tag + "_p"][None])
    b.update_pix_vals()
    np.testing.assert_array_equal(b.lrscv_intensity_maps()[0], np.tile(np.arange(nb, dtype=np.float64), (9, 1)))
    raw = b.read(L.BUF_IT)[0].copy()
    np.testing.assert_allclose(raw[:16], G[tag + "_It_orig_head"], rtol=0, atol=1e-12)
    b.set_first_iter(True)
    b.update_pix_vals()
    np.testing.assert_array_equal(b.lrscv_intensity_maps()[0], G[tag + "_maps"])
    check_it(b.read(L.BUF_IT)[0], tag, mtf_amd.MATH_REPLAY)
    b.close()


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("materialize", [0, 1])
@pytest.mark.parametrize("tag", TAGS)
def test_lrscv_golden9_fused(gpu_ctx, tag, materialize, math):
    """Batch.iterate (FCLK, CurrentSelf) from the fixture state: pass 1, then the fused pass blending every sample; the materialised It
    is the per-function route's bit for bit"""
    b = lrscv_batch(gpu_ctx, [tag], math)
    sm = mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, materialize=materialize, leven_marq=0)
    b.init_template(sm)
    b.set_state(G[tag + "_p"][None])
    b.set_first_iter(True)
    f, g, H = b.iterate(sm)
    np.testing.assert_array_equal(b.lrscv_intensity_maps()[0], G[tag + "_maps"])
    ft = float(G[tag + "_f"])
    assert abs(f[0] - ft) <= 1e-10 * abs(ft), (f[0], ft)
    assert rel(g[0], G[tag + "_g"]) < 1e-5, rel(g[0], G[tag + "_g"])
    assert rel(H[0], G[tag + "_H"]) < 1e-5, rel(H[0], G[tag + "_H"])
    if materialize:
        it_fused = b.read(L.BUF_IT)[0].copy()
        check_it(it_fused, tag, mtf_amd.MATH_REPLAY)   # (a materialising launch samples with the replay expression in either mode)
        b.update_pix_vals()
        np.testing.assert_array_equal(b.lrscv_intensity_maps()[0], G[tag + "_maps"])
        np.testing.assert_array_equal(b.read(L.BUF_IT)[0], it_fused)
    b.close()


def track_sm(method, materialize=0, max_iters=5):
    kw = dict(max_iters=max_iters, epsilon=0.0, materialize=materialize, leven_marq=0)
    if method == "esm":
        return mtf_amd.sm_desc(L.SM_ESM, jac_type=1, hess_type=2, **kw)
    if method == "fclk":
        return mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, **kw)
    return mtf_amd.sm_desc(L.SM_ICLK, hess_type=0, **kw)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("method", ["esm", "fclk", "iclk"])
@pytest.mark.parametrize("tag", TRACK_TAGS)
def test_lrscv_golden9_track(gpu_ctx, tag, method, math):
    """5 iterations of the device loop from the fixture state, with the case's once_per_frame: the last state update (ESM / FCLK) and
    the corners"""
    b = lrscv_batch(gpu_ctx, [tag], math)
    sm = track_sm(method)
    b.init_template(sm)
    b.set_state(G[tag + "_p"][None])
    b.track_trace(5)
    n, corners = b.track(sm)
    assert int(n[0]) == 5
    assert not b.first_iter()
    if method != "iclk":   # (ICLK's trace holds the step before its inversion)
        recs = b.read_track_trace(n)[0]
        np.testing.assert_allclose(recs[-1]["dp"], G[tag + "_" + method + "_dp"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(corners[0], G[tag + "_" + method + "_corners"], rtol=0, atol=1e-6)
    b.track_trace(0)
    b.close()


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("tag,method", [("near_50", "esm"), ("ship_50", "fclk"), ("aff_40", "esm"), ("lin_50", "iclk")])
def test_lrscv_track_64_targets_same_bits_as_one_at_a_time(gpu_ctx, tag, method, math):
    """64 targets at different states in one batch (chunked / multi-queue device loop, pass 1 per chunk) give the bits each gives alone"""
    B = 64
    rng = np.random.default_rng(17)
    S = 6 if cfg(tag)[10] else 8
    scale = [0.2, 0.2, 2e-3, 2e-3, 2e-3, 2e-3] if S == 6 else [2e-3, 2e-3, 0.2, 2e-3, 2e-3, 0.2, 1e-6, 1e-6]
    ps = np.stack([G[tag + "_p"]] + [G[tag + "_p"] + rng.uniform(-1, 1, S) * scale for _ in range(B - 1)])
    sm = track_sm(method, materialize=1 if method == "esm" else 0)
    b = lrscv_batch(gpu_ctx, [tag] * B, math)
    b.init_template(sm)
    b.set_state(ps)
    _, many = b.track(sm)
    b.close()
    if tag + "_" + method + "_corners" in G:
        np.testing.assert_allclose(many[0], G[tag + "_" + method + "_corners"], rtol=0, atol=1e-6)
    for k in range(B):
        b1 = lrscv_batch(gpu_ctx, [tag], math)
        b1.init_template(sm)
        b1.set_state(ps[k][None])
        _, one = b1.track(sm)
        b1.close()
        np.testing.assert_array_equal(many[k], one[0])


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("lin", [0, 1])
@pytest.mark.parametrize("method", ["esm", "fclk", "iclk"])
@pytest.mark.parametrize("tag7", ["r64n_50", "r64n_aff"])
def test_lrscv_one_sub_region_equals_rscv(gpu_ctx, tag7, method, lin, math):
    """1 x 1 LRSCV, once_per_frame 0: the weight is 1.0 and the blend 0 + m 1.0, so the maps, the state updates, the corners and the
    materialised It of a whole track are AM_RSCV's bit for bit"""
    nb, _, resx, resy, aff = (int(v) for v in G7[tag7 + "_cfg"])
    res = {}
    for am in (L.AM_RSCV, L.AM_LRSCV):
        gpu_ctx.set_image(G7["img"])
        b = mtf_amd.Batch(gpu_ctx, am, L.SSM_AFFINE if aff else L.SSM_HOMOGRAPHY, resx, resy, 3, mi_n_bins=nb)
        if am == L.AM_RSCV:
            b.set_rscv(0, lin, 0)
        else:
            b.set_lrscv(1, 1, 10, 10, 0, 0, lin)
        b.set_math_mode(math)
        b.set_corners(np.stack([G7[tag7 + "_corners"] + d for d in (0.0, 1.5, -2.0)]))
        sm = track_sm(method, materialize=1 if method == "esm" else 0)
        b.init_template(sm)
        b.set_state(np.stack([G7[tag7 + "_p"] * s for s in (1.0, 0.5, -0.7)]))
        b.track_trace(5)
        n, corners = b.track(sm)
        maps = b.rscv_intensity_map() if am == L.AM_RSCV else b.lrscv_intensity_maps()[:, 0]
        res[am] = (corners.copy(), maps.copy(), np.array([[r["dp"] for r in t] for t in b.read_track_trace(n)]),
                   b.read(L.BUF_IT).copy() if method == "esm" else None)
        b.track_trace(0)
        b.close()
    for a, c in zip(res[L.AM_RSCV], res[L.AM_LRSCV]):
        if a is not None:
            np.testing.assert_array_equal(a, c)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("method", ["esm", "fclk"])
def test_lrscv_once_per_frame_is_one_lrscv_pass_then_ssd(gpu_ctx, method, math):
    """once_per_frame 1: a 5-iteration track equals one LRSCV pass followed by 4 SSD passes from its state, bit for bit.  At 256 bins the
    normalisation is (256 - 1) / 255 = 1, so an AM_SSD batch samples the same template and the same raw patch"""
    tag = "n256_60"
    nb, resx, resy, nx, ny, sx, sy, *_ = cfg(tag)
    B = 3
    cs = np.stack([G[tag + "_corners"] + d for d in (0.0, 1.0, -1.5)])
    ps = np.stack([G[tag + "_p"] * s for s in (1.0, 0.6, -0.5)])
    gpu_ctx.set_image(G["img"])

    def lrscv(max_iters, once=1):
        b = mtf_amd.Batch(gpu_ctx, L.AM_LRSCV, L.SSM_HOMOGRAPHY, resx, resy, B, mi_n_bins=nb)
        b.set_lrscv(nx, ny, sx, sy, 0, once, 0)
        b.set_math_mode(math)
        b.set_corners(cs)
        sm = track_sm(method, max_iters=max_iters)
        b.init_template(sm)
        b.set_state(ps)
        _, corners = b.track(sm)
        return b, corners.copy()

    b5, c5 = lrscv(5)
    b5.close()
    b1, _ = lrscv(1)
    w1, p1 = b1.get_warp().copy(), b1.get_state().copy()
    b1.close()
    s = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, resx, resy, B)
    s.set_math_mode(math)
    s.set_corners(cs)
    sm = track_sm(method, max_iters=4)
    s.init_template(sm)
    s.set_state(p1)
    np.testing.assert_array_equal(s.get_warp(), w1)   # (the state carries the warp over exactly)
    _, c_ssd = s.track(sm)
    s.close()
    np.testing.assert_array_equal(c5, c_ssd)
    # with once_per_frame 0 the later passes map too: a different result
    b, c_every = lrscv(5, once=0)
    b.close()
    assert np.any(c_every != c5)


@pytest.mark.parametrize("once", [0, 1])
def test_lrscv_reproducible(gpu_ctx, once):
    """ten iterate calls and two track calls, 8 targets of 200 x 200, the shipped mapping (affine): identical bits"""
    tag = "ship_200"
    gpu_ctx.set_image(G["img"])
    B = 8
    b = mtf_amd.Batch(gpu_ctx, L.AM_LRSCV, L.SSM_HOMOGRAPHY, 200, 200, B, mi_n_bins=64)
    b.set_lrscv(3, 3, 10, 10, 1, once, 0)
    rng = np.random.default_rng(5)
    cs = np.stack([G[tag + "_corners"] + rng.uniform(-3, 3, (1, 1)) for _ in range(B)])
    ps = np.stack([synth.random_small_homography(rng, 0.4) for _ in range(B)])
    b.set_corners(cs)
    for mat in (0, 1):
        sm = mtf_amd.sm_desc(L.SM_ESM, materialize=mat, leven_marq=0)
        b.init_template(sm)
        first = None
        for _ in range(10):
            b.set_state(ps)
            b.set_first_iter(True)
            f, g, H = b.iterate(sm)
            cur = (f.copy(), g.copy(), H.copy(), b.lrscv_intensity_maps().copy()) + ((b.read(L.BUF_IT).copy(),) if mat else ())
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
        runs.append((corners.copy(), b.lrscv_intensity_maps().copy()))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    b.close()


def test_lrscv_refusals(gpu_ctx):
    gpu_ctx.set_image(G["img"])
    tag = "near_50"

    def fresh(resx=50, resy=50, nb=64):
        b = mtf_amd.Batch(gpu_ctx, L.AM_LRSCV, L.SSM_HOMOGRAPHY, resx, resy, 1, mi_n_bins=nb)
        b.set_corners(G[tag + "_corners"][None])
        return b

    b = fresh()
    with pytest.raises(mtf_amd.InvalidArgument, match="LRSCV :: Patch size .* not enough to use the specified region spacing"):
        b.set_lrscv(3, 3, 10, 25, 0, 0, 0)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="second-order"):
        b.init_template(mtf_amd.sm_desc(L.SM_ESM, sec_ord_hess=1))
    sm = mtf_amd.sm_desc(L.SM_ESM, leven_marq=0)
    b.init_template(sm)
    with pytest.raises(mtf_amd.LogicError, match="before init_template"):
        b.set_lrscv()
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="second-order"):
        b.iterate(mtf_amd.sm_desc(L.SM_ESM, sec_ord_hess=1))
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="LRSCV candidates"):
        b.score_candidates(np.zeros((4, 8)))
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="LRSCV is not available on the NN dataset"):
        b.nn_dataset(4, np.full(8, 0.01))
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="LRSCV is not available on the grid tracker"):
        b.grid_update(G[tag + "_corners"][None], sm)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="updateModel :: LRSCV"):
        b.update_model()
    lib = L.lib()
    pf = ctypes.c_void_p()
    desc = ctypes.create_string_buffer(4096)
    assert lib.mtfhip_pf_create(b._h, ctypes.addressof(desc), ctypes.addressof(pf)) == -2
    assert "LRSCV is not available on the particle filter" in lib.mtfhip_last_error().decode()
    b.close()
    b = fresh()
    b.set_lrscv(3, 3, 10, 10, 0, 1, 0)
    b.init_template(sm)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="LRSCV once_per_frame with Levenberg-Marquardt"):
        b.track(mtf_amd.sm_desc(L.SM_FCLK, leven_marq=1))
    b.close()
    b = fresh(100, 100, 256)   # 9 x 9 sub-regions: 289 cells x 256 bins x 8 B of pass-1 table
    b.set_lrscv(9, 9, 5, 5, 0, 0, 0)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="LDS"):
        b.init_template(sm)
    b.close()
    b = fresh(100, 100, 256)   # 6 x 6 sub-regions at spacing 0: one cell, but 36 maps x 256 bins x 8 B in the fused pass's LDS
    b.set_lrscv(6, 6, 0, 0, 0, 0, 0)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="LDS"):
        b.init_template(sm)
    b.close()
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="n_channels 3"):
        mtf_amd.Batch(gpu_ctx, L.AM_LRSCV, L.SSM_HOMOGRAPHY, 50, 50, 1, mi_n_bins=64, n_channels=3)
    with pytest.raises(mtf_amd.InvalidArgument, match="n_bins"):
        mtf_amd.Batch(gpu_ctx, L.AM_LRSCV, L.SSM_HOMOGRAPHY, 50, 50, 1, mi_n_bins=257)


@pytest.mark.parametrize("once,affine", [(1, 1), (0, 0)])
def test_lrscv_cpp_harness_matches_python(gpu_ctx, once, affine):
    """HipAM("lrscv") built from its LRSCVParams through the harness: under mtf::hip::LK (the device loop) the same corners as
    Batch.track bit for bit; under nt::ESM (the reference's loop over the AM / SSM virtuals, setFirstIter / clearFirstIter included)
    within 1e-6 px"""
    from mtf_amd import host
    import test_gpu_rscv
    f0, f1, c0, _ = test_gpu_rscv.gamma_pair()
    kw = dict(max_iters=10, epsilon=1e-6, leven_marq=0)
    gpu_ctx.set_image(f0)
    b = mtf_amd.Batch(gpu_ctx, L.AM_LRSCV, L.SSM_HOMOGRAPHY, 50, 50, 1, mi_n_bins=64)
    b.set_lrscv(3, 3, 10, 10, affine, once, 0)
    sm = mtf_amd.sm_desc(L.SM_ESM, materialize=0, **kw)
    b.set_corners(c0[None])
    b.init_template(sm)
    gpu_ctx.set_image(f1)
    _, corners = b.track(sm)
    b.close()
    for device_loop in (True, False):
        t = host.CppTracker.lrscv(L.SM_ESM, L.SSM_HOMOGRAPHY, 50, 50, n_bins=64, affine_mapping=affine, once_per_frame=once,
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
