"""The HIP RSCV path (am = MTFHIP_AM_RSCV: SSD on the current patch mapped through E[I0 | It] after every sampling) against the
independent float64 definitions of tests/golden/make_golden7.py (fixture lk_golden7.npz), in both math modes:

- the intensity map (bit for bit: integer sums), the mapped It (1e-9), df/dIt (1e-8), f (1e-10 relative), g and H (1e-5 relative)
  through the per-function entry points and Batch.iterate (materialise 0 and 1), and batches of 64, 256 and 7 bins on one context;
- bin agreement: the It the fused pass materialises is map[rint(It_orig)] bit for bit, It_orig sampled by the per-function route;
- the state update and the corners after 5 ESM / FCLK / ICLK iterations of Batch.track (1e-6 px), and many targets in one batch land on
  the same bits as the same targets one at a time;
- a tracking behaviour test under a monotone intensity change that defeats SSD, run-to-run reproducibility, the refused configurations,
  and the C++ HipAM("rscv") path through the harness (mtf::hip::LK bit for bit, nt::ESM within 1e-6 px)."""
import ctypes
import os

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "lk_golden7.npz"))
TAGS = [str(t) for t in G["tags"]]
TRACK_TAGS = [t for t in TAGS if t + "_esm_dp" in G]
MATHS = [mtf_amd.MATH_REPLAY, mtf_amd.MATH_FAST]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def cfg(tag):
    nb, lin, resx, resy, aff = (int(v) for v in G[tag + "_cfg"])
    return nb, lin, resx, resy, bool(aff)


def rscv_batch(ctx, tags, math, am=L.AM_RSCV):
    nb, lin, resx, resy, aff = cfg(tags[0])
    assert all(cfg(t)[2:] == cfg(tags[0])[2:] for t in tags)
    ctx.set_image(G["img"])
    b = mtf_amd.Batch(ctx, am, L.SSM_AFFINE if aff else L.SSM_HOMOGRAPHY, resx, resy, len(tags), mi_n_bins=nb)
    if am == L.AM_RSCV:
        b.set_rscv(0, lin, 0)
    b.set_math_mode(math)
    b.set_corners(np.stack([G[t + "_corners"] for t in tags]))
    return b


def check_it(It, tag):
    """the mapped current patch (BUF_IT)"""
    np.testing.assert_allclose(It[:16], G[tag + "_It_head"], rtol=0, atol=1e-9)
    if tag + "_It" in G:
        np.testing.assert_allclose(It, G[tag + "_It"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("tag", TAGS)
def test_rscv_golden7_interface(gpu_ctx, tag, math):
    b = rscv_batch(gpu_ctx, [tag], math)
    b.initialize_pix_vals(); b.initialize_pix_grad(); b.initialize_similarity(); b.initialize_grad(); b.initialize_hess()
    nb = cfg(tag)[0]
    np.testing.assert_array_equal(b.rscv_intensity_map()[0], np.arange(nb, dtype=np.float64))
    b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DI0_DX, L.BUF_J0)
    b.set_state(G[tag + "_p"][None])
    b.update_pix_vals(); b.update_similarity(False); b.update_curr_grad(); b.update_init_grad(); b.update_pix_grad()
    np.testing.assert_array_equal(b.rscv_intensity_map()[0], G[tag + "_map"])
    check_it(b.read(L.BUF_IT)[0], tag)
    f = float(G[tag + "_f"])
    assert abs(b.get_similarity()[0] - f) <= 1e-10 * abs(f)
    dft = b.read(L.BUF_DF_DIT)[0]
    np.testing.assert_allclose(dft[:16], G[tag + "_df_dIt_head"], rtol=1e-8, atol=1e-12)
    if tag + "_df_dIt" in G:
        np.testing.assert_allclose(dft, G[tag + "_df_dIt"], rtol=1e-8, atol=1e-12)
    b.cmpt_warped_pix_jacobian()
    assert rel(b.cmpt_curr_jacobian()[0], G[tag + "_g"]) < 1e-5
    assert rel(b.cmpt_curr_hessian()[0], G[tag + "_H_curr"]) < 1e-5
    assert rel(b.cmpt_self_hessian()[0], G[tag + "_H_self"]) < 1e-5
    b.close()


def fused_check(b, tags, materialize):
    """Batch.iterate (FCLK, CurrentSelf) from the fixture states: the fused pass maps every sample through pass 1's map"""
    sm = mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, materialize=materialize, leven_marq=0)
    b.init_template(sm)
    b.set_state(np.stack([G[t + "_p"] for t in tags]))
    f, g, H = b.iterate(sm)
    maps = b.rscv_intensity_map()
    for k, t in enumerate(tags):
        np.testing.assert_array_equal(maps[k][:cfg(t)[0]], G[t + "_map"])
        if materialize:
            check_it(b.read(L.BUF_IT)[k], t)
        ft = float(G[t + "_f"])
        assert abs(f[k] - ft) <= 1e-10 * abs(ft), (t, f[k], ft)
        assert rel(g[k], G[t + "_g"]) < 1e-5, (t, rel(g[k], G[t + "_g"]))
        assert rel(H[k], G[t + "_H_self"]) < 1e-5, (t, rel(H[k], G[t + "_H_self"]))


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("materialize", [0, 1])
@pytest.mark.parametrize("tag", TAGS)
def test_rscv_golden7_fused(gpu_ctx, tag, materialize, math):
    b = rscv_batch(gpu_ctx, [tag], math)
    fused_check(b, [tag], materialize)
    b.close()


@pytest.mark.parametrize("tag", TAGS)
def test_rscv_fused_bins_agree_with_per_function_it_orig(gpu_ctx, tag):
    """replay, materialise 1: the It the fused pass writes is map[rint(It_orig)] (or the linear form) bit for bit, with It_orig sampled by
    the per-function route at the same state -- an SSD batch's updatePixVals, times RSCV's normalisation, which is the same rounding"""
    nb, lin, *_ = cfg(tag)
    b = rscv_batch(gpu_ctx, [tag], mtf_amd.MATH_REPLAY)
    sm = mtf_amd.sm_desc(L.SM_ESM, materialize=1, leven_marq=0)
    b.init_template(sm)
    b.set_state(G[tag + "_p"][None])
    b.iterate(sm)
    it_fused = b.read(L.BUF_IT)[0].copy()
    m = b.rscv_intensity_map()[0]
    s = rscv_batch(gpu_ctx, [tag], mtf_amd.MATH_REPLAY, am=L.AM_SSD)
    s.init_template(sm)
    s.set_state(G[tag + "_p"][None])
    s.update_pix_vals()
    it_orig = ((nb - 1.0) / 255.0) * s.read(L.BUF_IT)[0]
    s.close()
    if lin:
        lx = np.clip(it_orig.astype(np.int64), 0, nb - 1)
        dx = it_orig - it_orig.astype(np.int64)
        hi = np.minimum(lx + 1, nb - 1)
        want = np.where(dx == 0, m[lx], (1 - dx) * m[lx] + dx * m[hi])
    else:
        want = m[np.clip(np.rint(it_orig).astype(np.int64), 0, nb - 1)]
    np.testing.assert_array_equal(it_fused, want)
    # and the per-function route on the RSCV batch itself (pass 1 from its It_orig buffer) lands on the same map and the same It
    b.update_pix_vals()
    np.testing.assert_array_equal(b.rscv_intensity_map()[0], m)
    np.testing.assert_array_equal(b.read(L.BUF_IT)[0], it_fused)
    b.close()


@pytest.mark.parametrize("math", MATHS)
def test_rscv_different_bin_counts_on_one_context(gpu_ctx, math):
    """batches of 64, 256 and 7 bins side by side on one context, each iterated in turn: no state leaks between them"""
    tags = ["r64n_50", "r256n_60", "r7n_37x23"]
    bs = [rscv_batch(gpu_ctx, [t], math) for t in tags]
    sm = mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, materialize=0, leven_marq=0)
    for b, t in zip(bs, tags):
        b.init_template(sm)
        b.set_state(G[t + "_p"][None])
    for b, t in zip(bs, tags):
        f, g, H = b.iterate(sm)
        np.testing.assert_array_equal(b.rscv_intensity_map()[0], G[t + "_map"])
        assert abs(f[0] - float(G[t + "_f"])) <= 1e-10 * abs(float(G[t + "_f"]))
        assert rel(g[0], G[t + "_g"]) < 1e-5
    for b in bs:
        b.close()


def track_sm(method, materialize=0):
    if method == "esm":
        return mtf_amd.sm_desc(L.SM_ESM, jac_type=1, hess_type=2, max_iters=5, epsilon=0.0, materialize=materialize, leven_marq=0)
    if method == "fclk":
        return mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, max_iters=5, epsilon=0.0, materialize=materialize, leven_marq=0)
    return mtf_amd.sm_desc(L.SM_ICLK, hess_type=0, max_iters=5, epsilon=0.0, materialize=materialize, leven_marq=0)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("method", ["esm", "fclk", "iclk"])
@pytest.mark.parametrize("tag", TRACK_TAGS)
def test_rscv_golden7_track(gpu_ctx, tag, method, math):
    """5 iterations of the device loop from the fixture state: the last state update (debug trace; ESM / FCLK) and the corners"""
    b = rscv_batch(gpu_ctx, [tag], math)
    sm = track_sm(method)
    b.init_template(sm)
    b.set_state(G[tag + "_p"][None])
    b.track_trace(5)
    n, corners = b.track(sm)
    assert int(n[0]) == 5
    if method != "iclk":   # (ICLK's trace holds the step before its inversion as the device applies it; the corners pin the update)
        recs = b.read_track_trace(n)[0]
        np.testing.assert_allclose(recs[-1]["dp"], G[tag + "_" + method + "_dp"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(corners[0], G[tag + "_" + method + "_corners"], rtol=0, atol=1e-6)
    b.track_trace(0)
    b.close()


@pytest.mark.parametrize("math", MATHS)
def test_rscv_track_many_targets_same_bits_as_one_at_a_time(gpu_ctx, math):
    """six targets of 200 x 200 at different states in one batch (the chunked / two-queue device loop, pass 1 per chunk) give the bits
    each gives alone, and the unperturbed one lands on the fixture's corners"""
    tag = "r64n_200"
    rng = np.random.default_rng(9)
    ps = [G[tag + "_p"]] + [G[tag + "_p"] + rng.uniform(-1, 1, 8) * [2e-3, 2e-3, 0.3, 2e-3, 2e-3, 0.3, 1e-6, 1e-6] for _ in range(5)]
    for method in ("esm", "fclk", "iclk"):
        sm = track_sm(method, materialize=1 if method == "esm" else 0)
        b = rscv_batch(gpu_ctx, [tag] * 6, math)
        b.init_template(sm)
        b.set_state(np.stack(ps))
        _, many = b.track(sm)
        b.close()
        np.testing.assert_allclose(many[0], G[tag + "_" + method + "_corners"], rtol=0, atol=1e-6)
        for k in range(6):
            b1 = rscv_batch(gpu_ctx, [tag], math)
            b1.init_template(sm)
            b1.set_state(ps[k][None])
            _, one = b1.track(sm)
            b1.close()
            np.testing.assert_array_equal(many[k], one[0])


def gamma_pair(shape=(256, 256)):
    """frame 1 = frame 0 warped by a known homography, then through a monotone non-linear curve (gamma 0.6, gain and offset)"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import numpy_ref as R
    f0 = synth.make_frame(*shape, seed=11).astype(np.float64)
    Wt = np.array([[1.0, -0.02, 3.2], [0.025, 1.0, -2.6], [0.0, 0.0, 1.0]])
    yy, xx = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    q = np.linalg.inv(Wt) @ np.vstack([xx.ravel(), yy.ravel(), np.ones(xx.size)])
    src = R.bilinear(f0, q[0] / q[2], q[1] / q[2]).reshape(shape)
    f1 = 20.0 + 0.85 * 255.0 * (np.clip(src, 0, 255) / 255.0) ** 0.6
    c0 = synth.square_corners(128, 128, 100)
    ct = Wt @ np.vstack([c0, np.ones(4)])
    return f0.astype(np.float32), np.clip(f1, 0, 255).astype(np.float32), c0, ct[:2] / ct[2]


def gamma_errors(ctx, math):
    f0, f1, c0, ct = gamma_pair()
    err = {}
    for key, am, lin in (("ssd", L.AM_SSD, 0), ("nearest", L.AM_RSCV, 0), ("linear", L.AM_RSCV, 1)):
        ctx.set_image(f0)
        b = mtf_amd.Batch(ctx, am, L.SSM_HOMOGRAPHY, 100, 100, 1, mi_n_bins=64)
        if am == L.AM_RSCV:
            b.set_rscv(0, lin, 0)
        b.set_math_mode(math)
        sm = mtf_amd.sm_desc(L.SM_ESM, max_iters=30, epsilon=1e-6, leven_marq=0)
        b.set_corners(c0[None])
        b.init_template(sm)
        ctx.set_image(f1)
        _, corners = b.track(sm)
        err[key] = float(np.abs(corners[0] - ct).max())
        b.close()
    return err


@pytest.mark.parametrize("math", MATHS)
def test_rscv_tracks_through_intensity_change_ssd_does_not(gpu_ctx, math):
    """ESM over a known homography plus a gamma-0.6 intensity curve, 64 bins: RSCV, which maps the current patch back onto the template's
    intensities, recovers the corners; SSD does not"""
    err = gamma_errors(gpu_ctx, math)
    print("corner errors (px):", err)
    assert err["nearest"] <= RSCV_GAMMA_TOL and err["linear"] <= RSCV_GAMMA_TOL, err
    assert err["ssd"] > 1.0 and err["ssd"] > 20 * max(err["nearest"], err["linear"]), err


RSCV_GAMMA_TOL = 0.25


def test_rscv_reproducible(gpu_ctx):
    """ten iterate calls and two track calls, 8 targets of 200 x 200: identical bits (pass 1's sums are integers)"""
    tag = "r64n_200"
    gpu_ctx.set_image(G["img"])
    B = 8
    b = mtf_amd.Batch(gpu_ctx, L.AM_RSCV, L.SSM_HOMOGRAPHY, 200, 200, B, mi_n_bins=64)
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
            f, g, H = b.iterate(sm)
            cur = (f.copy(), g.copy(), H.copy(), b.rscv_intensity_map().copy()) + ((b.read(L.BUF_IT).copy(),) if mat else ())
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
        runs.append((corners.copy(), b.rscv_intensity_map().copy()))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    b.close()


def test_rscv_refusals(gpu_ctx):
    gpu_ctx.set_image(G["img"])
    tag = "r64n_50"

    def fresh():
        b = mtf_amd.Batch(gpu_ctx, L.AM_RSCV, L.SSM_HOMOGRAPHY, 50, 50, 1, mi_n_bins=64)
        b.set_corners(G[tag + "_corners"][None])
        return b

    b = fresh()
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="use_bspl"):
        b.set_rscv(1, 0, 0)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="mapped_gradient"):
        b.set_rscv(0, 0, 1)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="second-order"):
        b.init_template(mtf_amd.sm_desc(L.SM_ESM, sec_ord_hess=1))
    sm = mtf_amd.sm_desc(L.SM_ESM, leven_marq=0)
    b.init_template(sm)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="second-order"):
        b.iterate(mtf_amd.sm_desc(L.SM_ESM, sec_ord_hess=1))
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="RSCVDist"):
        b.score_candidates(np.zeros((4, 8)))
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="RSCVDist"):
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
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="MCRSCV"):
        mtf_amd.Batch(gpu_ctx, L.AM_RSCV, L.SSM_HOMOGRAPHY, 50, 50, 1, mi_n_bins=64, n_channels=3)
    with pytest.raises(mtf_amd.InvalidArgument, match="n_bins"):
        mtf_amd.Batch(gpu_ctx, L.AM_RSCV, L.SSM_HOMOGRAPHY, 50, 50, 1, mi_n_bins=257)


@pytest.mark.parametrize("lin", [0, 1])
def test_rscv_cpp_harness_matches_python(gpu_ctx, lin):
    """HipAM("rscv") built from its RSCVParams through the harness: under mtf::hip::LK (the device loop) the same corners as Batch.track bit
    for bit; under nt::ESM (the reference's ESM loop over the AM / SSM virtuals: per-function entry points, host solve) within 1e-6 px"""
    from mtf_amd import host
    f0, f1, c0, _ = gamma_pair()
    kw = dict(max_iters=10, epsilon=1e-6, leven_marq=0)
    gpu_ctx.set_image(f0)
    b = mtf_amd.Batch(gpu_ctx, L.AM_RSCV, L.SSM_HOMOGRAPHY, 50, 50, 1, mi_n_bins=64)
    b.set_rscv(0, lin, 0)   # (both sides in the default math mode)
    sm = mtf_amd.sm_desc(L.SM_ESM, materialize=0, **kw)   # (mtf::hip::LK's loop does not materialise)
    b.set_corners(c0[None])
    b.init_template(sm)
    gpu_ctx.set_image(f1)
    _, corners = b.track(sm)
    b.close()
    for device_loop in (True, False):
        t = host.CppTracker.rscv(L.SM_ESM, L.SSM_HOMOGRAPHY, 50, 50, n_bins=64, weighted_mapping=lin, device_loop=device_loop, **kw)
        t.set_image(f0)
        t.initialize(c0)
        t.set_image(f1)
        t.update()
        cpp = np.asarray(t.get_region()).reshape(2, 4)
        if device_loop:
            np.testing.assert_array_equal(cpp, corners[0])
        else:
            np.testing.assert_allclose(cpp, corners[0], rtol=0, atol=1e-6)
