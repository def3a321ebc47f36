"""The HIP SCV path (am = MTFHIP_AM_SCV: SSD on the template re-mapped through E[It | I0_orig] before every similarity update) against
the independent float64 definitions of tests/golden/make_golden6.py (fixture lk_golden6.npz), in both math modes:

- the intensity map (bit for bit with Dirac histograms, 1e-12 with Bilinear ones), the re-mapped I0, f and df/dIt (the MI golden
  tolerances: f 1e-10 relative, df/dIt 1e-8), g and H (1e-5 relative) -- through the per-function entry points, Batch.iterate,
  batches of 64, 256 and 7 bins side by side (n_bins, like hist_type and weighted_mapping, is a property of the batch) and six
  targets in one batch of the device loop;
- the state update and the corners after 5 ESM / FCLK iterations of Batch.track (1e-6 px);
- a tracking behaviour test under a monotone intensity change that defeats SSD, run-to-run reproducibility of the fused passes, the
  refused configurations, and the C++ HipAM("scv") path through the harness (mtf::hip::LK bit for bit, nt::ESM within 1e-6 px)."""
import ctypes
import os

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "lk_golden6.npz"))
TAGS = [str(t) for t in G["tags"]]
TRACK_TAGS = [t for t in TAGS if t + "_esm_dp" in G]
MATHS = [mtf_amd.MATH_REPLAY, mtf_amd.MATH_FAST]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def cfg(tag):
    ht, nb, lin, resx, resy, aff = (int(v) for v in G[tag + "_cfg"])
    return ht, nb, lin, resx, resy, bool(aff)


def scv_batch(ctx, tags, math):
    ht, nb, lin, resx, resy, aff = cfg(tags[0])
    assert all(cfg(t)[3:] == cfg(tags[0])[3:] for t in tags)
    ctx.set_image(G["img"])
    b = mtf_amd.Batch(ctx, L.AM_SCV, L.SSM_AFFINE if aff else L.SSM_HOMOGRAPHY, resx, resy, len(tags), mi_n_bins=nb)
    b.set_scv(ht, lin, 0)
    b.set_math_mode(math)
    b.set_corners(np.stack([G[t + "_corners"] for t in tags]))
    return b


def check_map(m, tag):
    ref = G[tag + "_map"]
    if cfg(tag)[0] == 0:
        np.testing.assert_array_equal(m, ref)
    else:
        np.testing.assert_allclose(m, ref, rtol=1e-12, atol=1e-12)


def check_template(b, k, tag):
    """the re-mapped I0 (BUF_I0)"""
    I0 = b.read(L.BUF_I0)[k]
    np.testing.assert_allclose(I0[:16], G[tag + "_I0_head"], rtol=0, atol=1e-9)
    if tag + "_I0" in G:
        np.testing.assert_allclose(I0, G[tag + "_I0"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("tag", TAGS)
def test_scv_golden6_interface(gpu_ctx, tag, math):
    b = scv_batch(gpu_ctx, [tag], math)
    b.initialize_pix_vals(); b.initialize_pix_grad(); b.initialize_similarity(); b.initialize_grad(); b.initialize_hess()
    nb = cfg(tag)[1]
    np.testing.assert_array_equal(b.scv_intensity_map()[0], np.arange(nb, dtype=np.float64))
    b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DI0_DX, L.BUF_J0)
    b.set_state(G[tag + "_p"][None])
    b.update_pix_vals(); b.update_similarity(False); b.update_curr_grad(); b.update_init_grad(); b.update_pix_grad()
    check_map(b.scv_intensity_map()[0], tag)
    check_template(b, 0, tag)
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
    """Batch.iterate (FCLK, CurrentSelf) from the fixture states: the fused SSD pass on the re-mapped template"""
    sm = mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, materialize=materialize, leven_marq=0)
    b.init_template(sm)
    b.set_state(np.stack([G[t + "_p"] for t in tags]))
    f, g, H = b.iterate(sm)
    maps = b.scv_intensity_map()
    for k, t in enumerate(tags):
        check_map(maps[k][:cfg(t)[1]], t)
        check_template(b, k, t)
        ft = float(G[t + "_f"])
        assert abs(f[k] - ft) <= 1e-10 * abs(ft), (t, f[k], ft)
        assert rel(g[k], G[t + "_g"]) < 1e-5, (t, rel(g[k], G[t + "_g"]))
        assert rel(H[k], G[t + "_H_self"]) < 1e-5, (t, rel(H[k], G[t + "_H_self"]))


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("materialize", [0, 1])
@pytest.mark.parametrize("tag", TAGS)
def test_scv_golden6_fused(gpu_ctx, tag, materialize, math):
    b = scv_batch(gpu_ctx, [tag], math)
    fused_check(b, [tag], materialize)
    b.close()


@pytest.mark.parametrize("math", MATHS)
def test_scv_different_bin_counts_in_one_call_sequence(gpu_ctx, math):
    """batches of 64, 256 and 7 bins side by side on one context, each iterated in turn: no state leaks between them"""
    tags = ["d64n_50", "d256n_60", "d7n_37x23"]
    bs = [scv_batch(gpu_ctx, [t], math) for t in tags]
    sms = [mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, materialize=0, leven_marq=0) for _ in tags]
    for b, t, sm in zip(bs, tags, sms):
        b.init_template(sm)
        b.set_state(G[t + "_p"][None])
    for b, t, sm in zip(bs, tags, sms):
        f, g, H = b.iterate(sm)
        check_map(b.scv_intensity_map()[0], t)
        assert abs(f[0] - float(G[t + "_f"])) <= 1e-10 * abs(float(G[t + "_f"]))
        assert rel(g[0], G[t + "_g"]) < 1e-5
    for b in bs:
        b.close()


def track_sm(method, materialize=0):
    if method == "esm":
        return mtf_amd.sm_desc(L.SM_ESM, jac_type=1, hess_type=2, max_iters=5, epsilon=0.0, materialize=materialize, leven_marq=0)
    return mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, max_iters=5, epsilon=0.0, materialize=materialize, leven_marq=0)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("method", ["esm", "fclk"])
@pytest.mark.parametrize("tag", TRACK_TAGS)
def test_scv_golden6_track(gpu_ctx, tag, method, math):
    """5 iterations of the device loop from the fixture state: the last state update (debug trace) and the corners"""
    b = scv_batch(gpu_ctx, [tag], math)
    sm = track_sm(method)
    b.init_template(sm)
    b.set_state(G[tag + "_p"][None])
    b.track_trace(5)
    n, corners = b.track(sm)
    assert int(n[0]) == 5
    recs = b.read_track_trace(n)[0]
    np.testing.assert_allclose(recs[-1]["dp"], G[tag + "_" + method + "_dp"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(corners[0], G[tag + "_" + method + "_corners"], rtol=0, atol=1e-6)
    b.track_trace(0)
    b.close()


@pytest.mark.parametrize("math", MATHS)
def test_scv_track_many_targets_matches_single(gpu_ctx, math):
    """the chunked / two-queue device loop (no trace) on 6 copies of the 200 x 200 case: every target lands on the fixture's corners"""
    tag = "d64n_200"
    tags = [tag] * 6
    b = scv_batch(gpu_ctx, tags, math)
    for method in ("esm", "fclk"):
        sm = track_sm(method, materialize=1 if method == "esm" else 0)
        b.set_corners(np.stack([G[t + "_corners"] for t in tags]))   # (init_template samples the template at the current warp)
        b.init_template(sm)
        b.set_state(np.stack([G[t + "_p"] for t in tags]))
        n, corners = b.track(sm)
        for k in range(len(tags)):
            np.testing.assert_allclose(corners[k], G[tag + "_" + method + "_corners"], rtol=0, atol=1e-6)
    b.close()


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


@pytest.mark.parametrize("math", MATHS)
def test_scv_tracks_through_intensity_change_ssd_does_not(gpu_ctx, math):
    """ESM over a known homography plus a gamma-0.6 intensity curve, 64 bins: SCV recovers the corners, SSD does not.  Bilinear
    histograms (either mapping) land within 0.1 px.  Dirac histograms converge within 0.25 px: the map is the mean of (int)It over a
    template bin, half a bin below the mean of It, and that offset biases the SSD step on the re-mapped template (the reference's
    definition, not a device effect)."""
    f0, f1, c0, ct = gamma_pair()
    err = {}
    for key, am, ht, lin in (("ssd", L.AM_SSD, 0, 0), ("dirac", L.AM_SCV, 0, 0), ("bilinear", L.AM_SCV, 1, 0), ("bilinear_linear", L.AM_SCV, 1, 1)):
        gpu_ctx.set_image(f0)
        b = mtf_amd.Batch(gpu_ctx, am, L.SSM_HOMOGRAPHY, 100, 100, 1, mi_n_bins=64)
        if am == L.AM_SCV:
            b.set_scv(ht, lin, 0)
        b.set_math_mode(math)
        sm = mtf_amd.sm_desc(L.SM_ESM, max_iters=30, epsilon=1e-6, leven_marq=0)
        b.set_corners(c0[None])
        b.init_template(sm)
        gpu_ctx.set_image(f1)
        _, corners = b.track(sm)
        err[key] = float(np.abs(corners[0] - ct).max())
        b.close()
    assert err["bilinear"] <= 0.1 and err["bilinear_linear"] <= 0.1, err
    assert err["dirac"] <= 0.25, err
    assert err["ssd"] > 0.1 and err["ssd"] > 20 * max(err["dirac"], err["bilinear"]), err


@pytest.mark.parametrize("ht", [0, 1])
def test_scv_reproducible(gpu_ctx, ht):
    """ten iterate calls and two track calls, 8 targets of 200 x 200: identical bits (pass 1 sums in a fixed order)"""
    tag = "d64n_200"
    gpu_ctx.set_image(G["img"])
    B = 8
    b = mtf_amd.Batch(gpu_ctx, L.AM_SCV, L.SSM_HOMOGRAPHY, 200, 200, B, mi_n_bins=64)
    b.set_scv(ht, 0, 0)
    rng = np.random.default_rng(5)
    cs = np.stack([G[tag + "_corners"] + rng.uniform(-3, 3, (1, 1)) for _ in range(B)])
    ps = np.stack([synth.random_small_homography(rng, 0.4) for _ in range(B)])
    b.set_corners(cs)
    sm = mtf_amd.sm_desc(L.SM_ESM, materialize=0, leven_marq=0)
    b.init_template(sm)
    first = None
    for _ in range(10):
        b.set_state(ps)
        f, g, H = b.iterate(sm)
        cur = (f.copy(), g.copy(), H.copy(), b.scv_intensity_map().copy(), b.read(L.BUF_I0).copy())
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
        runs.append((corners.copy(), b.scv_intensity_map().copy()))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    b.close()


def test_scv_refusals(gpu_ctx):
    gpu_ctx.set_image(G["img"])
    tag = "d64n_50"

    def fresh():
        b = mtf_amd.Batch(gpu_ctx, L.AM_SCV, L.SSM_HOMOGRAPHY, 50, 50, 1, mi_n_bins=64)
        b.set_corners(G[tag + "_corners"][None])
        return b

    b = fresh()
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="BSpline"):
        b.set_scv(2, 0, 0)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="mapped_gradient"):
        b.set_scv(0, 0, 1)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="second-order"):
        b.init_template(mtf_amd.sm_desc(L.SM_ESM, sec_ord_hess=1))
    sm = mtf_amd.sm_desc(L.SM_ESM, leven_marq=0)
    b.init_template(sm)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="second-order"):
        b.iterate(mtf_amd.sm_desc(L.SM_ESM, sec_ord_hess=1))
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="SCVDist"):
        b.score_candidates(np.zeros((4, 8)))
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="SCVDist"):
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
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="MCSCV"):
        mtf_amd.Batch(gpu_ctx, L.AM_SCV, L.SSM_HOMOGRAPHY, 50, 50, 1, mi_n_bins=64, n_channels=3)


@pytest.mark.parametrize("ht,lin", [(0, 0), (1, 1)])
def test_scv_cpp_harness_matches_python(gpu_ctx, ht, lin):
    """HipAM("scv") built from its SCVParams through the harness: under mtf::hip::LK (the device loop) the same corners as Batch.track bit
    for bit; under nt::ESM (the reference's ESM loop over the AM / SSM virtuals: per-function entry points, host solve) within 1e-6 px"""
    from mtf_amd import host
    f0, f1, c0, _ = gamma_pair()
    kw = dict(max_iters=10, epsilon=1e-6, leven_marq=0)
    gpu_ctx.set_image(f0)
    b = mtf_amd.Batch(gpu_ctx, L.AM_SCV, L.SSM_HOMOGRAPHY, 50, 50, 1, mi_n_bins=64)
    b.set_scv(ht, lin, 0)   # (both sides in the default math mode)
    sm = mtf_amd.sm_desc(L.SM_ESM, materialize=0, **kw)   # (mtf::hip::LK's loop does not materialise)
    b.set_corners(c0[None])
    b.init_template(sm)
    gpu_ctx.set_image(f1)
    _, corners = b.track(sm)
    b.close()
    for device_loop in (True, False):
        t = host.CppTracker.scv(L.SM_ESM, L.SSM_HOMOGRAPHY, 50, 50, hist_type=ht, n_bins=64, weighted_mapping=lin, device_loop=device_loop, **kw)
        t.set_image(f0)
        t.initialize(c0)
        t.set_image(f1)
        t.update()
        cpp = np.asarray(t.get_region()).reshape(2, 4)
        if device_loop:
            np.testing.assert_array_equal(cpp, corners[0])
        else:
            np.testing.assert_allclose(cpp, corners[0], rtol=0, atol=1e-6)
