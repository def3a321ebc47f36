"""The HIP MI paths at the shipped configuration (10 bins, partition of unity) and at 10 / 9 / 5 bins against the independent NumPy
definitions directly (tests/golden/lk_golden5.npz, generator tests/golden/make_golden5.py; the C++ oracle is held to the same fixture
by tests/test_oracle_golden5.py): the interface entry points, the fused recompute passes that Batch.iterate and the device loop run
(k_mi_pass_hist / k_mi_pass_grad_hess <.., NB = 10>: ten-class sort, ragged tiles, the moment tables), several targets in one batch,
the candidate scorer -- and the run-to-run reproducibility of the fused passes.

Tolerances are test_gpu_golden.py's MI ones: f 1e-10 relative, df/dIt rtol 1e-8, g and H 1e-5 relative."""
import os

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lk_golden5.npz"))
TAGS = [str(t) for t in G["tags"]]
MATHS = [mtf_amd.MATH_REPLAY, mtf_amd.MATH_FAST]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def cfg(tag):
    nb, pou, resx, resy, aff = (int(v) for v in G[tag + "_cfg"])
    return nb, pou, resx, resy, bool(aff)


def mi_batch(ctx, tags):
    """one batch whose targets are the given fixture cases (same bin count, pou, patch and SSM)"""
    nb, pou, resx, resy, aff = cfg(tags[0])
    assert all(cfg(t) == cfg(tags[0]) for t in tags)
    ctx.set_image(G["img"])
    b = mtf_amd.Batch(ctx, L.AM_MI, L.SSM_AFFINE if aff else L.SSM_HOMOGRAPHY, resx, resy, len(tags), mi_n_bins=nb, mi_pou=pou)
    b.set_corners(np.stack([G[t + "_corners"] for t in tags]))
    return b


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("tag", TAGS)
def test_mi_golden5_interface(gpu_ctx, tag, math):
    """the per-function entry points (as test_gpu_golden.py::test_mi_golden): f, df/dIt, df_dIt . Jt and the current, init and self
    Hessians at the fixture state"""
    b = mi_batch(gpu_ctx, [tag])
    b.set_math_mode(math)
    b.initialize_pix_vals(); b.initialize_pix_grad(); b.initialize_similarity(); b.initialize_grad(); b.initialize_hess()
    np.testing.assert_allclose(b.read(L.BUF_I0)[0][:16], G[tag + "_I0n_head"], rtol=0, atol=1e-9)
    b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DI0_DX, L.BUF_J0)
    b.set_state(G[tag + "_p"][None])
    b.update_pix_vals(); b.update_similarity(False); b.update_curr_grad(); b.update_init_grad(); b.update_pix_grad()
    np.testing.assert_allclose(b.read(L.BUF_IT)[0][:16], G[tag + "_Itn_head"], rtol=0, atol=1e-9)
    f = float(G[tag + "_f"])
    assert abs(b.get_similarity()[0] - f) <= 1e-10 * abs(f)
    np.testing.assert_allclose(b.read(L.BUF_DF_DIT)[0][:16], G[tag + "_df_dIt_head"], rtol=1e-8, atol=1e-14)
    b.cmpt_warped_pix_jacobian()
    assert rel(b.cmpt_curr_jacobian()[0], G[tag + "_g_curr"]) < 1e-5
    assert rel(b.cmpt_curr_hessian()[0], G[tag + "_H_curr"]) < 1e-5
    assert rel(b.cmpt_init_hessian()[0], G[tag + "_H_init"]) < 1e-5
    assert rel(b.cmpt_self_hessian()[0], G[tag + "_H_self1"]) < 1e-5
    b.close()


def fused_check(b, tags, hk, math):
    """Batch.iterate from the fixture states (what _fused_follow and the device loop run): FCLK with the constant Hessian (HK = 0:
    init_template's cmptSelfHessian(J0) = H_init0) or the current self Hessian (HK = 1: the sorted pass, H_self1)"""
    b.set_math_mode(math)
    sm = mtf_amd.sm_desc(L.SM_FCLK, hess_type=hk, materialize=0, leven_marq=0)
    b.init_template(sm)
    b.set_state(np.stack([G[t + "_p"] for t in tags]))
    f, g, H = b.iterate(sm)
    for k, t in enumerate(tags):
        ft = float(G[t + "_f"])
        assert abs(f[k] - ft) <= 1e-10 * abs(ft), (t, f[k], ft)
        assert rel(g[k], G[t + "_g_curr"]) < 1e-5, (t, rel(g[k], G[t + "_g_curr"]))
        Href = G[t + ("_H_init0" if hk == 0 else "_H_self1")]
        assert rel(H[k], Href) < 1e-5, (t, rel(H[k], Href))


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("hk", [0, 1])
@pytest.mark.parametrize("tag", TAGS)
def test_mi_golden5_fused(gpu_ctx, tag, hk, math):
    b = mi_batch(gpu_ctx, [tag])
    fused_check(b, [tag], hk, math)
    b.close()


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("hk", [0, 1])
def test_mi_golden5_fused_one_batch(gpu_ctx, hk, math):
    """the three 10-bin + pou 40 x 40 cases (saturated, ramp, texture) as the targets of ONE batch, in two orders: per-target indexing
    of the passes (blockIdx.y, the tables and polynomial rows of each target)"""
    tags = [t for t in TAGS if cfg(t) == cfg("b10p_sat")]
    assert len(tags) >= 3
    for order in (tags, tags[::-1]):
        b = mi_batch(gpu_ctx, order)
        fused_check(b, order, hk, math)
        b.close()


@pytest.mark.parametrize("math", MATHS)
def test_mi_golden5_candidates(gpu_ctx, math):
    """the candidate scorer at 10 bins + pou (k_mi_pass_hist<.., CAND, NB = 10>): the similarity of the fixture state among others"""
    tag = "b10p_sat"
    b = mi_batch(gpu_ctx, [tag])
    b.set_math_mode(math)
    b.initialize_pix_vals(); b.initialize_similarity()
    rng = np.random.default_rng(5)
    states = np.vstack([synth.pf_candidate_states(rng, 5), G[tag + "_p"][None], np.zeros((1, 8)), synth.pf_candidate_states(rng, 4)])
    lik, sim = b.score_candidates(states, want_similarity=True)
    f = float(G[tag + "_f"])
    assert abs(sim[5] - f) <= 1e-8 * abs(f), (sim[5], f)
    # the template scored against itself is the largest MI of the set
    assert np.argmax(sim) == 6
    b.close()


@pytest.mark.parametrize("n_bins,pou", [(10, 1), (8, 0)])
def test_mi_fused_reproducible(gpu_ctx, frame, n_bins, pou):
    """Run to run on one device the fused MI passes give the same bits (the comment at api_mi_iter.hip's mi_enqueue_fast):
    the self-Hessian plan (HK = 1, the sorted pass with its moment tables), 8 targets of 200 x 200, ten Batch.iterate from one state in
    MATH_FAST, and two device-side Batch.track from one set of corners.  8 bins is the control."""
    rng = np.random.default_rng(91)
    B, res = 8, 200
    gpu_ctx.set_image(frame)
    corners = np.stack([synth.square_corners(130.0 + 80 * (k % 4), 150.0 + 170 * (k // 4), 230) + 0.1 * k for k in range(B)])
    b = mtf_amd.Batch(gpu_ctx, L.AM_MI, L.SSM_HOMOGRAPHY, res, res, B, mi_n_bins=n_bins, mi_pou=pou)
    b.set_math_mode(mtf_amd.MATH_FAST)
    sm = mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, materialize=0, leven_marq=0, max_iters=6, epsilon=1e-6)
    b.set_corners(corners)
    b.init_template(sm)
    states = np.stack([synth.random_small_homography(rng, 0.3) for _ in range(B)])
    ref = None
    for _ in range(10):
        b.set_state(states)
        out = b.iterate(sm)
        if ref is None:
            ref = out
            assert np.all(np.isfinite(out[2])) and np.all(out[0] > 0)
        else:
            for a, r in zip(out, ref):
                assert np.array_equal(a, r)
    frame2 = synth.warp_frame(frame, synth.random_small_homography(rng, 0.4), (256.0, 256.0))
    runs = []
    for _ in range(2):
        gpu_ctx.set_image(frame)
        b.set_corners(corners)
        b.init_template(sm)
        gpu_ctx.set_image(frame2)
        runs.append(b.track(sm))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert np.all(runs[0][0] >= 1)
    b.close()
