"""The SCV family's HIP kernels (SCV Dirac and Bilinear, RSCV, LSCV, LRSCV) across their seams, against the float64 restatements of
tests/golden/make_golden6.py .. make_golden9.py evaluated on the spot at the cases of tests/test_scv_seams_cpu.py (which holds the
restatements' two forms to each other and asserts the conditions on the inputs): patches below a wave and a chunk, on and past the
pass-1 workgroup count boundaries and past its cap, every bin-slot count of the Bilinear path, patches across and beyond the frame
edge, batches on and off the targets-per-launch chunk with targets that stop at different iterations, and the sub-region
decompositions of the localized models up to the LDS budget.

Tolerances (the project's): Dirac maps bit for bit, Bilinear maps 1e-12, the re-mapped I0 / mapped It 1e-9 absolute, f 1e-10 relative,
df/dIt rtol 1e-8, g and H 1e-5 relative, corners after 5 iterations 1e-6 px.  Every check runs in both math modes, through
Batch.iterate with materialise 0 and 1, and through the per-function chain (from_it for SCV / LSCV, the It_orig buffer and the apply
kernels for RSCV / LRSCV).

The bin-count cases sit on the texture, off the saturated blocks.  Across the edge of such a block (250 grey levels in one pixel) a sample
moves by 1e-12 when its coordinate moves by one unit in the last place, as it does between two correct float64 evaluations of the grid;
at 65 bins on the fixtures' 50 x 50 region one Bilinear bin rests on a weight of 0.0185 beside the zero block and its map entry then
moves by 5e-12 -- measured on the device: 4.87e-12, the device's template samples 3.3e-13 from the restatement's, the map of the
device's own samples within 2e-13 of the kernel's.  tests/test_scv_seams_cpu.py asserts that no case is conditioned like that."""
import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L

import test_scv_seams_cpu as T

pytestmark = pytest.mark.gpu
MATHS = [mtf_amd.MATH_REPLAY, mtf_amd.MATH_FAST]
AM = {"scv_d": L.AM_SCV, "scv_b": L.AM_SCV, "rscv": L.AM_RSCV, "lscv": L.AM_LSCV, "lrscv": L.AM_LRSCV}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def make_batch(ctx, c, model, math, corners=None, once=0):
    ctx.set_image(T.IMG)
    corners = c.corners[None] if corners is None else corners
    b = mtf_amd.Batch(ctx, AM[model], L.SSM_AFFINE if c.affine else L.SSM_HOMOGRAPHY, c.resx, c.resy, len(corners), mi_n_bins=c.nb)
    if model in ("scv_d", "scv_b"):
        b.set_scv(1 if model == "scv_b" else 0, T.model_linear(c, model), 0)
    elif model == "rscv":
        b.set_rscv(0, T.model_linear(c, model), 0)
    else:
        (b.set_lscv if model == "lscv" else b.set_lrscv)(c.geo[0], c.geo[1], c.geo[2], c.geo[3], int(c.mapping == 2), once, int(c.mapping == 1))
    b.set_math_mode(math)
    b.set_corners(corners)
    return b


def read_maps(b, model):
    if model in ("scv_d", "scv_b"):
        return b.scv_intensity_map()
    if model == "rscv":
        return b.rscv_intensity_map()
    return b.lscv_intensity_maps() if model == "lscv" else b.lrscv_intensity_maps()


def check_maps(m, r, model):
    if model == "scv_b":
        np.testing.assert_allclose(m, r["maps"], rtol=1e-12, atol=1e-12)
    else:
        np.testing.assert_array_equal(m, r["maps"])


def check_template(I0, r, c, model):
    """the re-mapped I0: 1e-9; LSCV with nearest mapping bit for bit, as tests/test_gpu_lscv.py holds it (a function of the template's
    bins, the maps and the weights, summed idx outer, idy inner: any other order of the sub-regions rounds differently)"""
    np.testing.assert_allclose(I0, r["tmpl"], rtol=0, atol=1e-9)
    if model == "lscv" and c.mapping == 0:
        np.testing.assert_array_equal(I0, r["tmpl"])


def check_similarity(r, f, g, H):
    n, top = r["cur"].size, max(float(np.abs(r["cur"]).max()), 1.0)
    noise = 0.5 * n * (64 * np.finfo(np.float64).eps * top) ** 2
    if abs(r["f"]) <= noise:   # (the map returns the patch itself -- Bilinear histograms wholly outside the frame: f is a sum of squared roundings)
        assert abs(f) <= noise, (f, r["f"])
    else:
        assert abs(f - r["f"]) <= 1e-10 * abs(r["f"]), (f, r["f"])
    if not np.any(r["g"]) and not np.any(r["H"]):     # (wholly outside the frame: no gradient anywhere, exactly)
        assert not np.any(g) and not np.any(H)
        return
    assert rel(g, r["g"]) < 1e-5, rel(g, r["g"])
    assert rel(H, r["H"]) < 1e-5, rel(H, r["H"])


def check_iterate(ctx, c, model, r=None, materializes=(0, 1)):
    """Batch.iterate (FCLK, CurrentSelf) at the case's state: maps, the mapped image, f, g, H"""
    r = T.ref(c.id, model) if r is None else r
    for math in MATHS:
        for mat in materializes:
            b = make_batch(ctx, c, model, math)
            sm = mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, materialize=mat, leven_marq=0)
            b.init_template(sm)
            b.set_state(c.p[None])
            b.set_first_iter(True)
            f, g, H = b.iterate(sm)
            check_maps(read_maps(b, model)[0], r, model)
            if model in ("scv_d", "scv_b", "lscv"):
                check_template(b.read(L.BUF_I0)[0], r, c, model)
            elif mat:
                np.testing.assert_allclose(b.read(L.BUF_IT)[0], r["cur"], rtol=0, atol=1e-9)
            check_similarity(r, f[0], g[0], H[0])
            b.close()


def check_interface(ctx, c, model, r=None):
    """the per-function chain: update_pix_vals, update_similarity and the gradient / Hessian entry points"""
    r = T.ref(c.id, model) if r is None else r
    for math in MATHS:
        b = make_batch(ctx, c, model, math)
        b.initialize_pix_vals(); b.initialize_pix_grad(); b.initialize_similarity(); b.initialize_grad(); b.initialize_hess()
        b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DI0_DX, L.BUF_J0)
        b.set_state(c.p[None])
        b.set_first_iter(True)
        b.update_pix_vals(); b.update_similarity(False); b.update_curr_grad(); b.update_init_grad(); b.update_pix_grad()
        check_maps(read_maps(b, model)[0], r, model)
        check_template(b.read(L.BUF_I0)[0], r, c, model)
        np.testing.assert_allclose(b.read(L.BUF_IT)[0], r["cur"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(b.read(L.BUF_DF_DIT)[0], r["dft"], rtol=1e-8, atol=1e-12)
        b.cmpt_warped_pix_jacobian()
        check_similarity(r, b.get_similarity()[0], b.cmpt_curr_jacobian()[0], b.cmpt_curr_hessian()[0])
        b.close()


def track_sm(method, max_iters=5, epsilon=0.0, materialize=0):
    kw = dict(max_iters=max_iters, epsilon=epsilon, materialize=materialize, leven_marq=0)
    if method == "esm":
        return mtf_amd.sm_desc(L.SM_ESM, jac_type=1, hess_type=2, **kw)
    return mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, **kw)


SMALL = [(c, m) for c, m in T.PAIRS if T.BY_ID[c].group in ("pixels", "bins", "geo") or (T.BY_ID[c].group == "edge" and T.BY_ID[c].edge != "outside")]


@pytest.mark.parametrize("cid,model", SMALL)
def test_seam_iterate(gpu_ctx, cid, model):
    check_iterate(gpu_ctx, T.BY_ID[cid], model)


@pytest.mark.parametrize("cid,model", SMALL)
def test_seam_per_function_chain(gpu_ctx, cid, model):
    check_interface(gpu_ctx, T.BY_ID[cid], model)


@pytest.mark.parametrize("cid,model", [(c, m) for c, m in T.PAIRS if T.BY_ID[c].group == "cap"])
def test_past_the_workgroup_cap(gpu_ctx, cid, model):
    """more than 64 workgroups' worth of chunks per target: every workgroup's chunk loop takes more than its nominal share"""
    check_iterate(gpu_ctx, T.BY_ID[cid], model)


@pytest.mark.parametrize("method", ["esm", "fclk"])
@pytest.mark.parametrize("cid,model", [(c, m) for c, m in T.PAIRS if T.BY_ID[c].track])
def test_seam_track(gpu_ctx, cid, model, method):
    c = T.BY_ID[cid]
    _, dps, corners_ref, _ = T.ref_track(cid, model, method)
    for math in MATHS:
        b = make_batch(gpu_ctx, c, model, math)
        sm = track_sm(method)
        b.init_template(sm)
        b.set_state(c.p[None])
        b.track_trace(5)
        n, corners = b.track(sm)
        assert int(n[0]) == 5
        np.testing.assert_allclose(b.read_track_trace(n)[0][-1]["dp"], dps[-1], rtol=0, atol=1e-6)
        np.testing.assert_allclose(corners[0], corners_ref, rtol=0, atol=1e-6)
        b.track_trace(0)
        b.close()


@pytest.mark.parametrize("cid,model", [(c, m) for c, m in T.PAIRS if T.BY_ID[c].edge == "outside"])
def test_wholly_outside_the_frame(gpu_ctx, cid, model):
    """every sample is the border constant: the map and f are the reference's (f is not zero: nearest mapping puts the template at the
    bin index), g and H are exactly zero, and a 20-iteration track leaves the corners where they were"""
    c = T.BY_ID[cid]
    r = T.ref(cid, model)
    assert not np.any(r["g"]) and not np.any(r["H"])
    assert abs(r["f"]) > 1.0 or model == "scv_b"   # (Bilinear: the populated bins map the constant onto itself, f is rounding noise)
    assert (r["It_orig"] == 128.0 * T.G6.pix_mult(c.nb)).all()
    check_iterate(gpu_ctx, c, model)
    check_interface(gpu_ctx, c, model)
    for math in MATHS:
        for method in ("esm", "fclk"):
            b = make_batch(gpu_ctx, c, model, math)
            sm = track_sm(method, max_iters=20)
            b.init_template(sm)
            before = b.get_corners()
            np.testing.assert_allclose(before[0], c.corners, rtol=0, atol=1e-9)
            _, corners = b.track(sm)
            assert np.isfinite(corners).all()
            np.testing.assert_array_equal(corners, before)   # (g == 0 and H == 0: every step is exactly zero)
            b.close()


@pytest.mark.parametrize("model", ["rscv", "lrscv"])
@pytest.mark.parametrize("cid", [c.id for c in T.CASES if c.group == "edge" and c.edge != "outside"] + ["px_5x13", "px_6x43"])
def test_fused_bins_agree_with_per_function_it_orig_at_the_edge(gpu_ctx, cid, model):
    """replay, materialise 1, half outside the frame and with a ragged last wave: the It the fused pass writes is the map of It_orig bit
    for bit, It_orig sampled by the per-function route (an SSD batch's updatePixVals times the normalisation); the premise -- border
    and image samples in one wave, N % 64 != 0 -- is asserted in tests/test_scv_seams_cpu.py"""
    c = T.BY_ID[cid]
    assert (c.resx * c.resy) % 64 != 0
    b = make_batch(gpu_ctx, c, model, mtf_amd.MATH_REPLAY)
    sm = mtf_amd.sm_desc(L.SM_ESM, materialize=1, leven_marq=0)
    b.init_template(sm)
    b.set_state(c.p[None])
    b.set_first_iter(True)
    b.iterate(sm)
    it_fused = b.read(L.BUF_IT)[0].copy()
    maps = read_maps(b, model)[0]
    gpu_ctx.set_image(T.IMG)
    s = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_AFFINE if c.affine else L.SSM_HOMOGRAPHY, c.resx, c.resy, 1)
    s.set_math_mode(mtf_amd.MATH_REPLAY)
    s.set_corners(c.corners[None])
    s.init_template(sm)
    s.set_state(c.p[None])
    s.update_pix_vals()
    it_orig = ((c.nb - 1.0) / 255.0) * s.read(L.BUF_IT)[0]
    s.close()
    np.testing.assert_allclose(it_orig, T.ref(cid, model)["It_orig"], rtol=0, atol=1e-9)
    if model == "rscv":
        want = maps[np.clip(np.rint(it_orig).astype(np.int64), 0, c.nb - 1)]
    else:
        want = T.G9.blend(it_orig, maps, None, T.weights(cid), c.geo[0], c.geo[1], False, False)
    np.testing.assert_array_equal(it_fused, want)
    b.set_first_iter(True)
    b.update_pix_vals()
    np.testing.assert_array_equal(read_maps(b, model)[0], maps)
    np.testing.assert_array_equal(b.read(L.BUF_IT)[0], it_fused)
    b.close()


# ------------------------------------------------------------------------------------------------------------------ batch seams
def run_batch(ctx, c, model, once, math, cs, ps, sm, twice=False):
    b = make_batch(ctx, c, model, math, corners=cs, once=once)
    out = []
    for _ in range(2 if twice else 1):
        b.set_corners(cs)
        b.init_template(sm)
        b.set_state(ps)
        b.track_trace(T.BATCH_MAX_ITERS)
        n, corners = b.track(sm)
        dps = [np.array([rec["dp"] for rec in t]) for t in b.read_track_trace(n)]
        out.append((n.copy(), corners.copy(), read_maps(b, model).copy(), dps))
        b.track_trace(0)
    b.close()
    return out


def same_run(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])
    for x, y in zip(a[3], b[3]):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("materialize", [1, 0])
@pytest.mark.parametrize("model,once,affine", T.BATCH_CONFIGS)
def test_batch_sizes_on_and_off_the_launch_chunk(gpu_ctx, monkeypatch, model, once, affine, materialize):
    """12 x 11 patches, batches of 1, tpl - 1, tpl, tpl + 1 and 2 tpl + 3 targets (tpl: the targets per launch of the chunked device
    loop, forced to a few targets) that stop at different iterations -- some at the solution, some displaced, one wholly outside the
    frame in the middle: the iteration counts are the reference's, every target's maps, state updates and corners are bit for bit
    those it gives alone, and a second track on the same batch equals the first (the arrival counters and the zeroed sums survive
    targets dropping out).  materialize 0: the lean launches, whose pass 1 of RSCV / LRSCV samples with the tolerance-mode arithmetic"""
    c = T.batch_case(affine)
    n_pix = c.resx * c.resy
    monkeypatch.setenv("MTFHIP_TRACK_CHUNK_PX", str(4 * n_pix))
    sm = track_sm("esm", max_iters=T.BATCH_MAX_ITERS, epsilon=T.BATCH_EPS, materialize=materialize)
    cs8, ps8, _ = T.batch_targets(affine, 8)
    probe = make_batch(gpu_ctx, c, model, mtf_amd.MATH_REPLAY, corners=cs8, once=once)
    probe.init_template(sm)
    tpl = probe.track_targets_per_launch(sm)
    probe.close()
    assert tpl == 4
    for math in MATHS:
        for B in (1, tpl - 1, tpl, tpl + 1, 2 * tpl + 3):
            cs, ps, kinds = T.batch_targets(affine, B)
            n_ref, _ = T.batch_ref_iters(affine, model, once, B)
            if B == 2 * tpl + 3:
                assert len(set(n_ref.tolist())) >= 3
            first, second = run_batch(gpu_ctx, c, model, once, math, cs, ps, sm, twice=True)
            np.testing.assert_array_equal(first[0], n_ref)
            same_run(first, second)
            assert np.isfinite(first[1]).all()
            for k in range(B):
                one = run_batch(gpu_ctx, c, model, once, math, cs[k:k + 1], ps[k:k + 1], sm)[0]
                same_run((first[0][k:k + 1], first[1][k:k + 1], first[2][k:k + 1], first[3][k:k + 1]), one)


# ------------------------------------------------------------------------------------------------------------------- LDS budget
@pytest.mark.parametrize("model", ["lscv", "lrscv"])
@pytest.mark.parametrize("nb", [64, 256])
def test_largest_sub_region_count_the_lds_budget_admits(gpu_ctx, model, nb):
    """1 x n sub-regions at spacing 1 on an 8 x 130 patch: the largest n whose cells fit the histogram LDS budget gives reference
    results, n + 1 is refused by init_template, and a correctly configured batch on the same context still works afterwards"""
    n, cells, cells_next = T.lds_limit_counts(nb)
    assert 8 * cells * nb <= T.LDS_HIST_BUDGET < 8 * cells_next * nb
    c = T.lds_case(nb, n)
    pa = T.G6.Patch(T.IMG64, nb, c.resx, c.resy, False, c.corners)
    r = T.evaluate(c, model, pa, pa.warp(c.p), T.G8.weights(*T.geo6(c)))
    check_iterate(gpu_ctx, c, model, r=r)
    check_interface(gpu_ctx, c, model, r=r)
    over = T.lds_case(nb, n + 1)
    b = make_batch(gpu_ctx, over, model, mtf_amd.MATH_REPLAY)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="LDS"):
        b.init_template(mtf_amd.sm_desc(L.SM_FCLK, hess_type=1, materialize=0, leven_marq=0))
    b.close()
    check_iterate(gpu_ctx, c, model, r=r, materializes=(0,))
