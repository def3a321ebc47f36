"""GPU: every image sampler on a frame whose pitch, origin and aspect are not the suite's usual ones.

One principle: an entry point run on the packed upload of a frame (ctx.set_image) and run again on the SAME pixels borrowed as a padded,
offset view of a larger device tensor (mtfhip_image_borrow with row_stride > width, the base pointer at an odd float offset) must give
the same bits -- the arithmetic does not depend on where a texel was fetched from.  The frame is 96 x 160 (and 48 x 160: lower than the
64 x 64 LDS window of k_iclk_track / k_grid_fb, so their fallback runs); it sits in the middle of a 256 x 203 tensor whose every other
element is 1e6, so a sampler that used w for the pitch, swapped w and h, or read past a border lands inside the allocation and returns a
WRONG NUMBER (test_frame_layout_cpu.py holds the fixture and checks that it discriminates).  Five targets per batch: one inside, one
across each border (where poison is adjacent and the sampler must give the reference's 128).

What equality cannot catch -- an error shared by both layouts -- is covered by the oracle on the non-square upload (last section), at
the tolerances of the corresponding tests in test_gpu_parity.py / test_gpu_trackers.py.

The library refuses none of the combinations below, so nothing here skips: an exception in either layout is a failure."""
import ctypes as C

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth

import test_frame_layout_cpu as FL

pytestmark = pytest.mark.gpu

MATHS = [mtf_amd.MATH_REPLAY, mtf_amd.MATH_FAST]
RES_IDS = ["%dx%d" % r for r in FL.RES]


@pytest.fixture(scope="module")
def lay():
    """name -> (logical frame on the host, its poisoned parent tensor on the device)"""
    import torch
    out = {name: (view, torch.from_numpy(FL.place(view)).to("cuda:0")) for name, view in FL.views().items()}
    torch.cuda.synchronize()
    return out


def borrow(ctx, view, parent):
    ctx.set_image_device(parent.data_ptr() + 4 * (FL.R0 * FL.PW + FL.C0), view.shape[0], view.shape[1], FL.PW, keep=parent)


def both_layouts(ctx, lay, fn, equal_nan=False):
    """fn(set_img) -> {name: array}, run with set_img(name) uploading the packed frame, then borrowing the padded view; every output
    must be bit-identical (equal_nan: NaN in the same places counts as identical).  The context is left with a packed image."""
    def packed(name):
        ctx.set_image(lay[name][0])

    def padded(name):
        borrow(ctx, *lay[name])
    try:
        want = fn(packed)
        got = fn(padded)
    finally:
        ctx.set_image(lay["a"][0])
    assert sorted(want) == sorted(got)
    bad = []
    for k in sorted(want):
        a, b = np.asarray(want[k]), np.asarray(got[k])
        assert a.shape == b.shape, k
        if not np.array_equal(a, b, equal_nan=equal_nan and a.dtype.kind == "f"):
            i = np.flatnonzero(a.ravel() != b.ravel())
            bad.append("%s: %d of %d differ, first at %d: packed %r, padded %r" % (k, i.size, a.size, i[0], a.ravel()[i[0]], b.ravel()[i[0]]))
    assert not bad, "\n".join(bad)
    return want


def read_materialised(b, out, key, sm_kind):
    """what a materialising iterate stores (mtfhip_batch_iterate, mi_enqueue): It for every search method; dIt_dx and Jt for ESM and FCLK.
    ICLK works on the template's gradient and Jacobian and stores neither -- reading them is refused, in both layouts."""
    out[key + "It"] = b.read(L.BUF_IT).copy()
    for name, buf in (("dIt_dx", L.BUF_DIT_DX), ("Jt", L.BUF_JT)):
        if sm_kind != L.SM_ICLK:
            out[key + name] = b.read(buf).copy()
        else:
            with pytest.raises(mtf_amd.LogicError):
                b.read(buf)


# ------------------------------------------------------------------ per-function interface
@pytest.mark.parametrize("math", MATHS, ids=["replay", "fast"])
@pytest.mark.parametrize("res", FL.RES, ids=RES_IDS)
@pytest.mark.parametrize("ssm", [L.SSM_HOMOGRAPHY, L.SSM_AFFINE], ids=["hom", "aff"])
def test_per_function_interface(gpu_ctx, lay, ssm, res, math):
    """initialize / update PixVals, PixGrad (chained and warped form), PixHess (both forms): k_pix_vals, k_img_grad*, k_img_hess*"""
    states = FL.small_states(ssm)

    def run(set_img):
        out = {}
        set_img("a")
        b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, ssm, res[0], res[1], FL.B)
        try:
            b.set_math_mode(math)
            b.set_corners(FL.targets())
            b.update_grad_pts(); b.update_hess_pts()
            b.initialize_pix_vals(); out["I0"] = b.read(L.BUF_I0).copy()
            b.initialize_pix_grad(); out["dI0_dx"] = b.read(L.BUF_DI0_DX).copy()
            b.initialize_pix_grad(warped=True); out["dI0_dx_warped"] = b.read(L.BUF_DI0_DX).copy()
            b.initialize_pix_hess(); out["d2I0_dx2"] = b.read(L.BUF_D2I0_DX2).copy()
            b.initialize_pix_hess(warped=True); out["d2I0_dx2_warped"] = b.read(L.BUF_D2I0_DX2).copy()
            set_img("b")
            b.set_state(states)
            b.update_grad_pts(); b.update_hess_pts()
            b.update_pix_vals(); out["It"] = b.read(L.BUF_IT).copy()
            b.update_pix_grad(); out["dIt_dx"] = b.read(L.BUF_DIT_DX).copy()
            b.update_pix_grad(warped=True); out["dIt_dx_warped"] = b.read(L.BUF_DIT_DX).copy()
            b.update_pix_hess(warped=False); out["d2It_dx2"] = b.read(L.BUF_D2IT_DX2).copy()
            b.update_pix_hess(warped=True); out["d2It_dx2_warped"] = b.read(L.BUF_D2IT_DX2).copy()
        finally:
            b.close()
        return out
    out = both_layouts(gpu_ctx, lay, run)
    # the border is the reference's constant, never a padding value; the inside target never meets it
    for k in ("I0", "It"):
        assert out[k].max() < 1e3 and np.all(out[k][0] != 128.0)
        assert all((out[k][t] == 128.0).any() for t in range(1, FL.B)), k


# ------------------------------------------------------------------ Batch.iterate
def _am_batch(ctx, cfg, ssm, res):
    if cfg in ("ssd", "ssd_so"):
        return mtf_amd.Batch(ctx, L.AM_SSD, ssm, res[0], res[1], FL.B)
    if cfg in ("ncc", "ncc_so"):
        return mtf_amd.Batch(ctx, L.AM_NCC, ssm, res[0], res[1], FL.B)
    if cfg == "mi8":
        return mtf_amd.Batch(ctx, L.AM_MI, ssm, res[0], res[1], FL.B, mi_n_bins=8)
    if cfg == "mi10pou":
        return mtf_amd.Batch(ctx, L.AM_MI, ssm, res[0], res[1], FL.B, mi_n_bins=10, mi_pou=1)
    am = dict(scv=L.AM_SCV, rscv=L.AM_RSCV, lscv=L.AM_LSCV, lrscv=L.AM_LRSCV)[cfg]
    b = mtf_amd.Batch(ctx, am, ssm, res[0], res[1], FL.B, mi_n_bins=32)
    small = res[0] * res[1] < 1000       # (3 x 3 sub-regions at the reference's spacing 10 do not fit a 17 x 13 patch)
    if cfg == "scv":
        b.set_scv()
    elif cfg == "rscv":
        b.set_rscv()
    elif cfg == "lscv":
        b.set_lscv(3, 3, 4, 3) if small else b.set_lscv()
    else:
        b.set_lrscv(3, 3, 4, 3) if small else b.set_lrscv()
    return b


def _sm(cfg, sm_kind, **kw):
    if cfg.endswith("_so"):     # a Hessian type with a second-order form for SSD and for NCC (check_sm, api_fused.hip)
        kw.update(sec_ord_hess=1, hess_type=5 if sm_kind == L.SM_ESM else 2)
    return mtf_amd.sm_desc(sm_kind, leven_marq=0, **kw)


AM_CFGS = ["ssd", "ncc", "mi8", "mi10pou", "scv", "rscv", "lscv", "lrscv", "ssd_so", "ncc_so"]
SM_IDS = {L.SM_ESM: "esm", L.SM_FCLK: "fclk", L.SM_ICLK: "iclk"}


@pytest.mark.parametrize("res", FL.RES, ids=RES_IDS)
@pytest.mark.parametrize("sm_kind", [L.SM_ESM, L.SM_FCLK, L.SM_ICLK], ids=SM_IDS.get)
@pytest.mark.parametrize("cfg", AM_CFGS)
def test_iterate(gpu_ctx, lay, cfg, sm_kind, res):
    """one fused iteration of every appearance model, homography and affine, both math modes, materialize 0 and 1: f, g, H, the template
    and whatever the launch materialised (the fused bodies, the MI passes, the SCV-family map builders, k_second_order_ssd)"""
    def run(set_img):
        out = {}
        for ssm in (L.SSM_HOMOGRAPHY, L.SSM_AFFINE):
            states = FL.small_states(ssm)
            for math in MATHS:
                for mat in (0, 1):
                    set_img("a")
                    b = _am_batch(gpu_ctx, cfg, ssm, res)
                    try:
                        sm = _sm(cfg, sm_kind, materialize=mat)
                        b.set_math_mode(math)
                        b.set_corners(FL.targets())
                        b.init_template(sm)
                        set_img("b")
                        b.set_state(states)
                        if cfg in ("lscv", "lrscv"):
                            b.set_first_iter(True)
                        f, g, H = b.iterate(sm)
                        key = "ssm%d math%d mat%d " % (ssm, math, mat)
                        out[key + "f"], out[key + "g"], out[key + "H"] = f, g, H
                        out[key + "I0"] = b.read(L.BUF_I0).copy()
                        if mat:
                            read_materialised(b, out, key, sm_kind)
                    finally:
                        b.close()
        return out
    out = both_layouts(gpu_ctx, lay, run)
    assert all(np.all(np.isfinite(v)) for v in out.values())


# ------------------------------------------------------------------ the device loops
TRACK_FORMS = (("default mat1", None, 1), ("default mat0", None, 0), ("MTFHIP_PERSIST=1", "MTFHIP_PERSIST", 0), ("MTFHIP_STEP=1", "MTFHIP_STEP", 0))


def _track_both(ctx, lay, monkeypatch, cfg, sm_kind, rows, res):
    """init_template on the first frame + track on the next, three iterations, in every form the loop can be asked for (the keys name the
    REQUEST: where the library picks one kernel whatever is asked, as for ICLK at 17 x 13, the forms repeat that kernel)"""
    first, nxt = ("a", "b") if rows == FL.H else ("sa", "sb")
    corners = FL.targets(rows)
    ssm = L.SSM_AFFINE if sm_kind == L.SM_FCLK else L.SSM_HOMOGRAPHY

    def run(set_img):
        out = {}
        for form, env, mat in TRACK_FORMS:
            for math in MATHS:
                if env:
                    monkeypatch.setenv(env, "1")
                set_img(first)
                b = _am_batch(ctx, cfg, ssm, res)
                try:
                    sm = mtf_amd.sm_desc(sm_kind, materialize=mat, leven_marq=0, max_iters=3, epsilon=1e-4)
                    b.set_math_mode(math)
                    b.set_corners(corners)
                    b.init_template(sm)
                    set_img(nxt)
                    n, c = b.track(sm)
                    key = "%s math%d " % (form, math)
                    out[key + "n_iters"], out[key + "corners"], out[key + "state"] = n, c, b.get_state()
                finally:
                    b.close()
                    if env:
                        monkeypatch.delenv(env)
        return out
    out = both_layouts(ctx, lay, run)
    assert all(np.all(np.isfinite(v)) for v in out.values())
    assert np.abs(out["default mat0 math1 corners"][0] - corners[0]).max() > 1e-3   # the inside target moved


@pytest.mark.parametrize("res", FL.RES, ids=RES_IDS)
@pytest.mark.parametrize("rows", [FL.H, FL.H_SMALL])
@pytest.mark.parametrize("cfg", ["ssd", "ncc"])
@pytest.mark.parametrize("sm_kind", [L.SM_ESM, L.SM_FCLK, L.SM_ICLK], ids=SM_IDS.get)
def test_track(gpu_ctx, lay, monkeypatch, sm_kind, cfg, rows, res):
    """the launch-per-pass loop (materialising and lean), the persistent loop (MTFHIP_PERSIST=1), the one-launch-per-pass form
    (MTFHIP_STEP=1).  ICLK at 17 x 13 takes the one-launch grid kernel k_iclk_track in all four (it has precedence over both switches)
    -- its tolerance-mode LDS window is clamped to the frame at 96 rows and falls back to global loads at 48"""
    _track_both(gpu_ctx, lay, monkeypatch, cfg, sm_kind, rows, res)


@pytest.mark.parametrize("res", FL.RES, ids=RES_IDS)
@pytest.mark.parametrize("rows", [FL.H, FL.H_SMALL])
@pytest.mark.parametrize("cfg", ["mi8", "scv"])
@pytest.mark.parametrize("sm_kind", [L.SM_ESM, L.SM_ICLK], ids=SM_IDS.get)
def test_track_mi_and_scv(gpu_ctx, lay, monkeypatch, sm_kind, cfg, rows, res):
    """the device loops of the models that have passes of their own between the pixel passes: MI (its recompute passes inside the loop) and
    SCV (the intensity map rebuilt from It every pass)"""
    _track_both(gpu_ctx, lay, monkeypatch, cfg, sm_kind, rows, res)


# ------------------------------------------------------------------ the grid tracker's forward-backward frame
@pytest.mark.parametrize("rows", [FL.H, FL.H_SMALL])
@pytest.mark.parametrize("am", [L.AM_NCC, L.AM_SSD], ids=["ncc", "ssd"])
def test_grid_forward_backward(gpu_ctx, lay, am, rows):
    """GridTracker with fb_err_thresh > 0: initialize on the first frame (keep_prev), the second frame, one update() -- the patch trackers
    with the backward estimation (mtfhip_grid_frame_fb: k_grid_fb runs the forward pass on the current frame and the backward pass on the
    KEPT frame in one launch in tolerance mode; replay mode takes the launch-by-launch form), update()'s own keep_prev of the second
    frame, and the re-initialisation of every patch on the moved region (k_template_init on the second frame).  Compared: all that
    mtfhip_grid_frame_fb returns (n_iters, corners, centroids, fb_prev_pts -- the centroids of the corners the backward pass arrived at --,
    the FB mask and the masked point sets), the region, the re-initialised templates, and the frame update() kept.
    The kept frame is the context's own packed clone in both runs (that is what keep_prev is for), so the backward pass samples a packed
    image either way: the padded layout reaches it through the clone's copy and through the re-initialisation in front of it.
    The fit of the grid SSM is host arithmetic and pluggable; a fixed small translation stands in for it, so that a patch that ran away
    (NaN from the previous frame, test_grid_fb_one_launch_equals_three) does not reach an SVD: NaN in the same places in both layouts is
    equality here.  One region inside the frame, one whose left edge is 3 px outside it, so that the first column of patches straddles
    the border and none lies wholly outside (a patch of constant 128 has zero variance: NCC is undefined there, in the reference as
    well)."""
    from mtf_amd.sm import GridTracker
    first, nxt = ("a", "b") if rows == FL.H else ("sa", "sb")
    regions = [synth.square_corners(80, rows / 2.0, 0.6 * rows), synth.square_corners(0.3 * rows - 3, rows / 2.0, 0.6 * rows)]
    moved = np.array([0.0, 0.0, 1.5, 0.0, 0.0, -0.75, 0.0, 0.0])

    def run(set_img):
        out = {}
        for math in MATHS:
            for r, region in enumerate(regions):
                set_img(first)
                gt = GridTracker(gpu_ctx, grid_size=4, patch_size=16, am=am, max_iters=3, fb_err_thresh=2.0, estimator=lambda p, c: moved)
                batch = gt.tracker.batch
                try:
                    batch.set_math_mode(math)
                    gt.initialize(region)
                    set_img(nxt)
                    key = "math%d region%d " % (math, r)
                    frame_fb = batch.grid_frame_fb

                    def recorded(*a, **kw):
                        res = frame_fb(*a, **kw)
                        out.update((key + k, np.array(v)) for k, v in res.items())
                        return res
                    batch.grid_frame_fb = recorded
                    out[key + "region"] = gt.update()
                    out[key + "fb_err_mask of update"] = np.array(gt.fb_err_mask)
                    out[key + "I0 after the reset"] = batch.read(L.BUF_I0).copy()
                    gpu_ctx.swap_prev()
                    out[key + "kept"] = gpu_ctx.get_image()
                    gpu_ctx.swap_prev()
                finally:
                    batch.close()
        return out
    out = both_layouts(gpu_ctx, lay, run, equal_nan=True)
    for k, v in out.items():
        if k.endswith("centroids") or k.endswith("fb_prev_pts"):
            assert np.isfinite(v).any(), k
        if k.endswith("kept"):
            assert np.array_equal(v, lay[nxt][0]), k
        if k.endswith("region"):
            assert np.all(np.isfinite(v)) and np.abs(v - regions[int(k.split("region")[1][0])]).max() > 0.5, k
        if k.endswith("I0 after the reset"):
            assert np.all(np.isfinite(v)) and v.max() < 1e3, k


# ------------------------------------------------------------------ candidate scoring and the NN dataset
def candidate_states(corners, sigma_t):
    """300 small homographies about a target; the first 40 carry its centre to x = 8 at the least 10 px to the left, across the left border"""
    rng = np.random.default_rng(3)
    states = rng.normal(size=(300, 8)) * np.array([0.01, 0.01, sigma_t, 0.01, 0.01, sigma_t, 1e-5, 1e-5])
    states[:40, 2] -= max(corners[0].mean() - 8.0, 10.0)
    return states


@pytest.mark.parametrize("res", FL.RES, ids=RES_IDS)
@pytest.mark.parametrize("am", [L.AM_SSD, L.AM_NCC], ids=["ssd", "ncc"])
def test_score_candidates_and_nn_dataset(gpu_ctx, lay, monkeypatch, am, res):
    """k_pf_score (300 candidates of each of the five targets, 40 of them pushed across the left border: for the inside target the rest
    take the hull shortcut, every other candidate the per-sample path), k_nn_dataset / k_nn_rows (64 samples), both math modes.
    (MTFHIP_PAIR_IMAGE=0: the row-pair copy exists for uploads only.)"""
    monkeypatch.setenv("MTFHIP_PAIR_IMAGE", "0")

    def run(set_img):
        out = {}
        set_img("b")
        for t, corners in enumerate(FL.targets()):
            states = candidate_states(corners, 3.0)
            b = mtf_amd.Batch(gpu_ctx, am, L.SSM_HOMOGRAPHY, res[0], res[1], 1)
            try:
                b.set_corners(corners[None]); b.initialize_pix_vals(); b.initialize_similarity()
                for math in MATHS:
                    b.set_math_mode(math)
                    key = "target%d math%d " % (t, math)
                    out[key + "lik"], out[key + "sim"] = b.score_candidates(states, want_similarity=True)
                    out[key + "warps"], out[key + "rows"] = b.nn_dataset(64, np.array([0.01, 0.01, 2.0, 0.01, 0.01, 2.0, 1e-5, 1e-5]), None, seed=4)
            finally:
                b.close()
        return out
    both_layouts(gpu_ctx, lay, run)


# ------------------------------------------------------------------ image plumbing on the padded view
def test_image_plumbing_on_a_padded_view(gpu_ctx, lay):
    """get_image, keep_prev (the stride-aware copy: a borrowed frame is CLONED), swap_prev and their corner cases, as
    prev_img = curr_img.clone() would leave them"""
    import torch
    ctx = gpu_ctx
    a, b = lay["a"][0], lay["b"][0]
    ta = torch.from_numpy(FL.place(a)).to("cuda:0")       # (this test overwrites its parent: a private one)
    tb = lay["b"][1]
    torch.cuda.synchronize()
    try:
        borrow(ctx, a, ta)
        assert ctx.image_shape() == (FL.H, FL.W)
        np.testing.assert_array_equal(ctx.get_image(), a)
        ctx.keep_prev()
        # keep_prev of a borrowed frame returns with the clone complete (mtfhip.h), so the caller writes its next frame into the same
        # buffer at once, on a stream of its own that nothing orders against the context's
        ta[FL.R0:FL.R0 + FL.H, FL.C0:FL.C0 + FL.W] = 7.0
        torch.cuda.synchronize()
        borrow(ctx, b, tb)
        np.testing.assert_array_equal(ctx.get_image(), b)
        ctx.swap_prev()
        assert ctx.image_shape() == (FL.H, FL.W)
        np.testing.assert_array_equal(ctx.get_image(), a)
        # keep_prev right after swap_prev: the current image IS the kept copy; both views then show it
        ctx.keep_prev()
        np.testing.assert_array_equal(ctx.get_image(), a)
        ctx.swap_prev()
        np.testing.assert_array_equal(ctx.get_image(), a)
        # keep_prev twice in a row on a borrowed frame
        borrow(ctx, b, tb)
        ctx.keep_prev(); ctx.keep_prev()
        np.testing.assert_array_equal(ctx.get_image(), b)
        ctx.swap_prev()
        np.testing.assert_array_equal(ctx.get_image(), b)
        ctx.swap_prev()
        np.testing.assert_array_equal(ctx.get_image(), b)
        # a frame of another shape kept after a larger one, and a padded frame kept after an uploaded one was kept
        sa, tsa = lay["sa"]
        ctx.set_image(a); ctx.keep_prev()
        borrow(ctx, sa, tsa); ctx.keep_prev()
        ctx.set_image(b)
        ctx.swap_prev()
        assert ctx.image_shape() == (FL.H_SMALL, FL.W)
        np.testing.assert_array_equal(ctx.get_image(), sa)
        ctx.swap_prev()
        np.testing.assert_array_equal(ctx.get_image(), b)
        # a padded pyramid source is refused cleanly; the packed one is taken
        borrow(ctx, b, tb)
        ctx2 = mtf_amd.Context(0)
        try:
            with pytest.raises(mtf_amd.FunctionNotImplemented, match="padded source rows"):
                ctx2.pyramid_level_from(ctx, FL.H // 2, FL.W // 2)
            ctx.set_image(b)
            ctx2.pyramid_level_from(ctx, FL.H // 2, FL.W // 2)
            assert ctx2.image_shape() == (FL.H // 2, FL.W // 2)
        finally:
            ctx2.close()
    finally:
        ctx.set_image(a)


def test_borrow_refuses_a_pitch_below_the_width(gpu_ctx, lay):
    """through the ABI (the library creates no context without a device, so this lives here): the image in place stays"""
    a, ta = lay["a"]
    gpu_ctx.set_image(a)
    rc = L.lib().mtfhip_image_borrow(gpu_ctx._h, C.c_void_p(ta.data_ptr()), FL.H, FL.W, FL.W - 1)
    assert rc == -1 and b"image_borrow: bad shape" in L.lib().mtfhip_last_error()
    with pytest.raises(mtf_amd.InvalidArgument):
        gpu_ctx.set_image_device(ta.data_ptr(), FL.H, FL.W, FL.W - 1, keep=ta)
    np.testing.assert_array_equal(gpu_ctx.get_image(), a)


# ------------------------------------------------------------------ the non-square upload against the oracle
def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = np.linalg.norm(b)
    return np.linalg.norm(a - b) / n if n > 0 else np.linalg.norm(a - b)


@pytest.mark.parametrize("res", FL.RES, ids=RES_IDS)
@pytest.mark.parametrize("ssm", [L.SSM_HOMOGRAPHY, L.SSM_AFFINE], ids=["hom", "aff"])
def test_non_square_samples_and_gradients_match_oracle(oracle, gpu_ctx, lay, ssm, res):
    """updatePixVals / updatePixGrad fed with the oracle's own points: bit for bit, as test_unfused_interface_chain and
    test_border_and_integer_coordinate_cases hold them on the square frame"""
    img = lay["b"][0]
    states = FL.small_states(ssm)
    gpu_ctx.set_image(img)
    b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, ssm, res[0], res[1], FL.B)
    try:
        b.set_corners(FL.targets())
        pts, want_v, want_g = [], [], []
        for t, corners in enumerate(FL.targets()):
            o_ssm = oracle.SSM(ssm, res[0], res[1]); o_ssm.set_corners(corners); o_ssm.set_state(states[t])
            p = o_ssm.get("curr_pts")
            pts.append(p.reshape(-1, 2).T)
            want_v.append(oracle.get_pix_vals(img, p)); want_g.append(oracle.get_img_grad(img, p).reshape(2, -1).T)
        pts = np.stack(pts)
        b.update_pix_vals(pts); b.update_pix_grad(pts)
        got_v, got_g = b.read(L.BUF_IT), b.read(L.BUF_DIT_DX)
        assert np.array_equal(got_v, np.stack(want_v))
        assert np.array_equal(got_g, np.stack(want_g))
    finally:
        b.close()


@pytest.mark.parametrize("res", FL.RES, ids=RES_IDS)
@pytest.mark.parametrize("am", [L.AM_SSD, L.AM_NCC], ids=["ssd", "ncc"])
def test_non_square_iterate_matches_oracle(oracle, gpu_ctx, lay, am, res):
    """the first ESM iteration of the five targets on the device's own grid against the oracle's trace: the device_grid bounds of
    _fused_follow in test_gpu_parity.py (f 1e-8; H 1e-5; g 1e-5 of max(|g|, its Cauchy-Schwarz scale))"""
    a, nxt = lay["a"][0], lay["b"][0]
    gpu_ctx.set_image(a)
    b = mtf_amd.Batch(gpu_ctx, am, L.SSM_HOMOGRAPHY, res[0], res[1], FL.B)
    try:
        params = dict(leven_marq=0, max_iters=1)
        sm = mtf_amd.sm_desc(L.SM_ESM, materialize=1, **params)
        b.set_math_mode(mtf_amd.MATH_REPLAY)
        b.set_corners(FL.targets())
        b.init_template(sm)
        gpu_ctx.set_image(nxt)
        f, g, H = b.iterate(sm)
        for t, corners in enumerate(FL.targets()):
            o_ssm = oracle.SSM(L.SSM_HOMOGRAPHY, res[0], res[1]); o_am = oracle.AM(am, res[0], res[1]); o_am.set_curr_img(a)
            trk = oracle.Tracker(L.SM_ESM, o_am, o_ssm, **params)
            trk.initialize(corners)
            o_am.set_curr_img(nxt)
            trk.update()
            rec = trk.trace()[0]
            g_scale = np.sqrt(abs(np.trace(rec["H"]))) * (np.sqrt(abs(2 * rec["f"])) if am == L.AM_SSD else 1.0)
            assert rel(f[t], rec["f"]) < 1e-8, t
            assert rel(H[t], rec["H"]) < 1e-5, t
            assert np.linalg.norm(g[t] - rec["g"]) < 1e-5 * max(np.linalg.norm(rec["g"]), g_scale), t
    finally:
        b.close()


@pytest.mark.parametrize("res", FL.RES, ids=RES_IDS)
@pytest.mark.parametrize("am", [L.AM_SSD, L.AM_NCC], ids=["ssd", "ncc"])
def test_non_square_candidate_scores_match_oracle(oracle, gpu_ctx, lay, am, res):
    """300 candidates of each of the five targets, and of the right-border target moved 12 px left (x up to 153: its unshifted candidates'
    hulls are inside a frame 160 wide and outside one 96 wide, so the hull shortcut answers to w), 40 of each pushed across the left
    border: rtol 1e-9 in both math modes, as test_pf_candidate_scores_at_the_frame_border"""
    img = lay["b"][0]
    cases = list(FL.targets()) + [FL.targets()[3] - np.array([[12.0], [0.0]])]
    gpu_ctx.set_image(img)
    for t, corners in enumerate(cases):
        states = candidate_states(corners, 2.0)
        o_ssm = oracle.SSM(L.SSM_HOMOGRAPHY, res[0], res[1]); o_am = oracle.AM(am, res[0], res[1]); o_am.set_curr_img(img)
        o_ssm.set_corners(corners)
        o_am.initialize_pix_vals(o_ssm.get("curr_pts")); o_am.initialize_similarity()
        lik_o, sim_o = oracle.pf_score(o_am, o_ssm, states)
        keep = np.isfinite(sim_o)
        assert keep.sum() >= 250, t
        b = mtf_amd.Batch(gpu_ctx, am, L.SSM_HOMOGRAPHY, res[0], res[1], 1)
        try:
            b.set_corners(corners[None]); b.initialize_pix_vals(); b.initialize_similarity()
            for mode in (L.MATH_FAST, L.MATH_REPLAY):
                b.set_math_mode(mode)
                lik, sim = b.score_candidates(states, want_similarity=True)
                np.testing.assert_allclose(sim[keep], sim_o[keep], rtol=1e-9, err_msg="target %d mode %d" % (t, mode))
                np.testing.assert_allclose(lik[keep], lik_o[keep], rtol=1e-9, atol=1e-300, err_msg="target %d mode %d" % (t, mode))
        finally:
            b.close()


def test_non_square_multichannel_matches_oracle(oracle, gpu_ctx, lay):
    """a 96 x 160 x 3 upload (stride = 3 w): template samples and the first ESM iteration of MCSSD at the bounds of
    test_multichannel_models_match_oracle (I0 1e-9 absolute; f 1e-7, H 1e-5, g 1e-4 of its scale)"""
    res = 17, 13
    frame = synth.make_frame_mc(FL.H, FL.W)
    p_true = synth.random_small_homography(np.random.default_rng(2027)) * 0.5
    frame2 = synth.warp_frame(frame, p_true, (FL.W / 2.0, FL.H / 2.0))
    params = dict(leven_marq=0, max_iters=1)
    try:
        gpu_ctx.set_image(frame)
        b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, res[0], res[1], FL.B, n_channels=3)
        try:
            sm = mtf_amd.sm_desc(L.SM_ESM, materialize=1, **params)
            b.set_corners(FL.targets())
            b.init_template(sm)
            I0 = b.read(L.BUF_I0).copy()
            gpu_ctx.set_image(frame2)
            b.update_pix_vals()
            It = b.read(L.BUF_IT).copy()
            f, g, H = b.iterate(sm)
            for t, corners in enumerate(FL.targets()):
                o_ssm = oracle.SSM(L.SSM_HOMOGRAPHY, res[0], res[1]); o_am = oracle.AM(L.AM_SSD, res[0], res[1])
                o_am.set_channels(3); o_ssm.set_channels(3)
                o_am.set_curr_img(frame)
                trk = oracle.Tracker(L.SM_ESM, o_am, o_ssm, **params)
                trk.initialize(corners)
                np.testing.assert_allclose(I0[t], o_am.get("I0"), rtol=0, atol=1e-9)
                o_am.set_curr_img(frame2)
                trk.update()
                rec = trk.trace()[0]
                np.testing.assert_allclose(It[t], o_am.get("It"), rtol=0, atol=1e-9)
                assert abs(f[t] - rec["f"]) <= 1e-7 * abs(rec["f"]), t
                assert np.linalg.norm(H[t] - rec["H"]) <= 1e-5 * np.linalg.norm(rec["H"]), t
                gs = max(np.linalg.norm(rec["g"]), 1e-3 * np.sqrt(abs(np.trace(rec["H"]))))
                assert np.linalg.norm(g[t] - rec["g"]) <= 1e-4 * gs, t
        finally:
            b.close()
    finally:
        gpu_ctx.set_image(lay["a"][0])
