"""The fused LK kernel rebuilds the template grid point of every row from the target's map and the lattice index (FusedArgs::grid_regen)
instead of reading INIT_PTS back, when the grid is the one set_corners laid out.  Writing the same INIT_PTS back through the C-ABI
clears that plan flag (the caller may have laid out its own grid), so the same inputs run once on each path: every materialised array,
f / g / H and the tracked warps must be the same bits."""
import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth

pytestmark = pytest.mark.gpu


def _corners(B, res, seed, parallelogram=True, H=512, W=512):
    rng = np.random.default_rng(seed)
    out = np.empty((B, 2, 4))
    for t in range(B):
        # (multiples of 1/8: the corner sums are exact, so the sheared quad is a parallelogram to the bit and its map is affine)
        cx, cy = np.round(rng.uniform(0.3 * W, 0.7 * W) * 8) / 8, np.round(rng.uniform(0.3 * H, 0.7 * H) * 8) / 8
        half = np.round((0.5 * res + rng.uniform(-4, 4)) * 8) / 8
        sh = np.round(rng.uniform(-0.1, 0.1) * half * 8) / 8
        x = np.array([cx - half + sh, cx + half + sh, cx + half - sh, cx - half - sh])
        y = np.array([cy - half, cy - half, cy + half, cy + half])
        if not parallelogram:
            x[2] += rng.uniform(2, 5)
            y[3] -= rng.uniform(2, 5)
        out[t, 0], out[t, 1] = x, y
    return out


def _run(ctx, am, ssm, res, B, corners, sm_kind, math, materialize, rewrite, frame1):
    b = mtf_amd.Batch(ctx, am, ssm, res, res, B)
    b.set_math_mode(math)
    b.set_corners(corners)
    pts0 = b.read(L.BUF_INIT_PTS)
    if rewrite:     # (before init_template, which marks J0 as the template's again: both runs rebuild J0 rows the same way)
        b.write(L.BUF_INIT_PTS, pts0)
    sm = mtf_amd.sm_desc(sm_kind, materialize=materialize, leven_marq=0, epsilon=-1.0, max_iters=1)
    b.init_template(sm)
    planned = b.grid_regen(sm)
    ctx.set_image(frame1)
    rng = np.random.default_rng(11)
    b.set_state(np.stack([synth.random_small_homography(rng, 0.5)[:b.S] for _ in range(B)]))
    f, g, Hm = b.iterate(sm)
    out = {"f": f, "g": g, "H": Hm, "pts": pts0}
    if materialize:
        out["It"] = b.read(L.BUF_IT)
        if sm_kind != mtf_amd.SM_ICLK:     # (ICLK takes no gradient of the current image)
            out["dIt"] = b.read(L.BUF_DIT_DX)
            out["Jt"] = b.read(L.BUF_JT)
    sm.max_iters = 5
    b.set_state(np.zeros((B, b.S)))
    n, c = b.track(sm)
    out["warps"] = b.get_warp()
    out["corners"] = c
    b.close()
    return out, planned


def _same(a, b):
    for k in a:
        assert a[k].shape == b[k].shape, k
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), "%s differs between the rebuilt and the read grid" % k


CASES = [
    # am, ssm, res, B, sm, math, materialize, parallelogram, the rebuild planned (grid_regen_kernel: materialising SSD homography, chained
    # FCLK / ESM, on a unit-z grid, at least kGridRegenMinRows = 8 rows per workgroup)
    (mtf_amd.AM_SSD, mtf_amd.SSM_HOMOGRAPHY, 200, 64, mtf_amd.SM_ESM, mtf_amd.MATH_FAST, 1, True, True),     # the headline shape
    (mtf_amd.AM_SSD, mtf_amd.SSM_HOMOGRAPHY, 100, 91, mtf_amd.SM_ESM, mtf_amd.MATH_REPLAY, 1, True, True),   # B not a multiple of the split
    (mtf_amd.AM_SSD, mtf_amd.SSM_HOMOGRAPHY, 100, 90, mtf_amd.SM_FCLK, mtf_amd.MATH_REPLAY, 1, True, True),
    (mtf_amd.AM_SSD, mtf_amd.SSM_HOMOGRAPHY, 300, 12, mtf_amd.SM_ESM, mtf_amd.MATH_REPLAY, 1, True, True),   # resx > one 256-point row
    (mtf_amd.AM_SSD, mtf_amd.SSM_HOMOGRAPHY, 200, 1, mtf_amd.SM_ESM, mtf_amd.MATH_FAST, 1, True, False),     # one target: 4 rows per workgroup
    (mtf_amd.AM_SSD, mtf_amd.SSM_HOMOGRAPHY, 100, 91, mtf_amd.SM_ICLK, mtf_amd.MATH_REPLAY, 1, True, False), # ICLK: reads INIT_PTS
    (mtf_amd.AM_SSD, mtf_amd.SSM_AFFINE, 100, 91, mtf_amd.SM_ESM, mtf_amd.MATH_REPLAY, 1, True, False),     # affine: reads INIT_PTS
    (mtf_amd.AM_SSD, mtf_amd.SSM_HOMOGRAPHY, 100, 91, mtf_amd.SM_ESM, mtf_amd.MATH_FAST, 0, True, False),    # lean: reads INIT_PTS
    (mtf_amd.AM_NCC, mtf_amd.SSM_HOMOGRAPHY, 100, 91, mtf_amd.SM_ESM, mtf_amd.MATH_FAST, 1, True, False),    # NCC: reads INIT_PTS
    (mtf_amd.AM_NCC, mtf_amd.SSM_AFFINE, 40, 7, mtf_amd.SM_FCLK, mtf_amd.MATH_FAST, 0, True, False),
    (mtf_amd.AM_SSD, mtf_amd.SSM_HOMOGRAPHY, 100, 91, mtf_amd.SM_ESM, mtf_amd.MATH_FAST, 1, False, False),   # unit_z 0: the flag stays off
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "am%d_ssm%d_%dx%d_B%d_sm%d_math%d_mat%d_%s" % (
    c[0], c[1], c[2], c[2], c[3], c[4], c[5], c[6], "para" if c[7] else "quad"))
def test_rebuilt_grid_matches_read_grid(gpu_ctx, frame, frame2, case):
    am, ssm, res, B, sm_kind, math, mat, para, planned = case
    corners = _corners(B, res, seed=res + B, parallelogram=para, H=1024 if res > 200 else 512, W=1024 if res > 200 else 512)
    big = res > 200
    f0, f1 = (np.pad(frame, ((0, 512), (0, 512)), mode="reflect"), np.pad(frame2, ((0, 512), (0, 512)), mode="reflect")) if big else (frame, frame2)
    gpu_ctx.set_image(f0)
    a, plan_a = _run(gpu_ctx, am, ssm, res, B, corners, sm_kind, math, mat, False, f1)
    gpu_ctx.set_image(f0)
    b, plan_b = _run(gpu_ctx, am, ssm, res, B, corners, sm_kind, math, mat, True, f1)
    assert plan_a == planned, "the rebuild was %splanned" % ("not " if planned else "")
    assert not plan_b, "a caller-written INIT_PTS must turn the rebuild off"
    _same(a, b)


def test_caller_points_are_used(gpu_ctx, frame, frame2):
    """after a caller writes INIT_PTS the kernel samples at the caller's points, not at the lattice of the corners: the grid moved by
    three pixels gives what a grid laid out inside corners moved by three pixels gives (to the rounding of the two layouts)"""
    B, res = 91, 100    # (>= 8 rows per workgroup: the rebuild is planned)
    corners = _corners(B, res, seed=5)
    sm = mtf_amd.sm_desc(mtf_amd.SM_ESM, materialize=1, leven_marq=0, epsilon=-1.0, max_iters=1)

    def it_of(corners, shift_pts):
        gpu_ctx.set_image(frame)
        b = mtf_amd.Batch(gpu_ctx, mtf_amd.AM_SSD, mtf_amd.SSM_HOMOGRAPHY, res, res, B)
        b.set_corners(corners)
        b.init_template(sm)
        assert b.grid_regen(sm)
        if shift_pts:
            b.write(L.BUF_INIT_PTS, b.read(L.BUF_INIT_PTS) + 3.0)
            assert not b.grid_regen(sm)
        gpu_ctx.set_image(frame2)
        b.set_state(np.zeros((B, 8)))
        b.iterate(sm)
        it = b.read(L.BUF_IT).copy()
        b.close()
        return it

    on_lattice = it_of(corners, False)
    moved_pts = it_of(corners, True)
    moved_corners = it_of(corners + 3.0, False)
    assert not np.allclose(moved_pts, on_lattice, rtol=1e-6)
    np.testing.assert_allclose(moved_pts, moved_corners, rtol=1e-9, atol=1e-9)


def test_points_follow_new_corners(gpu_ctx, frame, frame2):
    """set_corners with new corners: the rebuilt grid is the new lattice (same bits as a fresh batch on the new corners)"""
    B, res = 91, 100
    c1, c2 = _corners(B, res, seed=8), _corners(B, res, seed=9)
    sm = mtf_amd.sm_desc(mtf_amd.SM_ESM, materialize=1, leven_marq=0, epsilon=-1.0, max_iters=1)

    def it_after(batch, corners):
        gpu_ctx.set_image(frame)
        batch.set_corners(corners)
        batch.init_template(sm)
        assert batch.grid_regen(sm)
        gpu_ctx.set_image(frame2)
        batch.set_state(np.zeros((B, 8)))
        f, g, H = batch.iterate(sm)
        return batch.read(L.BUF_IT).copy(), g, H

    b = mtf_amd.Batch(gpu_ctx, mtf_amd.AM_SSD, mtf_amd.SSM_HOMOGRAPHY, res, res, B)
    it_after(b, c1)
    moved = it_after(b, c2)
    fresh_b = mtf_amd.Batch(gpu_ctx, mtf_amd.AM_SSD, mtf_amd.SSM_HOMOGRAPHY, res, res, B)
    fresh = it_after(fresh_b, c2)
    for x, y in zip(moved, fresh):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    b.close()
    fresh_b.close()
