"""The device RANSAC / LMedS / least-squares estimator of the grid SSM (mtfhip_ssm_estimate_from_pts, csrc/kernels_est.hip) against the
NumPy restatement of the reference (tests/helpers/est_ref.py) over the same hypothesis sequence, and the two grid drivers with est_params.

Discrete outputs (winning hypothesis, walked count, ok, mask, inlier count) are compared exactly, which only means something away from
ties: every compared case first asserts ON THE REFERENCE ALONE that no squared error of a walked hypothesis or of the final mask pass
lies within TIE_THR (relative) of the squared threshold and that no walked LMedS median lies within TIE_MED (relative) of the running
minimum.  A case that violates one raises -- it is a broken test case, not a skip.

Tolerance of the continuous outputs (state update, minMedian, sigma): the reference is run twice on every case, with the eigendecomposition
of LtL (as the reference does) and with an SVD of L itself (affine: lstsq against normal equations); the largest relative difference of
the two state updates over all cases is the floor two legitimate FP64 solvers leave, SOLVER_FLOOR, and the device -- a third solver
(cyclic Jacobi; centred normal equations) with another summation order -- gets T = 100 x that, never less than 1e-12.
SOLVER_FLOOR was measured over CASES and the stopping cases below with the caller-made lists: 1.814e-8, at the refined RANSAC homography of
65 points (the affine cases: 4.9e-9; unrefined fits: below 1e-11 -- the ten LM iterations, which stop on their count and not at the
optimum, carry a start's rounding forward).  test_solver_floor prints the same figure over every case this module ran, device-drawn
lists included, and fails if it has drifted by an order of magnitude (then the constant has to be measured again)."""
import os
import sys

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import host, synth
from mtf_amd.sm import GridTracker

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import est_cases as EC   # noqa: E402
import est_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

TIE_THR, TIE_MED = 1e-5, 1e-6
SOLVER_FLOOR = 1.82e-8      # measured: see the module docstring and test_solver_floor
T = max(100 * SOLVER_FLOOR, 1e-12)
FLOORS = []                 # (case id, eigh-vs-alt relative difference), filled as the cases run

ZERO_UPDATE = {R.HOMOGRAPHY: [-1, 0, 0, 0, -1, 0, 0, 0], R.AFFINE: [0, 0, -1, 0, 0, -1]}


def _scale(ssm):
    # the natural sizes of the parameterisation's entries: linear terms and pixels 1, projective terms 1 / (lattice extent in px)
    return np.array([1, 1, 1, 1, 1, 1, 1 / 400., 1 / 400.]) if ssm == R.HOMOGRAPHY else np.ones(6)


def rel_diff(ssm, a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(b), _scale(ssm))))


def both_params(method, mp, refine, max_iters, thresh=5.0, attempts=300):
    return (L.est_params(method, thresh, mp, refine, max_iters, attempts, 0.995, 10),
            R.Params(method, thresh, mp, refine, max_iters, attempts, 0.995, 10))


def reference(ssm, a, b, rp, subsets, cid):
    """the reference on the case, its tie margins asserted, the solver floor recorded"""
    ref = R.estimate(ssm, a, b, rp, subsets)
    alt = R.estimate(ssm, a, b, rp, subsets, solver="alt")
    m = ref["margins"]
    if not (m["threshold"] > TIE_THR and m["median"] > TIE_MED):
        raise RuntimeError("case %s sits on a tie: threshold margin %.3g, median margin %.3g -- pick another seed" % (cid, m["threshold"], m["median"]))
    if ref["ok"] and alt["ok"] and np.array_equal(ref["mask"], alt["mask"]):
        FLOORS.append((cid, rel_diff(ssm, alt["state_update"], ref["state_update"])))
    return ref


def compare(ssm, got, ref, cid):
    print("%s: ok %d/%d winner %d/%d walked %d/%d inliers %d/%d update diff %.3g (T %.3g)" % (
        cid, got.ok, ref["ok"], got.winner, ref["winner"], got.n_walked, ref["n_walked"], got.n_inliers, ref["n_inliers"],
        rel_diff(ssm, got.state_update, ref["state_update"]), T))
    assert got.ok == ref["ok"] and got.winner == ref["winner"] and got.n_walked == ref["n_walked"], cid
    assert np.array_equal(got.mask, ref["mask"]) and got.n_inliers == ref["n_inliers"], cid
    assert rel_diff(ssm, got.state_update, ref["state_update"]) <= T, cid
    if ref["min_median"] > 0:
        assert abs(got.min_median - ref["min_median"]) <= T * ref["min_median"] and abs(got.sigma - ref["sigma"]) <= T * ref["sigma"], cid
    else:
        assert got.min_median == 0 and got.sigma == 0, cid


# ---- the case table: n_pts x method x refine x SSM, plus the over-determined hypotheses ----
def _cases():
    out = []
    for ssm in (R.HOMOGRAPHY, R.AFFINE):
        mp0 = 4 if ssm == R.HOMOGRAPHY else 3
        for n, s in ((mp0, 2), (9, 3), (65, 9), (100, 10), (257, 17)):
            for method in (R.RANSAC, R.LMEDS, R.LEAST_SQUARES):
                for refine in (0, 1):
                    out.append(dict(ssm=ssm, n=n, s=s, method=method, refine=refine, mp=mp0, frac=0.0 if method == R.LEAST_SQUARES else 0.2))
        out.append(dict(ssm=ssm, n=100, s=10, method=R.RANSAC, refine=1, mp=mp0 + 1, frac=0.2))    # least-squares hypotheses
        out.append(dict(ssm=ssm, n=100, s=10, method=R.LMEDS, refine=1, mp=mp0 + 1, frac=0.2))
    for i, c in enumerate(out):
        c["id"] = "%s-n%d-%s-r%d-mp%d" % ("hom" if c["ssm"] == R.HOMOGRAPHY else "aff", c["n"], ("ransac", "lmeds", "lsq")[c["method"]], c["refine"], c["mp"])
        c["seed"] = 100 + i
    return out


CASES = _cases()


def _points(c, frac=None):
    return EC.make_points(c["ssm"], c["s"], c["seed"], c["frac"] if frac is None else frac, n=c["n"])


def _n_hyp(c, rp):
    if c["method"] == R.LEAST_SQUARES or c["n"] == c["mp"]:
        return 1
    full = rp.max_iters if c["method"] == R.RANSAC else R.lmeds_num_iters(rp.confidence, c["mp"], rp.max_iters)
    return min(full, 40) if c["n"] == 9 else full       # a 3 x 3 lattice has 78 four-point subsets without a collinear triple


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_caller_made_subsets(gpu_ctx, c):
    a, b, _ = _points(c)
    lp, rp = both_params(c["method"], c["mp"], c["refine"], 200)
    n_hyp = _n_hyp(c, rp)
    sub = EC.draw_subsets(c["seed"], a, b, n_hyp, c["mp"]) if c["n"] > c["mp"] else np.arange(c["mp"], dtype=np.int32)[None]
    assert len({tuple(sorted(r)) for r in sub.tolist()}) == len(sub)          # no subset twice, in any order
    ref = reference(c["ssm"], a, b, rp, sub, c["id"])
    got = gpu_ctx.estimate_warp_from_pts(c["ssm"], a, b, lp, subsets=sub)
    compare(c["ssm"], got, ref, c["id"])
    assert np.array_equal(got.subsets, sub)
    if c["n"] == c["mp"] or c["method"] == R.LEAST_SQUARES:
        assert got.mask.all() and got.ok


DRAWN = [c for c in CASES if c["method"] != R.LEAST_SQUARES and c["n"] > c["mp"]]   # (the other paths draw nothing)


@pytest.mark.parametrize("c", DRAWN, ids=[c["id"] for c in DRAWN])
def test_device_drawn_subsets(gpu_ctx, c):
    a, b, _ = _points(c)
    lp, rp = both_params(c["method"], c["mp"], c["refine"], 200)
    # the first seed whose replay through the reference is free of ties (decided on the reference alone)
    err = None
    for seed in range(1, 9):
        got = gpu_ctx.estimate_warp_from_pts(c["ssm"], a, b, lp, seed=seed)
        used = got.subsets[:got.n_walked + (0 if got.n_walked == len(got.subsets) else 1)]
        try:
            ref = reference(c["ssm"], a, b, rp, got.subsets, "%s-seed%d" % (c["id"], seed))
            break
        except RuntimeError as e:
            err = e
    else:
        raise err
    M, m = a.astype(np.float64), b.astype(np.float64)
    for row in used[:got.n_walked]:
        assert (row >= 0).all() and len(set(row.tolist())) == c["mp"], row                     # distinct indices
        assert R.check_subset(M[row]) and R.check_subset(m[row]), row                         # the reference's checkSubset
    compare(c["ssm"], got, ref, c["id"])


@pytest.mark.parametrize("ssm", [R.HOMOGRAPHY, R.AFFINE], ids=["homography", "affine"])
def test_ransac_stopping(gpu_ctx, ssm):
    mp = 4 if ssm == R.HOMOGRAPHY else 3
    # 10 % outliers: the rule stops early
    a, b, _ = EC.make_points(ssm, 10, 41, 0.10)
    lp, rp = both_params(R.RANSAC, mp, 1, 2000)
    sub = EC.draw_subsets(41, a, b, 300, mp)
    ref = reference(ssm, a, b, rp, sub, "stop-early")
    got = gpu_ctx.estimate_warp_from_pts(ssm, a, b, lp, subsets=sub)
    compare(ssm, got, ref, "stop-early")
    assert got.n_walked < 64
    # 60 % outliers, max_iters 70: every hypothesis is walked, and 70 is no multiple of the chunk
    a, b, _ = EC.make_points(ssm, 10, 42, 0.60)
    lp, rp = both_params(R.RANSAC, mp, 1, 70)
    sub = EC.draw_subsets(42, a, b, 70, mp)
    ref = reference(ssm, a, b, rp, sub, "walk-all")
    got = gpu_ctx.estimate_warp_from_pts(ssm, a, b, lp, subsets=sub)
    compare(ssm, got, ref, "walk-all")
    assert got.n_walked == 70


@pytest.mark.parametrize("ssm", [R.HOMOGRAPHY, R.AFFINE], ids=["homography", "affine"])
@pytest.mark.parametrize("method", [R.RANSAC, R.LMEDS], ids=["ransac", "lmeds"])
def test_all_points_on_one_line(gpu_ctx, ssm, method):
    # on one line EXACTLY, also after the rounding to float32: even integer x, y = x / 2 + 20 (a line through rounded coordinates is
    # not one to checkSubset, whose tolerance is FLT_EPSILON of the coordinate differences, and some of its triples would pass)
    x = 100.0 + 10.0 * np.arange(30)
    a = np.stack([x, 0.5 * x + 20], axis=1).astype(np.float32)
    b = (a + np.float32(3.0)).astype(np.float32)
    assert np.array_equal(a.astype(np.float64)[:, 1], 0.5 * x + 20) and not R.check_subset(a[[0, 7, 29]].astype(np.float64))
    lp, _ = both_params(method, 4 if ssm == R.HOMOGRAPHY else 3, 1, 200, attempts=5)
    got = gpu_ctx.estimate_warp_from_pts(ssm, a, b, lp, seed=3)
    assert not got.ok and got.mask.all() and got.n_inliers == 30 and got.n_walked == 0 and got.winner == -1
    assert np.array_equal(got.state_update, ZERO_UPDATE[ssm])
    assert (got.subsets == -1).all()


def test_sets_in_one_call_and_repeats_are_bit_identical(gpu_ctx):
    for ssm in (R.HOMOGRAPHY, R.AFFINE):
        for method in (R.RANSAC, R.LMEDS):
            lp, _ = both_params(method, 4, 1, 200)
            sets = [EC.make_points(ssm, s, 7 + s, 0.2, n=n)[:2] for s, n in ((10, 100), (6, 33), (17, 257))]
            many = gpu_ctx.estimate_warp_from_pts(ssm, [p[0] for p in sets], [p[1] for p in sets], lp, seed=11)
            again = gpu_ctx.estimate_warp_from_pts(ssm, [p[0] for p in sets], [p[1] for p in sets], lp, seed=11)
            for k, (a, b) in enumerate(sets):
                one = gpu_ctx.estimate_warp_from_pts(ssm, a, b, lp, seed=11)
                for other in (many[k], again[k]):
                    assert one.state_update.tobytes() == other.state_update.tobytes() and np.array_equal(one.mask, other.mask)
                    assert (one.ok, one.winner, one.n_walked, one.n_inliers, one.min_median, one.sigma) == \
                        (other.ok, other.winner, other.n_walked, other.n_inliers, other.min_median, other.sigma)
                    assert np.array_equal(one.subsets, other.subsets)
                assert one.ok


def test_argument_errors(gpu_ctx):
    lp, _ = both_params(R.RANSAC, 4, 1, 50)
    pts = np.zeros((3, 2), dtype=np.float32)
    with pytest.raises(mtf_amd.InvalidArgument, match="fewer than n_model_pts"):
        gpu_ctx.estimate_warp_from_pts(R.HOMOGRAPHY, pts, pts, lp)
    big = np.random.default_rng(0).uniform(0, 500, size=(L.EST_MAX_PTS + 1, 2)).astype(np.float32)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="at most 1024"):
        gpu_ctx.estimate_warp_from_pts(R.HOMOGRAPHY, big, big, lp)
    a, b, _ = EC.make_points(R.HOMOGRAPHY, 5, 1, 0.0)
    with pytest.raises(mtf_amd.InvalidArgument, match="subset index"):
        gpu_ctx.estimate_warp_from_pts(R.HOMOGRAPHY, a, b, lp, subsets=np.array([[0, 1, 2, 25]]))
    # 1024 points are supported
    a, b, _ = EC.make_points(R.HOMOGRAPHY, 32, 5, 0.1)
    got = gpu_ctx.estimate_warp_from_pts(R.HOMOGRAPHY, a, b, lp, seed=2)
    assert got.ok and got.n_inliers >= 900


def test_solver_floor():
    """runs after the cases above: the eigh-vs-SVD (lstsq-vs-normal-equations) distance over every case they touched, against SOLVER_FLOOR"""
    assert FLOORS, "no case ran before this one"
    worst = max(FLOORS, key=lambda t: t[1])
    print("solver floor over %d cases: %.3g at %s (SOLVER_FLOOR %.3g, T %.3g)" % (len(FLOORS), worst[1], worst[0], SOLVER_FLOOR, T))
    assert worst[1] <= 10 * SOLVER_FLOOR, worst


# ---- the grid drivers with est_params ----
CENTRE = (256.0, 256.0)
REGION = synth.square_corners(CENTRE[0], CENTRE[1], 280)


def _frames(frame, n, seed):   # the synthetic video of tests/test_gpu_grid.py
    rng = np.random.default_rng(seed)
    out, cur = [], frame
    for _ in range(n):
        cur = synth.warp_frame(cur, synth.random_small_homography(rng, 0.15), CENTRE)
        out.append(cur)
    return out


EST = {"ransac": (R.RANSAC, 5.0, 4, True, 2000, 300, 0.995, 10), "lmeds": (R.LMEDS, 5.0, 4, True, 10000, 300, 0.995, 10)}   # lmeds: Config/modules.cfg:37-45


@pytest.mark.parametrize("fb_err_thresh", [0.0, 2.0])
@pytest.mark.parametrize("est", sorted(EST))
@pytest.mark.parametrize("driver", ["python", "cpp"])
def test_grid_drivers_with_est_params(gpu_ctx, frame, driver, est, fb_err_thresh):
    gs, ps = 6, 25
    lp, rp = L.est_params(*EST[est]), R.Params(*EST[est])
    kw = dict(grid_size=gs, patch_size=ps, max_iters=20, epsilon=1e-4, reset_at_each_frame=1, grid_ssm=L.SSM_HOMOGRAPHY, fb_err_thresh=fb_err_thresh,
              est_params=lp, est_seed=5)
    if driver == "python":
        gpu_ctx.set_image(frame)
        g = GridTracker(gpu_ctx, am=L.AM_NCC, ssm=L.SSM_AFFINE, **kw)
    else:
        g = host.CppGridTracker(patch_sm=L.SM_ICLK, patch_am=L.AM_NCC, patch_ssm=L.SSM_AFFINE, hess_type=0, **kw)
        g.set_image(frame)
    g.initialize(REGION)
    region = REGION.copy()
    for k, f in enumerate(_frames(frame, 2, 77)):
        if driver == "python":
            gpu_ctx.set_image(f)
            g.update()
            a, b, seed = g.est_in_pts, g.est_out_pts, 5 + k
            upd, pix_mask, ok, fb_mask = g.ssm_update, g.pix_mask, g.est_ok, g.fb_err_mask
        else:
            g.set_image(f)
            g.update()
            a, b, seed = g.est_pairs()
            upd, pix_mask, ok, fb_mask = g.ssm_update(), g.pix_mask(), g.est_ok, g.fb_err_mask() if fb_err_thresh > 0 else None
        assert seed == 5 + k
        # the fit the driver made, again through the entry point (bit-identical), for the subsets it drew
        rep = gpu_ctx.estimate_warp_from_pts(L.SSM_HOMOGRAPHY, a, b, lp, seed=seed)
        assert rep.state_update.tobytes() == np.asarray(upd, dtype=np.float64).tobytes() and rep.ok == ok
        ref = reference(R.HOMOGRAPHY, a, b, rp, rep.subsets, "grid-%s-%s-fb%g-frame%d" % (driver, est, fb_err_thresh, k))
        compare(R.HOMOGRAPHY, rep, ref, "grid")
        want_mask = ref["mask"]
        if fb_err_thresh > 0:                                  # GridTracker.cc:335-340
            assert len(a) == int(np.count_nonzero(fb_mask))
            full = np.zeros(gs * gs, dtype=np.uint8)
            full[np.asarray(fb_mask, dtype=bool)] = want_mask
            want_mask = full
        else:
            assert len(a) == gs * gs
        assert np.array_equal(np.asarray(pix_mask, dtype=np.uint8), want_mask)
        region = mtf_amd.apply_warp_to_pts(L.SSM_HOMOGRAPHY, region, ref["state_update"])
        np.testing.assert_allclose(g.get_region(), region, rtol=0, atol=400 * T + 1e-9)
        region = g.get_region()
    if driver == "python":
        g.tracker.batch.close()
