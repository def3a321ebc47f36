"""GPU: the additive Lucas-Kanade search methods nt::FALK / nt::IALK on the device (MTFHIP_SM_FALK / _IALK: k_alk_pass + k_alk_finish behind
mtfhip_batch_init_template / _iterate / _track) against the restatement of the reference over the oracle (tests/helpers/alk_ref.py), against
the per-function route (nt::FALK / nt::IALK of the harness over HipAM / HipSSM) and against themselves (loop = single passes, batch = single
targets, packed = padded frame, call = call).

Tolerances are the existing tests' for FCLK, cited where they are used; nothing here is looser."""
import os
import sys

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import alk_cases as AC   # noqa: E402
import alk_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

METHODS = [L.SM_FALK, L.SM_IALK]
SIZE_IDS = ["%dx%d" % s for s in AC.SIZES]
# final / per-pass corners of a device loop against the CPU tracker: tests/test_gpu_trackers.py:378 (FCLK among its cases) and
# tests/test_gpu_parity.py:565 (every pass of the trace), both atol = 2e-4 pixels
TOL_CORNERS = 2e-4


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.linalg.norm(a - b)
    n = np.linalg.norm(b)
    return d / n if n > 0 else d


def c24(c8):
    return np.asarray(c8).reshape(4, 2).T


def oracle_grid(b, o_ssm):
    """the device gets the oracle's sample grid verbatim (tests/test_gpu_parity.py:311-316): every per-pixel quantity is then computed from
    identical inputs"""
    hm = o_ssm.get("init_pts_hm").reshape(-1, 3)
    b.write(L.BUF_INIT_PTS, o_ssm.get("init_pts").reshape(1, -1, 2).transpose(0, 2, 1))
    b.write(L.BUF_INIT_HXY, hm[:, :2].T[None])
    b.write(L.BUF_INIT_Z, hm[:, 2][None])
    b.set_state(np.zeros((1, b.S)))


def start_state(ssm):
    return AC.batch_start(ssm, 1)


# ------------------------------------------------------------------ one pass against the oracle
@pytest.mark.parametrize("size", AC.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("ssm", [AC.HOM, AC.AFF], ids=["hom", "aff"])
@pytest.mark.parametrize("am", [AC.SSD, AC.NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("method", METHODS, ids=AC.name)
def test_one_pass_parity(oracle, gpu_ctx, method, am, ssm, size):
    """One materialising iterate away from the identity state, on the oracle's grid: It, dIt_dx (FALK) and Jt equal the oracle's bit for bit
    (replay arithmetic), f, g, H and the update follow at the bounds tests/test_gpu_parity.py:383-386 sets for FCLK on the oracle's grid
    (only the order of the N-wide sums differs): f 1e-12, H 1e-9, g 1e-10 of its scale, the update 1e-6 relative or 1e-12 absolute."""
    frame0, frame1 = AC.frame0(), AC.warped(AC.warp_of(ssm))
    o_ssm = oracle.SSM(ssm, *size); o_am = oracle.AM(am, *size); o_am.set_curr_img(frame0)
    ref = R.AlkRef(method, o_am, o_ssm, hess_type=0, max_iters=1)
    ref.initialize(AC.REGION)
    gpu_ctx.set_image(frame0)
    b = mtf_amd.Batch(gpu_ctx, am, ssm, size[0], size[1], 1)
    try:
        b.set_corners(AC.REGION[None])
        oracle_grid(b, o_ssm)
        for ht in (0, 1, 2):
            ref.p["hess_type"] = ht
            sm = mtf_amd.sm_desc(method, materialize=1, hess_type=ht, max_iters=1)
            if ht == 0:
                b.init_template(sm)
                assert np.array_equal(b.read(L.BUF_I0)[0], o_am.get("I0"))
                assert np.array_equal(b.read(L.BUF_DI0_DX)[0], o_am.get("dI0_dx").reshape(2, -1).T)
                o_am.set_curr_img(frame1); gpu_ctx.set_image(frame1)
            p0 = start_state(ssm)
            o_ssm.set_state(p0); b.set_state(p0[None])
            rec = ref.update()["log"][0]
            f, g, H = b.iterate(sm)
            S = b.S
            assert np.array_equal(b.read(L.BUF_IT)[0], rec["It"]), ht
            assert np.array_equal(b.read(L.BUF_JT)[0], rec["Jt"].reshape(S, -1).T), ht
            if method == L.SM_FALK:
                assert np.array_equal(b.read(L.BUF_DIT_DX)[0], rec["dIt_dx"].reshape(2, -1).T), ht
            dp = -oracle.colpiv_qr_solve(H[0], g[0])
            g_scale = np.sqrt(abs(np.trace(rec["H"]))) * (np.sqrt(abs(2 * rec["f"])) if am == AC.SSD else 1.0)
            e = dict(f=rel(f[0], rec["f"]), H=rel(H[0], rec["H"]), g=float(np.linalg.norm(g[0] - rec["g"]) / max(np.linalg.norm(rec["g"]), g_scale)),
                     dp=rel(dp, rec["dp"]), dp_abs=float(np.abs(dp - rec["dp"]).max()))
            print("one_pass %s am %d ssm %d %s ht %d: %s" % (AC.name(method), am, ssm, size, ht, e))
            assert e["f"] < 1e-12, (ht, e)
            assert e["H"] < 1e-9, (ht, e)
            assert e["g"] < 1e-10, (ht, e)
            assert e["dp"] < 1e-6 or e["dp_abs"] < 1e-12, (ht, e)
    finally:
        b.close()


# ------------------------------------------------------------------ the device loop against the reference
def run_device_loop(ctx, method, am, ssm, size, frame0, frame1, region, start=None, trace=0, **params):
    ctx.set_image(frame0)
    b = mtf_amd.Batch(ctx, am, ssm, size[0], size[1], 1)
    try:
        b.set_corners(np.asarray(region)[None])
        sm = mtf_amd.sm_desc(method, **params)
        b.init_template(sm)
        if start is not None:
            b.set_state(np.asarray(start)[None])
        ctx.set_image(frame1)
        if trace:
            b.track_trace(trace)
        n_it, corners = b.track(sm)
        recs = b.read_track_trace(n_it)[0] if trace else None
        return int(n_it[0]), corners[0].copy(), b.get_state()[0].copy(), recs
    finally:
        b.close()


def check_against_reference(oracle, ssm, size, region, res, n_it, corners, state, recs, start=None):
    log = res["log"]
    assert n_it == res["n_iters"], (n_it, res["n_iters"])
    np.testing.assert_allclose(corners, c24(res["corners"]), rtol=0, atol=TOL_CORNERS)
    assert len(recs) == len(log)
    o = oracle.SSM(ssm, *size)
    s = np.zeros(len(state)) if start is None else np.asarray(start, dtype=np.float64).copy()
    for k, (d, r) in enumerate(zip(recs, log)):
        assert d["undo"] == r["undo"], k
        np.testing.assert_allclose(d["corners"], c24(r["corners"]), rtol=0, atol=TOL_CORNERS, err_msg="pass %d" % k)
        # the state of the pass: the updates applied so far, added up as the device adds them (an undo adds the negative); compared through
        # its image of the region's corners, at the corners' own tolerance
        s = s + (-d["dp"] if d["undo"] else d["dp"])
        np.testing.assert_allclose(o.apply_warp_to_corners(region, s), c24(r["corners"]), rtol=0, atol=TOL_CORNERS, err_msg="state, pass %d" % k)
    assert np.array_equal(s, state)      # what the loop left in the SSM is the sum of what it applied, bit for bit


@pytest.mark.parametrize("lm", [0, 1], ids=["gn", "lm"])
@pytest.mark.parametrize("ht", [0, 1, 2], ids=["initial_self", "current_self", "std"])
@pytest.mark.parametrize("method", METHODS, ids=AC.name)
def test_device_loop_follows_reference_ssd(oracle, gpu_ctx, method, ht, lm):
    """mtfhip_batch_track against alk_ref: every hess_type, Levenberg-Marquardt off and on, SSD + homography on the 37 x 23 patch and the
    warp of the Levenberg-Marquardt cases -- with InitialSelf and Levenberg-Marquardt the case test_alk_ref.py shows to reject steps.
    Undamped Gauss-Newton with the InitialSelf Hessian does not converge on that warp (the reference runs into max_iters, FALK 3.6 pixels
    off): a loop that does not contract keeps no fixed distance between two trajectories that start 1e-13 pixels apart, so that one
    combination takes the small homography of the other tests, on which the reference stops by epsilon like the rest."""
    c = AC.LM_CASES[method]
    params = dict(hess_type=ht, leven_marq=lm, lm_delta_init=c["lm_delta_init"], lm_delta_update=10.0, max_iters=c["max_iters"], epsilon=c["epsilon"])
    frame0, frame1 = AC.frame0(), AC.warped(AC.P_HOM if (ht == 0 and not lm) else c["p"])
    ref, res = R.track(oracle, method, AC.SSD, AC.HOM, 37, 23, frame0, frame1, AC.REGION, **params)
    assert res["n_iters"] < c["max_iters"]      # the reference stops by epsilon
    if lm and ht == 0:
        assert sum(r["undo"] for r in res["log"]) >= 1
    out = run_device_loop(gpu_ctx, method, AC.SSD, AC.HOM, (37, 23), frame0, frame1, AC.REGION, trace=c["max_iters"], materialize=0, **params)
    print("device_loop %s ht %d lm %d: n_iters %d (ref %d), undo %s, final corner diff %.3e" % (
        AC.name(method), ht, lm, out[0], res["n_iters"], "".join(str(int(r["undo"])) for r in res["log"]), np.abs(out[1] - c24(res["corners"])).max()))
    check_against_reference(oracle, AC.HOM, (37, 23), AC.REGION, res, *out)


@pytest.mark.parametrize("size", AC.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("lm", [0, 1], ids=["gn", "lm"])
@pytest.mark.parametrize("am,ssm,ht", [(AC.NCC, AC.AFF, 0), (AC.NCC, AC.HOM, 2), (AC.NCC, AC.AFF, 1), (AC.SSD, AC.AFF, 2)],
                         ids=["ncc_aff_initial_self", "ncc_hom_std", "ncc_aff_current_self", "ssd_aff_std"])
@pytest.mark.parametrize("method", METHODS, ids=AC.name)
def test_device_loop_follows_reference(oracle, gpu_ctx, method, am, ssm, ht, lm, size):
    """... NCC and the affine SSM, the three patch sizes, on the known small warps"""
    params = dict(hess_type=ht, leven_marq=lm, lm_delta_init=0.01, lm_delta_update=10.0, max_iters=12, epsilon=1e-4)
    frame0, frame1 = AC.frame0(), AC.warped(AC.warp_of(ssm))
    ref, res = R.track(oracle, method, am, ssm, size[0], size[1], frame0, frame1, AC.REGION, **params)
    out = run_device_loop(gpu_ctx, method, am, ssm, size, frame0, frame1, AC.REGION, trace=12, materialize=1, **params)
    print("device_loop %s am %d ssm %d ht %d lm %d %s: n_iters %d (ref %d), final corner diff %.3e" % (
        AC.name(method), am, ssm, ht, lm, size, out[0], res["n_iters"], np.abs(out[1] - c24(res["corners"])).max()))
    check_against_reference(oracle, ssm, size, AC.REGION, res, *out)


# ------------------------------------------------------------------ the loop against its own single passes
@pytest.mark.parametrize("am,ssm,size", [(AC.SSD, AC.HOM, (50, 50)), (AC.NCC, AC.AFF, (37, 23)), (AC.SSD, AC.AFF, (7, 5))], ids=["ssd_hom_50", "ncc_aff_37x23", "ssd_aff_7x5"])
@pytest.mark.parametrize("method", METHODS, ids=AC.name)
def test_device_loop_equals_single_passes_from_the_host(gpu_ctx, method, am, ssm, size):
    """mtfhip_batch_track with max_iters = n against n calls that each run one pass and its finish (max_iters = 1), and the reduced sums of
    every pass against mtfhip_batch_iterate at the state the pass ran at: bit for bit"""
    frame0, frame1 = AC.frame0(), AC.warped(AC.warp_of(ssm))
    params = dict(hess_type=1, leven_marq=0, epsilon=1e-4, materialize=1)
    n_it, corners, state, recs = run_device_loop(gpu_ctx, method, am, ssm, size, frame0, frame1, AC.REGION, trace=12, max_iters=12, **params)
    assert 2 <= n_it < 12
    gpu_ctx.set_image(frame0)
    b = mtf_amd.Batch(gpu_ctx, am, ssm, size[0], size[1], 1)
    try:
        b.set_corners(AC.REGION[None])
        one = mtf_amd.sm_desc(method, max_iters=1, **params)
        b.init_template(one)
        gpu_ctx.set_image(frame1)
        for k in range(n_it):
            f, g, H = b.iterate(one)
            assert np.array_equal(g[0], recs[k]["g"]) and np.array_equal(H[0], recs[k]["H"]), k
            if am == AC.SSD:
                assert f[0] == recs[k]["f"], k
            n1, c1 = b.track(one)
            assert int(n1[0]) == 1
            assert np.array_equal(c1[0], recs[k]["corners"]), k
        assert np.array_equal(c1[0], corners) and np.array_equal(b.get_state()[0], state)
        assert np.array_equal(b.get_corners()[0], corners)
    finally:
        b.close()


# ------------------------------------------------------------------ the device loop against the per-function route
@pytest.mark.parametrize("am,ssm,size,lm", [(AC.SSD, AC.HOM, (37, 23), 1), (AC.NCC, AC.AFF, (50, 50), 0), (AC.SSD, AC.AFF, (7, 5), 0), (AC.NCC, AC.HOM, (37, 23), 0)],
                         ids=["ssd_hom_37x23_lm", "ncc_aff_50", "ssd_aff_7x5", "ncc_hom_37x23"])
@pytest.mark.parametrize("method", METHODS, ids=AC.name)
def test_device_loop_against_the_harness(gpu_ctx, method, am, ssm, size, lm):
    """nt::FALK / nt::IALK of the harness over HipAM / HipSSM -- one C-ABI call per reference virtual, the solve and the update on the host --
    and the device loop: the same n_iters, corners within the device-loop tolerance.  The Levenberg-Marquardt case is the one with rejected
    steps."""
    from mtf_amd.host import CppTracker
    if lm:
        c = AC.LM_CASES[method]
        params = dict(hess_type=0, leven_marq=1, lm_delta_init=c["lm_delta_init"], lm_delta_update=10.0, max_iters=c["max_iters"], epsilon=c["epsilon"])
        frame1 = AC.warped(c["p"])
    else:
        params = dict(hess_type=0, leven_marq=0, lm_delta_init=0.01, lm_delta_update=10.0, max_iters=12, epsilon=1e-4)
        frame1 = AC.warped(AC.warp_of(ssm))
    frame0 = AC.frame0()
    n_it, corners, state, _ = run_device_loop(gpu_ctx, method, am, ssm, size, frame0, frame1, AC.REGION, materialize=0, **params)
    trk = CppTracker(method, am=am, ssm=ssm, resx=size[0], resy=size[1], **params)
    trk.set_image(frame0)
    trk.initialize(AC.REGION)
    trk.set_image(frame1)
    region = trk.update()
    print("harness %s am %d ssm %d %s lm %d: n_iters %d / %d, corner diff %.3e" % (AC.name(method), am, ssm, size, lm, n_it, trk.iters, np.abs(region - corners).max()))
    assert trk.iters == n_it
    np.testing.assert_allclose(corners, region, rtol=0, atol=TOL_CORNERS)


@pytest.mark.parametrize("method", METHODS, ids=AC.name)
def test_cpp_device_driver_equals_python(gpu_ctx, method):
    """mtf::hip::LK (C++, one mtfhip_batch_track per update()) and sm.LKTracker(host_solve=False): the same call, the same bits"""
    from mtf_amd.host import CppTracker
    from mtf_amd.sm import LKTracker
    params = dict(hess_type=2, leven_marq=0, max_iters=10, epsilon=1e-4)
    frame0, frame1 = AC.frame0(), AC.warped(AC.P_HOM)
    trk = CppTracker(method, am=AC.NCC, ssm=AC.HOM, resx=37, resy=23, device_loop=True, **params)
    trk.set_image(frame0); trk.initialize(AC.REGION); trk.set_image(frame1)
    region = trk.update()
    gpu_ctx.set_image(frame0)
    py = LKTracker(gpu_ctx, method, ssm=AC.HOM, resx=37, resy=23, n_targets=1, host_solve=False, am=AC.NCC, materialize=0, **params)
    try:
        py.initialize(AC.REGION[None])
        gpu_ctx.set_image(frame1)
        out = py.update()
        assert int(py.n_iters[0]) == trk.iters and 2 <= trk.iters < 10
        assert np.array_equal(out[0], region)
    finally:
        py.batch.close()


def test_host_solve_driver_follows_reference(oracle, gpu_ctx):
    """sm.LKTracker(host_solve=True) -- mtfhip_batch_iterate per pass, the solve and additiveUpdate on the host -- and sm.NTSearchMethod over
    the per-function entry points land where the reference does"""
    from mtf_amd.sm import LKTracker, NTSearchMethod
    params = dict(hess_type=0, leven_marq=0, max_iters=12, epsilon=1e-4)
    frame0, frame1 = AC.frame0(), AC.warped(AC.P_HOM)
    for method in METHODS:
        ref, res = R.track(oracle, method, AC.SSD, AC.HOM, 37, 23, frame0, frame1, AC.REGION, **params)
        for cls in (LKTracker, NTSearchMethod):
            gpu_ctx.set_image(frame0)
            t = cls(gpu_ctx, method, ssm=AC.HOM, resx=37, resy=23, n_targets=1, am=AC.SSD, **params)
            try:
                t.initialize(AC.REGION[None])
                gpu_ctx.set_image(frame1)
                np.testing.assert_allclose(t.update()[0], c24(res["corners"]), rtol=0, atol=TOL_CORNERS)
            finally:
                t.batch.close()


# ------------------------------------------------------------------ a batch whose targets stop behind different passes
@pytest.mark.parametrize("method,am,ssm", [(L.SM_FALK, AC.SSD, AC.HOM), (L.SM_IALK, AC.NCC, AC.AFF)], ids=["FALK_ssd_hom", "IALK_ncc_aff"])
def test_batch_of_three(oracle, gpu_ctx, method, am, ssm):
    size = (50, 50)
    refs = AC.batch_reference(method, am, ssm, size)
    n_ref = [r["n_iters"] for r in refs]
    assert len(set(n_ref)) == 3, n_ref          # asserted on the reference first: they stop behind different passes
    frame0, frame1 = AC.frame0(), AC.warped(AC.P_HOM)
    sm = mtf_amd.sm_desc(method, materialize=1, **AC.BATCH_PARAMS)
    starts = np.stack([AC.batch_start(ssm, t) for t in range(3)])

    def run(targets):
        gpu_ctx.set_image(frame0)
        b = mtf_amd.Batch(gpu_ctx, am, ssm, size[0], size[1], len(targets))
        try:
            b.set_corners(AC.BATCH_REGIONS[targets])
            b.init_template(sm)
            b.set_state(starts[targets])
            gpu_ctx.set_image(frame1)
            b.track_trace(AC.BATCH_PARAMS["max_iters"])
            n_it, corners = b.track(sm)
            return n_it.copy(), corners.copy(), b.get_state().copy(), b.read_track_trace(n_it), b.read(L.BUF_IT).copy()
        finally:
            b.close()
    n_it, corners, states, recs, It = run([0, 1, 2])
    assert list(n_it) == n_ref
    for t in range(3):
        np.testing.assert_allclose(corners[t], c24(refs[t]["corners"]), rtol=0, atol=TOL_CORNERS)
        # a stopped target does not move in the passes the others still run: its state is the sum of the updates of its own passes
        s = starts[t].copy()
        for d in recs[t]:
            s = s + d["dp"]
        assert np.array_equal(s, states[t]) and np.array_equal(recs[t][-1]["corners"], corners[t])
        # ... and the batch does what the target does alone, bit for bit (the interface arrays of its last pass included)
        n1, c1, s1, r1, It1 = run([t])
        assert int(n1[0]) == int(n_it[t])
        assert np.array_equal(c1[0], corners[t]) and np.array_equal(s1[0], states[t]) and np.array_equal(It1[0], It[t])


# ------------------------------------------------------------------ the frame's border, pitch and origin
@pytest.mark.parametrize("ssm", [AC.HOM, AC.AFF], ids=["hom", "aff"])
@pytest.mark.parametrize("method", METHODS, ids=AC.name)
def test_border_and_frame_layout(oracle, gpu_ctx, method, ssm):
    """Five targets on the 96 x 160 frame of test_gpu_frame_layout.py -- one inside, one across each border -- tracked on the packed upload
    and on the same pixels borrowed as a padded, offset view of a poisoned tensor (mtfhip_image_borrow): the same bits, the border value 128
    in every patch that leaves the frame, never a padding value; and the target across the left border lands where the reference does"""
    import torch
    import test_frame_layout_cpu as FL
    views = FL.views()
    parents = {k: torch.from_numpy(FL.place(v)).to("cuda:0") for k, v in views.items() if k in ("a", "b")}
    torch.cuda.synchronize()
    res = FL.RES[1]
    states = FL.small_states(ssm)
    params = dict(hess_type=1, leven_marq=0, max_iters=8, epsilon=1e-4)
    sm = mtf_amd.sm_desc(method, materialize=1, **params)

    def run(padded):
        def set_img(name):
            if padded:
                gpu_ctx.set_image_device(parents[name].data_ptr() + 4 * (FL.R0 * FL.PW + FL.C0), views[name].shape[0], views[name].shape[1], FL.PW, keep=parents[name])
            else:
                gpu_ctx.set_image(views[name])
        set_img("a")
        b = mtf_amd.Batch(gpu_ctx, AC.SSD, ssm, res[0], res[1], FL.B)
        try:
            b.set_corners(FL.targets())
            b.init_template(sm)
            out = dict(I0=b.read(L.BUF_I0).copy(), dI0_dx=b.read(L.BUF_DI0_DX).copy())
            set_img("b")
            b.set_state(states)
            f, g, H = b.iterate(sm)
            out.update(f=f, g=g, H=H, It1=b.read(L.BUF_IT).copy(), Jt1=b.read(L.BUF_JT).copy())
            n_it, corners = b.track(sm)
            out.update(n_it=n_it.copy(), corners=corners.copy(), It=b.read(L.BUF_IT).copy(), Jt=b.read(L.BUF_JT).copy())
            if method == L.SM_FALK:
                out["dIt_dx"] = b.read(L.BUF_DIT_DX).copy()
            return out
        finally:
            b.close()
    try:
        want, got = run(False), run(True)
    finally:
        gpu_ctx.set_image(views["a"])
    for k in sorted(want):
        assert np.array_equal(want[k], got[k]), k
    for k in ("I0", "It1"):
        assert want[k].max() < 1e3 and np.all(want[k][0] != 128.0)
        assert all((want[k][t] == 128.0).any() for t in range(1, FL.B)), k
    # the target across the left border against the reference
    t = 1
    o_ssm = oracle.SSM(ssm, *res); o_am = oracle.AM(AC.SSD, *res); o_am.set_curr_img(views["a"])
    ref = R.AlkRef(method, o_am, o_ssm, **params)
    ref.initialize(FL.targets()[t])
    o_ssm.set_state(states[t]); o_am.set_curr_img(views["b"])
    r = ref.update()
    assert (r["log"][0]["It"] == 128.0).any()
    assert int(want["n_it"][t]) == r["n_iters"]
    np.testing.assert_allclose(want["corners"][t], c24(r["corners"]), rtol=0, atol=TOL_CORNERS)


# ------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("am", [AC.SSD, AC.NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("method", METHODS, ids=AC.name)
def test_two_identical_calls_are_bit_identical(gpu_ctx, method, am):
    frame0, frame1 = AC.frame0(), AC.warped(AC.P_HOM)
    outs = [run_device_loop(gpu_ctx, method, am, AC.HOM, (50, 50), frame0, frame1, AC.REGION, trace=10, hess_type=2, leven_marq=1, max_iters=10, epsilon=1e-5,
                            materialize=1) for _ in range(2)]
    assert outs[0][0] == outs[1][0] and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    for a, b in zip(outs[0][3], outs[1][3]):
        for k in ("H", "g", "dp", "corners"):
            assert np.array_equal(a[k], b[k]), k
        assert a["f"] == b["f"]


# ------------------------------------------------------------------ refusals
def test_refusals(gpu_ctx):
    frame0 = AC.frame0()
    gpu_ctx.set_image(frame0)
    for method in METHODS:
        nm = AC.name(method)
        sm = mtf_amd.sm_desc(method, max_iters=3)
        for am, word in ((L.AM_MI, "MI"), (L.AM_SCV, "SCV"), (L.AM_RSCV, "RSCV"), (L.AM_LSCV, "LSCV"), (L.AM_LRSCV, "LRSCV")):
            b = mtf_amd.Batch(gpu_ctx, am, L.SSM_HOMOGRAPHY, 20, 20, 1)
            try:
                b.set_corners(AC.REGION[None])
                for call in (lambda: b.init_template(sm), lambda: b.iterate(sm), lambda: b.track(sm)):
                    with pytest.raises(mtf_amd.FunctionNotImplemented, match=r"%s with %s is not available on the device route" % (nm, word)):
                        call()
            finally:
                b.close()
        b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_AFFINE, 20, 20, 1)
        try:
            b.set_corners(AC.REGION[None])
            with pytest.raises(mtf_amd.FunctionNotImplemented, match=r"%s with sec_ord_hess is not available" % nm):
                b.init_template(mtf_amd.sm_desc(method, sec_ord_hess=1))
            with pytest.raises(mtf_amd._lib.MtfHipError, match="hess_type 3 invalid"):
                b.init_template(mtf_amd.sm_desc(method, hess_type=3))
            b.init_template(sm)
            with pytest.raises(mtf_amd.FunctionNotImplemented, match=r"%s with sec_ord_hess is not available" % nm):
                b.track(mtf_amd.sm_desc(method, sec_ord_hess=1))
            # the search method's setRegion and the region form of the loop belong to the compositional methods
            for call in (lambda: b.set_region(AC.REGION[None], sm), lambda: b.track_region(AC.REGION[None], sm)):
                with pytest.raises(mtf_amd.FunctionNotImplemented, match=r"additive search methods \(FALK / IALK\)"):
                    call()
        finally:
            b.close()
    # n_channels = 3
    gpu_ctx.set_image(synth.make_frame_mc(AC.H, AC.W, seed=11))
    try:
        for method in METHODS:
            b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, 20, 20, 1, n_channels=3)
            try:
                b.set_corners(AC.REGION[None])
                with pytest.raises(mtf_amd.FunctionNotImplemented, match=r"%s with n_channels 3 is not available" % AC.name(method)):
                    b.init_template(mtf_amd.sm_desc(method))
            finally:
                b.close()
    finally:
        gpu_ctx.set_image(frame0)


@pytest.mark.parametrize("method", METHODS, ids=AC.name)
def test_grid_frame_is_refused(gpu_ctx, method):
    """the grid tracker's one-launch frame with an additive search method: refused with its reason, with and without a region, and the batch
    stays usable"""
    gpu_ctx.set_image(AC.frame0())
    gd = L.GridDesc(2, 2, 20, 20, 0, 0, 1)
    b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_AFFINE, 20, 20, 4)
    try:
        iclk = mtf_amd.sm_desc(L.SM_ICLK, max_iters=3)
        b.grid_reset(gd, iclk, AC.REGION, 1)
        sm = mtf_amd.sm_desc(method, max_iters=3)
        for region in (AC.REGION, None):
            with pytest.raises(mtf_amd.FunctionNotImplemented, match=r"additive search methods \(FALK / IALK\).*grid frames"):
                b.grid_frame(gd, sm, region)
        with pytest.raises(mtf_amd.FunctionNotImplemented, match=r"additive search methods \(FALK / IALK\)"):
            b.grid_reset(gd, sm, AC.REGION, 1)
        n, c, cen = b.grid_frame(gd, iclk, AC.REGION)
        assert np.isfinite(c).all()
    finally:
        b.close()


# ------------------------------------------------------------------ the loop skeleton the additive methods share with track_core
# (api_track.hip: slab upload, Levenberg-Marquardt state, the look at the stop flags every eighth pass, read-back).  Three targets, an 11 x 9
# patch (99 pixels: no multiple of the block size), ten passes and a convergence threshold no update falls below, so that the look at
# the flags behind pass 8 is taken and finds every target active.  CurrentSelf Hessian: InitialSelf's constant Hessian is a host
# reduction whose summation order follows the read-back transport (test_gpu_trackers.py::test_copy_and_sync_fallback_gives_the_same_results).
SKEL_SIZE = (11, 9)
SKEL_ITERS = 10
SKEL_EPS = 1e-30
SKEL_CASES = [(m, am, lm) for m in METHODS for am in (AC.SSD, AC.NCC) for lm in (0, 1)]
SKEL_IDS = ["%s_%s_%s" % (AC.name(m), "ssd" if am == AC.SSD else "ncc", "lm" if lm else "gn") for m, am, lm in SKEL_CASES]


def skeleton_run(ctx, method, am, lm, epsilon=SKEL_EPS, trace=False):
    sm = mtf_amd.sm_desc(method, hess_type=1, leven_marq=lm, max_iters=SKEL_ITERS, epsilon=epsilon)
    ctx.set_image(AC.frame0())
    b = mtf_amd.Batch(ctx, am, AC.HOM, SKEL_SIZE[0], SKEL_SIZE[1], 3)
    try:
        b.set_corners(AC.BATCH_REGIONS)
        b.init_template(sm)
        b.set_state(np.stack([AC.batch_start(AC.HOM, t) for t in range(3)]))
        ctx.set_image(AC.warped(AC.P_HOM))
        if trace:
            b.track_trace(SKEL_ITERS)
        n_it, corners = b.track(sm)
        recs = b.read_track_trace(n_it) if trace else None
        return n_it.copy(), corners.copy(), b.get_state().copy(), recs
    finally:
        b.close()


@pytest.mark.parametrize("method,am,lm", SKEL_CASES, ids=SKEL_IDS)
def test_loop_skeleton_copy_and_sync_transport(gpu_ctx, monkeypatch, method, am, lm):
    """A batch created under MTFHIP_ZERO_COPY=0 (slab up by hipMemcpyAsync, back by copy + synchronisation) gives the corners, n_iters and
    final state of a default batch (ingest and publish kernels), bit for bit."""
    want = skeleton_run(gpu_ctx, method, am, lm)
    monkeypatch.setenv("MTFHIP_ZERO_COPY", "0")
    got = skeleton_run(gpu_ctx, method, am, lm)
    print("skeleton transport: n_iters %s / %s, max |d corners| %.3e, max |d state| %.3e" % (want[0], got[0], np.abs(want[1] - got[1]).max(),
                                                                                            np.abs(want[2] - got[2]).max()))
    assert list(want[0]) == [SKEL_ITERS] * 3      # no target stopped: the flags were looked at behind pass 8 and the loop went on
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2])


@pytest.mark.parametrize("method,am,lm", SKEL_CASES, ids=SKEL_IDS)
def test_loop_skeleton_trace_is_reproducible(gpu_ctx, method, am, lm):
    """With mtfhip_batch_track_trace on, the recorded passes equal those of the same call on a second batch, bit for bit"""
    a, b = skeleton_run(gpu_ctx, method, am, lm, trace=True), skeleton_run(gpu_ctx, method, am, lm, trace=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for t in range(3):
        assert len(a[3][t]) == len(b[3][t]) == int(a[0][t]) > 8
        for ra, rb in zip(a[3][t], b[3][t]):
            for k in ("H", "g", "dp", "corners"):
                assert np.array_equal(ra[k], rb[k]), (t, k)
            assert ra["f"] == rb["f"] and ra["undo"] == rb["undo"] and ra["lm_delta"] == rb["lm_delta"] and ra["has_H"] == rb["has_H"], t


@pytest.mark.parametrize("method,am,lm", SKEL_CASES, ids=SKEL_IDS)
def test_loop_skeleton_runs_every_pass_without_a_threshold(gpu_ctx, method, am, lm):
    """epsilon = 0: nothing can stop a target, so every target reports max_iters passes -- a look at the flags that ended the loop when it
    should not would leave fewer"""
    n_it, corners, states, _ = skeleton_run(gpu_ctx, method, am, lm, epsilon=0.0)
    assert list(n_it) == [SKEL_ITERS] * 3
    assert np.isfinite(corners).all() and np.isfinite(states).all()
