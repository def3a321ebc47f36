"""The HIP CCRE path (am = MTFHIP_AM_CCRE, AM/src/CCRE.cc) against the float64 NumPy reference of tests/golden/make_golden12.py (fixture
lk_golden12.npz), through every layer: the per-function entry points, one fused pass (Batch.iterate), the device loop (Batch.track),
set_region / track_region, the parameters, the refusals and the C++ harness.

Bounds.  MI's at the same bin counts (test_gpu_golden5.py: the same structure, N-wide sums and then logs): f 1e-10, the per-pixel gradient
vectors 1e-8, g and H 1e-5, all relative to the largest entry; dp 1e-6 and the tolerance-arithmetic pair 2e-6 / 1e-5 and the loop's 2e-4 px
from test_gpu_spss.py.  Each is widened to max(bound, 16 x the fixture's err_floor) where that is larger.  The generator samples in the
reference's own operation order, so It is the device's bit for bit and only the sums differ.  CCRE's passes are the same launches in both
arithmetic modes (step 0 always materialises), so tolerance arithmetic gives replay's bits and is held to equality, not to the pair.

Measured on one MI355X against the stored fixture: I0 and It bit for bit; f <= 2.6e-15, the gradient vectors <= 4.9e-15, g <= 5.8e-14,
H <= 6.3e-15, dp <= 5.5e-10 (the 7 x 9 case); the 2-bin case reads f 2.1e-12 (f = -1.5e-4 is what the logs of its four cells leave of terms
of order one), gradient vectors 5.8e-14, g 1.3e-13, H 2.2e-14, dp 2.6e-9: no quantity needs more than MI's bound.  Device loops (a record for every case and
run; whole where the run contracts, otherwise its first iterations: make_golden12.py): n_iters equal in every run, corners within 1.9e-6 px
for the whole loops and 1.5e-5 px for the cut ones; nt::ESM / FCLK / ICLK within 7.3e-7 px of the Python device loop, mtf::hip::LK 0 px."""
import os
import sys

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import make_golden12 as M  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "lk_golden12.npz"))
TAGS = [str(t) for t in G["tags"]]
BATCH3 = ["h50a", "h50b", "h50c"]
N_ITERS, LM_DELTA, LM_UPDATE = int(G["loop_cfg"][0]), float(G["loop_cfg"][1]), float(G["loop_cfg"][2])
REPLAY, FAST = mtf_amd.MATH_REPLAY, mtf_amd.MATH_FAST
B_F, B_DF, B_G, B_H = 1e-10, 1e-8, 1e-5, 1e-5            # MI's (test_gpu_golden5.py)
B_DP = 1e-6                                               # test_gpu_spss.py's replay bound on the update
LOOP_PX = 2e-4                                            # corners after a device loop (test_gpu_spss.py)

# (key, search method, jac_type, hess_type) -> the fixture's update
FIXTURE_METHODS = (("esm_ds", L.SM_ESM, 1, 2), ("esm_oo", L.SM_ESM, 0, 3), ("esm_std", L.SM_ESM, 1, 4), ("fclk_cs", L.SM_FCLK, 1, 1),
                   ("fclk_std", L.SM_FCLK, 1, 2), ("iclk_is", L.SM_ICLK, 1, 0), ("iclk_std", L.SM_ICLK, 1, 2))
# every served (search method, jac_type, hess_type): what MI's materialising route serves
SERVED = ([(L.SM_ESM, j, h) for j in (0, 1) for h in (0, 1, 2, 3, 4, 5)] + [(L.SM_FCLK, 1, h) for h in (0, 1, 2)] +
          [(L.SM_ICLK, 1, h) for h in (0, 1, 2)])
LOOP_KEYS = {"esm_ds": (L.SM_ESM, 1, 2), "fclk_cs": (L.SM_FCLK, 1, 1), "iclk_is": (L.SM_ICLK, 1, 0)}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def floor16(tag, name, base):
    """max(project bound, 16 x the fixture's float64-against-longdouble floor)"""
    return max(base, 16 * float(G[tag + "_err_floor_" + name]))


def cfg(tag):
    resx, resy, aff, nb, pou = (int(v) for v in G[tag + "_cfg"])
    return resx, resy, bool(aff), nb, pou


def make_batch(ctx, tags, math=REPLAY, am=L.AM_CCRE, **kw):
    resx, resy, aff, nb, pou = cfg(tags[0])
    assert all(cfg(t) == cfg(tags[0]) for t in tags)
    ctx.set_image(G["img"])
    if am == L.AM_CCRE:
        kw.setdefault("mi_n_bins", nb)
        kw.setdefault("mi_pre_seed", float(G[tags[0] + "_pre_seed"]))
        kw.setdefault("mi_partition_of_unity", pou)
    b = mtf_amd.Batch(ctx, am, L.SSM_AFFINE if aff else L.SSM_HOMOGRAPHY, resx, resy, len(tags), **kw)
    b.set_math_mode(math)
    b.set_corners(np.stack([G[t + "_corners"] for t in tags]))
    return b


def per_function(b, tags, chained=True):
    """the reference's call sequence of one iteration through the per-function entry points"""
    b.initialize_pix_vals()
    if chained:
        b.initialize_pix_grad()
        b.cmpt_pix_jacobian(L.JAC_WARPED, L.BUF_DI0_DX, L.BUF_J0)
    else:
        b.update_grad_pts(); b.initialize_pix_grad(warped=True)
        b.cmpt_pix_jacobian(L.JAC_INIT, L.BUF_DI0_DX, L.BUF_J0)
    b.initialize_similarity(); b.initialize_grad(); b.initialize_hess()
    f0 = b.get_similarity().copy()
    df_init = (b.read(L.BUF_DF_DI0).copy(), b.read(L.BUF_DF_DIT).copy())
    H0 = b.cmpt_self_hessian(L.BUF_J0)
    b.set_state(np.stack([G[t + "_p"] for t in tags]))
    b.update_pix_vals(); b.update_similarity(False); b.update_curr_grad(); b.update_init_grad()
    if chained:
        b.update_pix_grad(); b.cmpt_warped_pix_jacobian()
    else:
        b.update_grad_pts(); b.update_pix_grad(warped=True); b.cmpt_init_pix_jacobian(L.BUF_DIT_DX, L.BUF_JT)
    return f0, df_init, H0


def device_reference(b, k, tag):
    """the generator's expressions on the arrays the device sampled for target k"""
    _, _, _, nb, _ = cfg(tag)
    I0, It = b.read(L.BUF_I0)[k], b.read(L.BUF_IT)[k]
    J0, Jt = b.read(L.BUF_J0)[k], b.read(L.BUF_JT)[k]
    ps = float(G[tag + "_pre_seed"])
    return M.quantities(I0, It, J0, Jt, nb, ps), M.quantities(I0, I0, J0, J0, nb, ps)


def ref_g_H(q, H0, sm, jac, ht):
    """the search-method algebra over the reference's quantities"""
    if sm == L.SM_FCLK:
        g = q["g_curr"]
        H = H0 if ht == 0 else (q["H_self"] if ht == 1 else q["H_curr"])
    elif sm == L.SM_ICLK:
        g = q["g_init"]
        H = H0 if ht == 0 else (q["H_self"] if ht == 1 else q["H_init"])
    else:
        g = q["g_mean"] if jac == 0 else 0.5 * (q["g_curr"] - q["g_init"])
        H = {0: H0, 1: q["H_self"], 2: 0.5 * (q["H_self"] + H0), 3: q["H_mean"], 4: 0.5 * (q["H_init"] + q["H_curr"]), 5: q["H_curr"]}[ht]
    return g, H


# ------------------------------------------------------------------ 1. the per-function entry points
@pytest.mark.parametrize("chained", [1, 0])
@pytest.mark.parametrize("tag", TAGS)
def test_per_function_entry_points(gpu_ctx, tag, chained):
    b = make_batch(gpu_ctx, [tag])
    s = make_batch(gpu_ctx, [tag], am=L.AM_SSD)
    try:
        f0, df_init, H0 = per_function(b, [tag], bool(chained))
        _, _, _, nb, pou = cfg(tag)
        # the samples are ImageBase's under CCRE's scaling: an SSD batch's bits times the scaling, and the fixture's
        s.initialize_pix_vals(); s.set_state(G[tag + "_p"][None]); s.update_pix_vals()
        mult, add = M.pix_norm(nb, pou)
        for buf, name in ((L.BUF_I0, "I0"), (L.BUF_IT, "It")):
            assert np.array_equal(b.read(buf)[0], mult * s.read(buf)[0] + add), name
            assert np.array_equal(b.read(buf)[0], G[tag + "_" + name]), name
        f, lik = b.get_similarity()[0], b.get_likelihood()[0]
        dft, df0 = b.read(L.BUF_DF_DIT)[0], b.read(L.BUF_DF_DI0)[0]
        out = dict(g_curr=b.cmpt_curr_jacobian()[0], g_init=b.cmpt_init_jacobian()[0], g_diff=b.cmpt_difference_of_jacobians()[0],
                   H_self=b.cmpt_self_hessian()[0], H_curr=b.cmpt_curr_hessian()[0], H_init=b.cmpt_init_hessian()[0],
                   H_sum=b.cmpt_sum_of_hessians()[0])
        assert b.get_similarity()[0] == f                                  # (cmptSelfHessian takes the tables again: the same f)
        q, q0 = device_reference(b, 0, tag)
        q["g_diff"], q["H_sum"] = q["g_curr"] - q["g_init"], q["H_init"] + q["H_curr"]
        e = {n: rel(out[n], q[n]) for n in out}
        e["f"], e["df_dIt"], e["df_dI0"] = rel(f, q["f"]), rel(dft, q["df_dIt"]), rel(df0, q["df_dI0"])
        e["f_init"], e["df_init"], e["H0"] = rel(f0[0], q0["f"]), rel(df_init[0][0], q0["df_dIt"]), rel(H0[0], q0["H_self"])
        print("per_function %s chained %d: device-sampled %s" % (tag, chained, e))
        assert np.array_equal(df_init[0], df_init[1])                      # initializeGrad: df_dIt = df_dI0
        assert e["f"] < floor16(tag, "f", B_F) and e["f_init"] < B_F
        assert e["df_dIt"] < floor16(tag, "df_dIt", B_DF) and e["df_dI0"] < floor16(tag, "df_dI0", B_DF) and e["df_init"] < B_DF
        assert lik == pytest.approx(np.exp(-((f0[0] / f - 1) ** 2)), rel=1e-12)
        for n in ("g_curr", "g_init", "g_diff"):
            assert e[n] < floor16(tag, "g_init" if n == "g_init" else "g_curr", B_G), (n, e[n])
        for n in ("H_self", "H_curr", "H_init", "H_sum"):
            assert e[n] < floor16(tag, "H_curr" if n == "H_sum" else n, B_H), (n, e[n])
        assert e["H0"] < B_H
        if chained:
            fx = {n: rel(out[n], G[tag + "_" + n]) for n in ("g_curr", "g_init", "H_self", "H_curr", "H_init")}
            fx.update(f=rel(f, float(G[tag + "_f"])), f_init=rel(f0[0], float(G[tag + "_f_init"])), df_dIt=rel(dft, G[tag + "_df_dIt"]),
                      df_dI0=rel(df0, G[tag + "_df_dI0"]), df_init=rel(df_init[0][0], G[tag + "_df_init"]), H0=rel(H0[0], G[tag + "_H0"]))
            print("per_function %s: fixture %s" % (tag, fx))
            assert fx["f"] < floor16(tag, "f", B_F) and fx["f_init"] < B_F
            assert fx["df_dIt"] < floor16(tag, "df_dIt", B_DF) and fx["df_dI0"] < floor16(tag, "df_dI0", B_DF) and fx["df_init"] < B_DF
            for n in ("g_curr", "g_init"):
                assert fx[n] < floor16(tag, n, B_G), (n, fx[n])
            for n in ("H_self", "H_curr", "H_init"):
                assert fx[n] < floor16(tag, n, B_H), (n, fx[n])
            assert fx["H0"] < B_H
    finally:
        b.close(); s.close()


def test_prereq_only_leaves_f(gpu_ctx):
    b = make_batch(gpu_ctx, ["a25x20"])
    try:
        per_function(b, ["a25x20"])
        f = b.get_similarity()[0]
        b.set_state(np.zeros((1, 6)))
        b.update_pix_vals(); b.update_similarity(True)
        assert b.get_similarity()[0] == f
        b.update_similarity(False)
        assert b.get_similarity()[0] != f
    finally:
        b.close()


# ------------------------------------------------------------------ 2. one fused pass
def one_pass(b, tags, sm_id, jac, ht, chained, mat):
    sm = mtf_amd.sm_desc(sm_id, jac_type=jac, hess_type=ht, chained_warp=chained, materialize=mat, leven_marq=0)
    b.set_corners(np.stack([G[t + "_corners"] for t in tags]))      # (back to the template's region: init_template samples the current points)
    b.init_template(sm)
    b.set_state(np.stack([G[t + "_p"] for t in tags]))
    return b.iterate(sm)


@pytest.mark.parametrize("chained", [1, 0])
@pytest.mark.parametrize("tag", ["h50a", "h50p10", "a25x20", "a25x20i", "h7x9p4", "h13x11b2", "h13x11"])
def test_fused_pass_every_served_type(gpu_ctx, tag, chained):
    """chained and not: f, g, H and dp of every served method / jac_type / hess_type against the reference on the device's samples; the pass
    that materialises nothing gives the materialising pass's bits, in either arithmetic mode"""
    b = make_batch(gpu_ctx, [tag], REPLAY)
    bf = make_batch(gpu_ctx, [tag], FAST)
    try:
        worst = dict(f=0.0, g=0.0, H=0.0, dp=0.0)
        one_pass(b, [tag], L.SM_ESM, 1, 2, chained, 1)                 # (an ESM pass materialises Jt: the reference reads it)
        q, q0 = device_reference(b, 0, tag)
        for sm_id, jac, ht in SERVED:
            f, g, H = one_pass(b, [tag], sm_id, jac, ht, chained, 1)
            gr, Hr = ref_g_H(q, q0["H_self"], sm_id, jac, ht)
            dp, dpr = -np.linalg.solve(H[0], g[0]), -np.linalg.solve(Hr, gr)
            e = dict(f=rel(f[0], q["f"]), g=rel(g[0], gr), H=rel(H[0], Hr), dp=rel(dp, dpr))
            for n in e:
                worst[n] = max(worst[n], e[n])
            assert e["f"] < floor16(tag, "f", B_F) and e["g"] < floor16(tag, "g_curr", B_G) and e["H"] < floor16(tag, "H_curr", B_H), (sm_id, jac, ht, e)
            key = [k for k, s_, j_, h_ in FIXTURE_METHODS if (s_, j_, h_) == (sm_id, jac, ht)]
            if key:
                assert e["dp"] < floor16(tag, key[0] + "_dp", B_DP), (sm_id, jac, ht, e)
            fl, gl, Hl = one_pass(b, [tag], sm_id, jac, ht, chained, 0)
            assert np.array_equal(fl, f) and np.array_equal(gl, g) and np.array_equal(Hl, H), (sm_id, jac, ht)
            ft, gt, Ht = one_pass(bf, [tag], sm_id, jac, ht, chained, 0)
            assert np.array_equal(ft, f) and np.array_equal(gt, g) and np.array_equal(Ht, H), (sm_id, jac, ht)
        print("fused_pass %s chained %d worst: %s" % (tag, chained, worst))
    finally:
        b.close(); bf.close()


@pytest.mark.parametrize("mat", [0, 1])
@pytest.mark.parametrize("tag", TAGS)
def test_fused_pass_against_fixture(gpu_ctx, tag, mat):
    """the fixture's seven configurations, chained, against its stored f, g, H and dp"""
    b = make_batch(gpu_ctx, [tag], REPLAY)
    worst = dict(f=0.0, g=0.0, H=0.0, dp=0.0)
    try:
        q = {n: G[tag + "_" + n] for n in ("g_curr", "g_init", "g_mean", "H_self", "H_curr", "H_init", "H_mean")}
        for key, sm_id, jac, ht in FIXTURE_METHODS:
            f, g, H = one_pass(b, [tag], sm_id, jac, ht, 1, mat)
            gr, Hr = ref_g_H(q, G[tag + "_H0"], sm_id, jac, ht)
            e = dict(f=rel(f[0], float(G[tag + "_f"])), g=rel(g[0], gr), H=rel(H[0], Hr),
                     dp=rel(-np.linalg.solve(H[0], g[0]), G[tag + "_" + key + "_dp"]))
            for n in e:
                worst[n] = max(worst[n], e[n])
            assert e["f"] < floor16(tag, "f", B_F) and e["g"] < floor16(tag, "g_curr", B_G) and e["H"] < floor16(tag, "H_curr", B_H), (key, e)
            assert e["dp"] < floor16(tag, key + "_dp", B_DP), (key, e)
        print("fixture_pass %s mat %d worst: %s" % (tag, mat, worst))
    finally:
        b.close()


@pytest.mark.parametrize("chained", [0, 1])
@pytest.mark.parametrize("tag", ["h50a", "a25x20"])
def test_materialised_arrays_equal_per_function(gpu_ctx, tag, chained):
    """materialize 1: DF_DIT, DF_DI0, IT, DIT_DX and JT of an ESM pass are the per-function entry points' bits, chained or not"""
    b = make_batch(gpu_ctx, [tag])
    r = make_batch(gpu_ctx, [tag])
    try:
        one_pass(b, [tag], L.SM_ESM, 1, 2, chained, 1)
        per_function(r, [tag], bool(chained))
        for buf in (L.BUF_IT, L.BUF_DIT_DX, L.BUF_JT, L.BUF_DF_DIT, L.BUF_DF_DI0):
            assert np.array_equal(b.read(buf), r.read(buf)), buf
    finally:
        b.close(); r.close()


# ------------------------------------------------------------------ 3. the device loop
def loop_sm(key, lm, eps, mat=1, max_iters=N_ITERS):
    sm_id, jac, ht = LOOP_KEYS[key]
    return mtf_amd.sm_desc(sm_id, jac_type=jac, hess_type=ht, chained_warp=1, materialize=mat, max_iters=max_iters, epsilon=eps,
                           leven_marq=int(lm), lm_delta_init=LM_DELTA, lm_delta_update=LM_UPDATE)


def stored_sm(tag, key, lm, mat=1):
    """the loop the fixture stores for the run: the whole 10-iteration loop with its corner-change test where it contracts, otherwise its
    first <run>_loop_iters iterations without a test (make_golden12.py: as far as the run pins a second implementation)"""
    pre = "%s_%s%s_loop" % (tag, key, "_lm" if lm else "")
    return loop_sm(key, lm, float(G[pre + "_eps"]), mat=mat, max_iters=int(G[pre + "_iters"])), "_" + pre[len(tag) + 1:]


def run_track(ctx, tags, sm, math, tables=False):
    b = make_batch(ctx, tags, math)
    try:
        b.init_template(sm)
        b.set_state(np.stack([G[t + "_p"] for t in tags]))
        n, corners = b.track(sm)
        extra = (b.read(L.BUF_IT).copy(), b.get_similarity().copy()) if tables else None
        return n, corners, b.get_state(), extra
    finally:
        b.close()


def stored_runs(tags):
    return [(key, lm) for key in LOOP_KEYS for lm in (0, 1) if all("%s_%s%s_loop_n" % (t, key, "_lm" if lm else "") in G.files for t in tags)]


@pytest.mark.parametrize("math", [REPLAY, FAST])
@pytest.mark.parametrize("key,lm", stored_runs(BATCH3))
def test_track_follows_the_fixture(gpu_ctx, key, lm, math):
    """a batch of three targets on one template that stop at different passes: n_iters equal, corners within 2e-4 px; a target that stops
    early keeps its It and its similarity: the batch equals the targets one at a time bit for bit; two runs are bit-identical"""
    eps = float(G[BATCH3[0] + "_eps"])
    sm = loop_sm(key, lm, eps, mat=1 if math == REPLAY else 0)
    n, corners, _, ex = run_track(gpu_ctx, BATCH3, sm, math, tables=True)
    pre = "_" + key + ("_lm" if lm else "") + "_loop"
    want_n = [int(G[t + pre + "_n"]) for t in BATCH3]
    err = [float(np.abs(corners[k] - G[t + pre + "_corners"]).max()) for k, t in enumerate(BATCH3)]
    print("track %s lm %d math %d: n %s (fixture %s), corner error %s px" % (key, lm, math, n.tolist(), want_n, err))
    assert n.tolist() == want_n
    assert max(err) < LOOP_PX
    for k, t in enumerate(BATCH3):
        n1, c1, _, ex1 = run_track(gpu_ctx, [t], sm, math, tables=True)
        assert n1[0] == n[k] and np.array_equal(c1[0], corners[k]), t
        assert np.array_equal(ex1[0][0], ex[0][k]) and ex1[1][0] == ex[1][k], t
    n2, c2, _, _ = run_track(gpu_ctx, BATCH3, sm, math)
    assert np.array_equal(n2, n) and np.array_equal(c2, corners)


def test_track_batch_has_an_early_stop():
    want = [int(G[t + "_esm_ds_loop_n"]) for t in BATCH3]
    assert len(set(want)) > 1 and min(want) < N_ITERS


@pytest.mark.parametrize("tag", [t for t in TAGS if t not in BATCH3])
def test_track_every_other_case(gpu_ctx, tag):
    """every other case of the fixture -- N = 63 and the ragged N = 143, 2, 4, 10 and 16 bins, the integer image, affine -- and all six runs
    of each: the stored loop (stored_sm), n_iters equal, corners and state within the loop bound"""
    assert len(stored_runs([tag])) == 6
    for key, lm in stored_runs([tag]):
        sm, pre = stored_sm(tag, key, lm)
        n, corners, state, _ = run_track(gpu_ctx, [tag], sm, REPLAY)
        print("track %s %s lm %d (%d iterations, epsilon %g): n %d (fixture %d), corner error %.3g px" % (
            tag, key, lm, sm.max_iters, sm.epsilon, n[0], int(G[tag + pre + "_n"]), np.abs(corners[0] - G[tag + pre + "_corners"]).max()))
        assert n[0] == int(G[tag + pre + "_n"]), (key, lm)
        assert np.abs(corners[0] - G[tag + pre + "_corners"]).max() < LOOP_PX, (key, lm)
        assert np.abs(state[0] - G[tag + pre + "_state"]).max() < LOOP_PX, (key, lm)


@pytest.mark.parametrize("key", ["esm_ds", "fclk_cs", "iclk_is"])
def test_set_region_and_track_region(gpu_ctx, key):
    """set_region + track is track_region, and from the template's own region both are the loop from the identity (h50c's state is zero)"""
    tag = "h50c"
    assert not G[tag + "_p"].any()
    sm = loop_sm(key, 0, float(G[tag + "_eps"]))
    a, b = make_batch(gpu_ctx, [tag]), make_batch(gpu_ctx, [tag])
    try:
        a.init_template(sm); b.init_template(sm)
        a.set_region(G[tag + "_corners"][None], sm)
        n1, c1 = a.track(sm)
        n2, c2 = b.track_region(G[tag + "_corners"][None], sm)
        assert np.array_equal(n1, n2) and np.array_equal(c1, c2)
        pre = "_" + key + "_loop"
        assert n1[0] == int(G[tag + pre + "_n"])
        assert np.abs(c1[0] - G[tag + pre + "_corners"]).max() < LOOP_PX
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ 4. the parameters
def test_parameters_change_f_as_the_generator_says(gpu_ctx):
    """h50a's region and state at 8 bins, at 10 bins with partition of unity, and at pre_seed 0.5: three different f, each the fixture's"""
    fs = []
    for tag in ("h50a", "h50p10", "h50s0"):
        b = make_batch(gpu_ctx, [tag])
        try:
            f, _, _ = one_pass(b, [tag], L.SM_ESM, 1, 2, 1, 0)
            assert rel(f[0], float(G[tag + "_f"])) < floor16(tag, "f", B_F), tag
            fs.append(f[0])
        finally:
            b.close()
    assert len({round(v, 6) for v in fs}) == 3
    # Batch's own keyword for partition of unity and the older mi_pou are one field
    b = mtf_amd.Batch(gpu_ctx, L.AM_CCRE, L.SSM_HOMOGRAPHY, 10, 10, 1, mi_n_bins=10, mi_partition_of_unity=1)
    assert b.desc.mi_partition_of_unity == 1
    b.close()


# ------------------------------------------------------------------ 5. the refusals
NI = mtf_amd.FunctionNotImplemented
R_SO = "CCRE with second-order Hessians is not available on the device path"
R_ALK = r"CCRE is not available with the additive search methods \(FALK / IALK\)"
R_ENTRY = "CCRE is not available on this entry point"
R_CAND = r"CCRE is not available on this entry point \(CCREDist is a per-candidate histogram\)"


def refused(match, fn, *a, **kw):
    with pytest.raises(NI, match=match):
        fn(*a, **kw)


def test_refusals(gpu_ctx):
    """every refusal at the C ABI, each with its reason (the Python trackers' own guards are checked last and apart)"""
    tag = "h13x11"
    gpu_ctx.set_image(G["img"])
    # at batch_create
    refused("MCCCRE", mtf_amd.Batch, gpu_ctx, L.AM_CCRE, L.SSM_HOMOGRAPHY, 10, 10, 1, n_channels=3)
    for ssm in L.SSM_LOW_ORDER:
        refused("is served with SSD, NCC and SSIM only", mtf_amd.Batch, gpu_ctx, L.AM_CCRE, ssm, 10, 10, 1)
    with pytest.raises(mtf_amd.MtfHipError, match="CCRE::Too few bins 3 specified to enforce partition of unity constraint"):
        mtf_amd.Batch(gpu_ctx, L.AM_CCRE, L.SSM_HOMOGRAPHY, 10, 10, 1, mi_n_bins=3, mi_partition_of_unity=1)
    with pytest.raises(mtf_amd.MtfHipError, match=r"CCRE: n_bins 17 outside \[2, 16\]"):
        mtf_amd.Batch(gpu_ctx, L.AM_CCRE, L.SSM_HOMOGRAPHY, 10, 10, 1, mi_n_bins=17)
    b = make_batch(gpu_ctx, [tag])
    try:
        # getLikelihood needs initializeSimilarity's f
        with pytest.raises(mtf_amd.MtfHipError, match="CCRE before initializeSimilarity"):
            b.get_likelihood()
        corners = G[tag + "_corners"][None]
        bad = [(R_SO, mtf_amd.sm_desc(sm_id, hess_type=2, sec_ord_hess=1, leven_marq=0)) for sm_id in (L.SM_ESM, L.SM_FCLK, L.SM_ICLK)]
        bad += [(R_ALK, mtf_amd.sm_desc(sm_id, leven_marq=0)) for sm_id in (L.SM_FALK, L.SM_IALK)]
        # the fused entry points before a template exists ...
        for why, sm in bad:
            refused(why, b.init_template, sm)
        good = mtf_amd.sm_desc(L.SM_ESM, hess_type=2, leven_marq=0)
        b.init_template(good)
        b.set_state(G[tag + "_p"][None])
        before = b.iterate(good)
        # ... and behind one: iterate, track, set_region, track_region
        for why, sm in bad:
            refused(why, b.iterate, sm)
            refused(why, b.track, sm)
            refused("additive search methods" if why == R_ALK else why, b.set_region, corners, sm)
            refused("additive search methods" if why == R_ALK else why, b.track_region, corners, sm)
        # the second-order per-function entry points
        for fn in (b.cmpt_init_hessian2, b.cmpt_curr_hessian2, b.cmpt_self_hessian2, b.cmpt_sum_of_hessians2):
            refused(R_SO, fn)
        refused("CCRE has no online template update", b.update_model)
        # the grid entry points, the candidate scorer / sampler, the NN entry points
        iclk = mtf_amd.sm_desc(L.SM_ICLK, leven_marq=0)
        refused(R_ENTRY, b.grid_update, corners, iclk)
        gd = L.GridDesc(1, 1, 10, 10, 0, 0, 1)
        refused(R_ENTRY, b.grid_frame, gd, iclk, G[tag + "_corners"])
        refused(R_ENTRY, b.grid_reset, gd, iclk, G[tag + "_corners"], 1)
        refused(R_CAND, b.score_candidates, np.zeros((4, 8)))
        refused(R_CAND, b.sample_candidates, np.zeros((4, 8)))
        refused(R_CAND, b.nn_dataset, 4, np.full(8, 0.01))
        refused(R_CAND, b.nn_create, 4)
        # a refused call leaves the batch as it was: the same pass gives the same bits
        b.set_corners(corners); b.init_template(good); b.set_state(G[tag + "_p"][None])
        for x, y in zip(before, b.iterate(good)):
            assert np.array_equal(x, y)
    finally:
        b.close()


def test_pf_create_refused(gpu_ctx):
    """mtfhip_pf_create on a CCRE batch: refused before the descriptor is read"""
    import ctypes as C
    b = make_batch(gpu_ctx, ["h13x11"])
    try:
        desc, h = C.create_string_buffer(4096), C.c_void_p()
        rc = L.lib().mtfhip_pf_create(b._h, desc, C.byref(h))
        assert rc == -2 and not h.value
        assert b"pf_create: CCRE is not available on this entry point (CCREDist is a per-candidate histogram)" in L.lib().mtfhip_last_error()
    finally:
        b.close()


def test_python_trackers_refuse_before_the_c_abi(gpu_ctx):
    from mtf_amd import sm as SMOD
    for cls in (SMOD.GridTracker, SMOD.ParticleFilter, SMOD.NNDataset, SMOD.NNTracker):
        refused("the CCRE appearance model is served by LKTracker and NTSearchMethod only", cls, gpu_ctx, am=L.AM_CCRE)


# ------------------------------------------------------------------ 6. the Python tracker and the harness
@pytest.mark.parametrize("key", ["esm_ds", "fclk_cs", "iclk_is"])
def test_lktracker_follows_the_fixture(gpu_ctx, key):
    """sm.LKTracker(ctx, sm, am=AM_CCRE) with CCREParams as am_params: the host-side solve over iterate and the device loop, from the
    template's own region (h50c's state is zero), against the generator's loop"""
    from mtf_amd.sm import LKTracker
    tag = "h50c"
    sm_id, jac, ht = LOOP_KEYS[key]
    resx, resy, aff, nb, pou = cfg(tag)
    pre = "_" + key + "_loop"
    gpu_ctx.set_image(G["img"])
    for host_solve in (True, False):
        t = LKTracker(gpu_ctx, sm_id, ssm=L.SSM_HOMOGRAPHY, resx=resx, resy=resy, n_targets=1, host_solve=host_solve, am=L.AM_CCRE,
                      am_params=dict(mi_n_bins=nb, mi_pre_seed=float(G[tag + "_pre_seed"]), mi_partition_of_unity=pou), jac_type=jac, hess_type=ht,
                      max_iters=N_ITERS, epsilon=float(G[tag + "_eps"]), leven_marq=0)
        try:
            t.initialize(G[tag + "_corners"][None])
            corners = t.update()
            assert int(np.asarray(t.n_iters)[0]) == int(G[tag + pre + "_n"]), host_solve
            assert np.abs(np.asarray(corners)[0] - G[tag + pre + "_corners"]).max() < LOOP_PX, host_solve
        finally:
            t.batch.close()


# ------------------------------------------------------------------ 7. the harness
@pytest.mark.parametrize("key", ["esm_ds", "fclk_cs", "iclk_is"])
def test_harness_follows_the_python_device_loop(gpu_ctx, key):
    """nt::ESM / FCLK / ICLK over HipAM("ccre") call by call, and mtf::hip::LK (the device loop behind the same classes), against Batch.track"""
    from mtf_amd import host
    tag = "h50c"
    sm_id, jac, ht = LOOP_KEYS[key]
    eps = float(G[tag + "_eps"])
    n, corners, _, _ = run_track(gpu_ctx, [tag], loop_sm(key, 0, eps), REPLAY)
    resx, resy, aff, nb, pou = cfg(tag)
    for device_loop in (False, True):
        t = host.CppTracker.ccre(sm_id, L.SSM_HOMOGRAPHY, resx, resy, max_iters=N_ITERS, epsilon=eps, jac_type=jac, hess_type=ht, chained_warp=1,
                                 leven_marq=0, n_bins=nb, partition_of_unity=pou, pre_seed=float(G[tag + "_pre_seed"]), device_loop=device_loop)
        t.set_image(np.ascontiguousarray(G["img"]))
        t.initialize(G[tag + "_corners"])
        t.update()
        err = float(np.abs(t.get_region() - corners[0]).max())
        print("harness %s device_loop %d: %.3g px from Batch.track" % (key, device_loop, err))
        assert err < LOOP_PX
