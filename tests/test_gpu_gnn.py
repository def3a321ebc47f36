"""nt::NN's graph index gnn::GNN on the device (mtfhip_nn_gnn_*, kernels_gnn.hip; SM/src/NT/GNN.cc:30-203) against tests/helpers/gnn_ref.py.
The cases, seeds and shapes are tests/helpers/gnn_cases.py's; tests/test_gnn_ref.py asserts on the reference alone that they keep the caps
this file relies on (at most 2 % of neighbour-list positions not clear; every decision of every compared walk clear; walks that end off
the exact nearest row).
    build   at every clear position the index is the reference's; at EVERY position the extended-precision distance of the row to the
            device's neighbour equals the reference's sorted distance at that rank within DESIGN 4.12's bound -- 4 (feat_size + 1) 2^-53
            relative (SSD) or times ||a|| ||b|| (NCC); no index twice in a row; duplicated rows tie exactly; panels do not show
    search  degree n - 1: mtfhip_nn_search's index and distance BITS; degree 4 / 16: the reference's index and step count
    tracker sm.NNTracker(index="gnn") over three frames against gnn_ref.nn_update_gnn driven through the oracle's AM and SSM"""
import ctypes
import os
import sys

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd.sm import NNTracker

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gnn_cases as GC   # noqa: E402
import gnn_ref as G      # noqa: E402
import nn_cases as NC    # noqa: E402
import nn_ref as R       # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
SHAPE_IDS = lambda s: "%dx%d" % s   # noqa: E731
AMS = pytest.mark.parametrize("am", [R.SSD, R.NCC], ids=["ssd", "ncc"])


def _batch(ctx, shape, am):
    return mtf_amd.Batch(ctx, L.AM_NCC if am == R.NCC else L.AM_SSD, L.SSM_HOMOGRAPHY, shape[0], shape[1], 1)


def _handle(b, m):
    h = b.nn_create(len(m))
    b.nn_set_dataset(h, m, np.zeros((len(m), 8)))
    return h


def _scratch(nbytes):
    """the build's scratch budget for the calls that follow (None: the library's own)"""
    if nbytes is None:
        os.environ.pop("MTFHIP_GNN_SCRATCH_BYTES", None)
    else:
        os.environ["MTFHIP_GNN_SCRATCH_BYTES"] = str(int(nbytes))


def _check_graph(g, m, d, deg, am, tag):
    n, F = m.shape
    k = G.effective_degree(deg, n)
    assert g.shape == (n, k) and g.dtype == np.int32, tag
    if k == 0:
        return 0.0
    assert g.min() >= 0 and g.max() < n
    idx, dist = G.neighbour_lists(d, deg)
    unclear = G.unclear_positions(dist)
    assert np.array_equal(g[~unclear], idx[:, 1:][~unclear]), tag
    srt = np.sort(g, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1]), tag                     # no index twice in a row's list
    got, want = d[np.arange(n)[:, None], g], dist[:, 1:k + 1]
    norms = np.linalg.norm(m, axis=1)
    scale = np.abs(want) if am == R.SSD else norms[:, None] * norms[g]
    worst = float((np.abs(got - want) / np.maximum(4 * (F + 1) * U * scale, 1e-300)).max())
    print("%s: %d of %d positions unclear, worst |d - ref| / bound = %.3f" % (tag, int(unclear.sum()), unclear.size, worst))
    assert worst <= 1.0, tag
    return worst


@AMS
@pytest.mark.parametrize("shape", GC.BUILD_SHAPES, ids=SHAPE_IDS)
def test_build_equals_reference(gpu_ctx, shape, am):
    F = shape[0] * shape[1]
    b = _batch(gpu_ctx, shape, am)
    _scratch(None)
    for n in GC.BUILD_N:
        m, d = GC.build_case(n, F, am)
        h = _handle(b, m)
        for deg in GC.build_degrees(n):
            b.nn_gnn_build(h, dict(degree=deg))
            _check_graph(b.nn_gnn_get_graph(h, n), m, d, deg, am, "n=%d F=%d am=%d degree=%d" % (n, F, am, deg))
        b.nn_destroy(h)
    b.close()


@AMS
@pytest.mark.parametrize("F", [49, 625])
def test_duplicated_rows(gpu_ctx, F, am):
    """identical rows at indices of both parities (odd feat_size: both alignments): their distances to any row have the same bits, the tie
    goes to the lower index, and a row behind its twin keeps itself as a neighbour"""
    shape = (7, 7) if F == 49 else (25, 25)
    m = GC.dup_rows(F, am)
    d = G.all_distances(m, am)
    b = _batch(gpu_ctx, shape, am)
    h = _handle(b, m)
    _scratch(None)
    for deg in (GC.DUP_N - 1, 4, 1):
        b.nn_gnn_build(h, dict(degree=deg))
        g = b.nn_gnn_get_graph(h, GC.DUP_N)
        assert np.array_equal(g, G.build_graph(m, deg, am, dmat=d)), deg
        for dst, _ in GC.DUP_COPIES:
            assert deg < 2 or dst in g[dst]          # (two places: behind the triple's two lower twins)
    b.nn_destroy(h); b.close()


@AMS
@pytest.mark.parametrize("shape", [(7, 7), (16, 12)], ids=SHAPE_IDS)
def test_panels_and_repeated_builds_do_not_show(gpu_ctx, shape, am):
    """a build in panels of 3 rows, of 64 rows (four whole blocks and a last panel of one row) and in one panel: the same graph, bit for bit;
    and get_graph -> set_graph on a second handle gives identical searches"""
    F, n = shape[0] * shape[1], 257
    m, _ = GC.build_case(n, F, am)
    b = _batch(gpu_ctx, shape, am)
    h = _handle(b, m)
    graphs = []
    try:
        for budget in (None, None, 8 * n * 3, 8 * n * 70):
            _scratch(budget)
            for deg in (16, n - 1):
                b.nn_gnn_build(h, dict(degree=deg, max_steps=3))
                graphs.append(b.nn_gnn_get_graph(h, n))
    finally:
        _scratch(None)
    for k in range(2, len(graphs)):
        assert np.array_equal(graphs[k], graphs[k % 2]), k
    b.nn_gnn_build(h, dict(degree=16, max_steps=3))
    h2 = _handle(b, m)
    b.nn_gnn_set_graph(h2, graphs[0], dict(degree=16, max_steps=3))
    q = GC.rows(9, F, am, 4)
    starts = np.arange(9) * 28
    a1, a2 = b.nn_gnn_search(h, q, starts), b.nn_gnn_search(h2, q, starts)
    for x, y in zip(a1, a2):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert np.array_equal(b.nn_gnn_get_graph(h2, n), graphs[0])
    b.nn_destroy(h); b.nn_destroy(h2); b.close()


@AMS
@pytest.mark.parametrize("shape", GC.BUILD_SHAPES, ids=SHAPE_IDS)
def test_full_degree_walk_is_the_exhaustive_search(gpu_ctx, shape, am):
    """degree n - 1: one step sees every other row, and a row's sum is the exhaustive search's own code -- the same index, the same BITS"""
    F, n = shape[0] * shape[1], 257
    m, _ = GC.build_case(n, F, am)
    b = _batch(gpu_ctx, shape, am)
    h = _handle(b, m)
    _scratch(None)
    q = np.concatenate([GC.rows(6, F, am, 31), m[[0, 256, 101]]])
    idx, dist = b.nn_search(h, q)
    for ms in (1, 10):
        b.nn_gnn_build(h, dict(degree=0, max_steps=ms))
        for starts in (np.zeros(9, dtype=int), np.arange(9) * 32, np.full(9, 256), idx):
            gi, gd, gs = b.nn_gnn_search(h, q, starts)
            assert np.array_equal(gi, idx), (ms, starts)
            assert np.array_equal(gd.view(np.uint64), dist.view(np.uint64)), (ms, starts)
            assert np.all(gs == np.where(np.asarray(starts) == idx, 1, min(ms, 2)))
    b.nn_destroy(h); b.close()


@pytest.mark.parametrize("case", GC.WALK_CASES, ids=lambda c: c[0])
def test_walks_equal_reference(gpu_ctx, case):
    import torch
    name, am, shape, n, degree = case
    F = shape[0] * shape[1]
    w = GC.walk_case(case)
    m, q, starts = w["rows"], w["queries"], w["starts"]
    b = _batch(gpu_ctx, shape, am)
    h = _handle(b, m)
    _scratch(None)
    b.nn_gnn_build(h, dict(degree=degree))
    built = b.nn_gnn_get_graph(h, n)
    d = G.all_distances(m, am)
    _check_graph(built, m, d, degree, am, name)
    off = 0
    for ms in GC.WALK_MAX_STEPS:
        b.nn_gnn_set_graph(h, w["graph"], dict(degree=degree, max_steps=ms))
        gi, gd, gs = b.nn_gnn_search(h, q, starts)
        ref = w["walks"][ms]
        assert np.array_equal(gi, [r["idx"] for r in ref]), ms
        assert np.array_equal(gs, [r["n_steps"] for r in ref]), ms
        for j, r in enumerate(ref):
            scale = abs(r["dist"]) if am == R.SSD else np.linalg.norm(m[r["idx"]]) * np.linalg.norm(q[j])
            err, bound = abs(gd[j] - r["dist"]), 4 * (F + 1) * U * scale
            assert err <= bound, (ms, j, err, bound)
            off += r["idx"] != w["exact"][j][0]
        # the _dev form: the same bits
        qd, sd = torch.from_numpy(q.copy()).to("cuda:0"), torch.from_numpy(starts).to("cuda:0")
        idx_d = torch.full((GC.WALK_Q,), -7, dtype=torch.int32, device="cuda:0")
        dist_d = torch.zeros(GC.WALK_Q, dtype=torch.float64, device="cuda:0"); steps_d = torch.zeros_like(idx_d)
        torch.cuda.synchronize()
        b.nn_gnn_search_dev(h, qd.data_ptr(), GC.WALK_Q, sd.data_ptr(), idx_d.data_ptr(), dist_d.data_ptr(), steps_d.data_ptr())
        gpu_ctx.synchronize()
        assert np.array_equal(idx_d.cpu().numpy(), gi) and np.array_equal(steps_d.cpu().numpy(), gs)
        assert np.array_equal(dist_d.cpu().numpy().view(np.uint64), gd.view(np.uint64))
    assert off >= 1          # the index is the graph's, not the exhaustive one
    # start_nodes = None: every walk from the handle's start node, which a stateless search leaves alone
    b.nn_gnn_set_start(h, int(starts[5]))
    gi0, gd0, gs0 = b.nn_gnn_search(h, q[5:6])
    assert (gi0[0], gs0[0]) == (gi[5], gs[5]) and gd0[0] == gd[5] and b.nn_gnn_get_start(h) == starts[5]
    b.nn_destroy(h); b.close()


# ---- the tracker ----
_TRACK = {}


def _track_frames(frame, frame2):
    from mtf_amd import synth
    out = [frame2]
    for seed in (2027, 2028):
        out.append(synth.warp_frame(frame, synth.random_small_homography(np.random.default_rng(seed)) * 0.5, (256.0, 256.0)))
    return out


def _track_reference(oracle, frame, frame2, case):
    """the oracle's dataset, the reference's graph and nn_update_gnn over the three frames: computed once, shared, never changed"""
    name, am, ssm = case
    if name not in _TRACK:
        res, n = GC.TRACK_RES, GC.TRACK_N
        o_ssm = oracle.SSM(ssm, res, res); o_am = oracle.AM(am, res, res)
        o_am.set_curr_img(frame)
        corners = NC.track_corners(res)
        o_ssm.set_corners(corners)
        o_am.initialize_pix_vals(o_ssm.get("curr_pts"))
        S = 8 if ssm == 0 else 6
        perts = np.random.default_rng(40 + am + 2 * ssm).normal(size=(n, S)) * (NC.SIGMA_H if S == 8 else NC.SIGMA_A)
        perts[0] = 0.0
        feats = oracle.nn_generate_dataset(o_am, o_ssm, perts)
        graph = G.build_graph(feats, GC.TRACK_DEGREE, R.NCC if am == 1 else R.SSD)
        frames, refs, start = _track_frames(frame, frame2), [], GC.TRACK_START
        for img in frames:
            o_am.set_curr_img(img)
            r = G.nn_update_gnn(o_am, o_ssm, feats, perts, graph, start, GC.TRACK_MAX_STEPS, GC.TRACK_ITERS, GC.TRACK_EPS)
            start = r["next_start"]
            refs.append(r)
        for a in (feats, perts, graph):
            a.setflags(write=False)
        _TRACK[name] = dict(corners=corners, perts=perts, feats=feats, graph=graph, frames=frames, refs=refs)
    return _TRACK[name]


def _tracker(ctx, case, host_stepped=False, **kw):
    _, am, ssm = case
    old = os.environ.get("MTFHIP_NN_HOST_STEPPED")
    os.environ["MTFHIP_NN_HOST_STEPPED"] = "1" if host_stepped else "0"
    try:
        kw.setdefault("index", "gnn")
        kw.setdefault("gnn_params", dict(degree=GC.TRACK_DEGREE, max_steps=GC.TRACK_MAX_STEPS, start_node=GC.TRACK_START))
        return NNTracker(ctx, am=am, ssm=ssm, resx=GC.TRACK_RES, resy=GC.TRACK_RES, n_samples=GC.TRACK_N, max_iters=GC.TRACK_ITERS,
                         epsilon=GC.TRACK_EPS, **kw)
    finally:
        if old is None:
            del os.environ["MTFHIP_NN_HOST_STEPPED"]
        else:
            os.environ["MTFHIP_NN_HOST_STEPPED"] = old


def _corners8(c24):
    return np.asarray(c24).T.reshape(-1)


@pytest.mark.parametrize("case", GC.TRACK_CASES, ids=lambda c: c[0])
def test_tracker_follows_reference_and_forms_agree(oracle, gpu_ctx, frame, frame2, case):
    d = _track_reference(oracle, frame, frame2, case)
    am = case[1]
    out = {}
    for stepped in (False, True):
        gpu_ctx.set_image(frame)
        t = _tracker(gpu_ctx, case, host_stepped=stepped)
        t.initialize(d["corners"], features=d["feats"], perturbations=d["perts"], graph=d["graph"])
        assert np.array_equal(t.get_graph(), d["graph"])
        rec = []
        for img in d["frames"]:
            gpu_ctx.set_image(img)
            c = t.update()
            rec.append((c.copy(), t.n_iters, t.log.copy(), t.walk_starts.copy(), t.walk_steps.copy(), t.batch.nn_gnn_get_start(t._h)))
        out[stepped] = rec
        t.close()
    for f, (rec, ref) in enumerate(zip(out[False], d["refs"])):
        c, n_iters, log, starts, steps, next_start = rec
        assert ref["clear"]
        assert n_iters == ref["n_iters"] and log.shape == (n_iters, 3)
        assert np.array_equal(log[:, 0], ref["log"][:, 0]), f
        assert np.array_equal(starts, ref["starts"]) and np.array_equal(steps, ref["steps"]), f
        assert next_start == ref["next_start"]
        for i in range(n_iters):
            want = ref["log"][i, 1]
            err = abs(log[i, 1] - want)
            print("%s frame %d it=%d idx=%d start=%d steps=%d dist err=%.3e" % (case[0], f, i, int(log[i, 0]), starts[i], steps[i], err))
            assert err <= (1e-8 if am == 0 else 1e-9) * abs(want)
        print("%s frame %d corners err=%.3e" % (case[0], f, np.abs(_corners8(c) - ref["corners"]).max()))
        np.testing.assert_allclose(_corners8(c), ref["corners"], rtol=0, atol=1e-9)
    # the start node is carried: across iterations (a walk starts where the last one ended) and across frames
    for f in range(1, 3):
        assert out[False][f][3][0] == out[False][f - 1][5]
    for rec in out[False]:
        assert np.array_equal(rec[3][1:], rec[2][:-1, 0].astype(np.int32))
    assert out[False][0][3][0] == GC.TRACK_START
    # the host-stepped loop: the same kernels one iteration per call -- the same bits
    for ra, rb in zip(out[False], out[True]):
        for a, b_ in zip(ra, rb):
            assert np.array_equal(np.asarray(a), np.asarray(b_))


def test_cpp_driver_equals_python_driver(gpu_ctx, frame, frame2):
    """mtf::hip::NN with NNParams::index_type = GNN against sm.NNTracker(index="gnn"): the same draws, the same graph, the same walks"""
    from mtf_amd import host
    lib = host.lib()
    res, n, iters, seed = GC.TRACK_RES, GC.TRACK_N, 3, 21
    sg = np.zeros((2, 8)); sg[0] = NC.SIGMA_H * 0.3; sg[1] = NC.SIGMA_H
    cnt = np.array([63, n - 63], dtype=np.int32)
    corners = NC.track_corners(res)
    frames = _track_frames(frame, frame2)
    t = lib.mtfhost_nn_create_gnn(L.AM_SSD, L.SSM_HOMOGRAPHY, res, res, n, iters, 0.0, 2, sg.ctypes.data, None, cnt.ctypes.data, seed, 0, 1,
                                  GC.TRACK_DEGREE, GC.TRACK_MAX_STEPS, 0, 0, GC.TRACK_START)
    assert t, lib.mtfhost_last_error()
    c8 = np.ascontiguousarray(corners.T).reshape(-1)
    assert lib.mtfhost_set_image(t, frame.ctypes.data, frame.shape[0], frame.shape[1], frame.shape[1]) == 0, lib.mtfhost_last_error()
    assert lib.mtfhost_initialize(t, c8.ctypes.data) == 0, lib.mtfhost_last_error()
    cpp = []
    for img in frames:
        assert lib.mtfhost_set_image(t, img.ctypes.data, img.shape[0], img.shape[1], img.shape[1]) == 0, lib.mtfhost_last_error()
        it = ctypes.c_int()
        assert lib.mtfhost_update(t, ctypes.byref(it)) == 0, lib.mtfhost_last_error()
        out, log = np.empty(8), np.zeros((iters, 3))
        st, ns = np.zeros(iters, dtype=np.int32), np.zeros(iters, dtype=np.int32)
        assert lib.mtfhost_get_region(t, out.ctypes.data) == 0 and lib.mtfhost_nn_log(t, log.ctypes.data, iters) == it.value == iters
        assert lib.mtfhost_nn_walks(t, st.ctypes.data, ns.ctypes.data, iters) == iters
        cpp.append((out.reshape(4, 2).T.copy(), log, st, ns))
    lib.mtfhost_destroy(t)
    gpu_ctx.set_image(frame)
    p = NNTracker(gpu_ctx, n_samples=n, resx=res, resy=res, ssm_sigma=(sg[0], sg[1]), distr_n_samples=[63, n - 63], max_iters=iters, epsilon=0.0,
                  seed=seed, index="gnn", gnn_params=dict(degree=GC.TRACK_DEGREE, max_steps=GC.TRACK_MAX_STEPS, start_node=GC.TRACK_START))
    p.initialize(corners)
    feats, _ = p.get_dataset()
    _check_graph(p.get_graph(), feats, G.all_distances(feats), GC.TRACK_DEGREE, R.SSD, "built tracker graph")
    for img, (c_cpp, log, st, ns) in zip(frames, cpp):
        gpu_ctx.set_image(img)
        c = p.update()
        assert np.array_equal(c_cpp, c) and np.array_equal(log, p.log)
        assert np.array_equal(st, p.walk_starts) and np.array_equal(ns, p.walk_steps)
    p.close()


def test_random_start(oracle, gpu_ctx, frame, frame2):
    """two handles with one seed walk identically; the reported starts lie in range and, fed to the reference, reproduce the walks"""
    case = GC.TRACK_CASES[0]
    d = _track_reference(oracle, frame, frame2, case)
    recs = []
    for _ in range(2):
        gpu_ctx.set_image(frame)
        t = _tracker(gpu_ctx, case, gnn_params=dict(degree=GC.TRACK_DEGREE, max_steps=GC.TRACK_MAX_STEPS, random_start=True, seed=99))
        t.max_iters = 1
        t.initialize(d["corners"], features=d["feats"], perturbations=d["perts"], graph=d["graph"])
        rec = []
        for img in d["frames"] + d["frames"]:
            gpu_ctx.set_image(img)
            t.update()
            rec.append((int(t.log[0, 0]), t.log[0, 1], int(t.walk_starts[0]), int(t.walk_steps[0])))
        recs.append(rec)
        t.close()
    assert recs[0] == recs[1]
    starts = [r[2] for r in recs[0]]
    assert all(0 <= s < GC.TRACK_N for s in starts) and len(set(starts)) > 1
    o_ssm = oracle.SSM(case[2], GC.TRACK_RES, GC.TRACK_RES); o_am = oracle.AM(case[1], GC.TRACK_RES, GC.TRACK_RES)
    o_am.set_curr_img(frame); o_ssm.set_corners(d["corners"]); o_am.initialize_pix_vals(o_ssm.get("curr_pts"))
    for img, (idx, dist, start, steps) in zip(d["frames"] + d["frames"], recs[0]):
        o_am.set_curr_img(img)
        r = G.nn_update_gnn(o_am, o_ssm, d["feats"], d["perts"], d["graph"], start, GC.TRACK_MAX_STEPS, 1, 0.0)
        assert r["clear"]
        assert (idx, steps) == (int(r["log"][0, 0]), int(r["steps"][0])) and abs(dist - r["log"][0, 1]) <= 1e-8 * abs(r["log"][0, 1])


@pytest.mark.parametrize("case", [GC.TRACK_CASES[0], GC.TRACK_CASES[3]], ids=lambda c: c[0])
def test_exact_index_is_unchanged(gpu_ctx, frame, frame2, case):
    """index="exact" is the tracker built without the new arguments: the same bits"""
    _, am, ssm = case
    corners = NC.track_corners(GC.TRACK_RES)
    out = []
    for kw in (dict(), dict(index="exact"), dict(index="exact", gnn_params=dict(degree=4))):
        gpu_ctx.set_image(frame)
        t = NNTracker(gpu_ctx, am=am, ssm=ssm, resx=GC.TRACK_RES, resy=GC.TRACK_RES, n_samples=GC.TRACK_N, max_iters=3, epsilon=0.0, seed=5, **kw)
        t.initialize(corners)
        gpu_ctx.set_image(frame2)
        out.append((t.update().copy(), t.log.copy()))
        t.close()
    for c, log in out[1:]:
        assert np.array_equal(c, out[0][0]) and np.array_equal(log, out[0][1])


def test_refusals(gpu_ctx, frame):
    b = _batch(gpu_ctx, (7, 7), R.SSD)
    n = 1100
    m = GC.rows(n, 49, R.SSD, 1)
    h = b.nn_create(n)
    with pytest.raises(mtf_amd.LogicError, match="nn_gnn_build before"):
        b.nn_gnn_build(h, dict(degree=4))
    b.nn_set_dataset(h, m, np.zeros((n, 8)))
    for deg in (1024, 0, 2000):                                    # degree + 1 > 1024, asked for or effective
        with pytest.raises(mtf_amd.FunctionNotImplemented, match="1024"):
            b.nn_gnn_build(h, dict(degree=deg))
        with pytest.raises(mtf_amd.FunctionNotImplemented, match="1024"):
            b.nn_gnn_set_graph(h, np.zeros((n, 1024), dtype=np.int32), dict(degree=deg))
    with pytest.raises(mtf_amd.LogicError, match="nn_gnn_build"):    # no graph yet
        b.nn_gnn_search(h, m[:2], [0, 1])
    with pytest.raises(mtf_amd.LogicError, match="nn_gnn_build"):
        b.nn_gnn_get_graph(h, n)
    b.nn_gnn_build(h, dict(degree=1023))                           # the limit itself builds
    assert b.nn_gnn_get_graph(h, n).shape == (n, 1023)
    b.nn_gnn_build(h, dict(degree=3))
    assert b.nn_gnn_search(h, m[:2], [0, 1])[0].tolist() == [0, 1]
    with pytest.raises(mtf_amd.InvalidArgument, match="start node"):
        b.nn_gnn_search(h, m[:2], [0, n])
    with pytest.raises(mtf_amd.InvalidArgument):
        b.nn_gnn_set_start(h, n)
    with pytest.raises(mtf_amd.InvalidArgument, match="not a row"):
        b.nn_gnn_set_graph(h, np.full((n, 3), n, dtype=np.int32), dict(degree=3))
    b.nn_set_dataset(h, m, np.zeros((n, 8)))                       # a new dataset: the graph is gone
    with pytest.raises(mtf_amd.LogicError, match="invalidates"):
        b.nn_gnn_search(h, m[:2], [0, 1])
    b.nn_destroy(h); b.close()
    # update() with the GNN index and no graph
    gpu_ctx.set_image(frame)
    t = NNTracker(gpu_ctx, resx=7, resy=7, n_samples=50, index="exact")
    t.initialize(NC.track_corners(7))
    t.batch.nn_set_index(t._h, "gnn")
    with pytest.raises(mtf_amd.LogicError, match="nn_update with the GNN index"):
        t.update()
    t.batch.nn_gnn_build(t._h, dict(degree=4))
    t.update()
    t.batch.nn_build(t._h, [t.batch.nn_desc(50, t.ds.sigmas[0], t.ds.means[0], 3)])   # rebuilt rows: the graph is gone again
    with pytest.raises(mtf_amd.LogicError):
        t.update()
    t.close()
