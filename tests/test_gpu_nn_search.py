"""nt::NN's exact search on the device (mtfhip_nn_search / _dev, k_nn_search) against tests/helpers/nn_ref.py: random matrices handed over
through set_dataset, so both sides see identical features.  The index must equal the reference's (its gap condition asserted first); the
distance must lie within the bound that follows from the arithmetic -- every product rounded once, a sum of feat_size terms in any order,
and a factor 4 for the subtraction's own rounding:
    SSD  |d - ref| <= 4 (feat_size + 1) 2^-53 ref           (non-negative terms)
    NCC  |d - ref| <= 4 (feat_size + 1) 2^-53 ||a|| ||b||"""
import os
import sys

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import nn_cases as NC   # noqa: E402
import nn_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def _bound(am, F, ref, row, q):
    return 4 * (F + 1) * U * (ref if am == R.SSD else np.linalg.norm(row) * np.linalg.norm(q))


def _batch(ctx, shape, am):
    rx, ry, ch = shape
    return mtf_amd.Batch(ctx, L.AM_NCC if am == R.NCC else L.AM_SSD, L.SSM_HOMOGRAPHY, rx, ry, 1, n_channels=ch)


@pytest.mark.parametrize("am", [R.SSD, R.NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("shape", NC.SEARCH_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_search_equals_reference(gpu_ctx, shape, am):
    F = shape[0] * shape[1] * shape[2]
    m = NC.search_matrix(F, am)
    b = _batch(gpu_ctx, shape, am)
    assert b.nn_feature_size() == F
    worst = 0.0
    for n in NC.SEARCH_N:
        h = b.nn_create(n)
        b.nn_set_dataset(h, m[:n], np.zeros((n, 8)))
        for pos in NC.planted_positions(n):
            qs = NC.search_queries(m, n, pos, am, seed=n + pos)
            want = [R.nearest(m[:n], q, am) for q in qs]
            for Q in NC.SEARCH_Q:
                idx, dist = b.nn_search(h, qs[:Q])
                idx2, dist2 = b.nn_search(h, qs[:Q])
                assert np.array_equal(idx, idx2) and np.array_equal(dist.view(np.uint64), dist2.view(np.uint64))   # two calls, the same bits
                for j in range(Q):
                    k, best, second = want[j]
                    assert n == 1 or R.gap_ok(best, second)
                    assert idx[j] == k, (n, pos, Q, j)
                    err, bound = abs(dist[j] - best), _bound(am, F, best, m[k], qs[j])
                    print("F=%d n=%d pos=%d Q=%d j=%d err=%.3e bound=%.3e" % (F, n, pos, Q, j, err, bound))
                    assert err <= bound, (n, pos, Q, j, err, bound)
                    worst = max(worst, err / bound)
                assert idx[0] == pos
        b.nn_destroy(h)
    print("worst err / bound = %.3f" % worst)
    b.close()


@pytest.mark.parametrize("am", [R.SSD, R.NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("shape", [(7, 7, 1), (25, 25, 1), (24, 24, 1)], ids=lambda s: "%dx%dx%d" % s)
def test_duplicates_go_to_the_lower_index(gpu_ctx, shape, am):
    """exact copies of the best row at two indices -- with an odd feat_size one copy starts on a 16-byte boundary and one does not, and they
    sit in different waves and workgroups -- have equal distances, and the lower index wins"""
    F = shape[0] * shape[1]
    m = NC.search_matrix(F, am)[:257].copy()
    q = NC.search_queries(m, 257, 100, am, seed=9)[:1]
    b = _batch(gpu_ctx, shape, am)
    h = b.nn_create(257)
    for lo, hi in ((100, 201), (7, 256), (0, 1), (64, 65), (101, 200)):
        mm = m.copy()
        mm[lo] = m[100]; mm[hi] = m[100]
        if lo != 100 and hi != 100:
            mm[100] = m[99]
        b.nn_set_dataset(h, mm, np.zeros((257, 8)))
        idx, dist = b.nn_search(h, q)
        assert idx[0] == lo, (lo, hi, idx)
        solo = mm.copy(); solo[lo] = m[98]
        b.nn_set_dataset(h, solo, np.zeros((257, 8)))
        idx2, dist2 = b.nn_search(h, q)
        assert idx2[0] == hi and dist2[0] == dist[0]          # the same row stored elsewhere: the same bits
    b.nn_destroy(h); b.close()


def test_dev_twin_equals_host_form(gpu_ctx):
    import torch
    shape, am, n = (25, 25, 1), R.SSD, 257
    m = NC.search_matrix(625, am)
    qs = NC.search_queries(m, n, 5, am, seed=3)
    b = _batch(gpu_ctx, shape, am)
    h = b.nn_create(n)
    fd, pd = torch.from_numpy(m[:n]).to("cuda:0"), torch.zeros((n, 8), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    b.nn_set_dataset_dev(h, fd.data_ptr(), pd.data_ptr())
    qd = torch.from_numpy(qs).to("cuda:0")
    idx_d = torch.full((3,), -7, dtype=torch.int32, device="cuda:0"); dist_d = torch.zeros(3, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    b.nn_search_dev(h, qd.data_ptr(), 3, idx_d.data_ptr(), dist_d.data_ptr())
    gpu_ctx.synchronize()
    idx, dist = b.nn_search(h, qs)
    assert np.array_equal(idx_d.cpu().numpy(), idx) and np.array_equal(dist_d.cpu().numpy().view(np.uint64), dist.view(np.uint64))
    # get_dataset returns what set_dataset_dev was given
    f, p = b.nn_get_dataset(h, n)
    assert np.array_equal(f, m[:n]) and not p.any()
    out = torch.zeros_like(fd)
    b.nn_get_dataset_dev(h, out.data_ptr(), None)
    gpu_ctx.synchronize()
    assert torch.equal(out, fd)
    b.nn_destroy(h); b.close()


def test_refusals_name_their_reason(gpu_ctx, frame):
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, L.AM_MI, L.SSM_HOMOGRAPHY, 10, 10, 1)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="MI"):
        b.nn_create(10)
    b.close()
    b = mtf_amd.Batch(gpu_ctx, L.AM_SCV, L.SSM_HOMOGRAPHY, 10, 10, 1)
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="SCV"):
        b.nn_create(10)
    b.close()
    b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, 60, 50, 1, n_channels=3)     # 9000 entries
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="feat_size 9000"):
        b.nn_create(10)
    b.close()
    b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, 10, 10, 2)
    with pytest.raises(mtf_amd.InvalidArgument, match="one template"):
        b.nn_create(10)
    b.close()
    b = mtf_amd.Batch(gpu_ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, 10, 10, 1)
    h = b.nn_create(10)
    d = b.nn_desc(10, np.full(8, 0.01))
    d.additive_update = 1
    with pytest.raises(mtf_amd.FunctionNotImplemented, match="additive_update"):
        b.nn_build(h, [d])
    d.additive_update = 0
    with pytest.raises(mtf_amd.InvalidArgument, match="the handle 10"):
        b.nn_build(h, [b.nn_desc(4, np.full(8, 0.01))])
    with pytest.raises(mtf_amd.LogicError, match="before nn_build"):
        b.nn_search(h, np.zeros((1, 100)))
    with pytest.raises(mtf_amd.LogicError, match="before nn_build"):
        b.nn_update(h, 1, 0.01)
    with pytest.raises(mtf_amd.InvalidArgument, match="max_iters"):
        b.nn_update(h, 0, 0.01)
    b.nn_destroy(h); b.close()
