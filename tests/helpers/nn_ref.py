"""A float64 restatement of nt::NN's per-frame half (SM/src/NT/NN.cc:236-277) with the exhaustive index: the distance functors
SSDBaseDist::operator() (AM/src/SSDBase.cc:576-603: sum (a - b)^2) and NCCDist::operator() (AM/src/NCC.cc:568-591: -sum a b) as sums in
extended precision, the nearest row with its runner-up (the gap the tests assert before they compare an index), and NN::update driven through
the oracle's appearance model and state space model."""
import numpy as np

SSD, NCC = 0, 1
LD = np.longdouble


def ssd_dist(a, b):
    d = np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)
    return float((d * d).sum(dtype=LD))


def ncc_dist(a, b):
    return float(-(np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD)).sum(dtype=LD))


def distances(features, q, am=SSD):
    """the functor's value for every row, in extended precision -> float64 (n,)"""
    f = np.asarray(features, dtype=LD)
    qq = np.asarray(q, dtype=LD)[None]
    if am == NCC:
        return np.asarray(-(f * qq).sum(axis=1, dtype=LD), dtype=np.float64)
    d = f - qq
    return np.asarray((d * d).sum(axis=1, dtype=LD), dtype=np.float64)


def nearest(features, q, am=SSD):
    """(index, best distance, second-best distance) of the exhaustive search; of equal distances the first index; second = inf for one row"""
    d = distances(features, q, am)
    k = int(np.argmin(d))
    rest = np.delete(d, k)
    return k, float(d[k]), float(rest.min()) if len(rest) else float("inf")


def gap_ok(best, second):
    """the condition under which an index is compared at all: the runner-up is clear of the winner by far more than any rounding"""
    return second - best > 1e-6 * max(abs(best), 1.0)


def nn_update(o_am, o_ssm, features, perts, max_iters, eps):
    """NN::update (NN.cc:236-277, compositional): per iteration updatePixVals, updateDistFeat, the search, compositionalUpdate(
    perts[best_idx]), update_norm = ||prev_corners - corners||^2; stops behind the iteration whose update_norm < eps.
    -> dict(corners (8,) as the oracle lays them out, n_iters, log: rows (best_idx, best_dist, second_dist, update_norm))"""
    import oracle_py
    am = NCC if o_am.kind == 1 else SSD
    perts = np.asarray(perts, dtype=np.float64).reshape(len(features), -1)
    log = []
    for _ in range(max_iters):
        o_am.update_pix_vals(o_ssm.get("curr_pts"))
        q = oracle_py.am_dist_feat(o_am)
        k, best, second = nearest(features, q, am)
        prev = o_ssm.get("curr_corners").copy()
        o_ssm.compositional_update(perts[k])
        un = float(((prev - o_ssm.get("curr_corners")) ** 2).sum())
        log.append((k, best, second, un))
        if un < eps:
            break
    return dict(corners=o_ssm.get("curr_corners").copy(), n_iters=len(log), log=np.array(log))
