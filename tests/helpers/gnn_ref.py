"""A NumPy restatement of nt::NN's graph index gnn::GNN (SM/src/NT/GNN.cc) on nn_ref's extended-precision distances: the graph build
(buildGraph, GNN.cc:59-113), the greedy walk (searchGraph with K = 1, GNN.cc:115-203) and NN::update with the walk in place of the
exhaustive search (NT/NN.cc:236-277 with NN.cc:250-251).  Every decision a walk takes comes back with its gap (runner-up - best), so that a
test can assert the decision is clear (nn_ref.gap_ok) before it compares an index."""
import numpy as np

import nn_ref as R


def effective_degree(degree, n):
    """GNN's constructor (GNN.cc:15-19: 0 or > n -> n; negative -> -n / degree, C's division), then at most n - 1 (at degree = n the reference
    reads a list slot its loop never filled, GNN.cc:66, 98-100)"""
    if degree == 0 or degree > n:
        degree = n
    elif degree < 0:
        degree = n // (-degree)
    return min(degree, n - 1)


def all_distances(features, am=R.SSD):
    """computeDistances (GNN.cc:30-57): the functor between every two rows -> float64 (n, n)"""
    f = np.asarray(features)
    return np.stack([R.distances(f, f[i], am) for i in range(len(f))])


def neighbour_lists(dmat, degree):
    """buildGraph's insertion loop (GNN.cc:71-97) for every row: the degree + 1 smallest entries of the row under (dist ascending, index
    ascending), sorted -> (idx (n, degree + 1), dist (n, degree + 2): the list's distances and the first one left out, inf if none)"""
    n = len(dmat)
    deg = effective_degree(degree, n)
    idx = np.empty((n, deg + 1), dtype=np.int64)
    dist = np.full((n, deg + 2), np.inf)
    ar = np.arange(n)
    for i in range(n):
        order = np.lexsort((ar, dmat[i]))
        idx[i] = order[:deg + 1]
        m = min(deg + 2, n)
        dist[i, :m] = dmat[i][order[:m]]
    return idx, dist


def build_graph(features, degree, am=R.SSD, dmat=None):
    """buildGraph: the neighbours are entries 1 .. degree of the sorted list; the first entry is dropped whatever it is (GNN.cc:98-101)
    -> int32 (n, effective degree)"""
    d = all_distances(features, am) if dmat is None else dmat
    return neighbour_lists(d, degree)[0][:, 1:].astype(np.int32)


def unclear_positions(dist):
    """of neighbour_lists' dist: True where a neighbour position (entries 1 .. degree) is not clear of either adjacent entry -> (n, degree)"""
    lo, hi = dist[:, :-1], dist[:, 1:]
    with np.errstate(invalid="ignore"):
        ok = np.isinf(hi) | (hi - lo > 1e-6 * np.maximum(np.abs(lo), 1.0))   # nn_ref.gap_ok, entries k and k + 1 apart
    return ~(ok[:, :-1] & ok[:, 1:])


def search_graph(features, graph, q, start, max_steps, am=R.SSD):
    """searchGraph with K = 1 (GNN.cc:115-203) -> dict(idx, dist, path (the nodes the walk stood on), n_steps (steps taken, the ending one
    included), visited [(node, dist)], decisions [(best, runner_up)]: every comparison the result depends on -- per step the best neighbour
    against the second best (GNN.cc:141-165) and against parent_dist (GNN.cc:180), at the end the best visited node against the next
    (GNN.cc:191) --, next_start (GNN.cc:198))"""
    f = np.asarray(features)
    graph = np.asarray(graph).reshape(len(f), -1)
    r = int(start)
    parent = float(R.distances(f[r:r + 1], q, am)[0])               # GNN.cc:127-128
    visited, path, decisions, steps = [(r, parent)], [r], [], 0
    for _ in range(max_steps):                                      # GNN.cc:134
        nb = graph[r]
        if len(nb) == 0:
            break
        steps += 1
        d = R.distances(f[nb], q, am)
        pos = int(np.lexsort((np.arange(len(nb)), d))[0])           # (dist, position in the list): GNN.cc:150-164
        best = float(d[pos])
        others = np.delete(d, pos)
        if len(others):
            decisions.append((best, float(others.min())))
        visited.append((int(nb[pos]), best))                        # GNN.cc:174-178
        decisions.append((min(parent, best), max(parent, best)))
        if parent <= best:                                          # GNN.cc:180-183
            break
        r, parent = int(nb[pos]), best                              # GNN.cc:184-185
        path.append(r)
    k = min(range(len(visited)), key=lambda i: (visited[i][1], i))  # GNN.cc:191: ascending distance; of equals, the first visited
    rest = [v[1] for v in visited if v[0] != visited[k][0]]
    if rest:
        decisions.append((visited[k][1], min(rest)))
    return dict(idx=visited[k][0], dist=visited[k][1], path=path, n_steps=steps, visited=visited, decisions=decisions, next_start=visited[k][0])


def walk_clear(res):
    """every decision of a walk is clear under nn_ref.gap_ok; equal values (a node met twice) decide nothing"""
    return all(b == s or R.gap_ok(b, s) for b, s in res["decisions"])


def nn_update_gnn(o_am, o_ssm, features, perts, graph, start, max_steps, max_iters, eps):
    """nn_ref.nn_update with the walk in place of `nearest` and the start node carried along (GNN.cc:198)
    -> dict(corners, n_iters, log: rows (best_idx, best_dist, update_norm), starts, steps, clear, next_start)"""
    import oracle_py
    am = R.NCC if o_am.kind == 1 else R.SSD
    perts = np.asarray(perts, dtype=np.float64).reshape(len(features), -1)
    log, starts, steps, clear = [], [], [], True
    for _ in range(max_iters):
        o_am.update_pix_vals(o_ssm.get("curr_pts"))
        q = oracle_py.am_dist_feat(o_am)
        w = search_graph(features, graph, q, start, max_steps, am)
        clear = clear and walk_clear(w)
        starts.append(start); steps.append(w["n_steps"])
        start = w["next_start"]
        prev = o_ssm.get("curr_corners").copy()
        o_ssm.compositional_update(perts[w["idx"]])
        un = float(((prev - o_ssm.get("curr_corners")) ** 2).sum())
        log.append((w["idx"], w["dist"], un))
        if un < eps:
            break
    return dict(corners=o_ssm.get("curr_corners").copy(), n_iters=len(log), log=np.array(log), starts=np.array(starts), steps=np.array(steps),
                clear=clear, next_start=start)
