"""The cases tests/test_gnn_ref.py (the reference's own caps, no GPU) and tests/test_gpu_gnn.py (the device against the reference) share:
synthetic dataset rows 128 + 40 N(0, 1) from np.random.default_rng with fixed seeds (NCC: centred, unit norm), the build shapes and
degrees, the duplicated-row dataset, the walks' queries and start nodes.  References are computed once per process and never changed."""
import numpy as np

import gnn_ref as G
import nn_ref as R

# ---- build: n_samples x feat_size (49 = 7 x 7 and 625 = 25 x 25 are odd: every second row starts 8 bytes off a 16-byte boundary) ----
BUILD_N = [1, 2, 5, 64, 257, 1000]
BUILD_SHAPES = [(7, 7), (16, 12), (25, 25)]
FULL_DEGREE_MAX_N = 257          # at n = 1000 nearly every row of a full-degree list has a position that is not clear


def build_degrees(n):
    """the degrees asked for at n rows: 1, 4, 16 where n has that many other rows, n - 1, 0 (-> n, clamped to n - 1), -4 (-> n / 4)"""
    out = [d for d in (1, 4, 16) if d <= n - 1]
    if n <= FULL_DEGREE_MAX_N:
        out += [n - 1, 0]
    out.append(-4)
    return sorted(set(out), key=out.index)


def rows(n, F, am, seed):
    m = 128.0 + 40.0 * np.random.default_rng(seed).normal(size=(n, F))
    if am == R.NCC:
        m = m - m.mean(axis=1, keepdims=True)
        m = m / np.linalg.norm(m, axis=1, keepdims=True)
    return m


def build_seed(n, F, am):
    return 1000 * n + F + am


_DMAT = {}


def build_case(n, F, am):
    """(rows, all-pairs distances in extended precision) of a build case, shared and read-only"""
    key = (n, F, am)
    if key not in _DMAT:
        m = rows(n, F, am, build_seed(n, F, am))
        d = G.all_distances(m, am)
        m.setflags(write=False); d.setflags(write=False)
        _DMAT[key] = (m, d)
    return _DMAT[key]


# ---- duplicated rows, at rows of both alignments (odd feat_size: a row's alignment is its index's parity) ----
DUP_N = 40
DUP_COPIES = [(8, 3), (21, 10), (30, 12), (31, 12), (5, 4)]   # (row, the row it copies): 30 and 31 with 12 make a triple


def dup_rows(F, am):
    m = rows(DUP_N, F, am, 77 + F + am).copy()
    for dst, src in DUP_COPIES:
        m[dst] = m[src]
    return m


# ---- walks: (id, am, shape, n, degree) x max_steps, 32 queries near stored rows, starts spread over the rows ----
WALK_CASES = [("ssd-49-d4", R.SSD, (7, 7), 257, 4), ("ssd-625-d16", R.SSD, (25, 25), 300, 16), ("ncc-192-d4", R.NCC, (16, 12), 257, 4),
              ("ncc-49-d16", R.NCC, (7, 7), 300, 16)]
WALK_MAX_STEPS = [1, 3, 10]
WALK_Q = 32
_WALK = {}


def walk_case(case):
    """dict(rows, graph, queries, starts, walks[max_steps]: the reference's walks), shared and read-only"""
    name, am, shape, n, degree = case
    if name not in _WALK:
        F = shape[0] * shape[1]
        seed = 500 + n + F + am
        m = rows(n, F, am, seed)
        rng = np.random.default_rng(seed + 1)
        near = rng.integers(0, n, size=WALK_Q)
        if am == R.NCC:
            q = m[near] + 0.5 / np.sqrt(F) * rng.normal(size=(WALK_Q, F))
            q = q - q.mean(axis=1, keepdims=True)
            q = q / np.linalg.norm(q, axis=1, keepdims=True)
        else:
            q = m[near] + 20.0 * rng.normal(size=(WALK_Q, F))
        starts = ((np.arange(WALK_Q) * n) // WALK_Q + 3) % n
        graph = G.build_graph(m, degree, am)
        walks = {ms: [G.search_graph(m, graph, q[j], starts[j], ms, am) for j in range(WALK_Q)] for ms in WALK_MAX_STEPS}
        exact = [R.nearest(m, q[j], am) for j in range(WALK_Q)]
        for a in (m, q, graph):
            a.setflags(write=False)
        _WALK[name] = dict(rows=m, graph=graph, queries=q, starts=starts.astype(np.int32), walks=walks, exact=exact)
    return _WALK[name]


# ---- the tracker: (id, am, ssm); 300 samples of 25 x 25, degree 16, three frames ----
TRACK_CASES = [("ssd-hom", 0, 0), ("ncc-hom", 1, 0), ("ssd-aff", 0, 1), ("ncc-aff", 1, 1)]
TRACK_N, TRACK_RES, TRACK_DEGREE, TRACK_MAX_STEPS, TRACK_ITERS, TRACK_EPS, TRACK_START = 300, 25, 16, 10, 4, 1e-4, 7
