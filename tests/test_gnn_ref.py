"""tests/helpers/gnn_ref.py on its own (no GPU): the graph build and the walk of gnn::GNN (SM/src/NT/GNN.cc:59-203) on a hand-made 1-D
dataset whose graph and walks are written out by hand, build_graph against a plain lexsort, and the caps tests/test_gpu_gnn.py relies on,
asserted on the reference alone for exactly its seeds and shapes: at most 2 % of a case's neighbour-list positions are not clear of an
adjacent entry (nn_ref.gap_ok), every decision of every walk it compares is clear, and at least one walk per case ends off the exact
nearest row."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gnn_cases as GC   # noqa: E402
import gnn_ref as G      # noqa: E402
import nn_ref as R       # noqa: E402

X = np.arange(8, dtype=np.float64)[:, None] * 10.0      # rows 0, 10, .. 70
CHAIN = np.array([[1, 2], [0, 2], [1, 3], [2, 4], [3, 5], [4, 6], [5, 7], [6, 5]])


def test_walk_ends_at_the_nearest_row():
    w = G.search_graph(X, CHAIN, [31.0], 0, 10)
    # 0 (961) -> 2 (121) -> 3 (1); at 3 the best neighbour is 4 (81): parent_dist 1 <= 81 ends the walk
    assert w["path"] == [0, 2, 3] and w["n_steps"] == 3
    assert w["visited"] == [(0, 961.0), (2, 121.0), (3, 1.0), (4, 81.0)]
    assert (w["idx"], w["dist"], w["next_start"]) == (3, 1.0, 3) and R.nearest(X, [31.0])[0] == 3
    assert G.walk_clear(w)


def test_walk_stops_in_a_local_minimum():
    g = CHAIN.copy()
    g[2] = [1, 0]                                        # node 2 has no edge forward
    w = G.search_graph(X, g, [61.0], 0, 10)
    # 0 (3721) -> 2 (1681); its neighbours 1 (2601) and 0 (3721) are both farther: the walk ends at 2, the nearest row is 6
    assert w["path"] == [0, 2] and w["n_steps"] == 2 and (w["idx"], w["dist"]) == (2, 1681.0)
    assert R.nearest(X, [61.0])[0] == 6


def test_walk_cut_by_max_steps():
    w = G.search_graph(X, CHAIN, [61.0], 0, 2)
    # 0 -> 2 (1681) -> 3 (961), and the two steps are spent
    assert w["path"] == [0, 2, 3] and w["n_steps"] == 2 and (w["idx"], w["dist"]) == (3, 961.0)
    full = G.search_graph(X, CHAIN, [61.0], 0, 10)
    assert full["idx"] == 6 and full["n_steps"] == 6     # 0 -> 2 -> 3 -> 4 -> 5 -> 6, and the step at 6 that ends it
    assert G.search_graph(X, CHAIN, [61.0], 0, 0)["idx"] == 0 and G.search_graph(X, np.zeros((8, 0), dtype=int), [61.0], 5, 10)["n_steps"] == 0


def test_identical_row_at_a_lower_index_makes_a_row_its_own_neighbour():
    x = np.array([[5.0], [1.0], [5.0], [9.0]])           # row 2 is row 0 again
    # row 2's list: (0, row 0), (0, row 2), (16, row 1), (16, row 3): the FIRST entry goes, whatever it is (GNN.cc:98-101)
    assert G.build_graph(x, 1).tolist() == [[2], [0], [2], [0]]
    assert G.build_graph(x, 2).tolist() == [[2, 1], [0, 2], [2, 1], [0, 2]]
    assert G.build_graph(x, 0).tolist() == G.build_graph(x, 3).tolist() == [[2, 1, 3], [0, 2, 3], [2, 1, 3], [0, 2, 1]]


def test_effective_degree():
    assert [G.effective_degree(d, 10) for d in (0, 11, 10, 9, 3, -4, -3, -20)] == [9, 9, 9, 9, 3, 2, 3, 0]
    assert G.effective_degree(0, 1) == 0 and G.effective_degree(-4, 5) == 1


@pytest.mark.parametrize("am", [R.SSD, R.NCC], ids=["ssd", "ncc"])
def test_build_graph_is_a_lexsort_with_the_first_entry_dropped(am):
    m = GC.rows(37, 20, am, 3).copy()
    m[30] = m[4]
    d = G.all_distances(m, am)
    for deg in (1, 5, 36, 0, -4):
        g = G.build_graph(m, deg, am, dmat=d)
        k = G.effective_degree(deg, 37)
        want = np.array([sorted(range(37), key=lambda j: (d[i, j], j))[1:k + 1] for i in range(37)])
        assert g.shape == (37, k) and np.array_equal(g, want)
    assert np.array_equal(d, d.T)


@pytest.mark.parametrize("am", [R.SSD, R.NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("shape", GC.BUILD_SHAPES, ids=lambda s: "%dx%d" % s)
def test_build_cases_keep_the_cap_on_unclear_positions(shape, am):
    F = shape[0] * shape[1]
    for n in GC.BUILD_N:
        m, d = GC.build_case(n, F, am)
        for deg in GC.build_degrees(n):
            if G.effective_degree(deg, n) == 0:
                continue
            _, dist = G.neighbour_lists(d, deg)
            share = G.unclear_positions(dist).mean()
            print("n=%d F=%d am=%d degree=%d: %.4f %% of positions unclear" % (n, F, am, deg, 100 * share))
            assert share <= 0.02


@pytest.mark.parametrize("am", [R.SSD, R.NCC], ids=["ssd", "ncc"])
@pytest.mark.parametrize("F", [49, 625])
def test_duplicated_rows_tie_exactly_and_nothing_else_is_close(F, am):
    m = GC.dup_rows(F, am)
    d = G.all_distances(m, am)
    idx, dist = G.neighbour_lists(d, GC.DUP_N - 1)
    gap = np.diff(dist[:, :GC.DUP_N], axis=1)
    assert np.all((gap == 0) | (gap > 1e-6 * np.maximum(np.abs(dist[:, :GC.DUP_N - 1]), 1.0)))   # a tie is exact or there is none
    g = G.build_graph(m, GC.DUP_N - 1, am, dmat=d)
    for dst, src in GC.DUP_COPIES:
        twins = [j for j in range(GC.DUP_N) if np.array_equal(m[j], m[dst])]
        assert g[dst, 0] == twins[1] and g[twins[0], 0] == twins[1]      # the lowest twin goes: every other one keeps itself as a neighbour
        assert dst in g[dst]
    assert (gap == 0).sum() >= len(GC.DUP_COPIES)


@pytest.mark.parametrize("case", GC.WALK_CASES, ids=lambda c: c[0])
def test_walk_cases_are_clear_and_not_all_exact(case):
    w = GC.walk_case(case)
    off = 0
    for ms in GC.WALK_MAX_STEPS:
        for j, r in enumerate(w["walks"][ms]):
            assert G.walk_clear(r), (ms, j)
            k, best, second = w["exact"][j]
            assert R.gap_ok(best, second)
            off += r["idx"] != k
    print("%s: %d of %d walks end off the exact nearest row" % (case[0], off, len(GC.WALK_MAX_STEPS) * GC.WALK_Q))
    assert off >= 1
    assert len({r["n_steps"] for r in w["walks"][10]}) > 1      # the walks differ in length
