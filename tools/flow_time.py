#!/usr/bin/env python
"""Times the device optical flow (Context.estimate_optical_flow, one launch of k_ncc_flow per call) and GridTrackerFlow.update() and writes
profiles/flow_timing.md.

  python tools/flow_time.py [--calls 40] [--rounds 3] [--out profiles/flow_timing.md]

Shapes: 100 points x 10 x 10 (the reference's defaults: grid 10, window 10) and 400 points x 25 x 25; max_iters 30 with epsilon 0.01 (points
stop when they converge) and with epsilon 0 (every pass of every point runs); both arithmetic modes.  The yardstick a reader knows runs in the
same process, alternating call by call: GridTracker.update() (ICLK + NCC + affine patches in one launch, re-initialised every frame) at the
same point count and patch size.  Wall clock around the call behind a device synchronise (the call returns with its results on the host);
5 warm-up calls, then the median of `calls` calls; the whole measurement is repeated `rounds` times and the table gives the median of the
rounds' medians and their range.  The state (images, points, region) is restored in front of every call, outside the clock.  Reads nothing
outside the repository."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mtf_amd                                             # noqa: E402
from mtf_amd import _lib as L                              # noqa: E402
from mtf_amd import host, synth                            # noqa: E402
from mtf_amd.sm import GridTracker, GridTrackerFlow        # noqa: E402

MAX_ITERS, WARM = 30, 5
MODES = [(L.MATH_REPLAY, "replay"), (L.MATH_FAST, "tolerance")]
SHAPES = [(10, 10), (20, 25)]          # grid size, window / patch size


def region_for(win):
    return synth.square_corners(256.0, 256.0, 400 if win > 10 else 300)


def one_round(ctx, f0, f1, grid, win, calls):
    region = region_for(win)
    rows = {}
    flows = {(eps, m): GridTrackerFlow(ctx, grid_size=grid, search_window=win, max_iters=MAX_ITERS, epsilon=eps, math=m)
             for eps in (0.01, 0.0) for m, _ in MODES}
    # the same frame with the device estimator behind the flow (est_params, plain least squares: both launches enqueued back to back),
    # and through the C++ driver mtf::hip::GridFlow with its built-in least-squares fit (no NumPy in the fit)
    chained = {key: GridTrackerFlow(ctx, grid_size=grid, search_window=win, max_iters=MAX_ITERS, epsilon=key[0], math=key[1],
                                    est_params=L.est_params(L.EST_LEAST_SQUARES)) for key in flows}
    cpp = {key: host.CppGridTrackerFlow(grid_size=grid, search_window=win, max_iters=MAX_ITERS, epsilon=key[0], math=key[1]) for key in flows}
    t_chain = {k: [] for k in flows}
    t_cpp = {k: [] for k in flows}
    ctx.set_image(f0)
    yard = GridTracker(ctx, grid_size=grid, patch_size=win, am=L.AM_NCC, ssm=L.SSM_AFFINE, max_iters=MAX_ITERS)
    t_call = {k: [] for k in flows}
    t_upd = {k: [] for k in flows}
    t_yard, passes = [], {}
    try:
        for k in range(WARM + calls):
            for key, g in flows.items():
                eps, m = key
                ctx.set_image(f0); ctx.keep_prev(); ctx.set_image(f1)
                g.set_region(region)
                pts = g.prev_pts.copy()
                ctx.synchronize()
                t0 = time.perf_counter()
                _, ni, st = ctx.estimate_optical_flow(pts, (win, win), MAX_ITERS, eps, False, m)
                t1 = time.perf_counter()
                g.update()          # (raises LogicError if a point is lost: the figures below would not mean anything then)
                t2 = time.perf_counter()
                passes[key] = float(ni.mean())
                c, h = chained[key], cpp[key]
                ctx.set_image(f0); ctx.keep_prev(); ctx.set_image(f1)
                c.set_region(region)
                ctx.synchronize()
                t3 = time.perf_counter()
                c.update()
                t4 = time.perf_counter()
                h.set_image(f0); h.initialize(region); h.set_image(f1)
                t5 = time.perf_counter()
                h.update()
                t6 = time.perf_counter()
                if k >= WARM:
                    t_call[key].append((t1 - t0) * 1e6); t_upd[key].append((t2 - t1) * 1e6)
                    t_chain[key].append((t4 - t3) * 1e6); t_cpp[key].append((t6 - t5) * 1e6)
            ctx.set_image(f0)
            yard.initialize(region)
            ctx.set_image(f1)
            ctx.synchronize()
            t0 = time.perf_counter()
            yard.update()
            t1 = time.perf_counter()
            if k >= WARM:
                t_yard.append((t1 - t0) * 1e6)
        for key in flows:
            rows[key] = (float(np.median(t_call[key])), float(np.median(t_upd[key])), passes[key], float(np.median(t_chain[key])),
                         float(np.median(t_cpp[key])))
        rows["yard"] = (float(np.median(t_yard)), float(np.mean(yard.n_iters)))
    finally:
        yard.tracker.batch.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_timing.md"))
    args = ap.parse_args()
    ctx = mtf_amd.Context(0)
    f0 = synth.make_frame(512, 512)
    f1 = synth.warp_frame(f0, np.array([0.0, 0.0, 1.3, 0.0, 0.0, -0.8, 0.0, 0.0]), (256.0, 256.0))
    lines = ["# The device optical flow (k_ncc_flow) and GridTrackerFlow.update(): wall-clock time per call", "",
             "Written by `tools/flow_time.py --calls %d --rounds %d` on one MI355X.  Microseconds per call, wall clock behind a device synchronise"
             % (args.calls, args.rounds),
             "(the call returns with its results on the host); %d warm-up calls, the median of %d calls, and of that the median [min .. max] over %d"
             % (WARM, args.calls, args.rounds),
             "repeated rounds.  512 x 512 frames, the second shifted by (1.3, -0.8); max_iters %d; `passes`: mean passes per point.  `flow`: one" % MAX_ITERS,
             "Context.estimate_optical_flow call (upload of the points, one launch, download); `update`: one GridTrackerFlow.update() (the flow, the",
             "least-squares fit in NumPy, keep_prev); `update, est_params`: the same with the device estimator (plain least squares) enqueued behind",
             "the flow, one wait; `update, C++`: mtf::hip::GridFlow::update() with its built-in least-squares fit.  Yardstick, alternating in the same",
             "process: GridTracker.update() (ICLK + NCC + affine, one launch, patches re-initialised every frame, the NumPy fit) at the same point",
             "count and patch size.", "",
             "| points x window | epsilon | mode | passes | flow | update | update, est_params | update, C++ |", "|---|---|---|---|---|---|---|---|"]
    for grid, win in SHAPES:
        rounds = [one_round(ctx, f0, f1, grid, win, args.calls) for _ in range(args.rounds)]

        def cell(vals):
            return "%.1f [%.1f .. %.1f]" % (float(np.median(vals)), min(vals), max(vals))
        for eps in (0.01, 0.0):
            for m, name in MODES:
                row = "| %d x %d x %d | %g | %s | %.2f | %s | %s | %s | %s |" % (
                    grid * grid, win, win, eps, name, rounds[0][(eps, m)][2], cell([r[(eps, m)][0] for r in rounds]),
                    cell([r[(eps, m)][1] for r in rounds]), cell([r[(eps, m)][3] for r in rounds]), cell([r[(eps, m)][4] for r in rounds]))
                print(row, flush=True)
                lines.append(row)
        row = "| %d x %d x %d | 1e-4 | GridTracker.update() (yardstick) | %.2f | | %s | | |" % (grid * grid, win, win, rounds[0]["yard"][1],
                                                                                          cell([r["yard"][0] for r in rounds]))
        print(row, flush=True)
        lines.append(row)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
