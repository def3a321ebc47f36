#!/usr/bin/env python
"""Times nt::NN's graph index gnn::GNN on the device (mtfhip_nn_gnn_build, and mtfhip_nn_update with either index) and writes
profiles/gnn_timing.md.

  python tools/gnn_time.py [--repeats 200] [--limit 600] [--out profiles/gnn_timing.md]

Per size (1 000 / 10 000 / 100 000 x 2500 SSD, the dataset built on the device at a 50 x 50 template; the shipped GNNParams: degree 250,
max_steps 10) one child process under its own `timeout`; the sizes are chained, and nothing runs after a size that failed or ran out of
time -- the report then says which was the largest size measured.  A child measures
  - the graph build (mtfhip_nn_gnn_build: all-pairs distances in panels, the selection per row) by wall clock, the call synchronises;
  - update() at max_iters 1 by wall clock, median [p10 .. p90], with the GNN index and the exhaustive index ALTERNATING on the same handle
    (mtfhip_nn_set_index), the region reset before every call; the GNN walk once with the start node carried from call to call (what a
    tracker does: GNN.cc:198) and once from node 0 every time;
  - the walk's average step count in both.
Reads nothing outside the repository."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1000, 10000, 100000)
GNN = dict(degree=250, max_steps=10)


def pct(v):
    v = np.sort(np.asarray(v))
    return [float(np.median(v)), float(v[int(0.1 * (len(v) - 1))]), float(v[int(0.9 * (len(v) - 1))])]


def fmt(t):
    return "%.1f [%.1f .. %.1f]" % tuple(t)


def one(n, repeats):
    import mtf_amd
    from mtf_amd import synth
    from mtf_amd.sm import NNTracker
    ctx = mtf_amd.Context(0)
    frame = synth.make_frame(512, 512)
    frame2 = synth.warp_frame(frame, synth.random_small_homography(np.random.default_rng(2026)) * 0.5, (256.0, 256.0))
    corners = synth.square_corners(256.0, 256.0, 100.0)
    ctx.set_image(frame)
    t = NNTracker(ctx, resx=50, resy=50, n_samples=n, ssm_sigma=(0.01, 0.01, 1.0, 0.01, 0.01, 1.0, 5e-5, 5e-5), max_iters=1, epsilon=0.0, seed=1)
    t.initialize(corners)
    ctx.synchronize()
    builds = []
    for _ in range(2 if n <= 10000 else 1):
        t0 = time.perf_counter()
        t.batch.nn_gnn_build(t._h, GNN)
        builds.append(time.perf_counter() - t0)
    degree = t.get_graph().shape[1]
    ctx.set_image(frame2)
    warm = repeats // 10 + 5
    wall = dict(gnn=[], exact=[], cold=[])
    steps = dict(gnn=[], cold=[])
    agree = 0
    for k in range(warm + repeats):
        found = {}
        for kind in ("gnn", "exact", "cold"):
            t.index = "exact" if kind == "exact" else "gnn"
            t.batch.nn_set_index(t._h, t.index)
            if kind == "cold":
                carried = t.batch.nn_gnn_get_start(t._h)
                t.batch.nn_gnn_set_start(t._h, 0)
            t.set_region(corners)
            ctx.synchronize()
            t0 = time.perf_counter()
            t.update()
            t1 = time.perf_counter()
            found[kind] = int(t.log[0, 0])
            if kind == "cold":
                t.batch.nn_gnn_set_start(t._h, carried)
            if k >= warm:
                wall[kind].append((t1 - t0) * 1e6)
                if kind != "exact":
                    steps[kind].append(int(t.walk_steps[0]))
        if k >= warm:
            agree += found["gnn"] == found["exact"]
    t.close(); ctx.close()
    return dict(n=n, degree=int(degree), build_s=min(builds), gnn=pct(wall["gnn"]), exact=pct(wall["exact"]), cold=pct(wall["cold"]),
                steps=float(np.mean(steps["gnn"])), cold_steps=float(np.mean(steps["cold"])), agree=agree / float(repeats))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--limit", type=int, default=600, help="seconds a size may take")
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnn_timing.md"))
    args = ap.parse_args()
    if args.one:
        print("GNN_TIME " + json.dumps(one(args.one, args.repeats)), flush=True)
        return 0
    rows, stopped = [], None
    for n in SIZES:   # chained: a size that fails or runs out of time ends the run
        p = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", str(n), "--repeats", str(args.repeats)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("GNN_TIME ")]
        if p.returncode != 0 or not got:
            stopped = (n, p.returncode)
            sys.stderr.write(p.stdout[-2000:])
            break
        rows.append(json.loads(got[-1][len("GNN_TIME "):]))
        print(got[-1], flush=True)
    lines = ["# nt::NN's graph index (gnn::GNN) on the device: build and update timing", "",
             "Written by `tools/gnn_time.py --repeats %d` on one MI355X.  n x 2500 SSD datasets built on the device, GNNParams as shipped (degree 250," % args.repeats,
             "max_steps 10).  The build (mtfhip_nn_gnn_build: all-pairs distances in panels, the degree + 1 nearest of every row) in seconds by wall",
             "clock.  `update()` at max_iters 1 in microseconds by wall clock, median [p10 .. p90], the GNN index and the exhaustive index alternating on",
             "the same handle with the region reset before every call: \"carried\" starts each walk where the last one ended (GNN.cc:198), \"from node 0\"",
             "sets the start node to 0 before every call.  Steps: the walk's average step count.  Same row: how often the carried walk and the",
             "exhaustive search returned the same row.", "",
             "| dataset | degree | build, s | update() GNN, carried | steps | update() GNN, from node 0 | steps | update() exhaustive | same row |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %d x 2500 | %d | %.3f | %s | %.2f | %s | %.2f | %s | %.2f |" % (r["n"], r["degree"], r["build_s"], fmt(r["gnn"]), r["steps"], fmt(r["cold"]),
                                                                                   r["cold_steps"], fmt(r["exact"]), r["agree"]))
    if stopped:
        lines += ["", "The %d-row size did not finish within %d s (exit status %d): the largest size measured is the last row above." % (stopped[0], args.limit, stopped[1])]
    lines += ["", "A walk is 2 + max_steps launches enqueued back to back (the start nodes, the start node's distance, then one launch per step, whose last",
              "workgroup applies the rule; each returns at once when its walk is done) and one more that hands the result to the pick, against one search",
              "launch of the exhaustive index.  Not measured: the walk's launches by HIP events one by one, and whether the graph and the visited rows",
              "stay in the Infinity Cache between frames."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
