#!/usr/bin/env python
"""Times nt::NN's per-frame half on the device (mtfhip_nn_search / mtfhip_nn_update) and writes profiles/nn_search_timing.md.

  python tools/nn_search_time.py [--repeats 200] [--out profiles/nn_search_timing.md]

Per configuration (1 000 / 10 000 / 100 000 x 2500 SSD, 10 000 x 2500 NCC; the dataset built on the device at a 50 x 50 template):
  - the search launch alone by HIP events (the library's timers, family "nn_search"), median [p10 .. p90] of `repeats` calls, and the
    read bandwidth n_samples x feat_size x 8 bytes / median as a fraction of the 8 TB/s peak;
  - the whole update() by wall clock at max_iters 1 and 5 (epsilon 0: every iteration runs);
  - the baseline: NNDataset.nearest() on the host with the matrix already there (NumPy), fewer repeats at the large sizes.
Reads nothing outside the repository."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mtf_amd                      # noqa: E402
from mtf_amd import _lib as L       # noqa: E402
from mtf_amd import synth           # noqa: E402
from mtf_amd.sm import NNTracker    # noqa: E402

PEAK = 8.0e12


def pct(v):
    v = np.sort(np.asarray(v))
    return float(np.median(v)), float(v[int(0.1 * (len(v) - 1))]), float(v[int(0.9 * (len(v) - 1))])


def fmt(t):
    return "%.1f [%.1f .. %.1f]" % t


def measure(ctx, frame, frame2, am, n, repeats):
    corners = synth.square_corners(256.0, 256.0, 100.0)
    ctx.set_image(frame)
    t = NNTracker(ctx, am=am, resx=50, resy=50, n_samples=n, ssm_sigma=(0.01, 0.01, 1.0, 0.01, 0.01, 1.0, 5e-5, 5e-5), max_iters=1, epsilon=0.0, seed=1)
    t.initialize(corners)
    ctx.set_image(frame2)
    warm = repeats // 10 + 5
    kern, wall = [], {1: [], 5: []}
    for iters in (1, 5):
        t.max_iters = iters
        for k in range(warm + repeats):
            t.set_region(corners)
            ctx.synchronize()
            ctx.timing(True); ctx.timing_reset()
            t0 = time.perf_counter()
            t.update()
            t1 = time.perf_counter()
            if k >= warm:
                wall[iters].append((t1 - t0) * 1e6)
                if iters == 1:
                    kern.append(ctx.timing_get("nn_search")[0] * 1e3)
    ctx.timing(False)
    feats, _ = t.get_dataset()
    q = feats[n // 2] + 0.25
    ds = t.ds
    ds.features = feats
    reps = max(3, min(repeats, int(2e9 / feats.nbytes)))
    host = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        ds.nearest(q)
        host.append((time.perf_counter() - t0) * 1e6)
    t.close()
    ks = pct(kern)
    return dict(n=n, am="SSD" if am == L.AM_SSD else "NCC", kernel=ks, frac=n * 2500 * 8 / (ks[0] * 1e-6) / PEAK, up1=pct(wall[1]), up5=pct(wall[5]),
                host=pct(host[1:]), host_reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_search_timing.md"))
    args = ap.parse_args()
    ctx = mtf_amd.Context(0)
    frame = synth.make_frame(512, 512)
    frame2 = synth.warp_frame(frame, synth.random_small_homography(np.random.default_rng(2026)) * 0.5, (256.0, 256.0))
    rows = [measure(ctx, frame, frame2, am, n, args.repeats) for am, n in ((L.AM_SSD, 1000), (L.AM_SSD, 10000), (L.AM_SSD, 100000), (L.AM_NCC, 10000))]
    ctx.close()
    lines = ["# nt::NN on the device: search and update timing", "",
             "Written by `tools/nn_search_time.py --repeats %d` on one MI355X.  Microseconds, median [p10 .. p90].  The search launch is timed by HIP" % args.repeats,
             "events, `update()` (mtfhip_nn_update through sm.NNTracker: upload of the state, per iteration the query feature, the search and the",
             "pick-and-update launch, one read-back) and the host baseline (NNDataset.nearest(), NumPy, the matrix already on the host) by wall clock.",
             "Bandwidth: n_samples x 2500 x 8 bytes over the median of the search launch, as a fraction of the 8 TB/s peak.", "",
             "| dataset | search launch | of 8 TB/s | update(), max_iters 1 | update(), max_iters 5 | host nearest() | host repeats |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %d x 2500 %s | %s | %.2f | %s | %s | %s | %d |" % (r["n"], r["am"], fmt(r["kernel"]), r["frac"], fmt(r["up1"]), fmt(r["up5"]), fmt(r["host"]), r["host_reps"]))
    lines += ["", "Whether the 200 MB matrix of the 10 000-sample case stays in the 256 MB Infinity Cache between frames was not measured: no counter run was made."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
