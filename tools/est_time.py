#!/usr/bin/env python
"""Times the device grid-SSM estimator (mtfhip_ssm_estimate_from_pts) and what it costs a grid frame.

  python tools/est_time.py [--repeats 200] [--frames 300]

Per configuration: the kernel by HIP events (the library's own timers, family "est") and the whole call by wall clock (upload, launch,
download, synchronisation), median and the 10th / 90th percentile over `repeats` calls after a warm-up of repeats / 10 + 5.
  - the shipped LMedS size: 100 points, 55 hypotheses, refine 1 (Config/modules.cfg:37-45);
  - RANSAC at 256 points with 10 % and 60 % outliers, max_iters 2000.
Beside them the driver's host least-squares fit on the same points (mtf_amd.sm.least_squares_estimator is the Python one; the C++ one is
inside the frame figures), and mtf::hip::Grid::update() per frame with and without est_params in the video loop of the grid tests
(two synthetic frames alternating, 10 x 10 patches of 10 x 10, forward-backward estimation on and off).  Prints one JSON object.
Reads nothing outside the repository."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import mtf_amd                      # noqa: E402
from mtf_amd import _lib as L       # noqa: E402
from mtf_amd import host, synth     # noqa: E402
from mtf_amd.sm import least_squares_estimator   # noqa: E402
import est_cases as EC              # noqa: E402


def pct(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), p10=float(v[int(0.1 * (len(v) - 1))]), p90=float(v[int(0.9 * (len(v) - 1))]), n=len(v))


def time_est(ctx, ssm, a, b, p, repeats):
    warm = repeats // 10 + 5
    wall, kern, walked = [], [], []
    for k in range(warm + repeats):
        ctx.timing(True)
        ctx.timing_reset()
        t0 = time.perf_counter()
        r = ctx.estimate_warp_from_pts(ssm, a, b, p, seed=k + 1, want_subsets=False)
        t1 = time.perf_counter()
        if k >= warm:
            wall.append((t1 - t0) * 1e6)
            kern.append(ctx.timing_get("est")[0] * 1e3)
            walked.append(r.n_walked)
    ctx.timing(False)
    return dict(wall_us=pct(wall), kernel_us=pct(kern), walked=pct(walked))


def time_host_fit(ssm, a, b, repeats):
    fit = least_squares_estimator(ssm)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    t = []
    for k in range(repeats // 10 + 5 + repeats):
        t0 = time.perf_counter()
        fit(a64, b64)
        t.append((time.perf_counter() - t0) * 1e6)
    return pct(t[repeats // 10 + 5:])


def time_grid(frame_a, frame_b, region, est_params, fb, frames, rounds=5):
    g = host.CppGridTracker(grid_size=10, patch_size=10, patch_sm=L.SM_ICLK, patch_am=L.AM_NCC, patch_ssm=L.SSM_AFFINE, hess_type=0, max_iters=30,
                            epsilon=1e-4, reset_at_each_frame=1, fb_err_thresh=fb, est_params=est_params)
    g.set_image(frame_a)
    g.initialize(region)
    upd = [g.bench_video(frame_a, frame_b, frames)[0] for _ in range(rounds)]
    out = pct(upd)
    if est_params is not None:
        out["est_ok"] = g.est_ok
        out["walked_last"] = g.est_info()["n_walked"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--frames", type=int, default=300)
    args = ap.parse_args()
    ctx = mtf_amd.Context(0)
    out = {}
    a, b, _ = EC.make_points(L.SSM_HOMOGRAPHY, 10, 1, 0.2)
    shipped = L.est_params(L.EST_LMEDS, 5.0, 4, True, 10000, 300, 0.995, 10)
    out["lmeds_100pts_55hyp_refine"] = time_est(ctx, L.SSM_HOMOGRAPHY, a, b, shipped, args.repeats)
    out["host_least_squares_100pts_python"] = time_host_fit(L.SSM_HOMOGRAPHY, a, b, args.repeats)
    ransac = L.est_params(L.EST_RANSAC, 5.0, 4, True, 2000, 300, 0.995, 10)
    for frac in (0.1, 0.6):
        a, b, _ = EC.make_points(L.SSM_HOMOGRAPHY, 16, 2, frac)
        out["ransac_256pts_%d%%_outliers" % int(frac * 100)] = time_est(ctx, L.SSM_HOMOGRAPHY, a, b, ransac, args.repeats)
    ctx.close()
    frame_a = synth.make_frame(512, 512)
    frame_b = synth.warp_frame(frame_a, synth.random_small_homography(np.random.default_rng(2026)) * 0.5, (256.0, 256.0))
    region = synth.square_corners(256.0, 256.0, 280)
    for fb in (0.0, 2.0):
        for name, ep in (("least_squares_stand_in", None), ("device_lmeds_shipped", shipped), ("device_ransac", ransac)):
            out["grid_update_us_fb%g_%s" % (fb, name)] = time_grid(frame_a, frame_b, region, ep, fb, args.frames)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
