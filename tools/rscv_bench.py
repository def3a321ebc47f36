#!/usr/bin/env python
"""Times Batch.iterate for ESM + RSCV beside ESM + SSD and ESM + SCV (homography, chained; lean by default, --materialize 1 for the
materialising pass) at the same targets in one process and prints one JSON line: target-iters/s of each, the ratios, and RSCV's
algorithmic bytes per pixel on top of SSD's pass.

  python tools/rscv_bench.py [--targets 64] [--res 200] [--bins 64] [--linear 0] [--steps 200] [--warmup 20] [--only rscv|ssd|scv]
                             [--materialize 0|1]

Under `rocprofv3 --kernel-trace --stats -- python tools/rscv_bench.py --only rscv` the per-kernel times of RSCV's pass 1 (k_rscv_hist,
which also builds the map in its last-arriving workgroup per target) come out beside its fused pass (k_fused_rscv / k_fused_rscv_fast)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mtf_amd  # noqa: E402
from mtf_amd import _lib as L  # noqa: E402
from mtf_amd import synth  # noqa: E402


def rscv_bytes_per_px():
    """what RSCV adds per pixel and iteration, by construction (kernels_rscv.hip): pass 1 reads the grid point (16 B), four float texels
    (16 B; neighbouring pixels share most of them) and the template's code plane (1 B).  The fused pass reads and writes what SSD's does
    (the map sits in LDS); the map itself is n_bins-sized rows."""
    return 16 + 16 + 1


def run(am, a, img, corners):
    ctx = mtf_amd.Context(0)
    ctx.set_image(img)
    b = mtf_amd.Batch(ctx, am, L.SSM_HOMOGRAPHY, a.res, a.res, a.targets, mi_n_bins=a.bins)
    if am == L.AM_RSCV:
        b.set_rscv(0, a.linear, 0)
    sm = mtf_amd.sm_desc(L.SM_ESM, materialize=a.materialize, leven_marq=0)
    b.set_corners(corners)
    b.init_template(sm)
    rng = np.random.default_rng(1)
    ps = np.stack([synth.random_small_homography(rng, 0.3) for _ in range(a.targets)])
    for _ in range(a.warmup):
        b.set_state(ps)
        b.iterate(sm)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        b.set_state(ps)
        b.iterate(sm)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    b.close()
    ctx.close()
    return a.targets * a.steps / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=64)
    ap.add_argument("--res", type=int, default=200)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--linear", type=int, default=0, help="RSCVParams::weighted_mapping")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=["rscv", "ssd", "scv"], default=None)
    ap.add_argument("--materialize", type=int, default=0, help="1: the materialising fused pass (It, dIt_dx, Jt written)")
    a = ap.parse_args()
    img = synth.make_frame(1024, 1024, seed=3)
    rng = np.random.default_rng(0)
    corners = np.stack([synth.square_corners(rng.uniform(200, 824), rng.uniform(200, 824), 150) for _ in range(a.targets)])
    out = dict(materialize=a.materialize, targets=a.targets, res=a.res, bins=a.bins, linear=a.linear, steps=a.steps,
               rscv_bytes_per_px=rscv_bytes_per_px())
    for key, am in (("rscv", L.AM_RSCV), ("ssd", L.AM_SSD), ("scv", L.AM_SCV)):
        if a.only in (None, key):
            out[key + "_target_iters_per_s"] = run(am, a, img, corners)
    if a.only is None:
        out["rscv_over_ssd_time"] = out["ssd_target_iters_per_s"] / out["rscv_target_iters_per_s"]
        out["rscv_over_scv_time"] = out["scv_target_iters_per_s"] / out["rscv_target_iters_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
