#!/usr/bin/env python
"""Times Batch.iterate for ESM + SCV and ESM + SSD (homography, chained; lean by default, --materialize 1 for the
materialising pass) at the same targets in one process and
prints one JSON line: target-iters/s of each, the ratio, and SCV's algorithmic bytes per pixel beside SSD's.

  python tools/scv_bench.py [--targets 64] [--res 200] [--bins 64] [--hist 0] [--steps 200] [--warmup 20] [--only scv|ssd] [--materialize 0|1]

Under `rocprofv3 --kernel-trace --stats -- python tools/scv_bench.py --only scv` the per-kernel times of the SCV passes (k_scv_hist,
k_scv_map, k_scv_remap) come out beside the fused SSD pass (k_fused_ssd / k_fused_lean)."""
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


def scv_bytes_per_px(hist):
    """what the SCV passes move per pixel and iteration, by construction (kernels_scv.hip): pass 1 reads the grid point (16 B), four
    float texels (16 B; neighbouring pixels share most of them) and the template's code plane (2 B, Dirac) or I0_orig (8 B, Bilinear);
    the re-map reads the code plane (2 B, nearest) and writes I0 (8 B).  The map kernel moves n_bins-sized rows only."""
    return 16 + 16 + (2 if hist == 0 else 8) + 2 + 8


def run(am, a, img, corners):
    ctx = mtf_amd.Context(0)
    ctx.set_image(img)
    b = mtf_amd.Batch(ctx, am, L.SSM_HOMOGRAPHY, a.res, a.res, a.targets, mi_n_bins=a.bins)
    if am == L.AM_SCV:
        b.set_scv(a.hist, 0, 0)
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
    ap.add_argument("--hist", type=int, default=0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=["scv", "ssd"], default=None)
    ap.add_argument("--materialize", type=int, default=0, help="1: the materialising fused pass (It, dIt_dx, Jt written)")
    a = ap.parse_args()
    img = synth.make_frame(1024, 1024, seed=3)
    rng = np.random.default_rng(0)
    corners = np.stack([synth.square_corners(rng.uniform(200, 824), rng.uniform(200, 824), 150) for _ in range(a.targets)])
    out = dict(materialize=a.materialize, targets=a.targets, res=a.res, bins=a.bins, hist=a.hist, steps=a.steps, scv_bytes_per_px=scv_bytes_per_px(a.hist))
    if a.only != "ssd":
        out["scv_target_iters_per_s"] = run(L.AM_SCV, a, img, corners)
    if a.only != "scv":
        out["ssd_target_iters_per_s"] = run(L.AM_SSD, a, img, corners)
    if a.only is None:
        out["scv_over_ssd_time"] = out["ssd_target_iters_per_s"] / out["scv_target_iters_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
