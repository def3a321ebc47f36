#!/usr/bin/env python
"""Times Batch.iterate for ESM + LSCV beside ESM + SCV and ESM + SSD (homography, chained, lean) at the same targets in one process and
prints one JSON line of target-iters/s:
  lscv_every   3 x 3 sub-regions, spacing 10, nearest mapping, once_per_frame 0: a re-map in front of every iteration;
  lscv_first   the shipped configuration (affine_mapping 1, once_per_frame 1) on the first iteration of a frame (the flag set);
  lscv_later   the shipped configuration on a later iteration (the flag clear: no re-map, the SSD pass on the re-mapped template);
  scv, ssd     SCV Dirac + nearest, and SSD.

  python tools/lscv_bench.py [--targets 64] [--res 200] [--bins 64] [--steps 200] [--warmup 20] [--only lscv_every,scv,...]

Under `rocprofv3 --kernel-trace --stats -- python tools/lscv_bench.py --only lscv_every` the per-kernel times of the LSCV passes
(k_lscv_hist, k_lscv_remap) come out beside the fused SSD pass."""
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

KINDS = ("lscv_every", "lscv_first", "lscv_later", "scv", "ssd")


def run(kind, a, img, corners):
    ctx = mtf_amd.Context(0)
    ctx.set_image(img)
    am = {"scv": L.AM_SCV, "ssd": L.AM_SSD}.get(kind, L.AM_LSCV)
    b = mtf_amd.Batch(ctx, am, L.SSM_HOMOGRAPHY, a.res, a.res, a.targets, mi_n_bins=a.bins)
    if kind == "scv":
        b.set_scv(0, 0, 0)
    elif kind == "lscv_every":
        b.set_lscv(3, 3, 10, 10, 0, 0, 0)
    elif am == L.AM_LSCV:
        b.set_lscv(3, 3, 10, 10, 1, 1, 0)
    sm = mtf_amd.sm_desc(L.SM_ESM, materialize=0, leven_marq=0)
    b.set_corners(corners)
    b.init_template(sm)
    b.set_first_iter(kind == "lscv_first")
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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default=",".join(KINDS))
    a = ap.parse_args()
    img = synth.make_frame(1024, 1024, seed=3)
    rng = np.random.default_rng(0)
    corners = np.stack([synth.square_corners(rng.uniform(200, 824), rng.uniform(200, 824), 150) for _ in range(a.targets)])
    out = dict(targets=a.targets, res=a.res, bins=a.bins, steps=a.steps)
    for kind in a.only.split(","):
        out[kind + "_target_iters_per_s"] = run(kind, a, img, corners)
    if "scv_target_iters_per_s" in out and "lscv_every_target_iters_per_s" in out:
        out["lscv_every_over_scv_time"] = out["scv_target_iters_per_s"] / out["lscv_every_target_iters_per_s"]
    if "ssd_target_iters_per_s" in out and "lscv_first_target_iters_per_s" in out:
        out["lscv_first_minus_ssd_us_per_iter"] = 1e6 * a.targets * (1 / out["lscv_first_target_iters_per_s"] - 1 / out["ssd_target_iters_per_s"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
