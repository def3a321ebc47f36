#!/usr/bin/env python
"""Times Batch.iterate for ESM + LRSCV beside ESM + RSCV, LSCV and SSD (homography, chained) at the same targets in one process and
prints one JSON line of target-iters/s, lean (materialize 0) and materialising (materialize 1):
  lrscv_every  3 x 3 sub-regions, spacing 10, nearest mapping, once_per_frame 0: pass 1 and the blending fused pass every iteration;
  lrscv_first  the shipped configuration (affine_mapping 1, once_per_frame 1) on the first iteration of a frame (the flag set);
  lrscv_later  the shipped configuration on a later iteration (the flag clear: the SSD pass on the raw patch);
  rscv         RSCV, nearest mapping;
  lscv         LSCV, 3 x 3, nearest mapping, a re-map every iteration;
  ssd          SSD.

  python tools/lrscv_bench.py [--targets 64] [--res 200] [--bins 64] [--steps 200] [--warmup 20] [--only lrscv_every,rscv,...]
                              [--materialize 0,1]

Under `rocprofv3 --kernel-trace --stats -- python tools/lrscv_bench.py --only lrscv_every --materialize 0` the per-kernel times of
k_lrscv_hist and the LRSCV fused pass come out."""
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

KINDS = ("lrscv_every", "lrscv_first", "lrscv_later", "rscv", "lscv", "ssd")


def run(kind, mat, a, img, corners):
    ctx = mtf_amd.Context(0)
    ctx.set_image(img)
    am = {"rscv": L.AM_RSCV, "lscv": L.AM_LSCV, "ssd": L.AM_SSD}.get(kind, L.AM_LRSCV)
    b = mtf_amd.Batch(ctx, am, L.SSM_HOMOGRAPHY, a.res, a.res, a.targets, mi_n_bins=a.bins)
    if kind == "rscv":
        b.set_rscv(0, 0, 0)
    elif kind == "lscv":
        b.set_lscv(3, 3, 10, 10, 0, 0, 0)
    elif kind == "lrscv_every":
        b.set_lrscv(3, 3, 10, 10, 0, 0, 0)
    elif am == L.AM_LRSCV:
        b.set_lrscv(3, 3, 10, 10, 1, 1, 0)
    sm = mtf_amd.sm_desc(L.SM_ESM, materialize=mat, leven_marq=0)
    b.set_corners(corners)
    b.init_template(sm)
    rng = np.random.default_rng(1)
    ps = np.stack([synth.random_small_homography(rng, 0.3) for _ in range(a.targets)])
    first = kind == "lrscv_first"

    def step():
        b.set_state(ps)
        b.set_first_iter(first)
        b.iterate(sm)

    for _ in range(a.warmup):
        step()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
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
    ap.add_argument("--materialize", default="0,1")
    a = ap.parse_args()
    img = synth.make_frame(1024, 1024, seed=3)
    rng = np.random.default_rng(0)
    corners = np.stack([synth.square_corners(rng.uniform(200, 824), rng.uniform(200, 824), 150) for _ in range(a.targets)])
    out = dict(targets=a.targets, res=a.res, bins=a.bins, steps=a.steps)
    for mat in (int(m) for m in a.materialize.split(",")):
        sfx = "_mat" if mat else "_lean"
        for kind in a.only.split(","):
            out[kind + sfx + "_target_iters_per_s"] = run(kind, mat, a, img, corners)
        r = lambda k: out.get(k + sfx + "_target_iters_per_s")  # noqa: E731
        if r("rscv") and r("lrscv_every"):
            out["lrscv_every_over_rscv_time" + sfx] = r("rscv") / r("lrscv_every")
        if r("ssd") and r("lrscv_later"):
            out["lrscv_later_over_ssd_time" + sfx] = r("ssd") / r("lrscv_later")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
