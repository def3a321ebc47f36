#!/usr/bin/env python
"""Times the device loop (mtfhip_batch_track) of ESM + CCRE against ESM + MI on MI's materialising form and writes profiles/ccre_timing.md.

  python tools/ccre_time.py [--repeats 20] [--out profiles/ccre_timing.md]

A CCRE iteration is MI's materialising iteration (mi_enqueue, api_mi_iter.hip) with other weights, tables and Hessian formulas: the fused
SSD pass for It, dIt_dx and Jt, the histogram pass, the tables, the gradient pass with its Jacobian products, the Hessian pass.  It moves the
same bytes per pixel as that form, so that is the comparison: the tool switches MI's recompute form off for the process
(MTFHIP_MI_RECOMPUTE=0).  Shapes: 64 targets of 100 x 100 and of 400 x 400, 8 bins, homography; ESM with its class-default SumOfSelf
Hessian (cmptSelfHessian per pass: for CCRE two more histogram launches, cmptCumSelfHist) and with Std (cmptCurrHessian), and SumOfStd (two
Hessian passes, the init kind among them); a fixed pass count (max_iters 10, epsilon 0: every pass runs).  MI and CCRE alternate in one
process: one round times each once, `repeats` rounds; microseconds per pass by wall clock around the call (it returns with the results on
the host), median [p10 .. p90], and the ratio of the medians.  Reads nothing outside the repository."""
import argparse
import os
import sys
import time

import numpy as np

os.environ["MTFHIP_MI_RECOMPUTE"] = "0"      # (read once per process, before the library's first MI iteration)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mtf_amd                          # noqa: E402
from mtf_amd import _lib as L           # noqa: E402
from mtf_amd import synth               # noqa: E402
from mtf_amd.sm import LKTracker        # noqa: E402

MAX_ITERS = 10
N_BINS = 8
AMS = [(L.AM_MI, "MI (materialising)"), (L.AM_CCRE, "CCRE")]
ROWS = [("ESM SumOfSelf", 2), ("ESM Std", 5), ("ESM SumOfStd", 4)]


def pct(v):
    v = np.sort(np.asarray(v))
    return float(np.median(v)), float(v[int(0.1 * (len(v) - 1))]), float(v[int(0.9 * (len(v) - 1))])


def targets(n, size):
    """n square regions of `size` pixels spread over the 1024 x 1024 frame"""
    side = int(np.ceil(np.sqrt(n)))
    lo, hi = size / 2.0 + 20, 1024 - size / 2.0 - 20
    xs = np.linspace(lo, hi, side) if side > 1 else np.array([512.0])
    return np.stack([synth.square_corners(xs[k % side], xs[k // side], size) for k in range(n)])


def measure(ctx, frame, frame2, hess_type, res, corners, repeats):
    B = len(corners)
    ctx.set_image(frame)
    trackers = []
    try:
        for am, _ in AMS:
            t = LKTracker(ctx, L.SM_ESM, ssm=L.SSM_HOMOGRAPHY, resx=res, resy=res, n_targets=B, host_solve=False, am=am,
                          am_params=dict(mi_n_bins=N_BINS), hess_type=hess_type, max_iters=MAX_ITERS, epsilon=0.0, leven_marq=0, materialize=1)
            t.batch.set_math_mode(mtf_amd.MATH_REPLAY)
            t.initialize(corners)
            trackers.append(t)
        ctx.set_image(frame2)
        zeros = np.zeros((B, 8))
        times = [[] for _ in trackers]
        warm = repeats // 10 + 3
        for k in range(warm + repeats):
            for i, t in enumerate(trackers):          # MI and CCRE alternate
                t.batch.set_state(zeros)
                ctx.synchronize()
                t0 = time.perf_counter()
                t.update()
                t1 = time.perf_counter()
                assert int(np.asarray(t.n_iters).min()) == MAX_ITERS
                if k >= warm:
                    times[i].append((t1 - t0) * 1e6 / MAX_ITERS)
        return [pct(v) for v in times]
    finally:
        for t in trackers:
            t.batch.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ccre_timing.md"))
    args = ap.parse_args()
    ctx = mtf_amd.Context(0)
    frame = synth.make_frame(1024, 1024)
    frame2 = synth.warp_frame(frame, np.array([0.0, 0.0, 0.8, 0.0, 0.0, -0.6, 0.0, 0.0]), (512.0, 512.0))
    shapes = [("64 x 100 x 100", 64, 100, 100.0), ("64 x 400 x 400", 64, 400, 400.0)]
    lines = ["# CCRE on the device loop: time per pass against MI's materialising form", "",
             "Written by `tools/ccre_time.py --repeats %d` on one MI355X.  Microseconds per pass (wall clock of one mtfhip_batch_track call / %d"
             % (args.repeats, MAX_ITERS),
             "passes; max_iters %d, epsilon 0: every pass runs), median [p10 .. p90] of the calls; ESM, homography, %d bins, materialising," % (MAX_ITERS, N_BINS),
             "replay arithmetic; MI and CCRE alternate call by call in one process, the state is reset in front of every call.  MI runs its",
             "materialising form (MTFHIP_MI_RECOMPUTE=0), whose passes CCRE's are.  `x` = ratio of the medians to MI's.", "",
             "| shape | Hessian | " + " | ".join(n for _, n in AMS) + " |", "|---|---|" + "---|" * len(AMS)]
    for label, n, res, size in shapes:
        corners = targets(n, size)
        for name, ht in ROWS:
            r = measure(ctx, frame, frame2, ht, res, corners, args.repeats)
            cells = ["%.1f [%.1f .. %.1f]%s" % (m[0], m[1], m[2], "" if i == 0 else " x%.2f" % (m[0] / r[0][0])) for i, m in enumerate(r)]
            row = "| %s | %s | %s |" % (label, name, " | ".join(cells))
            print(row, flush=True)
            lines.append(row)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
