#!/usr/bin/env python
"""Times the device loop (mtfhip_batch_track) of the SSIM appearance model against NCC and writes profiles/ssim_timing.md.

  python tools/ssim_time.py [--repeats 40] [--out profiles/ssim_timing.md]

An SSIM pass IS an NCC pass -- the same kernels, the same 72 raw moments per target -- and what differs is the finish that reads the reduced
row: k_finish_track_ssim evaluates SSIM.cc's gradients and its unsymmetric Hessians from the moments (mtfhip_sm_system.h) where
k_finish_track evaluates NCC's.  NCC on its two-launch loop is the yardstick: the tool switches NCC's other routes off for the process
(MTFHIP_ICLK_ONE_LAUNCH_MAX=0: no one-launch ICLK kernel; MTFHIP_TRACK_DEFER_MAT=0: a materialising loop stores in every pass, as SSIM's
does), so the two columns run the same launches but for the finish.  Shapes: 64 targets of 200 x 200 and 256 targets of 25 x 25;
homography; ESM, FCLK and ICLK, lean (tolerance arithmetic, nothing materialised) and materialising (replay arithmetic); a fixed pass count
(max_iters 10, epsilon 0: every pass runs).  NCC and SSIM alternate in one process: one round times each once, `repeats` rounds;
microseconds per pass by wall clock around the call (the call returns with the results on the host), median [p10 .. p90], and the ratio of
the medians.  Reads nothing outside the repository."""
import argparse
import os
import sys
import time

import numpy as np

os.environ["MTFHIP_ICLK_ONE_LAUNCH_MAX"] = "0"      # (read once per process, before the library's first loop)
os.environ["MTFHIP_TRACK_DEFER_MAT"] = "0"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mtf_amd                          # noqa: E402
from mtf_amd import _lib as L           # noqa: E402
from mtf_amd import synth               # noqa: E402
from mtf_amd.sm import LKTracker        # noqa: E402

MAX_ITERS = 10
AMS = [(L.AM_NCC, "NCC"), (L.AM_SSIM, "SSIM")]
# (label, search method, hess_type, materialize, math mode): the class-default Hessians SumOfSelf, CurrentSelf, InitialSelf
ROWS = [("%s %s" % (name, "materialising" if mat else "lean"), sm, ht, mat, mtf_amd.MATH_REPLAY if mat else mtf_amd.MATH_FAST)
        for name, sm, ht in (("ESM", L.SM_ESM, 2), ("FCLK", L.SM_FCLK, 1), ("ICLK", L.SM_ICLK, 0)) for mat in (0, 1)]


def pct(v):
    v = np.sort(np.asarray(v))
    return float(np.median(v)), float(v[int(0.1 * (len(v) - 1))]), float(v[int(0.9 * (len(v) - 1))])


def targets(n, size):
    """n square regions of `size` pixels spread over the 1024 x 1024 frame"""
    side = int(np.ceil(np.sqrt(n)))
    lo, hi = size / 2.0 + 20, 1024 - size / 2.0 - 20
    xs = np.linspace(lo, hi, side) if side > 1 else np.array([512.0])
    return np.stack([synth.square_corners(xs[k % side], xs[k // side], size) for k in range(n)])


def measure(ctx, frame, frame2, sm_kind, hess_type, mat, math, res, corners, repeats):
    B = len(corners)
    ctx.set_image(frame)
    trackers = []
    try:
        for am, _ in AMS:
            t = LKTracker(ctx, sm_kind, ssm=L.SSM_HOMOGRAPHY, resx=res, resy=res, n_targets=B, host_solve=False, am=am, hess_type=hess_type,
                          max_iters=MAX_ITERS, epsilon=0.0, leven_marq=0, materialize=mat)
            t.batch.set_math_mode(math)
            t.initialize(corners)
            trackers.append(t)
        ctx.set_image(frame2)
        zeros = np.zeros((B, 8))
        times = [[] for _ in trackers]
        warm = repeats // 10 + 5
        for k in range(warm + repeats):
            for i, t in enumerate(trackers):          # NCC and SSIM alternate
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
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_timing.md"))
    args = ap.parse_args()
    ctx = mtf_amd.Context(0)
    frame = synth.make_frame(1024, 1024)
    frame2 = synth.warp_frame(frame, np.array([0.0, 0.0, 0.8, 0.0, 0.0, -0.6, 0.0, 0.0]), (512.0, 512.0))
    shapes = [("64 x 200 x 200", 64, 200, 100.0), ("256 x 25 x 25", 256, 25, 30.0)]
    lines = ["# SSIM on the device loop: time per pass against NCC", "",
             "Written by `tools/ssim_time.py --repeats %d` on one MI355X.  Microseconds per pass (wall clock of one mtfhip_batch_track call / %d"
             % (args.repeats, MAX_ITERS),
             "passes; max_iters %d, epsilon 0: every pass runs), median [p10 .. p90] of the calls; homography; NCC and SSIM alternate call by" % MAX_ITERS,
             "call in one process, the state is reset in front of every call.  `x` = ratio of the medians to NCC's.  Lean rows: tolerance",
             "arithmetic, nothing materialised; materialising rows: replay arithmetic, stores in every pass.  Both columns run NCC's pass",
             "kernels on the two-launch loop (NCC's one-launch ICLK kernel and its deferred materialisation are switched off for the",
             "process): the difference is the finish, k_finish_track_ssim against k_finish_track.", "",
             "| shape | loop | " + " | ".join(n for _, n in AMS) + " |", "|---|---|" + "---|" * len(AMS)]
    for label, n, res, size in shapes:
        corners = targets(n, size)
        for name, sm_kind, ht, mat, math in ROWS:
            r = measure(ctx, frame, frame2, sm_kind, ht, mat, math, res, corners, args.repeats)
            cells = ["%.1f [%.1f .. %.1f]%s" % (m[0], m[1], m[2], "" if i == 0 else " x%.2f" % (m[0] / r[0][0])) for i, m in enumerate(r)]
            row = "| %s | %s | %s |" % (label, name, " | ".join(cells))
            print(row, flush=True)
            lines.append(row)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
