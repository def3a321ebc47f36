#!/usr/bin/env python
"""Times the device loop (mtfhip_batch_track) of the Similitude, Isometry and Translation state space models against the Affine one and
writes profiles/lowdof_timing.md.

  python tools/lowdof_time.py [--repeats 100] [--out profiles/lowdof_timing.md]

The low-order models run the affine pixel pass and project its system in the finish, so they are expected at Affine's pass time (plus, on
a materialising call, the launch that writes the model's N x S Jacobian behind the loop).  Shapes: 64 targets of 200 x 200 and 256 targets
of 25 x 25; SSD; ESM and ICLK; a fixed pass count (max_iters 10, epsilon 0: every pass runs), nothing materialised, and ESM once more
with materialize = 1.  Affine and each model alternate in one process: one round times every model once, `repeats` rounds; microseconds
per pass by wall clock around the call (the call returns with the results on the host), median [p10 .. p90], and the ratio of the medians
to Affine's.  Reads nothing outside the repository."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mtf_amd                          # noqa: E402
from mtf_amd import _lib as L           # noqa: E402
from mtf_amd import synth               # noqa: E402
from mtf_amd.sm import LKTracker        # noqa: E402

MAX_ITERS = 10
SSMS = [(L.SSM_AFFINE, "Affine"), (L.SSM_SIMILITUDE, "Similitude"), (L.SSM_ISOMETRY, "Isometry"), (L.SSM_TRANSLATION, "Translation")]
METHODS = [(L.SM_ESM, "ESM", 2), (L.SM_ICLK, "ICLK", 0)]   # with their class-default Hessians: SumOfSelf, InitialSelf


def pct(v):
    v = np.sort(np.asarray(v))
    return float(np.median(v)), float(v[int(0.1 * (len(v) - 1))]), float(v[int(0.9 * (len(v) - 1))])


def targets(n, size):
    """n square regions of `size` pixels spread over the 1024 x 1024 frame"""
    side = int(np.ceil(np.sqrt(n)))
    lo, hi = size / 2.0 + 20, 1024 - size / 2.0 - 20
    xs = np.linspace(lo, hi, side) if side > 1 else np.array([512.0])
    return np.stack([synth.square_corners(xs[k % side], xs[k // side], size) for k in range(n)])


def measure(ctx, frame, frame2, sm_kind, hess_type, res, corners, repeats, materialize):
    B = len(corners)
    ctx.set_image(frame)
    trackers = []
    try:
        for ssm, _ in SSMS:
            t = LKTracker(ctx, sm_kind, ssm=ssm, resx=res, resy=res, n_targets=B, host_solve=False, am=L.AM_SSD, hess_type=hess_type,
                          max_iters=MAX_ITERS, epsilon=0.0, leven_marq=0, materialize=materialize)
            t.initialize(corners)
            trackers.append(t)
        ctx.set_image(frame2)
        zeros = [np.zeros((B, t.S)) for t in trackers]
        times = [[] for _ in trackers]
        warm = repeats // 10 + 5
        for k in range(warm + repeats):
            for i, t in enumerate(trackers):          # Affine and the three models alternate
                t.batch.set_state(zeros[i])
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
    ap.add_argument("--repeats", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowdof_timing.md"))
    args = ap.parse_args()
    ctx = mtf_amd.Context(0)
    frame = synth.make_frame(1024, 1024)
    frame2 = synth.warp_frame(frame, np.array([0.0, 0.0, 0.8, 0.0, 0.0, -0.6, 0.0, 0.0]), (512.0, 512.0))
    shapes = [("64 x 200 x 200", 64, 200, 100.0), ("256 x 25 x 25", 256, 25, 30.0)]
    lines = ["# Similitude / Isometry / Translation on the device loop: time per pass against Affine", "",
             "Written by `tools/lowdof_time.py --repeats %d` on one MI355X.  Microseconds per pass (wall clock of one mtfhip_batch_track call / %d"
             % (args.repeats, MAX_ITERS),
             "passes; max_iters %d, epsilon 0: every pass runs), median [p10 .. p90] of the calls; SSD; the four models alternate call by call" % MAX_ITERS,
             "in one process, the state is reset in front of every call.  `x` = ratio of the medians to Affine's.  `mat`: materialize = 1 (the",
             "low-order models then run one more launch per call, the N x S Jacobian behind the loop).", "",
             "| shape | method | " + " | ".join(n for _, n in SSMS) + " |", "|---|---|" + "---|" * len(SSMS)]
    for label, n, res, size in shapes:
        corners = targets(n, size)
        for sm_kind, name, ht in METHODS:
            for mat in ((0, 1) if sm_kind == L.SM_ESM else (0,)):
                r = measure(ctx, frame, frame2, sm_kind, ht, res, corners, args.repeats, mat)
                cells = ["%.1f [%.1f .. %.1f]%s" % (m[0], m[1], m[2], "" if i == 0 else " x%.2f" % (m[0] / r[0][0])) for i, m in enumerate(r)]
                row = "| %s | %s%s | %s |" % (label, name, " mat" if mat else "", " | ".join(cells))
                print(row, flush=True)
                lines.append(row)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
