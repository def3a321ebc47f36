#!/usr/bin/env python
"""Times the additive Lucas-Kanade search methods on the device (mtfhip_batch_track with MTFHIP_SM_FALK / _IALK) and writes
profiles/alk_timing.md.

  python tools/alk_time.py [--repeats 200] [--out profiles/alk_timing.md]

Per shape (one 50 x 50 target, one 200 x 200 target, 64 targets of 200 x 200; SSD, homography, max_iters 10, epsilon 0: every pass runs;
nothing materialised), wall clock of one update() per call, median [p10 .. p90] of `repeats` calls, microseconds:
  - FALK and IALK on the device loop (k_alk_pass + k_alk_finish per pass, one read-back per call);
  - the per-function route the library offered for them before: nt::FALK / nt::IALK of the harness over HipAM / HipSSM (one C-ABI call per
    reference virtual, the solve and additiveUpdate on the host) for the single targets, and sm.NTSearchMethod (the same call sequence over
    a batch) for the 64 targets;
  - FCLK and ICLK on their device loop at the same shapes as a yardstick, in replay and in tolerance-mode arithmetic.  FALK and FCLK run
    with the CurrentSelf Hessian (a gradient and a Hessian per pass), IALK and ICLK with InitialSelf.
Reads nothing outside the repository."""
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
from mtf_amd.host import CppTracker     # noqa: E402
from mtf_amd.sm import LKTracker, NTSearchMethod   # noqa: E402

MAX_ITERS = 10
NAMES = {L.SM_FALK: "FALK", L.SM_IALK: "IALK", L.SM_FCLK: "FCLK", L.SM_ICLK: "ICLK"}
HESS = {L.SM_FALK: 1, L.SM_FCLK: 1, L.SM_IALK: 0, L.SM_ICLK: 0}


def pct(v):
    v = np.sort(np.asarray(v))
    return float(np.median(v)), float(v[int(0.1 * (len(v) - 1))]), float(v[int(0.9 * (len(v) - 1))])


def fmt(t):
    return "%.1f [%.1f .. %.1f]" % t if t else "-"


def targets(n, size):
    """n square regions of `size` pixels spread over the 1024 x 1024 frame"""
    side = int(np.ceil(np.sqrt(n)))
    lo, hi = size / 2.0 + 20, 1024 - size / 2.0 - 20
    xs = np.linspace(lo, hi, side) if side > 1 else np.array([512.0])
    return np.stack([synth.square_corners(xs[k % side], xs[k // side], size) for k in range(n)])


def time_calls(reset, call, repeats, sync):
    warm = repeats // 10 + 5
    out = []
    for k in range(warm + repeats):
        reset()
        sync()
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if k >= warm:
            out.append((t1 - t0) * 1e6)
    return pct(out)


def device_loop(ctx, frame, frame2, sm_kind, res, corners, repeats, math=None):
    B = len(corners)
    ctx.set_image(frame)
    t = LKTracker(ctx, sm_kind, ssm=L.SSM_HOMOGRAPHY, resx=res, resy=res, n_targets=B, host_solve=False, am=L.AM_SSD, hess_type=HESS[sm_kind],
                  max_iters=MAX_ITERS, epsilon=0.0, leven_marq=0, materialize=0)
    try:
        if math is not None:
            t.batch.set_math_mode(math)
        t.initialize(corners)
        ctx.set_image(frame2)
        zero = np.zeros((B, t.S))
        return time_calls(lambda: t.batch.set_state(zero), t.update, repeats, ctx.synchronize)
    finally:
        t.batch.close()


def per_function_single(frame, frame2, sm_kind, res, corners, repeats):
    t = CppTracker(sm_kind, am=L.AM_SSD, ssm=L.SSM_HOMOGRAPHY, resx=res, resy=res, hess_type=HESS[sm_kind], max_iters=MAX_ITERS, epsilon=0.0, leven_marq=0)
    t.set_image(frame)
    t.initialize(corners[0])
    t.set_image(frame2)
    return time_calls(lambda: t.set_region(corners[0]), t.update, repeats, lambda: None)


def per_function_batch(ctx, frame, frame2, sm_kind, res, corners, repeats):
    B = len(corners)
    ctx.set_image(frame)
    t = NTSearchMethod(ctx, sm_kind, am=L.AM_SSD, ssm=L.SSM_HOMOGRAPHY, resx=res, resy=res, n_targets=B, hess_type=HESS[sm_kind], max_iters=MAX_ITERS,
                       epsilon=0.0, leven_marq=0)
    try:
        t.initialize(corners)
        ctx.set_image(frame2)
        zero = np.zeros((B, t.S))
        return time_calls(lambda: t.batch.set_state(zero), t.update, max(10, repeats // 10), ctx.synchronize)
    finally:
        t.batch.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alk_timing.md"))
    args = ap.parse_args()
    ctx = mtf_amd.Context(0)
    frame = synth.make_frame(1024, 1024)
    frame2 = synth.warp_frame(frame, synth.random_small_homography(np.random.default_rng(2026)) * 0.25, (512.0, 512.0))
    shapes = [("1 x 50 x 50", 1, 50, 100.0), ("1 x 200 x 200", 1, 200, 200.0), ("64 x 200 x 200", 64, 200, 100.0)]
    lines = ["# nt::FALK / nt::IALK on the device: timing of update()", "",
             "Written by `tools/alk_time.py --repeats %d` on one MI355X.  Microseconds per update() call by wall clock, median [p10 .. p90]; SSD," % args.repeats,
             "homography, max_iters %d, epsilon 0 (every pass runs), nothing materialised; the state is reset in front of every call." % MAX_ITERS,
             "Device loop: mtfhip_batch_track.  Per-function route: nt::FALK / nt::IALK of the harness over HipAM / HipSSM for one target,",
             "sm.NTSearchMethod (the same call sequence, batched; a tenth of the repeats) for 64.  FALK and FCLK with the CurrentSelf Hessian,",
             "IALK and ICLK with InitialSelf; FCLK / ICLK in replay and in tolerance-mode arithmetic (FALK / IALK have the replay form only).", "",
             "| shape | method | device loop | per pass | per-function route | FCLK / ICLK replay | FCLK / ICLK tolerance mode | per pass / yardstick (replay) |",
             "|---|---|---|---|---|---|---|---|"]
    for label, B, res, size in shapes:
        corners = targets(B, size)
        for sm_kind, yard in ((L.SM_FALK, L.SM_FCLK), (L.SM_IALK, L.SM_ICLK)):
            dev = device_loop(ctx, frame, frame2, sm_kind, res, corners, args.repeats)
            base = per_function_single(frame, frame2, sm_kind, res, corners, args.repeats) if B == 1 else \
                per_function_batch(ctx, frame, frame2, sm_kind, res, corners, args.repeats)
            y_rep = device_loop(ctx, frame, frame2, yard, res, corners, args.repeats, math=mtf_amd.MATH_REPLAY)
            y_fast = device_loop(ctx, frame, frame2, yard, res, corners, args.repeats, math=mtf_amd.MATH_FAST)
            line = "| %s | %s | %s | %.1f | %s | %s %s | %s | %.2f |" % (label, NAMES[sm_kind], fmt(dev), dev[0] / MAX_ITERS, fmt(base), NAMES[yard], fmt(y_rep), fmt(y_fast),
                                                                      dev[0] / y_rep[0])
            print(line, flush=True)
            lines.append(line)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
