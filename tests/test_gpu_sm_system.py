"""GPU: `iterate` followed by a host solve and the device loop are the same method -- both read a search method's f, g and H from
mtf_amd/csrc/mtfhip_sm_system.h.  For every case of tests/helpers/sm_system_cases.py on one target of 12 x 10 samples (SSD, NCC and SPSS;
ESM, FCLK, ICLK with every hess_type / jac_type the fused path accepts, FALK and IALK; the five state space models; Levenberg-Marquardt off
and on), pass 0 of the device loop's trace is compared with `iterate`'s (f, g, H) from the same start, materialize = 1: in replay
arithmetic, and in fast arithmetic where the loop ends its pass with finish_track_fast_body (first-order SSD on homography and affine).

The two paths may reduce different block rows, and in fast arithmetic the loop's pixel pass is the tolerance-mode one while a
materialising `iterate` replays the reference, so the bound is measured, not derived: the worst difference over the cases on the commit
before the header existed (H relative in the Frobenius norm; g scaled as tests/test_gpu_edges.py scales it, by
max(|g|, sqrt(|tr H| |2 f|)); f relative), and four times that is allowed.  Measured on that commit: MEASURED below."""
import os
import sys

import numpy as np
import pytest

import mtf_amd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sm_system_cases as K   # noqa: E402

pytestmark = pytest.mark.gpu

# worst differences on the parent commit (this test passes there unmodified) and the bounds, 4 x
# (H and g came out bit for bit equal in all 448 + 68 cases, so they are held to equality; f differs in the one-launch loop of
# first-order ICLK, which sums its similarity in another order: worst cases ncc-hom-iclk-h0 and ssd-aff-iclk-h0)
MEASURED = {"replay": dict(H=0.0, g=0.0, f=1.0693244247010412e-14), "fast": dict(H=0.0, g=0.0, f=8.75346793253323e-15)}
BOUND = {m: {k: 4 * v for k, v in d.items()} for m, d in MEASURED.items()}
# ... and for the 95 x 97 target, where `iterate` and the loop sum their block rows in different runs (worst: ncc-hom-esm-h2, ssd-hom-esm-h2)
MEASURED_LARGE = {"replay": dict(H=3.2044718343769555e-19, g=2.787674954940518e-17, f=1.7341444076392524e-16),
                  "fast": dict(H=3.7326636775833906e-22, g=3.6227343876066e-19, f=1.7341444076392524e-16)}
BOUND_LARGE = {m: {k: 4 * v for k, v in d.items()} for m, d in MEASURED_LARGE.items()}


def fast_body_runs(c):
    return c["am"] == K.SSD and c["ssm"] in (K.HOM, K.AFF) and c["sm"] in (K.ESM, K.FCLK, K.ICLK)


def differences(ctx, frame, frame2, mode, shapes=(K.SMALL,), pick=lambda c: True):
    """worst (difference, case) per quantity, and how many cases recorded H in their trace"""
    worst, with_H, n = dict(H=(0.0, ""), g=(0.0, ""), f=(0.0, "")), 0, 0
    for c in K.cases(shapes=shapes):
        if (mode == "fast" and not fast_body_runs(c)) or not pick(c):
            continue
        r = K.run(ctx, frame, frame2, c, mtf_amd.MATH_FAST if mode == "fast" else mtf_amd.MATH_REPLAY, 1)
        cid = K.case_id(c)
        assert int(r["n_it"][0]) == 1 and len(r["recs"]) == 1, cid
        rec, f, g, H = r["recs"][0], r["f"][0], r["g"][0], r["H"][0]
        assert not rec["undo"], cid
        n += 1
        d = dict(f=abs(rec["f"] - f) / abs(f))
        if rec["has_H"]:   # (the one-launch loop of first-order ICLK works from the constant template Hessian and may record none)
            with_H += 1
            d["H"] = np.linalg.norm(rec["H"] - H) / np.linalg.norm(H)
            d["g"] = np.linalg.norm(rec["g"] - g) / max(np.linalg.norm(g), np.sqrt(abs(np.trace(H)) * abs(2 * f)))
        for k, v in d.items():
            assert np.isfinite(v), (cid, k)
            if v > worst[k][0]:
                worst[k] = (float(v), cid)
    return worst, with_H, n


@pytest.mark.parametrize("mode", ["replay", "fast"])
def test_pass_0_of_the_device_loop_is_iterate(gpu_ctx, frame, frame2, mode):
    worst, with_H, n = differences(gpu_ctx, frame, frame2, mode)
    print("%s: %d cases, %d with H in the trace; worst %s" % (mode, n, with_H, worst), file=sys.stderr)
    # (on the parent commit the same counts: the six and four cases without H are the one-launch loop of first-order ICLK)
    assert (n, with_H) == ((448, 442) if mode == "replay" else (68, 64))
    for k, (v, cid) in worst.items():
        assert v <= BOUND[mode][k], (mode, k, v, cid, BOUND[mode][k])


def test_three_run_row_sum_target(gpu_ctx, frame, frame2):
    """one target of 95 x 97 samples has more than eight block rows, so both finish bodies take the three-run sum (fin_sum_runs /
    fin_sum_combine): ESM with its default Hessian on the homography, SSD in both arithmetic modes and NCC, within BOUND_LARGE"""
    for mode, ams in (("replay", (K.SSD, K.NCC)), ("fast", (K.SSD,))):
        def pick(c):
            return c["am"] in ams and c["ssm"] == K.HOM and c["sm"] == K.ESM and (c["hess_type"], c["jac_type"], c["leven_marq"]) == (2, 1, 0)
        worst, with_H, n = differences(gpu_ctx, frame, frame2, mode, shapes=(K.LARGE,), pick=pick)
        print("95 x 97 %s: %d cases; worst %s" % (mode, n, worst), file=sys.stderr)
        assert (n, with_H) == (len(ams), len(ams))
        for k, (v, cid) in worst.items():
            assert v <= BOUND_LARGE[mode][k], (mode, k, v, cid, BOUND_LARGE[mode][k])
