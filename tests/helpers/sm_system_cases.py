"""The cases over which a search method's f, g and H are stated once (mtf_amd/csrc/mtfhip_sm_system.h): every (appearance model, search
method, hess_type, jac_type) the fused entry points accept, on every state space model, with and without Levenberg-Marquardt, in both
arithmetic modes -- and the one way a case is run: template on `frame`, a small known start, one `iterate` and one traced `track` on
`frame2`.  tests/test_gpu_sm_system.py runs the 12 x 10 cases."""
import numpy as np

import mtf_amd
from mtf_amd import _lib as L

ESM, FCLK, ICLK, FALK, IALK = L.SM_ESM, L.SM_FCLK, L.SM_ICLK, L.SM_FALK, L.SM_IALK
SSD, NCC, SPSS = L.AM_SSD, L.AM_NCC, L.AM_SPSS
HOM, AFF, SIM, ISO, TRA = L.SSM_HOMOGRAPHY, L.SSM_AFFINE, L.SSM_SIMILITUDE, L.SSM_ISOMETRY, L.SSM_TRANSLATION
AM_NAME = {SSD: "ssd", NCC: "ncc", SPSS: "spss"}
SM_NAME = {ESM: "esm", FCLK: "fclk", ICLK: "iclk", FALK: "falk", IALK: "ialk"}
SSM_NAME = {HOM: "hom", AFF: "aff", SIM: "sim", ISO: "iso", TRA: "tra"}
SMALL, LARGE = (12, 10), (95, 97)     # samples per target: one block row; more than eight block rows (the three-run sum)

# a start a few tenths of a pixel off, in each model's own parameterisation
START = {HOM: [0.004, -0.003, 0.6, 0.002, -0.005, -0.4, 2e-5, -1e-5], AFF: [0.6, -0.4, 0.004, -0.003, 0.002, -0.005],
         SIM: [0.6, -0.4, 0.004, 0.003], ISO: [0.6, -0.4, 0.003], TRA: [0.6, -0.4]}


def sm_variants(am, sm):
    """(hess_type, jac_type) that check_sm and fused_args accept for the first-order fused path (include/mtfhip.h)"""
    if sm in (FALK, IALK):
        return [(h, 1) for h in range(3)]
    out = []
    for h in range(6 if sm == ESM else 3):
        if sm == ICLK and h == 1:                 # fused ICLK with CurrentSelf: the un-fused entry points
            continue
        if am == SPSS and sm == ESM and h == 4:   # SumOfStd needs two weighted Gram matrices in one pass
            continue
        out += [(h, j) for j in ((0, 1) if sm == ESM else (1,))]
    return out


def cases(shapes=(SMALL, LARGE)):
    """dicts am, ssm, sm, hess_type, jac_type, leven_marq, res -- the compositional methods on the five SSMs (SPSS: homography and
    affine; the low-order models serve SSD and NCC), the additive ones on homography and affine with SSD and NCC"""
    out = []
    for res in shapes:
        for am in (SSD, NCC, SPSS):
            for ssm in (HOM, AFF, SIM, ISO, TRA):
                if am == SPSS and ssm not in (HOM, AFF):
                    continue
                for sm in (ESM, FCLK, ICLK, FALK, IALK):
                    if sm in (FALK, IALK) and (am == SPSS or ssm not in (HOM, AFF)):
                        continue
                    for h, j in sm_variants(am, sm):
                        for lm in (0, 1):
                            out.append(dict(am=am, ssm=ssm, sm=sm, hess_type=h, jac_type=j, leven_marq=lm, res=res))
    return out


def case_id(c):
    return "%s-%s-%s-h%d-j%d-lm%d-%dx%d" % (AM_NAME[c["am"]], SSM_NAME[c["ssm"]], SM_NAME[c["sm"]], c["hess_type"], c["jac_type"],
                                             c["leven_marq"], c["res"][0], c["res"][1])


def run(ctx, frame, frame2, c, math_mode, max_iters, with_iterate=True):
    """one case: (f, g, H) of `iterate` (materialize = 1) and, from the same start, n_iters, final corners and the trace of `track`"""
    resx, resy = c["res"]
    ctx.set_image(frame)
    b = mtf_amd.Batch(ctx, c["am"], c["ssm"], resx, resy, 1)
    try:
        b.set_math_mode(math_mode)
        b.set_corners(mtf_amd.synth.square_corners(256, 256, 60)[None])
        kw = dict(hess_type=c["hess_type"], jac_type=c["jac_type"], leven_marq=c["leven_marq"], max_iters=max_iters)
        sm = mtf_amd.sm_desc(c["sm"], materialize=1, **kw)
        b.init_template(sm)
        ctx.set_image(frame2)
        start = np.asarray(START[c["ssm"]], dtype=np.float64)[None]
        out = {}
        if with_iterate:
            b.set_state(start)
            out["f"], out["g"], out["H"] = b.iterate(sm)
        b.set_state(start)
        b.track_trace(max_iters + 2)
        n_it, final = b.track(sm)
        recs = b.read_track_trace(n_it)[0]
        b.track_trace(0)
        out["n_it"], out["final"], out["recs"] = n_it.copy(), np.asarray(final).copy(), recs
        return out
    finally:
        b.close()
