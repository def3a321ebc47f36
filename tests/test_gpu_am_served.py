"""Every refusal that depends on the appearance model and the place alone, at the C ABI itself: for each (model, place) pair the literal
table of tests/helpers/am_served_table.py marks refused, the cheapest call that reaches the site returns MTFHIP_ERR_NOT_IMPLEMENTED (-2) and
leaves exactly the table's bytes in mtfhip_last_error().  The table was typed from the sources before mtfhip_am_served.h replaced the five
refusal helpers, and this file passed unchanged on that commit: it pins that behaviour, not the header's.  SSD, which every place serves,
runs the same calls as a check of the served side: none of them returns -2.

One 10 x 10 single-target homography batch per model, 8 bins where the model reads bins; a refusal comes before any state is looked at, so
only SSD needs a template."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import am_served_table as T   # noqa: E402

pytestmark = pytest.mark.gpu
CORNERS = synth.square_corners(256, 256, 40)


def new_batch(ctx, am, **kw):
    return mtf_amd.Batch(ctx, am, L.SSM_HOMOGRAPHY, 10, 10, 1, mi_n_bins=8, **kw)


def pf_create(b):
    desc, h = C.create_string_buffer(4096), C.c_void_p()
    rc = L.lib().mtfhip_pf_create(b._h, desc, C.byref(h))
    assert not h.value
    L.check(rc)


def nn_create(b):
    b.nn_destroy(b.nn_create(4))


def calls(ctx, am, b):
    """(place, entry point's name in the message, the call), in an order that leaves the SSD batch with the template each call needs"""
    esm2 = mtf_amd.sm_desc(L.SM_ESM, hess_type=2, sec_ord_hess=1)
    iclk = mtf_amd.sm_desc(L.SM_ICLK)
    gd = L.GridDesc(1, 1, 10, 10, 0, 0, 1)

    def ready(sm):
        if am == T.SSD:
            b.set_corners(CORNERS[None]); b.init_template(sm)

    return [
        ("3ch", "batch_create", lambda: new_batch(ctx, am, n_channels=3).close()),
        ("sec_ord", "init_template", lambda: b.init_template(esm2)),
        ("sec_ord", "cmpt_init_hessian (second order)", b.cmpt_init_hessian2),
        ("sec_ord", "cmpt_curr_hessian (second order)", b.cmpt_curr_hessian2),
        ("sec_ord", "cmpt_self_hessian (second order)", b.cmpt_self_hessian2),
        ("sec_ord", "cmpt_sum_of_hessians (second order)", b.cmpt_sum_of_hessians2),
        ("additive", "init_template", lambda: b.init_template(mtf_amd.sm_desc(L.SM_FALK))),
        ("update_model", "update_model", lambda: (ready(iclk), b.update_model())),
        ("score_candidates", "score_candidates", lambda: b.score_candidates(np.zeros((4, 8)))),
        ("sample_candidates", "sample_candidates", lambda: b.sample_candidates(np.zeros((4, 8)))),
        ("nn_dataset", "nn_dataset", lambda: b.nn_dataset(4, np.full(8, 0.01))),
        ("nn_create", "nn_create", lambda: nn_create(b)),
        ("pf_create", "pf_create", lambda: pf_create(b)),
        ("grid", "grid_update", lambda: b.grid_update(CORNERS[None], iclk)),
        ("grid", "grid_frame", lambda: b.grid_frame(gd, iclk, CORNERS)),
    ]


@pytest.mark.parametrize("am", T.MODELS)
def test_refused_pairs_are_refused_with_the_tables_bytes(gpu_ctx, frame, am):
    gpu_ctx.set_image(frame)
    b = new_batch(gpu_ctx, am)
    try:
        b.set_corners(CORNERS[None])
        seen = set()
        for place, fn, call in calls(gpu_ctx, am, b):
            want = T.text(am, place, fn)
            seen.add(place)
            if want is None and am != T.SSD:
                continue                      # (the served side is SSD's to show: another model would need its own template and parameters)
            try:
                call()
                code, msg = 0, ""
            except mtf_amd.MtfHipError as e:
                code, msg = e.code, L.lib().mtfhip_last_error().decode()
            if want is None:
                assert code != -2, (place, fn, code, msg)
            else:
                assert code == -2 and msg == want, (place, fn, code, msg, want)
        assert seen == set(T.PLACES) and all((am, p) in T.REFUSALS for p in T.PLACES)
    finally:
        b.close()

