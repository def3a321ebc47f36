"""The seams of the histogram appearance models (MI, CCRE), no GPU: the conditions the references alone must meet on every case of
tests/helpers/hist_seam_cases.py so that the device comparison of tests/test_gpu_hist_seams.py is meaningful.

(a) the table covers what it claims: every pixel shape on `inside`, every region on the three edge shapes, every MI_CASES row on every region
    and on both SSMs there, every bin-count group, unique ids; a CCRE case stands for every served method (the device test runs them all);
(b) every case is finite.  Wholly outside the frame, and on `flat0` (wholly inside the exact-zero block), f is finite and g and H are exactly
    zero: every image gradient there is a difference of equal samples.  Established here for both regions, for the oracle's MI at 8 bins and
    at 10 bins with partition of unity and for the CCRE generator at 8 and 16 bins -- `flat0` needed no replacement;
(c) the half-outside regions have 20 .. 80 % of their template samples equal to the border constant, and every edge has a shape whose
    64-aligned runs (the waves of a kernel that takes the pixels in order) mix the two kinds;
(d) no sample coordinate is within 1e-6 of an integer, and no normalised sample within 1e-9 of a bin boundary (where the B-spline pieces
    switch) unless it is exactly reproducible: the border constant, the exact 0 and 255 blocks (pou's exact 1.0 among them);
(e) the jitter floor: corners moved by the seeded +-1e-12 px of tests/test_lk_seams_cpu.py move the oracle's f, H and g by less than a tenth
    of the device-grid bounds of tests/test_gpu_parity.py::_fused_follow.  A condition on the table, not a tolerance;
(f) at FCLK the oracle agrees with the independent NumPy float64 definitions (numpy_mi: tests/golden/make_golden5.py::mi_case for two frames)
    within the tolerances of tests/test_oracle_golden5.py;
(g) the CCRE generator at the new bin counts against its own definition, with the tolerances of tests/test_ccre_ref.py: df_dI0 (and df_dIt
    where no template window is cut) is the long-double central difference of f within 1e-6, and at It = I0 the self and the current
    Hessian agree within 1e-13.  (make_golden12.py has one form of each expression, the dense one; these are the checks test_ccre_ref.py
    makes of it.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hist_seam_cases as K   # noqa: E402

LD = np.longdouble
BOUND_F, BOUND_H, BOUND_G = K.TP.FOLLOW_BOUNDS["device_grid"]


def test_table_covers_what_it_claims():
    assert 200 <= len(K.CASES) <= 300 and len(set(K.IDS)) == len(K.CASES)
    mi = [c for c in K.CASES if c.am == K.MI]
    cc = [c for c in K.CASES if c.am == K.CCRE]
    for am_cases in (mi, cc):
        for shape in K.PIXEL_SHAPES:                                  # every shape on `inside`
            assert any((c.resx, c.resy) == shape and c.region == "inside" for c in am_cases), shape
        for shape in K.EDGE_SHAPES:                                   # every edge region on the three edge shapes
            assert {c.region for c in am_cases if (c.resx, c.resy) == shape} >= set(K.EDGE_REGIONS), shape
    for region in K.REGIONS:                                          # every row on every region, and both SSMs there
        assert {c.row for c in mi if c.region == region} == set(range(13)), region
        assert {c.ssm for c in mi if c.region == region} == {K.HOM, K.AFF}, region
        assert {c.ssm for c in cc if c.region == region} == {K.HOM, K.AFF}, region
        assert {c.extra["chained_warp"] for c in cc if c.region == region} == {0, 1}, region
    for region in K.EDGE_REGIONS:                                     # both configurations of each model on every edge region
        assert {(c.nb, c.pou) for c in mi if c.region == region} == {(8, 0), (10, 1)}
        assert {(c.nb, c.pou) for c in cc if c.region == region} == {(8, 0), (16, 0)}
    # below 400 pixels the pixel-count group is affine
    assert all(c.ssm == K.AFF for c in K.CASES if c.group == "px" and K.n_pix(c) < 400)
    assert {c.ssm for c in K.CASES if c.group == "px" and K.n_pix(c) >= 400} == {K.HOM, K.AFF}
    # the bin-count groups
    assert {c.nb for c in cc if c.group == "bins"} == set(K.BINS_DENSE) == {c.nb for c in mi if c.group == "bins"}
    assert {(c.nb, c.pou) for c in mi if c.group == "bins_rc"} == set(K.BINS_RECOMPUTE)
    assert all(c.row in K.RECOMPUTE_ROWS for c in mi if c.group == "bins_rc")
    assert {c.row for c in mi if c.group == "bins_rc"} == set(K.RECOMPUTE_ROWS)
    # kMiPairs' pairs per lane, ceil(nb^2 / 64), step inside the dense list
    pairs = {nb: -(-nb * nb // 64) for nb in K.BINS_DENSE + [8]}
    assert pairs[8] < pairs[9] and pairs[11] < pairs[12] and pairs[13] < pairs[14]
    assert sum(c.group == "cap" for c in K.CASES) == 2 and K.CAP_SHAPE[0] * K.CAP_SHAPE[1] > 64 * 1024
    for corners in K.REGIONS.values():
        assert np.all(np.abs(corners - np.round(corners)) > 1e-3)
    img, img2 = K.frames()
    assert img.shape == (256, 256) and img.dtype == np.float32 and img2.dtype == np.float32 and not np.array_equal(img, img2)


def _exact(pts, img):
    """samples that are exactly reproducible: outside the frame (the border constant), or in a cell whose four texels are equal (the exact 0
    and 255 blocks: raw 0 is exactly 0, or pou's exact 1.0; raw 255 is 255 to the rounding of the four weights, whatever the coordinates)"""
    h, w = img.shape
    x, y = pts
    outside = (x < 0) | (x > w - 1) | (y < 0) | (y > h - 1)
    lx, ly = np.clip(np.floor(x).astype(int), 0, w - 2), np.clip(np.floor(y).astype(int), 0, h - 2)
    flat = (img[ly, lx] == img[ly, lx + 1]) & (img[ly, lx] == img[ly + 1, lx]) & (img[ly, lx] == img[ly + 1, lx + 1])
    return outside | flat


def _off_the_boundaries(v, pts, img, what):
    assert np.abs(pts - np.round(pts)).min() > 1e-6, what
    near = np.abs(v - np.round(v)) <= 1e-9
    assert not (near & ~_exact(pts, img)).any(), what


@pytest.mark.parametrize("cid", K.MI_IDS)
def test_mi_reference_conditions(oracle, cid):
    c = K.BY_ID[cid]
    ref = K.reference(oracle, cid)
    rec = ref["rec"]
    mult, add = K.R.mi_pix_norm(c.nb, c.pou)
    # (b)
    assert np.isfinite(rec["f"]) and np.all(np.isfinite(rec["g"])) and np.all(np.isfinite(rec["H"]))
    pts = ref["init_pts"].reshape(-1, 2).T
    if c.region in K.FLAT:
        flat = mult * (128.0 if c.region == "outside" else 0.0) + add
        assert np.all(ref["I0"] == flat) and np.all(ref["It"] == flat)
        assert np.all(rec["g"] == 0.0) and np.all(rec["H"] == 0.0)
        if c.region == "flat0" and c.pou:
            assert flat == 1.0
        return
    assert np.abs(rec["H"]).max() > 0 and np.abs(rec["g"]).max() > 0
    # (c)
    if c.region in K.HALF_OUTSIDE:
        border = ref["I0"] == mult * 128.0 + add
        assert 0.2 <= border.mean() <= 0.8, border.mean()
    # (d)
    _off_the_boundaries(ref["I0"], pts, K.frames()[0], "I0")
    _off_the_boundaries(ref["It"], pts, K.frames()[1], "It")
    if c.region == "h50a":
        assert (ref["I0"] == add).sum() > 20 and (ref["I0"] == mult * 255.0 + add).sum() > 20
    # (e)
    if c.group == "cap":
        return          # (one more 65 792-pixel oracle run: the jitter floor of this region is held at the fourteen other shapes)
    fl = K.case_floor(oracle, cid)
    print("%s: jitter floor %s" % (cid, fl))
    assert fl["f"] < 0.1 * BOUND_F and fl["H"] < 0.1 * BOUND_H and fl["g"] < 0.1 * BOUND_G, fl


def test_every_edge_has_a_mixed_wave(oracle):
    for region in K.HALF_OUTSIDE:
        mixed = []
        for c in K.CASES:
            if c.am == K.MI and c.region == region and K.n_pix(c) >= 64:
                mult, add = K.R.mi_pix_norm(c.nb, c.pou)
                border = K.reference(oracle, c.id)["I0"] == mult * 128.0 + add
                mixed.append(any(0 < border[s:s + 64].sum() < 64 for s in range(0, K.n_pix(c), 64)))
        assert mixed and any(mixed), region


FCLK_H = {0: "H_init0", 1: "H_self1", 2: "H_curr"}


@pytest.mark.parametrize("cid", [c.id for c in K.CASES if c.am == K.MI and c.sm == K.FCLK and c.group != "cap"])
def test_oracle_agrees_with_the_numpy_definitions_at_fclk(oracle, cid):
    """(f): f 1e-10, g and H 1e-5 (tests/test_oracle_golden5.py); on the flat regions both are exactly zero"""
    c = K.BY_ID[cid]
    rec = K.reference(oracle, cid)["rec"]
    m = K.numpy_mi(c.nb, c.pou, c.resx, c.resy, c.ssm == K.AFF, K.REGIONS[c.region])
    H = m[FCLK_H[c.extra.get("hess_type", 1)]]
    assert abs(rec["f"] - m["f"]) <= 1e-10 * abs(m["f"])
    if c.region in K.FLAT:
        assert not m["Jt"].any() and not m["g"].any() and not H.any()
        return
    assert K.rel(rec["g"], m["g"]) < 1e-5, K.rel(rec["g"], m["g"])
    assert K.rel(rec["H"], H) < 1e-5, K.rel(rec["H"], H)


# ---------------------------------------------------------------- CCRE
@pytest.mark.parametrize("cid", [i for i in K.CCRE_IDS if K.BY_ID[i].group != "cap"])
def test_ccre_reference_conditions(cid):
    c = K.BY_ID[cid]
    a = K.ccre_arrays(c.resx, c.resy, c.ssm == K.AFF, K.REGIONS[c.region], c.nb, c.pou)
    q, q0 = K.ccre_quantities(a, c.nb)
    mult, add = K.G12.pix_norm(c.nb, c.pou)
    assert np.isfinite(q["f"]) and np.isfinite(q0["f"])
    for sm, jac, ht in K.CCRE_METHODS:
        g, H = K.TC.ref_g_H(q, q0["H_self"], sm, jac, ht)
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(H)), (sm, jac, ht)
        if c.region in K.FLAT:
            assert not np.any(g) and not np.any(H), (sm, jac, ht)
    if c.region in K.FLAT:
        flat = mult * (128.0 if c.region == "outside" else 0.0) + add
        assert np.all(a["I0"] == flat) and np.all(a["It"] == flat) and not a["J0"].any() and not a["Jt"].any()
        return
    if c.region in K.HALF_OUTSIDE:
        border = a["I0"] == mult * 128.0 + add
        assert 0.2 <= border.mean() <= 0.8, border.mean()
    _off_the_boundaries(a["I0"], a["pts"], K.frames()[0], "I0")
    _off_the_boundaries(a["It"], a["pts"], K.frames()[1], "It")


def _f(I0, It, nb):
    z = np.zeros((I0.size, 1), dtype=LD)
    return K.G12.quantities(I0, It, z, z, nb, K.PRE_SEED, LD)["f"]


@pytest.mark.parametrize("nb", K.BINS_DENSE)
def test_ccre_generator_at_the_new_bin_counts(nb):
    """(g), on the 50 x 50 patch of the bin-count group"""
    a = K.ccre_arrays(K.BIN_SHAPE[0], K.BIN_SHAPE[1], False, K.REGIONS["h50a"], nb, 0)
    q, q0 = K.ccre_quantities(a, nb)
    assert K.TC.rel(q0["H_self"], q0["H_curr"]) < 1e-13
    I0, It = a["I0"].astype(LD), a["It"].astype(LD)
    h = LD(1e-6)
    fl = np.trunc(a["I0"])
    cut = bool(((fl - 1 < 0) | ((fl + 2 > nb - 1) & (a["I0"] > fl))).any())
    assert cut                      # (h50a's region holds raw 0 and raw 255: a window is cut at either end)
    scale_0 = np.abs(q["df_dI0"]).max()
    ok = np.flatnonzero((np.abs(a["I0"] - np.rint(a["I0"])) > 1e-3) & (np.abs(a["It"] - np.rint(a["It"])) > 1e-3))
    for k in ok[:: max(1, ok.size // 4)][:4]:
        e = np.zeros(I0.size, dtype=LD)
        e[k] = h
        fd0 = float((_f(I0 + e, It, nb) - _f(I0 - e, It, nb)) / (2 * h))
        assert abs(fd0 - q["df_dI0"][k]) < 1e-6 * scale_0, (k, fd0, q["df_dI0"][k])


# ---------------------------------------------------------------- the loops (Part B)
def test_the_solve_of_a_zero_system_is_zero(oracle):
    """what the flat regions' loops rest on: H = 0, g = 0 gives no update (the rank-revealing solve), so the corners stay and the loop stops"""
    for S in (6, 8):
        assert not np.any(oracle.colpiv_qr_solve(np.zeros((S, S)), np.zeros(S)))


@pytest.mark.parametrize("model", range(len(K.MI_LOOP_MODELS)))
def test_mi_loops_stop_clear_of_epsilon(oracle, model):
    """every loop of Part B has an epsilon no corner change comes within a factor 1.5 of, so n_iters can be held to equality; the batch of
    three stops after different passes"""
    sm, extra, nb, pou = K.MI_LOOP_MODELS[model]
    for shape in K.LOOP_SHAPES:
        for region in K.LOOP_REGIONS:
            run = K.mi_trace(oracle, sm, K.HOM, extra, shape[0], shape[1], K.REGIONS[region], nb, pou)
            eps, margin = K.pick_eps([run])
            print(shape, region, K.sm_name(sm), eps, margin, K.stop_at(run["changes"], eps))
            assert margin > 1.5, (shape, region, eps, margin)
            assert np.all(np.isfinite(run["corners"]))
    runs = [K.mi_trace(oracle, sm, K.HOM, extra, K.BATCH3_SHAPE[0], K.BATCH3_SHAPE[1], K.REGIONS[r], nb, pou) for r in K.BATCH3]
    eps, margin = K.pick_eps(runs)
    n = [K.stop_at(r["changes"], eps) for r in runs]
    print("batch of three", K.sm_name(sm), eps, margin, n)
    assert margin > 1.5 and len(set(n)) > 1 and n[2] == 1


@pytest.mark.parametrize("key", K.CCRE_LOOP_KEYS)
def test_ccre_loops_pin_at_least_one_iteration(key):
    for shape in K.LOOP_SHAPES:
        for region in K.LOOP_REGIONS:
            ref = K.ccre_loop(shape[0], shape[1], region, K.CCRE_LOOP_BINS, key)
            print(shape, region, key, ref["iters"])
            assert ref["iters"] >= 1, (shape, region)
            if region == "flat0":
                assert all(np.array_equal(c, K.REGIONS[region]) for c in ref["corners"])
    if key == K.CCRE_BATCH_KEY:
        iters = [K.ccre_loop(K.BATCH3_SHAPE[0], K.BATCH3_SHAPE[1], r, K.CCRE_LOOP_BINS, key)["iters"] for r in K.BATCH3]
        assert min(iters) >= 2, iters          # the flat target stops after one pass, its neighbours go on


# ---------------------------------------------------------------- three channels, candidates
@pytest.mark.parametrize("shape", K.MC_SHAPES, ids=lambda s: "%dx%d" % s)
def test_three_channel_reference_conditions(oracle, shape):
    """3 NP rows = 63, 66, 255, 258: a 64-row chunk ends inside a pixel; finite, not flat, the jitter floor a tenth of the device-grid bounds"""
    resx, resy = shape
    assert (3 * resx * resy) % 64 in (63, 2) and (3 * resx * resy) % 3 == 0 and 64 % 3 != 0
    ref = K.mi_reference(oracle, K.FCLK, K.HOM, {}, resx, resy, K.REGIONS["inside"], 8, 0, 3)
    assert ref["I0"].size == 3 * resx * resy
    rec = ref["rec"]
    assert np.isfinite(rec["f"]) and np.abs(rec["H"]).max() > 0 and np.all(np.isfinite(rec["H"])) and np.all(np.isfinite(rec["g"]))
    fl = K.mi_floor(oracle, K.FCLK, K.HOM, {}, resx, resy, K.REGIONS["inside"], 8, 0, 3)
    assert fl["f"] < 0.1 * BOUND_F and fl["H"] < 0.1 * BOUND_H and fl["g"] < 0.1 * BOUND_G, fl


def test_batch_and_candidate_shapes():
    assert [s[0] * s[1] for s in K.CAND_SHAPES] == [63, 65, 1025] and K.N_CAND == 37
    assert len({c.tobytes() for c in K.CYCLE}) == 4


def test_the_cumulative_window_clamps_are_beyond_every_eight_bit_sample():
    """cum_fill's min(a.lo, nb) and ccre_cum_dot's P[min(a.lo, CCRE_NB - 1)] (mtfhip_mi_device.h, mtfhip_ccre_device.h) bind only for a
    window that starts at or past the last bin.  A raw 255 -- the largest sample of an 8-bit frame, the border constant and every saturated
    block included -- is normalised to the last bin (or, with partition of unity, to the one before it) at most one rounding above it, so
    its window starts two bins lower: no case of this table, and no frame in [0, 255], reaches either clamp.  They guard frames that leave
    that range; a kernel without them cannot be told apart here, and with such a frame it would index past its slab, so the suite holds the
    rows below the window (cum_fill's 1.0 rows, which every CCRE case sums) instead."""
    for nb in range(2, 17):
        for pou in ((0, 1) if nb >= 4 else (0,)):
            mult, add = K.G12.pix_norm(nb, pou)
            v = mult * 255.0 + add
            lo = max(0, int(v) - 1)
            assert int(v) <= nb - 1 and lo <= nb - 2, (nb, pou, v, lo)          # (min(lo, nb) = lo and min(lo, CCRE_NB - 1) = lo)
