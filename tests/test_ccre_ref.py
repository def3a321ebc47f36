"""CCRE (am = MTFHIP_AM_CCRE, AM/src/CCRE.cc) without a GPU: the float64 generator tests/golden/make_golden12.py against itself (derivatives,
the relations at It = I0, pixels at 255), the host / device tables header mtfhip_ccre_tables.h as a stand-alone sanitised program against the
generator's tables, and the ABI with the refusals that need no device."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "mtf_amd", "csrc")
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden12 as M  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "lk_golden12.npz"))
TAGS = [str(t) for t in G["tags"]]
LD = np.longdouble


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def cfg(tag):
    resx, resy, aff, nb, pou = (int(v) for v in G[tag + "_cfg"])
    return resx, resy, bool(aff), nb, pou


def patch(tag):
    resx, resy, aff, nb, pou = cfg(tag)
    pa = M.G10.Patch(G["img"].astype(np.float64), resx, resy, aff, G[tag + "_corners"])
    mult, add = M.pix_norm(nb, pou)
    return pa, mult, add


# ------------------------------------------------------------------ the fixture
def test_cases_cover_the_issue():
    shapes = {cfg(t)[:3] for t in TAGS}
    assert {(7, 9, False), (13, 11, False), (50, 50, False), (25, 20, True)} <= shapes
    assert {(8, 0), (10, 1), (4, 1), (16, 0), (2, 0)} <= {cfg(t)[3:] for t in TAGS}
    assert 7 * 9 < 64 and (13 * 11) % 64 != 0
    I0, It = G["h50a_I0"], G["h50a_It"]
    assert (I0 == 0).any() and (I0 == 7).any() and (It == 7).any()          # raw 0 and raw 255 (bin nb - 1 exactly)
    for name in ("I0", "It"):                                                # the quantised region on the lattice: integers, on the branch boundaries
        v = G["a25x20i_" + name]
        assert (v == np.rint(v)).sum() > v.size // 2
    # a loop record for every case and every run; each case has one of more than one iteration, and the 50 x 50 and 25 x 20 cases whole loops
    for t in TAGS:
        iters = [int(G["%s_%s%s_loop_iters" % (t, k, lm)]) for k in ("esm_ds", "fclk_cs", "iclk_is") for lm in ("", "_lm")]
        assert min(iters) >= 1 and max(iters) >= 2, (t, iters)
        if cfg(t)[:2] in ((50, 50), (25, 20)):
            assert max(iters) == int(G["loop_cfg"][0]), (t, iters)
    n3 = [int(G["h50%s_esm_ds_loop_n" % s]) for s in "abc"]
    assert len(set(n3)) > 1 and min(n3) < int(G["loop_cfg"][0])             # one target of the batch of three stops early


@pytest.mark.parametrize("tag", ["h50a", "a25x20i", "h7x9p4", "h13x11b2"])
def test_fixture_regenerates_from_its_inputs(tag):
    pa, mult, add = patch(tag)
    _, _, _, nb, _ = cfg(tag)
    p = G[tag + "_p"]
    It, Jt = pa.sample(pa.warp(p), p)
    assert np.array_equal(mult * It + add, G[tag + "_It"]) and np.array_equal(mult * pa.I0o + add, G[tag + "_I0"])
    q = M.quantities(G[tag + "_I0"], G[tag + "_It"], mult * pa.J0, mult * Jt, nb, float(G[tag + "_pre_seed"]))
    for name in M.SUMMED + ("df_dIt", "df_dI0"):
        assert np.array_equal(np.asarray(q[name], dtype=np.float64), G[tag + "_" + name]), name


# ------------------------------------------------------------------ the generator against itself
NO_DFDIT_FD = ("h50a", "h50b", "h50c", "h50s0", "h13x11b2")      # the cases with a template pixel in the first or the last two bins


def _f(I0, It, nb, ps):
    z = np.zeros((I0.size, 1), dtype=LD)
    return M.quantities(I0, It, z, z, nb, ps, LD)["f"]


@pytest.mark.parametrize("tag", TAGS)
def test_gradients_are_the_central_differences_of_f(tag):
    """in longdouble, pixel by pixel.  df_dI0 is the derivative of f in I0 for every case.  df_dIt is the derivative in It where every
    template window sums to one -- no pixel of I0 whose window is cut at bin 0 or at the last bin (always so with partition of unity); where
    one is cut, cum_hist is no longer the row sum of cum_joint, and the reference's expression (kept) leaves that term out, as MI's does
    (make_golden5.py)"""
    _, _, _, nb, pou = cfg(tag)
    ps = float(G[tag + "_pre_seed"])
    I0, It = G[tag + "_I0"].astype(LD), G[tag + "_It"].astype(LD)
    h = LD(1e-6)
    fl = np.trunc(G[tag + "_I0"])
    # (a value exactly on a bin has no weight in its fourth tap: a raw 255 under partition of unity, on bin nb - 2, loses nothing)
    cut = bool(((fl - 1 < 0) | ((fl + 2 > nb - 1) & (G[tag + "_I0"] > fl))).any())
    assert not (pou and cut)
    assert cut == (tag in NO_DFDIT_FD), (tag, cut)
    scale_t, scale_0 = np.abs(G[tag + "_df_dIt"]).max(), np.abs(G[tag + "_df_dI0"]).max()
    # (pixels away from the piece boundaries by more than the step: across one the one-sided derivatives of the truncated constants' pieces differ)
    ok = np.flatnonzero((np.abs(G[tag + "_I0"] - np.rint(G[tag + "_I0"])) > 1e-3) & (np.abs(G[tag + "_It"] - np.rint(G[tag + "_It"])) > 1e-3))
    for k in ok[:: max(1, ok.size // 6)][:6]:
        e = np.zeros(I0.size, dtype=LD)
        e[k] = h
        fd0 = float((_f(I0 + e, It, nb, ps) - _f(I0 - e, It, nb, ps)) / (2 * h))
        assert abs(fd0 - G[tag + "_df_dI0"][k]) < 1e-6 * scale_0, (k, fd0, G[tag + "_df_dI0"][k])
        if not cut:
            fdt = float((_f(I0, It + e, nb, ps) - _f(I0, It - e, nb, ps)) / (2 * h))
            assert abs(fdt - G[tag + "_df_dIt"][k]) < 1e-6 * scale_t, (k, fdt, G[tag + "_df_dIt"][k])


@pytest.mark.parametrize("tag", ["h50a", "h50p10", "a25x20", "h7x9p4", "h13x11b2"])
def test_relations_at_the_template(tag):
    """with It = I0: updateSimilarity's f is initializeSimilarity's, df_dIt is initializeGrad's vector, and cmptSelfHessian(J0) equals
    cmptCurrHessian(J0) to rounding (Diagnostics)"""
    pa, mult, add = patch(tag)
    _, _, _, nb, _ = cfg(tag)
    I0, J0 = G[tag + "_I0"], mult * pa.J0
    q = M.quantities(I0, I0, J0, J0, nb, float(G[tag + "_pre_seed"]))
    assert q["f"] == float(G[tag + "_f_init"])
    assert np.array_equal(q["df_dIt"], G[tag + "_df_init"])
    assert rel(q["H_self"], q["H_curr"]) < 1e-13
    assert rel(q["H_self"], G[tag + "_H0"]) == 0


@pytest.mark.parametrize("nb,pou", [(8, 0), (16, 0), (2, 0), (10, 1), (4, 1)])
def test_pixels_at_255(nb, pou):
    """a raw 255 lands exactly on norm_pix_max; its window ends there (two bins wide without partition of unity) and its cumulative weight
    in that bin is cumBSpl3(0) = 1 / 2, 1 in every bin below the window"""
    mult, add = M.pix_norm(nb, pou)
    N = 97
    It = np.full(N, mult * 255.0 + add)
    top = nb - 2 if pou else nb - 1
    assert It[0] == top
    I0 = np.linspace(add, top, N)
    norm = 1.0 / (N + nb * nb * 10.0)
    B, _, _, C, dC, _, _ = M.weights(I0, It, nb, norm, np.float64)
    t = M.tables(C, B, nb, 10.0, norm)
    assert np.array_equal(C[top], np.full(N, 0.5)) and (C[:max(0, top - 1)] == 1).all()
    # the window reaches one bin further up where there is one (partition of unity): cumBSpl3(1) = 1 / 24 to the truncated constants; then 0
    if pou:
        assert np.allclose(C[top + 1], 1.0 / 24, rtol=0, atol=1e-10)
    assert (C[top + 1 + pou:] == 0).all() and (dC[top + 1 + pou:] == 0).all()
    assert C.shape[0] == top + 1 + pou
    assert t["raw_cum"][top] == 0.5 * N
    assert np.allclose(t["raw_joint"][top], 0.5 * B.sum(axis=1), rtol=1e-15, atol=0)
    if not pou:
        assert np.count_nonzero(C[:, 0] != 1) == 2 or nb == 2


# ------------------------------------------------------------------ the host / device tables header
PROGRAM = r"""
#include "mtfhip_ccre_tables.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace mtfhip;
/* in: records of [nb, pre_seed, norm, raw 3R (padded to 816)]; out: the table block after CCRE_TB_INIT from the template's sums, then
 * CCRE_TB_UPDATE with_self from the current patch's -- [f_init, f, block CCRE_SIZE] per record */
int main(int argc, char **argv) {
	if (argc != 4) return 2;
	const int n = atoi(argv[3]);
	const int REC = 3 + 2 * 816;
	std::vector<double> in((size_t)n * REC), out((size_t)n * (2 + CCRE_SIZE));
	FILE *f = fopen(argv[1], "rb");
	if (!f || fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
	fclose(f);
	for (int k = 0; k < n; ++k) {
		const double *r = &in[(size_t)k * REC];
		const int nb = (int)r[0];
		const int R = nb + nb * nb;
		std::vector<double> raw0(r + 3, r + 3 + 3 * R), raw1(r + 3 + 816, r + 3 + 816 + 3 * R);   /* exact sizes: the sanitizer sees every read */
		std::vector<double> tb(CCRE_SIZE, 0.0), red(1);
		double *o = &out[(size_t)k * (2 + CCRE_SIZE)];
		ccre_tables(0, 1, [] {}, nb, r[1], r[2], CCRE_TB_INIT, 0, raw0.data(), tb.data(), red.data(), &o[0]);
		ccre_tables(0, 1, [] {}, nb, r[1], r[2], CCRE_TB_UPDATE, 1, raw1.data(), tb.data(), red.data(), &o[1]);
		for (int q = 0; q < CCRE_SIZE; ++q) o[2 + q] = tb[q];
	}
	f = fopen(argv[2], "wb");
	if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
	fclose(f);
	return 0;
}
"""
OFF = dict(HIST_0=0, CUM_T=16, JOINT=64, L=320, P=576, SELF_JOINT=832, SELF_L=1088, COLSUM=1344, RATIO=1360, HIST_T=1376, SIZE=1408)


@pytest.fixture(scope="module")
def table_outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("ccre_tables")
    src, exe, fin, fout = str(d / "t.cpp"), str(d / "t"), str(d / "in.bin"), str(d / "out.bin")
    open(src, "w").write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, src, "-o", exe], check=True)
    recs = []
    for tag in TAGS:
        _, _, _, nb, _ = cfg(tag)
        ps, N, R = float(G[tag + "_pre_seed"]), G[tag + "_I0"].size, nb + nb * nb
        norm = 1.0 / (N + nb * nb * ps)
        B, _, _, C0, _, _, _ = M.weights(G[tag + "_I0"], G[tag + "_I0"], nb, norm, np.float64)
        raw0, raw1 = np.zeros(816), np.zeros(816)
        raw0[:R] = np.concatenate([C0.sum(axis=1), (C0 @ B.T).ravel()])
        raw0[2 * R:2 * R + nb] = G[tag + "_raw_hist0"]
        raw1[:2 * R + nb] = G[tag + "_raw"]
        recs.append(np.concatenate([[nb, ps, norm], raw0, raw1]))
    np.stack(recs).tofile(fin)
    r = subprocess.run([exe, fin, fout, str(len(TAGS))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    out = np.fromfile(fout).reshape(len(TAGS), 2 + OFF["SIZE"])
    return {t: out[k] for k, t in enumerate(TAGS)}


@pytest.mark.parametrize("tag", TAGS)
def test_tables_header_matches_the_generator(table_outputs, tag):
    """ccre_tables on the generator's raw sums: the same few operations per cell -- seeds, logs, differences -- so a few ulps of the cell;
    f and the column sums add nb^2 / nb of them"""
    o = table_outputs[tag]
    _, _, _, nb, _ = cfg(tag)
    tb = o[2:]

    def sq(off):
        return tb[off:off + 256].reshape(16, 16)[:nb, :nb]
    assert abs(o[0] - float(G[tag + "_f_init"])) <= 1e-13 * max(1.0, abs(float(G[tag + "_f_init"])))
    assert abs(o[1] - float(G[tag + "_f"])) <= 1e-13 * max(1.0, abs(float(G[tag + "_f"])))
    for off, name in (("HIST_0", "hist0"), ("CUM_T", "cum_hist"), ("COLSUM", "colsum"), ("HIST_T", "hist_t")):
        assert rel(tb[OFF[off]:OFF[off] + nb], G[tag + "_" + name]) < 1e-14, name
    for off, name in (("JOINT", "cum_joint"), ("SELF_JOINT", "self_joint")):
        assert rel(sq(OFF[off]), G[tag + "_" + name]) < 1e-14, name
    # the log terms: differences of logs of order |log norm| ~ 8, so absolute
    for off, name in (("L", "L"), ("SELF_L", "self_L")):
        assert np.abs(sq(OFF[off]) - G[tag + "_" + name]).max() < 1e-13, name
    L = G[tag + "_L"]
    P = np.vstack([np.zeros(nb), np.cumsum(1 + L, axis=0)[:-1]])
    assert np.abs(sq(OFF["P"]) - P).max() < 1e-12
    assert rel(tb[OFF["RATIO"]:OFF["RATIO"] + nb], G[tag + "_colsum"] / G[tag + "_hist0"]) < 1e-14


def test_table_block_fits_the_mi_block():
    hdr = open(os.path.join(CSRC, "mtfhip_ccre_tables.h")).read()
    internal = open(os.path.join(CSRC, "mtfhip_internal.h")).read()
    assert "CCRE_SIZE = %d" % OFF["SIZE"] in hdr and "MI_SIZE = 1600" in internal and OFF["SIZE"] <= 1600
    for name, off in OFF.items():
        assert "CCRE_%s = %d" % (name, off) in hdr, name


# ------------------------------------------------------------------ the ABI
def test_ccre_abi():
    import mtf_amd
    from mtf_amd import _lib as L
    assert L.AM_CCRE == 9 and mtf_amd.AM_CCRE == 9
    assert "MTFHIP_AM_CCRE = 9" in open(os.path.join(ROOT, "include", "mtfhip.h")).read()
    lib = ctypes.CDLL(L.LIB_PATH)
    for s in L.SYMBOLS:
        assert hasattr(lib, s), s
    host = ctypes.CDLL(os.path.join(ROOT, "mtf_amd", "libmtfharness.so"))
    assert hasattr(host, "mtfhost_create_ccre")


def _create(**kw):
    """mtfhip_batch_create's validation runs before the context is looked at: a dummy context reaches every refusal that needs no device"""
    from mtf_amd import _lib as L
    from mtf_amd.api import PatchDesc
    d = dict(am=L.AM_CCRE, ssm=L.SSM_HOMOGRAPHY, resx=10, resy=10, grad_eps=1e-8, likelihood_alpha=1.0, mi_n_bins=8, mi_pre_seed=10.0, mi_pou=0,
             hess_eps=1.0, n_channels=1)
    d.update(kw)
    desc = PatchDesc(*[d[k] for k in ("am", "ssm", "resx", "resy", "grad_eps", "likelihood_alpha", "mi_n_bins", "mi_pre_seed", "mi_pou", "hess_eps",
                                      "n_channels")])
    dummy = ctypes.create_string_buffer(4096)
    h = ctypes.c_void_p()
    rc = L.lib().mtfhip_batch_create(ctypes.cast(dummy, ctypes.c_void_p), ctypes.byref(desc), 1, ctypes.byref(h))
    return rc, L.lib().mtfhip_last_error().decode()


def test_refusals_that_need_no_device():
    from mtf_amd import _lib as L
    rc, msg = _create(mi_n_bins=3, mi_pou=1)
    assert rc != 0 and "CCRE::Too few bins 3 specified to enforce partition of unity constraint" in msg
    rc, msg = _create(mi_n_bins=17)
    assert rc != 0 and "CCRE: n_bins 17 outside [2, 16]" in msg
    rc, msg = _create(mi_n_bins=1)
    assert rc != 0 and "n_bins 1" in msg
    rc, msg = _create(n_channels=3)
    assert rc == -2 and "MCCCRE" in msg
    for ssm in L.SSM_LOW_ORDER:
        rc, msg = _create(ssm=ssm)
        assert rc == -2 and "is served with SSD, NCC and SSIM only" in msg


def test_python_trackers_refuse_ccre_before_any_device_call():
    import mtf_amd
    from mtf_amd import sm
    for cls in (sm.GridTracker, sm.ParticleFilter, sm.NNDataset, sm.NNTracker):
        with pytest.raises(mtf_amd.FunctionNotImplemented):
            cls(None, am=mtf_amd.AM_CCRE)


def test_host_layer_refuses_symmetrical_grad():
    """HipAM("ccre") with CCREParams::symmetrical_grad = 1 throws FunctonNotImplemented before any device call"""
    from mtf_amd import host
    with pytest.raises(Exception) as e:
        host.CppTracker.ccre(0, symmetrical_grad=1)
    assert "symmetrical_grad" in str(e.value)
