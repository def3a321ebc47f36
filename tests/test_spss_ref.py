"""The SPSS appearance model (AM/src/SPSS.cc) without a GPU: the float64 reference of tests/golden/make_golden10.py against the model's
own properties -- df_dIt is the derivative of f, df_dI0 is the reference's expression and differs from the derivative by exactly
-2 c a / den^2, the self and curr Hessians coincide at It = I0, the self Hessian is negative definite, the likelihood is 1 at It = I0 --
and the ABI: the exported symbol, the unchanged mtfhip_patch_desc, and what fused_select serves for am = 7."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mtf_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden10 as M  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "lk_golden10.npz"))
TAGS = [str(t) for t in G["tags"]]


def _patch(tag):
    resx, resy, affine = (int(v) for v in G[tag + "_cfg"])
    pa = M.Patch(G["img"].astype(np.float64), resx, resy, bool(affine), G[tag + "_corners"])
    return pa, M.spss_c(float(G[tag + "_k"])), bool(affine)


def test_fixture_regenerates_from_its_inputs():
    """the stored per-pixel vectors and sums are what the table gives for the stored image, corners and state"""
    for tag in TAGS:
        pa, c, _ = _patch(tag)
        It, Jt = pa.sample(pa.warp(G[tag + "_p"]), G[tag + "_p"])
        q = M.quantities(pa.I0o, It, pa.J0, Jt, c)
        assert np.array_equal(It, G[tag + "_It"])
        for name in ("df_dIt", "df_dI0", "f", "g_curr", "g_init", "H_self", "H_curr", "H_init"):
            assert np.array_equal(np.asarray(q[name]), G[tag + "_" + name]), (tag, name)
        assert float(G[tag + "_f"]) <= It.size
        for name in ("f", "g_curr", "g_init", "H_self", "H_curr", "H_init"):
            assert 0 <= float(G[tag + "_err_floor_" + name]) < 1e-13, (tag, name)


def test_cases_cover_the_seams():
    shapes = {tuple(int(v) for v in G[t + "_cfg"]) for t in TAGS}
    assert {(50, 50, 0), (37, 23, 0), (7, 5, 1), (40, 40, 1)} <= shapes
    assert any(float(G[t + "_k"]) == 0.03 for t in TAGS)
    assert any((G[t + "_It"] == 128.0).sum() > 0 for t in TAGS), "no case samples the border value"
    assert all(np.abs(G[t + "_p"]).max() > 0 for t in TAGS)
    loops = [t for t in TAGS if t + "_eps" in G.files]
    assert sum(tuple(G[t + "_cfg"]) == (50, 50, 0) for t in loops) >= 3
    assert len({int(G[t + "_esm_ds_loop_n"]) for t in loops if tuple(G[t + "_cfg"]) == (50, 50, 0)}) > 1


@pytest.mark.parametrize("tag", TAGS)
def test_df_dIt_is_the_derivative_of_f(tag):
    """central difference of f in It, pixel by pixel (f is a plain sum over pixels), to 1e-6 relative"""
    pa, c, _ = _patch(tag)
    a, b = pa.I0o, G[tag + "_It"]
    h = 1e-4 * np.maximum(np.abs(b), 1.0)
    fd = (M.per_pixel(a, b + h, c)[0] - M.per_pixel(a, b - h, c)[0]) / (2 * h)
    dft = G[tag + "_df_dIt"]
    assert np.abs(fd - dft).max() <= 1e-6 * np.abs(dft).max()


@pytest.mark.parametrize("tag", TAGS)
def test_df_dI0_is_the_references_expression(tag):
    pa, c, _ = _patch(tag)
    a, b = pa.I0o, G[tag + "_It"]
    den = a * a + b * b + c
    df0 = G[tag + "_df_dI0"]
    assert np.array_equal(df0, 2 * (b * (b * b - a * a) + c * (b - 2 * a)) / (den * den))
    # the derivative of fv in a has c (b - a): the stored vector is that minus 2 c a / den^2, exactly (up to the rounding of two forms)
    true = 2 * (b * (b * b - a * a) + c * (b - a)) / (den * den)
    gap = -2 * c * a / (den * den)
    assert np.abs((df0 - true) - gap).max() <= 8 * np.finfo(float).eps * np.abs(true).max()
    assert np.abs(gap).max() > 0
    h = 1e-4 * np.maximum(np.abs(a), 1.0)
    fd = (M.per_pixel(a + h, b, c)[0] - M.per_pixel(a - h, b, c)[0]) / (2 * h)
    assert np.abs(fd - true).max() <= 1e-6 * np.abs(true).max()


@pytest.mark.parametrize("tag", TAGS)
def test_hessians_at_the_template(tag):
    """at It = I0: fv = 1 and df_dIt = 2 a (1 - fv) / den = 0, so w_curr = -2 / den = w_self and H_curr == H_self (to rounding); that
    Hessian over J0 is the fixture's H0"""
    pa, c, _ = _patch(tag)
    a = pa.I0o
    fv, dft, _, ws, wc, _ = M.per_pixel(a, a, c)
    assert np.allclose(fv, 1.0, rtol=0, atol=4e-16)
    assert np.array_equal(ws, -2 / (2 * a * a + c))
    # df_dIt(a, a) = 2 a (1 - fv) / den vanishes with 1 - fv, so w_curr = w_self to rounding
    assert np.abs(wc - ws).max() <= 64 * np.finfo(float).eps * np.abs(ws).max()
    H_self, H_curr = M.wgram(ws, pa.J0), M.wgram(wc, pa.J0)
    assert np.abs(H_curr - H_self).max() <= 1e-12 * np.abs(H_self).max()
    assert np.array_equal(H_self, G[tag + "_H0"])


@pytest.mark.parametrize("tag", TAGS)
def test_self_hessian_negative_definite(tag):
    for name in ("H_self", "H0"):
        H = G[tag + "_" + name]
        assert np.allclose(H, H.T, rtol=1e-12, atol=0)
        assert np.linalg.eigvalsh(H).max() < 0, (tag, name)


def test_likelihood_is_one_at_the_template():
    for tag in TAGS:
        pa, c, _ = _patch(tag)
        f = M.per_pixel(pa.I0o, pa.I0o, c)[0].sum()
        assert np.exp(1.0 * (f - pa.I0o.size)) == pytest.approx(1.0, abs=1e-12)
        assert np.exp(1.0 * (float(G[tag + "_f"]) - pa.I0o.size)) < 1.0


def test_k_changes_f():
    assert float(G["a40_f"]) != float(G["a40k3_f"])
    assert np.array_equal(G["a40_It"], G["a40k3_It"]) and np.array_equal(G["a40_p"], G["a40k3_p"])


def test_spss_abi_symbols_exported():
    from mtf_amd import _lib as L
    assert L.AM_SPSS == 7
    assert "mtfhip_batch_set_spss" in L.SYMBOLS
    lib = ctypes.CDLL(L.LIB_PATH)
    for s in L.SYMBOLS:
        assert hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "mtfhip.h")).read()
    assert "MTFHIP_AM_SPSS = 7" in hdr
    assert "MTFHIP_BUF_COUNT = 22" in hdr
    import mtf_amd
    assert mtf_amd.AM_SPSS == 7 and hasattr(mtf_amd.Batch, "set_spss")


def test_python_trackers_refuse_spss_before_any_device_call():
    """GridTracker, ParticleFilter, NNDataset and NNTracker raise before they touch their context (None here)"""
    import mtf_amd
    from mtf_amd import sm
    for cls in (sm.GridTracker, sm.ParticleFilter, sm.NNDataset, sm.NNTracker):
        with pytest.raises(mtf_amd.FunctionNotImplemented):
            cls(None, am=mtf_amd.AM_SPSS)


# mtfhip_patch_desc as it was before SPSS (x86-64 / SysV): the struct is unchanged
DESC_LAYOUT = dict(size=72, am=0, ssm=4, resx=8, resy=12, grad_eps=16, likelihood_alpha=24, mi_n_bins=32, mi_pre_seed=40,
                   mi_partition_of_unity=48, hess_eps=56, n_channels=64)


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_patch_desc_layout_from_header_spss(tmp_path):
    """the header itself, compiled: sizeof / offsetof of every field, the new enumerator and the new setter's type"""
    fields = [k for k in DESC_LAYOUT if k != "size"]
    body = "".join('printf("%%s %%zu\\n", "%s", offsetof(mtfhip_patch_desc, %s));' % (f, f) for f in fields)
    src = tmp_path / "desc.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mtfhip.h"\nint main(void){printf("size %%zu\\n", sizeof(mtfhip_patch_desc));%s'
                   'int (*s)(mtfhip_batch *, double) = mtfhip_batch_set_spss; (void)s; return MTFHIP_AM_SPSS == 7 ? 0 : 1;}\n' % body)
    subprocess.check_call(["cc", "-c", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "desc.o"), str(src)])
    src2 = tmp_path / "desc2.c"
    src2.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mtfhip.h"\nint main(void){printf("size %%zu\\n", sizeof(mtfhip_patch_desc));%s'
                    'return MTFHIP_AM_SPSS == 7 ? 0 : 1;}\n' % body)
    exe = tmp_path / "desc2"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src2)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    got = {out[i]: int(out[i + 1]) for i in range(0, len(out), 2)}
    assert got == DESC_LAYOUT


PROGRAM = r"""
#include "mtfhip_fused_dispatch.h"
#include <cstdio>
using namespace mtfhip;
typedef FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_SPSS> U;
int main() {
	int fails = 0, served = 0, visited = 0;
	for (int route = 0; route < 3; ++route)
	for (int C : {1, 3}) for (int ssm : {MTFHIP_SSM_HOMOGRAPHY, MTFHIP_SSM_AFFINE}) for (int mode = 0; mode < 3; ++mode)
	for (int ch = 0; ch < 2; ++ch) for (int mat = 0; mat < 2; ++mat) for (int fm = 0; fm < 2; ++fm) {
		const FusedKey k = fused_select(route, MTFHIP_AM_SPSS, C, ssm, mode, ch, mat, fm);
		const bool want = route == FUSED_ROUTE_LOOP && C == 1;
		if (k.served != want) { ++fails; std::printf("route %d C %d ssm %d mode %d ch %d mat %d fm %d: served %d\n", route, C, ssm, mode, ch, mat, fm, (int)k.served); }
		if (!k.served) continue;
		++served;
		const bool fast = fm && !mat;
		if (k.am != MTFHIP_AM_SPSS || k.mc || k.ssm != ssm || k.mode != mode || k.mat != (mat != 0) || k.fast != fast ||
			k.chained != (ch || (fast && mode == 2))) { ++fails; std::printf("wrong key\n"); }
		if (grid_regen_kernel(MTFHIP_AM_SPSS, ssm, ch, mode, mat)) { ++fails; std::printf("grid rebuild planned\n"); }
		int calls = 0;
		const bool r = fused_visit<U>(k, [&](auto AM, auto, auto, auto, auto, auto) { ++calls; if (AM() != MTFHIP_AM_SPSS) ++fails; });
		if (!r || calls != 1) { ++fails; std::printf("visit: %d calls\n", calls); }
		visited += calls;
		/* ... and no other unit takes the key */
		if (fused_visit<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>(k, [&](auto, auto, auto, auto, auto, auto) {})) { ++fails; std::printf("an SSD kernel takes an SPSS key\n"); }
	}
	int n = 0;
	for (int i = 0; i < U::count; ++i) n += fused_reachable(U::route, U::key(i));
	std::printf("served %d visited %d instantiations %d\n", served, visited, n);
	return fails ? 1 : 0;
}
"""


@pytest.mark.skipif(shutil.which("c++") is None and shutil.which("g++") is None, reason="no C++ compiler")
def test_fused_select_serves_spss_on_the_loop_route_only(tmp_path):
    src = tmp_path / "sel.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "sel"
    subprocess.check_call([shutil.which("c++") or shutil.which("g++"), "-std=c++17", "-I", CSRC, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    # 2 SSM x 3 MODE x 2 CHAINED x 2 MAT x 2 FAST inputs on the loop route; tolerance ICLK is one kernel for both CHAINED, and FAST
    # with MAT is the replay kernel: 2 SSM x (3 MODE x 2 CHAINED x 2 MAT replay + (2 x 2 + 1) lean tolerance) = 34 kernels
    assert r.stdout.split() == ["served", "48", "visited", "48", "instantiations", "34"]
