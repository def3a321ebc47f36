"""The SSIM appearance model (AM/src/SSIM.cc) without a GPU.  The float64 reference of tests/golden/make_golden11.py, written from the centred
vectors, against the model's own properties (the integer quotient, the asymmetry of the init / curr Hessians, the definite self Hessian,
the likelihood, the constants); the moment algebra of mtf_amd/csrc/mtfhip_sm_system.h (ssim_*) -- a host program over that header alone,
fed the RAW moments an NCC pass would reduce for each stored case -- against the fixture at the replay bounds; and the ABI: the exported
symbol, the unchanged mtfhip_patch_desc, what fused_select serves for am = 8, the Python trackers' refusals.

Bounds of the moment algebra: f 1e-12, H 1e-9, g 1e-10, dp 1e-6 relative, each max(bound, 16 x the fixture's err_floor) (the fixture's
own float64-against-longdouble rounding).  The algebra's figures: f <= 8.6e-15, g <= 3.8e-13, H <= 1.7e-14, dp <= 6.5e-8."""
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
import make_golden11 as M  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "lk_golden11.npz"))
TAGS = [str(t) for t in G["tags"]]
B_F, B_H, B_G, B_DP = 1e-12, 1e-9, 1e-10, 1e-6
NAMES = ("f", "g_curr", "g_init", "g_mean", "H_self", "H_curr", "H_init", "H_mean")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def floor16(tag, name, base):
    return max(base, 16 * float(G[tag + "_err_floor_" + name]))


def model(tag):
    resx, resy, ssm = (int(v) for v in G[tag + "_cfg"])
    mo = M.Model(G["img"].astype(np.float64), resx, resy, ssm, G[tag + "_corners"])
    k1, k2 = (float(v) for v in G[tag + "_k"])
    return mo, M.ssim_c(k1), M.ssim_c(k2)


_cache = {}


def case(tag):
    """(model, c1, c2, It, Jt) of a stored case, sampled once"""
    if tag not in _cache:
        mo, c1, c2 = model(tag)
        It, Jt = mo.sample(mo.warp(G[tag + "_p"]), G[tag + "_p"])
        _cache[tag] = (mo, c1, c2, It, Jt)
    return _cache[tag]


def test_fixture_regenerates_from_its_inputs():
    """the whole file, bit for bit, from the generator's own inputs"""
    out = M.build()
    assert sorted(out) == sorted(G.files)
    for k in G.files:
        assert np.array_equal(np.asarray(out[k]), G[k]), k
    for tag in TAGS:
        for name in NAMES + ("H0",):
            assert 0 <= float(G[tag + "_err_floor_" + name]) < 1e-12, (tag, name)


def test_cases_cover_the_seams():
    shapes = {tuple(int(v) for v in G[t + "_cfg"]) for t in TAGS}
    assert {(7, 9, 0), (25, 25, 1), (16, 16, 0), (50, 50, 0), (20, 20, 2), (20, 20, 3), (20, 20, 4)} <= shapes
    assert sum(tuple(G[t + "_cfg"]) == (50, 50, 0) for t in TAGS) == 3
    assert any((G[t + "_It"] == 128.0).sum() > 0 for t in TAGS), "no case samples the border value"
    loops = [t for t in TAGS if t + "_eps" in G.files]
    kinds = {int(G[t + "_cfg"][2]) for t in loops}
    assert 0 in kinds and 1 in kinds and kinds & {2, 3, 4}
    # loops are stored per method, where the method is flagged well-conditioned; every method has a case of each kind of model, and the
    # Isometry (whose update goes through cos / sin / atan2) carries ESM's and ICLK's
    for k, m in enumerate(M.LOOPS):
        for t in TAGS:
            assert ((t + "_" + m + "_loop_n") in G.files) == bool(G[t + "_well"][k]), (t, m)
        have = {int(G[t + "_cfg"][2]) for t in loops if G[t + "_well"][k]}
        assert 0 in have and 1 in have and have & {2, 3, 4}, m
    assert G["iso20_well"].tolist() == [1, 0, 1]
    assert len({int(G[t + "_esm_ds_loop_n"]) for t in loops if tuple(G[t + "_cfg"]) == (50, 50, 0)}) > 1


def test_update_floor_and_the_tolerance_bound():
    """<tag>_dp_jitter: the reference's own updates under a 1e-12 px shift of the corners.  16 x it (tests/test_gpu_ssim.py: dp_bound) stays
    under tolerance arithmetic's 1e-5 for the 50 x 50 cases, Similitude and Translation; it is 1.3e-5 for the 25 x 25 affine and the
    Isometry case, 3.0e-5 for the 16 x 16 homography and 5.6e-3 for the 7 x 9 one"""
    b16 = {t: 16 * float(G[t + "_dp_jitter"]) for t in TAGS}
    assert sorted(t for t in TAGS if b16[t] > 1e-5) == ["a25", "a25k", "h16", "h7x9", "iso20"]
    assert all(b16[t] < 1.4e-5 for t in ("a25", "a25k", "iso20")) and 2e-5 < b16["h16"] < 4e-5 and 1e-3 < b16["h7x9"] < 1e-2


def test_integer_quotient_is_zero_and_matters():
    """(2 / (patch_size - 1)) is 0 for every stored N; writing it 2.0 / (N - 1) moves H_curr by more than 1e-5 of its size"""
    for tag in TAGS:
        N = int(G[tag + "_cfg"][0]) * int(G[tag + "_cfg"][1])
        assert 2 // (N - 1) == 0
        assert rel(G[tag + "_H_curr_fq"], G[tag + "_H_curr"]) > 1e-5, tag
    mo, c1, c2, It, Jt = case("h7x9")
    q, qf = M.quantities(mo.I0, It, mo.J0, Jt, c1, c2), M.quantities(mo.I0, It, mo.J0, Jt, c1, c2, int_quot=False)
    assert np.array_equal(q["H_self"], qf["H_self"]) and not np.array_equal(q["H_init"], qf["H_init"])


def test_init_and_curr_hessians_are_not_symmetric():
    """max |H - H^T| of H_curr and H_init exceeds 1e-5 of max |H| in a stored case of every method's kind, and every stored dp solves the
    matrix as it stands, not a symmetrised one"""
    for name in ("H_curr", "H_init", "H_mean"):
        asym = {t: float(np.abs(G[t + "_" + name] - G[t + "_" + name].T).max() / np.abs(G[t + "_" + name]).max()) for t in TAGS}
        for ssm_kinds in ((0,), (1,), (2, 3, 4)):
            assert max(v for t, v in asym.items() if int(G[t + "_cfg"][2]) in ssm_kinds) > 1e-5, (name, ssm_kinds)
    tag = "a25"
    mo, c1, c2, It, Jt = case(tag)
    q = M.quantities(mo.I0, It, mo.J0, Jt, c1, c2)
    g, H = M.g_and_H(q, G[tag + "_H0"], "fclk_std")
    assert np.array_equal(-np.linalg.solve(H, g), G[tag + "_fclk_std_dp"])
    assert rel(-np.linalg.solve(0.5 * (H + H.T), g), G[tag + "_fclk_std_dp"]) > 1e-6


@pytest.mark.parametrize("tag", TAGS)
def test_self_hessian_symmetric_negative_definite(tag):
    for name in ("H_self", "H0"):
        H = G[tag + "_" + name]
        assert np.allclose(H, H.T, rtol=1e-12, atol=0)
        assert np.linalg.eigvalsh(0.5 * (H + H.T)).max() < 0, (tag, name)


def test_likelihood_is_one_at_the_template():
    for tag in TAGS:
        mo, c1, c2, _, _ = case(tag)
        f = M.scalars(mo.I0, mo.I0, c1, c2)["f"]
        assert f == pytest.approx(1.0, abs=1e-14)
        assert M.likelihood(f) == pytest.approx(1.0, abs=1e-12)
        assert M.likelihood(float(G[tag + "_f"])) < 1.0


def test_constants_change_f():
    assert float(G["a25_f"]) != float(G["a25k_f"])
    assert np.array_equal(G["a25_It"], G["a25k_It"]) and np.array_equal(G["a25_p"], G["a25k_p"])
    assert G["a25_k"].tolist() == [M.K1_DEFAULT, M.K2_DEFAULT] and G["a25k_k"].tolist() != G["a25_k"].tolist()


def test_gradient_is_the_references_not_the_derivative():
    """the analytic gradient carries N where the derivative of f has N - 1: close to a central difference of f, not equal to it"""
    mo, c1, c2, It, Jt = case("a25")
    s = M.scalars(mo.I0, It, c1, c2)
    rng = np.random.default_rng(3)
    v = rng.standard_normal(It.size)
    h = 1e-4
    fd = (M.scalars(mo.I0, It + h * v, c1, c2)["f"] - M.scalars(mo.I0, It - h * v, c1, c2)["f"]) / (2 * h)
    an = float(s["df_dIt"] @ v)
    assert abs(fd - an) < 1e-2 * abs(an) and abs(fd - an) > 1e-7 * abs(an)


# ------------------------------------------------------------------ the moment algebra of mtfhip_sm_system.h
REC_IN = 8 + 72 + 72 + 52
REC_OUT = 1 + 3 * 8 + 5 * 64 + 8 * (8 + 64)
PROGRAM = r"""
#include "mtfhip_sm_system.h"
#include <cstdio>
#include <vector>
using namespace mtfhip;
/* record: S lo N m0 ss0 c1 c2 0 | row[72] (Gram of Jt) | row[72] (Gram of the mean Jacobian) | tm[52]
 * -> f | curr_jac(Jt) init_jac(J0) curr_jac(Jm) | H_self(Jt) H_curr(Jt) H_init(J0) H_curr(Jm) H0 (column-major, stride SS) | per method g[8], H[64] */
static const int METHODS[8][3] = {{0, 1, 2}, {0, 0, 3}, {0, 1, 4}, {0, 1, 5}, {1, 1, 1}, {1, 1, 2}, {2, 1, 0}, {2, 1, 2}};
int main(int argc, char **argv) {
	if (argc != 3) return 2;
	FILE *fi = std::fopen(argv[1], "rb"), *fo = std::fopen(argv[2], "wb");
	if (!fi || !fo) return 2;
	std::vector<double> in(8 + 72 + 72 + 52);
	while (std::fread(in.data(), sizeof(double), in.size(), fi) == in.size()) {
		const int S = (int)in[0], lo = (int)in[1];
		const double *row = &in[8], *rowm = &in[80], *tm = &in[152];
		const SsimSys q = ssim_sys(row, tm, in[3], in[4], in[2], in[5], in[6]), qm = ssim_sys(rowm, tm, in[3], in[4], in[2], in[5], in[6]);
		const SsimSys q0 = ssim_sys_template(tm, in[3], in[4], in[2], in[5], in[6]);
		const int SS = lo == 2 ? 4 : (lo == 3 ? 3 : (lo == 4 ? 2 : S));
		std::vector<double> out(1 + 3 * 8 + 5 * 64 + 8 * (8 + 64), 0.0);
		int oob = 0;
		auto G = [&](auto g, int s) { auto ge = [&](int a) { if (a < 0 || a >= S) ++oob; return g(a); }; return lo ? lowdof_g(lo, s, ge) : ge(s); };
		auto H = [&](auto h, int r, int c) { auto he = [&](int a, int b) { if (a < 0 || a >= S || b < 0 || b >= S) ++oob; return h(a, b); }; return lo ? lowdof_h(lo, r, c, he) : he(r, c); };
		auto h0 = [&](int r, int c) { return ssim_hess(q0, NCC_H_SELF, NCC_J0, r, c); };
		out[0] = q.f;
		for (int c = 0; c < SS; ++c) {
			out[1 + c] = G([&](int s) { return ssim_curr_jac(q, NCC_JT, s); }, c);
			out[9 + c] = G([&](int s) { return ssim_init_jac(q, NCC_J0, s); }, c);
			out[17 + c] = G([&](int s) { return ssim_curr_jac(q, NCC_JM, s); }, c);
			for (int r = 0; r < SS; ++r) {
				const int k = c * SS + r;
				out[25 + k] = H([&](int a, int b) { return ssim_hess(q, NCC_H_SELF, NCC_JT, a, b); }, r, c);
				out[25 + 64 + k] = H([&](int a, int b) { return ssim_hess(q, NCC_H_CURR, NCC_JT, a, b); }, r, c);
				out[25 + 128 + k] = H([&](int a, int b) { return ssim_hess(q, NCC_H_INIT, NCC_J0, a, b); }, r, c);
				out[25 + 192 + k] = H([&](int a, int b) { return ssim_hess(qm, NCC_H_CURR, NCC_JM, a, b); }, r, c);
				out[25 + 256 + k] = H(h0, r, c);
			}
		}
		for (int m = 0; m < 8; ++m) {
			mtfhip_sm_desc sm = mtfhip_sm_desc();
			sm.sm = METHODS[m][0]; sm.jac_type = METHODS[m][1]; sm.hess_type = METHODS[m][2];
			const bool hess_mean = sm.sm == MTFHIP_SM_ESM && sm.hess_type == 3;   /* (what fused_args asks of the pass) */
			if (!ncc_has_gram(ncc_h_which(sm), hess_mean)) return 3;
			const SsimSys &qq = hess_mean ? qm : q;
			double *o = &out[25 + 320 + m * 72];
			for (int c = 0; c < SS; ++c) {
				o[c] = G([&](int s) { return ssim_g(sm, qq, s); }, c);
				for (int r = 0; r < SS; ++r) o[8 + c * SS + r] = H([&](int a, int b) { return ssim_h(sm, qq, h0(a, b), a, b); }, r, c);
			}
		}
		if (oob) return 4;
		std::fwrite(out.data(), sizeof(double), out.size(), fo);
	}
	std::fclose(fi);
	return std::fclose(fo) ? 2 : 0;
}
"""


def tri(Gm, S):
    out = np.zeros(36)
    k = 0
    for a in range(8):
        for c in range(a, 8):
            if c < S:
                out[k] = Gm[a, c]
            k += 1
    return out


def pad8(v):
    out = np.zeros(8)
    out[:v.size] = v
    return out


def moment_record(tag):
    """the raw moments an NCC pass reduces for the case (NCC_* / NCC_TM_* slots), over the affine-coordinate rows for a low-order model"""
    mo, c1, c2, It, Jt = case(tag)
    ssm = int(G[tag + "_cfg"][2])
    I0, J0 = mo.I0, mo.J0
    lo = ssm if ssm >= 2 else 0
    if lo:
        J0 = mo.pa.J0_aff
        _, Jt = mo.pa.sample(mo.warp(G[tag + "_p"]), affine_rows=True)
    S, N = J0.shape[1], I0.size
    m0 = I0.sum() / N
    rows = []
    for X in (Jt, (J0 + Jt) / 2):
        rows.append(np.concatenate([tri(X.T @ X, S), pad8(Jt.sum(0)), pad8(It @ Jt), pad8(I0 @ Jt), pad8(It @ J0),
                                    [It.sum(), (It * It).sum(), (I0 * It).sum(), 0.0]]))
    tm = np.concatenate([pad8(J0.sum(0)), pad8(I0 @ J0), tri(J0.T @ J0, S)])
    head = np.array([S, lo, N, m0, ((I0 - m0) ** 2).sum(), c1, c2, 0.0])
    return np.concatenate([head, rows[0], rows[1], tm])


@pytest.fixture(scope="module")
def moment_outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("ssim_sys")
    src, exe, fin, fout = str(d / "t.cpp"), str(d / "t"), str(d / "in.bin"), str(d / "out.bin")
    open(src, "w").write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, src, "-o", exe], check=True)
    recs = np.stack([moment_record(t) for t in TAGS])
    assert recs.shape[1] == REC_IN
    recs.tofile(fin)
    r = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    out = np.fromfile(fout).reshape(len(TAGS), REC_OUT)
    return {t: out[k] for k, t in enumerate(TAGS)}


def test_moment_algebra_matches_the_centred_reference(moment_outputs):
    """ssim_sys / ssim_curr_jac / ssim_init_jac / ssim_hess / ssim_g / ssim_h (and lowdof_g / lowdof_h over them) on the raw moments of every
    stored case against the fixture, which was computed from the centred vectors"""
    worst = dict(f=0.0, g=0.0, H=0.0, dp=0.0)
    for tag in TAGS:
        o = moment_outputs[tag]
        ssm = int(G[tag + "_cfg"][2])
        SS = {0: 8, 1: 6, 2: 4, 3: 3, 4: 2}[ssm]
        e = rel(o[0], float(G[tag + "_f"]))
        worst["f"] = max(worst["f"], e)
        assert e < floor16(tag, "f", B_F), (tag, e)
        for k, name in enumerate(("g_curr", "g_init", "g_mean")):
            e = rel(o[1 + 8 * k:1 + 8 * k + SS], G[tag + "_" + name])
            worst["g"] = max(worst["g"], e)
            assert e < floor16(tag, name, B_G), (tag, name, e)
        for k, name in enumerate(("H_self", "H_curr", "H_init", "H_mean", "H0")):
            Hd = o[25 + 64 * k:25 + 64 * k + SS * SS].reshape(SS, SS).T
            e = rel(Hd, G[tag + "_" + name])
            worst["H"] = max(worst["H"], e)
            assert e < floor16(tag, name, B_H), (tag, name, e)
        q = {n: G[tag + "_" + n] for n in NAMES}
        for m, key in enumerate(M.METHODS):
            oo = o[25 + 320 + 72 * m:25 + 320 + 72 * (m + 1)]
            g, H = oo[:SS], oo[8:8 + SS * SS].reshape(SS, SS).T
            gr, Hr = M.g_and_H(q, G[tag + "_H0"], key)
            eg, eH = rel(g, gr), rel(H, Hr)
            edp = rel(-np.linalg.solve(H, g), G[tag + "_" + key + "_dp"])
            worst["g"], worst["H"], worst["dp"] = max(worst["g"], eg), max(worst["H"], eH), max(worst["dp"], edp)
            assert eg < floor16(tag, key + "_g", B_G) and eH < floor16(tag, key + "_H", B_H) and edp < B_DP, (tag, key, eg, eH, edp)
    print("moment algebra worst:", worst)


# ------------------------------------------------------------------ the ABI and the dispatch table
def test_ssim_abi_symbols_exported():
    from mtf_amd import _lib as L
    assert L.AM_SSIM == 8
    assert "mtfhip_batch_set_ssim" in L.SYMBOLS
    lib = ctypes.CDLL(L.LIB_PATH)
    for s in L.SYMBOLS:
        assert hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "mtfhip.h")).read()
    assert "MTFHIP_AM_SSIM = 8" in hdr
    assert "MTFHIP_BUF_COUNT = 22" in hdr
    import mtf_amd
    assert mtf_amd.AM_SSIM == 8 and hasattr(mtf_amd.Batch, "set_ssim")


def test_python_trackers_refuse_ssim_before_any_device_call():
    """GridTracker, ParticleFilter, NNDataset and NNTracker raise before they touch their context (None here)"""
    import mtf_amd
    from mtf_amd import sm
    for cls in (sm.GridTracker, sm.ParticleFilter, sm.NNDataset, sm.NNTracker):
        with pytest.raises(mtf_amd.FunctionNotImplemented):
            cls(None, am=mtf_amd.AM_SSIM)


# mtfhip_patch_desc as it was before SSIM (x86-64 / SysV): the constants travel through the setter, the struct is unchanged
DESC_LAYOUT = dict(size=72, am=0, ssm=4, resx=8, resy=12, grad_eps=16, likelihood_alpha=24, mi_n_bins=32, mi_pre_seed=40,
                   mi_partition_of_unity=48, hess_eps=56, n_channels=64)


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_patch_desc_layout_from_header_ssim(tmp_path):
    """the header itself, compiled: sizeof / offsetof of every field, the new enumerator and the new setter's type"""
    fields = [k for k in DESC_LAYOUT if k != "size"]
    body = "".join('printf("%%s %%zu\\n", "%s", offsetof(mtfhip_patch_desc, %s));' % (f, f) for f in fields)
    src = tmp_path / "desc.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mtfhip.h"\nint main(void){printf("size %%zu\\n", sizeof(mtfhip_patch_desc));%s'
                   'int (*s)(mtfhip_batch *, double, double) = mtfhip_batch_set_ssim; (void)s; return MTFHIP_AM_SSIM == 8 ? 0 : 1;}\n' % body)
    subprocess.check_call(["cc", "-c", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "desc.o"), str(src)])
    src2 = tmp_path / "desc2.c"
    src2.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mtfhip.h"\nint main(void){printf("size %%zu\\n", sizeof(mtfhip_patch_desc));%s'
                    'return MTFHIP_AM_SSIM == 8 ? 0 : 1;}\n' % body)
    exe = tmp_path / "desc2"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src2)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    got = {out[i]: int(out[i + 1]) for i in range(0, len(out), 2)}
    assert got == DESC_LAYOUT


SELECT_PROGRAM = r"""
#include "mtfhip_fused_dispatch.h"
#include <cstdio>
using namespace mtfhip;
template <class U> static int count() { int n = 0; for (int i = 0; i < U::count; ++i) n += fused_reachable(U::route, U::key(i)); return n; }
int main() {
	int fails = 0, served = 0;
	for (int route = 0; route < 3; ++route)
	for (int C : {1, 3}) for (int ssm : {MTFHIP_SSM_HOMOGRAPHY, MTFHIP_SSM_AFFINE}) for (int mode = 0; mode < 3; ++mode)
	for (int ch = 0; ch < 2; ++ch) for (int mat = 0; mat < 2; ++mat) for (int fm = 0; fm < 2; ++fm) {
		const FusedKey k = fused_select(route, MTFHIP_AM_SSIM, C, ssm, mode, ch, mat, fm);
		const bool want = route == FUSED_ROUTE_LOOP && C == 1;
		if (k.served != want) { ++fails; std::printf("route %d C %d ssm %d mode %d ch %d mat %d fm %d: served %d\n", route, C, ssm, mode, ch, mat, fm, (int)k.served); }
		if (!k.served) continue;
		++served;
		/* the key is NCC's for the same launch, and the unit that holds NCC's kernels takes it */
		if (!(k == fused_select(route, MTFHIP_AM_NCC, C, ssm, mode, ch, mat, fm)) || k.am != MTFHIP_AM_NCC || k.mc) { ++fails; std::printf("not NCC's key\n"); }
		if (grid_regen_kernel(MTFHIP_AM_SSIM, ssm, ch, mode, mat)) { ++fails; std::printf("grid rebuild planned\n"); }
		int calls = 0;
		const bool r = fused_visit<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>(k, [&](auto AM, auto, auto, auto, auto, auto) { ++calls; if (AM() != MTFHIP_AM_NCC) ++fails; });
		if (!r || calls != 1) { ++fails; std::printf("visit: %d calls\n", calls); }
	}
	std::printf("served %d fused %d fused_mc %d fused_rscv %d fused_lrscv %d fused_spss %d step %d persist %d\n", served,
		count<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>(), count<FusedUnit<FUSED_ROUTE_LOOP, true, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>(),
		count<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_RSCV>>(), count<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_LRSCV>>(),
		count<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_SPSS>>(), count<FusedUnit<FUSED_ROUTE_STEP, false, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>(),
		count<FusedUnit<FUSED_ROUTE_PERSIST, false, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>());
	return fails ? 1 : 0;
}
"""


@pytest.mark.skipif(shutil.which("c++") is None and shutil.which("g++") is None, reason="no C++ compiler")
def test_fused_select_maps_ssim_to_ncc_keys_on_the_loop_route_only(tmp_path):
    src = tmp_path / "sel.cpp"
    src.write_text(SELECT_PROGRAM)
    exe = tmp_path / "sel"
    subprocess.check_call([shutil.which("c++") or shutil.which("g++"), "-std=c++17", "-I", CSRC, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    # 48 inputs on the loop route; no unit's count moves (tests/test_fused_dispatch.py: UNIT_KERNELS, and SPSS's 34)
    assert r.stdout.split() == ["served", "48", "fused", "68", "fused_mc", "68", "fused_rscv", "34", "fused_lrscv", "34", "fused_spss", "34",
                                "step", "44", "persist", "44"]


def test_pass_units_hold_no_ssim_kernel():
    """SSIM adds no kernel to the pass units: their sources do not name it"""
    for f in ("mtfhip_fused_device.h", "kernels_fused.hip", "kernels_fused_mc.hip", "kernels_fused_rscv.hip", "kernels_fused_lrscv.hip",
              "kernels_fused_spss.hip", "kernels_step.hip", "kernels_persist.hip"):
        assert "SSIM" not in open(os.path.join(CSRC, f)).read().upper(), f
