"""The single statement of a search method's f, g and H (mtf_amd/csrc/mtfhip_sm_system.h), checked without a GPU: a stand-alone host
program includes nothing but that header, is compiled with -ffp-contract=off under the address and undefined-behaviour sanitizers and
runs as a process of its own.  It evaluates f, g and H of reduced rows for every (appearance model, search method, hess_type, jac_type,
S in {8, 6}, low-order SSM) the header serves; the rows are sums over random per-pixel data, and the expected values are a NumPy
restatement of the reference's definitions on the per-pixel vectors themselves -- NCC from its centred, normalised vectors (NCC.cc:124-389),
not from the moment algebra; SSD from the residual (SSDBase.cc:169-311); SPSS from its per-pixel scores, gradients and weights (SPSS.cc);
the low-order models from their explicit per-pixel Jacobians J_S (Translation.h:45-63, Isometry.cc:115-135, Similitude.cc:163-210).

The bound is rounding only.  With the well-conditioned inputs below (400 pixels, b and c of NCC some thousands, f near 0.9) the worst
relative difference (2-norm of the difference over the 2-norm of the expected f, g or H) measured on the build machine is 6.0e-14
(NCC's Hessians, whose moment form cancels Gram(X) against sX sX^T / N); the bound is 8 x that, 4.8e-13."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mtf_amd", "csrc")
MEASURED, BOUND = 6.0e-14, 4.8e-13

ESM, FCLK, ICLK = 0, 1, 2
SSD, NCC, SPSS, FROM_ACC = 0, 1, 7, 100      # FROM_ACC: an SSD-family row with TrackState::h_from_acc (what MI's finish asks for)
SIM, ISO, TRA = 2, 3, 4
ACC_H, ACC_G, ACC_RR, ACC_G2 = 0, 36, 44, 45
NCC_GRAM, NCC_SJ, NCC_ITJ, NCC_I0J, NCC_ITJ0, NCC_IT, NCC_IT2, NCC_I0IT = 0, 36, 44, 52, 60, 68, 69, 70
REC_OUT = 1 + 8 + 64 + 1 + 4
EX = 1.5      # a second-order addend handed to ncc_h

PROGRAM = r"""
#include "mtfhip_sm_system.h"
#include <cstdio>
#include <vector>
using namespace mtfhip;

/* record: am sm hess_type jac_type S lo N m0 c | row[72] | h0[64] | tm[52]  ->  f | g[8] | H[64] (column-major, stride S or SS) | reads out of range |
 * NCC: ncc_h_which | ncc_has_gram of it under the pass's hess_mean | under the other | H(0, 1) with a second-order addend 1.5 */
int main(int argc, char **argv) {
	if (argc != 3) return 2;
	FILE *fi = std::fopen(argv[1], "rb"), *fo = std::fopen(argv[2], "wb");
	if (!fi || !fo) return 2;
	std::vector<double> in(9 + 72 + 64 + 52);
	while (std::fread(in.data(), sizeof(double), in.size(), fi) == in.size()) {
		const int am = (int)in[0], S = (int)in[4], lo = (int)in[5];
		mtfhip_sm_desc sm = mtfhip_sm_desc();
		sm.sm = (int)in[1]; sm.hess_type = (int)in[2]; sm.jac_type = (int)in[3];
		const double *row = &in[9], *h0 = &in[9 + 72], *tm = &in[9 + 72 + 64];
		const bool ncc = am == 1, spss = am == 7, from_acc = am == 100;
		NccSys q = NccSys();
		if (ncc) q = ncc_sys(row, tm, in[7], in[8], in[6]);
		double out[1 + 8 + 64 + 1 + 4] = {0};
		int oob = 0;
		auto g_aff = [&](int s) { if (s < 0 || s >= S) ++oob; return ncc ? ncc_g(sm, q, s) : ssd_g(sm, spss, row, s); };
		auto h_aff = [&](int r, int c) {
			if (r < 0 || r >= S || c < 0 || c >= S) ++oob;
			return ncc ? ncc_h(sm, q, h0[(r < c ? c : r) * S + (r < c ? r : c)], 0.0, r, c) : ssd_h(sm, from_acc, spss, row, h0, S, r, c);
		};
		out[0] = ncc ? q.f : ssd_f(spss, row);
		const int SS = lo == 2 ? 4 : (lo == 3 ? 3 : (lo == 4 ? 2 : S));
		for (int c = 0; c < SS; ++c) {
			out[1 + c] = lo ? lowdof_g(lo, c, g_aff) : g_aff(c);
			for (int r = 0; r < SS; ++r) out[9 + c * SS + r] = lo ? lowdof_h(lo, r, c, h_aff) : h_aff(r, c);
		}
		out[73] = (double)oob;
		if (ncc) {
			const bool hess_mean = sm.sm == MTFHIP_SM_ESM && sm.hess_type == 3;   /* (what fused_args asks of the pass) */
			out[74] = ncc_h_which(sm);
			out[75] = ncc_has_gram(ncc_h_which(sm), hess_mean);
			out[76] = ncc_has_gram(ncc_h_which(sm), !hess_mean);
			out[77] = ncc_h(sm, q, h0[1 * S + 0], 1.5, 0, 1);
		}
		std::fwrite(out, sizeof(double), 78, fo);
	}
	std::fclose(fi);
	return std::fclose(fo) ? 2 : 0;
}
"""


def variants(am, sm):
    if am == FROM_ACC:
        return {ESM: [(2, 1), (4, 1)], FCLK: [(1, 1)], ICLK: [(0, 1), (2, 1)]}[sm]
    out = []
    for h in range(6 if sm == ESM else 3):
        if (sm == ICLK and h == 1) or (am == SPSS and sm == ESM and h == 4):
            continue
        out += [(h, j) for j in ((0, 1) if sm == ESM else (1,))]
    return out


def tri(G, S):
    """upper triangle of an S x S matrix in the accumulator row's order (stride 8); entries of rows / columns >= S: NaN"""
    out = np.full(36, np.nan)
    k = 0
    for a in range(8):
        for c in range(a, 8):
            if c < S:
                out[k] = G[a, c]
            k += 1
    return out


class Pixels:
    """random per-pixel data of one target and the reference's definitions on it"""

    def __init__(self, rng, S, n=400):
        self.S, self.n = S, n
        x = np.linspace(0, 6, n)
        self.I0 = 128 + 60 * np.sin(x * 1.7 + rng.uniform(0, 6)) + 30 * rng.standard_normal(n)
        self.It = 20 + 0.8 * self.I0 + 12 * rng.standard_normal(n)
        self.J0 = rng.standard_normal((n, S)) * rng.uniform(1, 40, S) + rng.uniform(-5, 5, S)
        self.Jt = self.J0 + 0.2 * rng.standard_normal((n, S)) * rng.uniform(1, 40, S)
        self.spss_c = (0.01 * 255.0) ** 2

    # ---- NCC.cc:124-389 on the centred, normalised vectors
    def ncc(self, It=None):
        I0, It = self.I0, self.It if It is None else It
        I0c, Itc = I0 - I0.mean(), It - It.mean()
        c, b = np.linalg.norm(I0c), np.linalg.norm(Itc)
        I0n, Itn = I0c / c, Itc / b
        f = I0n @ Itn
        return dict(f=f, b=b, c=c, I0n=I0n, Itn=Itn, df_dIt=(I0n - f * Itn) / b, df_dI0=(Itn - f * I0n) / c)

    def ncc_hess(self, kind, X, It=None):
        q = self.ncc(It)
        Jc = (X - X.mean(axis=0)) / q["b"]
        G, ut, u0 = -Jc.T @ Jc, Jc.T @ q["Itn"], Jc.T @ q["I0n"]
        if kind == "self":
            return G + np.outer(ut, ut)
        last = np.outer(ut, ut) if kind == "curr" else np.outer(u0, u0)
        return q["f"] * G - np.outer(ut, u0) - np.outer(u0, ut) + 3 * last

    # ---- SPSS.cc:113-230
    def spss(self, It=None):
        I0, It, c = self.I0, self.It if It is None else It, self.spss_c
        den = I0 * I0 + It * It + c
        fv = (2 * I0 * It + c) / den
        df_dIt = 2 * (I0 - fv * It) / den
        df_dI0 = 2 * (It * (It * It - I0 * I0) + c * (It - 2 * I0)) / (den * den)
        return dict(f=fv.sum(), df_dIt=df_dIt, df_dI0=df_dI0, w_init=-2 * (fv + I0 * df_dI0) / den, w_curr=-2 * (fv + 3 * df_dIt * It) / den,
                    w_self=-2 / (2 * It * It + c))

    def record(self, am, sm, ht, jt, J0=None, Jt=None):
        """(row[72], h0[64], tm[52], m0, c) as the pass and the template initialisation leave them, and the expected (f, g, H), over the
        Jacobians given (default: the target's own S columns)"""
        J0 = self.J0 if J0 is None else J0
        Jt = self.Jt if Jt is None else Jt
        S = J0.shape[1]
        I0, It, Jm = self.I0, self.It, (J0 + Jt) / 2
        esm, fclk, iclk = sm == ESM, sm == FCLK, sm == ICLK
        row, tm, m0, c = np.full(72, np.nan), np.full(52, np.nan), 0.0, 1.0
        if am == NCC:
            q = self.ncc()
            Jh = Jm if (esm and ht == 3) else Jt
            row[NCC_GRAM:36] = tri(Jh.T @ Jh, S)
            row[NCC_SJ:NCC_SJ + S], row[NCC_ITJ:NCC_ITJ + S], row[NCC_I0J:NCC_I0J + S] = Jt.sum(axis=0), It @ Jt, I0 @ Jt
            row[NCC_ITJ0:NCC_ITJ0 + S] = It @ J0
            row[NCC_IT], row[NCC_IT2], row[NCC_I0IT] = It.sum(), It @ It, I0 @ It
            tm[0:S], tm[8:8 + S], tm[16:52] = J0.sum(axis=0), I0 @ J0, tri(J0.T @ J0, S)
            m0, c = I0.mean(), q["c"]
            h0 = self.ncc_hess("self", J0, It=I0)
            f = q["f"]
            if fclk:
                g = q["df_dIt"] @ Jt
            elif iclk:
                g = q["df_dI0"] @ J0
            else:
                g = q["df_dIt"] @ Jm if jt == 0 else 0.5 * (q["df_dIt"] @ Jt - q["df_dI0"] @ J0)
            if ht == 0:
                H = h0
            elif iclk:
                H = self.ncc_hess("init", J0)
            elif fclk:
                H = self.ncc_hess("self" if ht == 1 else "curr", Jt)
            else:
                H = {1: lambda: self.ncc_hess("self", Jt), 2: lambda: 0.5 * (self.ncc_hess("self", Jt) + h0),
                     3: lambda: self.ncc_hess("curr", Jm), 4: lambda: 0.5 * (self.ncc_hess("init", J0) + self.ncc_hess("curr", Jt)),
                     5: lambda: self.ncc_hess("curr", Jt)}[ht]()
        elif am == SPSS:
            p, p0 = self.spss(), self.spss(It=I0)
            h0 = (J0 * p0["w_self"][:, None]).T @ J0
            Jg = Jm if (esm and jt == 0) else Jt
            if iclk:
                Hrow = (J0 * p["w_init"][:, None]).T @ J0
            elif fclk:
                Hrow = (Jt * p["w_curr" if ht == 2 else "w_self"][:, None]).T @ Jt
            else:
                Jh = Jm if ht == 3 else Jt
                Hrow = (Jh * p["w_curr" if ht >= 3 else "w_self"][:, None]).T @ Jh
            row[ACC_H:36], row[ACC_RR] = tri(Hrow, S), p["f"]
            row[ACC_G:ACC_G + S], row[ACC_G2:ACC_G2 + S] = p["df_dIt"] @ Jg, p["df_dI0"] @ J0
            f = p["f"]
            g = p["df_dI0"] @ J0 if iclk else (0.5 * (p["df_dIt"] @ Jt - p["df_dI0"] @ J0) if (esm and jt != 0) else p["df_dIt"] @ Jg)
            H = h0 if ht == 0 else (0.5 * (Hrow + h0) if (esm and ht == 2) else Hrow)
        else:
            # SSD (SSDBase.cc:169-311): df_dIt = I0 - It, df_dI0 = It - I0, every Hessian the negated Gram matrix of its row
            r = It - I0
            h0 = -J0.T @ J0
            Jh = Jm if (esm and ht == 3) else Jt
            row[ACC_H:36], row[ACC_RR] = tri(Jh.T @ Jh, S), r @ r
            row[ACC_G:ACC_G + S] = (-r) @ Jt if fclk else ((-r) @ (J0 + Jt) if esm else r @ J0)
            row[ACC_G2:ACC_G2 + 8] = np.nan
            f = -0.5 * (r @ r)
            g = (-r) @ Jt if fclk else ((-r) @ Jm if esm else r @ J0)
            if am == FROM_ACC:
                # MI's finish: every non-constant type reads the row as it stands, ICLK's included; SumOfStd arrives summed
                H = h0 if ht == 0 else (0.5 * (-Jh.T @ Jh + h0) if (esm and ht == 2) else -Jh.T @ Jh)
            elif ht == 0 or iclk:
                H = h0
            elif esm and ht in (2, 4):
                H = 0.5 * (-Jt.T @ Jt + h0)
            else:
                H = -Jh.T @ Jh
        h0p = np.full(64, np.nan)
        h0p[:S * S] = h0.T.reshape(-1)      # column-major S x S
        return (row, h0p, tm, m0, c), (f, g, H)


def lowdof_columns(lo, Ja):
    """J_S = J_aff M, written out per pixel"""
    cols = {TRA: [Ja[:, 0], Ja[:, 1]], ISO: [Ja[:, 0], Ja[:, 1], Ja[:, 4] - Ja[:, 3]],
            SIM: [Ja[:, 0], Ja[:, 1], Ja[:, 2] + Ja[:, 5], Ja[:, 4] - Ja[:, 3]]}[lo]
    return np.stack(cols, axis=1)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("sm_system")
    src, exe, fin, fout = str(d / "t.cpp"), str(d / "t"), str(d / "in.bin"), str(d / "out.bin")
    open(src, "w").write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, src, "-o", exe], check=True)
    rng = np.random.default_rng(20261019)
    recs, expect = [], []
    for S in (8, 6):
        px = Pixels(rng, S)
        for am in (SSD, NCC, SPSS, FROM_ACC):
            for sm in (ESM, FCLK, ICLK):
                for ht, jt in variants(am, sm):
                    for lo in ((0,) if S == 8 else (0, SIM, ISO, TRA)):
                        (row, h0, tm, m0, c), (f, g, H) = px.record(am, sm, ht, jt)
                        if lo:   # expected: the same definitions over the model's own per-pixel Jacobians
                            _, (f, g, H) = px.record(am, sm, ht, jt, lowdof_columns(lo, px.J0), lowdof_columns(lo, px.Jt))
                        recs.append(np.concatenate([[am, sm, ht, jt, S, lo, px.n, m0, c], row, h0, tm]))
                        expect.append(dict(am=am, sm=sm, ht=ht, jt=jt, S=S, lo=lo, f=f, g=g, H=H))
    np.asarray(recs, dtype=np.float64).tofile(fin)
    r = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    out = np.fromfile(fout).reshape(len(recs), REC_OUT)
    return expect, out


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


def test_f_g_H_against_the_per_pixel_definitions(results):
    expect, out = results
    assert len(expect) == 54 + 4 * 54      # S = 8; S = 6 as it stands and projected onto the three low-order models
    worst = 0.0
    for e, o in zip(expect, out):
        SS = len(e["g"])
        f, g, H = o[0], o[1:1 + SS], o[9:9 + SS * SS].reshape(SS, SS).T
        what = "am %(am)d sm %(sm)d hess_type %(ht)d jac_type %(jt)d S %(S)d lo %(lo)d" % e
        assert np.all(np.isfinite(o)), what      # (a NaN is a slot of a row / column >= S that was read)
        errs = (abs(f - e["f"]) / abs(e["f"]), _rel(g, e["g"]), _rel(H, e["H"]))
        worst = max(worst, *errs)
        assert max(errs) < BOUND, (what, errs)
    print("worst relative difference %.2e (measured %.1e, bound %.1e)" % (worst, MEASURED, BOUND), file=sys.stderr)


def test_rows_and_columns_beyond_S_are_never_read(results):
    """the program's entry callables count every (r, c) or s outside [0, S) the projections ask for; the slots of the rows, of h0 and of
    the template moments that belong to rows / columns >= S hold NaN and none reaches an output"""
    expect, out = results
    assert np.all(out[:, 73] == 0) and np.all(np.isfinite(out))
    for e, o in zip(expect, out):
        SS = len(e["g"])
        assert np.all(o[1 + SS:9] == 0) and np.all(o[9 + SS * SS:73] == 0)


def test_projected_H_of_a_symmetric_affine_H_is_symmetric(results):
    """every H_aff here is symmetric; H_S(r, c) and H_S(c, r) add the same (at most four) products in another order, so they agree to the
    rounding of that sum"""
    expect, out = results
    n = 0
    for e, o in zip(expect, out):
        if not e["lo"]:
            continue
        SS = len(e["g"])
        H = o[9:9 + SS * SS].reshape(SS, SS).T
        assert np.abs(H - H.T).max() <= 4 * np.finfo(float).eps * 4 * np.abs(e["H"]).max(), e
        n += 1
    assert n == 3 * 54


def test_ncc_gram_source_and_second_order_addend(results):
    """the Jacobian whose Gram matrix an NCC Hessian takes from the row (ncc_h_which): none for InitialSelf and for ICLK, the mean
    Jacobian's for ESM Original, Jt's otherwise; the row has it exactly when the pass ran with the matching hess_mean (ncc_has_gram,
    what the host's refusal tests); and ncc_h adds the second-order term to every type but InitialSelf and SumOfSelf (NCC.cc:391-410
    overrides cmptInit / CurrHessian only)"""
    expect, out = results
    n = 0
    for e, o in zip(expect, out):
        if e["am"] != NCC or e["lo"]:
            continue
        n += 1
        which = 0 if (e["ht"] == 0 or e["sm"] == ICLK) else (2 if (e["sm"] == ESM and e["ht"] == 3) else 1)
        assert (o[74], o[75], o[76]) == (which, 1.0, 1.0 if which == 0 else 0.0), e
        h01 = o[9 + 1 * e["S"] + 0]
        if e["ht"] == 0 or (e["sm"] == ESM and e["ht"] == 2):
            assert o[77] == h01, e
        else:
            assert abs((o[77] - h01) - EX) <= 4 * np.finfo(float).eps * max(abs(h01), EX), e
    assert n == 2 * 17
