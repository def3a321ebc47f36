/*
 * mtfhip_sm_system.h -- the rule that turns one target's reduced accumulator row into a search method's f, g and H (before damping),
 * stated ONCE for the host-side assembly (api_fused.hip: assemble_rows, api_ncc_moments.hip) and the device-side finish
 * (mtfhip_finish_device.h): the accumulator slots, the Hessian source predicates, the SSD-family and SPSS entries, NCC from its raw
 * moments, and the projection of the affine-coordinate system onto a low-order SSM.  Both sides are compiled with -ffp-contract=off, so
 * one expression gives one set of bits: `iterate` followed by a host solve and the device loop are the same method because they call
 * the same functions.  Nothing here needs the HIP runtime; a host compiler takes the header as it stands.
 */
#ifndef MTFHIP_SM_SYSTEM_H
#define MTFHIP_SM_SYSTEM_H

#include <cmath>
#include "../../include/mtfhip.h"

#if defined(__HIPCC__)
#define MTFHIP_HD __host__ __device__ inline __attribute__((always_inline))
#define MTFHIP_LOOP_AS_LOOP _Pragma("unroll 1")
#else
#define MTFHIP_HD inline
#define MTFHIP_LOOP_AS_LOOP
#endif

namespace mtfhip {

/* accumulator slots produced by the reducing kernels, per target */
enum {
	ACC_H = 0,            /* 36: upper triangle of sum J_a J_b, row-major over (a<=b) with S=8 stride */
	ACC_G = 36,           /* 8 : sum v_i * Jrow_i  (v = residual-type vector of the mode) */
	ACC_RR = 44,          /* 1 : sum r^2 */
	ACC_G2 = 45,          /* 8 : second gemv (ESM generic: df_dI0 * J0) */
	ACC_COUNT = 56        /* padded so the halving butterfly divides evenly 3 times */
};
/* partial / reduced row of the fused NCC iteration: raw moments over the pixels of a target (J = the row the Hessian is
 * built from -- Jt, or the mean of J0 and Jt for ESM's Original Hessian; the g-type sums always use Jt and J0 themselves) */
enum {
	NCC_GRAM = 0,         /* 36: sum J_a J_b, upper triangle as ACC_H */
	NCC_SJ = 36,          /* 8 : sum Jt */
	NCC_ITJ = 44,         /* 8 : sum It Jt */
	NCC_I0J = 52,         /* 8 : sum I0 Jt */
	NCC_ITJ0 = 60,        /* 8 : sum It J0 */
	NCC_IT = 68, NCC_IT2 = 69, NCC_I0IT = 70,
	NCC_ACC_COUNT = 72    /* 72 -> 36 -> 18 -> 9 under the halving butterfly */
};
/* the template's constant moments beside an NCC row ([52]: TrackState::ncc_tm, TargetHost::ncc_tm) */
enum { NCC_TM_SJ0 = 0 /* 8: sum J0 */, NCC_TM_I0J0 = 8 /* 8: sum I0 J0 */, NCC_TM_GRAM0 = 16 /* 36: Gram(J0), as ACC_H */, NCC_TM_COUNT = 52 };

/* index of (a, b), a <= b, in the upper-triangle order of the accumulator row (stride 8) */
MTFHIP_HD constexpr int tri8(int a, int b) { return a * 8 - (a * (a - 1)) / 2 + (b - a); }
MTFHIP_HD constexpr int tri8_sym(int r, int c) { return r < c ? tri8(r, c) : tri8(c, r); }

/* ---- where a search method's Hessian comes from (NT/FCLK.cc:260-288, NT/ESM.cc:298-377, NT/ICLK.cc:206-251) ----
 * h_from_acc: every non-constant Hessian type reads the reduced row, ICLK's included, and ESM's SumOfStd arrives summed (MI).
 * spss: the row is an SPSS pass's -- ICLK's Std Hessian is not constant (cmptInitHessian weights J0 J0^T by a function of It,
 * SPSS.cc:160-165) and comes from the row; ESM's SumOfStd is not served from one row (check_sm). */
MTFHIP_HD bool sm_use_h0(const mtfhip_sm_desc &sm, bool h_from_acc, bool spss) {
	return (sm.hess_type == 0) || (!spss && sm.sm == MTFHIP_SM_ICLK && !h_from_acc);
}
MTFHIP_HD bool sm_sum_h0(const mtfhip_sm_desc &sm, bool h_from_acc, bool spss) {
	return (sm.sm == MTFHIP_SM_ESM) && (sm.hess_type == 2 || (sm.hess_type == 4 && !h_from_acc && !spss));
}
/* ESM's Jacobian over an SSD-family row is half the sum the pass accumulates (the mean of the two rows, SSDBase.cc:169-191) */
MTFHIP_HD double sm_gscale(const mtfhip_sm_desc &sm) { return (sm.sm == MTFHIP_SM_ESM) ? 0.5 : 1.0; }

/* ---- the SSD family and SPSS: f, g(s) and H(r, c) of one reduced row ----
 * SSD: ACC_RR = sum r^2, ACC_G = sum r Jrow, ACC_H = Gram(row), whose negative is the Hessian (SSDBase.cc:169-191,287-311).
 * SPSS: ACC_RR = f itself (a sum of scores), ACC_H the WEIGHTED Gram matrix, i.e. the Hessian with its sign, ACC_G = sum df_dIt row and
 * ACC_G2 = sum df_dI0 J0 row, from which the search method's Jacobian is cmptCurrJacobian (FCLK; ESM jac_type Original, over the mean
 * row), cmptInitJacobian (ICLK) or half the difference (ESM DiffOfJacs, AppearanceModel.h:161-164, NT/ESM.cc:309).
 * The *_of forms take the operands as values (finish_track_fast_body holds them in registers), the others read them. */
MTFHIP_HD double ssd_f(bool spss, const double *row) { return spss ? row[ACC_RR] : -row[ACC_RR] / 2; }
MTFHIP_HD double ssd_g_of(const mtfhip_sm_desc &sm, bool spss, double g1, double g2) {
	if (spss) {
		if (sm.sm == MTFHIP_SM_ICLK) return g2;
		if (sm.sm == MTFHIP_SM_ESM && sm.jac_type != 0) return 0.5 * (g1 - g2);
		return g1;
	}
	return sm_gscale(sm) * g1;
}
MTFHIP_HD double ssd_g(const mtfhip_sm_desc &sm, bool spss, const double *row, int s) {
	return ssd_g_of(sm, spss, row[ACC_G + s], row[ACC_G2 + s]);
}
/* hacc: the row's ACC_H entry; h0v: the constant Hessian's */
MTFHIP_HD double ssd_h_of(bool use_h0, bool sum_h0, bool spss, double hacc, double h0v) {
	double v = use_h0 ? h0v : (spss ? hacc : -hacc);
	if (sum_h0) v = (v + h0v) * 0.5;
	return v;
}
/* (the constant Hessian as entry (r, c) of the column-major S x S h0, not from a triangle: MI's initial self Hessian with its
 * second-order part is not symmetric in the homography's last two rows / columns; every other one is, and reads the same numbers) */
MTFHIP_HD double ssd_h(const mtfhip_sm_desc &sm, bool h_from_acc, bool spss, const double *row, const double *h0, int S, int r, int c) {
	return ssd_h_of(sm_use_h0(sm, h_from_acc, spss), sm_sum_h0(sm, h_from_acc, spss), spss, row[ACC_H + tri8_sym(r, c)], h0[c * S + r]);
}

/* ---- NCC on the fused path: everything NCC.cc derives from centred vectors, written in raw moments ----
 * With mt = mean(It), m0 = mean(I0), b = |It - mt|, c = |I0 - m0|, f = a / (b c)  (NCC.cc:124-161) and, for a pixel
 * Jacobian X with column sums sX, Gram(X), sum It X = itX, sum I0 X = i0X:
 *   Jc = (X - mean(X)) / b                       G(X)  = -Jc^T Jc            = -(Gram(X) - sX sX^T / N) / b^2
 *   ut(X) = Jc^T (It - mt) / b = (itX - mt sX) / b^2        u0(X) = Jc^T (I0 - m0) / c = (i0X - m0 sX) / (b c)
 *   df_dIt . X = u0 - f ut   (NCC.cc:196-234, 252-266)       df_dI0 . X = (b / c) (ut - f u0)   (NCC.cc:163-194, 236-250)
 *   cmptCurrHessian = f G - ut u0^T - u0 ut^T + 3 ut ut^T   (NCC.cc:304-335)    cmptInitHessian: ... + 3 u0 u0^T (NCC.cc:282-303)
 *   cmptSelfHessian = G + ut ut^T   (NCC.cc:337-389)
 * (the reference also subtracts the mean of the gradient vectors, which is zero up to rounding because the centred
 * vectors sum to zero; it does not survive into the moments).  Moments of the mean Jacobian (J0 + Jt) / 2 are the means of
 * the moments, except its Gram matrix, which the kernel accumulates itself when hess_mean is set. */
/* the reduced row (NCC_* slots), the template's moments (NCC_TM_*), mean(I0), |I0 - mean| and N, with the scalars of the row */
struct NccSys {
	const double *row, *tm;
	double N, m0, c;
	double mt, b2, b, f;
};
enum { NCC_J0 = 0, NCC_JT = 1, NCC_JM = 2 };          /* `which`: the Jacobian a vector or Hessian is taken over -- J0, Jt, their mean */
enum { NCC_H_INIT = 0, NCC_H_CURR = 1, NCC_H_SELF = 2 };   /* `kind`: cmptInitHessian, cmptCurrHessian, cmptSelfHessian */
MTFHIP_HD NccSys ncc_sys(const double *row, const double *tm, double m0, double c, double N) {
	NccSys q;
	q.row = row; q.tm = tm; q.N = N; q.m0 = m0; q.c = c;
	q.mt = row[NCC_IT] / N;
	q.b2 = row[NCC_IT2] - N * q.mt * q.mt; q.b = sqrt(q.b2);
	q.f = (row[NCC_I0IT] - N * m0 * q.mt) / (q.b * c);
	return q;
}
/* the Gram matrix the row carries is Jt's, or the mean Jacobian's when the pass ran with hess_mean; J0's is the template's */
MTFHIP_HD bool ncc_has_gram(int which, bool hess_mean) { return which == NCC_J0 || (which == NCC_JM) == hess_mean; }
/* one moment of J0 (tm[c0 + s], or the row's sum It J0 for c0 < 0), of Jt (row[ct + s]) or of their mean */
MTFHIP_HD double ncc_mom(const NccSys &q, int which, int c0, int ct, int s) {
	const double v0 = c0 >= 0 ? q.tm[c0 + s] : q.row[NCC_ITJ0 + s], vt = q.row[ct + s];
	return which == NCC_J0 ? v0 : (which == NCC_JT ? vt : (v0 + vt) / 2);
}
MTFHIP_HD double ncc_sj(const NccSys &q, int which, int s) { return ncc_mom(q, which, NCC_TM_SJ0, NCC_SJ, s); }
MTFHIP_HD double ncc_ut(const NccSys &q, int which, int s) { return (ncc_mom(q, which, -1, NCC_ITJ, s) - q.mt * ncc_sj(q, which, s)) / q.b2; }
MTFHIP_HD double ncc_u0(const NccSys &q, int which, int s) { return (ncc_mom(q, which, NCC_TM_I0J0, NCC_I0J, s) - q.m0 * ncc_sj(q, which, s)) / (q.b * q.c); }
MTFHIP_HD double ncc_curr_jac(const NccSys &q, int which, int s) { return ncc_u0(q, which, s) - q.f * ncc_ut(q, which, s); }
MTFHIP_HD double ncc_init_jac(const NccSys &q, int which, int s) { return (q.b / q.c) * (ncc_ut(q, which, s) - q.f * ncc_u0(q, which, s)); }
/* entry (r, c) of a Hessian; kk = tri8_sym(r, c) */
MTFHIP_HD double ncc_hess(const NccSys &q, int kind, int which, int r, int c, int kk) {
	const double gram = which == NCC_J0 ? q.tm[NCC_TM_GRAM0 + kk] : q.row[NCC_GRAM + kk];
	const double G = -(gram - ncc_sj(q, which, r) * ncc_sj(q, which, c) / q.N) / q.b2;
	const double utr = ncc_ut(q, which, r), utc = ncc_ut(q, which, c);
	if (kind == NCC_H_SELF) return G + utr * utc;
	const double u0r = ncc_u0(q, which, r), u0c = ncc_u0(q, which, c);
	return q.f * G - utr * u0c - u0r * utc + 3 * (kind == NCC_H_CURR ? utr * utc : u0r * u0c);
}
MTFHIP_HD double ncc_hess(const NccSys &q, int kind, int which, int r, int c) { return ncc_hess(q, kind, which, r, c, tri8_sym(r, c)); }
/* the search method's Jacobian: FCLK cmptCurrJacobian(Jt), ICLK cmptInitJacobian(J0), ESM Original cmptCurrJacobian(mean),
 * ESM DiffOfJacs half of (df_dIt . Jt) - (df_dI0 . J0) (NCC.cc:268-280) */
MTFHIP_HD double ncc_g(const mtfhip_sm_desc &sm, const NccSys &q, int s) {
	if (sm.sm == MTFHIP_SM_FCLK) return ncc_curr_jac(q, NCC_JT, s);
	if (sm.sm == MTFHIP_SM_ICLK) return ncc_init_jac(q, NCC_J0, s);
	if (sm.jac_type == 0) return ncc_curr_jac(q, NCC_JM, s);
	return 0.5 * (ncc_curr_jac(q, NCC_JT, s) - ncc_init_jac(q, NCC_J0, s));
}
/* ... and the Jacobian whose Gram matrix its Hessian needs from the row (ncc_has_gram), NCC_J0 for none */
MTFHIP_HD int ncc_h_which(const mtfhip_sm_desc &sm) {
	if (sm.hess_type == 0 || sm.sm == MTFHIP_SM_ICLK) return NCC_J0;
	return (sm.sm == MTFHIP_SM_ESM && sm.hess_type == 3) ? NCC_JM : NCC_JT;
}
/* ... and its Hessian, entry (r, c).  h0v: the constant self Hessian's entry; ex: the second-order term of the entry (sec_ord_hess,
 * NCC.cc:391-410: the weighted pixel-Hessian sums of k_second_order_ssd's NCC form), 0 without */
MTFHIP_HD double ncc_h(const mtfhip_sm_desc &sm, const NccSys &q, double h0v, double ex, int r, int c) {
	const int ht = sm.hess_type, kk = tri8_sym(r, c);
	if (ht == 0) return h0v;
	if (sm.sm == MTFHIP_SM_ICLK) return ncc_hess(q, NCC_H_INIT, NCC_J0, r, c, kk) + ex;   /* Std: cmptInitHessian(J0) */
	if (sm.sm == MTFHIP_SM_FCLK || ht == 1 || ht == 5) return ncc_hess(q, ht == 1 ? NCC_H_SELF : NCC_H_CURR, NCC_JT, r, c, kk) + ex;
	if (ht == 2) return 0.5 * (ncc_hess(q, NCC_H_SELF, NCC_JT, r, c, kk) + h0v);   /* SumOfSelf */
	if (ht == 3) return ncc_hess(q, NCC_H_CURR, NCC_JM, r, c, kk) + ex;   /* Original: cmptCurrHessian(mean) */
	return 0.5 * (ncc_hess(q, NCC_H_INIT, NCC_J0, r, c, kk) + ncc_hess(q, NCC_H_CURR, NCC_JT, r, c, kk)) + ex;   /* SumOfStd */
}

/* ---- the low-order SSMs: J_S = J_aff M with M constant, 6 x SS, at most two +-1 entries per column (Translation.h:45-63,
 * Isometry.cc:115-135,162-185, Similitude.cc:163-210) --
 *   Translation [Ja0, Ja1]    Isometry [Ja0, Ja1, Ja4 - Ja3]    Similitude [Ja0, Ja1, Ja2 + Ja5, Ja4 - Ja3]
 * -- and every g and H above is linear / bilinear in the rows: g_S = g_aff M, H_S = M^T H_aff M, an entry of H_S a sum of at most four
 * of H_aff.  Taken behind the affine entries and in front of the Levenberg-Marquardt scaling (the reference damps the S x S Hessian),
 * the equilibration and the elimination.  col k of M: rows a0 and (a1 >= 0) a1 with sign s1. ---- */
MTFHIP_HD void lowdof_col(int lo_ssm, int k, int &a0, int &a1, double &s1) {
	a0 = k; a1 = -1; s1 = 0.0;
	if (k >= 2) { const bool sum = lo_ssm == MTFHIP_SSM_SIMILITUDE && k == 2; a0 = sum ? 2 : 4; a1 = sum ? 5 : 3; s1 = sum ? 1.0 : -1.0; }
}
/* entry (r, c) of H_S over h(row, col) of the affine system (one copy of the callable's body, not four: the loops stay loops) */
template <class HEntry>
MTFHIP_HD double lowdof_h(int lo_ssm, int r, int c, HEntry &&h) {
	int r0, r1, c0, c1; double sr, sc;
	lowdof_col(lo_ssm, r, r0, r1, sr); lowdof_col(lo_ssm, c, c0, c1, sc);
	double v = 0.0;
	MTFHIP_LOOP_AS_LOOP
	for (int u = 0; u < 2; ++u) {
		const int ru = u ? r1 : r0;
		if (ru < 0) continue;
		MTFHIP_LOOP_AS_LOOP
		for (int w = 0; w < 2; ++w) {
			const int cw = w ? c1 : c0;
			if (cw >= 0) v += (u ? sr : 1.0) * (w ? sc : 1.0) * h(ru, cw);
		}
	}
	return v;
}
template <class GEntry>
MTFHIP_HD double lowdof_g(int lo_ssm, int s, GEntry &&g) {
	int a0, a1; double s1;
	lowdof_col(lo_ssm, s, a0, a1, s1);
	return g(a0) + (a1 >= 0 ? s1 * g(a1) : 0.0);
}

} // namespace mtfhip
#endif
