/*
 * mtfhip_sm_system.h -- the rule that turns one target's reduced accumulator row into a search method's f, g and H (before damping),
 * stated ONCE for the host-side assembly (api_fused.hip: assemble_rows, api_ncc.hip) and the device-side finish
 * (mtfhip_finish_device.h): the accumulator slots, the Hessian source predicates, the SSD-family and SPSS entries, NCC from its raw
 * moments, SSIM from the same moments, and the projection of the affine-coordinate system onto a low-order SSM.  Both sides are compiled with -ffp-contract=off, so
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

/* ---- SSIM on NCC's moments: everything SSIM.cc derives from its centred vectors is a function of the row an NCC pass reduces ----
 * With N the patch size, m0 / mt the means, x0 = I0 - m0, xt = It - mt, c1 = (255 k1)^2, c2 = (255 k2)^2 (SSIM.cc:36-39, 98-111):
 *   v0 = x0.x0 / (N - 1)   vt = (sum It^2 - N mt^2) / (N - 1)   cross = (sum I0 It - N m0 mt) / (N - 1)
 *   a = 2 mt m0 + c1   b = 2 cross + c2   c = mt^2 + m0^2 + c1   d = vt + v0 + c2   f = a b / (c d)
 * and for a pixel Jacobian X (`which`, as ncc_mom): sX = sum X, p0 = X^T x0 = sum I0 X - m0 sX, pt = X^T xt = sum It X - mt sX, Gram(X).
 * Gradients (SSIM.cc:113-142), mu = 2 / (N c d): df_dIt = mu (a x0 - f c xt) + gs_t, gs_t = 2 (m0 b - mt f d) / (c d (N - 1)), hence
 *   X^T df_dIt = mu (a p0 - f c pt) + gs_t sX          and X^T df_dI0 the same with I0 and It exchanged
 * (the N against N - 1 is the reference's: the vectors are not the derivatives of f, and are kept).  Hessians (SSIM.cc:144-287): every term
 * is Gram(X), sX sX^T or an outer product (X^T u)(X^T v)^T with u, v in span{x0, xt, 1}; the expressions are ssim_hess's, term by term the
 * reference's.  Kept as the reference has them:
 *   - (2 / (patch_size - 1)) at SSIM.cc:169,183,223,237 is an INTEGER quotient (0 for N >= 4): SsimSys::qi; the 2.0 / (patch_size - 1) at
 *     :177,231 is floating point;
 *   - cmptInitHessian and cmptCurrHessian are NOT symmetric (p0 sX^T, pt p0^T): every consumer takes entry (r, c), never a triangle;
 *   - at :168 and :222 the reference multiplies the column X^T gv^T by a COLUMN, which Eigen only evaluates with its assertions compiled out;
 *     the vector is taken as the row that makes the product conform (the outer product every neighbouring term is).
 * Not kept, because it is state and not algebra: cmptSelfHessian overwrites the members c and d until the next updateSimilarity
 * (SSIM.cc:273-274), and initializeSimilarity reads cross_pix_var before it is set (:64, unused before the first update).  Nothing here
 * carries such members: every Hessian is taken with the c and d of the row's own similarity, and after init_template f = 1. */
struct SsimSys {
	const double *row, *tm;
	double N, m0, mt, c1, c2;
	double vt, a, b, c, d, cd, f;       /* SSIM.cc:98-111 */
	double mu, gs_t, gs_0;              /* mult_factor, curr_grad_scal, init_grad_scal (SSIM.cc:113-142) */
	double qi;                          /* (2 / (patch_size - 1)), the integer quotient */
};
/* ss0: sum (I0 - m0)^2 of the template.  row may be NULL for the system AT the template (It = I0: ssim_sys_template) */
MTFHIP_HD SsimSys ssim_sys_of(const double *row, const double *tm, double m0, double ss0, double N, double c1, double c2, double mt, double tt, double cr) {
	SsimSys q;
	q.row = row; q.tm = tm; q.N = N; q.m0 = m0; q.mt = mt; q.c1 = c1; q.c2 = c2;
	const double v0 = ss0 / (N - 1);
	q.vt = tt / (N - 1);
	q.a = 2 * mt * m0 + c1;
	q.b = 2 * (cr / (N - 1)) + c2;
	q.c = mt * mt + m0 * m0 + c1;
	q.d = q.vt + v0 + c2;
	q.cd = q.c * q.d;
	q.f = (q.a * q.b) / q.cd;
	q.mu = 2.0 / (N * q.cd);
	q.gs_t = 2 * (m0 * q.b - mt * q.f * q.d) / (q.cd * (N - 1));
	q.gs_0 = 2 * (mt * q.b - m0 * q.f * q.d) / (q.cd * (N - 1));
	const long long n = (long long)N;
	q.qi = n > 1 ? (double)(2 / (n - 1)) : 0.0;
	return q;
}
MTFHIP_HD SsimSys ssim_sys(const double *row, const double *tm, double m0, double ss0, double N, double c1, double c2) {
	const double mt = row[NCC_IT] / N;
	return ssim_sys_of(row, tm, m0, ss0, N, c1, c2, mt, row[NCC_IT2] - N * mt * mt, row[NCC_I0IT] - N * m0 * mt);
}
/* It = I0: the system init_template leaves (f = 1) and the one the constant self Hessian H0 = cmptSelfHessian(J0) is taken at; only NCC_J0 moments */
MTFHIP_HD SsimSys ssim_sys_template(const double *tm, double m0, double ss0, double N, double c1, double c2) {
	return ssim_sys_of(nullptr, tm, m0, ss0, N, c1, c2, m0, ss0, ss0);
}
/* one moment of J0, Jt or their mean (ncc_mom's scheme over the two arrays themselves) */
MTFHIP_HD double ssim_mom(const SsimSys &q, int which, int c0, int ct, int s) {
	if (which == NCC_J0) return c0 >= 0 ? q.tm[c0 + s] : q.row[NCC_ITJ0 + s];
	const double vt = q.row[ct + s];
	return which == NCC_JT ? vt : ((c0 >= 0 ? q.tm[c0 + s] : q.row[NCC_ITJ0 + s]) + vt) / 2;
}
MTFHIP_HD double ssim_sj(const SsimSys &q, int which, int s) { return ssim_mom(q, which, NCC_TM_SJ0, NCC_SJ, s); }
MTFHIP_HD double ssim_p0(const SsimSys &q, int which, int s) { return ssim_mom(q, which, NCC_TM_I0J0, NCC_I0J, s) - q.m0 * ssim_sj(q, which, s); }
MTFHIP_HD double ssim_pt(const SsimSys &q, int which, int s) { return ssim_mom(q, which, -1, NCC_ITJ, s) - q.mt * ssim_sj(q, which, s); }
/* X^T init_grad_vec^T / X^T curr_grad_vec^T (the gradient without its scalar part) and cmptInitJacobian / cmptCurrJacobian */
MTFHIP_HD double ssim_gv(const SsimSys &q, bool curr, int which, int s) {
	const double po = curr ? ssim_p0(q, which, s) : ssim_pt(q, which, s), pu = curr ? ssim_pt(q, which, s) : ssim_p0(q, which, s);
	return q.mu * (q.a * po - q.f * q.c * pu);
}
MTFHIP_HD double ssim_curr_jac(const SsimSys &q, int which, int s) { return ssim_gv(q, true, which, s) + q.gs_t * ssim_sj(q, which, s); }
MTFHIP_HD double ssim_init_jac(const SsimSys &q, int which, int s) { return ssim_gv(q, false, which, s) + q.gs_0 * ssim_sj(q, which, s); }
/* entry (r, c) of cmptInitHessian / cmptCurrHessian / cmptSelfHessian (kind: NCC_H_*) over the Jacobian `which` */
MTFHIP_HD double ssim_hess(const SsimSys &q, int kind, int which, int r, int c) {
	const int kk = tri8_sym(r, c);
	const double gram = which == NCC_J0 ? q.tm[NCC_TM_GRAM0 + kk] : q.row[NCC_GRAM + kk];
	const double N = q.N, sr = ssim_sj(q, which, r), sc = ssim_sj(q, which, c);
	if (kind == NCC_H_SELF) {   /* SSIM.cc:270-287 */
		const double cs = 2 * (q.mt * q.mt) + q.c1, ds = 2 * q.vt + q.c2, cds = cs * ds;
		const double m1 = 2.0 / (N * cds), m2 = 2.0 / ((N - 1) * cds);
		return cs * m1 * ((1.0 / N) * sr * sc - gram) - (m2 * ds / N) * sr * sc;
	}
	/* SSIM.cc:200-238 (curr; :144-185 init is the same with I0 and It exchanged): `o` the other image's, `u` the image's own the Hessian is taken in */
	const bool curr = kind == NCC_H_CURR;
	const double mo = curr ? q.m0 : q.mt, mu = curr ? q.mt : q.m0, gs = curr ? q.gs_t : q.gs_0;
	const double por = curr ? ssim_p0(q, which, r) : ssim_pt(q, which, r);
	const double pur = curr ? ssim_pt(q, which, r) : ssim_p0(q, which, r), puc = curr ? ssim_pt(q, which, c) : ssim_p0(q, which, c);
	const double gr = curr ? ssim_curr_jac(q, which, r) : ssim_init_jac(q, which, r), gc = curr ? ssim_curr_jac(q, which, c) : ssim_init_jac(q, which, c);
	const double a_diff = 2.0 * mo / N, c_diff = 2.0 * mu / N;
	const double m1 = 2.0 / (N * q.cd), m2 = 2.0 / ((N - 1) * q.cd);
	const double wr = q.qi * pur / q.d + (c_diff / q.c) * sr, wc = q.qi * puc / q.d + (c_diff / q.c) * sc;
	const double ur = m2 * ((2 * mo / (N - 1)) * por - (mu * (q.d * gr + (2.0 / (N - 1)) * q.f * pur) + (q.f * q.d / N) * sr)) - gs * wr;
	return m1 * (a_diff * por * sc - pur * (q.c * gc + q.f * c_diff * sc) - q.f * q.c * (gram - (1.0 / N) * sr * sc))
		- ssim_gv(q, curr, which, r) * wc + ur * sc;
}
/* the search method's Jacobian and Hessian: NCC's wiring (ncc_g, ncc_h; ncc_h_which / ncc_has_gram say which Gram matrix the pass must carry).
 * ESM calls updateCurrGrad and updateInitGrad in every pass (NT/ESM.cc:247-252), FCLK the first alone, ICLK the second: no method reads a
 * gradient member another pass left.  h0v: entry (r, c) of the constant self Hessian */
MTFHIP_HD double ssim_g(const mtfhip_sm_desc &sm, const SsimSys &q, int s) {
	if (sm.sm == MTFHIP_SM_FCLK) return ssim_curr_jac(q, NCC_JT, s);
	if (sm.sm == MTFHIP_SM_ICLK) return ssim_init_jac(q, NCC_J0, s);
	if (sm.jac_type == 0) return ssim_curr_jac(q, NCC_JM, s);
	return 0.5 * (ssim_curr_jac(q, NCC_JT, s) - ssim_init_jac(q, NCC_J0, s));
}
MTFHIP_HD double ssim_h(const mtfhip_sm_desc &sm, const SsimSys &q, double h0v, int r, int c) {
	const int ht = sm.hess_type;
	if (ht == 0) return h0v;
	if (sm.sm == MTFHIP_SM_ICLK) return ssim_hess(q, NCC_H_INIT, NCC_J0, r, c);   /* Std: cmptInitHessian(J0) */
	if (sm.sm == MTFHIP_SM_FCLK || ht == 1 || ht == 5) return ssim_hess(q, ht == 1 ? NCC_H_SELF : NCC_H_CURR, NCC_JT, r, c);
	if (ht == 2) return 0.5 * (ssim_hess(q, NCC_H_SELF, NCC_JT, r, c) + h0v);   /* SumOfSelf */
	if (ht == 3) return ssim_hess(q, NCC_H_CURR, NCC_JM, r, c);   /* Original: cmptCurrHessian(mean) */
	return 0.5 * (ssim_hess(q, NCC_H_INIT, NCC_J0, r, c) + ssim_hess(q, NCC_H_CURR, NCC_JT, r, c));   /* SumOfStd */
}
/* SSIM::getLikelihood, SSIM.cc:45-48 */
MTFHIP_HD double ssim_likelihood(double f, double alpha) { const double d = (1.0 / f) - 1; return exp(-alpha * d * d); }

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
