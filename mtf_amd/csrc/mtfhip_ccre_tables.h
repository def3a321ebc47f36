/*
 * mtfhip_ccre_tables.h -- the n_bins^2-sized algebra of the CCRE appearance model (AM/src/CCRE.cc), stated once for the host and the
 * device, in the manner of mtfhip_sm_system.h: from the raw sums of a histogram pass to the per-target table block the pixel passes read.
 * The device runs ccre_tables with one workgroup per target (k_ccre_tables, kernels_ccre.hip); a host program runs it with one "thread"
 * (tests/test_ccre_ref.py holds it to the float64 fixture generator).  Nothing here touches a pixel.
 */
#ifndef MTFHIP_CCRE_TABLES_H
#define MTFHIP_CCRE_TABLES_H
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MTFHIP_CCRE_HD __host__ __device__ inline
#else
#define MTFHIP_CCRE_HD inline
#endif

namespace mtfhip {

/* Per-target table block (doubles; a bin pair (i, j) -- i the cumulative bin of the current patch, j the bin of the template -- sits at
 * i * CCRE_NB + j).  It fills the block an MI batch keeps (MI_SIZE, mtfhip_internal.h): a batch has one appearance model for life. */
enum {
	CCRE_NB = 16,
	CCRE_HIST_0 = 0,        /* init_hist(j)                                             CCRE.cc:175-189 */
	CCRE_CUM_T = 16,        /* curr_cum_hist(i)                                         :325, :398 */
	CCRE_LOG_0 = 32, CCRE_LOG_CUM = 48,
	CCRE_JOINT = 64,        /* cum_joint_hist(i, j)                                     :326, :399 */
	CCRE_L = 320,           /* ccre_log_term(i, j)                                      :406-410 */
	CCRE_P = 576,           /* sum_{i' < i} (1 + ccre_log_term(i', j)): the rows below a pixel's window, where C = 1 (:440-450) */
	CCRE_SELF_JOINT = 832,  /* self_cum_joint_hist(i, j)                                :607, :634 */
	CCRE_SELF_L = 1088,     /* self_ccre_log_term(i, j)                                 :638-642 */
	CCRE_COLSUM = 1344,     /* cum_joint_hist_sum(j) = sum_i cum_joint_hist(i, j)       :533-543 */
	CCRE_RATIO = 1360,      /* cum_joint_hist_sum(j) / init_hist(j): what init_hist_grad_ratio / init_hist_hess_ratio are multiplied with */
	CCRE_HIST_T = 1376,     /* curr_hist(j) of cmptCumSelfHist                          :606, :633 */
	CCRE_LOG_T = 1392,
	CCRE_SIZE = 1408
};
/* what a call refreshes: the whole block from the template alone (initializeSimilarity :159-278: A = B = I0), the current patch's half
 * (updateSimilarity :319-414), or init_hist only (a second initializeSimilarity, :175-189) */
enum { CCRE_TB_INIT = 0, CCRE_TB_UPDATE = 1, CCRE_TB_HIST0 = 2 };

/* pre-seeding and normalisation: hist = norm (n_bins pre_seed + sum), joint = norm (pre_seed + sum)  (CCRE.cc:105, :175, :188, :233, :252) */
MTFHIP_CCRE_HD double ccre_seed_hist(double s, int nb, double pre_seed, double norm) { return (s + nb * pre_seed) * norm; }
MTFHIP_CCRE_HD double ccre_seed_joint(double s, double pre_seed, double norm) { return (s + pre_seed) * norm; }
/* hist_factor of cmptCurrHessian / cmptSelfHessian (:598, :674) */
MTFHIP_CCRE_HD double ccre_hess_factor(double joint, double cum) { return (1.0 / joint) - (1.0 / cum); }
/* entry (r, c) of what one bin pair adds to cmptInitHessian (:538-541): row^T (row / joint - 2 ratio_row), ratio_row = g / init_hist(j);
 * and of what one template bin adds (:544): cum_joint_hist_sum(j) ratio_row^T ratio_row */
MTFHIP_CCRE_HD double ccre_init_pair(double q_r, double q_c, double g_c, double joint, double h0) { return q_r * (q_c / joint - 2.0 * (g_c / h0)); }
MTFHIP_CCRE_HD double ccre_init_bin(double g_r, double g_c, double colsum, double h0) { return colsum * (g_r / h0) * (g_c / h0); }

/* raw: the sums over the pixels, one row of three histogram passes: R = nb + nb^2 doubles each --
 *   [0, R)    sum_p C_i | sum_p C_i beta_j       cumulative weights of A times the template's (A = It; I0 for CCRE_TB_INIT)
 *   [R, 2R)   .         | sum_p C_i beta_j(It)   cmptCumSelfHist (with_self)
 *   [2R, 3R)  sum_p beta_j | .                   the plain histogram: of I0 (CCRE_TB_INIT / _HIST0), of It (with_self)
 * tid / nth: this thread and how many run the function together; sync(): a barrier among them (nothing for one thread);
 * red: nth doubles they share.  f_out: f = sum cum_joint * ccre_log_term (:260, :413), written by thread 0. */
template <class Sync>
MTFHIP_CCRE_HD void ccre_tables(int tid, int nth, Sync sync, int nb, double pre_seed, double norm, int mode, int with_self,
	const double *raw, double *tb, double *red, double *f_out) {
	const int R = nb + nb * nb;
	const bool h0 = mode != CCRE_TB_UPDATE, rest = mode != CCRE_TB_HIST0;
	for (int k = tid; k < nb; k += nth) {
		if (h0) { const double v = ccre_seed_hist(raw[2 * R + k], nb, pre_seed, norm); tb[CCRE_HIST_0 + k] = v; tb[CCRE_LOG_0 + k] = log(v); }
		if (rest) { const double v = ccre_seed_hist(raw[k], nb, pre_seed, norm); tb[CCRE_CUM_T + k] = v; tb[CCRE_LOG_CUM + k] = log(v); }
		if (rest && with_self) { const double v = ccre_seed_hist(raw[2 * R + k], nb, pre_seed, norm); tb[CCRE_HIST_T + k] = v; tb[CCRE_LOG_T + k] = log(v); }
	}
	if (rest) {
		for (int q = tid; q < nb * nb; q += nth) {
			const int i = q / nb, j = q % nb;
			tb[CCRE_JOINT + i * CCRE_NB + j] = ccre_seed_joint(raw[nb + q], pre_seed, norm);
			if (with_self) tb[CCRE_SELF_JOINT + i * CCRE_NB + j] = ccre_seed_joint(raw[R + nb + q], pre_seed, norm);
		}
	}
	sync();
	double part = 0;
	if (rest) {
		for (int q = tid; q < nb * nb; q += nth) {
			const int i = q / nb, j = q % nb;
			const double jv = tb[CCRE_JOINT + i * CCRE_NB + j];
			const double lt = log(jv) - tb[CCRE_LOG_CUM + i] - tb[CCRE_LOG_0 + j];
			tb[CCRE_L + i * CCRE_NB + j] = lt;
			part += jv * lt;
			if (with_self) tb[CCRE_SELF_L + i * CCRE_NB + j] = log(tb[CCRE_SELF_JOINT + i * CCRE_NB + j]) - tb[CCRE_LOG_CUM + i] - tb[CCRE_LOG_T + j];
		}
	}
	red[tid] = part;
	sync();
	if (rest) {
		for (int j = tid; j < nb; j += nth) {
			double cs = 0, pre = 0;
			for (int i = 0; i < nb; ++i) {
				tb[CCRE_P + i * CCRE_NB + j] = pre;
				pre += 1 + tb[CCRE_L + i * CCRE_NB + j];
				cs += tb[CCRE_JOINT + i * CCRE_NB + j];
			}
			tb[CCRE_COLSUM + j] = cs;
			tb[CCRE_RATIO + j] = cs / tb[CCRE_HIST_0 + j];
		}
		if (tid == 0 && f_out) {
			double s = 0;
			for (int k = 0; k < nth; ++k) s += red[k];
			*f_out = s;
		}
	}
}

} // namespace mtfhip
#endif
