/*
 * api_ccre.hip -- the Cross Cumulative Residual Entropy appearance model (AM/src/CCRE.cc, first order, symmetrical_grad = 0): its per-function
 * similarity, gradients and Hessians, one fused iteration for a host-side solve (ccre_iterate) and the CCRE driver of the device-side loop
 * (track_loop_ccre, behind track_core in api_track.hip).  The skeleton is MI's materialising iteration (mi_enqueue, api_mi_iter.hip) with
 * cumulative weights on the current patch's side, CCRE's tables and its Hessian formulas; a CCRE batch keeps its state in the buffers an MI
 * batch has (d_mi_tb, d_mi_part, d_mi_red, d_mi_f, d_mi_H).
 * (C-ABI implementation, include/mtfhip.h; the kernels: kernels_ccre.hip and k_mi_hist<.., CUM> of kernels_mi.hip; no CPU fallback: HIP
 * kernels or an error)
 */
#include "mtfhip_api_internal.h"
#include "mtfhip_ccre_tables.h"

static int ccre_read_f(mtfhip_batch *b, bool as_max) {
	std::vector<double> f(b->B);
	HIP_TRY(hipMemcpyAsync(f.data(), b->d_mi_f, sizeof(double) * b->B, hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	for (int t = 0; t < b->B; ++t) b->th[t].f = f[t];
	if (as_max) b->ccre_f_max = f;   /* max_similarity, CCRE.cc:261 */
	return MTFHIP_OK;
}
/* the histogram passes of one table refresh, each into its own columns of the block rows (launch_ccre_tables), and the tables.
 * mode: CCRE_TB_* (mtfhip_ccre_tables.h); with_self: cmptCumSelfHist's two histograms of It ride along (CCRE.cc:604-643) */
static void ccre_hist_tables(mtfhip_batch *b, int mode, int with_self) {
	const int nb = b->desc.mi_n_bins, nblk = mi_blocks(b), R = nb + nb * nb;
	const double *I0 = b->buf[MTFHIP_BUF_I0], *It = b->buf[MTFHIP_BUF_IT];
	hipStream_t st = b->ctx->stream;
	const BatchView bv = b->view();
	TimedScope ts(b->ctx, "ccre_hist");
	if (mode != mtfhip::CCRE_TB_HIST0) launch_ccre_hist(bv, nb, b->mi_hist_norm, mode == mtfhip::CCRE_TB_INIT ? I0 : It, I0, b->d_mi_part, nblk, b->mi_row_len, st);
	if (mode != mtfhip::CCRE_TB_UPDATE) launch_mi_hist(bv, nb, b->mi_hist_norm, I0, I0, b->d_mi_part + 2 * R, nblk, b->mi_row_len, st);
	else if (with_self) {
		launch_ccre_hist(bv, nb, b->mi_hist_norm, It, It, b->d_mi_part + R, nblk, b->mi_row_len, st);
		launch_mi_hist(bv, nb, b->mi_hist_norm, It, It, b->d_mi_part + 2 * R, nblk, b->mi_row_len, st);
	}
	launch_ccre_tables(bv, nb, b->desc.mi_pre_seed, b->mi_hist_norm, mode, with_self, b->d_mi_part, nblk, b->mi_row_len, b->d_mi_tb, b->d_mi_f, st);
}

/* CCRE::initializeSimilarity CCRE.cc:159-278: everything from the template alone (A = B = I0); a second call refreshes init_hist only */
int ccre_initialize_similarity(mtfhip_batch *b) {
	const bool first = !b->init_sim;
	ccre_hist_tables(b, first ? mtfhip::CCRE_TB_INIT : mtfhip::CCRE_TB_HIST0, 0);
	if (first) TRY(ccre_read_f(b, true));
	return MTFHIP_OK;
}
/* CCRE::updateSimilarity CCRE.cc:319-414 */
int ccre_update_similarity(mtfhip_batch *b, int prereq_only) {
	ccre_hist_tables(b, mtfhip::CCRE_TB_UPDATE, 0);
	if (!prereq_only) TRY(ccre_read_f(b, false));
	return MTFHIP_OK;
}
/* which 0: updateInitGrad (CCRE.cc:425-464) into DF_DI0; 1: updateCurrGrad (:465-476) into DF_DIT; 2: initializeGrad (:287-308): the current-side
 * expression with the cumulative weights of I0 itself into DF_DI0, and df_dIt = df_dI0 */
int ccre_grad(mtfhip_batch *b, int which) {
	const int nb = b->desc.mi_n_bins, ng = std::min(simple_blocks_per_target(b->N), 64);
	const double *I0 = b->buf[MTFHIP_BUF_I0], *It = b->buf[MTFHIP_BUF_IT];
	const mtfhip::MiJ0Rebuild none{nullptr, nullptr, nullptr, 0, 0};
	TimedScope ts(b->ctx, "ccre_grad");
	launch_ccre_grad_gemv(b->view(), nb, b->mi_hist_norm, which == 2 ? I0 : It, I0, b->d_mi_tb, nullptr, nullptr, none,
		which == 1 ? b->buf[MTFHIP_BUF_DF_DIT] : (which == 2 ? b->buf[MTFHIP_BUF_DF_DI0] : nullptr), which == 0 ? b->buf[MTFHIP_BUF_DF_DI0] : nullptr,
		b->d_partials, ng, b->ctx->stream);
	if (which == 2)
		HIP_TRY(hipMemcpyAsync(b->buf[MTFHIP_BUF_DF_DIT], b->buf[MTFHIP_BUF_DF_DI0], sizeof(double) * b->N * b->B, hipMemcpyDeviceToDevice, b->ctx->stream));
	return MTFHIP_OK;
}
/* one Hessian pass into out ([B][64], column-major S x S): kind 0 cmptInitHessian (CCRE.cc:521-560), 1 cmptCurrHessian (:564-602),
 * 2 cmptSelfHessian (:644-678; its tables must be there: ccre_hist_tables with_self) */
static void ccre_hess_pass(mtfhip_batch *b, int kind, int j_buf, double *out) {
	const int nb = b->desc.mi_n_bins, nblk = mi_blocks(b);
	hipStream_t st = b->ctx->stream;
	TimedScope ts(b->ctx, "ccre_hess");
	launch_ccre_hess(b->view(), nb, b->mi_hist_norm, kind, b->buf[MTFHIP_BUF_IT], b->buf[MTFHIP_BUF_I0], b->d_mi_tb, b->buf[j_buf], b->d_mi_part, nblk,
		b->mi_row_len, st);
	launch_finish_rows(b->d_mi_part, nblk, b->mi_row_len, b->d_mi_red, b->B, st);
	launch_ccre_hess_finish(b->view(), nb, kind, b->d_mi_red, b->mi_row_len, b->d_mi_tb, out, st);
}
int ccre_hessian(mtfhip_batch *b, int j_buf, int kind, double *H) {
	const int S = b->S;
	/* cmptCumSelfHist (CCRE.cc:604-643) is part of cmptSelfHessian; the block rows of the last similarity update are gone by now (every
	 * Hessian pass writes its own there), so the current patch's half of the tables is taken again beside it: the same values */
	if (kind == 2) ccre_hist_tables(b, mtfhip::CCRE_TB_UPDATE, 1);
	ccre_hess_pass(b, kind, j_buf, b->d_mi_H);
	std::vector<double> h(64 * (size_t)b->B);
	HIP_TRY(hipMemcpyAsync(h.data(), b->d_mi_H, sizeof(double) * h.size(), hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	for (int t = 0; t < b->B; ++t) std::memcpy(H + (size_t)t * S * S, &h[64 * t], sizeof(double) * S * S);
	return MTFHIP_OK;
}
/* CCRE::getLikelihood CCRE.h:72-75 with likelihood_beta = 0 (the descriptor carries alpha alone): d = max_similarity / f - 1.
 * max_similarity is initializeSimilarity's f: without one there is nothing to compare with */
int ccre_likelihood(const mtfhip_batch *b, int t, double *l) {
	if ((int)b->ccre_f_max.size() != b->B) return fail(MTFHIP_ERR_LOGIC, "getLikelihood: CCRE before initializeSimilarity (max_similarity is its f)");
	const double d = (b->ccre_f_max[t] / b->th[t].f) - 1;
	*l = std::exp(-b->desc.likelihood_alpha * d * d);
	return MTFHIP_OK;
}

extern "C" {

/* One ESM / FCLK / ICLK iteration with CCRE, the passes of mi_enqueue (api_mi_iter.hip):
 *   0. the fused LK kernel (SSD instantiation, materialising): warp -> It, dIt_dx, Jt (its SSD sums are ignored; CCRE's pixel scaling
 *      travels in norm_mult / norm_add).  ICLK: It only.  Targets whose `active` flag is 0 keep their It / Jt, and so their tables.
 *   1. k_mi_hist<.., CUM>: cumulative histogram of It and cumulative joint (It, I0) -- and for the self Hessians (It, It) and the plain
 *      histogram of It -- then k_ccre_tables.
 *   2. k_ccre_grad_gemv: both gradient vectors and df_dIt . Jt, df_dI0 . J0 in one pass.
 *   3. k_ccre_hess + k_ccre_hess_finish for the Hessian the search method reads (twice for SumOfStd).
 * Results on the device as mi_enqueue leaves them: d_mi_f [B]; d_mi_H = [B][64] H | [B][16] g rows | [B][64] cmptInitHessian(J0) of SumOfStd. */
static int ccre_grad_blocks(const mtfhip_batch *b) { return std::min(simple_blocks_per_target(b->N), 64); }
static int ccre_gmode(const MiPlan &pl) { return pl.iclk ? 0 : (pl.fclk ? 1 : (pl.orig_jac ? 2 : 3)); }
static int ccre_enqueue(mtfhip_batch *b, const mtfhip_sm_desc *sm, const MiPlan &pl, const int *active, bool reduce_g = true) {
	const int nb = b->desc.mi_n_bins;
	hipStream_t st = b->ctx->stream;
	/* 0 */
	mtfhip_sm_desc s0 = *sm;
	s0.sm = pl.need_jt ? MTFHIP_SM_FCLK : MTFHIP_SM_ICLK; s0.hess_type = pl.need_jt ? 1 : 0; s0.materialize = 1; s0.sec_ord_hess = 0;
	FusedArgs fa;
	TRY(fused_args(b, &s0, fa));
	fa.active = active;
	{
		TimedScope ts(b->ctx, "fused_lk");
		BatchView v = fused_view(b, fa);
		v.am = MTFHIP_AM_SSD;   /* (the launch IS the SSD pass: its kernel is chosen by the view's model) */
		launch_fused_ssd(v, b->ctx->img, fa, b->d_partials, fused_blocks_per_target(b->N, b->B), st);
	}
	b->it_valid = true;
	b->dit_valid = b->jt_valid = pl.need_jt;
	if (pl.need_mean) {
		TRY(ensure_buf(b, MTFHIP_BUF_JM));
		TimedScope ts(b->ctx, "mean_jacobian");
		launch_mean_jacobian(b->view(), st);
	}
	/* 1 */
	ccre_hist_tables(b, mtfhip::CCRE_TB_UPDATE, pl.self ? 1 : 0);
	/* 2 */
	double *d_g = b->d_mi_H + 64 * (size_t)b->B;
	{
		TimedScope ts(b->ctx, "ccre_grad");
		const int ng = ccre_grad_blocks(b);
		launch_ccre_grad_gemv(b->view(), nb, b->mi_hist_norm, b->buf[MTFHIP_BUF_IT], b->buf[MTFHIP_BUF_I0], b->d_mi_tb,
			pl.iclk ? nullptr : b->buf[pl.orig_jac ? MTFHIP_BUF_JM : MTFHIP_BUF_JT],
			(pl.fclk || pl.orig_jac) ? nullptr : b->buf[MTFHIP_BUF_J0], mi_j0_rebuild(b), sm->materialize ? b->buf[MTFHIP_BUF_DF_DIT] : nullptr,
			sm->materialize ? b->buf[MTFHIP_BUF_DF_DI0] : nullptr, b->d_partials, ng, st);
		if (reduce_g) launch_finish_rows(b->d_partials, ng, 16, d_g, b->B, st);   /* (the device-side loop sums the rows in its finish) */
	}
	/* 3 */
	switch (pl.hk) {
	case MiPlan::H_SUM_STD:   /* cmptSumOfHessians = cmptInitHessian(J0) + cmptCurrHessian(Jt) (AppearanceModel.h:194-206) */
		ccre_hess_pass(b, 0, MTFHIP_BUF_J0, b->d_mi_H + 80 * (size_t)b->B);
		ccre_hess_pass(b, 1, MTFHIP_BUF_JT, b->d_mi_H);
		break;
	case MiPlan::H_SELF_JT: ccre_hess_pass(b, 2, MTFHIP_BUF_JT, b->d_mi_H); break;
	case MiPlan::H_CURR_JT: ccre_hess_pass(b, 1, MTFHIP_BUF_JT, b->d_mi_H); break;
	case MiPlan::H_CURR_JM: ccre_hess_pass(b, 1, MTFHIP_BUF_JM, b->d_mi_H); break;
	case MiPlan::H_INIT_J0: ccre_hess_pass(b, 0, MTFHIP_BUF_J0, b->d_mi_H); break;
	default: break;
	}
	return MTFHIP_OK;
}
/* g, H of the search method as in NT/ESM.cc:298-377, NT/FCLK.cc:260-288, NT/ICLK.cc:206-251 (the host assembly of mi_iterate) */
int ccre_iterate(mtfhip_batch *b, const mtfhip_sm_desc *sm, double *f, double *g, double *H) {
	const int S = b->S;
	hipStream_t st = b->ctx->stream;
	const MiPlan pl(sm);
	TRY(ccre_enqueue(b, sm, pl, nullptr));
	const size_t B = (size_t)b->B;
	std::vector<double> out(B * 145);
	HIP_TRY(hipMemcpyAsync(out.data(), b->d_mi_H, sizeof(double) * (pl.hk == MiPlan::H_SUM_STD ? 144 : 80) * B, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(out.data() + 144 * B, b->d_mi_f, sizeof(double) * B, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (int t = 0; t < b->B; ++t) {
		const double *Hs = &out[64 * (size_t)t], *gs = &out[64 * B + 16 * (size_t)t], *H2 = &out[80 * B + 64 * (size_t)t];
		TargetHost &h = b->th[t];
		h.f = out[144 * B + t];
		if (f) f[t] = h.f;
		double *gt = g + (size_t)t * S, *Ht = H + (size_t)t * S * S;
		for (int s = 0; s < S; ++s) gt[s] = pl.iclk ? gs[8 + s] : ((pl.fclk || pl.orig_jac) ? gs[s] : 0.5 * (gs[s] - gs[8 + s]));
		for (int k = 0; k < S * S; ++k) {
			const int r = k % S, c = k / S;
			const double hv = Hs[c * S + r];   /* k_ccre_hess_finish writes column-major S x S */
			Ht[k] = pl.hk == MiPlan::H_CONST ? h.h0[k]
				: (pl.esm && sm->hess_type == 2) ? 0.5 * (hv + h.h0[k])
				: pl.hk == MiPlan::H_SUM_STD ? 0.5 * (hv + H2[c * S + r])
				: hv;
		}
	}
	return MTFHIP_OK;
}

/* the CCRE driver of track_core (api_track.hip), as track_loop_mi's materialising form: the passes leave g and H on the device and
 * k_finish_track_mi runs the shared finish over them (solve, compositional update, convergence test, Levenberg-Marquardt on d_mi_f) */
int track_loop_ccre(mtfhip_batch *b, const mtfhip_sm_desc *sm, TrackState &ts, const TrackCtx &cx) {
	const MiPlan pl(sm);
	ts.h_from_acc = 1;
	const BatchView bv = b->view();
	std::vector<int> h_flags;
	for (int it = 0; it < cx.max_passes; ++it) {
		TRY(ccre_enqueue(b, sm, pl, b->d_active, false));
		launch_finish_track_mi(bv, *sm, ts, pl.hk == MiPlan::H_SUM_STD, ccre_gmode(pl), b->d_mi_H, b->d_partials, ccre_grad_blocks(b), b->d_mi_red, b->ctx->stream);
		if (loop_all_stopped(sm, cx.max_passes, it, b->d_active, b->B, b->ctx->stream, h_flags)) break;
	}
	return MTFHIP_OK;
}

} /* extern "C" */
