/*
 * api_mi.hip -- the Mutual Information appearance model's per-function code (AM/src/MI.cc): its row of kAmOps (the histogram passes, the
 * gradients from the factor tables, the Hessians), the self weight of the second-order self Hessian, and MI's half of the deferred-fusion
 * layer (api_lazy.hip).  The fused iteration and the device-side loop's driver: api_mi_iter.hip
 * (C-ABI implementation, include/mtfhip.h; the kernels: kernels_mi.hip, kernels_mi_fused.hip; shared declarations: mtfhip_api_internal.h;
 * no CPU fallback: HIP kernels or an error)
 */
#include "mtfhip_api_internal.h"

extern "C" {

/* ------------------------------------------------------------------ per function (MI's row of kAmOps) */
static int mi_read_f(mtfhip_batch *b) {
	std::vector<double> f(b->B);
	HIP_TRY(hipMemcpyAsync(f.data(), b->d_mi_f, sizeof(double) * b->B, hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	for (int t = 0; t < b->B; ++t) b->th[t].f = f[t];
	return MTFHIP_OK;
}
/* workgroups per target for the MI histogram / Hessian passes: enough to fill the chip (~4 per CU over the batch), few
 * enough that every wave amortises its register-resident bin accumulators over many 64-pixel chunks and that the
 * fixed-order finish has short columns to add */
int mi_blocks(const mtfhip_batch *b) {
	int nb = 1024 / b->B;
	if (nb < 1) nb = 1;
	return std::min(nb, simple_blocks_per_target(b->N));
}
/* mode 0 initialise (A = B = I0), 1 update (A = It, B = I0), 2 self (A = B = It) */
static int mi_hist_pass(mtfhip_batch *b, int mode, int first_init) {
	const int nb = b->desc.mi_n_bins, nblk = mi_blocks(b);
	const double *A = b->buf[mode == 0 ? MTFHIP_BUF_I0 : MTFHIP_BUF_IT];
	const double *Bv = b->buf[mode == 2 ? MTFHIP_BUF_IT : MTFHIP_BUF_I0];
	TimedScope ts(b->ctx, "mi_hist");
	launch_mi_hist(b->view(), nb, b->mi_hist_norm, A, Bv, b->d_mi_part, nblk, b->mi_row_len, b->ctx->stream);
	launch_mi_hist_finish(b->view(), nb, b->desc.mi_pre_seed, b->mi_hist_norm, mode, first_init, b->d_mi_part, nblk,
		b->mi_row_len, b->d_mi_tb, b->d_mi_f, b->ctx->stream);
	if (mode == 2) b->lz.mi_self_it = b->lz.ver[MTFHIP_BUF_IT];
	return MTFHIP_OK;
}
/* MI::initializeSimilarity MI.cc:207-287 */
int mi_initialize_similarity(mtfhip_batch *b) {
	const int first = b->init_sim ? 0 : 1;
	TRY(mi_hist_pass(b, 0, first));
	if (first) TRY(mi_read_f(b));
	return MTFHIP_OK;
}
/* MI::updateSimilarity MI.cc:346-382 */
int mi_update_similarity(mtfhip_batch *b, int prereq_only) {
	TRY(mi_hist_pass(b, 1, 0));
	b->lz.df0_it_ver = b->lz.ver[MTFHIP_BUF_IT];
	if (!prereq_only) TRY(mi_read_f(b));
	return MTFHIP_OK;
}
/* which 0: MI::updateInitGrad, 1: updateCurrGrad, each behind a refresh of its factor table; 2: initializeGrad (MI.cc:299-332): df_dI0
 * from the initial tables, df_dIt = df_dI0 */
int mi_grad(mtfhip_batch *b, int which) {
	const int nb = b->desc.mi_n_bins;
	const double *I0 = b->buf[MTFHIP_BUF_I0], *It = b->buf[MTFHIP_BUF_IT];
	{
		TimedScope ts(b->ctx, "mi_grad");
		if (which != 2) launch_mi_factor(b->view(), nb, which, b->d_mi_tb, b->ctx->stream);
		if (which == 1) launch_mi_grad(b->view(), nb, b->mi_hist_norm, It, I0, b->d_mi_tb, MI_T_CURR, b->buf[MTFHIP_BUF_DF_DIT], b->ctx->stream);
		else launch_mi_grad(b->view(), nb, b->mi_hist_norm, I0, which == 2 ? I0 : It, b->d_mi_tb, MI_T_INIT, b->buf[MTFHIP_BUF_DF_DI0], b->ctx->stream);
	}
	if (which == 2)
		HIP_TRY(hipMemcpyAsync(b->buf[MTFHIP_BUF_DF_DIT], b->buf[MTFHIP_BUF_DF_DI0], sizeof(double) * b->N * b->B, hipMemcpyDeviceToDevice, b->ctx->stream));
	return MTFHIP_OK;
}
/* kind 0 init (MI.cc:461-513), 1 curr (:603-637), 2 self (:515-601, the returned second pass) */
int mi_hessian(mtfhip_batch *b, int j_buf, int kind, double *H) {
	const int nb = b->desc.mi_n_bins, nblk = mi_blocks(b), S = b->S;
	if (kind == 2) {   /* cmptSelfHist MI.cc:639-659 -- unless the fused histogram pass of this iteration took it along */
		b->lz.mi_want_self = true;
		if (b->lz.no_cache || b->lz.mi_self_it != b->lz.ver[MTFHIP_BUF_IT]) TRY(mi_hist_pass(b, 2, 0));
	}
	const double *A = b->buf[kind == 0 ? MTFHIP_BUF_I0 : MTFHIP_BUF_IT];
	const double *Bv = b->buf[kind == 1 ? MTFHIP_BUF_I0 : MTFHIP_BUF_IT];
	const int table = kind == 0 ? MI_T_INIT : (kind == 1 ? MI_T_CURR : MI_T_SELF);
	const int joint = kind == 2 ? MI_SELF_JOINT : MI_JOINT;
	const int hist = kind == 0 ? MI_HIST_INIT : MI_HIST_CURR;
	{
		TimedScope ts(b->ctx, "mi_hess");
		launch_mi_hess(b->view(), nb, b->mi_hist_norm, A, Bv, b->d_mi_tb, table, kind == 0, b->buf[j_buf], b->d_mi_part, nblk,
			b->mi_row_len, b->ctx->stream);
		/* two short launches instead of one long one: the column sums are spread over the chip, the assembly reads one row */
		launch_finish_rows(b->d_mi_part, nblk, b->mi_row_len, b->d_mi_red, b->B, b->ctx->stream);
		launch_mi_hess_finish(b->view(), nb, b->d_mi_red, 1, b->mi_row_len, b->d_mi_tb, joint, hist, kind == 0, b->d_mi_H,
			b->ctx->stream);
	}
	std::vector<double> h(64 * (size_t)b->B);
	HIP_TRY(hipMemcpyAsync(h.data(), b->d_mi_H, sizeof(double) * h.size(), hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	for (int t = 0; t < b->B; ++t) std::memcpy(H + (size_t)t * S * S, &h[64 * t], sizeof(double) * S * S);
	return MTFHIP_OK;
}
/* the second-order self Hessian's pixel weights into d_d2_w: sum_r curr_hist_grad(r) * sum_t curr_hist_mat(t) * self_grad_factor(r, t)
 * (MI.cc:710-723); the self table must be there (the first-order cmptSelfHessian fills it) */
int mi_self_weight(mtfhip_batch *b) {
	HIP_TRY(b->d_d2_w.reserve((size_t)b->N * b->B));
	launch_mi_grad(b->view(), b->desc.mi_n_bins, b->mi_hist_norm, b->buf[MTFHIP_BUF_IT], b->buf[MTFHIP_BUF_IT], b->d_mi_tb, MI_T_SELF,
		b->d_d2_w, b->ctx->stream);
	return MTFHIP_OK;
}

/* ------------------------------------------------------------------ MI's half of the deferred-fusion layer */
/* updateSimilarity of a deferred sequence, for the It a materialising fused launch has just written: one histogram pass (with the self
 * histogram when the search method has been asking for self Hessians) and one table kernel, as passes 1 of mi_enqueue (api_mi_iter.hip) */
static void mi_lazy_hist_tables(mtfhip_batch *b) {
	mtfhip_batch::Lazy &L = b->lz;
	const int nb = b->desc.mi_n_bins, nblk = mi_blocks(b);
	const double *It = b->buf[MTFHIP_BUF_IT], *I0 = b->buf[MTFHIP_BUF_I0];
	hipStream_t st = b->ctx->stream;
	const bool self = L.mi_want_self && !L.no_cache;
	TimedScope ts(b->ctx, "mi_hist");
	if (self) launch_mi_hist_self(b->view(), nb, b->mi_hist_norm, It, I0, b->d_mi_part, nblk, b->mi_row_len, st);
	else launch_mi_hist(b->view(), nb, b->mi_hist_norm, It, I0, b->d_mi_part, nblk, b->mi_row_len, st);
	launch_mi_tables_iter(b->view(), nb, b->desc.mi_pre_seed, b->mi_hist_norm, self ? 1 : 0, b->d_mi_part, nblk, b->mi_row_len, b->d_mi_tb,
		b->d_mi_f, st);
	L.mi_self_it = self ? L.ver[MTFHIP_BUF_IT] : -1;
}
/* lazy_try_similarity's MI tail: the lean launch wrote It (its SSD sums are ignored); now the histogram pass, the table kernel and f */
int mi_lazy_similarity(mtfhip_batch *b) {
	mi_lazy_hist_tables(b);
	return mi_read_f(b);
}
/* lazy_try_fused's MI form: the recognised sequence is served by the fused MI passes (api_mi_iter.hip: mi_enqueue describes
 * them) -- the fused LK kernel materialising It / dIt_dx / Jt, the histogram and table pass, one gradient + Jacobian-product pass that
 * also writes the gradient vectors the recorded update*Grad calls would have written.  `sm` carries what lazy_try_fused classified. */
int mi_lazy_fused(mtfhip_batch *b, int trig, int j_a, const mtfhip_sm_desc &sm, bool replay, double *g, int *done) {
	mtfhip_batch::Lazy &L = b->lz;
	const bool iclk = sm.sm == MTFHIP_SM_ICLK;
	if (trig == LAZY_CURR_JAC && j_a != MTFHIP_BUF_JT) return MTFHIP_OK;   /* Original Jacobian: df_dIt . Jm is not accumulated */
	if (sm.sm != MTFHIP_SM_FCLK && !L.ig) return MTFHIP_OK;                /* df_dI0 comes from updateInitGrad */
	const int nb = b->desc.mi_n_bins, S = b->S;
	hipStream_t st = b->ctx->stream;
	if (replay || !iclk) {   /* (ICLK on a current IT needs nothing from the image) */
		mtfhip_sm_desc s0 = sm;
		s0.sm = iclk ? MTFHIP_SM_ICLK : MTFHIP_SM_FCLK; s0.hess_type = iclk ? 0 : 1; s0.materialize = 1;
		FusedArgs fa;
		TRY(fused_args(b, &s0, fa));
		{
			TimedScope ts(b->ctx, "fused_lk");
			launch_fused_ssd(fused_view(b, fa), b->ctx->img, fa, b->d_partials, fused_blocks_per_target(b->N, b->B), st);
		}
		const bool self_was = L.mi_self_it == L.ver[MTFHIP_BUF_IT];
		touch(b, MTFHIP_BUF_IT);
		if (!replay && self_was) L.mi_self_it = L.ver[MTFHIP_BUF_IT];   /* same bits */
		b->it_valid = true;
		L.it_epoch = L.epoch;
		if (!iclk) { touch(b, MTFHIP_BUF_DIT_DX); touch(b, MTFHIP_BUF_JT); b->dit_valid = b->jt_valid = true; }
	}
	const double *It = b->buf[MTFHIP_BUF_IT], *I0 = b->buf[MTFHIP_BUF_I0];
	if (replay) mi_lazy_hist_tables(b);
	else {   /* updateSimilarity already ran for this IT: only the factor tables update*Grad would refresh */
		TimedScope ts(b->ctx, "mi_hist");
		launch_mi_factor(b->view(), nb, 1, b->d_mi_tb, st);
		launch_mi_factor(b->view(), nb, 0, b->d_mi_tb, st);
	}
	L.df0_it_ver = L.ver[MTFHIP_BUF_IT];
	double *d_g = b->d_mi_H + 64 * (size_t)b->B;
	{
		TimedScope ts(b->ctx, "mi_grad");
		const int ng = std::min(simple_blocks_per_target(b->N), 64);
		launch_mi_grad_gemv(b->view(), nb, b->mi_hist_norm, It, I0, b->d_mi_tb, iclk ? nullptr : b->buf[MTFHIP_BUF_JT],
			sm.sm == MTFHIP_SM_FCLK ? nullptr : b->buf[MTFHIP_BUF_J0], mi_j0_rebuild(b), L.cg ? b->buf[MTFHIP_BUF_DF_DIT] : nullptr,
			L.ig ? b->buf[MTFHIP_BUF_DF_DI0] : nullptr, b->d_partials, ng, st);
		launch_finish_rows(b->d_partials, ng, 16, d_g, b->B, st);
	}
	const bool want_mean = L.jm != 0;
	L.pv = L.gp = L.pg = L.pj = L.sim = L.cg = L.ig = L.jm = 0;
	if (want_mean) TRY(do_mean_jacobian(b));
	std::vector<double> out((size_t)17 * b->B);
	HIP_TRY(hipMemcpyAsync(out.data(), d_g, sizeof(double) * 16 * b->B, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(out.data() + (size_t)16 * b->B, b->d_mi_f, sizeof(double) * b->B, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (int t = 0; t < b->B; ++t) {
		const double *gs = &out[(size_t)16 * t];
		if (replay) b->th[t].f = out[(size_t)16 * b->B + t];
		for (int s = 0; s < S; ++s)
			g[(size_t)t * S + s] = trig == LAZY_INIT_JAC ? gs[8 + s] : (trig == LAZY_CURR_JAC ? gs[s] : gs[s] - gs[8 + s]);
	}
	*done = 1;
	return MTFHIP_OK;
}

} /* extern "C" */
