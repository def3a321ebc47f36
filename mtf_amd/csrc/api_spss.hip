/*
 * api_spss.hip -- the Sum of Pixelwise Structural Similarity appearance model's own state (AM/src/SPSS.cc): its parameter k, what a fused
 * launch reads for a search method (its row's f, g and H: the SPSS entries of mtfhip_sm_system.h), and the per-function similarity, gradients and Hessians
 * (C-ABI implementation, include/mtfhip.h; the kernels: kernels_spss.hip, kernels_fused_spss.hip; no CPU fallback: HIP kernels or an error)
 */
#include "mtfhip_api_internal.h"

/* the weight of the Gram matrix the pass accumulates and the row of its current Jacobian, by search method and Hessian type (NT/FCLK.cc:262-283,
 * NT/ESM.cc:298-377, NT/ICLK.cc:204-252): the self types weight Jt by cmptSelfHessian's factor, the Std types by cmptCurrHessian's (ESM Original:
 * over the mean row, FusedArgs::hess_mean) or, for ICLK, J0 by cmptInitHessian's; InitialSelf reads the constant H0 and ignores the sum */
SpssArgs spss_args(const mtfhip_batch *b, const mtfhip_sm_desc *sm) {
	SpssArgs sp;
	sp.c = b->spss_c;
	const int ht = sm->hess_type;
	if (sm->sm == MTFHIP_SM_ICLK) sp.weight = ht == 2 ? SPSS_W_INIT : SPSS_W_SELF;
	else if (sm->sm == MTFHIP_SM_FCLK) sp.weight = ht == 2 ? SPSS_W_CURR : SPSS_W_SELF;
	else sp.weight = ht >= 3 ? SPSS_W_CURR : SPSS_W_SELF;
	sp.g_mean = (sm->sm == MTFHIP_SM_ESM && sm->jac_type == 0) ? 1 : 0;
	return sp;
}

/* SPSS::initializeSimilarity SPSS.cc:94-100: It = I0, f_vec = 1, f = patch_size */
int spss_initialize_similarity(mtfhip_batch *b) {
	if (b->init_sim) return MTFHIP_OK;
	HIP_TRY(hipMemsetAsync(b->buf[MTFHIP_BUF_DF_DI0], 0, sizeof(double) * b->N * b->B, b->ctx->stream));
	for (auto &h : b->th) h.f = (double)b->N;
	return MTFHIP_OK;
}
int spss_update_similarity(mtfhip_batch *b, int prereq_only) {
	/* (f_vec, f_vec_den and It_sqr are functions of I0 and It: every kernel that needs them recomputes them, so prereq_only has nothing to store) */
	if (prereq_only) return MTFHIP_OK;
	const int nblk = simple_blocks_per_target(b->N);
	{
		TimedScope ts(b->ctx, "spss_similarity");
		launch_spss_similarity(b->view(), b->spss_c, b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t) b->th[t].f = b->h_acc[(size_t)t * ACC_COUNT + ACC_RR];
	return MTFHIP_OK;
}
/* which 0: updateInitGrad, 1: updateCurrGrad, 2: initializeGrad (SPSS.cc:104-114) */
int spss_update_grad(mtfhip_batch *b, int which) {
	if (which == 2) return zero_grad_vectors(b);
	TimedScope ts(b->ctx, "spss_grad");
	launch_spss_grad(b->view(), b->spss_c, which, b->buf[which ? MTFHIP_BUF_DF_DIT : MTFHIP_BUF_DF_DI0], b->ctx->stream);
	return MTFHIP_OK;
}
int spss_weighted_hessian(mtfhip_batch *b, int j_buf, int weight, double *H) {
	const int nblk = simple_blocks_per_target(b->N), S = b->S;
	{
		TimedScope ts(b->ctx, "spss_hessian");
		launch_spss_hessian(b->view(), b->spss_c, weight, b->buf[j_buf], b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t) {
		const double *src = b->h_acc + (size_t)t * ACC_COUNT + ACC_H;
		double *Ht = H + (size_t)t * S * S;
		int k = 0;
		for (int a = 0; a < 8; ++a)
			for (int c = a; c < 8; ++c) {
				if (a < S && c < S) { Ht[c * S + a] = src[k]; Ht[a * S + c] = src[k]; }
				++k;
			}
	}
	return MTFHIP_OK;
}
/* SPSS::cmptInitHessian / cmptCurrHessian / cmptSelfHessian: kind 0 init, 1 curr, 2 self */
int spss_hessian(mtfhip_batch *b, int j_buf, int kind, double *H) {
	static const int weight[3] = {SPSS_W_INIT, SPSS_W_CURR, SPSS_W_SELF};
	return spss_weighted_hessian(b, j_buf, weight[kind], H);
}
/* SPSS::getLikelihood SPSS.cc:46-48 */
int spss_likelihood(const mtfhip_batch *b, int t, double *l) {
	*l = std::exp(b->desc.likelihood_alpha * (b->th[t].f - (double)b->N));
	return MTFHIP_OK;
}

extern "C" {

int mtfhip_batch_set_spss(mtfhip_batch *b, double k) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "set_spss: NULL batch");
	if (!spss_am(b)) return fail(MTFHIP_ERR_INVALID_ARG, "set_spss: the batch's appearance model is %d, not SPSS", b->desc.am);
	if (b->init_pix_vals || b->init_sim)
		return fail(MTFHIP_ERR_LOGIC, "set_spss: k is fixed once the template is initialised (call it before init_template / initialize_similarity)");
	if (!std::isfinite(k)) return fail(MTFHIP_ERR_INVALID_ARG, "set_spss: k is not a finite number");
	const double kk = k > 0 ? k : 0.01;
	/* SPSS.cc:37-38: c = k (PIX_MAX - PIX_MIN); c *= c */
	double c = kk * (255.0 - 0.0);
	c *= c;
	/* c keeps f_vec_den = I0^2 + It^2 + c away from zero on black pixels: a k whose c is not a normal number would divide by zero there */
	if (!std::isnormal(c)) return fail(MTFHIP_ERR_INVALID_ARG, "set_spss: k = %g gives c = (255 k)^2 = %g, which is not a normal number", kk, c);
	b->spss_k = kk;
	b->spss_c = c;
	return MTFHIP_OK;
}

} /* extern "C" */
