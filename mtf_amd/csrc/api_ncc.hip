/*
 * api_ncc.hip -- the Normalized Cross Correlation appearance model's own code (AM/src/NCC.cc): its row of kAmOps (the per-function similarity,
 * gradients and Hessians over the two-pass kernels, with the scalars mirrored in TargetHost and d_ncc), and NCC on the fused path in the raw
 * moments the fused kernels accumulate (the algebra: mtfhip_sm_system.h): the host mirrors of one reduced row's scalars, the template's
 * moments, the deferred-fusion layer's outputs and cached Hessians.  SSIM's initializeSimilarity is NCC's (the same mean and centred sum)
 * (C-ABI implementation, include/mtfhip.h; shared declarations: mtfhip_api_internal.h; no CPU fallback: HIP kernels or an error)
 */
#include "mtfhip_api_internal.h"

extern "C" {

/* ------------------------------------------------------------------ per function (NCC's row of kAmOps) */
int push_ncc(mtfhip_batch *b) {
	std::vector<double> s(8 * (size_t)b->B, 0.0);
	for (int t = 0; t < b->B; ++t) {
		const TargetHost &h = b->th[t];
		double *p = &s[8 * t];
		p[0] = h.I0_mean; p[1] = h.c; p[2] = h.It_mean; p[3] = h.b; p[4] = h.f; p[5] = h.gmean; p[6] = h.i0_ss;
	}
	HIP_TRY(hipMemcpyAsync(b->d_ncc, s.data(), sizeof(double) * s.size(), hipMemcpyHostToDevice, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	return MTFHIP_OK;
}
static int ncc_mean_of(mtfhip_batch *b, int buf, double TargetHost::*dst) {
	int nblk = simple_blocks_per_target(b->N);
	{
		TimedScope ts(b->ctx, "ncc_stats");
		launch_vec_sum(b->view(), b->buf[buf], b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t) b->th[t].*dst = b->h_acc[(size_t)t * ACC_COUNT + ACC_RR] / (double)b->N;
	return MTFHIP_OK;
}
/* NCC::initializeSimilarity NCC.cc:55-95
 * (SSIM::initializeSimilarity SSIM.cc:50-76 keeps the template's mean and centred sum of squares, as NCC's does, and f = 1) */
int ncc_initialize_similarity(mtfhip_batch *b) {
	TRY(ncc_mean_of(b, MTFHIP_BUF_I0, &TargetHost::I0_mean));
	if (!b->init_sim)
		for (auto &h : b->th) h.It_mean = h.I0_mean;
	TRY(push_ncc(b));
	int nblk = simple_blocks_per_target(b->N);
	{
		TimedScope ts(b->ctx, "ncc_stats");
		launch_ncc_centered(b->view(), b->d_ncc, b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t) {
		TargetHost &h = b->th[t];
		h.i0_ss = b->h_acc[(size_t)t * ACC_COUNT + ACC_G + 2];   /* (SSIM's init_pix_var is this over N - 1, SSIM.cc:58) */
		h.c = std::sqrt(h.i0_ss);
		/* (SSIM::initializeSimilarity SSIM.cc:66-72: curr_pix_var = cross_pix_var = init_pix_var, f = 1 -- the system at It = I0) */
		if (!b->init_sim) { h.f = 1; h.b = h.c; if (ssim_am(b)) { h.it_ss = h.i0_ss; h.a = h.i0_ss; } }
	}
	return push_ncc(b);
}
/* NCC::updateSimilarity NCC.cc:124-161 (f is needed on the host whatever prereq_only says: the gradients read the scalars) */
int ncc_update_similarity(mtfhip_batch *b, int) {
	TRY(ncc_mean_of(b, MTFHIP_BUF_IT, &TargetHost::It_mean));
	TRY(push_ncc(b));
	int nblk = simple_blocks_per_target(b->N);
	{
		TimedScope ts(b->ctx, "ncc_stats");
		launch_ncc_centered(b->view(), b->d_ncc, b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t) {
		TargetHost &h = b->th[t];
		h.a = b->h_acc[(size_t)t * ACC_COUNT + ACC_G + 0];
		h.b = std::sqrt(b->h_acc[(size_t)t * ACC_COUNT + ACC_G + 1]);
		double bc = h.b * h.c;
		h.f = h.a / bc;
	}
	TRY(push_ncc(b));
	b->lz.df0_it_ver = b->lz.ver[MTFHIP_BUF_IT];
	return MTFHIP_OK;
}
/* which 0: NCC::updateInitGrad, 1: updateCurrGrad (NCC.cc:163-234) -- also what refreshes a gradient vector a fused launch skipped
 * (ensure_one, api_lazy.hip); 2: initializeGrad (NCC.cc:97-122) */
int ncc_grad(mtfhip_batch *b, int which) {
	if (which == 2) return zero_grad_vectors(b);
	if (b->ncc_host_newer) { TRY(push_ncc(b)); b->ncc_host_newer = false; }
	int nblk = simple_blocks_per_target(b->N);
	double *dst = b->buf[which ? MTFHIP_BUF_DF_DIT : MTFHIP_BUF_DF_DI0];
	{
		TimedScope ts(b->ctx, "ncc_grad");
		launch_ncc_grad(b->view(), b->d_ncc, which, dst, b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t) b->th[t].gmean = b->h_acc[(size_t)t * ACC_COUNT + ACC_RR] / (double)b->N;
	TRY(push_ncc(b));
	{
		TimedScope ts(b->ctx, "ncc_grad");
		launch_sub_mean(b->view(), dst, b->d_ncc, b->ctx->stream);
	}
	stale_clear(b, !which, which != 0);
	return MTFHIP_OK;
}
/* NCC::cmptInitHessian / cmptCurrHessian / cmptSelfHessian NCC.cc:282-389 (fast_hess = 0);
 * kind 0 init, 1 curr, 2 self.  H is column-major S x S per target. */
int ncc_hessian(mtfhip_batch *b, int j_buf, int kind, double *H) {
	if (ncc_hessian_from_cache(b, j_buf, kind, H)) return MTFHIP_OK;
	if (b->ncc_host_newer) { TRY(push_ncc(b)); b->ncc_host_newer = false; }
	const int S = b->S;
	int nblk = simple_blocks_per_target(b->N);
	{
		TimedScope ts(b->ctx, "ncc_hess");
		launch_col_sum(b->view(), b->buf[j_buf], b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_acc(b, nblk));
	std::vector<double> cm(8 * (size_t)b->B, 0.0);
	for (int t = 0; t < b->B; ++t)
		for (int s = 0; s < S; ++s) cm[8 * t + s] = b->h_acc[(size_t)t * ACC_COUNT + ACC_G + s] / (double)b->N;
	HIP_TRY(hipMemcpyAsync(b->d_colmean, cm.data(), sizeof(double) * cm.size(), hipMemcpyHostToDevice, b->ctx->stream));
	TRY(push_ncc(b));
	{
		TimedScope ts(b->ctx, "ncc_hess");
		launch_ncc_hess(b->view(), b->d_ncc, b->d_colmean, b->buf[j_buf], b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t) {
		const double *acc = b->h_acc + (size_t)t * ACC_COUNT;
		const double f = b->th[t].f;
		double *Ht = H + (size_t)t * S * S;
		int k = 0;
		for (int r = 0; r < 8; ++r)
			for (int c = r; c < 8; ++c) {
				if (r < S && c < S) {
					const double G = acc[ACC_H + k];
					const double ut_r = acc[ACC_G + r], ut_c = acc[ACC_G + c];
					const double u0_r = acc[ACC_G2 + r], u0_c = acc[ACC_G2 + c];
					double v;
					if (kind == 0) v = -f * G - ut_r * u0_c - u0_r * ut_c + 3 * u0_r * u0_c;
					else if (kind == 1) v = -f * G - ut_r * u0_c - u0_r * ut_c + 3 * ut_r * ut_c;
					else v = -G + ut_r * ut_c;
					Ht[c * S + r] = v; Ht[r * S + c] = v;
				}
				++k;
			}
	}
	return MTFHIP_OK;
}

/* ------------------------------------------------------------------ the fused path's raw moments */
/* the scalars of one target's NCC system (ncc_host_sys; mtfhip_sm_system.h has the formulas and their citations) are also what the host mirrors of NCC.cc's members (It_mean, b, a, f) hold after an iteration on these moments */
void ncc_refresh_mirrors(const mtfhip_batch *b, TargetHost &h, const double *M) {
	const NccSys q = ncc_host_sys(b, h, M);
	h.It_mean = q.mt; h.b = q.b; h.a = M[NCC_I0IT] - q.N * q.m0 * q.mt; h.f = q.f;
}
/* sum J0, sum I0 J0 and Gram(J0) of the template (after every change of J0) */
int ncc_template_moments(mtfhip_batch *b) {
	const int nblk = simple_blocks_per_target(b->N), S = b->S;
	{
		TimedScope ts(b->ctx, "ncc_hess");
		launch_col_sum(b->view(), b->buf[MTFHIP_BUF_J0], b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t)
		for (int s = 0; s < 8; ++s) b->th[t].ncc_tm[NCC_TM_SJ0 + s] = s < S ? b->h_acc[(size_t)t * ACC_COUNT + ACC_G + s] : 0.0;
	std::vector<double> g((size_t)b->B * S);
	TRY(gemv_to_host(b, b->buf[MTFHIP_BUF_I0], MTFHIP_BUF_J0, nullptr, -1, 0, g.data(), 0));
	for (int t = 0; t < b->B; ++t)
		for (int s = 0; s < 8; ++s) b->th[t].ncc_tm[NCC_TM_I0J0 + s] = s < S ? g[(size_t)t * S + s] : 0.0;
	{
		TimedScope ts(b->ctx, "gram");
		launch_gram(b->view(), b->buf[MTFHIP_BUF_J0], b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t) std::memcpy(b->th[t].ncc_tm + NCC_TM_GRAM0, b->h_acc + (size_t)t * ACC_COUNT + ACC_H, sizeof(double) * 36);
	/* device copy for the device-side finish (k_finish_track) */
	HIP_TRY(b->d_ncc_tm.reserve(NCC_TM_COUNT * (size_t)b->B));
	std::vector<double> tm((size_t)NCC_TM_COUNT * b->B);
	for (int t = 0; t < b->B; ++t) std::memcpy(&tm[NCC_TM_COUNT * (size_t)t], b->th[t].ncc_tm, sizeof(double) * NCC_TM_COUNT);
	HIP_TRY(hipMemcpyAsync(b->d_ncc_tm, tm.data(), sizeof(double) * tm.size(), hipMemcpyHostToDevice, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	return MTFHIP_OK;
}

/* deferred fusion, NCC: the AM-level Jacobian the trigger asked for, and the moment rows kept for the Hessian calls */
int ncc_lazy_outputs(mtfhip_batch *b, int trig, int j_a, bool hess_mean, double *g) {
	mtfhip_batch::Lazy &L = b->lz;
	const int S = b->S;
	for (int t = 0; t < b->B; ++t) {
		const double *M = b->h_acc + (size_t)t * NCC_ACC_COUNT;
		TargetHost &h = b->th[t];
		ncc_refresh_mirrors(b, h, M);
		const NccSys q = ncc_host_sys(b, h, M);
		double *o = g + (size_t)t * S;
		const int which = (trig == LAZY_CURR_JAC && j_a == MTFHIP_BUF_JM) ? NCC_JM : NCC_JT;
		for (int s = 0; s < S; ++s) {
			if (trig == LAZY_INIT_JAC) { o[s] = ncc_init_jac(q, NCC_J0, s); continue; }
			o[s] = ncc_curr_jac(q, which, s);
			if (trig == LAZY_DIFF_JAC) o[s] -= ncc_init_jac(q, NCC_J0, s);   /* (df_dIt . Jt) - (df_dI0 . J0), NCC.cc:268-280 */
		}
	}
	b->ncc_host_newer = true;
	if (!L.no_cache) {
		L.ncc_M.assign(b->h_acc.get(), b->h_acc + (size_t)NCC_ACC_COUNT * b->B);
		L.ncc_M_mean = hess_mean;
		L.ncc_M_it = L.ver[MTFHIP_BUF_IT]; L.ncc_M_jt = L.ver[MTFHIP_BUF_JT]; L.ncc_M_jm = L.ver[MTFHIP_BUF_JM];
	}
	return MTFHIP_OK;
}
/* 1 when H was produced from the cached moment rows; kind: NCC_H_INIT / _CURR / _SELF */
int ncc_hessian_from_cache(mtfhip_batch *b, int j_buf, int kind, double *H) {
	mtfhip_batch::Lazy &L = b->lz;
	if (L.no_cache || L.ncc_M.empty() || L.ncc_M_it != L.ver[MTFHIP_BUF_IT]) return 0;
	int which;
	if (j_buf == MTFHIP_BUF_J0) { if (L.ncc_tm_ver != L.ver[MTFHIP_BUF_J0]) return 0; which = NCC_J0; }
	else if (j_buf == MTFHIP_BUF_JT) { if (L.ncc_M_mean || L.ncc_M_jt != L.ver[MTFHIP_BUF_JT]) return 0; which = NCC_JT; }
	else { if (!L.ncc_M_mean || L.ncc_M_jm != L.ver[MTFHIP_BUF_JM] || L.ncc_M_jt != L.ver[MTFHIP_BUF_JT] || L.ncc_tm_ver != L.ver[MTFHIP_BUF_J0]) return 0; which = NCC_JM; }
	if (!ncc_has_gram(which, L.ncc_M_mean)) return 0;
	const int S = b->S;
	for (int t = 0; t < b->B; ++t) {
		const NccSys q = ncc_host_sys(b, b->th[t], &L.ncc_M[(size_t)t * NCC_ACC_COUNT]);
		for (int c = 0; c < S; ++c)
			for (int r = 0; r < S; ++r) H[(size_t)t * S * S + c * S + r] = ncc_hess(q, kind, which, r, c);
	}
	return 1;
}

} /* extern "C" */
