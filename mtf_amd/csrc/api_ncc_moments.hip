/*
 * api_ncc_moments.hip -- NCC on the fused path in the raw moments the fused kernels accumulate (the algebra: mtfhip_sm_system.h): the host mirrors of
 * one reduced row's scalars, the template's moments, the deferred-fusion layer's outputs and cached Hessians
 * (C-ABI implementation, include/mtfhip.h; shared declarations: mtfhip_api_internal.h; no CPU fallback: HIP kernels or an error)
 */
#include "mtfhip_api_internal.h"

extern "C" {

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
