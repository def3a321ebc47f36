/*
 * api_ssim.hip -- the Structural Similarity appearance model's own state (AM/src/SSIM.cc): its parameters k1 and k2, the constant self Hessian
 * from the template's moments, and the per-function similarity, gradients and Hessians.  The fused entry points run NCC's pass kernels and
 * read their rows through ssim_sys / ssim_g / ssim_h (mtfhip_sm_system.h): on the host in assemble_rows (api_fused.hip), on the device in
 * k_finish_track_ssim.
 * (C-ABI implementation, include/mtfhip.h; the kernels: kernels_ssim.hip; no CPU fallback: HIP kernels or an error)
 */
#include "mtfhip_api_internal.h"

/* cmptSelfHessian(J0) at It = I0 (SSIM.cc:270-287; NT/ESM.cc:133-141, NT/FCLK.cc:120-128, NT/ICLK.cc:96-118) from th[].ncc_tm, column-major S x S */
int ssim_h0(const mtfhip_batch *b, double *H0) {
	const int S = b->S;
	for (int t = 0; t < b->B; ++t) {
		const TargetHost &h = b->th[t];
		const SsimSys q = ssim_sys_template(h.ncc_tm, h.I0_mean, h.i0_ss, (double)b->N, b->ssim_c1, b->ssim_c2);
		for (int c = 0; c < S; ++c)
			for (int r = 0; r < S; ++r) H0[(size_t)t * S * S + c * S + r] = ssim_hess(q, NCC_H_SELF, NCC_J0, r, c);
	}
	return MTFHIP_OK;
}

/* the system of the mirrors a similarity update left (mean and centred sums of It): what updateCurrGrad / updateInitGrad read */
static SsimSys ssim_mirror_sys(const mtfhip_batch *b, const TargetHost &h) {
	return ssim_sys_of(nullptr, nullptr, h.I0_mean, h.i0_ss, (double)b->N, b->ssim_c1, b->ssim_c2, h.It_mean, h.it_ss, h.a);
}

/* SSIM::updateSimilarity SSIM.cc:98-111.  The reference computes f whatever prereq_only says, and the gradients need the scalars on the
 * host: prereq_only changes nothing here either */
int ssim_update_similarity(mtfhip_batch *b, int prereq_only) {
	(void)prereq_only;
	const int nblk = simple_blocks_per_target(b->N);
	{
		TimedScope ts(b->ctx, "ssim_similarity");
		launch_ssim_similarity(b->view(), b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_acc(b, nblk));
	const double N = (double)b->N;
	for (int t = 0; t < b->B; ++t) {
		TargetHost &h = b->th[t];
		const double *s = b->h_acc + (size_t)t * ACC_COUNT + ACC_G;
		h.It_mean = s[0] / N;
		h.it_ss = s[1] - N * h.It_mean * h.It_mean;
		h.a = s[2] - N * h.I0_mean * h.It_mean;
		h.f = ssim_mirror_sys(b, h).f;
	}
	b->ncc_host_newer = true;
	return MTFHIP_OK;
}
/* which 1 / 0: SSIM::updateCurrGrad / updateInitGrad SSIM.cc:113-142 into DF_DIT / DF_DI0; 2: initializeGrad (SSIM.cc:78-96) */
int ssim_update_grad(mtfhip_batch *b, int curr) {
	if (curr == 2) return zero_grad_vectors(b);
	std::vector<double> sc(8 * (size_t)b->B, 0.0);
	for (int t = 0; t < b->B; ++t) {
		const SsimSys q = ssim_mirror_sys(b, b->th[t]);
		double *p = &sc[8 * (size_t)t];
		p[0] = curr ? q.m0 : q.mt; p[1] = curr ? q.mt : q.m0; p[2] = q.mu; p[3] = q.a; p[4] = q.f * q.c; p[5] = curr ? q.gs_t : q.gs_0;
	}
	HIP_TRY(hipMemcpyAsync(b->d_colmean, sc.data(), sizeof(double) * sc.size(), hipMemcpyHostToDevice, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));   /* (sc is this call's) */
	TimedScope ts(b->ctx, "ssim_grad");
	launch_ssim_grad(b->view(), b->d_colmean, curr, b->buf[curr ? MTFHIP_BUF_DF_DIT : MTFHIP_BUF_DF_DI0], b->ctx->stream);
	return MTFHIP_OK;
}
/* SSIM::cmptInitHessian / cmptCurrHessian / cmptSelfHessian SSIM.cc:144-287 over any Jacobian buffer: one reduction of its moments beside the
 * current patch's (k_ssim_hess), then ssim_hess entry by entry -- the row stands where an NCC pass's stands, the buffer where its Jt does */
static_assert(NCC_H_INIT == 0 && NCC_H_CURR == 1 && NCC_H_SELF == 2, "kind 0 init, 1 curr, 2 self, as every model's Hessian takes it");
int ssim_hessian(mtfhip_batch *b, int j_buf, int kind, double *H) {
	const int nblk = simple_blocks_per_target(b->N), S = b->S;
	{
		TimedScope ts(b->ctx, "ssim_hess");
		launch_ssim_hess(b->view(), b->buf[j_buf], b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_rows(b, nblk, NCC_ACC_COUNT));
	for (int t = 0; t < b->B; ++t) {
		const TargetHost &h = b->th[t];
		const SsimSys q = ssim_sys(b->h_acc + (size_t)t * NCC_ACC_COUNT, nullptr, h.I0_mean, h.i0_ss, (double)b->N, b->ssim_c1, b->ssim_c2);
		for (int c = 0; c < S; ++c)
			for (int r = 0; r < S; ++r) H[(size_t)t * S * S + c * S + r] = ssim_hess(q, kind, NCC_JT, r, c);
	}
	return MTFHIP_OK;
}

extern "C" {

int mtfhip_batch_set_ssim(mtfhip_batch *b, double k1, double k2) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "set_ssim: NULL batch");
	if (!ssim_am(b)) return fail(MTFHIP_ERR_INVALID_ARG, "set_ssim: the batch's appearance model is %d, not SSIM", b->desc.am);
	if (b->init_pix_vals || b->init_sim)
		return fail(MTFHIP_ERR_LOGIC, "set_ssim: k1 and k2 are fixed once the template is initialised (call it before init_template / initialize_similarity)");
	if (!std::isfinite(k1) || !std::isfinite(k2)) return fail(MTFHIP_ERR_INVALID_ARG, "set_ssim: k1 / k2 is not a finite number");
	const double a1 = k1 > 0 ? k1 : 0.01, a2 = k2 > 0 ? k2 : 0.03;
	/* SSIM.cc:36-39: c1 = k1 (PIX_MAX - PIX_MIN); c1 *= c1; c2 likewise */
	double c1 = a1 * (255.0 - 0.0), c2 = a2 * (255.0 - 0.0);
	c1 *= c1; c2 *= c2;
	/* c1 and c2 keep c = mt^2 + m0^2 + c1 and d = vt + v0 + c2 away from zero on black or flat patches */
	if (!std::isnormal(c1) || !std::isnormal(c2))
		return fail(MTFHIP_ERR_INVALID_ARG, "set_ssim: k1 = %g, k2 = %g give c1 = %g, c2 = %g, which are not both normal numbers", a1, a2, c1, c2);
	b->ssim_k1 = a1; b->ssim_k2 = a2;
	b->ssim_c1 = c1; b->ssim_c2 = c2;
	return MTFHIP_OK;
}

} /* extern "C" */
