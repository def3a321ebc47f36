/*
 * api_ncc_moments.hip -- NCC on the fused path in the raw moments the fused kernels accumulate: the search methods' f, g and H of one reduced row, the
 * template's moments, the deferred-fusion layer's outputs and cached Hessians
 * (C-ABI implementation, include/mtfhip.h; shared declarations: mtfhip_api_internal.h; no CPU fallback: HIP kernels or an error)
 */
#include "mtfhip_api_internal.h"

extern "C" {

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
struct NccX { const double *gram; double s[8], it[8], i0[8]; };
struct NccScalars { double N, mt, m0, b, b2, c, f; };
static void ncc_vecs(const NccScalars &q, const NccX &X, int S, double *ut, double *u0) {
	for (int s = 0; s < S; ++s) {
		ut[s] = (X.it[s] - q.mt * X.s[s]) / q.b2;
		u0[s] = (X.i0[s] - q.m0 * X.s[s]) / (q.b * q.c);
	}
}
/* kind 0 init, 1 curr, 2 self; H column-major S x S */
static void ncc_hess_from_moments(const NccScalars &q, const NccX &X, int S, int kind, double *H) {
	double ut[8], u0[8];
	ncc_vecs(q, X, S, ut, u0);
	for (int r = 0; r < S; ++r)
		for (int c = 0; c < S; ++c) {
			const int a = r < c ? r : c, d = r < c ? c : r;
			const double G = -(X.gram[a * 8 - (a * (a - 1)) / 2 + (d - a)] - X.s[r] * X.s[c] / q.N) / q.b2;
			double v;
			if (kind == 2) v = G + ut[r] * ut[c];
			else v = q.f * G - ut[r] * u0[c] - u0[r] * ut[c] + 3 * (kind == 1 ? ut[r] * ut[c] : u0[r] * u0[c]);
			H[c * S + r] = v;
		}
}
static NccScalars ncc_scalars(const mtfhip_batch *b, const TargetHost &h, const double *M) {
	NccScalars q;
	q.N = (double)b->N; q.mt = M[NCC_IT] / q.N; q.m0 = h.I0_mean; q.c = h.c;
	const double a = M[NCC_I0IT] - q.N * q.m0 * q.mt;
	q.b2 = M[NCC_IT2] - q.N * q.mt * q.mt; q.b = std::sqrt(q.b2);
	q.f = a / (q.b * q.c);
	return q;
}
/* ... which are also what the host mirrors of NCC.cc's members (It_mean, b, a, f) hold after an iteration on these moments */
void ncc_refresh_mirrors(const mtfhip_batch *b, TargetHost &h, const double *M) {
	const NccScalars q = ncc_scalars(b, h, M);
	h.It_mean = q.mt; h.b = q.b; h.a = M[NCC_I0IT] - q.N * q.m0 * q.mt; h.f = q.f;
}
static void ncc_x(const mtfhip_batch *b, const TargetHost &h, const double *M, int which /* 0 J0, 1 Jt, 2 Jm */, bool gram_is_mean, NccX &X) {
	const int S = b->S;
	for (int s = 0; s < 8; ++s) X.s[s] = X.it[s] = X.i0[s] = 0;
	for (int s = 0; s < S; ++s) {
		const double s0 = h.ncc_sj0[s], it0 = M[NCC_ITJ0 + s], i00 = h.ncc_i0j0[s];
		const double st = M[NCC_SJ + s], itt = M[NCC_ITJ + s], i0t = M[NCC_I0J + s];
		if (which == 0) { X.s[s] = s0; X.it[s] = it0; X.i0[s] = i00; }
		else if (which == 1) { X.s[s] = st; X.it[s] = itt; X.i0[s] = i0t; }
		else { X.s[s] = (s0 + st) / 2; X.it[s] = (it0 + itt) / 2; X.i0[s] = (i00 + i0t) / 2; }
	}
	X.gram = which == 0 ? h.ncc_gram0 : ((which == 2) == gram_is_mean ? M + NCC_GRAM : nullptr);
}
/* one target's reduced moment row -> the SM's f, g, H (before LM damping); NT/ESM.cc:298-377, NT/FCLK.cc:260-288, NT/ICLK.cc:206-251 */
int ncc_assemble(const mtfhip_batch *b, const mtfhip_sm_desc *sm, bool hess_mean, const double *M, TargetHost &h,
	double *f, double *g, double *H) {
	const int S = b->S;
	ncc_refresh_mirrors(b, h, M);
	const NccScalars q = ncc_scalars(b, h, M);
	if (f) *f = q.f;
	NccX X0, Xt, Xm;
	ncc_x(b, h, M, 0, hess_mean, X0); ncc_x(b, h, M, 1, hess_mean, Xt); ncc_x(b, h, M, 2, hess_mean, Xm);
	double ut[8], u0[8];
	auto curr_jac = [&](const NccX &X, double *o) { ncc_vecs(q, X, S, ut, u0); for (int s = 0; s < S; ++s) o[s] = u0[s] - q.f * ut[s]; };
	auto init_jac = [&](const NccX &X, double *o) { ncc_vecs(q, X, S, ut, u0); for (int s = 0; s < S; ++s) o[s] = (q.b / q.c) * (ut[s] - q.f * u0[s]); };
	if (sm->sm == MTFHIP_SM_FCLK) curr_jac(Xt, g);
	else if (sm->sm == MTFHIP_SM_ICLK) init_jac(X0, g);
	else if (sm->jac_type == 0) curr_jac(Xm, g);
	else { double gt[8], g0[8]; curr_jac(Xt, gt); init_jac(X0, g0); for (int s = 0; s < S; ++s) g[s] = 0.5 * (gt[s] - g0[s]); }
	const int ht = sm->hess_type;
	auto need = [&](const NccX &X) { return X.gram ? MTFHIP_OK : fail(MTFHIP_ERR_LOGIC, "fused NCC: the Gram matrix this Hessian needs was not accumulated"); };
	if (ht == 0) { std::memcpy(H, h.h0, sizeof(double) * S * S); return MTFHIP_OK; }
	if (sm->sm == MTFHIP_SM_ICLK) { ncc_hess_from_moments(q, X0, S, 0, H); return MTFHIP_OK; }   /* Std: cmptInitHessian(J0) */
	if (sm->sm == MTFHIP_SM_FCLK || ht == 1 || ht == 5) { TRY(need(Xt)); ncc_hess_from_moments(q, Xt, S, ht == 1 ? 2 : 1, H); return MTFHIP_OK; }
	if (ht == 2) {   /* SumOfSelf */
		TRY(need(Xt)); ncc_hess_from_moments(q, Xt, S, 2, H);
		for (int k = 0; k < S * S; ++k) H[k] = 0.5 * (H[k] + h.h0[k]);
		return MTFHIP_OK;
	}
	if (ht == 3) { TRY(need(Xm)); ncc_hess_from_moments(q, Xm, S, 1, H); return MTFHIP_OK; }   /* Original: cmptCurrHessian(mean) */
	/* SumOfStd: (cmptInitHessian(J0) + cmptCurrHessian(Jt)) / 2 */
	TRY(need(Xt));
	double Hi[64];
	ncc_hess_from_moments(q, X0, S, 0, Hi); ncc_hess_from_moments(q, Xt, S, 1, H);
	for (int k = 0; k < S * S; ++k) H[k] = 0.5 * (H[k] + Hi[k]);
	return MTFHIP_OK;
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
		for (int s = 0; s < 8; ++s) b->th[t].ncc_sj0[s] = s < S ? b->h_acc[(size_t)t * ACC_COUNT + ACC_G + s] : 0.0;
	std::vector<double> g((size_t)b->B * S);
	TRY(gemv_to_host(b, b->buf[MTFHIP_BUF_I0], MTFHIP_BUF_J0, nullptr, -1, 0, g.data(), 0));
	for (int t = 0; t < b->B; ++t)
		for (int s = 0; s < 8; ++s) b->th[t].ncc_i0j0[s] = s < S ? g[(size_t)t * S + s] : 0.0;
	{
		TimedScope ts(b->ctx, "gram");
		launch_gram(b->view(), b->buf[MTFHIP_BUF_J0], b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t) std::memcpy(b->th[t].ncc_gram0, b->h_acc + (size_t)t * ACC_COUNT + ACC_H, sizeof(double) * 36);
	/* device copy for the device-side finish (k_finish_track) */
	HIP_TRY(b->d_ncc_tm.reserve(52 * (size_t)b->B));
	std::vector<double> tm((size_t)52 * b->B);
	for (int t = 0; t < b->B; ++t) {
		std::memcpy(&tm[52 * (size_t)t], b->th[t].ncc_sj0, sizeof(double) * 8);
		std::memcpy(&tm[52 * (size_t)t + 8], b->th[t].ncc_i0j0, sizeof(double) * 8);
		std::memcpy(&tm[52 * (size_t)t + 16], b->th[t].ncc_gram0, sizeof(double) * 36);
	}
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
		const NccScalars q = ncc_scalars(b, h, M);
		NccX X;
		double ut[8], u0[8], *o = g + (size_t)t * S;
		if (trig == LAZY_INIT_JAC) {
			ncc_x(b, h, M, 0, hess_mean, X); ncc_vecs(q, X, S, ut, u0);
			for (int s = 0; s < S; ++s) o[s] = (q.b / q.c) * (ut[s] - q.f * u0[s]);
		} else {
			ncc_x(b, h, M, (trig == LAZY_CURR_JAC && j_a == MTFHIP_BUF_JM) ? 2 : 1, hess_mean, X); ncc_vecs(q, X, S, ut, u0);
			for (int s = 0; s < S; ++s) o[s] = u0[s] - q.f * ut[s];
			if (trig == LAZY_DIFF_JAC) {   /* (df_dIt . Jt) - (df_dI0 . J0), NCC.cc:268-280 */
				ncc_x(b, h, M, 0, hess_mean, X); ncc_vecs(q, X, S, ut, u0);
				for (int s = 0; s < S; ++s) o[s] -= (q.b / q.c) * (ut[s] - q.f * u0[s]);
			}
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
/* 1 when H was produced from the cached moment rows */
int ncc_hessian_from_cache(mtfhip_batch *b, int j_buf, int kind, double *H) {
	mtfhip_batch::Lazy &L = b->lz;
	if (L.no_cache || L.ncc_M.empty() || L.ncc_M_it != L.ver[MTFHIP_BUF_IT]) return 0;
	int which;
	if (j_buf == MTFHIP_BUF_J0) { if (L.ncc_tm_ver != L.ver[MTFHIP_BUF_J0]) return 0; which = 0; }
	else if (j_buf == MTFHIP_BUF_JT) { if (L.ncc_M_mean || L.ncc_M_jt != L.ver[MTFHIP_BUF_JT]) return 0; which = 1; }
	else { if (!L.ncc_M_mean || L.ncc_M_jm != L.ver[MTFHIP_BUF_JM] || L.ncc_M_jt != L.ver[MTFHIP_BUF_JT] || L.ncc_tm_ver != L.ver[MTFHIP_BUF_J0]) return 0; which = 2; }
	for (int t = 0; t < b->B; ++t) {
		const double *M = &L.ncc_M[(size_t)t * NCC_ACC_COUNT];
		const NccScalars q = ncc_scalars(b, b->th[t], M);
		NccX X;
		ncc_x(b, b->th[t], M, which, L.ncc_M_mean, X);
		if (!X.gram) return 0;
		ncc_hess_from_moments(q, X, b->S, kind, H + (size_t)t * b->S * b->S);
	}
	return 1;
}

} /* extern "C" */
