/*
 * kernels_spss.hip -- the Sum of Pixelwise Structural Similarity appearance model (AM/src/SPSS.cc) behind the per-function AppearanceModel
 * entry points: updateSimilarity's f_vec and its sum, updateCurrGrad / updateInitGrad, and the three first-order Hessians, which are
 * per-pixel WEIGHTED Gram matrices of a pixel Jacobian.  The reference's expressions with IEEE divisions in its order (the library is
 * compiled without contraction); the vectors it keeps beside I0 and It (I0_sqr, It_sqr, f_vec_den, f_vec) are recomputed from the two
 * buffers, df_dIt / df_dI0 are read from theirs where the reference reads its members.  The fused pass: kernels_fused_spss.hip.
 */
#include "mtfhip_device.h"

namespace mtfhip {

/* SPSS::updateSimilarity SPSS.cc:116-123: f_vec = (2 I0 It + c) / (I0^2 + It^2 + c), f = f_vec.sum() */
__global__ __launch_bounds__(kBlock) void k_spss_similarity(BatchView bv, double c, double *partials, int nblk) {
	__shared__ double lds[4 * 1];
	const int t = blockIdx.y, N = bv.N;
	const double *It = bv.buf[MTFHIP_BUF_IT] + (size_t)t * N;
	const double *I0 = bv.buf[MTFHIP_BUF_I0] + (size_t)t * N;
	double acc[1] = {0.0};
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += nblk * kBlock) {
		const double a = I0[i], b = It[i];
		const double den = (a * a + b * b) + c;
		acc[0] += (2 * a * b + c) / den;
	}
	block_reduce_store<1>(acc, partials + ((size_t)t * nblk + blockIdx.x) * ACC_COUNT + ACC_RR, lds);
}

/* SPSS::updateCurrGrad SPSS.cc:149-150: df_dIt = 2 (I0 - f_vec It) / f_vec_den; SPSS::updateInitGrad SPSS.cc:134-138:
 * df_dI0 = 2 (It (It^2 - I0^2) + c (It - 2 I0)) / f_vec_den^2 (not the derivative of f_vec in I0, which has c (It - I0): kept as written) */
__global__ __launch_bounds__(kBlock) void k_spss_grad(double c, int curr, const double *I0, const double *It, double *out, size_t n) {
	for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
		const double a = I0[i], b = It[i];
		const double a2 = a * a, b2 = b * b;
		const double den = (a2 + b2) + c;
		if (curr) {
			const double fv = (2 * a * b + c) / den;
			out[i] = 2 * (a - fv * b) / den;
		} else {
			out[i] = 2 * (b * (b2 - a2) + c * (b - 2 * a)) / (den * den);
		}
	}
}

/* SPSS::cmptSelfHessian SPSS.cc:221-225 (w = -2 / (2 It^2 + c)), cmptCurrHessian :191-196 (w = -2 (f_vec + 3 df_dIt It) / f_vec_den),
 * cmptInitHessian :160-165 (w = -2 (f_vec + I0 df_dI0) / f_vec_den): upper triangle of sum_i w_i J[i, a] J[i, b] into ACC_H */
__global__ __launch_bounds__(kBlock) void k_spss_hessian(BatchView bv, double c, int weight, const double *J_all, double *partials, int nblk) {
	__shared__ double lds[4 * 36];
	const int t = blockIdx.y, N = bv.N, S = bv.S;
	const double *J = J_all + (size_t)t * N * S;
	const double *It = bv.buf[MTFHIP_BUF_IT] + (size_t)t * N;
	const double *I0 = bv.buf[MTFHIP_BUF_I0] + (size_t)t * N;
	const double *dft = bv.buf[MTFHIP_BUF_DF_DIT] + (size_t)t * N;
	const double *df0 = bv.buf[MTFHIP_BUF_DF_DI0] + (size_t)t * N;
	double acc[36];
#pragma unroll
	for (int k = 0; k < 36; ++k) acc[k] = 0.0;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += nblk * kBlock) {
		const double a = I0[i], b = It[i];
		const double b2 = b * b;
		double w;
		if (weight == SPSS_W_SELF) w = -2 / (2 * b2 + c);
		else if (weight == SPSS_W_SELF0) w = -2 / (2 * (a * a) + c);   /* the template's own: initializeSimilarity's It_sqr = I0_sqr (SPSS.cc:95-96) */
		else {
			const double den = (a * a + b2) + c;
			const double fv = (2 * a * b + c) / den;
			w = weight == SPSS_W_CURR ? -2 * (fv + 3 * dft[i] * b) / den : -2 * (fv + a * df0[i]) / den;
		}
		double r[kMaxS];
#pragma unroll
		for (int s = 0; s < kMaxS; ++s) r[s] = s < S ? J[(size_t)s * N + i] : 0.0;
		int k = 0;
#pragma unroll
		for (int p = 0; p < kMaxS; ++p) {
			const double wp = w * r[p];
#pragma unroll
			for (int q = p; q < kMaxS; ++q) { acc[k] = fma(wp, r[q], acc[k]); ++k; }
		}
	}
	block_reduce_store<36>(acc, partials + ((size_t)t * nblk + blockIdx.x) * ACC_COUNT + ACC_H, lds);
}

void launch_spss_similarity(const BatchView &bv, double c, double *partials, int nblk, hipStream_t st) {
	MTFHIP_LAUNCH(k_spss_similarity, grid2(nblk, bv.B), dim3(kBlock), 0, st, bv, c, partials, nblk);
}
void launch_spss_grad(const BatchView &bv, double c, int curr, double *out, hipStream_t st) {
	const size_t n = (size_t)bv.N * bv.B;
	const unsigned blocks = (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, 4096);
	MTFHIP_LAUNCH(k_spss_grad, dim3(blocks), dim3(kBlock), 0, st, c, curr, bv.buf[MTFHIP_BUF_I0], bv.buf[MTFHIP_BUF_IT], out, n);
}
void launch_spss_hessian(const BatchView &bv, double c, int weight, const double *J, double *partials, int nblk, hipStream_t st) {
	MTFHIP_LAUNCH(k_spss_hessian, grid2(nblk, bv.B), dim3(kBlock), 0, st, bv, c, weight, J, partials, nblk);
}

} // namespace mtfhip
