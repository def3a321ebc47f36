/*
 * kernels_ssim.hip -- the Structural Similarity appearance model (AM/src/SSIM.cc) on the device.  Every quantity SSIM derives is a function
 * of the raw moments an NCC pass reduces (the algebra: mtfhip_sm_system.h, ssim_*), so the fused path launches NCC's pass kernels unchanged
 * (fused_select) and what is SSIM's own is here: the finish of the two-launch loop that reads those rows as SSIM does -- k_finish_track_ssim
 * and its low-order sibling, finish_track_body's SSIM form -- and the kernels behind the per-function AppearanceModel entry points:
 * updateSimilarity's three sums, updateCurrGrad / updateInitGrad, and one reduction of a pixel Jacobian's moments from which each of the
 * three first-order Hessians is assembled.  A translation unit of its own: the finish kernels of kernels_fused.hip stay what they were.
 */
#include "mtfhip_finish_kernel.h"

namespace mtfhip {

/* the finish over the rows of an NCC pass, read as SSIM (c1, c2: the model's constants, SSIM.cc:36-39): pivoting, both arithmetic modes of
 * the pass (api_track.hip leaves fast_finish off for it) */
__global__ __launch_bounds__(256) void k_finish_track_ssim(BatchView bv, mtfhip_sm_desc sm, TrackState ts,
	const double *partials, int nblk, PhaseCtl pc, HostPublish pub, int pub_t0, double c1, double c2) {
	finish_track_kernel<false, false, true>(bv, sm, ts, partials, nblk, pc, pub, pub_t0, c1, c2);
}
/* ... of a low-order SSM's batch (TrackState::lo_ssm): the projection of the affine system takes SSIM's entries as it takes NCC's */
__global__ __launch_bounds__(256) void k_finish_track_ssim_lo(BatchView bv, mtfhip_sm_desc sm, TrackState ts,
	const double *partials, int nblk, PhaseCtl pc, HostPublish pub, int pub_t0, double c1, double c2) {
	finish_track_kernel<true, false, true>(bv, sm, ts, partials, nblk, pc, pub, pub_t0, c1, c2);
}
void launch_finish_track_ssim(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts, const double *partials, int nblk,
	hipStream_t st, PhaseCtl pc, const HostPublish &pub, int pub_t0, double c1, double c2) {
	/* the rows are 72 wide: two waves load them, the first one solves; many block rows (a single large target): 240 lanes sum them */
	const dim3 block(nblk > 8 ? 256 : 128);
	if (ts.lo_ssm) MTFHIP_LAUNCH(k_finish_track_ssim_lo, dim3(bv.B), block, 0, st, bv, sm, ts, partials, nblk, pc, pub, pub_t0, c1, c2);
	else MTFHIP_LAUNCH(k_finish_track_ssim, dim3(bv.B), block, 0, st, bv, sm, ts, partials, nblk, pc, pub, pub_t0, c1, c2);
}

/* SSIM::updateSimilarity SSIM.cc:98-111 in raw moments: sum It, sum It^2, sum I0 It into ACC_G + 0 .. 2 of the block rows */
__global__ __launch_bounds__(kBlock) void k_ssim_similarity(BatchView bv, double *partials, int nblk) {
	__shared__ double lds[4 * 4];
	const int t = blockIdx.y, N = bv.N;
	const double *It = bv.buf[MTFHIP_BUF_IT] + (size_t)t * N;
	const double *I0 = bv.buf[MTFHIP_BUF_I0] + (size_t)t * N;
	double acc[4] = {0.0, 0.0, 0.0, 0.0};
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += nblk * kBlock) {
		const double a = I0[i], b = It[i];
		acc[0] += b; acc[1] += b * b; acc[2] += a * b;
	}
	block_reduce_store<4>(acc, partials + ((size_t)t * nblk + blockIdx.x) * ACC_COUNT + ACC_G, lds);
}

/* SSIM::updateCurrGrad / updateInitGrad SSIM.cc:113-142: out = mult_factor (a (Io - mo) - f c (Iu - mu)) + grad_scal, Io the other image and
 * Iu the one the gradient is taken in; sc: [B][8] = mo, mu, mult_factor, a, f c, grad_scal of each target */
__global__ __launch_bounds__(kBlock) void k_ssim_grad(int N, const double *sc, const double *Io, const double *Iu, double *out) {
	const int t = blockIdx.y;
	const double *s = sc + 8 * (size_t)t;
	const double mo = s[0], mu = s[1], mult = s[2], a = s[3], fc = s[4], gs = s[5];
	const size_t base = (size_t)t * N;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock)
		out[base + i] = mult * (a * (Io[base + i] - mo) - fc * (Iu[base + i] - mu)) + gs;
}

/* the moments of a pixel Jacobian X the three first-order Hessians are functions of (SSIM.cc:144-287), in the slots an NCC pass gives its Jt:
 * Gram(X) | sum X | sum It X | sum I0 X, and sum It, sum It^2, sum I0 It -- one 72-wide row per block, the slots it has nothing for zero */
__global__ __launch_bounds__(kBlock) void k_ssim_hess(BatchView bv, const double *J_all, double *partials, int nblk) {
	__shared__ double lds[4 * NCC_ACC_COUNT];
	const int t = blockIdx.y, N = bv.N, S = bv.S;
	const double *J = J_all + (size_t)t * N * S;
	const double *It = bv.buf[MTFHIP_BUF_IT] + (size_t)t * N;
	const double *I0 = bv.buf[MTFHIP_BUF_I0] + (size_t)t * N;
	double acc[NCC_ACC_COUNT];
#pragma unroll
	for (int k = 0; k < NCC_ACC_COUNT; ++k) acc[k] = 0.0;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += nblk * kBlock) {
		const double a = I0[i], b = It[i];
		double r[kMaxS];
#pragma unroll
		for (int s = 0; s < kMaxS; ++s) r[s] = s < S ? J[(size_t)s * N + i] : 0.0;
		int k = 0;
#pragma unroll
		for (int p = 0; p < kMaxS; ++p) {
#pragma unroll
			for (int q = p; q < kMaxS; ++q) { acc[NCC_GRAM + k] += r[p] * r[q]; ++k; }
		}
#pragma unroll
		for (int s = 0; s < kMaxS; ++s) { acc[NCC_SJ + s] += r[s]; acc[NCC_ITJ + s] += b * r[s]; acc[NCC_I0J + s] += a * r[s]; }
		acc[NCC_IT] += b; acc[NCC_IT2] += b * b; acc[NCC_I0IT] += a * b;
	}
	block_reduce_store<NCC_ACC_COUNT>(acc, partials + ((size_t)t * nblk + blockIdx.x) * NCC_ACC_COUNT, lds);
}

void launch_ssim_similarity(const BatchView &bv, double *partials, int nblk, hipStream_t st) {
	MTFHIP_LAUNCH(k_ssim_similarity, grid2(nblk, bv.B), dim3(kBlock), 0, st, bv, partials, nblk);
}
void launch_ssim_grad(const BatchView &bv, const double *sc, int curr, double *out, hipStream_t st) {
	const int blocks = std::min((bv.N + kBlock - 1) / kBlock, 1024);
	const double *I0 = bv.buf[MTFHIP_BUF_I0], *It = bv.buf[MTFHIP_BUF_IT];
	MTFHIP_LAUNCH(k_ssim_grad, grid2(blocks, bv.B), dim3(kBlock), 0, st, bv.N, sc, curr ? I0 : It, curr ? It : I0, out);
}
void launch_ssim_hess(const BatchView &bv, const double *J, double *partials, int nblk, hipStream_t st) {
	MTFHIP_LAUNCH(k_ssim_hess, grid2(nblk, bv.B), dim3(kBlock), 0, st, bv, J, partials, nblk);
}

} // namespace mtfhip
