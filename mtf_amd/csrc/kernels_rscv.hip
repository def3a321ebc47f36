/*
 * kernels_rscv.hip -- the Reversed SCV appearance model (AM/src/RSCV.cc): the intensity map RSCV::updatePixVals builds from the current
 * patch (RSCV.cc:170-238).  RSCV is SSD on It = map(It_orig); the map is applied inside the fused pass (kernels_fused_rscv.hip) or, on
 * the per-function path, by k_rscv_apply.
 *
 *   k_rscv_codes  (init)  per pixel of I0: (int)I0, the template's column of the joint histogram -- fixed until the template changes
 *   k_rscv_hist   pass 1  It_orig (sampled at the current warp with the arithmetic of the fused pass that follows, or read from the
 *                         It_orig buffer on the per-function path) and the two sums per CURRENT bin the map needs:
 *                           map[b] = sum_j j joint(b, j) / curr_hist(b)  needs only  sum over the pixels of bin (int)It_orig of (int)I0,
 *                         and their count, so the n_bins^2 joint histogram never exists.  LDS u32 atomics per workgroup, one row of
 *                         2 n_bins sums per workgroup; the last workgroup of a target to arrive sums the rows into 64-bit integers and
 *                         writes the map with the reference's division and its empty-bin rule (map[b] = b where curr_hist(b) == 0).
 *                         Reads 16 B/px (grid point) + 4 texels + 1 B/px (code plane).
 *   k_rscv_apply          It = map(It_orig), nearest or linear (per-function path)
 *
 * Reproducibility.  Every sum is an integer, exact in any order (u32 per workgroup: at most 255 x 2^26 / 64 < 2^32 per bin; u64 across
 * workgroups), and stays exact as a double; the map is identical run to run.
 * Bin agreement.  A pixel must fall in the bin of the histogram the fused pass looks it up in, so pass 1 evaluates It_orig exactly as the
 * fused pass it runs in front of does (mtfhip_fused_device.h: issue_tex + row_compute): the replay expression for MATH_REPLAY and every
 * materialising launch; for the lean tolerance-mode launches the FMA warp, the same interior-cell test of the same 64-pixel wave (the
 * fused pass walks a target's pixels in rows of 256 starting at multiples of 256, so wave w of a row holds pixels [64 k, 64 k + 64)),
 * the closed-form interpolant when the whole wave is interior and the reference's sampler otherwise.
 */
#include "mtfhip_rscv_device.h"

namespace mtfhip {

__global__ __launch_bounds__(kBlock) void k_rscv_codes(int N, int nb, const double *i0, unsigned char *code) {
	const int t = blockIdx.y;
	const double *x = i0 + (size_t)t * N;
	unsigned char *c = code + (size_t)t * N;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
		int lo = (int)x[i];
		lo = lo < 0 ? 0 : (lo > nb - 1 ? nb - 1 : lo);
		c[i] = (unsigned char)lo;
	}
}

template <int SSM, int KIND>
__global__ __launch_bounds__(kBlock) void k_rscv_hist(BatchView bv, ImgView im, RscvArgs a, int nblk) {
	__shared__ unsigned s_sum[kRscvMaxBins], s_cnt[kRscvMaxBins];
	__shared__ int s_last;
	const int t = blockIdx.y;
	if (a.active && !a.active[t]) return;   /* (uniform over the target's workgroups: nobody counts itself in) */
	const int N = bv.N, nb = a.nb;
	const double2 *ip = reinterpret_cast<const double2 *>(bv.buf[bv.unit_z ? MTFHIP_BUF_INIT_PTS : MTFHIP_BUF_INIT_HXY]) + (size_t)t * N;
	const double *iz = bv.buf[MTFHIP_BUF_INIT_Z] + (size_t)t * N;
	const double *ito = a.it_orig ? a.it_orig + (size_t)t * N : nullptr;
	const unsigned char *code = a.code + (size_t)t * N;
	Warp9 W;
	if constexpr (KIND != RSCV_IT_FROM_BUF) W = load_warp(bv.warps + 9 * t);
	for (int b = threadIdx.x; b < kRscvMaxBins; b += kBlock) { s_sum[b] = 0u; s_cnt[b] = 0u; }
	__syncthreads();
	/* 256-pixel chunks at multiples of 256: a wave holds the 64 pixels a wave of the fused pass holds */
	const int n_chunks = (N + kBlock - 1) / kBlock;
	for (int ch = blockIdx.x; ch < n_chunks; ch += nblk) {
		const int i = ch * kBlock + threadIdx.x;
		if (i < N) {
			double itv;
			if constexpr (KIND == RSCV_IT_FROM_BUF) {
				itv = ito[i];
			} else {
				const double2 p = ip[i];
				const double z = bv.unit_z ? 1.0 : iz[i];
				itv = rscv_it_orig<SSM, KIND>(im, W, a, p.x, p.y, z);
			}
			/* getDiracJointHist (histUtils.cc:370-394): joint((int)It_orig, (int)I0) += 1, curr_hist((int)It_orig) += 1 */
			int bt = (int)itv;
			bt = bt < 0 ? 0 : (bt > nb - 1 ? nb - 1 : bt);
			atomicAdd(&s_sum[bt], (unsigned)code[i]);
			atomicAdd(&s_cnt[bt], 1u);
		}
	}
	__syncthreads();
	unsigned *part = a.part + (size_t)t * nblk * 2 * nb;
	unsigned *row = part + (size_t)blockIdx.x * 2 * nb;
	for (int b = threadIdx.x; b < nb; b += kBlock) { st_coh(row + b, s_sum[b]); st_coh(row + nb + b, s_cnt[b]); }
	/* the last workgroup of the target to arrive builds the map (kernels_step.hip's hand-over: write-through rows, acknowledged, then an
	 * agent-scope arrival) */
	wait_stores_acked();
	__syncthreads();
	if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(a.arrive + t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nblk - 1u;
	__syncthreads();
	if (!s_last) return;
	if (threadIdx.x == 0) st_coh(a.arrive + t, 0u);
	/* RSCV::updatePixVals RSCV.cc:211-229: intensity_map(b) = sum_j j joint(b, j) / curr_hist(b), or b where curr_hist(b) == 0 */
	for (int b = threadIdx.x; b < nb; b += kBlock) {
		unsigned long long s = 0, c = 0;
		for (int k0 = 0; k0 < nblk; k0 += 8) {
			unsigned vs[8], vc[8];
#pragma unroll
			for (int j = 0; j < 8; ++j) {
				const bool in = k0 + j < nblk;
				const unsigned *r = part + (size_t)(in ? k0 + j : 0) * 2 * nb;
				vs[j] = in ? ld_coh(r + b) : 0u;
				vc[j] = in ? ld_coh(r + nb + b) : 0u;
			}
#pragma unroll
			for (int j = 0; j < 8; ++j) { s += vs[j]; c += vc[j]; }
		}
		a.map[(size_t)t * nb + b] = c == 0 ? (double)b : (double)s / (double)c;
	}
}

/* utils::mapPixVals<Nearest / Linear> (imgUtils.h:696-703): It = map(It_orig) */
__global__ __launch_bounds__(kBlock) void k_rscv_apply(int N, int nb, int linear, const double *map, const double *ito, double *It) {
	__shared__ double s_map[kRscvMaxBins];
	const int t = blockIdx.y;
	for (int b = threadIdx.x; b < nb; b += kBlock) s_map[b] = map[(size_t)t * nb + b];
	__syncthreads();
	const double *x = ito + (size_t)t * N;
	double *out = It + (size_t)t * N;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) out[i] = rscv_map_val(s_map, nb, linear, x[i]);
}

void launch_rscv_codes(int N, int B, int nb, const double *i0, unsigned char *code, hipStream_t st) {
	MTFHIP_LAUNCH(k_rscv_codes, grid2(simple_blocks_per_target(N), B), dim3(kBlock), 0, st, N, nb, i0, code);
}
template <int SSM>
static void launch_rscv_hist_ssm(const BatchView &bv, const ImgView &im, const RscvArgs &a, hipStream_t st) {
	const int nblk = imap_hist_blocks(bv.N, kImapChunks);
	const dim3 g = grid2(nblk, bv.B);
	switch (a.kind) {
	case RSCV_IT_REPLAY: MTFHIP_LAUNCH((k_rscv_hist<SSM, RSCV_IT_REPLAY>), g, dim3(kBlock), 0, st, bv, im, a, nblk); break;
	case RSCV_IT_FAST_ICLK: MTFHIP_LAUNCH((k_rscv_hist<SSM, RSCV_IT_FAST_ICLK>), g, dim3(kBlock), 0, st, bv, im, a, nblk); break;
	case RSCV_IT_FAST_CHAINED: MTFHIP_LAUNCH((k_rscv_hist<SSM, RSCV_IT_FAST_CHAINED>), g, dim3(kBlock), 0, st, bv, im, a, nblk); break;
	case RSCV_IT_FAST_QSTEP: MTFHIP_LAUNCH((k_rscv_hist<SSM, RSCV_IT_FAST_QSTEP>), g, dim3(kBlock), 0, st, bv, im, a, nblk); break;
	default: MTFHIP_LAUNCH((k_rscv_hist<SSM, RSCV_IT_FROM_BUF>), g, dim3(kBlock), 0, st, bv, im, a, nblk); break;
	}
}
void launch_rscv_hist(const BatchView &bv, const ImgView &im, const RscvArgs &a, hipStream_t st) {
	if (bv.ssm == MTFHIP_SSM_HOMOGRAPHY) launch_rscv_hist_ssm<MTFHIP_SSM_HOMOGRAPHY>(bv, im, a, st);
	else launch_rscv_hist_ssm<MTFHIP_SSM_AFFINE>(bv, im, a, st);
}
void launch_rscv_apply(int N, int B, int nb, int linear, const double *map, const double *it_orig, double *It, hipStream_t st) {
	MTFHIP_LAUNCH(k_rscv_apply, grid2(simple_blocks_per_target(N), B), dim3(kBlock), 0, st, N, nb, linear, map, it_orig, It);
}

} // namespace mtfhip
