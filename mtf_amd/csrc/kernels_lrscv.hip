/*
 * kernels_lrscv.hip -- the Localized Reversed SCV appearance model (AM/src/LRSCV.cc): the sub-region maps LRSCV::updatePixVals builds
 * from the current patch (LRSCV.cc:224-292).  LRSCV is SSD on It = sum_r w(i, r) map_r(It_orig); the blend is applied inside the fused
 * pass (kernels_fused_lrscv.hip) or, on the per-function path, by k_lrscv_apply.
 *
 *   k_lrscv_hist  pass 1  It_orig (sampled at the current warp with the arithmetic of the fused pass that follows -- rscv_it_orig, as
 *                         k_rscv_hist -- or read from the It_orig buffer on the per-function path) and, per sub-region r and CURRENT bin
 *                         b, the two Dirac sums the map needs:
 *                           map_r[b] = sum_j j joint_r(b, j) / curr_hist_r(b)  needs only  sum over the pixels of r in current bin b of
 *                           (int)I0, and their count.
 *                         Keyed by (cell, current bin) on LSCV's cell plane (every pixel of a cell lies in the same sub-regions): one
 *                         u32 pair per pixel into a workgroup's LDS table, then lscv_hand_over (mtfhip_lscv_device.h) -- the target's
 *                         sums, the last-arriving workgroup's maps with the reference's division and its empty-bin rule (map[b] = b
 *                         where curr_hist(b) == 0), the FP64 affine fit with affine_mapping, the sums zeroed for the next launch.
 *                         Reads 16 B/px (grid point) + 4 texels + 1 B/px (RSCV's code plane) + 2 B/px (the cell plane, one per batch).
 *   k_lrscv_apply         It = lrscv_blend(It_orig) (per-function path)
 *
 * Reproducibility.  Every sum is an integer, exact in any order (u32: imap_capture refuses patches where (n_bins - 1) N could overflow
 * one), and stays exact as a double; the maps are identical run to run.  Bin agreement: as kernels_rscv.hip's.
 */
#include "mtfhip_rscv_device.h"
#include "mtfhip_lscv_device.h"

namespace mtfhip {

template <int SSM, int KIND>
__global__ __launch_bounds__(kBlock) void k_lrscv_hist(BatchView bv, ImgView im, LrscvArgs a, int nblk) {
	extern __shared__ unsigned s_tab[];   /* [2][ncell nb]: the sums of (int)I0, then the counts, keyed by (cell, current bin) */
	__shared__ int s_last;
	const int t = blockIdx.y;
	if (a.active && !a.active[t]) return;   /* (uniform over the target's workgroups: nobody counts itself in) */
	const int N = bv.N, nb = a.nb, E = a.ncell * nb;
	unsigned *s_sum = s_tab, *s_cnt = s_tab + E;
	const double2 *ip = reinterpret_cast<const double2 *>(bv.buf[bv.unit_z ? MTFHIP_BUF_INIT_PTS : MTFHIP_BUF_INIT_HXY]) + (size_t)t * N;
	const double *iz = bv.buf[MTFHIP_BUF_INIT_Z] + (size_t)t * N;
	const double *ito = a.it_orig ? a.it_orig + (size_t)t * N : nullptr;
	const unsigned char *code = a.code + (size_t)t * N;
	Warp9 W;
	if constexpr (KIND != RSCV_IT_FROM_BUF) W = load_warp(bv.warps + 9 * t);
	for (int e = threadIdx.x; e < 2 * E; e += kBlock) s_tab[e] = 0u;
	__syncthreads();
	/* 256-pixel chunks at multiples of 256: a wave holds the 64 pixels a wave of the fused pass holds (rscv_it_orig's interior test is
	 * per wave, so every lane whose pixel is < N samples, whether or not its pixel lies in a sub-region) */
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
			const unsigned cl = a.cell[i];
			if (cl != 0xffffu) {   /* (in no sub-region: no histogram counts it) */
				/* getDiracJointHist over a sub-region (histUtils.cc:396-419) with the current patch first: joint((int)It, (int)I0) += 1,
				 * curr_hist((int)It) += 1 (LRSCV.cc:240-243) */
				int bt = (int)itv;
				bt = bt < 0 ? 0 : (bt > nb - 1 ? nb - 1 : bt);
				const int e = (int)cl * nb + bt;
				atomicAdd(&s_sum[e], (unsigned)code[i]);
				atomicAdd(&s_cnt[e], 1u);
			}
		}
	}
	__syncthreads();
	lscv_hand_over(a, t, nblk, s_tab, s_last);
}

/* LRSCV.cc:249-254: It = the blend of It_orig's images through the sub-region maps */
__global__ __launch_bounds__(kBlock) void k_lrscv_apply(int N, LrscvMap lm, const double *ito, double *It) {
	extern __shared__ double s_map[];   /* affine: [R][2] (a_r, c_r); else [R][nb] */
	const int t = blockIdx.y;
	const int M = lm.affine ? 2 * lm.R : lm.R * lm.nb;
	for (int e = threadIdx.x; e < M; e += kBlock) s_map[e] = lm.map[(size_t)t * M + e];
	__syncthreads();
	const double *x = ito + (size_t)t * N;
	double *out = It + (size_t)t * N;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) out[i] = lrscv_blend(s_map, lm, lm.wts + i, (unsigned)N, x[i]);
}

template <int SSM>
static void launch_lrscv_hist_ssm(const BatchView &bv, const ImgView &im, const LrscvArgs &a, hipStream_t st) {
	const int nblk = imap_hist_blocks(bv.N, kImapChunksLocal);
	const dim3 g = grid2(nblk, bv.B);
	const size_t lds = sizeof(unsigned) * 2 * (size_t)a.ncell * a.nb;
	switch (a.kind) {
	case RSCV_IT_REPLAY: MTFHIP_LAUNCH((k_lrscv_hist<SSM, RSCV_IT_REPLAY>), g, dim3(kBlock), lds, st, bv, im, a, nblk); break;
	case RSCV_IT_FAST_ICLK: MTFHIP_LAUNCH((k_lrscv_hist<SSM, RSCV_IT_FAST_ICLK>), g, dim3(kBlock), lds, st, bv, im, a, nblk); break;
	case RSCV_IT_FAST_CHAINED: MTFHIP_LAUNCH((k_lrscv_hist<SSM, RSCV_IT_FAST_CHAINED>), g, dim3(kBlock), lds, st, bv, im, a, nblk); break;
	case RSCV_IT_FAST_QSTEP: MTFHIP_LAUNCH((k_lrscv_hist<SSM, RSCV_IT_FAST_QSTEP>), g, dim3(kBlock), lds, st, bv, im, a, nblk); break;
	default: MTFHIP_LAUNCH((k_lrscv_hist<SSM, RSCV_IT_FROM_BUF>), g, dim3(kBlock), lds, st, bv, im, a, nblk); break;
	}
}
void launch_lrscv_hist(const BatchView &bv, const ImgView &im, const LrscvArgs &a, hipStream_t st) {
	if (bv.ssm == MTFHIP_SSM_HOMOGRAPHY) launch_lrscv_hist_ssm<MTFHIP_SSM_HOMOGRAPHY>(bv, im, a, st);
	else launch_lrscv_hist_ssm<MTFHIP_SSM_AFFINE>(bv, im, a, st);
}
void launch_lrscv_apply(int N, int B, const LrscvMap &lm, const double *it_orig, double *It, hipStream_t st) {
	const size_t lds = sizeof(double) * (size_t)(lm.affine ? 2 * lm.R : lm.R * lm.nb);
	MTFHIP_LAUNCH(k_lrscv_apply, grid2(simple_blocks_per_target(N), B), dim3(kBlock), lds, st, N, lm, it_orig, It);
}

} // namespace mtfhip
