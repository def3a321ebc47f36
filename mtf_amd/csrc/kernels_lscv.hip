/*
 * kernels_lscv.hip -- the Localized SCV appearance model (AM/src/LSCV.cc): the template re-map that LSCV::updateSimilarity runs in front
 * of SSDBase::updateSimilarity (LSCV.cc:263-304).  LSCV is SSD on the re-mapped template, so everything behind these kernels is the SSD
 * path (the fused SSD kernels of kernels_fused.hip, unchanged, read the re-mapped I0 from MTFHIP_BUF_I0).
 *
 *   k_lscv_hist   pass 1  It (sampled at the current warp with k_scv_hist's arithmetic, or read from MTFHIP_BUF_IT on the per-function
 *                         path) and, per sub-region r and template bin b, the two Dirac sums the map needs:
 *                           map_r[b] = sum_i i joint_r(i, b) / init_hist_r(b)  needs only  sum over the pixels of r in template bin b of
 *                           (int)It, and their count.
 *                         The sub-region boundaries cut the patch into at most (2 n_x - 1)(2 n_y - 1) cells, and every pixel of a cell
 *                         lies in the same sub-regions: a workgroup adds one u32 pair per pixel into its (cell, bin) table in LDS and
 *                         adds the table's non-zero entries into the target's u32 sums with agent-scope atomics.  The last workgroup
 *                         of a target to arrive (kernels_rscv.hip's hand-over) adds the cells of each sub-region, writes the maps with
 *                         the reference's division and its empty-bin rule (map[b] = b where init_hist(b) == 0), zeroes the sums for the
 *                         next launch and, with affine_mapping, fits map_r[k] ~ a_r k + c_r over k = 0 .. n_bins - 1 in FP64.
 *                         Reads 16 B/px (grid point) + 4 texels + 2 B/px (code plane) + 2 B/px (cell plane, one per batch).
 *   k_lscv_remap          I0 = sum over idx (outer), idy (inner) of w(i, r) mapped_r(I0_orig), each product rounded, no FMA: the
 *                         reference's order and rounding.  Nearest reads the code plane (2 B/px), linear and affine I0_orig (8 B/px);
 *                         the weights are one [n_sub][N] table per batch (8 n_sub B/px, shared by the batch's targets); 8 B/px out.
 *
 * Reproducibility.  Every histogram sum is an integer, exact in any order (u32: imap_capture refuses patches where (n_bins - 1) N could
 * overflow one), and stays exact as a double, so the maps are identical run to run and equal to the float64 reference's.  The affine
 * fit sums in a fixed order (lane l takes k = l, l + 64, ..., in order; then a xor butterfly, whose every step adds the same two values
 * on both lanes).  Indices are clamped to [0, n_bins - 1], as in kernels_scv.hip.
 */
#include "mtfhip_lscv_device.h"

namespace mtfhip {

template <int SSM>
__global__ __launch_bounds__(kBlock) void k_lscv_hist(BatchView bv, ImgView im, LscvArgs a, int nblk) {
	extern __shared__ unsigned s_tab[];   /* [2][ncell nb]: the sums of (int)It, then the counts */
	__shared__ int s_last;
	const int t = blockIdx.y;
	if (a.active && !a.active[t]) return;   /* (uniform over the target's workgroups: nobody counts itself in) */
	const int N = bv.N, nb = a.nb, E = a.ncell * nb;
	unsigned *s_sum = s_tab, *s_cnt = s_tab + E;
	const double *It = bv.buf[MTFHIP_BUF_IT] + (size_t)t * N;
	const double2 *ip = reinterpret_cast<const double2 *>(bv.buf[bv.unit_z ? MTFHIP_BUF_INIT_PTS : MTFHIP_BUF_INIT_HXY]) + (size_t)t * N;
	const double *iz = bv.buf[MTFHIP_BUF_INIT_Z] + (size_t)t * N;
	const unsigned short *code = a.code + (size_t)t * N;
	Warp9 W;
	if (!a.from_it) W = load_warp(bv.warps + 9 * t);
	for (int e = threadIdx.x; e < 2 * E; e += kBlock) s_tab[e] = 0u;
	__syncthreads();
	const int n_chunks = (N + kBlock - 1) / kBlock;
	for (int ch = blockIdx.x; ch < n_chunks; ch += nblk) {
		const int i = ch * kBlock + threadIdx.x;
		if (i >= N) continue;
		const unsigned cl = a.cell[i];
		if (cl == 0xffffu) continue;   /* (in no sub-region: no histogram counts it) */
		double itv;
		if (a.from_it) {
			itv = It[i];
		} else {
			/* curr_pts = curr_warp * init_pts_hm, dehomogenised (Homography.cc:86-90, Affine.cc:104), then getPixVal -- k_scv_hist's */
			double hx, hy, z;
			if (bv.unit_z) { const double2 p = ip[i]; hx = p.x; hy = p.y; z = 1.0; }
			else { const double2 p = ip[i]; hx = p.x; hy = p.y; z = iz[i]; }
			double wx, wy;
			if constexpr (SSM == MTFHIP_SSM_HOMOGRAPHY) {
				const double cx = W.m[0] * hx + W.m[1] * hy + W.m[2] * z;
				const double cy = W.m[3] * hx + W.m[4] * hy + W.m[5] * z;
				const double D = W.m[6] * hx + W.m[7] * hy + W.m[8] * z;
				wx = cx / D; wy = cy / D;
			} else {
				wx = W.m[0] * hx + W.m[1] * hy + W.m[2] * z;
				wy = W.m[3] * hx + W.m[4] * hy + W.m[5] * z;
			}
			itv = a.norm_mult * pix_val(im, wx, wy) + a.norm_add;
		}
		/* getDiracJointHist over a sub-region (histUtils.cc:396-419): joint((int)It, (int)I0_orig) += 1, init_hist((int)I0_orig) += 1 */
		int bt = (int)itv;
		bt = bt < 0 ? 0 : (bt > nb - 1 ? nb - 1 : bt);
		const int e = (int)cl * nb + (code[i] & 0xff);
		atomicAdd(&s_sum[e], (unsigned)bt);
		atomicAdd(&s_cnt[e], 1u);
	}
	__syncthreads();
	lscv_hand_over(a, t, nblk, s_tab, s_last);
}

/* LSCV.cc:286-300: I0_mapped through sub-region r's map (affine, utils::mapPixVals<Linear / Nearest>, imgUtils.h:682-703), then
 * I0 += I0_mapped * sub_region_wts(pix, r) for idx outer, idy inner */
__global__ __launch_bounds__(kBlock) void k_lscv_remap(int N, LscvArgs a, double *I0) {
	extern __shared__ double s_map[];   /* affine: [R][2] (a_r, c_r); else [R][nb] */
	const int t = blockIdx.y;
	if (a.active && !a.active[t]) return;
	const int nb = a.nb, nx = a.nx, ny = a.ny, R = nx * ny;
	const int M = a.affine ? 2 * R : R * nb;
	const double *src = a.affine ? a.aff + (size_t)t * 2 * R : a.map + (size_t)t * R * nb;
	for (int e = threadIdx.x; e < M; e += kBlock) s_map[e] = src[e];
	__syncthreads();
	const unsigned short *c = a.code + (size_t)t * N;
	const double *x = a.i0o + (size_t)t * N;
	double *out = I0 + (size_t)t * N;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
		double v = 0.0, dx = 0.0;
		int lx = 0, ux = 0, nr = 0;
		if (a.affine || a.linear) {
			v = x[i];
			lx = (int)v;
			dx = v - lx;
			lx = lx < 0 ? 0 : (lx > nb - 1 ? nb - 1 : lx);
			ux = lx + 1 < nb ? lx + 1 : nb - 1;
		} else {
			nr = c[i] >> 8;
		}
		double acc = 0.0;
		for (int idx = 0; idx < nx; ++idx)
			for (int idy = 0; idy < ny; ++idy) {
				const int r = idy * nx + idx;
				double m;
				if (a.affine) {
					m = s_map[2 * r] * v + s_map[2 * r + 1];
				} else if (a.linear) {
					const double *mr = s_map + r * nb;
					m = dx == 0 ? mr[lx] : (1 - dx) * mr[lx] + dx * mr[ux];
				} else {
					m = s_map[r * nb + nr];
				}
				acc += m * a.wts[(size_t)r * N + i];
			}
		out[i] = acc;
	}
}

void launch_lscv_update(const BatchView &bv, const ImgView &im, const LscvArgs &a, double *I0, hipStream_t st) {
	const int nblk = imap_hist_blocks(bv.N, kImapChunksLocal);
	const size_t lds_hist = sizeof(unsigned) * 2 * (size_t)a.ncell * a.nb;
	if (bv.ssm == MTFHIP_SSM_HOMOGRAPHY) MTFHIP_LAUNCH(k_lscv_hist<MTFHIP_SSM_HOMOGRAPHY>, grid2(nblk, bv.B), dim3(kBlock), lds_hist, st, bv, im, a, nblk);
	else MTFHIP_LAUNCH(k_lscv_hist<MTFHIP_SSM_AFFINE>, grid2(nblk, bv.B), dim3(kBlock), lds_hist, st, bv, im, a, nblk);
	const size_t lds_map = sizeof(double) * (a.affine ? 2 * (size_t)a.nx * a.ny : (size_t)a.nx * a.ny * a.nb);
	MTFHIP_LAUNCH(k_lscv_remap, grid2(simple_blocks_per_target(bv.N), bv.B), dim3(kBlock), lds_map, st, bv.N, a, I0);
}

} // namespace mtfhip
