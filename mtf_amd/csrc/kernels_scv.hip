/*
 * kernels_scv.hip -- the Sum of Conditional Variance appearance model (AM/src/SCV.cc): the template re-map that SCV::updateSimilarity
 * runs in front of SSDBase::updateSimilarity.  SCV is SSD on the re-mapped template, so everything behind these kernels is the SSD path
 * (the fused SSD kernels of kernels_fused.hip, unchanged, read the re-mapped I0 from MTFHIP_BUF_I0).
 *
 *   k_scv_codes  (init)  per pixel of I0_orig: (int)I0_orig (the Dirac / Bilinear template bin) | (int)rint(I0_orig) << 8 (the nearest
 *                        mapping's index) -- the template's bins are fixed, so they are worked out once
 *   k_scv_hist   pass 1  It (sampled at the current warp, or read from MTFHIP_BUF_IT on the per-function path) and the two per-bin sums
 *                        the map needs:  map[b] = sum_i i joint(i, b) / init_hist(b)  needs only
 *                          Dirac:    sum over the pixels of template bin b of (int)It, and their count;
 *                          Bilinear: t_wt It and t_wt into column b_0, b_wt It and b_wt into column b_0 + 1 (l p + r (p + 1) = It),
 *                        so the n_bins^2 joint histogram never exists.  Reads 16 B/px (grid point) + 4 texels + 2 B/px (Dirac, the
 *                        code plane) or 8 B/px (Bilinear, I0_orig); writes one row of 2 n_bins sums per workgroup.
 *   k_scv_map            the workgroup rows summed in workgroup order, then the reference's division and its empty-bin rule
 *                        (map[b] = b where init_hist(b) == 0)
 *   k_scv_remap          I0 = map(I0_orig): nearest (map[(int)rint(x)]) from the code plane (2 B/px), linear from I0_orig (8 B/px); 8 B/px out
 *
 * Reproducibility.  Dirac sums are integers: pass 1 adds them with LDS integer atomics (exact in any order) and they stay exact as
 * doubles.  Bilinear sums have a fixed order: the 256 pixels of a chunk are staged in LDS, wave w owns the pixels [64 w, 64 w + 64) of
 * the chunk and lane l the bins l, l + 64, l + 128, l + 192, and adds its pixels in pixel order; the four waves' tables are summed in wave
 * order at the end.  The workgroup rows are summed by k_scv_map in workgroup order.  Both are identical run to run.
 * Indices are clamped to [0, n_bins - 1]: pixel values outside [0, 255] (the reference would index out of its histograms) stay in bounds.
 */
#include "mtfhip_device.h"

namespace mtfhip {

__global__ __launch_bounds__(kBlock) void k_scv_codes(int N, int nb, const double *i0o, unsigned short *code) {
	const int t = blockIdx.y;
	const double *x = i0o + (size_t)t * N;
	unsigned short *c = code + (size_t)t * N;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
		const double v = x[i];
		int lo = (int)v, nr = (int)rint(v);
		lo = lo < 0 ? 0 : (lo > nb - 1 ? nb - 1 : lo);
		nr = nr < 0 ? 0 : (nr > nb - 1 ? nb - 1 : nr);
		c[i] = (unsigned short)(lo | (nr << 8));
	}
}

template <int SSM>
__global__ __launch_bounds__(kBlock) void k_scv_hist(BatchView bv, ImgView im, ScvArgs a, double *part, int nblk) {
	__shared__ int s_bin[kBlock];
	__shared__ double s_v0[kBlock], s_w0[kBlock], s_v1[kBlock], s_w1[kBlock];
	__shared__ double s_tab[4][2][kScvMaxBins];
	__shared__ unsigned s_isum[kScvMaxBins], s_icnt[kScvMaxBins];   /* Dirac: integer sums, exact in any order */
	const int t = blockIdx.y;
	if (a.active && !a.active[t]) return;
	const int N = bv.N, nb = a.nb, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const bool bil = a.hist == 1;
	const double *It = bv.buf[MTFHIP_BUF_IT] + (size_t)t * N;
	const double2 *ip = reinterpret_cast<const double2 *>(bv.buf[bv.unit_z ? MTFHIP_BUF_INIT_PTS : MTFHIP_BUF_INIT_HXY]) + (size_t)t * N;
	const double *iz = bv.buf[MTFHIP_BUF_INIT_Z] + (size_t)t * N;
	const unsigned short *code = a.code + (size_t)t * N;
	const double *i0o = a.i0o + (size_t)t * N;
	Warp9 W;
	if (!a.from_it) W = load_warp(bv.warps + 9 * t);
	double s[4] = {0.0, 0.0, 0.0, 0.0}, w[4] = {0.0, 0.0, 0.0, 0.0};
	const int nk = (nb + 63) >> 6;   /* bin slots per lane in use */
	if (!bil) {
		for (int b = threadIdx.x; b < kScvMaxBins; b += kBlock) { s_isum[b] = 0u; s_icnt[b] = 0u; }
		__syncthreads();
	}
	const int n_chunks = (N + kBlock - 1) / kBlock;
	for (int ch = blockIdx.x; ch < n_chunks; ch += nblk) {
		const int i = ch * kBlock + threadIdx.x;
		int bin = -2;   /* (no bin: a padding pixel of the last chunk) */
		double v0 = 0.0, w0 = 0.0, v1 = 0.0, w1 = 0.0;
		if (i < N) {
			double itv;
			if (a.from_it) {
				itv = It[i];
			} else {
				/* curr_pts = curr_warp * init_pts_hm, dehomogenised (Homography.cc:86-90, Affine.cc:104), then getPixVal */
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
			if (bil) {
				/* getBilinearJointHist (histUtils.cc:421-461) with I0_orig as the second image */
				const double x0 = i0o[i];
				int b0 = (int)x0;
				const double b_wt = x0 - b0, t_wt = 1 - b_wt;
				b0 = b0 < 0 ? 0 : (b0 > nb - 1 ? nb - 1 : b0);
				bin = b0;
				v0 = t_wt * itv; w0 = t_wt;
				if (b_wt != 0 && b0 + 1 < nb) { v1 = b_wt * itv; w1 = b_wt; }
			} else {
				/* getDiracJointHist (histUtils.cc:370-394): joint((int)It, (int)I0_orig) += 1 */
				int bt = (int)itv;
				bt = bt < 0 ? 0 : (bt > nb - 1 ? nb - 1 : bt);
				bin = code[i] & 0xff;
				v0 = (double)bt; w0 = 1.0;
			}
		}
		if (!bil) {
			/* (a workgroup sums at most 255 x 2^26 / 64 < 2^32: no u32 overflow) */
			if (bin >= 0) { atomicAdd(&s_isum[bin], (unsigned)v0); atomicAdd(&s_icnt[bin], 1u); }
			continue;
		}
		s_bin[threadIdx.x] = bin; s_v0[threadIdx.x] = v0; s_w0[threadIdx.x] = w0; s_v1[threadIdx.x] = v1; s_w1[threadIdx.x] = w1;
		__syncthreads();
		const int j0 = wave * 64;
		for (int j = j0; j < j0 + 64; ++j) {
			const int bj = s_bin[j];   /* (one LDS broadcast per pixel) */
			const double a0 = s_v0[j], c0 = s_w0[j];
			const double a1 = s_v1[j], c1 = s_w1[j];
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				if (k >= nk) break;   /* (uniform) */
				if (bj == lane + 64 * k) { s[k] += a0; w[k] += c0; }
				if (bj + 1 == lane + 64 * k) { s[k] += a1; w[k] += c1; }
			}
		}
		__syncthreads();
	}
	double *row = part + ((size_t)t * nblk + blockIdx.x) * 2 * nb;
	if (!bil) {
		__syncthreads();
		for (int b = threadIdx.x; b < nb; b += kBlock) { row[b] = (double)s_isum[b]; row[nb + b] = (double)s_icnt[b]; }
		return;
	}
#pragma unroll
	for (int k = 0; k < 4; ++k) { s_tab[wave][0][lane + 64 * k] = s[k]; s_tab[wave][1][lane + 64 * k] = w[k]; }
	__syncthreads();
	for (int b = threadIdx.x; b < nb; b += kBlock) {
		double ss = s_tab[0][0][b], ww = s_tab[0][1][b];
		for (int q = 1; q < 4; ++q) { ss += s_tab[q][0][b]; ww += s_tab[q][1][b]; }
		row[b] = ss; row[nb + b] = ww;
	}
}

/* SCV::updateSimilarity SCV.cc:208-229: intensity_map(b) = wt_sum / init_hist(b), or b where init_hist(b) == 0 */
__global__ __launch_bounds__(kBlock) void k_scv_map(int nb, const int *active, const double *part, int nblk, double *map) {
	const int t = blockIdx.x;
	if (active && !active[t]) return;
	for (int b = threadIdx.x; b < nb; b += kBlock) {
		const double *col = part + (size_t)t * nblk * 2 * nb + b;
		double ss = 0.0, ww = 0.0;
		for (int k = 0; k < nblk; ++k) { ss += col[(size_t)k * 2 * nb]; ww += col[(size_t)k * 2 * nb + nb]; }
		map[(size_t)t * nb + b] = ww == 0 ? (double)b : ss / ww;
	}
}

/* utils::mapPixVals<Nearest / Linear> (imgUtils.h:682-703): I0 = map(I0_orig) */
__global__ __launch_bounds__(kBlock) void k_scv_remap(int N, int nb, int linear, const int *active, const double *map, const unsigned short *code,
	const double *i0o, double *I0) {
	__shared__ double s_map[kScvMaxBins];
	const int t = blockIdx.y;
	if (active && !active[t]) return;
	for (int b = threadIdx.x; b < nb; b += kBlock) s_map[b] = map[(size_t)t * nb + b];
	__syncthreads();
	const unsigned short *c = code + (size_t)t * N;
	const double *x = i0o + (size_t)t * N;
	double *out = I0 + (size_t)t * N;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
		if (linear) {
			const double v = x[i];
			int lx = (int)v;
			const double dx = v - lx;
			lx = lx < 0 ? 0 : (lx > nb - 1 ? nb - 1 : lx);
			const int ux = lx + 1 < nb ? lx + 1 : nb - 1;
			out[i] = dx == 0 ? s_map[lx] : (1 - dx) * s_map[lx] + dx * s_map[ux];
		} else {
			out[i] = s_map[c[i] >> 8];
		}
	}
}

void launch_scv_codes(int N, int B, int nb, const double *i0o, unsigned short *code, hipStream_t st) {
	MTFHIP_LAUNCH(k_scv_codes, grid2(simple_blocks_per_target(N), B), dim3(kBlock), 0, st, N, nb, i0o, code);
}
void launch_scv_update(const BatchView &bv, const ImgView &im, const ScvArgs &a, double *part, double *map, double *I0, hipStream_t st) {
	const int nblk = imap_hist_blocks(bv.N, kImapChunks);
	if (bv.ssm == MTFHIP_SSM_HOMOGRAPHY) MTFHIP_LAUNCH(k_scv_hist<MTFHIP_SSM_HOMOGRAPHY>, grid2(nblk, bv.B), dim3(kBlock), 0, st, bv, im, a, part, nblk);
	else MTFHIP_LAUNCH(k_scv_hist<MTFHIP_SSM_AFFINE>, grid2(nblk, bv.B), dim3(kBlock), 0, st, bv, im, a, part, nblk);
	MTFHIP_LAUNCH(k_scv_map, dim3(bv.B), dim3(kBlock), 0, st, a.nb, a.active, (const double *)part, nblk, map);
	MTFHIP_LAUNCH(k_scv_remap, grid2(simple_blocks_per_target(bv.N), bv.B), dim3(kBlock), 0, st, bv.N, a.nb, a.linear, a.active, (const double *)map, a.code,
		a.i0o, I0);
}

} // namespace mtfhip
