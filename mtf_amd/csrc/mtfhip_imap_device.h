/*
 * mtfhip_imap_device.h -- what the pass-1 kernels of the SCV family (kernels_imap.hip) share: the bin clamp, the It expression of every
 * RSCV_IT_* kind, the walk over a target's pixels, and the hand-over that ends a localized pass 1.
 *
 * Bin agreement.  A pixel must fall in the bin of the histogram the pass behind pass 1 looks it up in, so pass 1 evaluates It exactly as
 * that pass does.  SCV and LSCV run in front of an SSD pass on the re-mapped template and bin It with the replay expression
 * (RSCV_IT_REPLAY).  RSCV and LRSCV run in front of the fused pass that maps every sample (mtfhip_fused_device.h: issue_tex +
 * row_compute): the replay expression for MATH_REPLAY and every materialising launch; for the lean tolerance-mode launches the FMA warp,
 * the same interior-cell test of the same 64-pixel wave (the fused pass walks a target's pixels in rows of 256 starting at multiples of
 * 256, so wave w of a row holds pixels [64 k, 64 k + 64)), the closed-form interpolant when the whole wave is interior and the
 * reference's sampler otherwise.  On the per-function path It is read from a buffer (RSCV_IT_FROM_BUF).
 */
#ifndef MTFHIP_IMAP_DEVICE_H
#define MTFHIP_IMAP_DEVICE_H
#include "mtfhip_fused_device.h"

namespace mtfhip {

/* indices are clamped to [0, n_bins - 1]: pixel values outside [0, 255] (the reference would index out of its histograms) stay in bounds */
__device__ __forceinline__ int imap_bin(int b, int nb) { return b < 0 ? 0 : (b > nb - 1 ? nb - 1 : b); }

/* It of one pixel at the current warp, as the pass behind pass 1 computes it (above); the fast kinds are called by every lane of a wave
 * whose pixel is < N */
template <int SSM, int KIND>
__device__ __forceinline__ double rscv_it_orig(const ImgView &im, const Warp9 &W, const ImapArgs &a, double hx, double hy, double z) {
	if constexpr (KIND == RSCV_IT_REPLAY) {
		/* curr_pts = curr_warp * init_pts_hm, dehomogenised (Homography.cc:86-90, Affine.cc:104), then getPixVal */
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
		return a.norm_mult * pix_val(im, wx, wy) + a.norm_add;
	} else {
		/* issue_tex, FAST (z = 1 on a unit-z grid: W.m[2] * 1.0 is W.m[2]) */
		double wx, wy, cx, cy, D, inv = 1.0;
		if constexpr (SSM == MTFHIP_SSM_HOMOGRAPHY) {
			cx = fma(W.m[0], hx, fma(W.m[1], hy, W.m[2] * z));
			cy = fma(W.m[3], hx, fma(W.m[4], hy, W.m[5] * z));
			D = fma(W.m[6], hx, fma(W.m[7], hy, W.m[8] * z));
			inv = rcp_fast(D);
			wx = cx * inv; wy = cy * inv;
		} else {
			wx = fma(W.m[0], hx, fma(W.m[1], hy, W.m[2] * z));
			wy = fma(W.m[3], hx, fma(W.m[4], hy, W.m[5] * z));
			cx = wx; cy = wy; D = 1.0;
		}
		const int lx = (int)wx, ly = (int)wy;
		const double lxd = (double)lx, lyd = (double)ly;
		bool fast = (wx >= 0) & (wy >= 0) & (wx != lxd) & (wy != lyd) & (lx < im.w - 1) & (ly < im.h - 1);
		const double eps = a.grad_eps;
		if constexpr (KIND == RSCV_IT_FAST_CHAINED) {
			/* row_compute, MODE != 2 && CHAINED: the axis-aligned neighbours */
			const double px0 = wx + eps, px1 = wx - eps, py2 = wy + eps, py3 = wy - eps;
			fast = fast & (px0 < lxd + 1) & (px1 > lxd) & (py2 < lyd + 1) & (py3 > lyd);
		} else if constexpr (KIND == RSCV_IT_FAST_QSTEP) {
			/* row_compute, QSTEP: the rounded steps of updateGradPts */
			const double ex0 = W.m[0] * eps, ex1 = W.m[3] * eps, ex2 = W.m[6] * eps;
			const double ey0 = W.m[1] * eps, ey1 = W.m[4] * eps, ey2 = W.m[7] * eps;
			double dpx_x, dpy_x, dpx_y, dpy_y;
			if constexpr (SSM == MTFHIP_SSM_HOMOGRAPHY) {
				const double dd_x = fd_step_sym(D, ex2), dd_y = fd_step_sym(D, ey2);
				dpx_x = fma(-wx, dd_x, fd_step_sym(cx, ex0)) * inv; dpy_x = fma(-wy, dd_x, fd_step_sym(cy, ex1)) * inv;
				dpx_y = fma(-wx, dd_y, fd_step_sym(cx, ey0)) * inv; dpy_y = fma(-wy, dd_y, fd_step_sym(cy, ey1)) * inv;
			} else {
				(void)ex2; (void)ey2;
				dpx_x = fd_step_sym(wx, ex0); dpy_x = fd_step_sym(wy, ex1); dpx_y = fd_step_sym(wx, ey0); dpy_y = fd_step_sym(wy, ey1);
			}
			const double mx = fmax(fabs(dpx_x), fabs(dpx_y)), my = fmax(fabs(dpy_x), fabs(dpy_y));
			fast = fast & (wx - mx > lxd) & (wx + mx < lxd + 1) & (wy - my > lyd) & (wy + my < lyd + 1);
		}
		if (__builtin_amdgcn_ballot_w64(!fast) == 0) {
			/* every lane of the wave is interior: its cell's four texels exist */
			const float *r0 = im.data + (size_t)ly * im.stride + lx;
			const float *r1 = r0 + im.stride;
			double v, bgx, bgy;
			bilin_fast(r0[0], r0[1], r1[0], r1[1], wx - lxd, wy - lyd, v, bgx, bgy);
			return fma(a.norm_mult, v, a.norm_add);
		}
		return a.norm_mult * pix_val(im, wx, wy) + a.norm_add;
	}
}

/* The pass-1 walk of target t's pixels by workgroup blockIdx.x of nblk: 256-pixel chunks at multiples of 256, so that a wave holds the 64
 * pixels a wave of the fused pass holds.  step(i, it) runs on every thread of every chunk, the padding lanes i >= bv.N of the last chunk
 * included (SCV's Bilinear staging has barriers in it); it() is pixel i's It of kind KIND, for i < bv.N.  When to call it is the model's:
 * a fast kind ballots over the wave, so its model samples every lane with i < bv.N; replay and the buffer read have no wave-wide step. */
template <int SSM, int KIND, class F>
__device__ __forceinline__ void imap_walk(const BatchView &bv, const ImgView &im, const ImapArgs &a, int t, int nblk, F &&step) {
	const int N = bv.N;
	const double2 *ip = reinterpret_cast<const double2 *>(bv.buf[bv.unit_z ? MTFHIP_BUF_INIT_PTS : MTFHIP_BUF_INIT_HXY]) + (size_t)t * N;
	const double *iz = bv.buf[MTFHIP_BUF_INIT_Z] + (size_t)t * N;
	const double *src = nullptr;
	Warp9 W;
	if constexpr (KIND == RSCV_IT_FROM_BUF) src = a.src + (size_t)t * N;
	else W = load_warp(bv.warps + 9 * t);
	const int n_chunks = (N + kBlock - 1) / kBlock;
	for (int ch = blockIdx.x; ch < n_chunks; ch += nblk) {
		const int i = ch * kBlock + threadIdx.x;
		step(i, [&]() -> double {
			if constexpr (KIND == RSCV_IT_FROM_BUF) {
				return src[i];
			} else {
				const double2 p = ip[i];
				const double z = bv.unit_z ? 1.0 : iz[i];
				return rscv_it_orig<SSM, KIND>(im, W, a, p.x, p.y, z);
			}
		});
	}
}

/* The hand-over that ends the localized pass 1 of LSCV and LRSCV: a workgroup adds its (cell, bin) table to the target's u32 sums; the
 * last one of the target to arrive adds the cells of each sub-region, writes the maps (map[b] = sum / count, or b where the count is 0),
 * zeroes the sums for the next launch and, with affine_mapping, fits map_r[k] ~ a_r k + c_r over k = 0 .. n_bins - 1 in FP64.  Which bin
 * keys the table (the template's for LSCV, the current patch's for LRSCV) and which value is summed is the caller's; the arithmetic here
 * is the same for both.  s_tab: the workgroup's [2][ncell nb] table (sums, then counts), complete (after a __syncthreads) */
__device__ __forceinline__ void lscv_hand_over(const ImapArgs &a, int t, int nblk, unsigned *s_tab, int &s_last) {
	const int nb = a.nb, E = a.ncell * nb;
	unsigned *s_sum = s_tab, *s_cnt = s_tab + E;
	unsigned *tot = a.tot + (size_t)t * 2 * E;
	for (int e = threadIdx.x; e < 2 * E; e += kBlock) {
		const unsigned v = s_tab[e];
		if (v) __hip_atomic_fetch_add(tot + e, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	/* the last workgroup of the target to arrive builds the maps (acknowledged sums, then an agent-scope arrival) */
	wait_stores_acked();
	__syncthreads();
	if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(a.arrive + t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nblk - 1u;
	__syncthreads();
	if (!s_last) return;
	if (threadIdx.x == 0) st_coh(a.arrive + t, 0u);
	for (int e = threadIdx.x; e < 2 * E; e += kBlock) { s_tab[e] = ld_coh(tot + e); st_coh(tot + e, 0u); }
	__syncthreads();
	/* LSCV.cc:274-285 / LRSCV.cc:263-277: intensity_map(b) = (the bin's sum) / (its count), or b where the count is 0 */
	const int nx = a.nx, R = a.nx * a.ny;
	double *map = a.map + (size_t)t * R * nb;
	for (int e = threadIdx.x; e < R * nb; e += kBlock) {
		const int r = e / nb, b = e - r * nb, idx = r % nx, idy = r / nx;
		const int cx0 = a.crng[2 * idx], cx1 = a.crng[2 * idx + 1], cy0 = a.crng[2 * nx + 2 * idy], cy1 = a.crng[2 * nx + 2 * idy + 1];
		unsigned long long s = 0, c = 0;
		for (int cy = cy0; cy <= cy1; ++cy)
			for (int cx = cx0; cx <= cx1; ++cx) {
				const int k = (cy * a.ncx + cx) * nb + b;
				s += s_sum[k]; c += s_cnt[k];
			}
		st_coh(map + e, c == 0 ? (double)b : (double)s / (double)c);
	}
	if (!a.affine) return;
	wait_stores_acked();
	__syncthreads();
	/* affine_mapping (LSCV.cc:286-288, LRSCV.cc:279-281): least squares of map against [k, 1], k = 0 .. n_bins - 1, by the normal equations; sum k and
	 * sum k^2 are exact integers */
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (int r = wave; r < R; r += kBlock / 64) {
		double sm = 0.0, skm = 0.0;
		for (int k = lane; k < nb; k += 64) { const double m = ld_coh(map + (size_t)r * nb + k); sm += m; skm += (double)k * m; }
#pragma unroll
		for (int off = 32; off >= 1; off >>= 1) { sm += __shfl_xor(sm, off); skm += __shfl_xor(skm, off); }
		if (lane == 0) {
			const double n = (double)nb, sk = (double)nb * (nb - 1) / 2, skk = (double)(nb - 1) * nb * (2 * nb - 1) / 6;
			const double det = n * skk - sk * sk;
			a.aff[((size_t)t * R + r) * 2] = (n * skm - sk * sm) / det;
			a.aff[((size_t)t * R + r) * 2 + 1] = (skk * sm - sk * skm) / det;
		}
	}
}

} // namespace mtfhip
#endif
