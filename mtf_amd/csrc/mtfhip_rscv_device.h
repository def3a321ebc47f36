/*
 * mtfhip_rscv_device.h -- It_orig of the current-patch intensity maps (RSCV: kernels_rscv.hip, LRSCV: kernels_lrscv.hip), sampled with
 * the arithmetic of the fused pass that follows the map's pass 1 (see kernels_rscv.hip's header: bin agreement)
 */
#ifndef MTFHIP_RSCV_DEVICE_H
#define MTFHIP_RSCV_DEVICE_H
#include "mtfhip_fused_device.h"

namespace mtfhip {

/* It_orig of one pixel, as the fused pass computes it (kernels_rscv.hip's header); called by every lane of a wave whose pixel is < N;
 * a: norm_mult, norm_add, grad_eps (RscvArgs, LrscvArgs) */
template <int SSM, int KIND, class A>
__device__ __forceinline__ double rscv_it_orig(const ImgView &im, const Warp9 &W, const A &a, double hx, double hy, double z) {
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

} // namespace mtfhip
#endif
