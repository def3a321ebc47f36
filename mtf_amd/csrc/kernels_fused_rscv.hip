/*
 * kernels_fused_rscv.hip -- the fused Lucas-Kanade iteration for the Reversed SCV appearance model (AM/src/RSCV.cc): fused_lk_body
 * (mtfhip_fused_device.h) instantiated with AM = MTFHIP_AM_RSCV, i.e. SSD on the current patch mapped through the target's intensity
 * map right after it is sampled.  The maps come from pass 1 (kernels_rscv.hip), enqueued in front of every launch.  A translation unit
 * of its own, so that the SSD / NCC instantiations of kernels_fused.hip stay exactly what they were.
 */
#include "mtfhip_fused_device.h"

namespace mtfhip {

template <int SSM, bool CHAINED, int MODE, bool MAT>
__global__ __launch_bounds__(kBlock, MTFHIP_FUSED_WAVES) void k_fused_rscv(BatchView bv, ImgView im, FusedArgs fa, double *partials, int nblk,
	RscvMap rm) {
	fused_lk_body<MTFHIP_AM_RSCV, SSM, CHAINED, MODE, MAT>(bv, im, fa, partials, nblk, rm);
}
/* tolerance-mode lean launches */
template <int SSM, int MODE, bool CHAINED>
__global__ __launch_bounds__(kBlock, MTFHIP_FAST_WAVES) void k_fused_rscv_fast(BatchView bv, ImgView im, FusedArgs fa, double *partials, int nblk,
	RscvMap rm) {
	fused_lk_body<MTFHIP_AM_RSCV, SSM, CHAINED, MODE, false, true>(bv, im, fa, partials, nblk, rm);
}

/* the map lives in the dynamic LDS: nb doubles */
template <int SSM, bool CHAINED, int MODE>
static void launch_rscv_mat(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const RscvMap &rm,
	hipStream_t st) {
	const dim3 g = grid2(nblk, bv.B);
	const size_t lds = sizeof(double) * (size_t)rm.nb;
	if (fa.materialize) MTFHIP_LAUNCH((k_fused_rscv<SSM, CHAINED, MODE, true>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, rm);
	else MTFHIP_LAUNCH((k_fused_rscv<SSM, CHAINED, MODE, false>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, rm);
}
template <int SSM, bool CHAINED>
static void launch_rscv_mode(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const RscvMap &rm,
	hipStream_t st) {
	if (fa.mode == 0) launch_rscv_mat<SSM, CHAINED, 0>(bv, im, fa, partials, nblk, rm, st);
	else if (fa.mode == 1) launch_rscv_mat<SSM, CHAINED, 1>(bv, im, fa, partials, nblk, rm, st);
	else launch_rscv_mat<SSM, CHAINED, 2>(bv, im, fa, partials, nblk, rm, st);
}
/* the same choice of instantiation as launch_fused_fast (kernels_fused.hip): rscv_it_kind (api_rscv.hip) mirrors it for pass 1 */
template <int SSM>
static void launch_rscv_fast(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const RscvMap &rm,
	hipStream_t st) {
	const dim3 g = grid2(nblk, bv.B);
	const size_t lds = sizeof(double) * (size_t)rm.nb;
	if (fa.mode == 2) MTFHIP_LAUNCH((k_fused_rscv_fast<SSM, 2, true>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, rm);
	else if (fa.mode == 0 && fa.chained) MTFHIP_LAUNCH((k_fused_rscv_fast<SSM, 0, true>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, rm);
	else if (fa.mode == 0) MTFHIP_LAUNCH((k_fused_rscv_fast<SSM, 0, false>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, rm);
	else if (fa.chained) MTFHIP_LAUNCH((k_fused_rscv_fast<SSM, 1, true>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, rm);
	else MTFHIP_LAUNCH((k_fused_rscv_fast<SSM, 1, false>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, rm);
}
void launch_fused_rscv(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const RscvMap &rm,
	hipStream_t st) {
	const bool hom = bv.ssm == MTFHIP_SSM_HOMOGRAPHY;
	if (fa.fast_math && !fa.materialize) {
		if (hom) launch_rscv_fast<MTFHIP_SSM_HOMOGRAPHY>(bv, im, fa, partials, nblk, rm, st);
		else launch_rscv_fast<MTFHIP_SSM_AFFINE>(bv, im, fa, partials, nblk, rm, st);
		return;
	}
	if (hom && fa.chained) launch_rscv_mode<MTFHIP_SSM_HOMOGRAPHY, true>(bv, im, fa, partials, nblk, rm, st);
	else if (hom) launch_rscv_mode<MTFHIP_SSM_HOMOGRAPHY, false>(bv, im, fa, partials, nblk, rm, st);
	else if (fa.chained) launch_rscv_mode<MTFHIP_SSM_AFFINE, true>(bv, im, fa, partials, nblk, rm, st);
	else launch_rscv_mode<MTFHIP_SSM_AFFINE, false>(bv, im, fa, partials, nblk, rm, st);
}

} // namespace mtfhip
