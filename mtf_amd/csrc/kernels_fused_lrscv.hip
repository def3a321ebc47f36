/*
 * kernels_fused_lrscv.hip -- the fused Lucas-Kanade iteration for the Localized Reversed SCV appearance model (AM/src/LRSCV.cc):
 * fused_lk_body (mtfhip_fused_device.h) instantiated with AM = MTFHIP_AM_LRSCV, i.e. SSD on the current patch whose every sample is
 * replaced, right after it is taken, by the per-pixel blend of its images through the target's sub-region maps.  The maps come from
 * pass 1 (kernels_lrscv.hip), enqueued in front of every launch that maps.  A translation unit of its own, so that the instantiations of
 * kernels_fused.hip and kernels_fused_rscv.hip stay exactly what they were.
 */
#include "mtfhip_fused_device.h"

namespace mtfhip {

template <int SSM, bool CHAINED, int MODE, bool MAT>
__global__ __launch_bounds__(kBlock, MTFHIP_FUSED_WAVES) void k_fused_lrscv(BatchView bv, ImgView im, FusedArgs fa, double *partials, int nblk,
	LrscvMap lm) {
	fused_lk_body<MTFHIP_AM_LRSCV, SSM, CHAINED, MODE, MAT>(bv, im, fa, partials, nblk, RscvMap{}, lm);
}
/* tolerance-mode lean launches */
template <int SSM, int MODE, bool CHAINED>
__global__ __launch_bounds__(kBlock, MTFHIP_FAST_WAVES) void k_fused_lrscv_fast(BatchView bv, ImgView im, FusedArgs fa, double *partials, int nblk,
	LrscvMap lm) {
	fused_lk_body<MTFHIP_AM_LRSCV, SSM, CHAINED, MODE, false, true>(bv, im, fa, partials, nblk, RscvMap{}, lm);
}

/* the maps live in the dynamic LDS: R nb doubles, or 2 R with affine_mapping (api_lrscv.hip keeps them within 64 KB less the kernel's
 * static arrays) */
static size_t lrscv_lds(const LrscvMap &lm) { return sizeof(double) * (size_t)(lm.affine ? 2 * lm.R : lm.R * lm.nb); }
template <int SSM, bool CHAINED, int MODE>
static void launch_lrscv_mat(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const LrscvMap &lm,
	hipStream_t st) {
	const dim3 g = grid2(nblk, bv.B);
	const size_t lds = lrscv_lds(lm);
	if (fa.materialize) MTFHIP_LAUNCH((k_fused_lrscv<SSM, CHAINED, MODE, true>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, lm);
	else MTFHIP_LAUNCH((k_fused_lrscv<SSM, CHAINED, MODE, false>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, lm);
}
template <int SSM, bool CHAINED>
static void launch_lrscv_mode(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const LrscvMap &lm,
	hipStream_t st) {
	if (fa.mode == 0) launch_lrscv_mat<SSM, CHAINED, 0>(bv, im, fa, partials, nblk, lm, st);
	else if (fa.mode == 1) launch_lrscv_mat<SSM, CHAINED, 1>(bv, im, fa, partials, nblk, lm, st);
	else launch_lrscv_mat<SSM, CHAINED, 2>(bv, im, fa, partials, nblk, lm, st);
}
/* the same choice of instantiation as launch_fused_fast (kernels_fused.hip): rscv_it_kind (api_rscv.hip) mirrors it for pass 1 (k_lrscv_hist) */
template <int SSM>
static void launch_lrscv_fast(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const LrscvMap &lm,
	hipStream_t st) {
	const dim3 g = grid2(nblk, bv.B);
	const size_t lds = lrscv_lds(lm);
	if (fa.mode == 2) MTFHIP_LAUNCH((k_fused_lrscv_fast<SSM, 2, true>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, lm);
	else if (fa.mode == 0 && fa.chained) MTFHIP_LAUNCH((k_fused_lrscv_fast<SSM, 0, true>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, lm);
	else if (fa.mode == 0) MTFHIP_LAUNCH((k_fused_lrscv_fast<SSM, 0, false>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, lm);
	else if (fa.chained) MTFHIP_LAUNCH((k_fused_lrscv_fast<SSM, 1, true>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, lm);
	else MTFHIP_LAUNCH((k_fused_lrscv_fast<SSM, 1, false>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, lm);
}
void launch_fused_lrscv(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const LrscvMap &lm,
	hipStream_t st) {
	const bool hom = bv.ssm == MTFHIP_SSM_HOMOGRAPHY;
	if (fa.fast_math && !fa.materialize) {
		if (hom) launch_lrscv_fast<MTFHIP_SSM_HOMOGRAPHY>(bv, im, fa, partials, nblk, lm, st);
		else launch_lrscv_fast<MTFHIP_SSM_AFFINE>(bv, im, fa, partials, nblk, lm, st);
		return;
	}
	if (hom && fa.chained) launch_lrscv_mode<MTFHIP_SSM_HOMOGRAPHY, true>(bv, im, fa, partials, nblk, lm, st);
	else if (hom) launch_lrscv_mode<MTFHIP_SSM_HOMOGRAPHY, false>(bv, im, fa, partials, nblk, lm, st);
	else if (fa.chained) launch_lrscv_mode<MTFHIP_SSM_AFFINE, true>(bv, im, fa, partials, nblk, lm, st);
	else launch_lrscv_mode<MTFHIP_SSM_AFFINE, false>(bv, im, fa, partials, nblk, lm, st);
}

} // namespace mtfhip
