/*
 * kernels_fused_mc.hip -- the fused Lucas-Kanade iteration of the multi-channel appearance models (MCSSD, MCNCC: SSD / NCC with
 * n_channels = 3, AM/src/MCSSD.cc, AM/src/MCNCC.cc over Utilities/src/imgUtils.cc:861-1005).  One of the translation units of
 * libmtfhip.so; the body is fused_lk_body<..., MC = true> (mtfhip_fused_device.h): one launch per iteration, a thread per
 * (pixel, channel) row, the pixel's grid point shared by its C rows, the partial rows those of the single-channel pass
 * (so k_finish_track, the host assembly and the NCC moment algebra serve both).  Launches that materialise nothing take the
 * tolerance-mode form (k_fused_mc_fast) unless the batch is in replay arithmetic.
 */
#include "mtfhip_fused_device.h"

namespace mtfhip {

template <int AM, int SSM, bool CHAINED, int MODE, bool MAT>
__global__ __launch_bounds__(kBlock, MTFHIP_FUSED_WAVES) void k_fused_mc(BatchView bv, ImgView im, FusedArgs fa, double *partials, int nblk) {
	fused_lk_body<AM, SSM, CHAINED, MODE, MAT, false, false, true>(bv, im, fa, partials, nblk);
}

/* tolerance-mode lean launches (FAST: closed-form gradient of the channel's bilinear cell, reciprocals, FMAs; see fused_lk_body) */
template <int AM, int SSM, int MODE, bool CHAINED>
__global__ __launch_bounds__(kBlock, MTFHIP_FAST_WAVES) void k_fused_mc_fast(BatchView bv, ImgView im, FusedArgs fa, double *partials, int nblk) {
	fused_lk_body<AM, SSM, CHAINED, MODE, false, true, false, true>(bv, im, fa, partials, nblk);
}
void launch_fused_mc(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, hipStream_t st) {
	const dim3 g = grid2(nblk, bv.B);
	/* (mapped = false: launch_fused_ssd hands the launches with maps to their own units) */
	const FusedKey k = fused_select(FUSED_ROUTE_LOOP, bv.am, bv.C, bv.ssm, fa.mode, fa.chained, fa.materialize, fa.fast_math, false);
	const bool launched = fused_visit<FusedUnit<FUSED_ROUTE_LOOP, true, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>(k, [&](auto AM, auto SSM, auto CH, auto MD, auto MAT, auto FAST) {
		if constexpr (FAST())
			MTFHIP_LAUNCH((k_fused_mc_fast<AM(), SSM(), MD(), CH()>), g, dim3(kBlock), 0, st, bv, im, fa, partials, nblk);
		else
			MTFHIP_LAUNCH((k_fused_mc<AM(), SSM(), CH(), MD(), MAT()>), g, dim3(kBlock), 0, st, bv, im, fa, partials, nblk);
	});
	if (!launched) note_launch_error(hipErrorInvalidDeviceFunction, __FILE__, __LINE__);   /* (no kernel for this launch: an error, not a skipped pass) */
}

} // namespace mtfhip
