/*
 * kernels_fused_rscv.hip -- the fused Lucas-Kanade iteration for the Reversed SCV appearance model (AM/src/RSCV.cc): fused_lk_body
 * (mtfhip_fused_device.h) instantiated with AM = MTFHIP_AM_RSCV, i.e. SSD on the current patch mapped through the target's intensity
 * map right after it is sampled.  The maps come from pass 1 (kernels_imap.hip), enqueued in front of every launch.  A translation unit
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
void launch_fused_rscv(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const RscvMap &rm,
	hipStream_t st) {
	const dim3 g = grid2(nblk, bv.B);
	const size_t lds = sizeof(double) * (size_t)rm.nb;
	const FusedKey k = fused_select(FUSED_ROUTE_LOOP, MTFHIP_AM_RSCV, bv.C, bv.ssm, fa.mode, fa.chained, fa.materialize, fa.fast_math);
	const bool launched = fused_visit<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_RSCV>>(k, [&](auto, auto SSM, auto CH, auto MD, auto MAT, auto FAST) {
		if constexpr (FAST())
			MTFHIP_LAUNCH((k_fused_rscv_fast<SSM(), MD(), CH()>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, rm);
		else
			MTFHIP_LAUNCH((k_fused_rscv<SSM(), CH(), MD(), MAT()>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, rm);
	});
	if (!launched) note_launch_error(hipErrorInvalidDeviceFunction, __FILE__, __LINE__);   /* (no kernel for this launch: an error, not a skipped pass) */
}

} // namespace mtfhip
