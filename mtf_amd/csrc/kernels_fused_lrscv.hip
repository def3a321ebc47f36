/*
 * kernels_fused_lrscv.hip -- the fused Lucas-Kanade iteration for the Localized Reversed SCV appearance model (AM/src/LRSCV.cc):
 * fused_lk_body (mtfhip_fused_device.h) instantiated with AM = MTFHIP_AM_LRSCV, i.e. SSD on the current patch whose every sample is
 * replaced, right after it is taken, by the per-pixel blend of its images through the target's sub-region maps.  The maps come from
 * pass 1 (kernels_imap.hip), enqueued in front of every launch that maps.  A translation unit of its own, so that the instantiations of
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

/* the maps live in the dynamic LDS: R nb doubles, or 2 R with affine_mapping (api_imap.hip keeps them within 64 KB less the kernel's
 * static arrays) */
static size_t lrscv_lds(const LrscvMap &lm) { return sizeof(double) * (size_t)(lm.affine ? 2 * lm.R : lm.R * lm.nb); }
void launch_fused_lrscv(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const LrscvMap &lm,
	hipStream_t st) {
	const dim3 g = grid2(nblk, bv.B);
	const size_t lds = lrscv_lds(lm);
	const FusedKey k = fused_select(FUSED_ROUTE_LOOP, MTFHIP_AM_LRSCV, bv.C, bv.ssm, fa.mode, fa.chained, fa.materialize, fa.fast_math);
	const bool launched = fused_visit<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_LRSCV>>(k, [&](auto, auto SSM, auto CH, auto MD, auto MAT, auto FAST) {
		if constexpr (FAST())
			MTFHIP_LAUNCH((k_fused_lrscv_fast<SSM(), MD(), CH()>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, lm);
		else
			MTFHIP_LAUNCH((k_fused_lrscv<SSM(), CH(), MD(), MAT()>), g, dim3(kBlock), lds, st, bv, im, fa, partials, nblk, lm);
	});
	if (!launched) note_launch_error(hipErrorInvalidDeviceFunction, __FILE__, __LINE__);   /* (no kernel for this launch: an error, not a skipped pass) */
}

} // namespace mtfhip
