/*
 * kernels_fused_spss.hip -- the fused Lucas-Kanade iteration for the Sum of Pixelwise Structural Similarity appearance model
 * (AM/src/SPSS.cc): fused_lk_body (mtfhip_fused_device.h) instantiated with AM = MTFHIP_AM_SPSS.  One pixel pass, no moments and no
 * histogram: per pixel the score f_vec = (2 I0 It + c) / (I0^2 + It^2 + c), the gradient entries df_dIt and df_dI0 (not each other's
 * negative) and the weight of the pixel's outer product in the Hessian the search method asked for (SpssArgs), into the 56-wide row --
 * ACC_H the weighted Gram matrix, ACC_G sum df_dIt row, ACC_G2 sum df_dI0 J0 row, ACC_RR sum f_vec.  A materialising launch also writes
 * df_dIt / df_dI0 beside It, dIt_dx and Jt.  The two-launch loop only (fused_select); the finish over these rows is k_finish_track_spss
 * (below: finish_track_body's SPSS form).  A translation unit of its own, so that the SSD / NCC instantiations of kernels_fused.hip stay exactly what they were.
 */
#include "mtfhip_finish_kernel.h"
#include "mtfhip_fused_device.h"

namespace mtfhip {

template <int SSM, bool CHAINED, int MODE, bool MAT>
__global__ __launch_bounds__(kBlock, MTFHIP_FUSED_WAVES) void k_fused_spss(BatchView bv, ImgView im, FusedArgs fa, double *partials, int nblk,
	SpssArgs sp) {
	fused_lk_body<MTFHIP_AM_SPSS, SSM, CHAINED, MODE, MAT>(bv, im, fa, partials, nblk, RscvMap{}, LrscvMap{}, sp);
}
/* tolerance-mode lean launches */
template <int SSM, int MODE, bool CHAINED>
__global__ __launch_bounds__(kBlock, MTFHIP_FAST_WAVES) void k_fused_spss_fast(BatchView bv, ImgView im, FusedArgs fa, double *partials, int nblk,
	SpssArgs sp) {
	fused_lk_body<MTFHIP_AM_SPSS, SSM, CHAINED, MODE, false, true>(bv, im, fa, partials, nblk, RscvMap{}, LrscvMap{}, sp);
}

/* the finish over the rows of an SPSS pass (finish_track_body's SPSS form): f, g and H read with SPSS's signs and its two
 * gemvs, solved with pivoting, in both arithmetic modes (api_track.hip leaves fast_finish off for it) */
__global__ __launch_bounds__(256) void k_finish_track_spss(BatchView bv, mtfhip_sm_desc sm, TrackState ts,
	const double *partials, int nblk, PhaseCtl pc, HostPublish pub, int pub_t0) {
	finish_track_kernel<false, true>(bv, sm, ts, partials, nblk, pc, pub, pub_t0);
}
void launch_finish_track_spss(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts, const double *partials, int nblk,
	hipStream_t st, PhaseCtl pc, const HostPublish &pub, int pub_t0, dim3 block) {
	MTFHIP_LAUNCH(k_finish_track_spss, dim3(bv.B), block, 0, st, bv, sm, ts, partials, nblk, pc, pub, pub_t0);
}

void launch_fused_spss(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const SpssArgs &sp,
	hipStream_t st) {
	const dim3 g = grid2(nblk, bv.B);
	const FusedKey k = fused_select(FUSED_ROUTE_LOOP, MTFHIP_AM_SPSS, bv.C, bv.ssm, fa.mode, fa.chained, fa.materialize, fa.fast_math);
	const bool launched = fused_visit<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_SPSS>>(k, [&](auto, auto SSM, auto CH, auto MD, auto MAT, auto FAST) {
		if constexpr (FAST())
			MTFHIP_LAUNCH((k_fused_spss_fast<SSM(), MD(), CH()>), g, dim3(kBlock), 0, st, bv, im, fa, partials, nblk, sp);
		else
			MTFHIP_LAUNCH((k_fused_spss<SSM(), CH(), MD(), MAT()>), g, dim3(kBlock), 0, st, bv, im, fa, partials, nblk, sp);
	});
	if (!launched) note_launch_error(hipErrorInvalidDeviceFunction, __FILE__, __LINE__);   /* (no kernel for this launch: an error, not a skipped pass) */
}

} // namespace mtfhip
