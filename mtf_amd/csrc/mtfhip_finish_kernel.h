/*
 * mtfhip_finish_kernel.h -- the body of the stand-alone finish kernels of the two-launch loop: k_finish_track and k_finish_track_lo
 * (kernels_fused.hip), k_finish_track_spss (kernels_fused_spss.hip), k_finish_track_ssim and k_finish_track_ssim_lo (kernels_ssim.hip).  finish_track_body / finish_track_fast_body (mtfhip_finish_device.h) plus
 * the launch's own business: issue priority, the delivery of a stopped target to the host, the queues' phase stamps.
 */
#ifndef MTFHIP_FINISH_KERNEL_H
#define MTFHIP_FINISH_KERNEL_H
#include "mtfhip_finish_device.h"
#include "mtfhip_grid_device.h"

namespace mtfhip {

/* ===================================================================== */
/* the stand-alone finish kernels' body (k_finish_track, k_finish_track_lo: kernels_fused.hip; k_finish_track_spss: kernels_fused_spss.hip) */
/* ===================================================================== */
/* pc (two-queue loop): the queues run best half a period apart -- one's fill / drain / solve under the other's streaming (48-49 us per
 * step of 64 x 200 x 200, the two pixel passes starting 23-25 us apart) -- but started together, or on some boxes by themselves, they
 * stay close to lockstep (55-56 us).  Each queue's solve stamps the wall clock when it ends, and ends no sooner than `frac` of its own
 * last period after the other queue's stamp: a queue that runs too close behind the other is held back until it is not. */
/* ts.finish_prio: the waves of this launch raise their issue priority once, at entry (a kernel argument: a scalar branch around one
 * s_setprio, no per-segment flips) and drop it again in front of the phase spin, which sleeps.
 * pub.host (the chunked loop's fused delivery, api_track.hip): a target's wave hands the target's warp, state, corners and iteration count to
 * the host exactly once -- in the pass that stops it, or in the last pass the host enqueues (ts.last_pass) if it is still active then -- with
 * the hand-over of publish_target; the arrivals of all passes and both queues count to pub.B, the last one raises the host's flag.  pub_t0:
 * the launch's first target in the batch (bv and ts are the chunk's views). */
/* SSIM (k_finish_track_ssim / _ssim_lo, kernels_ssim.hip): finish_track_body's SSIM form over an NCC pass's rows, with the model's constants */
template <bool LO, bool SPSS = false, bool SSIM = false>
__device__ __forceinline__ void finish_track_kernel(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts,
	const double *partials, int nblk, const PhaseCtl &pc, const HostPublish &pub, int pub_t0, double ssim_c1 = 0.0, double ssim_c2 = 0.0) {
	if (ts.finish_prio) __builtin_amdgcn_s_setprio(3);
	const int t = blockIdx.x;
	__shared__ int s_stopped;
	if (pub.host && threadIdx.x == 0) __hip_atomic_store(&s_stopped, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
	if constexpr (SSIM) finish_track_body<false, false, LO, false, true>(bv, sm, ts, partials, nblk, t, pub.host ? &s_stopped : nullptr, ssim_c1, ssim_c2);
	else if constexpr (SPSS) finish_track_body<false, false, false, true>(bv, sm, ts, partials, nblk, t, pub.host ? &s_stopped : nullptr);
	else if constexpr (LO) finish_track_body<false, false, true>(bv, sm, ts, partials, nblk, t, pub.host ? &s_stopped : nullptr);
	else if (ts.fast_finish) finish_track_fast_body(bv, sm, ts, partials, nblk, t, pub.host ? &s_stopped : nullptr);
	else finish_track_body(bv, sm, ts, partials, nblk, t, pub.host ? &s_stopped : nullptr);
	if (pub.host && threadIdx.x < 64) {
		/* the first wave alone: its lane 0 cleared and set the flag (1: active at entry, 3: stopped by this pass), and everything the bodies leave
		 * for the host is stored by lanes of this wave -- the warp's entry q by lane q; the state by lane 0 (finish_track_body) or entry q by
		 * lane q (the fast body); the corners' entries 2q and 2q + 1 by lane q < 4 (finish_track_body) or entry q by lane q; the iteration
		 * count by lane 0.  Lane q reads entry q back, so some entries cross lanes: that is in order at wavefront scope (the stores are
		 * issued before the loads of the same wave, to the same addresses), which is all this needs -- no barrier and no wait for the stores
		 * on the passes that deliver nothing */
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		const int ran = __hip_atomic_load(&s_stopped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
		if (ran == 3 || (ran && ts.last_pass)) {
			const int lane = threadIdx.x;
			const double wq = lane < 9 ? bv.warps[9 * t + lane] : 0.0, sq = lane < 8 ? bv.states[8 * t + lane] : 0.0, cq = lane < 8 ? ts.corners[8 * t + lane] : 0.0;
			publish_target(pub, pub_t0 + t, wq, sq, cq, __hip_atomic_load(ts.n_iters + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT), pub.B);
		}
	}
	if (ts.finish_prio) __builtin_amdgcn_s_setprio(0);
	if (pc.mine && blockIdx.x == 0 && threadIdx.x == 0) {
		const unsigned long long prev = ld_coh(pc.mine), other = ld_coh(pc.other);
		unsigned long long now = wall_clock64();   /* 100 MHz */
		if (prev && other && now > prev && now - prev < 50000ull) {   /* (a period of less than 500 us: the queue is in its stride) */
			const unsigned long long min_lag = (unsigned long long)((double)(now - prev) * pc.frac);
			while (now > other && now - other < min_lag) { __builtin_amdgcn_s_sleep(8); now = wall_clock64(); }
		}
		st_coh(pc.mine, now);
	}
}



} // namespace mtfhip
#endif
