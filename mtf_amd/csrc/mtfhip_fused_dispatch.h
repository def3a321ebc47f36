/*
 * mtfhip_fused_dispatch.h -- which instantiation of fused_lk_body (mtfhip_fused_device.h) a launch runs, and the visitor that turns that
 * choice into template arguments.  Host-only and free of the HIP runtime (it needs include/mtfhip.h for the enums and nothing else), so
 * that the table can be checked by a stand-alone program (tests/test_fused_dispatch.py).
 *
 * fused_select() is the one place that knows how the runtime choice -- appearance model, channels, state-space model, search method's
 * mode, chained warp, materialising or lean, replay or tolerance arithmetic -- becomes the key {AM, SSM, CHAINED, MODE, MAT, FAST} of a
 * kernel, and which choices each of the three routes serves.  The seven translation units that instantiate fused_lk_body keep their
 * __global__ wrappers and call fused_visit() with a generic lambda that names the wrapper; rscv_it_kind, grid_regen_kernel and
 * track_step_available are read off the same key.  A new appearance model adds its line to fused_select() and a unit with its wrappers.
 */
#ifndef MTFHIP_FUSED_DISPATCH_H
#define MTFHIP_FUSED_DISPATCH_H

#include <type_traits>
#include <utility>
#include "../../include/mtfhip.h"

namespace mtfhip {

/* the three routes of a Lucas-Kanade pass: the two-launch loop (kernels_fused*.hip: pixel pass, then k_finish_track; also a single
 * iterate), one launch per pass (kernels_step.hip), one launch per loop (kernels_persist.hip) */
enum { FUSED_ROUTE_LOOP = 0, FUSED_ROUTE_STEP = 1, FUSED_ROUTE_PERSIST = 2 };

/* how pass 1 of RSCV / LRSCV obtains It_orig -- the expression of the fused pass it runs in front of (fused_it_kind), so that every
 * pixel lands in the bin the fused pass looks it up in: replay (MATH_REPLAY, every materialising launch); tolerance mode ICLK, chained
 * FCLK / ESM, non-chained FCLK / ESM (each with its own interior test, mtfhip_fused_device.h); or read from the It_orig buffer
 * (per-function path) */
enum { RSCV_IT_REPLAY = 0, RSCV_IT_FAST_ICLK = 1, RSCV_IT_FAST_CHAINED = 2, RSCV_IT_FAST_QSTEP = 3, RSCV_IT_FROM_BUF = 4 };

/* the template arguments of one instantiation; mc: the multi-channel body (MC = true, kernels_fused_mc.hip); served = false: the route
 * has no kernel for the input, and the other fields say nothing */
struct FusedKey {
	int am, ssm, mode;     /* MTFHIP_AM_SSD / _NCC (also an SSIM batch's) / _RSCV / _LRSCV / _SPSS ; MTFHIP_SSM_* ; 0 FCLK, 1 ESM, 2 ICLK */
	bool chained, mat, fast, mc, served;
};
constexpr bool operator==(const FusedKey &a, const FusedKey &b) {
	return a.served == b.served && (!a.served || (a.am == b.am && a.ssm == b.ssm && a.mode == b.mode && a.chained == b.chained &&
		a.mat == b.mat && a.fast == b.fast && a.mc == b.mc));
}

/* mapped: the launch has the intensity maps of a pass 1 enqueued in front of it (RSCV: always; LRSCV: not on the later passes of a frame
 * under once_per_frame, LRSCV.cc:234-235) */
constexpr FusedKey fused_select(int route, int am, int channels, int ssm, int mode, bool chained, bool materialize, bool fast_math,
	bool mapped = true) {
	FusedKey k{};
	/* the appearance model of the kernel: SCV and LSCV re-map the template between the passes and run SSD on it; MI takes It and the
	 * Jacobians a materialising SSD pass writes and ignores its sums (mi_enqueue, api_mi_iter.hip); RSCV and LRSCV map the current patch
	 * inside the pass (an LRSCV pass without maps is an SSD pass on the raw patch; an RSCV one is not launched) */
	switch (am) {
	case MTFHIP_AM_SSD: case MTFHIP_AM_SCV: case MTFHIP_AM_LSCV: case MTFHIP_AM_MI: k.am = MTFHIP_AM_SSD; break;
	case MTFHIP_AM_NCC: k.am = MTFHIP_AM_NCC; break;
	case MTFHIP_AM_RSCV: if (!mapped) return k; k.am = MTFHIP_AM_RSCV; break;
	case MTFHIP_AM_LRSCV: k.am = mapped ? MTFHIP_AM_LRSCV : MTFHIP_AM_SSD; break;
	/* SPSS (kernels_fused_spss.hip): single channel, the two-launch loop only (`plain` below keeps it off the one-launch routes) */
	case MTFHIP_AM_SPSS: if (channels != 1) return k; k.am = MTFHIP_AM_SPSS; break;
	/* SSIM: every quantity of SSIM.cc is a function of the raw moments an NCC pass reduces (mtfhip_sm_system.h), so its launches ARE NCC's
	 * kernels; single channel, the two-launch loop only -- the finish that reads the row as SSIM is k_finish_track_ssim (kernels_ssim.hip) */
	case MTFHIP_AM_SSIM: if (channels != 1) return k; k.am = MTFHIP_AM_NCC; break;
	default: return k;
	}
	/* the mapping kernels take every row as a pixel of one plane; MCSSD / MCNCC are SSD / NCC with the multi-channel body */
	k.mc = channels > 1 && k.am != MTFHIP_AM_RSCV && k.am != MTFHIP_AM_LRSCV;
	k.ssm = ssm == MTFHIP_SSM_HOMOGRAPHY ? MTFHIP_SSM_HOMOGRAPHY : MTFHIP_SSM_AFFINE;
	k.mode = mode == 0 ? 0 : (mode == 1 ? 1 : 2);
	/* the tolerance-mode (lean) form materialises nothing; its ICLK body takes no gradient and is instantiated once, as CHAINED */
	k.fast = fast_math && !materialize;
	k.mat = materialize;
	k.chained = chained || (k.fast && k.mode == 2);
	/* the one-launch routes take single-channel SSD and NCC (an intensity map is rebuilt between the passes by launches of its own) */
	const bool plain = channels == 1 && (am == MTFHIP_AM_SSD || am == MTFHIP_AM_NCC);
	switch (route) {
	case FUSED_ROUTE_LOOP: k.served = true; break;
	/* the two forms the device-side loop launches by default: lean in tolerance arithmetic, materialising in replay arithmetic */
	case FUSED_ROUTE_STEP: k.served = plain && (k.fast || (!fast_math && materialize)); break;
	/* never materialises: the interface-visible arrays of an iteration are the two-launch loop's business */
	case FUSED_ROUTE_PERSIST: k.served = plain && !materialize; break;
	default: break;
	}
	return k.served ? k : FusedKey{};
}

/* a key is one the route can launch iff it is what fused_select makes of its own fields */
constexpr bool fused_reachable(int route, const FusedKey &k) {
	return k.served && fused_select(route, k.am, k.mc ? 3 : 1, k.ssm, k.mode, k.chained, k.mat, k.fast) == k;
}

/* the It_orig expression of the fused launch with key k (rscv_it_orig, mtfhip_rscv_device.h) */
constexpr int fused_it_kind(const FusedKey &k) {
	return !k.fast ? RSCV_IT_REPLAY : (k.mode == 2 ? RSCV_IT_FAST_ICLK : (k.chained ? RSCV_IT_FAST_CHAINED : RSCV_IT_FAST_QSTEP));
}

/* the fused instantiations that carry the grid rebuild (FusedArgs::grid_regen): the materialising SSD launch, homography, chained
 * warp, FCLK or ESM -- the headline's kernel and its FCLK sibling, which keep their occupancy and stay clear of scratch with it
 * (-Rpass-analysis=kernel-resource-usage, profiles/r07_resource_usage.txt); the others (lean / NCC / affine / non-chained / ICLK /
 * mapping) would lose a wave per SIMD or spill, and read INIT_PTS; so do MI's launches of the SSD kernels */
constexpr bool fused_key_grid_regen(const FusedKey &k) {
	return k.served && !k.mc && !k.fast && k.am == MTFHIP_AM_SSD && k.ssm == MTFHIP_SSM_HOMOGRAPHY && k.chained && k.mode != 2 && k.mat;
}
/* the same for a single-channel launch in replay arithmetic on the two-launch route: on the device with a kernel's own template
 * arguments, on the host with the batch's */
constexpr bool grid_regen_kernel(int am, int ssm, bool chained, int mode, bool mat) {
	return am != MTFHIP_AM_MI && fused_key_grid_regen(fused_select(FUSED_ROUTE_LOOP, am, 1, ssm, mode, chained, mat, false));
}

/* ---- the visitor ---- */

/* what one translation unit instantiates: the route it serves, the body (MC) and the appearance models of its wrappers */
template <int ROUTE, bool MC, int... AMS>
struct FusedUnit {
	static constexpr int route = ROUTE;
	static constexpr int n_am = (int)sizeof...(AMS);
	static constexpr int count = n_am * 48;   /* x 2 SSM x 2 CHAINED x 3 MODE x 2 MAT x 2 FAST */
	static constexpr int am_at(int i) { constexpr int ams[] = {AMS...}; return ams[i]; }
	static constexpr FusedKey key(int i) {
		return FusedKey{am_at(i / 48), (i / 24) % 2 ? MTFHIP_SSM_AFFINE : MTFHIP_SSM_HOMOGRAPHY, (i / 4) % 3, (i / 12) % 2 != 0, (i / 2) % 2 != 0,
			i % 2 != 0, MC, true};
	}
	/* -1: not a key of this unit */
	static constexpr int index(const FusedKey &k) {
		if (!k.served || k.mc != MC) return -1;
		for (int a = 0; a < n_am; ++a)
			if (am_at(a) == k.am)
				return (((a * 2 + (k.ssm == MTFHIP_SSM_AFFINE)) * 2 + k.chained) * 3 + k.mode) * 4 + k.mat * 2 + k.fast;
		return -1;
	}
};

template <class U, int I, class F>
bool fused_visit_one(F &f) {
	constexpr FusedKey k = U::key(I);
	static_assert(U::index(k) == I, "FusedUnit: key() and index() disagree");
	/* only what fused_select can return for the unit's route is instantiated */
	if constexpr (fused_reachable(U::route, k)) {
		f(std::integral_constant<int, k.am>{}, std::integral_constant<int, k.ssm>{}, std::bool_constant<k.chained>{},
			std::integral_constant<int, k.mode>{}, std::bool_constant<k.mat>{}, std::bool_constant<k.fast>{});
		return true;
	}
	return false;
}
template <class U, class F, int... I>
bool fused_visit_seq(int idx, F &f, std::integer_sequence<int, I...>) {
	return ((idx == I && fused_visit_one<U, I>(f)) || ...);
}
/* calls f(AM, SSM, CHAINED, MODE, MAT, FAST) -- std::integral_constant tags -- for the instantiation k of unit U; false, and no call,
 * when k is not one of the unit's */
template <class U, class F>
bool fused_visit(const FusedKey &k, F &&f) {
	return fused_visit_seq<U>(U::index(k), f, std::make_integer_sequence<int, U::count>{});
}

} // namespace mtfhip

#endif
