/*
 * kernels_fused.hip -- the fused Lucas-Kanade iteration (SSD and NCC) and the device-side solve + update
 * (one of the translation units of libmtfhip.so; conventions and the shared device helpers: mtfhip_device.h)
 */
#include "mtfhip_finish_kernel.h"
#include "mtfhip_fused_device.h"
#include "mtfhip_grid_device.h"

namespace mtfhip {

template <int SSM, bool CHAINED, int MODE, bool MAT>
__global__ __launch_bounds__(kBlock, MTFHIP_FUSED_WAVES) void k_fused_ssd(BatchView bv, ImgView im, FusedArgs fa, double *partials, int nblk) {
	fused_lk_body<MTFHIP_AM_SSD, SSM, CHAINED, MODE, MAT>(bv, im, fa, partials, nblk);
}
template <int SSM, bool CHAINED, int MODE, bool MAT>
__global__ __launch_bounds__(kBlock, MTFHIP_FUSED_WAVES) void k_fused_ncc(BatchView bv, ImgView im, FusedArgs fa, double *partials, int nblk) {
	fused_lk_body<MTFHIP_AM_NCC, SSM, CHAINED, MODE, MAT>(bv, im, fa, partials, nblk);
}
/* tolerance-mode lean launches (see fused_lk_body) */
template <int AM, int SSM, int MODE, bool CHAINED>
__global__ __launch_bounds__(kBlock, MTFHIP_FAST_WAVES) void k_fused_fast(BatchView bv, ImgView im, FusedArgs fa, double *partials, int nblk) {
	fused_lk_body<AM, SSM, CHAINED, MODE, false, true>(bv, im, fa, partials, nblk);
}


/* stand-alone finish: one wave per target (finish_track_kernel, mtfhip_finish_kernel.h) */
__global__ __launch_bounds__(256) void k_finish_track(BatchView bv, mtfhip_sm_desc sm, TrackState ts,
	const double *partials, int nblk, PhaseCtl pc, HostPublish pub, int pub_t0) {
	finish_track_kernel<false>(bv, sm, ts, partials, nblk, pc, pub, pub_t0);
}
/* the same for a batch of a low-order SSM (TrackState::lo_ssm): finish_track_body with the projection and the model's update, in both arithmetic
 * modes (api_track.hip leaves fast_finish off for it) */
__global__ __launch_bounds__(256) void k_finish_track_lo(BatchView bv, mtfhip_sm_desc sm, TrackState ts,
	const double *partials, int nblk, PhaseCtl pc, HostPublish pub, int pub_t0) {
	finish_track_kernel<true>(bv, sm, ts, partials, nblk, pc, pub, pub_t0);
}

/* MI device-side loop: g and H of the fused MI passes (mi_H = [B][64] H column-major | [B][16] unused here | [B][64] second H of
 * SumOfStd; gpart = the gradient pass's block rows [B][ng][16]) laid out as the reduced row the finish reads for SSD --
 * ACC_H = upper triangle of -H, ACC_G = the Jacobian sum the search method scales (ESM halves it, NT/ESM.cc:246-255) -- and
 * the finish itself, in one launch.  gmode: 0 ICLK, 1 FCLK, 2 ESM Original, 3 ESM DiffOfJacs. */
__global__ __launch_bounds__(64) void k_finish_track_mi(BatchView bv, mtfhip_sm_desc sm, TrackState ts, int sum_std, int gmode,
	const double *mi_H, const double *gpart, int ng, double *rows) {
	const int t = blockIdx.x, lane = threadIdx.x, S = bv.S, B = bv.B;
	const double *Hs = mi_H + 64 * (size_t)t, *H2 = mi_H + 80 * (size_t)B + 64 * (size_t)t;
	double *row = rows + (size_t)t * ACC_COUNT;
	__shared__ double gs[16];
	if (lane < 16) gs[lane] = column_sum(gpart + (size_t)t * ng * 16 + lane, ng, 16);
	if (lane < ACC_COUNT - 36) row[36 + lane] = 0.0;
	const int a = lane >> 3, c = lane & 7;
	if (a <= c) {
		double hv = 0.0;
		if (c < S) { hv = Hs[c * S + a]; if (sum_std) hv = 0.5 * (hv + H2[c * S + a]); }
		row[ACC_H + a * 8 - (a * (a - 1)) / 2 + (c - a)] = -hv;
	}
	__syncthreads();
	if (lane < S) {
		const double gt = gs[lane], g0 = gs[8 + lane];
		row[ACC_G + lane] = gmode == 0 ? g0 : (gmode == 1 ? gt : (gmode == 2 ? 2.0 * gt : gt - g0));
	}
	__syncthreads();   /* the row is read back by the same workgroup */
	finish_track_body(bv, sm, ts, rows, 1, t);
}

/* ===================================================================== */
/* launchers                                                              */
/* ===================================================================== */

/* the unit's instantiations and the one of a launch: fused_select / fused_visit (mtfhip_fused_dispatch.h) */
void launch_fused_ssd(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk,
	hipStream_t st, const FusedMaps *maps, const SpssArgs *sp) {
	/* (the API enqueues pass 1 of RSCV / LRSCV in front and hands its maps over.  RSCV: no map, no launch; LRSCV without one -- a later
	 * pass of a frame under once_per_frame -- is an SSD pass on the raw patch, LRSCV.cc:234-235) */
	const bool mapped = bv.am == MTFHIP_AM_RSCV ? (maps && maps->rm.map) : (bv.am == MTFHIP_AM_LRSCV && maps && maps->lm.map);
	const FusedKey k = fused_select(FUSED_ROUTE_LOOP, bv.am, bv.C, bv.ssm, fa.mode, fa.chained, fa.materialize, fa.fast_math, mapped);
	if (!k.served) return;
	if (k.am == MTFHIP_AM_RSCV) { launch_fused_rscv(bv, im, fa, partials, nblk, maps->rm, st); return; }
	if (k.am == MTFHIP_AM_LRSCV) { launch_fused_lrscv(bv, im, fa, partials, nblk, maps->lm, st); return; }
	if (k.am == MTFHIP_AM_SPSS) {   /* (the API hands its constant and what the search method reads: a launch without them is an error) */
		if (sp) launch_fused_spss(bv, im, fa, partials, nblk, *sp, st);
		else note_launch_error(hipErrorInvalidValue, __FILE__, __LINE__);
		return;
	}
	if (k.mc) { launch_fused_mc(bv, im, fa, partials, nblk, st); return; }   /* MCSSD / MCNCC */
	const dim3 g = grid2(nblk, bv.B);
	const bool launched = fused_visit<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>(k, [&](auto AM, auto SSM, auto CH, auto MD, auto MAT, auto FAST) {
		if constexpr (FAST())
			MTFHIP_LAUNCH((k_fused_fast<AM(), SSM(), MD(), CH()>), g, dim3(kBlock), 0, st, bv, im, fa, partials, nblk);
		else if constexpr (AM() == MTFHIP_AM_NCC)
			MTFHIP_LAUNCH((k_fused_ncc<SSM(), CH(), MD(), MAT()>), g, dim3(kBlock), 0, st, bv, im, fa, partials, nblk);
		else {   /* (grid_regen: the lattice products, fused_lk_body) */
			const size_t tab = MAT() && fa.grid_regen ? sizeof(double2) * (size_t)(fa.g_resx + fa.g_resy) : 0;
			MTFHIP_LAUNCH((k_fused_ssd<SSM(), CH(), MD(), MAT()>), g, dim3(kBlock), tab, st, bv, im, fa, partials, nblk);
		}
	});
	if (!launched) note_launch_error(hipErrorInvalidDeviceFunction, __FILE__, __LINE__);   /* (no kernel for this launch: an error, not a skipped pass) */
}
void launch_finish_track(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts, const double *partials,
	int nblk, hipStream_t st, PhaseCtl pc, const HostPublish &pub, int pub_t0) {
	/* NCC rows are 72 wide: two waves load them, the first one solves; many block rows (a single large target): 240 lanes sum them */
	const dim3 block(nblk > 8 ? 256 : (bv.am == MTFHIP_AM_NCC ? 128 : 64));
	if (bv.am == MTFHIP_AM_SPSS) launch_finish_track_spss(bv, sm, ts, partials, nblk, st, pc, pub, pub_t0, block);   /* (kernels_fused_spss.hip) */
	else if (ts.lo_ssm) MTFHIP_LAUNCH(k_finish_track_lo, dim3(bv.B), block, 0, st, bv, sm, ts, partials, nblk, pc, pub, pub_t0);
	else MTFHIP_LAUNCH(k_finish_track, dim3(bv.B), block, 0, st, bv, sm, ts, partials, nblk, pc, pub, pub_t0);
}

void launch_finish_track_mi(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts, int sum_std, int gmode,
	const double *mi_H, const double *gpart, int ng, double *rows, hipStream_t st) {
	MTFHIP_LAUNCH(k_finish_track_mi, dim3(bv.B), dim3(64), 0, st, bv, sm, ts, sum_std, gmode, mi_H, gpart, ng, rows);
}

/* The single-target launches read the warp and the state out of the kernel-argument segment at an offset computed from the C++
 * layout of (BatchView, ImgView, FusedArgs) -- fused_lk_body's static_asserts check the structs, not what the runtime actually
 * puts into the segment.  This probe has the fused kernels' leading parameters, reads the seventeen doubles with the same
 * arithmetic and hands them back: the library asks once per process and keeps the warp upload in front of every launch if the
 * answer is not what it passed in. */
__global__ void k_kernarg_probe(BatchView bv, ImgView im, FusedArgs fa, double *out) {
	const char *kernarg = (const char *)__builtin_amdgcn_kernarg_segment_ptr();
	const double *kw = reinterpret_cast<const double *>(kernarg + sizeof(BatchView) + sizeof(ImgView) + offsetof(FusedArgs, iw));
	if (threadIdx.x < 17) out[threadIdx.x] = kw[threadIdx.x];
	if (threadIdx.x == 17) out[17] = (double)(bv.B + im.w + fa.mode);   /* (the arguments are live) */
}
bool kernarg_layout_verified(hipStream_t st) {
	static int state = -1;   /* -1 not asked, 0 no, 1 yes */
	if (state >= 0) return state == 1;
	state = 0;
	Dev<double> d_out;
	if (d_out.reserve(18) != hipSuccess) { (void)hipGetLastError(); return false; }
	BatchView bv{}; ImgView im{}; FusedArgs fa{};
	bv.B = 1; im.w = 2; fa.mode = 3; fa.inline_warp = 1;
	for (int q = 0; q < 9; ++q) fa.iw[q] = 0.5 + 1.25 * q;
	for (int q = 0; q < 8; ++q) fa.is[q] = -3.0 - 0.75 * q;
	double h[18] = {0};
	hipLaunchKernelGGL(k_kernarg_probe, dim3(1), dim3(64), 0, st, bv, im, fa, d_out.get());
	bool ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, st) == hipSuccess &&
		hipStreamSynchronize(st) == hipSuccess;
	for (int q = 0; ok && q < 9; ++q) ok = h[q] == fa.iw[q];
	for (int q = 0; ok && q < 8; ++q) ok = h[9 + q] == fa.is[q];
	state = ok ? 1 : 0;
	return ok;
}

#ifdef MTFHIP_FIN_TRACE
void debug_fin_trace(unsigned long long *out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fin_trace), sizeof(unsigned long long) * 16); }
#endif
} // namespace mtfhip
