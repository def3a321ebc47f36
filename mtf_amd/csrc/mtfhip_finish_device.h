/*
 * mtfhip_finish_device.h -- the device-side finish of an LK iteration (solve, compositional update, convergence test),
 * shared by the translation units that end an iteration with it (kernels_fused.hip: k_finish_track, k_finish_track_mi;
 * kernels_mi_fused.hip: k_mi_finish_fast).  No relocatable device code: the body is inlined into each kernel.
 */
#ifndef MTFHIP_FINISH_DEVICE_H
#define MTFHIP_FINISH_DEVICE_H
#include "mtfhip_device.h"

namespace mtfhip {

#ifdef MTFHIP_FIN_TRACE
__device__ unsigned long long g_fin_trace[16];
#define FIN_STAMP(k) do { if (t == 0 && threadIdx.x == 0) g_fin_trace[k] = clock64(); } while (0)
#else
#define FIN_STAMP(k) do { } while (0)
#endif

/* ---- what the two finish bodies share beside the system itself (mtfhip_sm_system.h) ---- */
/* COH (k_track_persist): everything the loop rewrites between passes -- partial rows, warp, state, corners, counters, flags, the
 * Levenberg-Marquardt block -- is read and written with the coherent accessors of mtfhip_device.h (st_coh / ld_coh). */
template <bool COH> __device__ __forceinline__ double fin_ld(const double *p) { if constexpr (COH) return ld_coh(p); else return *p; }
template <bool COH> __device__ __forceinline__ int fin_ld(const int *p) { if constexpr (COH) return ld_coh(p); else return *p; }
template <bool COH> __device__ __forceinline__ void fin_st(double *p, double v) { if constexpr (COH) st_coh(p, v); else *p = v; }
template <bool COH> __device__ __forceinline__ void fin_st(int *p, int v) { if constexpr (COH) st_coh(p, v); else *p = v; }

/* Fixed-order sum of the block rows of target t, column by column.  Up to eight rows (the batched decomposition) one lane per column sums
 * them in one round trip; a single large target has 157: the rows are cut into three contiguous runs (multiples of eight rows) summed by
 * three groups of 80 lanes and combined in run order -- 7 rounds instead of 20.  (Workgroups of fewer than 240 threads keep the single
 * run.)  Two steps, so that the caller's other loads and its test of `active` sit between the requests and their use: fin_sum_runs
 * returns the lane's column sum of a single run, or leaves the runs' sums in part_s; fin_sum_combine (a barrier for three runs) gives
 * lane < RL its column. */
__device__ __forceinline__ int fin_sum_n_runs(int nblk) { return (nblk > 8 && blockDim.x >= 240) ? 3 : 1; }
template <bool COH>
__device__ __forceinline__ double fin_sum_runs(const double *partials, int nblk, int RL, int t, double (*part_s)[80]) {
	const int lane = threadIdx.x;
	const int n_runs = fin_sum_n_runs(nblk);
	const int run_len = n_runs == 1 ? nblk : ((nblk + 3 * 8 - 1) / (3 * 8)) * 8;
	const int run = n_runs == 1 ? 0 : lane / 80, col = n_runs == 1 ? lane : lane % 80;
	double v_acc = 0;
	if (col < RL && run < n_runs) {
		const int b0 = run * run_len, b1 = (b0 + run_len < nblk) ? b0 + run_len : nblk;
		const double *p = partials + (size_t)t * nblk * RL + col;
		auto ld = [&](size_t off) -> double { return fin_ld<COH>(p + off); };
		/* eight block rows in flight per lane */
		double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, s7 = 0;
		int b = b0;
		for (; b + 7 < b1; b += 8) {
			s0 += ld((size_t)b * RL); s1 += ld((size_t)(b + 1) * RL);
			s2 += ld((size_t)(b + 2) * RL); s3 += ld((size_t)(b + 3) * RL);
			s4 += ld((size_t)(b + 4) * RL); s5 += ld((size_t)(b + 5) * RL);
			s6 += ld((size_t)(b + 6) * RL); s7 += ld((size_t)(b + 7) * RL);
		}
		for (; b < b1; ++b) s0 += ld((size_t)b * RL);
		const double v = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
		if (n_runs == 1) v_acc = v; else part_s[run][col] = v;
	}
	return v_acc;
}
__device__ __forceinline__ double fin_sum_combine(int nblk, int RL, double v_acc, const double (*part_s)[80]) {
	const int lane = threadIdx.x;
	if (fin_sum_n_runs(nblk) > 1) {
		__syncthreads();
		if (lane < RL) v_acc = (part_s[0][lane] + part_s[1][lane]) + part_s[2][lane];
	}
	return v_acc;
}

/* the target stops iterating; behind a pass that did not materialise (TrackState::lean_pass) the warp and the state the pass ran at
 * are kept for the trailing materialising launch */
template <bool COH, bool LO>
__device__ __forceinline__ void fin_stop_target(const TrackState &ts, int t, int *stop_flag, const double *w_old, const double *s_old) {
	fin_st<COH>(ts.active + t, 0);
	if (stop_flag) __hip_atomic_store(stop_flag, 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
	if (ts.lean_pass || (LO && ts.keep_last)) {
		for (int q = 0; q < 9; ++q) fin_st<COH>(ts.warp_last + 9 * t + q, w_old[q]);
		for (int q = 0; q < 8; ++q) fin_st<COH>(ts.state_last + 8 * t + q, s_old[q]);
		if (ts.lean_pass) fin_st<COH>(ts.need_mat + t, 1);
	}
}

/* Levenberg-Marquardt: the accept / undo decision on the similarity f of this pass (NT/ESM.cc:186-232, NT/FCLK.cc:205-250,
 * NT/ICLK.cc:181-199): a pure function of the block's words; returns undo and rescales delta */
__device__ __forceinline__ bool fin_lm_decide(double f, double prev_f, double &delta, bool state_reset, int iter_id, double update) {
	bool undo = false;
	if (!state_reset) {
		if (iter_id > 0) {
			if (f < prev_f) { delta *= update; undo = true; }
			else if (f > prev_f) delta /= update;
		}
	}
	return undo;
}
/* ... and what one lane writes back of it */
template <bool COH>
__device__ __forceinline__ void fin_lm_store(double *lmp, double f, double delta, bool state_reset, bool undo) {
	fin_st<COH>(lmp + 1, delta);
	if (undo) fin_st<COH>(lmp + 2, 1.0);
	else { fin_st<COH>(lmp + 2, 0.0); if (!state_reset) fin_st<COH>(lmp + 0, f); }
}

/* the close of a pass, one lane: count it, test convergence on the corner change, stop the target */
template <bool COH, bool ADDITIVE, bool LO>
__device__ __forceinline__ void fin_count_and_stop(const mtfhip_sm_desc &sm, const TrackState &ts, int t, int *stop_flag, double *lmp, double *trec,
	int n_it_prev, int lm_iter_id, bool undo, double change, const double *w_old, const double *s_old) {
	const int n_it = n_it_prev + 1;   /* passes done (the reference's iters_done) */
	fin_st<COH>(ts.n_iters + t, n_it);
	if (trec) trec[89] = (double)n_it_prev;
	if (lmp) {
		/* an undo pass skips the convergence test (`continue`); it consumes an iteration in the for loops of ESM and ICLK
		 * (NT/ESM.cc:179, NT/ICLK.cc:169) but not in FCLK's while loop (NT/FCLK.cc:193-223) */
		const int id = lm_iter_id + ((undo && sm.sm == MTFHIP_SM_FCLK && !ADDITIVE) ? 0 : 1);
		fin_st<COH>(lmp + 3, (double)id);
		if ((!undo && change < sm.epsilon) || id >= sm.max_iters) fin_stop_target<COH, LO>(ts, t, stop_flag, w_old, s_old);
	} else if (change < sm.epsilon || n_it >= sm.max_iters) fin_stop_target<COH, LO>(ts, t, stop_flag, w_old, s_old);
}

/* ===================================================================== */
/* on-device solve + compositional update (batched drivers only)          */
/* ===================================================================== */
/* One wave64 per target, one launch per LK iteration:
 *   (1) fixed-order sum of the per-workgroup partial rows (what k_finish does for the host-driven path),
 *   (2) g and H of the search method from the accumulators (NT/FCLK.cc:260-288, NT/ESM.cc:298-377 with
 *       SSDBase.cc:169-191,287-311, NT/ICLK.cc:206-251),
 *   (3) H dp = -g by Gauss-Jordan elimination spread over the 64 lanes (lane = matrix entry) on the
 *       symmetrically diagonal-scaled system; every SSD Hessian here is a negated Gram matrix, i.e.
 *       definite, so no pivoting is needed (the reference uses Eigen's colPivHouseholderQr, NT/FCLK.cc:298),
 *   (4) the (inverse) compositional update and the corner-change test on lane 0
 *       (Homography.cc:73-92,109-114, Affine.cc:90-106,145-150, NT/FCLK.cc:314-339). */
/* Body of the device-side finish, executed by the first wave of the calling workgroup (all threads of the workgroup
 * must call it: it contains workgroup barriers). */
/* COH (k_track_persist): the coherent accessors, fin_ld / fin_st above. */
/* ADDITIVE (k_alk_finish, kernels_alk.hip: nt::FALK / nt::IALK, NT/FALK.cc:229-246, NT/IALK.cc:180-194): the solved update is ADDED to the
 * state -- StateSpaceModel::additiveUpdate, ProjectiveBase.cc:51-55: curr_state += state_update, the warp rebuilt from the state
 * (getWarpFromState), the corners from the warp -- and a Levenberg-Marquardt undo adds its negative (NT/FALK.cc:156-158); the `continue`
 * behind an undo consumes an iteration of their for loops (NT/FALK.cc:141,166).  The caller hands in the search method as FCLK: g and H
 * are FCLK's functions of the reduced row (cmptCurrJacobian / cmptSelfHessian / cmptCurrHessian of the pass's own pixel Jacobian). */
/* stop_flag (k_finish_track's delivery to the host; LDS, cleared by the caller, or NULL): 1 once the target is known to have been active at entry,
 * 3 when this pass stops it -- written by lane 0 of the first wave, the wave that reads it afterwards */
/* LO (k_finish_track_lo, kernels_fused.hip): the finish of a low-order SSM's batch (TrackState::lo_ssm) -- the projection of the affine-coordinate
 * system and the model's own update.  A template parameter, not a run-time branch: the kernels of homography and affine batches are
 * compiled without any of it (the Isometry's cos / sin / atan2 alone would raise their register and scratch demand). */
/* SPSS (k_finish_track_spss, kernels_fused_spss.hip): the reduced row is an SPSS pass's (kernels_fused_spss.hip) -- ACC_RR = f itself (a sum of scores
 * that Levenberg-Marquardt maximises as it stands), ACC_H the WEIGHTED Gram matrix, i.e. the Hessian with its sign, ACC_G = sum df_dIt row
 * and ACC_G2 = sum df_dI0 J0 row, from which the search method's Jacobian is cmptCurrJacobian (FCLK; ESM jac_type Original, over the mean
 * row), cmptInitJacobian (ICLK) or half the difference (ESM DiffOfJacs, AppearanceModel.h:161-164, NT/ESM.cc:309).  ICLK's Std Hessian
 * is not constant (cmptInitHessian weights J0 J0^T by a function of It, SPSS.cc:160-165) and comes from the row; the curr / init weights
 * change sign, so every non-self system is solved with pivoting. */
/* SSIM (k_finish_track_ssim / _ssim_lo, kernels_ssim.hip): the reduced row is an NCC pass's -- the same 72 raw moments, the same template
 * moments -- read as SSIM reads them (ssim_sys / ssim_g / ssim_h, mtfhip_sm_system.h): beside mean(I0), slot 6 of the target's NCC scalars
 * holds sum (I0 - mean)^2 itself, and c1, c2 arrive as arguments of the kernel (no field of TrackState: the other kernels' argument
 * segments keep their layout).  cmptInitHessian / cmptCurrHessian are not symmetric: every entry is taken as (r, c), and the elimination
 * pivots as for NCC. */
template <bool COH = false, bool ADDITIVE = false, bool LO = false, bool SPSS = false, bool SSIM = false>
__device__ __forceinline__ void finish_track_body(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts,
	const double *partials, int nblk, int t, int *stop_flag = nullptr, double ssim_c1 = 0.0, double ssim_c2 = 0.0) {
	auto LD = [](const double *p) -> double { return fin_ld<COH>(p); };
	auto LDI = [](const int *p) -> int { return fin_ld<COH>(p); };
	auto ST = [](double *p, double v) { fin_st<COH>(p, v); };
	FIN_STAMP(0);
	__shared__ double acc_s[NCC_ACC_COUNT];   /* >= ACC_COUNT */
	__shared__ double A[8][9];
	__shared__ double dps[8];
	__shared__ double h0s[64], Ws[9], crs[8], ics[12], tms[NCC_TM_COUNT], ncs[SSIM ? 8 : 2], sos[8];
	const int lane = threadIdx.x;
	const bool wv0 = lane < 64;
	const int S = bv.S;
	/* a low-order SSM (LO; TrackState::lo_ssm, uniform over the launch): S is the affine pass's row width 6 and everything up to h_entry /
	 * g_entry is the affine finish; the system that is damped, equilibrated and eliminated is the SS x SS projection of it */
	const int lo = LO ? ts.lo_ssm : 0;
	const int SS = lo ? ts.SS : S;
	/* NCC: the reduced row holds raw moments (NCC_* slots, NCC_ACC_COUNT wide); tms = sum J0 | sum I0 J0 | Gram(J0) of the
	 * template, ncs = mean(I0), |I0 - mean|.  The calling workgroup then has at least 128 threads. */
	const bool ncc = SSIM || bv.am == MTFHIP_AM_NCC;   /* (an SSIM batch's rows are NCC's) */
	constexpr int NCS = SSIM ? 7 : 2;
	const int RL = ncc ? (int)NCC_ACC_COUNT : (int)ACC_COUNT;
	/* every global operand of this target -- the `active` flag included -- is requested up front, in parallel across
	 * the lanes, and only then is the flag tested: one memory round trip instead of two (flag, then operands); the
	 * rest of the routine runs out of LDS / registers */
	const int act = LDI(ts.active + t);
	const int n_it_prev = LDI(ts.n_iters + t);   /* passes done so far (uniform: a scalar load) */
	double v_h0 = 0, v_w = 0, v_cr = 0, v_ic = 0, v_acc = 0, v_tm = 0, v_nc = 0, v_so = 0;
	if (wv0) {
		v_h0 = ts.h0[(size_t)t * 64 + lane];
		if (lane < 9) v_w = LD(bv.warps + 9 * t + lane);
		if ((ADDITIVE || ts.lean_pass || (LO && ts.keep_last)) && lane < 8) v_so = LD(bv.states + 8 * t + lane);   /* (the state this pass ran at: stop_target, the additive update) */
		if (lane < 8) v_cr = LD(ts.corners + 8 * t + lane);
		if (lane < 12) v_ic = ts.init_corners_hm[12 * t + lane];
		if (ncc) {
			if (lane < NCC_TM_COUNT) v_tm = ts.ncc_tm[(size_t)t * NCC_TM_COUNT + lane];
			if (lane < NCS) v_nc = ts.ncc[(size_t)t * 8 + lane];
		}
	}
	__shared__ double part_s[3][80];
	v_acc = fin_sum_runs<COH>(partials, nblk, RL, t, part_s);
	if (!act) return;
	if (stop_flag && lane == 0) __hip_atomic_store(stop_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
	FIN_STAMP(1);
	if (wv0) {
		h0s[lane] = v_h0;
		if (lane < 9) Ws[lane] = v_w;
		if (lane < 8) { crs[lane] = v_cr; sos[lane] = v_so; }
		if (lane < 12) ics[lane] = v_ic;
		if (lane < NCC_TM_COUNT) tms[lane] = v_tm;
		if (lane < NCS) ncs[lane] = v_nc;
	}
	v_acc = fin_sum_combine(nblk, RL, v_acc, part_s);
	if (lane < RL) { acc_s[lane] = v_acc; ST(ts.acc + (size_t)t * RL + lane, v_acc); }
	__syncthreads();
	FIN_STAMP(2);
	const int i = (lane >> 3) & 7, j = lane & 7;
	/* the system of this pass: mtfhip_sm_system.h.  NCC's scalars once, from the reduced row and the template's constants */
	NccSys nq = NccSys();
	SsimSys sq = SsimSys();
	if constexpr (SSIM) sq = ssim_sys(acc_s, tms, ncs[0], ncs[6], (double)bv.N, ssim_c1, ssim_c2);
	else if (ncc) nq = ncc_sys(acc_s, tms, ncs[0], ncs[1], (double)bv.N);
	const double f_row = SSIM ? sq.f : (ncc ? nq.f : ssd_f(SPSS, acc_s));
	/* ---- Levenberg-Marquardt: the accept / undo test on the similarity of this pass (uniform over the workgroup) ---- */
	double *lmp = ts.lm ? ts.lm + (size_t)t * kLmStride : nullptr;
	double lm_delta = 0.0;
	int lm_iter_id = n_it_prev;   /* (LM keeps its own counter) */
	bool undo = false;
	if (lmp) {
		const double f_use = ts.f_ext ? LD(ts.f_ext + t) : f_row;   /* (MI's similarity is not a function of the row) */
		const double prev_f = LD(lmp + 0);
		lm_delta = LD(lmp + 1);
		const bool state_reset = LD(lmp + 2) != 0.0;
		lm_iter_id = (int)LD(lmp + 3);
		undo = fin_lm_decide(f_use, prev_f, lm_delta, state_reset, lm_iter_id, sm.lm_delta_update);
		__syncthreads();   /* every thread has read the LM block before lane 0 rewrites it */
		if (lane == 0) fin_lm_store<COH>(lmp, f_use, lm_delta, state_reset, undo);
	}
	/* entry (r, c) of H and entry s of g as the search method holds them, padded to 8 x 8: thin adapters over mtfhip_sm_system.h */
	auto h_entry = [&](int r, int c) -> double {
		if (r >= S || c >= S) return r == c ? -1.0 : 0.0;
		if constexpr (SSIM) return ssim_h(sm, sq, h0s[c * S + r], r, c);
		/* sec_ord_hess: + sum_p df_dI[p] d2I_dp2[:, p] (SSDBase.cc:313-415; NCC.cc:391-410); the homography blocks are not symmetric in their
		 * last two rows / columns (Homography.cc:421,613,796), so the entry is taken as (r, c), not from a triangle */
		if (ncc) return ncc_h(sm, nq, h0s[(r < c ? c : r) * S + (r < c ? r : c)], ts.h_extra ? ts.h_extra_scale * ts.h_extra[(size_t)t * S * S + c * S + r] : 0.0, r, c);
		double v = ssd_h(sm, ts.h_from_acc != 0, SPSS, acc_s, h0s, S, r, c);
		if (ts.h_extra) v += ts.h_extra_scale * ts.h_extra[(size_t)t * S * S + c * S + r];
		return v;
	};
	auto g_entry = [&](int s) -> double {
		if constexpr (SSIM) return ssim_g(sm, sq, s);
		return (!SPSS && ncc) ? ncc_g(sm, nq, s) : ssd_g(sm, SPSS, acc_s, s);
	};
	/* Symmetric diagonal equilibration by POWERS OF TWO: the products are exact, so the scaled elimination follows the unscaled
	 * one bit for bit while its pivots stay near one (and a frexp / ldexp pair replaces the square root and the division of
	 * 1 / sqrt|d|, a microsecond of dependent arithmetic on an idle workgroup). */
	auto pow2_scale = [](double d) -> double { return d != 0 ? ldexp(1.0, -(ilogb(fabs(d)) / 2)) : 1.0; };
	/* Gauss-Jordan; with partial pivoting where the system can be indefinite: the SSD Hessians are negated Gram matrices (definite;
	 * a flat template's zero pivot leaves its unknown at zero), but NCC's Std / SumOfStd and MI's Hessians can be indefinite away
	 * from convergence, where the reference's colPivHouseholderQr (NT/FCLK.cc:298) does not care either.  (A row-per-lane
	 * elimination in registers with v_readlane broadcasts was measured slower than this LDS form: 8.9 k against 6.9 k clocks.) */
	const bool pivoting = SPSS || ncc || ts.h_from_acc || ts.h_extra != nullptr;   /* (the search and the row swap are two barriers and eight LDS reads per step: skipped for SSD) */
	/* The low-order SSMs: the SS x SS projection of the affine system (lowdof_h / lowdof_g, mtfhip_sm_system.h), taken here: behind h_entry /
	 * g_entry, in front of the damping, the equilibration and the elimination; rows and columns >= SS are padded as above */
	auto lo_h = [&](int r, int c) -> double { return (r >= SS || c >= SS) ? (r == c ? -1.0 : 0.0) : lowdof_h(lo, r, c, h_entry); };
	auto lo_g = [&](int s) -> double { return lowdof_g(lo, s, g_entry); };
	double hii, hjj, hij = 0.0, gi = 0.0;
	if (lo) {
		hii = lo_h(i, i); hjj = lo_h(j, j);
		if (wv0) { hij = lo_h(i, j); gi = (j == 0 && i < SS) ? lo_g(i) : 0.0; }
	} else {
		hii = h_entry(i, i); hjj = h_entry(j, j);
		if (wv0) { hij = h_entry(i, j); gi = (j == 0 && i < S) ? g_entry(i) : 0.0; }
	}
	const double si = pow2_scale(hii), sj = pow2_scale(hjj);
	double *trec = (ts.trace && n_it_prev < ts.trace_cap) ? ts.trace + ((size_t)t * ts.trace_cap + n_it_prev) * kTraceStride : nullptr;   /* debug trace */
	if (wv0) {
		/* hessian(i, i) += leven_marq_delta * hessian(i, i) (NT/ESM.cc:262-265) */
		A[i][j] = hij * si * sj * ((lmp && i == j && i < SS) ? 1.0 + lm_delta : 1.0);
		if (j == 0) A[i][8] = gi * si;
		if (trec) {
			trec[8 * i + j] = (i < SS && j < SS) ? hij : 0.0;
			if (j == 0) trec[64 + i] = gi;
			if (lane == 0) {
				trec[88] = ts.f_ext ? LD(ts.f_ext + t) : f_row;
				trec[90] = undo ? 1.0 : 0.0; trec[91] = lm_delta; trec[92] = 1.0;
			}
		}
	}
	__syncthreads();
	FIN_STAMP(3);
#pragma unroll
	for (int k = 0; k < 8; ++k) {
		if (pivoting) {
			int pr = k;
			double best = fabs(A[k][k]);
#pragma unroll
			for (int r = k + 1; r < 8; ++r) { const double v = fabs(A[r][k]); if (v > best) { best = v; pr = r; } }
			const int src = i == k ? pr : (i == pr ? k : i);   /* row i after the swap of rows k and pr */
			const double mine = A[src][j], rhs = A[src][8];
			__syncthreads();
			if (wv0) { A[i][j] = mine; if (j == 0) A[i][8] = rhs; }
			__syncthreads();
		}
		const double piv = A[k][k], aik = A[i][k], akj = A[k][j], bk = A[k][8];
		const double f = (i != k && piv != 0) ? aik / piv : 0.0;
		__syncthreads();
		if (wv0 && i != k) {
			A[i][j] -= f * akj;
			if (j == 0) A[i][8] -= f * bk;
		}
		__syncthreads();
	}
	if (wv0 && j == 0) {
		const double d = A[i][i];
		dps[i] = (i < SS && d != 0) ? -(A[i][8] / d) * si : 0.0;
	}
	__syncthreads();
	FIN_STAMP(4);
	/* ---- compositional update and corner test.  The expressions (and their order) are those of the straightforward serial form;
	 * what is independent is spread over the lanes -- the 9 + 9 + 8 IEEE divisions of invertState, of the homography
	 * normalisation and of the corner dehomogenisation were ~35 dependent division latencies on one lane of an otherwise
	 * idle workgroup, now four. ---- */
	__shared__ double xs[9], nxy[8];
	const bool hom = bv.ssm == MTFHIP_SSM_HOMOGRAPHY;
	if (lane < 8) {
		const double v = undo ? LD(lmp + 4 + lane) : dps[lane];   /* undo: the previous state_update is taken back */
		if (lmp && !undo) ST(lmp + 4 + lane, v);
		dps[lane] = v;
		if (trec) trec[72 + lane] = v;
	}
	__syncthreads();
	double dp[8];
#pragma unroll
	for (int s = 0; s < 8; ++s) dp[s] = dps[s];
	double Wn[9];
	double *Wp = bv.warps + 9 * t, *st = bv.states + 8 * t;
	if constexpr (ADDITIVE) {
		/* curr_state += state_update (undo: its negative), then setState: getWarpFromState (Homography.cc:94-107, Affine.cc:116-130) */
		double sn[8];
#pragma unroll
		for (int s = 0; s < 8; ++s) sn[s] = sos[s] + (undo ? -dp[s] : dp[s]);
		if (hom) {
			Wn[0] = 1 + sn[0]; Wn[1] = sn[1]; Wn[2] = sn[2]; Wn[3] = sn[3]; Wn[4] = 1 + sn[4]; Wn[5] = sn[5];
			Wn[6] = sn[6]; Wn[7] = sn[7]; Wn[8] = 1;
		} else {
			Wn[0] = 1 + sn[2]; Wn[1] = sn[3]; Wn[2] = sn[0]; Wn[3] = sn[4]; Wn[4] = 1 + sn[5]; Wn[5] = sn[1];
			Wn[6] = 0; Wn[7] = 0; Wn[8] = 1;
		}
		double sq = 0;
#pragma unroll
		for (int q = 0; q < 8; ++q) if (lane == q) sq = sn[q];
		if (lane < S) ST(st + lane, sq);
	} else {
	double U[9];
	if (hom) {
		U[0] = 1 + dp[0]; U[1] = dp[1]; U[2] = dp[2]; U[3] = dp[3]; U[4] = 1 + dp[4]; U[5] = dp[5];
		U[6] = dp[6]; U[7] = dp[7]; U[8] = 1;
	} else if (lo) {
		/* getWarpFromState of the model: Translation.cc:86-93, Similitude.cc:123-141, Isometry.cc:68-86 */
		double u00 = 1.0, u10 = 0.0;
		if (lo == MTFHIP_SSM_SIMILITUDE) { u00 = 1 + dp[2]; u10 = dp[3]; }
		else if (lo == MTFHIP_SSM_ISOMETRY) { u00 = cos(dp[2]); u10 = sin(dp[2]); }
		U[0] = u00; U[1] = -u10; U[2] = dp[0]; U[3] = u10; U[4] = u00; U[5] = dp[1];
		U[6] = 0; U[7] = 0; U[8] = 1;
	} else {
		U[0] = 1 + dp[2]; U[1] = dp[3]; U[2] = dp[0]; U[3] = dp[4]; U[4] = 1 + dp[5]; U[5] = dp[1];
		U[6] = 0; U[7] = 0; U[8] = 1;
	}
	/* forward step: ICLK applies the inverse of the solved update (NT/ICLK.cc:266-267); undo: ESM / FCLK apply the inverse of
	 * the previous update (NT/ESM.cc:194-195), ICLK re-applies it (NT/ICLK.cc:188) */
	if (lo == MTFHIP_SSM_TRANSLATION) {
		/* Translation::invertState negates (Translation.cc:103-105); its compositionalUpdate adds (:75-84), which W * U below does */
		if ((sm.sm == MTFHIP_SM_ICLK) != undo) { U[2] = -dp[0]; U[5] = -dp[1]; }
	} else
	if ((sm.sm == MTFHIP_SM_ICLK) != undo) {
		/* invertState: inverse through cofactors, normalised by (2,2) */
		double c[9];
		c[0] = U[4] * U[8] - U[5] * U[7]; c[1] = U[2] * U[7] - U[1] * U[8]; c[2] = U[1] * U[5] - U[2] * U[4];
		c[3] = U[5] * U[6] - U[3] * U[8]; c[4] = U[0] * U[8] - U[2] * U[6]; c[5] = U[2] * U[3] - U[0] * U[5];
		c[6] = U[3] * U[7] - U[4] * U[6]; c[7] = U[1] * U[6] - U[0] * U[7]; c[8] = U[0] * U[4] - U[1] * U[3];
		double det = U[0] * c[0] + U[1] * c[3] + U[2] * c[6];
		double inv_det = 1.0 / det;
#pragma unroll
		for (int q = 0; q < 9; ++q) c[q] *= inv_det;
		double n22 = c[8];
		double cq = 0;
#pragma unroll
		for (int q = 0; q < 9; ++q) if (lane == q) cq = c[q];
		if (lane < 9) xs[lane] = cq / n22;
		__syncthreads();
#pragma unroll
		for (int q = 0; q < 9; ++q) U[q] = xs[q];
		__syncthreads();   /* xs is reused below */
		/* round-trip through the state parameterisation as getStateFromWarp / getWarpFromState do */
		U[0] = 1 + (U[0] - 1); U[4] = 1 + (U[4] - 1); U[8] = 1;
		if (!hom) { U[6] = 0; U[7] = 0; }
		if (lo) {
			/* ... which for Similitude reads (0, 0) - 1 and (1, 0) (Similitude.cc:144-153) and for Isometry atan2((1, 0), (0, 0))
			 * (Isometry.cc:88-97); the matrix is rebuilt from those alone */
			double u00 = U[0], u10 = U[3];
			if (lo == MTFHIP_SSM_ISOMETRY) { const double theta = atan2(U[3], U[0]); u00 = cos(theta); u10 = sin(theta); }
			U[0] = u00; U[1] = -u10; U[3] = u10; U[4] = u00;
		}
	}
	double Wo[9];
#pragma unroll
	for (int q = 0; q < 9; ++q) Wo[q] = Ws[q];
#pragma unroll
	for (int r = 0; r < 3; ++r)
#pragma unroll
		for (int c2 = 0; c2 < 3; ++c2)
			Wn[3 * r + c2] = Wo[3 * r] * U[c2] + Wo[3 * r + 1] * U[3 + c2] + Wo[3 * r + 2] * U[6 + c2];
	if (hom) {
		double n22 = Wn[8];
		double wq = 0;
#pragma unroll
		for (int q = 0; q < 9; ++q) if (lane == q) wq = Wn[q];
		if (lane < 9) xs[lane] = wq / n22;
		__syncthreads();
#pragma unroll
		for (int q = 0; q < 9; ++q) Wn[q] = xs[q];
		if (lane == 0) {
			ST(st + 0, Wn[0] - 1); ST(st + 1, Wn[1]); ST(st + 2, Wn[2]); ST(st + 3, Wn[3]); ST(st + 4, Wn[4] - 1); ST(st + 5, Wn[5]);
			ST(st + 6, Wn[6]); ST(st + 7, Wn[7]);
		}
	} else if (lane == 0) {
		ST(st + 0, Wn[2]); ST(st + 1, Wn[5]); ST(st + 2, Wn[0] - 1); ST(st + 3, Wn[1]); ST(st + 4, Wn[3]); ST(st + 5, Wn[4] - 1);
	}
	}   /* (!ADDITIVE) */
	{
		double wq = 0;
#pragma unroll
		for (int q = 0; q < 9; ++q) if (lane == q) wq = Wn[q];
		if (lane < 9) ST(Wp + lane, wq);
	}
	double *cr = ts.corners + 8 * t;
	if (lane < 4) {
		const int q = lane;
		double X = ics[3 * q], Y = ics[3 * q + 1], Z = ics[3 * q + 2];
		double nx = Wn[0] * X + Wn[1] * Y + Wn[2] * Z, ny = Wn[3] * X + Wn[4] * Y + Wn[5] * Z;
		if (hom) {
			double d = Wn[6] * X + Wn[7] * Y + Wn[8] * Z;
			nx = nx / d; ny = ny / d;
		}
		nxy[2 * q] = nx; nxy[2 * q + 1] = ny;
		ST(cr + 2 * q, nx); ST(cr + 2 * q + 1, ny);
		if (trec) { trec[80 + 2 * q] = nx; trec[81 + 2 * q] = ny; }
	}
	__syncthreads();
	FIN_STAMP(5);
	if (lane != 0) return;
	double change = 0;
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		double ddx = crs[2 * q] - nxy[2 * q], ddy = crs[2 * q + 1] - nxy[2 * q + 1];
		change += ddx * ddx + ddy * ddy;
	}
	fin_count_and_stop<COH, ADDITIVE, LO>(sm, ts, t, stop_flag, lmp, trec, n_it_prev, lm_iter_id, undo, change, Ws, sos);
	FIN_STAMP(6);
}


/* ---------------------------------------------------------------------------------------------------------------------
 * Tolerance-mode finish (TrackState::fast_finish: MTFHIP_MATH_FAST, SSD family, first-order Hessian, no pivoting needed).
 * finish_track_body keeps the reference's expressions and IEEE divisions and eliminates in LDS with two barriers per pivot --
 * ~3.7 us of dependent latency behind the row sums on a workgroup that has nothing else to do.  Here every lane of wave 0 holds
 * the whole 8 x 8 system in registers and solves it redundantly: LDL^T without pivoting (the SSD Hessians are negated Gram
 * matrices; a zero pivot leaves its unknown at zero, as there), reciprocals by v_rcp_f64 + two Newton steps, the inverse of
 * the update through cofactors with the determinant cancelled, no equilibration (scaling by powers of two changes nothing
 * without pivoting).  No LDS and no barrier between the reduced row and the stores.  Same g, H, Levenberg-Marquardt logic,
 * update and convergence test as finish_track_body; results agree with it to rounding (~1e-13 relative on dp).
 * --------------------------------------------------------------------------------------------------------------------- */
template <bool COH = false>
__device__ __forceinline__ void finish_track_fast_body(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts,
	const double *partials, int nblk, int t, int *stop_flag = nullptr) {
	auto LD = [](const double *p) -> double { return fin_ld<COH>(p); };
	auto LDI = [](const int *p) -> int { return fin_ld<COH>(p); };
	auto ST = [](double *p, double v) { fin_st<COH>(p, v); };
	__shared__ double f_acc[ACC_COUNT], f_h0[64], f_w[9], f_cr[8], f_ic[12], f_lm[kLmStride + 1], f_part[3][80], f_so[8];
	const int lane = threadIdx.x;
	const bool wv0 = lane < 64;
	const int S = bv.S;
	constexpr int RL = ACC_COUNT;
	const int act = LDI(ts.active + t);
	FIN_STAMP(0);
	const int n_it_prev = LDI(ts.n_iters + t);
	double *lmp = ts.lm ? ts.lm + (size_t)t * kLmStride : nullptr;
	double v_h0 = 0, v_w = 0, v_cr = 0, v_ic = 0, v_acc = 0, v_lm = 0, v_f = 0, v_so = 0;
	if (wv0) {
		if (ts.lean_pass && lane < 8) v_so = LD(bv.states + 8 * t + lane);   /* (the state this pass ran at: stop_target) */
		/* (the Levenberg-Marquardt block and an external similarity ride on the same round trip) */
		if (lmp && lane < kLmStride) v_lm = LD(lmp + lane);
		if (ts.f_ext && lane == 0) v_f = LD(ts.f_ext + t);
		v_h0 = ts.h0[(size_t)t * 64 + lane];
		if (lane < 9) v_w = LD(bv.warps + 9 * t + lane);
		if (lane < 8) v_cr = LD(ts.corners + 8 * t + lane);
		if (lane < 12) v_ic = ts.init_corners_hm[12 * t + lane];
	}
	v_acc = fin_sum_runs<COH>(partials, nblk, RL, t, f_part);
	if (!act) return;
	if (stop_flag && lane == 0) __hip_atomic_store(stop_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
	FIN_STAMP(1);
	if (wv0) {
		f_h0[lane] = v_h0;
		if (lane < 9) f_w[lane] = v_w;
		if (lane < 8) { f_cr[lane] = v_cr; f_so[lane] = v_so; }
		if (lane < 12) f_ic[lane] = v_ic;
		if (lane < kLmStride) f_lm[lane] = v_lm;
		if (lane == 0) f_lm[kLmStride] = v_f;
	}
	v_acc = fin_sum_combine(nblk, RL, v_acc, f_part);
	if (lane < RL) { f_acc[lane] = v_acc; ST(ts.acc + (size_t)t * RL + lane, v_acc); }
	__syncthreads();
	if (!wv0) return;   /* the rest is wave 0's, without barriers */
	FIN_STAMP(2);
	/* ---- Levenberg-Marquardt accept / undo (NT/ESM.cc:186-232, NT/FCLK.cc:205-250, NT/ICLK.cc:181-199) ---- */
	double lm_delta = 0.0;
	int lm_iter_id = n_it_prev;
	bool undo = false;
	const double f_now = ts.f_ext ? f_lm[kLmStride] : ssd_f(false, f_acc);
	if (lmp) {
		const double prev_f = f_lm[0];
		lm_delta = f_lm[1];
		const bool state_reset = f_lm[2] != 0.0;
		lm_iter_id = (int)f_lm[3];
		undo = fin_lm_decide(f_now, prev_f, lm_delta, state_reset, lm_iter_id, sm.lm_delta_update);
		if (lane == 0) fin_lm_store<COH>(lmp, f_now, lm_delta, state_reset, undo);
	}
	/* (the SSD family's selection, mtfhip_sm_system.h: this body never serves SPSS rows, nor MI's -- h_from_acc is false by construction) */
	/* ---- the system, lower triangle, in the registers of every lane ---- */
	/* (every LDS operand is requested unconditionally and up front -- one wait; guarded reads were 36 round trips) */
	double aH[36], aG[8], hI[36];
#pragma unroll
	for (int k = 0; k < 36; ++k) aH[k] = f_acc[ACC_H + k];
#pragma unroll
	for (int k = 0; k < 8; ++k) aG[k] = f_acc[ACC_G + k];
#pragma unroll
	for (int r = 0; r < 8; ++r)
#pragma unroll
		for (int c = 0; c <= r; ++c) hI[r * (r + 1) / 2 + c] = f_h0[(r * S + c) & 63];
	double M[8][8], y[8];
#pragma unroll
	for (int r = 0; r < 8; ++r) {
#pragma unroll
		for (int c = 0; c <= r; ++c) {
			const double v = ssd_h_of(sm_use_h0(sm, false, false), sm_sum_h0(sm, false, false), false, aH[tri8(c, r)], hI[r * (r + 1) / 2 + c]);
			M[r][c] = r < S ? v : (r == c ? -1.0 : 0.0);   /* (c <= r) */
		}
		y[r] = r < S ? ssd_g_of(sm, false, aG[r], 0.0) : 0.0;
	}
	FIN_STAMP(3);
	double *trec = (ts.trace && n_it_prev < ts.trace_cap) ? ts.trace + ((size_t)t * ts.trace_cap + n_it_prev) * kTraceStride : nullptr;   /* debug trace */
	if (trec && lane == 0) {
#pragma unroll
		for (int r = 0; r < 8; ++r) {
#pragma unroll
			for (int c = 0; c < 8; ++c) trec[8 * r + c] = (r < S && c < S) ? (c <= r ? M[r][c] : M[c][r]) : 0.0;
			trec[64 + r] = y[r];
		}
		trec[88] = f_now; trec[90] = undo ? 1.0 : 0.0; trec[91] = lm_delta; trec[92] = 1.0;
	}
	double dp[8];
	if (!undo) {
		if (lmp) {   /* hessian(i, i) += leven_marq_delta * hessian(i, i) (NT/ESM.cc:262-265) */
#pragma unroll
			for (int r = 0; r < 8; ++r) if (r < S) M[r][r] *= 1.0 + lm_delta;
		}
		/* L D L^T in place (L below the diagonal, D on it), then L z = g, D w = z, L^T x = w; dp = -x */
		double inv[8];
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			const double d = M[k][k];
			inv[k] = d != 0 ? rcp_fast(d) : 0.0;
			double l[8];
#pragma unroll
			for (int i = k + 1; i < 8; ++i) l[i] = M[i][k] * inv[k];
#pragma unroll
			for (int i = k + 1; i < 8; ++i) {
#pragma unroll
				for (int j = k + 1; j <= i; ++j) M[i][j] = fma(-l[i], M[j][k], M[i][j]);
			}
#pragma unroll
			for (int i = k + 1; i < 8; ++i) { M[i][k] = l[i]; y[i] = fma(-l[i], y[k], y[i]); }
		}
#pragma unroll
		for (int k = 7; k >= 0; --k) {
			double x = y[k] * inv[k];
#pragma unroll
			for (int i = k + 1; i < 8; ++i) x = fma(-M[i][k], dp[i], x);
			dp[k] = x;
		}
#pragma unroll
		for (int k = 0; k < 8; ++k) dp[k] = k < S ? -dp[k] : 0.0;
		if (lmp) {
#pragma unroll
			for (int q = 0; q < 8; ++q) if (lane == q) ST(lmp + 4 + q, dp[q]);
		}
	} else {
		/* undo: the previous state_update is taken back */
#pragma unroll
		for (int q = 0; q < 8; ++q) dp[q] = f_lm[4 + q];
	}
	FIN_STAMP(4);
	/* ---- compositional update (Homography.cc:73-92,109-114, Affine.cc:90-106,145-150) and the corner test ---- */
	const bool hom = bv.ssm == MTFHIP_SSM_HOMOGRAPHY;
	double U[9];
	if (hom) {
		U[0] = 1 + dp[0]; U[1] = dp[1]; U[2] = dp[2]; U[3] = dp[3]; U[4] = 1 + dp[4]; U[5] = dp[5]; U[6] = dp[6]; U[7] = dp[7]; U[8] = 1;
	} else {
		U[0] = 1 + dp[2]; U[1] = dp[3]; U[2] = dp[0]; U[3] = dp[4]; U[4] = 1 + dp[5]; U[5] = dp[1]; U[6] = 0; U[7] = 0; U[8] = 1;
	}
	/* ICLK applies the inverse of the solved update (NT/ICLK.cc:266-267); undo: ESM / FCLK apply the inverse of the previous
	 * update (NT/ESM.cc:194-195), ICLK re-applies it (NT/ICLK.cc:188) */
	if ((sm.sm == MTFHIP_SM_ICLK) != undo) {
		double c[9];   /* cofactors; normalised by the (2, 2) entry: the determinant cancels */
		c[0] = U[4] * U[8] - U[5] * U[7]; c[1] = U[2] * U[7] - U[1] * U[8]; c[2] = U[1] * U[5] - U[2] * U[4];
		c[3] = U[5] * U[6] - U[3] * U[8]; c[4] = U[0] * U[8] - U[2] * U[6]; c[5] = U[2] * U[3] - U[0] * U[5];
		c[6] = U[3] * U[7] - U[4] * U[6]; c[7] = U[1] * U[6] - U[0] * U[7]; c[8] = U[0] * U[4] - U[1] * U[3];
		const double ic8 = rcp_fast(c[8]);
#pragma unroll
		for (int q = 0; q < 8; ++q) U[q] = c[q] * ic8;
		U[8] = 1;
		if (!hom) { U[6] = 0; U[7] = 0; }
	}
	double Wn[9];
#pragma unroll
	for (int r = 0; r < 3; ++r) {
		const double w0 = f_w[3 * r], w1 = f_w[3 * r + 1], w2 = f_w[3 * r + 2];
#pragma unroll
		for (int c2 = 0; c2 < 3; ++c2) Wn[3 * r + c2] = fma(w0, U[c2], fma(w1, U[3 + c2], w2 * U[6 + c2]));
	}
	if (hom) {
		const double in22 = rcp_fast(Wn[8]);
#pragma unroll
		for (int q = 0; q < 8; ++q) Wn[q] *= in22;
		Wn[8] = 1;
	}
	double St[8];
	if (hom) { St[0] = Wn[0] - 1; St[1] = Wn[1]; St[2] = Wn[2]; St[3] = Wn[3]; St[4] = Wn[4] - 1; St[5] = Wn[5]; St[6] = Wn[6]; St[7] = Wn[7]; }
	else { St[0] = Wn[2]; St[1] = Wn[5]; St[2] = Wn[0] - 1; St[3] = Wn[1]; St[4] = Wn[3]; St[5] = Wn[4] - 1; St[6] = 0; St[7] = 0; }
	double Cr[8], change = 0;
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		const double X = f_ic[3 * q], Y = f_ic[3 * q + 1], Z = f_ic[3 * q + 2];
		double nx = fma(Wn[0], X, fma(Wn[1], Y, Wn[2] * Z)), ny = fma(Wn[3], X, fma(Wn[4], Y, Wn[5] * Z));
		if (hom) { const double idn = rcp_fast(fma(Wn[6], X, fma(Wn[7], Y, Wn[8] * Z))); nx *= idn; ny *= idn; }
		const double ddx = f_cr[2 * q] - nx, ddy = f_cr[2 * q + 1] - ny;
		change += ddx * ddx + ddy * ddy;
		Cr[2 * q] = nx; Cr[2 * q + 1] = ny;
	}
	FIN_STAMP(5);
	/* (every lane holds the same numbers: lane q stores entry q) */
	double wq = 0, sq = 0, cq = 0;
#pragma unroll
	for (int q = 0; q < 9; ++q) if (lane == q) wq = Wn[q];
#pragma unroll
	for (int q = 0; q < 8; ++q) if (lane == q) { sq = St[q]; cq = Cr[q]; }
	if (lane < 9) ST(bv.warps + 9 * t + lane, wq);
	if (lane < S) ST(bv.states + 8 * t + lane, sq);
	if (lane < 8) ST(ts.corners + 8 * t + lane, cq);
	if (lane != 0) return;
	if (trec) {
#pragma unroll
		for (int q = 0; q < 8; ++q) { trec[72 + q] = dp[q]; trec[80 + q] = Cr[q]; }
	}
	fin_count_and_stop<COH, false, false>(sm, ts, t, stop_flag, lmp, trec, n_it_prev, lm_iter_id, undo, change, f_w, f_so);
	FIN_STAMP(6);
}

} // namespace mtfhip
#endif
