/*
 * api_mi_iter.hip -- the fused MI iteration: its materialising and recompute forms, one iteration for a host-side solve (mi_iterate) and the MI driver
 * of the device-side loop (track_loop_mi, behind track_core in api_track.hip)
 * (C-ABI implementation, include/mtfhip.h; shared declarations: mtfhip_api_internal.h; no CPU fallback: HIP kernels or an error)
 */
#include "mtfhip_api_internal.h"

extern "C" {

/* One ESM / FCLK / ICLK iteration with MI in four pixel-level launches instead of seventeen:
 *   0. the fused LK kernel (SSD instantiation, FCLK-type, materialising): warp -> It, dIt_dx, Jt in one pass (its SSD
 *      sums are ignored; MI's pixel scaling travels in norm_mult / norm_add).  ICLK: It only.
 *   1. k_mi_hist<MFMA, SELF>: histogram of It, joint (It, I0) and -- for the self Hessians -- joint (It, It), one pass;
 *      k_mi_tables_iter: pre-seeding, logs, similarity and the three gradient-factor tables in one launch
 *      (MI.cc:346-382, 399-403, 427-431, 651-658).
 *   2. k_mi_grad_gemv: both gradient vectors and df_dIt . Jt, df_dI0 . J0 in one pass (instead of 2 x k_mi_grad, k_gemv, k_finish).
 *   3. k_mi_hess<MFMA> + k_mi_hess_finish for the self Hessian (MI.cc:565-601) when the Hessian type needs it.
 * (Folding 2 into 3 was tried: 294 VGPRs, one wave per SIMD, 223 us instead of 95 + 35.)
 * g, H of the search method as in NT/ESM.cc:298-377, NT/FCLK.cc:260-288, NT/ICLK.cc:206-251. */
static int mi_grad_blocks(const mtfhip_batch *b) { return std::min(simple_blocks_per_target(b->N), 64); }   /* block rows per target of pass 2 */
/* Enqueues the passes of one fused MI iteration (pl: MiPlan, mtfhip_api_internal.h).  Results on the device: d_mi_f [B]; d_mi_H = [B][64] Hessian (column-major
 * S x S) | [B][16] df_dIt . J, df_dI0 . J0 | [B][64] cmptInitHessian(J0) of SumOfStd.  `active` (device, may be NULL): targets
 * whose flag is 0 keep their It / Jt (the device-side loop). */
static int mi_enqueue(mtfhip_batch *b, const mtfhip_sm_desc *sm, const MiPlan &pl, const int *active, bool reduce_g = true) {
	const int nb = b->desc.mi_n_bins, nblk = mi_blocks(b);
	hipStream_t st = b->ctx->stream;
	/* 0 */
	mtfhip_sm_desc s0 = *sm;
	s0.sm = pl.need_jt ? MTFHIP_SM_FCLK : MTFHIP_SM_ICLK; s0.hess_type = pl.need_jt ? 1 : 0; s0.materialize = 1; s0.sec_ord_hess = 0;
	FusedArgs fa;
	TRY(fused_args(b, &s0, fa));
	fa.active = active;
	{
		TimedScope ts(b->ctx, "fused_lk");
		launch_fused_ssd(fused_view(b, fa), b->ctx->img, fa, b->d_partials, fused_blocks_per_target(b->N, b->B), st);
	}
	b->it_valid = true;
	b->dit_valid = b->jt_valid = pl.need_jt;
	if (pl.need_mean) {
		TRY(ensure_buf(b, MTFHIP_BUF_JM));
		TimedScope ts(b->ctx, "mean_jacobian");
		launch_mean_jacobian(b->view(), st);
	}
	/* 1 */
	const double *It = b->buf[MTFHIP_BUF_IT], *I0 = b->buf[MTFHIP_BUF_I0];
	{
		TimedScope ts(b->ctx, "mi_hist");
		if (pl.self) launch_mi_hist_self(b->view(), nb, b->mi_hist_norm, It, I0, b->d_mi_part, nblk, b->mi_row_len, st);
		else launch_mi_hist(b->view(), nb, b->mi_hist_norm, It, I0, b->d_mi_part, nblk, b->mi_row_len, st);
		launch_mi_tables_iter(b->view(), nb, b->desc.mi_pre_seed, b->mi_hist_norm, pl.self ? 1 : 0, b->d_mi_part, nblk, b->mi_row_len, b->d_mi_tb,
			b->d_mi_f, st);
	}
	/* 2 */
	double *d_g = b->d_mi_H + 64 * (size_t)b->B;
	{
		TimedScope ts(b->ctx, "mi_grad");
		const int ng = mi_grad_blocks(b);
		launch_mi_grad_gemv(b->view(), nb, b->mi_hist_norm, It, I0, b->d_mi_tb,
			pl.iclk ? nullptr : b->buf[pl.orig_jac ? MTFHIP_BUF_JM : MTFHIP_BUF_JT],
			(pl.fclk || pl.orig_jac) ? nullptr : b->buf[MTFHIP_BUF_J0], mi_j0_rebuild(b), sm->materialize ? b->buf[MTFHIP_BUF_DF_DIT] : nullptr,
			sm->materialize ? b->buf[MTFHIP_BUF_DF_DI0] : nullptr, b->d_partials, ng, st);
		if (reduce_g) launch_finish_rows(b->d_partials, ng, 16, d_g, b->B, st);   /* (the device-side loop sums the rows in its finish) */
	}
	/* 3: kind 0 init (MI.cc:461-513), 1 curr (:603-637), 2 self (:515-601), as mi_hessian in api_mi.hip */
	auto hess_pass = [&](int kind, int j_buf, double *out) {
		const double *A = b->buf[kind == 0 ? MTFHIP_BUF_I0 : MTFHIP_BUF_IT], *Bv = b->buf[kind == 1 ? MTFHIP_BUF_I0 : MTFHIP_BUF_IT];
		TimedScope ts(b->ctx, "mi_hess");
		launch_mi_hess(b->view(), nb, b->mi_hist_norm, A, Bv, b->d_mi_tb, kind == 0 ? MI_T_INIT : (kind == 1 ? MI_T_CURR : MI_T_SELF), kind == 0,
			b->buf[j_buf], b->d_mi_part, nblk, b->mi_row_len, st);
		launch_finish_rows(b->d_mi_part, nblk, b->mi_row_len, b->d_mi_red, b->B, st);
		launch_mi_hess_finish(b->view(), nb, b->d_mi_red, 1, b->mi_row_len, b->d_mi_tb, kind == 2 ? MI_SELF_JOINT : MI_JOINT,
			kind == 0 ? MI_HIST_INIT : MI_HIST_CURR, kind == 0, out, st);
	};
	switch (pl.hk) {
	case MiPlan::H_SUM_STD:   /* cmptSumOfHessians = cmptInitHessian(J0) + cmptCurrHessian(Jt) (MI.h) */
		hess_pass(0, MTFHIP_BUF_J0, b->d_mi_H + 80 * (size_t)b->B);
		hess_pass(1, MTFHIP_BUF_JT, b->d_mi_H);
		break;
	case MiPlan::H_SELF_JT: hess_pass(2, MTFHIP_BUF_JT, b->d_mi_H); break;
	case MiPlan::H_CURR_JT: hess_pass(1, MTFHIP_BUF_JT, b->d_mi_H); break;
	case MiPlan::H_CURR_JM: hess_pass(1, MTFHIP_BUF_JM, b->d_mi_H); break;
	case MiPlan::H_INIT_J0: hess_pass(0, MTFHIP_BUF_J0, b->d_mi_H); break;
	default: break;
	}
	return MTFHIP_OK;
}
/* The recompute form of the same iteration (kernels_mi_fused.hip): two pixel-level launches that read 28 + 44 B/px and write
 * nothing per pixel, instead of four that move 324 B/px.  Tolerance-mode arithmetic, the reference's 8 bins, nothing
 * materialised, every first-order type but SumOfStd (two Hessian passes: it keeps the materialising form). */
static bool mi_fast_ok(const mtfhip_batch *b, const mtfhip_sm_desc *sm, const MiPlan &pl) {
	static const bool enabled = !(std::getenv("MTFHIP_MI_RECOMPUTE") && std::getenv("MTFHIP_MI_RECOMPUTE")[0] == '0');
	/* r06: other bin counts up to ten (the shipped mi_n_bins 10, Config/modules.cfg:115) in the polynomial forms of pass 2 -- the constant and the
	 * self Hessian, single channel; 8 bins: every first-order form but SumOfStd */
	const int nb = b->desc.mi_n_bins;
	const bool bins_ok = nb == 8 || (nb <= 10 && b->C == 1 && (pl.hk == MiPlan::H_CONST || pl.hk == MiPlan::H_SELF_JT));
	return enabled && b->math_mode == MTFHIP_MATH_FAST && bins_ok && !sm->materialize && pl.hk != MiPlan::H_SUM_STD;
}
static MiFastPlan mi_fast_plan(const mtfhip_batch *b, const MiPlan &pl, const int *active, const mtfhip_sm_desc *sm) {
	MiFastPlan fp;
	fp.nb = b->desc.mi_n_bins;
	fp.nonchained = (sm && !sm->chained_warp) ? 1 : 0;
	fp.hk = pl.hk == MiPlan::H_CONST ? 0 : (pl.hk == MiPlan::H_SELF_JT ? 1 : (pl.hk == MiPlan::H_INIT_J0 ? 3 : 2));
	fp.hrow = pl.hk == MiPlan::H_CURR_JM ? 2 : (pl.hk == MiPlan::H_INIT_J0 ? 1 : 0);
	fp.need_dft = !pl.iclk; fp.need_df0 = !(pl.fclk || pl.orig_jac); fp.g_mean = pl.orig_jac;
	const bool need_j0 = fp.need_df0 || fp.g_mean || fp.hrow != 0;
	const MiJ0Rebuild rb = mi_j0_rebuild(b);
	fp.j0_mode = !need_j0 ? 0 : (rb.dI0 ? 1 : 2);
	fp.j0_init_variant = rb.init_variant;
	fp.grad_eps = b->desc.grad_eps; fp.norm_mult = b->norm_mult; fp.norm_add = b->norm_add; fp.hist_norm = b->mi_hist_norm;
	{
		/* (partition of unity, MI.cc:80-94: pixel values are mapped to [1, n_bins - 2], so every cubic B-spline window lies inside the bins and its
		 * weights sum to one: the histogram of It is the joint histogram's row sum to rounding -- MTFHIP_MI_HIST_ROWSUM=0: its own block product) */
		const char *e_rs = std::getenv("MTFHIP_MI_HIST_ROWSUM");   /* (read per plan: the parity test flips it) */
		const bool rowsum_env = !(e_rs && e_rs[0] == '0');
		fp.hist_from_joint = (rowsum_env && b->desc.mi_partition_of_unity) ? 1 : 0;
	}
	fp.active = active; fp.tb = b->d_mi_tb;
	return fp;
}
/* sec_ord_hess: sum_p df_dI(p) d2I_dp2(p) with MI's own per-pixel gradients / self gradient factor, from this iteration's tables
 * (d_mi_tb: filled by launch_mi_tables_iter in both forms of the iteration) -- one more pixel pass into d_d2_out */
static void mi_second_order(mtfhip_batch *b, const mtfhip_sm_desc *sm, int own_pts) {
	TimedScope tsc(b->ctx, "second_order");
	const int nb2 = simple_blocks_per_target(b->N);
	launch_second_order_ssd(b->view(), b->ctx->img, second_order_term(sm, MTFHIP_AM_MI), sm->chained_warp ? 1 : 0, b->d0_variant, b->desc.grad_eps,
		b->hess_eps, b->norm_mult, b->norm_add, b->d_d2_part, nb2, b->d_d2_out, b->ctx->stream, own_pts, SecondOrderNcc{nullptr, 0, nullptr},
		SecondOrderMi{b->d_mi_tb, b->mi_hist_norm});
}
/* how the finish combines the two gradient rows into g: ICLK's, FCLK's, ESM's on the mean Jacobian, ESM's difference */
static int mi_gmode(const MiPlan &pl) { return pl.iclk ? 0 : (pl.fclk ? 1 : (pl.orig_jac ? 2 : 3)); }
/* enqueues pass 1, the tables, pass 2 and the finish; do_track: the finish also solves, updates and tests convergence */
/* so_own_pts: -1 no second-order term; 1 inside the device loop (points re-derived from the warp), 0 from CURR_PTS (iterate) */
static int mi_enqueue_fast(mtfhip_batch *b, const mtfhip_sm_desc *sm, const MiPlan &pl, const int *active, const TrackState &ts, int do_track,
	int so_own_pts = -1) {
	const int nblk = mi_blocks(b);
	hipStream_t st = b->ctx->stream;
	MiFastPlan fp = mi_fast_plan(b, pl, active, sm);
	HIP_TRY(b->d_mi_poly.reserve((size_t)mi_poly_size(b->desc.mi_n_bins) * b->B));
	fp.poly = b->d_mi_poly;
	const BatchView bv = b->view();
	/* pass 1 holds 45.7 KB of LDS per workgroup: THREE workgroups per CU, so mi_blocks' ~4 per CU ran as one full round and a second one
	 * at a third of the occupancy (1024 workgroups over 768 slots; r05 ablation: the pass is bound by its sampling, 105 of 120 us, not
	 * by the block products).  Its own count: the largest multiple of the resident slots that the partial-row buffer holds. */
	/* (r05 advisor: nblk1 follows the device's resident slots, so tolerance mode's summation grouping -- and with it the last bits of its sums --
	 * depends on the CU count: results are reproducible run to run on one device, not bit for bit across devices; MTFHIP_MI_PASS1_BLOCKS pins it.
	 * Run to run on one device holds at every bin count: pass 2 sums its moment tables per wave, in wave order, with no atomics across
	 * waves -- tests/test_gpu_golden5.py::test_mi_fused_reproducible) */
	int nblk1 = nblk;
	{
		static const char *e_b1 = std::getenv("MTFHIP_MI_PASS1_BLOCKS");
		const int slots = 3 * std::max(b->ctx->n_cus, 1);
		if (e_b1) nblk1 = std::min(nblk, std::max(1, std::atoi(e_b1)));
		else if ((long)nblk * b->B > slots && slots / b->B >= 1) nblk1 = std::min(nblk, slots / b->B);
	}
	{
		TimedScope tsc(b->ctx, "mi_pass1");
		launch_mi_pass_hist(bv, b->ctx->img, fp, b->d_mi_part, nblk1, b->mi_row_len, st);
	}
	/* (the dense Hessian kinds read the tables themselves: no polynomial tables) */
	if (fp.hk <= 1) launch_mi_tables_poly(bv, fp.nb, b->desc.mi_pre_seed, b->mi_hist_norm, fp.hk == 1 ? 1 : 0, b->d_mi_part, nblk1, b->mi_row_len, b->d_mi_tb, b->d_mi_f, b->d_mi_poly, st);
	else launch_mi_tables_iter(bv, fp.nb, b->desc.mi_pre_seed, b->mi_hist_norm, fp.hk == 1 ? 1 : 0, b->d_mi_part, nblk1, b->mi_row_len, b->d_mi_tb, b->d_mi_f, st);
	{
		TimedScope tsc(b->ctx, "mi_pass2");
		launch_mi_pass_grad_hess(bv, b->ctx->img, fp, b->d_mi_part, nblk, st);
	}
	if (so_own_pts >= 0) mi_second_order(b, sm, so_own_pts);
	launch_mi_finish_fast(bv, *sm, ts, fp, mi_gmode(pl), do_track, b->d_mi_part, nblk, b->d_mi_H, b->d_mi_H + 64 * (size_t)b->B, b->d_mi_red, st);
	b->it_valid = b->dit_valid = b->jt_valid = false;
	return MTFHIP_OK;
}
int mi_iterate(mtfhip_batch *b, const mtfhip_sm_desc *sm, double *f, double *g, double *H) {
	const int S = b->S;
	hipStream_t st = b->ctx->stream;
	const MiPlan pl(sm);
	const int term = second_order_term(sm, MTFHIP_AM_MI);
	const int S2 = S * S;
	std::vector<double> so;
	if (term >= 0) {
		if (b->desc.mi_n_bins != 8) return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "iterate: second-order MI Hessians with other than 8 bins go through the per-function entry points");
		if (term != 0 && term != 4 && !b->init_pix_hess) return fail(MTFHIP_ERR_LOGIC, "iterate: init_template was run without sec_ord_hess");
		TRY(ensure_pts(b));
		TRY(ensure_second_order_scratch(b));
	}
	if (mi_fast_ok(b, sm, pl)) {
		TrackState ts{b->d_acc, b->d_h0, b->d_corners, b->d_init_corners_hm, b->d_active, b->d_iters, nullptr, nullptr, 1, nullptr, nullptr};
		TRY(mi_enqueue_fast(b, sm, pl, nullptr, ts, 0, term >= 0 ? 0 : -1));
	} else {
		TRY(mi_enqueue(b, sm, pl, nullptr));
		if (term >= 0) mi_second_order(b, sm, 0);
	}
	if (term >= 0) {
		so.resize((size_t)S2 * b->B);
		HIP_TRY(hipMemcpyAsync(so.data(), b->d_d2_out, sizeof(double) * so.size(), hipMemcpyDeviceToHost, st));
	}
	const size_t B = (size_t)b->B;
	std::vector<double> out(B * 145);
	HIP_TRY(hipMemcpyAsync(out.data(), b->d_mi_H, sizeof(double) * (pl.hk == MiPlan::H_SUM_STD ? 144 : 80) * B, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(out.data() + 144 * B, b->d_mi_f, sizeof(double) * B, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (int t = 0; t < b->B; ++t) {
		const double *Hs = &out[64 * (size_t)t], *gs = &out[64 * B + 16 * (size_t)t], *H2 = &out[80 * B + 64 * (size_t)t];
		TargetHost &h = b->th[t];
		h.f = out[144 * B + t];
		if (f) f[t] = h.f;
		double *gt = g + (size_t)t * S, *Ht = H + (size_t)t * S * S;
		for (int s = 0; s < S; ++s) gt[s] = pl.iclk ? gs[8 + s] : ((pl.fclk || pl.orig_jac) ? gs[s] : 0.5 * (gs[s] - gs[8 + s]));
		for (int k = 0; k < S * S; ++k) {
			const int r = k % S, c = k / S;
			const double hv = Hs[c * S + r];   /* k_mi_hess_finish writes column-major S x S */
			Ht[k] = pl.hk == MiPlan::H_CONST ? h.h0[k]
				: (pl.esm && sm->hess_type == 2) ? 0.5 * (hv + h.h0[k])
				: pl.hk == MiPlan::H_SUM_STD ? 0.5 * (hv + H2[c * S + r])
				: hv;
			if (term >= 0) Ht[k] += ((term == 1 || (pl.esm && sm->hess_type == 2)) ? 0.5 : 1.0) * so[(size_t)t * S2 + k];   /* (k_plane_sum_finish: entry (r, c) at c S + r, as Ht) */
		}
	}
	return MTFHIP_OK;
}

/* the MI driver of track_core (api_track.hip): the fused MI passes leave g and H on the device; k_finish_track_mi lays them out as one reduced
 * row per target and runs the same finish (solve, compositional update, convergence test) -- no host round trip per iteration */
int track_loop_mi(mtfhip_batch *b, const mtfhip_sm_desc *sm, TrackState &ts, const TrackCtx &cx) {
	const MiPlan pl(sm);
	ts.h_from_acc = 1;
	const bool fast = mi_fast_ok(b, sm, pl);
	const BatchView bv = b->view();
	std::vector<int> h_flags;
	for (int it = 0; it < cx.max_passes; ++it) {
		if (fast) {
			TRY(mi_enqueue_fast(b, sm, pl, b->d_active, ts, 1, cx.so_term >= 0 ? 1 : -1));
		} else {
			TRY(mi_enqueue(b, sm, pl, b->d_active, false));
			if (cx.so_term >= 0) mi_second_order(b, sm, 1);
			launch_finish_track_mi(bv, *sm, ts, pl.hk == MiPlan::H_SUM_STD, mi_gmode(pl), b->d_mi_H, b->d_partials, mi_grad_blocks(b), b->d_mi_red, b->ctx->stream);
		}
		if (loop_all_stopped(sm, cx.max_passes, it, b->d_active, b->B, b->ctx->stream, h_flags)) break;
	}
	return MTFHIP_OK;
}

} /* extern "C" */
