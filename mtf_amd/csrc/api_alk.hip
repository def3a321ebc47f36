/*
 * api_alk.hip -- the additive search methods nt::FALK / nt::IALK (MTFHIP_SM_FALK / _IALK) behind mtfhip_batch_init_template / _iterate /
 * _track: what they serve and refuse, the template initialisation, one iteration for a host-side solve, and the device loop
 * (C-ABI implementation, include/mtfhip.h; kernels: kernels_alk.hip; shared declarations: mtfhip_api_internal.h)
 *
 * No CPU fallback exists: every entry point either runs its HIP kernels or returns an error.
 */
#include "mtfhip_api_internal.h"

extern "C" {

static const char *alk_name(const mtfhip_sm_desc *sm) { return sm->sm == MTFHIP_SM_FALK ? "FALK" : "IALK"; }

/* What the device route of FALK / IALK serves: SSD and NCC, single channel, first-order Hessians.  Everything else is the harness
 * classes' (nt::FALK / nt::IALK over the per-function entry points, mtf_amd/host/harness/SearchMethods.cpp). */
static int alk_check(const mtfhip_batch *b, const mtfhip_sm_desc *sm, const char *fn) {
	if (!sm) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);
	if (sm->hess_type < 0 || sm->hess_type > 2) return fail(MTFHIP_ERR_INVALID_ARG, "%s: hess_type %d invalid for search method %d", fn, sm->hess_type, sm->sm);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);
	if (b->desc.am == MTFHIP_AM_MI)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: %s with MI is not available on the device route (use nt::%s over the per-function entry points)", fn, alk_name(sm), alk_name(sm));
	if (intensity_mapped(b))
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: %s with %s is not available on the device route (use nt::%s over the per-function entry points)", fn, alk_name(sm),
			intensity_mapped_name(b), alk_name(sm));
	if (b->desc.am != MTFHIP_AM_SSD && b->desc.am != MTFHIP_AM_NCC) return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: unknown appearance model", fn);
	if (b->C != 1)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: %s with n_channels %d is not available on the device route (use nt::%s over the per-function entry points)", fn, alk_name(sm),
			b->C, alk_name(sm));
	if (sm->sec_ord_hess)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: %s with sec_ord_hess is not available on the device route (use nt::%s over the per-function entry points)", fn, alk_name(sm),
			alk_name(sm));
	return MTFHIP_OK;
}

/* the body of nt::FALK::initialize / nt::IALK::initialize after ssm->initialize (NT/FALK.cc:96-122, NT/IALK.cc:58-82): I0 and dI0_dx at
 * the current points and, for InitialSelf, init_pix_jacobian = cmptPixJacobian(dI0_dx) at the current state and its self Hessian */
int alk_init_template(mtfhip_batch *b, const mtfhip_sm_desc *sm) {
	FLUSH(b);
	if (b) { touch_all(b); b->lz.it_epoch = -1; TRY(ensure_df(b)); }
	TRY(alk_check(b, sm, "init_template"));
	if (!b->have_corners) return fail(MTFHIP_ERR_LOGIC, "init_template before set_corners");
	b->init_pix_vals = b->init_pix_grad = b->init_sim = b->init_grad = false;   /* am->clearInitStatus() */
	TRY(mtfhip_am_initialize_pix_vals(b, nullptr));
	TRY(mtfhip_am_initialize_pix_grad(b, nullptr));
	TRY(mtfhip_am_initialize_similarity(b));
	TRY(mtfhip_am_initialize_grad(b));
	TRY(mtfhip_am_initialize_hess(b));
	const int S = b->S;
	std::vector<double> H0((size_t)b->B * S * S, 0.0), h0dev((size_t)b->B * 64, 0.0);
	if (sm->hess_type == 0) {
		TRY(mtfhip_ssm_cmpt_pix_jacobian(b, MTFHIP_JAC_PIX, MTFHIP_BUF_DI0_DX, MTFHIP_BUF_J0));
		TRY(mtfhip_am_cmpt_self_hessian(b, MTFHIP_BUF_J0, H0.data()));
	}
	for (int t = 0; t < b->B; ++t) {
		std::memset(b->th[t].h0, 0, sizeof(b->th[t].h0));
		std::memcpy(b->th[t].h0, &H0[(size_t)t * S * S], sizeof(double) * S * S);
		std::memcpy(&h0dev[(size_t)t * 64], b->th[t].h0, sizeof(double) * 64);
	}
	HIP_TRY(hipMemcpyAsync(b->d_h0, h0dev.data(), sizeof(double) * h0dev.size(), hipMemcpyHostToDevice, b->ctx->stream));
	/* (the compositional loops' inverse of the constant Hessian and template moments do not exist for these methods: cleared, so that
	 * nothing stale is left behind for a later search method that skips its own init_template) */
	HIP_TRY(hipMemsetAsync(b->d_h0inv, 0, sizeof(double) * 64 * (size_t)b->B, b->ctx->stream));
	if (b->desc.am == MTFHIP_AM_NCC) {
		if (!b->d_ncc_tm) HIP_TRY(hipMalloc(&b->d_ncc_tm, sizeof(double) * 52 * (size_t)b->B));
		HIP_TRY(hipMemsetAsync(b->d_ncc_tm, 0, sizeof(double) * 52 * (size_t)b->B, b->ctx->stream));
	}
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));   /* h0dev is a stack-lifetime buffer */
	b->j0_is_template = false;   /* (J0, where it exists, is the cmptPixJacobian form: the compositional kernels' rebuild does not apply) */
	return MTFHIP_OK;
}

static int alk_args(mtfhip_batch *b, const mtfhip_sm_desc *sm, int n_targets, AlkArgs &a, int &nblk) {
	a.ialk = sm->sm == MTFHIP_SM_IALK ? 1 : 0;
	a.materialize = sm->materialize ? 1 : 0;
	a.grad_eps = b->desc.grad_eps; a.norm_mult = b->norm_mult; a.norm_add = b->norm_add;
	a.active = nullptr;
	fused_decomposition(b->N, n_targets, nblk, a.rows_per_block);
	if (nblk > b->nblk_max) return fail(MTFHIP_ERR_LOGIC, "%s: %d partial rows per target exceed the batch's %d", alk_name(sm), nblk, b->nblk_max);
	if (a.materialize) {
		TRY(ensure_buf(b, MTFHIP_BUF_IT)); TRY(ensure_buf(b, MTFHIP_BUF_JT));
		if (!a.ialk) TRY(ensure_buf(b, MTFHIP_BUF_DIT_DX));
	}
	return MTFHIP_OK;
}
static void alk_mark_outputs(mtfhip_batch *b, const AlkArgs &a) {
	b->it_valid = a.materialize != 0;
	b->jt_valid = a.materialize != 0;
	b->dit_valid = a.materialize != 0 && !a.ialk;
}

/* one pass at the current state: f, g = cmptCurrJacobian(curr_pix_jacobian) and H by hess_type as the search method holds them before
 * damping and the solve (NT/FALK.cc:144-221, NT/IALK.cc:101-171) */
int alk_iterate(mtfhip_batch *b, const mtfhip_sm_desc *sm, double *f, double *g, double *H) {
	FLUSH_AM(b);   /* the pass derives the sample points from the warp: CURR_PTS may stay stale */
	if (b) { touch_all(b); b->lz.it_epoch = -1; TRY(ensure_df(b)); }
	TRY(alk_check(b, sm, "iterate"));
	if (!g || !H) return fail(MTFHIP_ERR_INVALID_ARG, "iterate: NULL output");
	if (!b->init_pix_vals || !b->init_pix_grad) return fail(MTFHIP_ERR_LOGIC, "iterate before init_template");
	TRY(need_image(b));
	AlkArgs a; int nblk;
	TRY(alk_args(b, sm, b->B, a, nblk));
	{
		TimedScope ts(b->ctx, "alk_pass");
		launch_alk_pass(b->view(), b->ctx->img, a, b->d_partials, nblk, b->ctx->stream);
	}
	alk_mark_outputs(b, a);
	mtfhip_sm_desc smf = *sm;
	smf.sm = MTFHIP_SM_FCLK;   /* the row's type: g = df_dIt . Jt, H from Jt's own sums */
	const int S2 = b->S * b->S;
	if (b->desc.am == MTFHIP_AM_NCC) {
		TRY(read_rows(b, nblk, NCC_ACC_COUNT));
		for (int t = 0; t < b->B; ++t) {
			double ft;
			TRY(ncc_assemble(b, &smf, false, b->h_acc + (size_t)t * NCC_ACC_COUNT, b->th[t], &ft, g + (size_t)t * b->S, H + (size_t)t * S2));
			if (f) f[t] = ft;
		}
		b->ncc_host_newer = true;
		return MTFHIP_OK;
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t) {
		double ft;
		assemble(b, &smf, b->h_acc + (size_t)t * ACC_COUNT, b->th[t].h0, &ft, g + (size_t)t * b->S, H + (size_t)t * S2);
		b->th[t].f = ft;
		if (f) f[t] = ft;
	}
	return MTFHIP_OK;
}

/* The whole update() loop (NT/FALK.cc:132-257, NT/IALK.cc:90-199) on the device: max_iters x (k_alk_pass, k_alk_finish) enqueued back to
 * back -- a pass of a target whose stop flag is down returns at once -- and one read-back of the state slab.  A rejected
 * Levenberg-Marquardt step consumes an iteration of the for loop (the `continue` of NT/FALK.cc:166), so max_iters passes bound the call. */
int alk_track(mtfhip_batch *b, const mtfhip_sm_desc *sm, int *n_iters, double *corners) {
	FLUSH_AM(b);
	if (b) { touch_all(b); b->lz.it_epoch = -1; TRY(ensure_df(b)); }
	TRY(alk_check(b, sm, "track"));
	if (sm->max_iters <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "track: max_iters must be positive");
	if (!b->init_pix_vals || !b->init_pix_grad) return fail(MTFHIP_ERR_LOGIC, "track before init_template");
	TRY(need_image(b));
	hipStream_t st = b->ctx->stream;
	const bool ncc = b->desc.am == MTFHIP_AM_NCC;
	if (ncc && !b->d_ncc_tm) return fail(MTFHIP_ERR_LOGIC, "track before init_template");
	AlkArgs a; int nblk;
	TRY(alk_args(b, sm, b->B, a, nblk));
	/* active = 1, iters = 0, corners, warps, states, NCC scalars: one pinned async copy of the whole slab (as track_core, api_fused.hip) */
	b->fresh_reinit = false;
	std::memcpy(b->h_stage_b + 45 * sizeof(double) * (size_t)b->B, b->h_stage_a + 45 * sizeof(double) * (size_t)b->B, 9 * sizeof(double) * (size_t)b->B);
	fill_stage(b, b->h_stage_b, nullptr, 1, true);
	if (b->h_stage_b_dev) launch_ingest_host(b->h_stage_b_dev, b->d_slab, b->slab_bytes, st);
	else HIP_TRY(hipMemcpyAsync(b->d_slab, b->h_stage_b, b->slab_bytes, hipMemcpyHostToDevice, st));
	b->warps_dirty = false;   /* the slab carries the warps */
	a.active = b->d_active;
	TrackState ts{b->d_acc, b->d_h0, b->d_corners, b->d_init_corners_hm, b->d_active, b->d_iters, ncc ? b->d_ncc : nullptr, ncc ? b->d_ncc_tm : nullptr, 0, nullptr, nullptr,
		b->d_trace, b->trace_cap};
	if (b->d_trace) HIP_TRY(hipMemsetAsync(b->d_trace, 0, sizeof(double) * kTraceStride * (size_t)b->trace_cap * b->B, st));
	if (sm->leven_marq) {
		/* per-target LM state: prev_similarity 0, leven_marq_delta = lm_delta_init, no pending reset, iteration 0 */
		if (!b->d_lm) HIP_TRY(hipMalloc(&b->d_lm, sizeof(double) * kLmStride * (size_t)b->B));
		std::vector<double> lm0((size_t)kLmStride * b->B, 0.0);
		for (int t = 0; t < b->B; ++t) lm0[(size_t)kLmStride * t + 1] = sm->lm_delta_init;
		HIP_TRY(hipMemcpyAsync(b->d_lm, lm0.data(), sizeof(double) * lm0.size(), hipMemcpyHostToDevice, st));
		HIP_TRY(hipStreamSynchronize(st));   /* lm0 is a stack-lifetime buffer */
		ts.lm = b->d_lm;
	}
	mtfhip_sm_desc smf = *sm;
	smf.sm = MTFHIP_SM_FCLK;   /* the row's type (k_alk_finish) */
	const BatchView bv = b->view();
	std::vector<int> h_active;
	for (int it = 0; it < sm->max_iters; ++it) {
		{
			TimedScope tsc(b->ctx, "alk_pass");
			launch_alk_pass(bv, b->ctx->img, a, b->d_partials, nblk, st);
		}
		{
			TimedScope tsc(b->ctx, "alk_finish");
			launch_alk_finish(bv, smf, ts, b->d_partials, nblk, st);
		}
		/* with a reachable convergence test the flags are looked at every eighth iteration: one small copy + sync against up to seven
		 * idle iterations (as track_core) */
		if (sm->epsilon > 0 && (it + 1) % 8 == 0 && it + 1 < sm->max_iters) {
			h_active.resize(b->B);
			HIP_TRY(hipMemcpyAsync(h_active.data(), b->d_active, sizeof(int) * b->B, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			bool any = false;
			for (int v : h_active) any = any || v != 0;
			if (!any) break;
		}
	}
	const char *h_res = b->h_stage_b;
	if (b->h_pub_dev) {
		const unsigned long long seq = ++b->acc_seq;
		launch_publish_host(b->d_slab, b->h_pub_dev, b->slab_bytes, b->d_fin_count, b->h_flag_dev, seq, st);
		TRY(wait_host_flag(b, seq));
		h_res = b->h_pub;
	} else {
		HIP_TRY(hipMemcpyAsync(b->h_stage_b, b->d_slab, b->slab_bytes, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	{
		const size_t Bt = (size_t)b->B;
		const double *p = reinterpret_cast<const double *>(h_res);
		const double *w = p, *s = p + 9 * Bt, *cr = p + 17 * Bt;
		const int *iters = reinterpret_cast<const int *>(h_res + b->slab_dbl_bytes) + Bt;
		for (int t = 0; t < b->B; ++t) {
			std::memcpy(b->th[t].warp.m, w + 9 * t, sizeof(double) * 9);
			std::memcpy(b->th[t].state, s + 8 * t, sizeof(double) * 8);
			std::memcpy(b->th[t].corners, cr + 8 * t, sizeof(double) * 8);
			if (n_iters) n_iters[t] = iters[t];
			if (corners) std::memcpy(corners + 8 * t, cr + 8 * t, sizeof(double) * 8);
		}
	}
	alk_mark_outputs(b, a);
	b->pts_stale = true;       /* CURR_PTS follow the final warp when an un-fused kernel next needs them */
	b->stage_a_busy = false;   /* the stream has drained: whatever set_corners staged has been consumed */
	return MTFHIP_OK;
}

} /* extern "C" */
