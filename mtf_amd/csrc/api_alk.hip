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
	TRY(am_refuse(b, fn, AM_AT_ADDITIVE_SM, alk_name(sm)));
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
	TRY(begin_entry(b));
	TRY(alk_check(b, sm, "init_template"));
	if (!b->have_corners) return fail(MTFHIP_ERR_LOGIC, "init_template before set_corners");
	b->init_pix_vals = b->init_pix_grad = b->init_sim = b->init_grad = false;   /* am->clearInitStatus() */
	TRY(mtfhip_am_initialize_pix_vals(b, nullptr));
	TRY(mtfhip_am_initialize_pix_grad(b, nullptr));
	TRY(mtfhip_am_initialize_similarity(b));
	TRY(mtfhip_am_initialize_grad(b));
	TRY(mtfhip_am_initialize_hess(b));
	const int S = b->S;
	std::vector<double> H0((size_t)b->B * S * S, 0.0);
	if (sm->hess_type == 0) {
		TRY(mtfhip_ssm_cmpt_pix_jacobian(b, MTFHIP_JAC_PIX, MTFHIP_BUF_DI0_DX, MTFHIP_BUF_J0));
		TRY(mtfhip_am_cmpt_self_hessian(b, MTFHIP_BUF_J0, H0.data()));
	}
	/* (the compositional loops' inverse of the constant Hessian and template moments do not exist for these methods: cleared, so that
	 * nothing stale is left behind for a later search method that skips its own init_template) */
	TRY(store_h0(b, H0.data(), false));
	if (b->desc.am == MTFHIP_AM_NCC) {
		HIP_TRY(b->d_ncc_tm.reserve(NCC_TM_COUNT * (size_t)b->B));
		HIP_TRY(hipMemsetAsync(b->d_ncc_tm, 0, sizeof(double) * NCC_TM_COUNT * (size_t)b->B, b->ctx->stream));
	}
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));   /* (store_h0's staging) */
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
	TRY(begin_entry(b));
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
	return assemble_rows(b, &smf, false, nblk, nullptr, 1.0, f, g, H);
}

/* The whole update() loop (NT/FALK.cc:132-257, NT/IALK.cc:90-199) on the device: max_iters x (k_alk_pass, k_alk_finish) enqueued back to
 * back between the shared skeleton's upload and read-back of the state slab (api_track.hip) -- a pass of a target whose stop flag is down
 * returns at once.  A rejected Levenberg-Marquardt step consumes an iteration of the for loop (the `continue` of NT/FALK.cc:166), so max_iters passes bound the call. */
int alk_track(mtfhip_batch *b, const mtfhip_sm_desc *sm, int *n_iters, double *corners) {
	FLUSH_AM(b);
	TRY(begin_entry(b));
	TRY(alk_check(b, sm, "track"));
	if (sm->max_iters <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "track: max_iters must be positive");
	if (!b->init_pix_vals || !b->init_pix_grad) return fail(MTFHIP_ERR_LOGIC, "track before init_template");
	TRY(need_image(b));
	hipStream_t st = b->ctx->stream;
	const bool ncc = b->desc.am == MTFHIP_AM_NCC;
	if (ncc && !b->d_ncc_tm) return fail(MTFHIP_ERR_LOGIC, "track before init_template");
	AlkArgs a; int nblk;
	TRY(alk_args(b, sm, b->B, a, nblk));
	b->fresh_reinit = false;
	TRY(loop_upload_slab(b, st, false));
	a.active = b->d_active;
	TrackState ts{b->d_acc, b->d_h0, b->d_corners, b->d_init_corners_hm, b->d_active, b->d_iters, ncc ? b->d_ncc : nullptr, ncc ? b->d_ncc_tm : nullptr, 0, nullptr, nullptr,
		b->d_trace, b->trace_cap};
	if (b->d_trace) HIP_TRY(hipMemsetAsync(b->d_trace, 0, sizeof(double) * kTraceStride * (size_t)b->trace_cap * b->B, st));
	if (sm->leven_marq) TRY(loop_lm_state(b, sm, st, &ts.lm));
	mtfhip_sm_desc smf = *sm;
	smf.sm = MTFHIP_SM_FCLK;   /* the row's type (k_alk_finish) */
	const BatchView bv = b->view();
	std::vector<int> h_flags;
	for (int it = 0; it < sm->max_iters; ++it) {
		{
			TimedScope tsc(b->ctx, "alk_pass");
			launch_alk_pass(bv, b->ctx->img, a, b->d_partials, nblk, st);
		}
		{
			TimedScope tsc(b->ctx, "alk_finish");
			launch_alk_finish(bv, smf, ts, b->d_partials, nblk, st);
		}
		hipError_t poll_active_flags = hipSuccess;   /* (a poll that cannot be made is this call's error; track_core goes on enqueueing) */
		if (loop_all_stopped(sm, sm->max_iters, it, b->d_active, b->B, st, h_flags, &poll_active_flags)) break;
		HIP_TRY(poll_active_flags);
	}
	const char *h_res;
	TRY(loop_read_back(b, st, 0, n_iters, corners, &h_res));
	alk_mark_outputs(b, a);
	loop_done(b);
	return MTFHIP_OK;
}

} /* extern "C" */
