/*
 * api_lazy.hip -- the deferred-fusion layer behind the per-function entry points (mtfhip_batch::Lazy; SSD, NCC and MI, single channel):
 * replay, refresh, and the fused execution of a recognised call sequence.
 *
 * The pixel-level producers of an iteration (updatePixVals, updatePixGrad, cmpt*PixJacobian, updateSimilarity, update*Grad, the mean
 * Jacobian) only record themselves (api_am.hip).  What happens to the record:
 *   - lazy_try_fused, on the first call that needs a number on the host (cmptInitJacobian / cmptCurrJacobian / cmptDifferenceOfJacobians):
 *     ONE fused launch with materialize = 1 when the pending calls plus that request are one of
 *       FCLK  NT/FCLK.cc:171-358: updatePixVals, updateSimilarity, updateCurrGrad, pixel gradient + pixel Jacobian, cmptCurrJacobian(Jt)
 *       ESM   NT/ESM.cc:170-296: ... updateInitGrad, cmptDifferenceOfJacobians(J0, Jt)   (jac_type Original: cmptCurrJacobian(Jm))
 *       ICLK  NT/ICLK.cc:160-299: updatePixVals, updateSimilarity, updateInitGrad, cmptInitJacobian(J0)
 *     (MI: the fused MI passes, mi_lazy_fused in api_mi.hip; NCC: the moment forms of api_ncc.hip);
 *   - lazy_try_similarity, on getSimilarity() / getLikelihood() right after updatePixVals + updateSimilarity -- Levenberg-Marquardt's test
 *     in the middle of every iteration (NT/ESM.cc:186-204, FCLK.cc:205-223, ICLK.cc:181-199): one launch of the lean (ICLK-type) fused kernel;
 *   - lazy_flush, from every other entry point: the recorded calls replayed through the un-fused kernels, in the order they were made --
 *     so the buffers and results are those of the call-by-call execution either way.
 * The gradient vectors a fused launch stood in for are marked stale and derived on first use (ensure_one / ensure_df), from the IT they
 * belong to: the current one, or the shadow that protect_stale keeps when IT has to change first.
 * (C-ABI implementation, include/mtfhip.h; shared declarations: mtfhip_api_internal.h; no CPU fallback: HIP kernels or an error)
 */
#include "mtfhip_api_internal.h"

extern "C" {

/* SSD's DF_DI0 = It - I0 and DF_DIT = -DF_DI0 (SSDBase.cc:75-121), NCC's gradient vectors (NCC.cc:163-234), when a fused
 * launch stood in for the calls that write them: derived from the IT (current or shadow) and scalars they belong to */
void stale_clear(mtfhip_batch *b, bool df0, bool dft) {
	mtfhip_batch::Lazy &L = b->lz;
	if (df0) L.df0_stale = L.df0_sh = false;
	if (dft) L.dft_stale = L.dft_sh = false;
	if (!L.df0_sh && !L.dft_sh) L.shadow_valid = false;
}
static void swap_shadow(mtfhip_batch *b) {
	b->buf[MTFHIP_BUF_IT].swap(b->d_it_shadow);
	if (b->desc.am == MTFHIP_AM_NCC)
		for (int t = 0; t < b->B; ++t) {
			TargetHost &h = b->th[t]; mtfhip_batch::Lazy::NccSave &v = b->lz.ncc_shadow[t];
			std::swap(h.It_mean, v.It_mean); std::swap(h.a, v.a); std::swap(h.b, v.b); std::swap(h.f, v.f);
		}
	b->ncc_host_newer = true;   /* d_ncc has to follow whichever set of scalars is current */
}
int ensure_one(mtfhip_batch *b, bool curr) {
	mtfhip_batch::Lazy &L = b->lz;
	if (curr ? !L.dft_stale : !L.df0_stale) return MTFHIP_OK;
	const bool sh = curr ? L.dft_sh : L.df0_sh;
	if (sh) swap_shadow(b);
	int rc = MTFHIP_OK;
	if (const auto op = am_ops(b).grad) {   /* (NCC: update*Grad itself, which also clears the mark) */
		rc = op(b, curr ? 1 : 0);
	} else {
		/* the residual kernel writes It - I0 into the view's DF_DI0; for df_dIt it is pointed at DF_DIT and negated in place */
		BatchView v = b->view();
		if (curr) v.buf[MTFHIP_BUF_DF_DI0] = b->buf[MTFHIP_BUF_DF_DIT];
		{
			TimedScope ts(b->ctx, "ssd_residual");
			launch_ssd_residual(v, b->d_partials, simple_blocks_per_target(b->N), b->ctx->stream);
		}
		if (curr) {
			TimedScope ts(b->ctx, "negate");
			launch_negate(b->buf[MTFHIP_BUF_DF_DIT], b->buf[MTFHIP_BUF_DF_DIT], (size_t)b->N * b->B, b->ctx->stream);
		}
	}
	if (sh) swap_shadow(b);
	if (rc) return rc;
	stale_clear(b, !curr, curr);
	return MTFHIP_OK;
}
int ensure_df(mtfhip_batch *b) {
	TRY(ensure_one(b, false));
	return ensure_one(b, true);
}
/* IT is about to be overwritten by a launch that re-produces df_dI0 (w0) / df_dIt (wt) or not: stale vectors that it does
 * not re-produce keep their IT by a buffer swap instead of being derived now */
int protect_stale(mtfhip_batch *b, bool w0, bool wt) {
	mtfhip_batch::Lazy &L = b->lz;
	const bool cur0 = L.df0_stale && !w0 && !L.df0_sh, curt = L.dft_stale && !wt && !L.dft_sh;
	if (!cur0 && !curt) return MTFHIP_OK;
	if (L.shadow_valid) {   /* an older shadow is still referenced (rare): settle it first */
		if (L.df0_sh) TRY(ensure_one(b, false));
		if (L.dft_sh) TRY(ensure_one(b, true));
	}
	HIP_TRY(b->d_it_shadow.reserve(b->per_target[MTFHIP_BUF_IT] * b->B));
	L.ncc_shadow.resize(b->B);
	for (int t = 0; t < b->B; ++t) { const TargetHost &h = b->th[t]; L.ncc_shadow[t] = {h.It_mean, h.a, h.b, h.f}; }
	b->buf[MTFHIP_BUF_IT].swap(b->d_it_shadow);   /* the launch fills the other buffer; th keeps the current scalars */
	L.shadow_valid = true;
	if (cur0) L.df0_sh = true;
	if (curt) L.dft_sh = true;
	return MTFHIP_OK;
}
/* replays the recorded calls through the un-fused kernels, in the order they were made */
int lazy_flush(mtfhip_batch *b, bool pts) {
	mtfhip_batch::Lazy &L = b->lz;
	if (b->init_mirror_seq && !b->hold_init_pull) TRY(pull_init_mirrors(b));   /* (a fused template initialisation left its small results in a pinned record) */
	/* whatever follows a full flush may launch a kernel that reads the current points; so may the replayed calls */
	if (pts || L.pv || L.gp || L.pg || L.pj) TRY(ensure_pts(b));
	if (!L.any()) return MTFHIP_OK;
	struct Op { long seq; int kind; };
	Op ops[8]; int n = 0;
	if (L.pv) ops[n++] = {L.pv, 0};
	if (L.gp) ops[n++] = {L.gp, 1};
	if (L.pg) ops[n++] = {L.pg, 2};
	if (L.pj) ops[n++] = {L.pj, 3};
	if (L.sim) ops[n++] = {L.sim, 4};
	if (L.cg) ops[n++] = {L.cg, 5};
	if (L.ig) ops[n++] = {L.ig, 6};
	if (L.jm) ops[n++] = {L.jm, 7};
	std::sort(ops, ops + n, [](const Op &x, const Op &y) { return x.seq < y.seq; });
	const int pg_kind = L.pg_kind, pj_variant = L.pj_variant; const bool need_f = L.sim_need_f;
	L.pv = L.gp = L.pg = L.pj = L.sim = L.cg = L.ig = L.jm = 0;   /* cleared first: the executors below may flush */
	for (int i = 0; i < n; ++i) {
		switch (ops[i].kind) {
		case 0: TRY(do_update_pix_vals(b, nullptr)); break;
		case 1: TRY(do_update_grad_pts(b, b->desc.grad_eps)); break;
		case 2: TRY(pix_grad_common(b, nullptr, pg_kind == 2, false)); break;
		case 3: TRY(do_cmpt_pix_jacobian(b, pj_variant, MTFHIP_BUF_DIT_DX, MTFHIP_BUF_JT)); break;
		case 4: TRY(do_update_similarity(b, need_f ? 0 : 1)); break;
		case 5: TRY(do_update_curr_grad(b)); break;
		case 6: if (const auto op = am_ops(b).grad) TRY(op(b, 0)); break;   /* (null: SSD::updateInitGrad is empty, SSDBase.h) */
		default: TRY(do_mean_jacobian(b)); break;
		}
	}
	return MTFHIP_OK;
}
/* `*done` = 1 when the pending calls plus this Jacobian request were served by ONE fused launch (g filled with the AM's
 * raw Jacobian), 0 when the caller has to flush and take the un-fused route */
int lazy_try_fused(mtfhip_batch *b, int trig, int j_a, int j_b, double *g, int *done) {
	*done = 0;
	mtfhip_batch::Lazy &L = b->lz;
	if (!L.enabled) return MTFHIP_OK;
	/* either updatePixVals + updateSimilarity are part of the pending set, or they already ran for this very warp and image */
	const bool replay = L.pv && L.sim && L.pv < L.sim;
	const bool current = !L.pv && !L.sim && L.it_epoch == L.epoch && L.df0_it_ver == L.ver[MTFHIP_BUF_IT];
	if (!replay && !current) return MTFHIP_OK;
	if (!b->init_pix_vals || !b->init_sim || !b->have_corners || !b->ctx->img.data || b->ctx->img.channels != 1) return MTFHIP_OK;
	mtfhip_sm_desc sm;
	std::memset(&sm, 0, sizeof(sm));
	sm.materialize = 1; sm.max_iters = 1; sm.chained_warp = 1;
	bool pixel_chain = false;
	if (L.pg || L.pj || L.gp) {
		if (!L.pg || !L.pj || L.pg > L.pj) return MTFHIP_OK;
		if (L.pg_kind == 1) { if (L.gp || L.pj_variant != MTFHIP_JAC_WARPED) return MTFHIP_OK; }
		else { if (!L.gp || L.gp > L.pg || L.pj_variant != MTFHIP_JAC_INIT) return MTFHIP_OK; sm.chained_warp = 0; }
		pixel_chain = true;
	}
	if (L.jm && (!pixel_chain || L.jm < L.pj)) return MTFHIP_OK;
	double gscale = 1.0;
	if (trig == LAZY_INIT_JAC) {
		if (pixel_chain || L.jm || j_a != MTFHIP_BUF_J0 || !b->buf[MTFHIP_BUF_J0]) return MTFHIP_OK;
		sm.sm = MTFHIP_SM_ICLK; sm.hess_type = 0;
	} else {
		if (!pixel_chain || !L.cg || L.cg < L.sim) return MTFHIP_OK;   /* (L.sim is 0 when it already ran) */
		if (trig == LAZY_DIFF_JAC) {
			if (j_a != MTFHIP_BUF_J0 || j_b != MTFHIP_BUF_JT || !b->buf[MTFHIP_BUF_J0]) return MTFHIP_OK;
			sm.sm = MTFHIP_SM_ESM; sm.hess_type = L.jm ? 3 : 5;
		} else if (j_a == MTFHIP_BUF_JT) {
			sm.sm = MTFHIP_SM_FCLK; sm.hess_type = 2;
		} else if (j_a == MTFHIP_BUF_JM && L.jm && b->buf[MTFHIP_BUF_J0]) {
			sm.sm = MTFHIP_SM_ESM; sm.hess_type = 3; gscale = 0.5;   /* df_dIt . (J0 + Jt) / 2, the halving is exact */
		} else return MTFHIP_OK;
	}
	if (b->desc.am == MTFHIP_AM_MI) return mi_lazy_fused(b, trig, j_a, sm, replay, g, done);
	const bool ncc = b->desc.am == MTFHIP_AM_NCC;
	if (ncc && trig == LAZY_INIT_JAC && !L.ig) return MTFHIP_OK;   /* NCC's df_dI0 comes from updateInitGrad */
	/* gradients a previous fused launch skipped and this one will not re-produce keep their IT (when IT is current the
	 * launch rewrites the same bits, nothing to protect) */
	if (replay) TRY(protect_stale(b, ncc ? L.ig != 0 : true, L.cg != 0));
	if (current && trig == LAZY_INIT_JAC && !L.no_cache) {
		/* the lean launch behind getSimilarity() already accumulated this Jacobian for the same IT and J0: no launch */
		bool served = false;
		if (!ncc && L.sim_g_it == L.ver[MTFHIP_BUF_IT] && L.sim_g_j0 == L.ver[MTFHIP_BUF_J0] && !L.sim_g.empty()) {
			for (int t = 0; t < b->B; ++t) std::memcpy(g + (size_t)t * b->S, &L.sim_g[(size_t)8 * t], sizeof(double) * b->S);
			served = true;
		} else if (ncc && !L.ncc_M.empty() && L.ncc_M_it == L.ver[MTFHIP_BUF_IT] && L.ncc_tm_ver == L.ver[MTFHIP_BUF_J0]) {
			std::memcpy(b->h_acc, L.ncc_M.data(), sizeof(double) * L.ncc_M.size());
			const long jt = L.ncc_M_jt, jm = L.ncc_M_jm; const bool mean = L.ncc_M_mean;
			TRY(ncc_lazy_outputs(b, trig, j_a, mean, g));
			L.ncc_M_jt = jt; L.ncc_M_jm = jm;   /* the rows are unchanged: what they hold about Jt / Jm stays as it was */
			served = true;
		}
		if (served) {
			if (ncc && L.ig) { L.df0_stale = true; L.df0_sh = false; if (!L.dft_sh) L.shadow_valid = false; }
			L.ig = 0;
			*done = 1;
			return MTFHIP_OK;
		}
	}
	if (ncc && sm.sm != MTFHIP_SM_FCLK && L.ncc_tm_ver != L.ver[MTFHIP_BUF_J0]) {   /* moments of the template's Jacobian */
		TRY(ncc_template_moments(b));
		L.ncc_tm_ver = L.ver[MTFHIP_BUF_J0];
	}
	FusedArgs fa;
	TRY(fused_args(b, &sm, fa));
	const int nblk = fused_blocks_per_target(b->N, b->B);
	{
		TimedScope ts(b->ctx, "fused_lk");
		launch_fused_ssd(fused_view(b, fa), b->ctx->img, fa, b->d_partials, nblk, b->ctx->stream);
	}
	touch(b, MTFHIP_BUF_IT);
	b->it_valid = true;
	L.it_epoch = L.epoch;
	if (fa.mode != 2) { touch(b, MTFHIP_BUF_DIT_DX); touch(b, MTFHIP_BUF_JT); b->dit_valid = b->jt_valid = true; }
	const bool want_mean = L.jm != 0;
	/* the N-sized gradient vectors the consumed calls would have written: SSD's df_dI0 is updateSimilarity's residual,
	 * NCC's comes from updateInitGrad; df_dIt from updateCurrGrad in both */
	if (ncc ? L.ig != 0 : replay) { L.df0_stale = true; L.df0_sh = false; }
	L.df0_it_ver = L.ver[MTFHIP_BUF_IT];          /* (when IT was current the launch rewrote the same bits) */
	if (L.cg) { L.dft_stale = true; L.dft_sh = false; }
	if (!L.df0_sh && !L.dft_sh) L.shadow_valid = false;
	L.pv = L.gp = L.pg = L.pj = L.sim = L.cg = L.ig = L.jm = 0;
	if (want_mean) TRY(do_mean_jacobian(b));
	if (ncc) {
		TRY(read_rows(b, nblk, NCC_ACC_COUNT));
		TRY(ncc_lazy_outputs(b, trig, j_a, fa.hess_mean != 0, g));
		*done = 1;
		return MTFHIP_OK;
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t) {
		const double *acc = b->h_acc + (size_t)t * ACC_COUNT;
		b->th[t].f = -acc[ACC_RR] / 2;
		for (int s = 0; s < b->S; ++s) g[(size_t)t * b->S + s] = gscale * acc[ACC_G + s];
	}
	if (fa.mode != 2 && !L.no_cache) {   /* the Gram matrix the launch accumulated: Jt, or Jm with hess_mean */
		L.gram_buf = fa.hess_mean ? MTFHIP_BUF_JM : MTFHIP_BUF_JT;
		L.gram_ver = L.ver[L.gram_buf];
		L.gram.resize((size_t)36 * b->B);
		for (int t = 0; t < b->B; ++t) std::memcpy(&L.gram[(size_t)36 * t], b->h_acc + (size_t)t * ACC_COUNT + ACC_H, sizeof(double) * 36);
	}
	*done = 1;
	return MTFHIP_OK;
}

/* getSimilarity() right after updatePixVals + updateSimilarity: one launch of the lean (ICLK-type) fused kernel
 * writes IT and accumulates what f needs, instead of sample + residual (SSD) or sample + two reduction passes with
 * two host round trips (NCC).  Anything else pending, or nothing pending: not taken, the caller flushes. */
int lazy_try_similarity(mtfhip_batch *b) {
	mtfhip_batch::Lazy &L = b->lz;
	if (!L.enabled || !L.pv || !L.sim || L.pv > L.sim || L.gp || L.pg || L.pj || L.cg || L.ig || L.jm) return MTFHIP_OK;
	if (!b->init_pix_vals || !b->init_sim || !b->have_corners || !b->ctx->img.data || b->ctx->img.channels != 1) return MTFHIP_OK;
	const bool ncc = b->desc.am == MTFHIP_AM_NCC;
	mtfhip_sm_desc sm;
	std::memset(&sm, 0, sizeof(sm));
	sm.sm = MTFHIP_SM_ICLK; sm.hess_type = 0; sm.materialize = 1; sm.max_iters = 1; sm.chained_warp = 1;
	FusedArgs fa;
	TRY(fused_args(b, &sm, fa));
	const bool mi = b->desc.am == MTFHIP_AM_MI;
	if (!mi) TRY(protect_stale(b, !ncc, false));   /* SSD's updateSimilarity re-produces df_dI0 */
	const int nblk = fused_blocks_per_target(b->N, b->B);
	{
		TimedScope ts(b->ctx, "fused_lk");
		launch_fused_ssd(fused_view(b, fa), b->ctx->img, fa, b->d_partials, nblk, b->ctx->stream);
	}
	touch(b, MTFHIP_BUF_IT);
	b->it_valid = true;
	L.it_epoch = L.epoch;
	L.df0_it_ver = L.ver[MTFHIP_BUF_IT];
	if (!ncc && !mi) { L.df0_stale = true; L.df0_sh = false; if (!L.dft_sh) L.shadow_valid = false; }
	L.pv = L.sim = 0;
	if (mi) return mi_lazy_similarity(b);
	if (ncc) {
		TRY(read_rows(b, nblk, NCC_ACC_COUNT));
		for (int t = 0; t < b->B; ++t) ncc_refresh_mirrors(b, b->th[t], b->h_acc + (size_t)t * NCC_ACC_COUNT);
		b->ncc_host_newer = true;
		if (!L.no_cache) {   /* sum It J0 and the scalars: enough for cmptInitJacobian / cmptInitHessian of this IT */
			L.ncc_M.assign(b->h_acc.get(), b->h_acc + (size_t)NCC_ACC_COUNT * b->B);
			L.ncc_M_mean = false; L.ncc_M_it = L.ver[MTFHIP_BUF_IT]; L.ncc_M_jt = L.ncc_M_jm = -1;
		}
		return MTFHIP_OK;
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t) b->th[t].f = -b->h_acc[(size_t)t * ACC_COUNT + ACC_RR] / 2;
	if (!L.no_cache) {
		L.sim_g.resize((size_t)8 * b->B);
		for (int t = 0; t < b->B; ++t) std::memcpy(&L.sim_g[(size_t)8 * t], b->h_acc + (size_t)t * ACC_COUNT + ACC_G, sizeof(double) * 8);
		L.sim_g_it = L.ver[MTFHIP_BUF_IT]; L.sim_g_j0 = L.ver[MTFHIP_BUF_J0];
	}
	return MTFHIP_OK;
}

} /* extern "C" */
