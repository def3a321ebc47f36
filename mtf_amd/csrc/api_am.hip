/*
 * api_am.hip -- the per-function AppearanceModel entry points: ImageBase, kAmOps (what differs by model) and the entry points over it with
 * SSD's bodies, the Jacobian / Hessian entry points, second order.  Each model's own code is in its unit (api_ncc.hip, api_mi.hip,
 * api_spss.hip, api_ssim.hip, api_ccre.hip, api_imap.hip), the deferred-fusion layer that records and replays these calls in api_lazy.hip
 * (C-ABI implementation, include/mtfhip.h; shared declarations: mtfhip_api_internal.h)
 *
 * No CPU fallback exists: every entry point either runs its HIP kernels or returns an error.
 */
#include "mtfhip_api_internal.h"

/* NCC::getLikelihood NCC.cc:50-53, MI::getLikelihood and SSIM::getLikelihood SSIM.cc:45-48 are one form: d = 1 / f - 1 */
static int recip_likelihood(const mtfhip_batch *b, int t, double *l) { *l = ssim_likelihood(b->th[t].f, b->desc.likelihood_alpha); return MTFHIP_OK; }
/* one row per MTFHIP_AM_* (AmOps, mtfhip_api_internal.h).  A null entry: the SSD body of the entry point -- SSD and the SCV family */
static const AmOps kAmOps[] = {
	{nullptr, nullptr, nullptr, nullptr, nullptr},
	{ncc_initialize_similarity, ncc_update_similarity, ncc_grad, ncc_hessian, recip_likelihood},
	{mi_initialize_similarity, mi_update_similarity, mi_grad, mi_hessian, recip_likelihood},
	{nullptr, nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr, nullptr},
	{nullptr, nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr, nullptr},
	{spss_initialize_similarity, spss_update_similarity, spss_update_grad, spss_hessian, spss_likelihood},
	{ncc_initialize_similarity, ssim_update_similarity, ssim_update_grad, ssim_hessian, recip_likelihood},
	{ccre_initialize_similarity, ccre_update_similarity, ccre_grad, ccre_hessian, ccre_likelihood},
};
static_assert(sizeof(kAmOps) / sizeof(kAmOps[0]) == MTFHIP_AM_CCRE + 1, "one row of operations per MTFHIP_AM_*");
const AmOps &am_ops(const mtfhip_batch *b) { return kAmOps[b->desc.am]; }

extern "C" {

/* ------------------------------------------------------------------ ImageBase */
int mtfhip_am_initialize_pix_vals(mtfhip_batch *b, const double *pts) {
	FLUSH(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "initialize_pix_vals: NULL batch");
	TRY(need_image(b));
	const double *dp;
	TRY(resolve_pts(b, pts, MTFHIP_BUF_CURR_PTS, 2 * (size_t)b->NP, &dp));
	++b->frame_count;   /* ImageBase.cc:74 */
	{
		TimedScope ts(b->ctx, "sample");
		launch_sample(b->view(), b->ctx->img, dp, b->buf[MTFHIP_BUF_I0], b->norm_mult, b->norm_add, b->ctx->stream);
	}
	if (!b->init_pix_vals) {
		HIP_TRY(hipMemcpyAsync(b->buf[MTFHIP_BUF_IT], b->buf[MTFHIP_BUF_I0], sizeof(double) * b->N * b->B, hipMemcpyDeviceToDevice, b->ctx->stream));
		b->init_pix_vals = true;
		b->it_valid = true;
	}
	return imap_capture(b);   /* the SCV family's initializePixVals (SCV.cc:166, RSCV.cc:124-168, LSCV.cc:232, LRSCV.cc:197-222) */
}
/* SSD::updateModel AM/src/SSD.cc:49-75, NCC::updateModel AM/src/NCC.cc:539-566 (the search methods call it at the end of update()
 * when enable_learning is set, NT/ESM.cc:293-295): template <- average with the patch at pts, then AppearanceModel::reinitialize
 * (AppearanceModel.h:119-123).  learning_rate outside [0, 1] = running average over the frames seen (SSD.cc:45). */
int mtfhip_am_update_model(mtfhip_batch *b, const double *pts, double learning_rate) {
	FLUSH(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "update_model: NULL batch");
	TRY(am_refuse(b, "update_model", AM_AT_UPDATE_MODEL));   /* (served: SSD and NCC) */
	TRY(single_channel(b, "update_model"));
	if (!b->init_pix_vals) return fail(MTFHIP_ERR_LOGIC, "update_model before initializePixVals");
	TRY(need_image(b));
	TRY(ensure_df(b));
	const double *dp;
	TRY(resolve_pts(b, pts, MTFHIP_BUF_CURR_PTS, 2 * (size_t)b->NP, &dp));
	++b->frame_count;
	const int running = (learning_rate < 0 || learning_rate > 1) ? 1 : 0;
	{
		TimedScope ts(b->ctx, "sample");
		launch_update_model(b->view(), b->ctx->img, dp, b->buf[MTFHIP_BUF_I0], b->norm_mult, b->norm_add, (double)b->frame_count,
			learning_rate, running, b->ctx->stream);
	}
	/* everything cached about the template is void: buffer versions (Gram / moment caches), NCC's template scalars and moments */
	touch_all(b); b->lz.it_epoch = -1;
	/* reinitialize(): the initialize* functions called again refresh what depends on the template only (NCC: mean and norm of I0,
	 * NCC.cc:50-95; SSD: nothing; initializeGrad / initializeHess hold no template state for SSD and NCC) */
	if (b->init_sim) TRY(mtfhip_am_initialize_similarity(b));
	if (b->desc.am == MTFHIP_AM_NCC && b->d_ncc_tm && b->j0_is_template) TRY(ncc_template_moments(b));
	return MTFHIP_OK;
}
int do_update_pix_vals(mtfhip_batch *b, const double *pts) {
	TRY(need_image(b));
	TRY(protect_stale(b, false, false));   /* IT is about to change: gradients skipped by a fused launch keep the old IT */
	const double *dp;
	TRY(resolve_pts(b, pts, MTFHIP_BUF_CURR_PTS, 2 * (size_t)b->NP, &dp));
	const int mapped = imap_update_pix_vals(b, dp);   /* RSCV / LRSCV::updatePixVals: It = map(It_orig) (RSCV.cc:170-238, LRSCV.cc:224-261) */
	if (mapped == IMAP_NOT_MINE) {
		TimedScope ts(b->ctx, "sample");
		launch_sample(b->view(), b->ctx->img, dp, b->buf[MTFHIP_BUF_IT], b->norm_mult, b->norm_add, b->ctx->stream);
	} else TRY(mapped);
	touch(b, MTFHIP_BUF_IT);
	b->lz.it_epoch = pts ? -1 : b->lz.epoch;
	b->it_valid = true;
	return MTFHIP_OK;
}
int mtfhip_am_update_pix_vals(mtfhip_batch *b, const double *pts) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "update_pix_vals: NULL batch");
	if (b->lz.enabled && !pts && b->init_pix_vals && b->have_corners && b->ctx->img.data && b->ctx->img.channels == 1) {
		if (b->lz.pv || b->lz.sim) FLUSH(b);
		b->lz.pv = ++b->lz.seq;
		b->it_valid = true;
		return MTFHIP_OK;
	}
	FLUSH(b);
	return do_update_pix_vals(b, pts);
}
int pix_grad_common(mtfhip_batch *b, const double *pts, bool warped, bool init) {
	TRY(need_image(b));
	const double *dp;
	if (warped) TRY(resolve_pts(b, pts, MTFHIP_BUF_GRAD_PTS, 8 * (size_t)b->NP, &dp));
	else TRY(resolve_pts(b, pts, MTFHIP_BUF_CURR_PTS, 2 * (size_t)b->NP, &dp));
	double *dst = b->buf[init ? MTFHIP_BUF_DI0_DX : MTFHIP_BUF_DIT_DX];
	{
		TimedScope ts(b->ctx, warped ? "warped_img_grad" : "img_grad");
		if (warped) launch_warped_img_grad(b->view(), b->ctx->img, dp, dst, b->desc.grad_eps, b->norm_mult, b->ctx->stream);
		else launch_img_grad(b->view(), b->ctx->img, dp, dst, b->desc.grad_eps, b->norm_mult, b->ctx->stream);
	}
	touch(b, init ? MTFHIP_BUF_DI0_DX : MTFHIP_BUF_DIT_DX);
	if (init) b->j0_is_template = false;
	if (init && !b->init_pix_grad) {
		HIP_TRY(hipMemcpyAsync(b->buf[MTFHIP_BUF_DIT_DX], b->buf[MTFHIP_BUF_DI0_DX], sizeof(double) * 2 * b->N * b->B, hipMemcpyDeviceToDevice, b->ctx->stream));
		b->init_pix_grad = true;
		b->dit_valid = true;
	}
	if (!init) b->dit_valid = true;
	return MTFHIP_OK;
}
int mtfhip_am_initialize_pix_grad(mtfhip_batch *b, const double *pts) {
	FLUSH(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "initialize_pix_grad: NULL batch");
	return pix_grad_common(b, pts, false, true);
}
static int lazy_record_pix_grad(mtfhip_batch *b, int kind) {
	if (b->lz.pg || b->lz.pj) FLUSH(b);
	b->lz.pg = ++b->lz.seq; b->lz.pg_kind = kind;
	b->dit_valid = true;
	return MTFHIP_OK;
}
int mtfhip_am_update_pix_grad(mtfhip_batch *b, const double *pts) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "update_pix_grad: NULL batch");
	if (b->lz.enabled && !pts && b->have_corners && b->ctx->img.data && b->ctx->img.channels == 1)
		return lazy_record_pix_grad(b, 1);
	FLUSH(b);
	return pix_grad_common(b, pts, false, false);
}
int mtfhip_am_initialize_pix_grad_warped(mtfhip_batch *b, const double *gp) {
	FLUSH(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "initialize_pix_grad_warped: NULL batch");
	return pix_grad_common(b, gp, true, true);
}
int mtfhip_am_update_pix_grad_warped(mtfhip_batch *b, const double *gp) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "update_pix_grad_warped: NULL batch");
	/* only after a deferred update_grad_pts: the fused kernel derives the warped gradient points from the current warp */
	if (b->lz.enabled && !gp && b->lz.gp && b->ctx->img.data && b->ctx->img.channels == 1)
		return lazy_record_pix_grad(b, 2);
	FLUSH(b);
	return pix_grad_common(b, gp, true, false);
}

/* ------------------------------------------------------------------ AppearanceModel */
static int am_supported(mtfhip_batch *b, const char *fn) {
	if (b->desc.am >= 0 && b->desc.am < (int)(sizeof(kAmTraits) / sizeof(kAmTraits[0]))) return MTFHIP_OK;   /* (every model with a row of traits) */
	return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s :: appearance model %d is not available on the device path yet", fn, b->desc.am);
}

int mtfhip_am_initialize_similarity(mtfhip_batch *b) {
	FLUSH(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "initialize_similarity: NULL batch");
	TRY(am_supported(b, "initializeSimilarity"));
	/* (a model's own reads init_sim: what a second call refreshes is the model's) */
	if (const auto op = am_ops(b).initialize_similarity) TRY(op(b));
	else if (!b->init_sim) {
		HIP_TRY(hipMemsetAsync(b->buf[MTFHIP_BUF_DF_DI0], 0, sizeof(double) * b->N * b->B, b->ctx->stream));
		for (auto &h : b->th) h.f = 0;
	}
	b->init_sim = true;
	return MTFHIP_OK;
}
/* NCC, SPSS and SSIM::initializeGrad (NCC.cc:97-122, SPSS.cc:104-114, SSIM.cc:78-96): the gradient vectors start at zero */
int zero_grad_vectors(mtfhip_batch *b) {
	HIP_TRY(hipMemsetAsync(b->buf[MTFHIP_BUF_DF_DI0], 0, sizeof(double) * b->N * b->B, b->ctx->stream));
	HIP_TRY(hipMemsetAsync(b->buf[MTFHIP_BUF_DF_DIT], 0, sizeof(double) * b->N * b->B, b->ctx->stream));
	return MTFHIP_OK;
}
int mtfhip_am_initialize_grad(mtfhip_batch *b) {
	FLUSH(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "initialize_grad: NULL batch");
	TRY(am_supported(b, "initializeGrad"));
	if (!b->init_grad) {
		if (const auto op = am_ops(b).grad) TRY(op(b, 2));
		else HIP_TRY(hipMemcpyAsync(b->buf[MTFHIP_BUF_DF_DIT], b->buf[MTFHIP_BUF_DF_DI0], sizeof(double) * b->N * b->B, hipMemcpyDeviceToDevice, b->ctx->stream));
	}
	b->init_grad = true;
	return MTFHIP_OK;
}
int mtfhip_am_initialize_hess(mtfhip_batch *b) {
	FLUSH(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "initialize_hess: NULL batch");
	return am_supported(b, "initializeHess");
}
int mtfhip_am_update_similarity(mtfhip_batch *b, int prereq_only) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "update_similarity: NULL batch");
	TRY(am_supported(b, "updateSimilarity"));
	if (!b->init_sim) return fail(MTFHIP_ERR_LOGIC, "updateSimilarity before initializeSimilarity");
	if (b->lz.enabled && b->lz.pv) {   /* only behind a deferred updatePixVals: otherwise nothing to fuse with */
		if (b->lz.sim || b->lz.cg) FLUSH(b);
		if (b->lz.pv) {
			b->lz.sim = ++b->lz.seq; b->lz.sim_need_f = !prereq_only;
			return MTFHIP_OK;
		}
	}
	FLUSH(b);
	return do_update_similarity(b, prereq_only);
}
int do_update_similarity(mtfhip_batch *b, int prereq_only) {
	if (const auto op = am_ops(b).update_similarity) return op(b, prereq_only);
	/* SCV / LSCV::updateSimilarity (SCV.cc:194-230, LSCV.cc:263-304): the intensity map(s) from It and I0_orig, I0 re-mapped, then
	 * SSDBase::updateSimilarity */
	TRY(imap_before_pass(b, nullptr, 0, nullptr, nullptr, 1, b->first_iter != 0, b->ctx->stream, nullptr));
	int nblk = simple_blocks_per_target(b->N);
	{
		TimedScope ts(b->ctx, "ssd_residual");
		launch_ssd_residual(b->view(), b->d_partials, nblk, b->ctx->stream);
	}
	stale_clear(b, true, false);
	b->lz.df0_it_ver = b->lz.ver[MTFHIP_BUF_IT];
	if (prereq_only) return MTFHIP_OK;
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t) b->th[t].f = -b->h_acc[(size_t)t * ACC_COUNT + ACC_RR] / 2;
	return MTFHIP_OK;
}
int do_update_curr_grad(mtfhip_batch *b) {
	if (const auto op = am_ops(b).grad) return op(b, 1);
	if (b->lz.df0_stale) TRY(ensure_one(b, false));
	TimedScope ts(b->ctx, "negate");
	launch_negate(b->buf[MTFHIP_BUF_DF_DI0], b->buf[MTFHIP_BUF_DF_DIT], (size_t)b->N * b->B, b->ctx->stream);
	stale_clear(b, false, true);
	return MTFHIP_OK;
}
int mtfhip_am_update_curr_grad(mtfhip_batch *b) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "update_curr_grad: NULL batch");
	TRY(am_supported(b, "updateCurrGrad"));
	if (b->lz.enabled) {
		if (b->lz.cg) FLUSH(b);
		b->lz.cg = ++b->lz.seq;
		return MTFHIP_OK;
	}
	FLUSH(b);
	return do_update_curr_grad(b);
}
int mtfhip_am_update_init_grad(mtfhip_batch *b) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "update_init_grad: NULL batch");
	TRY(am_supported(b, "updateInitGrad"));
	if (ssd_like(b)) return MTFHIP_OK;   /* SSD::updateInitGrad is empty: df_dI0 is updateSimilarity's residual */
	if (b->lz.enabled) {   /* NCC */
		if (b->lz.ig) FLUSH(b);
		b->lz.ig = ++b->lz.seq;
		return MTFHIP_OK;
	}
	FLUSH(b);
	if (const auto op = am_ops(b).grad) return op(b, 0);
	return MTFHIP_OK;
}
int mtfhip_am_get_similarity(mtfhip_batch *b, double *f) {
	if (!b || !f) return fail(MTFHIP_ERR_INVALID_ARG, "get_similarity: NULL argument");
	TRY(lazy_try_similarity(b));
	FLUSH_AM(b);
	for (int t = 0; t < b->B; ++t) f[t] = b->th[t].f;
	return MTFHIP_OK;
}
int mtfhip_am_get_likelihood(mtfhip_batch *b, double *l) {
	if (!b || !l) return fail(MTFHIP_ERR_INVALID_ARG, "get_likelihood: NULL argument");
	TRY(lazy_try_similarity(b));
	FLUSH_AM(b);
	const auto op = am_ops(b).likelihood;
	for (int t = 0; t < b->B; ++t) {
		if (op) TRY(op(b, t, &l[t]));
		else l[t] = std::exp(-b->desc.likelihood_alpha * std::sqrt(-b->th[t].f / (double)b->N));   /* SSD::getLikelihood SSD.h:41-43 */
	}
	return MTFHIP_OK;
}

int gemv_to_host(mtfhip_batch *b, const double *v1, int j1, const double *v2, int j2, int sum_mode, double *g, int diff) {
	int nblk = simple_blocks_per_target(b->N);
	{
		TimedScope ts(b->ctx, "gemv");
		launch_gemv(b->view(), v1, b->buf[j1], v2, j2 >= 0 ? b->buf[j2] : nullptr, sum_mode, b->d_partials, nblk, b->ctx->stream);
	}
	TRY(read_acc(b, nblk));
	for (int t = 0; t < b->B; ++t)
		for (int s = 0; s < b->S; ++s) {
			double v = b->h_acc[(size_t)t * ACC_COUNT + ACC_G + s];
			if (diff) v -= b->h_acc[(size_t)t * ACC_COUNT + ACC_G2 + s];
			g[(size_t)t * b->S + s] = v;
		}
	return MTFHIP_OK;
}
static int j_ready(mtfhip_batch *b, int id, const char *fn) {
	if (!j_buf_ok(id)) return fail(MTFHIP_ERR_INVALID_ARG, "%s: Jacobian buffer id %d is not J0/JT/JM", fn, id);
	if (!b->buf[id]) return fail(MTFHIP_ERR_LOGIC, "%s: Jacobian buffer %d was never produced", fn, id);
	if (id == MTFHIP_BUF_JT && !b->jt_valid) return fail(MTFHIP_ERR_LOGIC, "%s: JT is not materialised", fn);
	return MTFHIP_OK;
}
int mtfhip_am_cmpt_init_jacobian(mtfhip_batch *b, int j0_buf, double *g) {
	if (!b || !g) return fail(MTFHIP_ERR_INVALID_ARG, "cmpt_init_jacobian: NULL argument");
	TRY(am_supported(b, "cmptInitJacobian"));
	TRY(j_ready(b, j0_buf, "cmptInitJacobian"));
	{ int done; TRY(lazy_try_fused(b, LAZY_INIT_JAC, j0_buf, -1, g, &done)); if (done) return MTFHIP_OK; }
	FLUSH_AM(b);
	TRY(ensure_df(b));
	return gemv_to_host(b, b->buf[MTFHIP_BUF_DF_DI0], j0_buf, nullptr, -1, 0, g, 0);
}
int mtfhip_am_cmpt_curr_jacobian(mtfhip_batch *b, int jt_buf, double *g) {
	if (!b || !g) return fail(MTFHIP_ERR_INVALID_ARG, "cmpt_curr_jacobian: NULL argument");
	TRY(am_supported(b, "cmptCurrJacobian"));
	TRY(j_ready(b, jt_buf, "cmptCurrJacobian"));
	{ int done; TRY(lazy_try_fused(b, LAZY_CURR_JAC, jt_buf, -1, g, &done)); if (done) return MTFHIP_OK; }
	FLUSH_AM(b);
	TRY(ensure_df(b));
	return gemv_to_host(b, b->buf[MTFHIP_BUF_DF_DIT], jt_buf, nullptr, -1, 0, g, 0);
}
int mtfhip_am_cmpt_difference_of_jacobians(mtfhip_batch *b, int j0_buf, int jt_buf, double *g) {
	if (!b || !g) return fail(MTFHIP_ERR_INVALID_ARG, "cmpt_difference_of_jacobians: NULL argument");
	TRY(am_supported(b, "cmptDifferenceOfJacobians"));
	TRY(j_ready(b, j0_buf, "cmptDifferenceOfJacobians"));
	TRY(j_ready(b, jt_buf, "cmptDifferenceOfJacobians"));
	{ int done; TRY(lazy_try_fused(b, LAZY_DIFF_JAC, j0_buf, jt_buf, g, &done)); if (done) return MTFHIP_OK; }
	FLUSH_AM(b);
	TRY(ensure_df(b));
	if (!ssd_like(b)) /* (df_dIt * dIt_dp) - (df_dI0 * dI0_dp), NCC.cc:268-280, AppearanceModel.h:161-164 */
		return gemv_to_host(b, b->buf[MTFHIP_BUF_DF_DIT], jt_buf, b->buf[MTFHIP_BUF_DF_DI0], j0_buf, 0, g, 1);
	/* SSD: df_dIt * (dI0_dpssm + dIt_dpssm), SSDBase.cc:186 */
	return gemv_to_host(b, b->buf[MTFHIP_BUF_DF_DIT], jt_buf, nullptr, j0_buf, 1, g, 0);
}
/* J^T J of a pixel Jacobian, from the host-side copy when the buffer has not been written since that copy was made
 * (the fused launch of this iteration accumulated it; the template's J0 only changes with the template) */
static int gram_to_host(mtfhip_batch *b, int j_buf, double *H, double scale, bool accumulate) {
	mtfhip_batch::Lazy &L = b->lz;
	const double *src = nullptr;
	if (!L.no_cache) {
		if (j_buf == L.gram_buf && L.gram_ver == L.ver[j_buf] && !L.gram.empty()) src = L.gram.data();
		else if (j_buf == MTFHIP_BUF_J0 && L.gram0_ver == L.ver[j_buf] && !L.gram0.empty()) src = L.gram0.data();
	}
	if (!src) {
		int nblk = simple_blocks_per_target(b->N);
		{
			TimedScope ts(b->ctx, "gram");
			launch_gram(b->view(), b->buf[j_buf], b->d_partials, nblk, b->ctx->stream);
		}
		TRY(read_acc(b, nblk));
		std::vector<double> &dst = j_buf == MTFHIP_BUF_J0 ? L.gram0 : L.gram;
		dst.resize((size_t)36 * b->B);
		for (int t = 0; t < b->B; ++t) std::memcpy(&dst[(size_t)36 * t], b->h_acc + (size_t)t * ACC_COUNT + ACC_H, sizeof(double) * 36);
		if (j_buf == MTFHIP_BUF_J0) L.gram0_ver = L.ver[j_buf];
		else { L.gram_buf = j_buf; L.gram_ver = L.ver[j_buf]; }
		src = dst.data();
	}
	const int S = b->S;
	for (int t = 0; t < b->B; ++t) {
		int k = 0;
		for (int a = 0; a < 8; ++a)
			for (int c = a; c < 8; ++c) {
				if (a < S && c < S) {
					double v = scale * src[(size_t)36 * t + k];
					double *Ht = H + (size_t)t * S * S;
					if (accumulate) { Ht[c * S + a] += v; if (a != c) Ht[a * S + c] += v; }
					else { Ht[c * S + a] = v; Ht[a * S + c] = v; }
				}
				++k;
			}
	}
	return MTFHIP_OK;
}
/* cmptInitHessian / cmptCurrHessian / cmptSelfHessian (kind 0 / 1 / 2) of the Jacobian in j_buf; fn, ref: the entry point's and the reference's name */
static int cmpt_hessian(mtfhip_batch *b, int j_buf, int kind, double *H, const char *fn, const char *ref) {
	FLUSH_AM(b);
	if (!b || !H) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);
	TRY(am_supported(b, ref));
	TRY(j_ready(b, j_buf, ref));
	if (const auto op = am_ops(b).hessian) return op(b, j_buf, kind, H);
	return gram_to_host(b, j_buf, H, -1.0, false);
}
int mtfhip_am_cmpt_init_hessian(mtfhip_batch *b, int j0_buf, double *H) { return cmpt_hessian(b, j0_buf, 0, H, "cmpt_init_hessian", "cmptInitHessian"); }
int mtfhip_am_cmpt_curr_hessian(mtfhip_batch *b, int jt_buf, double *H) { return cmpt_hessian(b, jt_buf, 1, H, "cmpt_curr_hessian", "cmptCurrHessian"); }
int mtfhip_am_cmpt_self_hessian(mtfhip_batch *b, int jt_buf, double *H) { return cmpt_hessian(b, jt_buf, 2, H, "cmpt_self_hessian", "cmptSelfHessian"); }
int mtfhip_am_cmpt_sum_of_hessians(mtfhip_batch *b, int j0_buf, int jt_buf, double *H) {
	FLUSH_AM(b);
	if (!b || !H) return fail(MTFHIP_ERR_INVALID_ARG, "cmpt_sum_of_hessians: NULL argument");
	TRY(am_supported(b, "cmptSumOfHessians"));
	TRY(j_ready(b, j0_buf, "cmptSumOfHessians"));
	TRY(j_ready(b, jt_buf, "cmptSumOfHessians"));
	if (const auto op = am_ops(b).hessian) {
		/* generic AppearanceModel::cmptSumOfHessians AppearanceModel.h:196-208 */
		std::vector<double> H0((size_t)b->B * b->S * b->S);
		TRY(op(b, j0_buf, 0, H0.data()));
		TRY(op(b, jt_buf, 1, H));
		for (size_t i = 0; i < H0.size(); ++i) H[i] += H0[i];
		return MTFHIP_OK;
	}
	TRY(gram_to_host(b, j0_buf, H, -1.0, false));
	return gram_to_host(b, jt_buf, H, -1.0, true);
}
int do_mean_jacobian(mtfhip_batch *b) {
	TRY(ensure_buf(b, MTFHIP_BUF_JM));
	TimedScope ts(b->ctx, "mean_jacobian");
	launch_mean_jacobian(b->view(), b->ctx->stream);
	touch(b, MTFHIP_BUF_JM);
	return MTFHIP_OK;
}
int mtfhip_sm_mean_jacobian(mtfhip_batch *b) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "mean_jacobian: NULL batch");
	TRY(j_ready(b, MTFHIP_BUF_J0, "mean_jacobian"));
	TRY(j_ready(b, MTFHIP_BUF_JT, "mean_jacobian"));
	if (b->lz.enabled && b->lz.pj) {
		if (b->lz.jm) FLUSH(b);
		if (b->lz.pj) { TRY(ensure_buf(b, MTFHIP_BUF_JM)); b->lz.jm = ++b->lz.seq; return MTFHIP_OK; }
	}
	FLUSH(b);
	return do_mean_jacobian(b);
}

/* ------------------------------------------------------------------ second order (sec_ord_hess) */
static int hess_buf_ok(int id) { return id == MTFHIP_BUF_D2I0_DX2 || id == MTFHIP_BUF_D2IT_DX2; }
static int d2_buf_ok(int id) { return id == MTFHIP_BUF_D2I0_DP2 || id == MTFHIP_BUF_D2IT_DP2 || id == MTFHIP_BUF_D2IM_DP2; }

int mtfhip_ssm_update_hess_pts(mtfhip_batch *b, double hess_eps) {
	FLUSH(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "update_hess_pts: NULL batch");
	TRY(lowdof_refuse(b, "update_hess_pts"));
	if (!b->have_corners) return fail(MTFHIP_ERR_LOGIC, "update_hess_pts before set_corners");
	TRY(ensure_buf(b, MTFHIP_BUF_HESS_PTS));
	TimedScope ts(b->ctx, "hess_pts");
	launch_hess_pts(b->view(), hess_eps, b->ctx->stream);
	return MTFHIP_OK;
}

/* ImageBase::initializePixHess / updatePixHess, both overloads (AM/src/ImageBase.cc:174-240, 316-338, 364-386) */
static int pix_hess_common(mtfhip_batch *b, const double *pts, const double *hess_pts, bool warped, bool init) {
	TRY(need_image(b));
	TRY(ensure_buf(b, MTFHIP_BUF_D2I0_DX2));
	TRY(ensure_buf(b, MTFHIP_BUF_D2IT_DX2));
	const size_t N = b->N, NP = b->NP;
	const double *dp, *dh = nullptr;
	TRY(resolve_pts(b, pts, MTFHIP_BUF_CURR_PTS, 2 * NP, &dp));
	if (warped) {
		if (!hess_pts) {
			if (!b->buf[MTFHIP_BUF_HESS_PTS]) return fail(MTFHIP_ERR_LOGIC, "pix_hess: device hess_pts not available (call update_hess_pts)");
			dh = b->buf[MTFHIP_BUF_HESS_PTS];
		} else {
			double *stage = b->d_scratch_pts + 2 * NP * b->B;
			HIP_TRY(hipMemcpyAsync(stage, hess_pts, sizeof(double) * 16 * NP * b->B, hipMemcpyHostToDevice, b->ctx->stream));
			dh = stage;
		}
	}
	double *dst = b->buf[init ? MTFHIP_BUF_D2I0_DX2 : MTFHIP_BUF_D2IT_DX2];
	{
		TimedScope ts(b->ctx, warped ? "warped_img_hess" : "img_hess");
		if (warped) launch_warped_img_hess(b->view(), b->ctx->img, dp, dh, dst, b->hess_eps, b->norm_mult, b->ctx->stream);
		else launch_img_hess(b->view(), b->ctx->img, dp, dst, b->hess_eps, b->norm_mult, b->ctx->stream);
	}
	if (init && !b->init_pix_hess) {
		HIP_TRY(hipMemcpyAsync(b->buf[MTFHIP_BUF_D2IT_DX2], b->buf[MTFHIP_BUF_D2I0_DX2], sizeof(double) * 4 * N * b->B, hipMemcpyDeviceToDevice, b->ctx->stream));
		b->init_pix_hess = true;
	}
	return MTFHIP_OK;
}
int mtfhip_am_initialize_pix_hess(mtfhip_batch *b, const double *pts) {
	FLUSH(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "initialize_pix_hess: NULL batch");
	TRY(lowdof_refuse(b, "initialize_pix_hess"));
	return pix_hess_common(b, pts, nullptr, false, true);
}
int mtfhip_am_update_pix_hess(mtfhip_batch *b, const double *pts) {
	FLUSH(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "update_pix_hess: NULL batch");
	TRY(lowdof_refuse(b, "update_pix_hess"));
	return pix_hess_common(b, pts, nullptr, false, false);
}
int mtfhip_am_initialize_pix_hess_warped(mtfhip_batch *b, const double *pts, const double *hess_pts) {
	FLUSH(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "initialize_pix_hess_warped: NULL batch");
	TRY(lowdof_refuse(b, "initialize_pix_hess_warped"));
	return pix_hess_common(b, pts, hess_pts, true, true);
}
int mtfhip_am_update_pix_hess_warped(mtfhip_batch *b, const double *pts, const double *hess_pts) {
	FLUSH(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "update_pix_hess_warped: NULL batch");
	TRY(lowdof_refuse(b, "update_pix_hess_warped"));
	return pix_hess_common(b, pts, hess_pts, true, false);
}

int mtfhip_ssm_cmpt_pix_hessian(mtfhip_batch *b, int variant, int hess_buf, int grad_buf, int dst_buf) {
	FLUSH(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "cmpt_pix_hessian: NULL batch");
	TRY(lowdof_refuse(b, "cmpt_pix_hessian"));
	if (variant < MTFHIP_JAC_INIT || variant > MTFHIP_JAC_APPROX) return fail(MTFHIP_ERR_INVALID_ARG, "unknown pixel Hessian variant %d", variant);
	if (!hess_buf_ok(hess_buf)) return fail(MTFHIP_ERR_INVALID_ARG, "hess_buf must be D2I0_DX2 or D2IT_DX2");
	if (grad_buf != MTFHIP_BUF_DI0_DX && grad_buf != MTFHIP_BUF_DIT_DX) return fail(MTFHIP_ERR_INVALID_ARG, "grad_buf must be DI0_DX or DIT_DX");
	if (!d2_buf_ok(dst_buf)) return fail(MTFHIP_ERR_INVALID_ARG, "dst_buf must be D2I0_DP2, D2IT_DP2 or D2IM_DP2");
	/* Affine implements Init and Warped only (SSM/include/mtf/SSM/Affine.h); the others are ssm_func_not_implemeted
	 * (StateSpaceModel.h:186-197) */
	if (b->desc.ssm == MTFHIP_SSM_AFFINE && (variant == MTFHIP_JAC_PIX || variant == MTFHIP_JAC_APPROX))
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s :: function not implemented yet", variant == MTFHIP_JAC_PIX ? "cmptPixHessian" : "cmptApproxPixHessian");
	if (!b->have_corners) return fail(MTFHIP_ERR_LOGIC, "cmpt_pix_hessian before set_corners");
	if (!b->buf[hess_buf]) return fail(MTFHIP_ERR_LOGIC, "cmpt_pix_hessian: image Hessian %d was never computed", hess_buf);
	TRY(ensure_buf(b, dst_buf));
	TimedScope ts(b->ctx, "pix_hessian");
	launch_pix_hessian(b->view(), variant, b->buf[hess_buf], b->buf[grad_buf], b->buf[dst_buf], b->ctx->stream);
	return MTFHIP_OK;
}

int mtfhip_sm_mean_pix_hessian(mtfhip_batch *b) {
	FLUSH_AM(b);
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "mean_pix_hessian: NULL batch");
	TRY(lowdof_refuse(b, "mean_pix_hessian"));
	if (!b->buf[MTFHIP_BUF_D2I0_DP2] || !b->buf[MTFHIP_BUF_D2IT_DP2]) return fail(MTFHIP_ERR_LOGIC, "mean_pix_hessian: init / curr pixel Hessians not computed");
	TRY(ensure_buf(b, MTFHIP_BUF_D2IM_DP2));
	TimedScope ts(b->ctx, "mean_pix_hessian");
	launch_mean_planes(b->buf[MTFHIP_BUF_D2I0_DP2], b->buf[MTFHIP_BUF_D2IT_DP2], b->buf[MTFHIP_BUF_D2IM_DP2],
		(size_t)b->B * b->N * b->S * b->S, b->ctx->stream);
	return MTFHIP_OK;
}

/* H[t] += sum_p w[p] * (d2a[:, p] (+ d2b[:, p])) */
static int add_second_order(mtfhip_batch *b, int d2a, int d2b, const double *dev_w, double *H) {
	if (!d2_buf_ok(d2a) || (d2b >= 0 && !d2_buf_ok(d2b))) return fail(MTFHIP_ERR_INVALID_ARG, "pixel-Hessian buffer must be D2I0_DP2, D2IT_DP2 or D2IM_DP2");
	if (!b->buf[d2a] || (d2b >= 0 && !b->buf[d2b])) return fail(MTFHIP_ERR_LOGIC, "second-order Hessian: pixel Hessian buffer was never computed");
	const int nblk = simple_blocks_per_target(b->N), S = b->S;
	TRY(ensure_second_order_scratch(b));
	{
		TimedScope ts(b->ctx, "pix_hess_weighted_sum");
		launch_weighted_plane_sum(b->view(), b->buf[d2a], d2b >= 0 ? b->buf[d2b] : nullptr, dev_w, b->d_d2_part, nblk, b->d_d2_out, b->ctx->stream);
	}
	std::vector<double> h((size_t)S * S * b->B);
	HIP_TRY(hipMemcpyAsync(h.data(), b->d_d2_out, sizeof(double) * h.size(), hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	for (size_t i = 0; i < h.size(); ++i) H[i] += h[i];
	return MTFHIP_OK;
}
/* SSDBase.cc:313-343 ; NCC.cc:391-400 ; MI.cc:659-673 */
int mtfhip_am_cmpt_init_hessian2(mtfhip_batch *b, int j0_buf, int d2_buf, double *H) {
	FLUSH_AM(b);
	TRY(am_refuse(b, "cmpt_init_hessian (second order)", AM_AT_SEC_ORD_HESS));
	TRY(lowdof_refuse(b, "cmpt_init_hessian (second order)"));
	if (b) TRY(ensure_df(b));   /* the second-order terms are weighted by df_dI */
	TRY(mtfhip_am_cmpt_init_hessian(b, j0_buf, H));
	return add_second_order(b, d2_buf, -1, b->buf[MTFHIP_BUF_DF_DI0], H);
}
/* SSDBase.cc:345-375 ; NCC.cc:401-410 ; MI.cc:680-694 */
int mtfhip_am_cmpt_curr_hessian2(mtfhip_batch *b, int jt_buf, int d2_buf, double *H) {
	FLUSH_AM(b);
	TRY(am_refuse(b, "cmpt_curr_hessian (second order)", AM_AT_SEC_ORD_HESS));
	TRY(lowdof_refuse(b, "cmpt_curr_hessian (second order)"));
	if (b) TRY(ensure_df(b));   /* the second-order terms are weighted by df_dI */
	TRY(mtfhip_am_cmpt_curr_hessian(b, jt_buf, H));
	return add_second_order(b, d2_buf, -1, b->buf[MTFHIP_BUF_DF_DIT], H);
}
/* SSD: first order only (SSDBase.h:95-98) ; NCC: am_func_not_implemeted (AppearanceModel.h:188-191) ; MI.cc:696-733 */
int mtfhip_am_cmpt_self_hessian2(mtfhip_batch *b, int jt_buf, int d2_buf, double *H) {
	FLUSH_AM(b);
	TRY(am_refuse(b, "cmpt_self_hessian (second order)", AM_AT_SEC_ORD_HESS));
	TRY(lowdof_refuse(b, "cmpt_self_hessian (second order)"));
	if (b) TRY(ensure_df(b));   /* the second-order terms are weighted by df_dI */
	if (!b || !H) return fail(MTFHIP_ERR_INVALID_ARG, "cmpt_self_hessian (second order): NULL argument");
	if (b->desc.am == MTFHIP_AM_NCC) return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "ncc :: cmptSelfHessian(second order) :: function not implemented yet");
	TRY(mtfhip_am_cmpt_self_hessian(b, jt_buf, H));
	if (b->desc.am == MTFHIP_AM_SSD) return MTFHIP_OK;
	TRY(mi_self_weight(b));   /* MI: the self table was filled by the first-order call above */
	return add_second_order(b, d2_buf, -1, b->d_d2_w, H);
}
/* SSDBase.cc:377-415 (both pixel Hessians weighted by df_dI0) ; NCC / MI: generic AppearanceModel.h:209-219 */
int mtfhip_am_cmpt_sum_of_hessians2(mtfhip_batch *b, int j0_buf, int jt_buf, int d20_buf, int d2t_buf, double *H) {
	FLUSH_AM(b);
	TRY(am_refuse(b, "cmpt_sum_of_hessians (second order)", AM_AT_SEC_ORD_HESS));
	TRY(lowdof_refuse(b, "cmpt_sum_of_hessians (second order)"));
	if (b) TRY(ensure_df(b));   /* the second-order terms are weighted by df_dI */
	if (!b || !H) return fail(MTFHIP_ERR_INVALID_ARG, "cmpt_sum_of_hessians (second order): NULL argument");
	if (b->desc.am == MTFHIP_AM_SSD) {
		TRY(mtfhip_am_cmpt_sum_of_hessians(b, j0_buf, jt_buf, H));
		return add_second_order(b, d20_buf, d2t_buf, b->buf[MTFHIP_BUF_DF_DI0], H);
	}
	std::vector<double> H0((size_t)b->B * b->S * b->S);
	TRY(mtfhip_am_cmpt_init_hessian2(b, j0_buf, d20_buf, H0.data()));
	TRY(mtfhip_am_cmpt_curr_hessian2(b, jt_buf, d2t_buf, H));
	for (size_t i = 0; i < H0.size(); ++i) H[i] += H0[i];
	return MTFHIP_OK;
}


} /* extern "C" */
