/*
 * api_fused.hip -- the fused path: what a search method may ask of it (check_sm), template initialisation and set_region, the arguments of a fused
 * launch, one iteration for a host-side solve (mtfhip_batch_iterate) and the lean similarity of the deferred-fusion layer
 * (C-ABI implementation, include/mtfhip.h; shared declarations: mtfhip_api_internal.h)
 *
 * No CPU fallback exists: every entry point either runs its HIP kernels or returns an error.
 */
#include "mtfhip_api_internal.h"

extern "C" {

/* ------------------------------------------------------------------ fused path */
int check_sm(const mtfhip_batch *b, const mtfhip_sm_desc *sm, const char *fn) {
	if (!b || !sm) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);
	/* the additive methods live behind init_template / iterate / track alone (api_alk.hip): what else comes here with them -- set_region,
	 * track_region, the grid tracker's frames -- is refused */
	if (alk_sm(sm->sm))
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: the additive search methods (FALK / IALK) are served by init_template / iterate / track only (set_region, track_region "
			"and the grid frames are not available with them)", fn);
	if (sm->sm < MTFHIP_SM_ESM || sm->sm > MTFHIP_SM_ICLK) return fail(MTFHIP_ERR_INVALID_ARG, "%s: unknown search method %d", fn, sm->sm);
	int max_h = sm->sm == MTFHIP_SM_ESM ? 5 : 2;
	if (sm->hess_type < 0 || sm->hess_type > max_h) return fail(MTFHIP_ERR_INVALID_ARG, "%s: hess_type %d invalid for search method %d", fn, sm->hess_type, sm->sm);
	/* the low-order SSMs: first-order Hessians (their pixel Hessians are not available: mtfhip_ssm_cmpt_pix_hessian) */
	if (b->lo_ssm && sm->sec_ord_hess)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: sec_ord_hess is not available with the %s state space model (first-order Hessians only)", fn, ssm_name(b->lo_ssm));
	if (b->desc.am == MTFHIP_AM_NCC) {
		/* NCC overrides the second-order cmptInit / CurrHessian (NCC.cc:391-410) but not cmptSelfHessian: the self types throw
		 * FunctonNotImplemented in the reference (AppearanceModel.h:188-191) */
		if (sm->sec_ord_hess && !(sm->sm == MTFHIP_SM_ESM ? sm->hess_type >= 3 : sm->hess_type == 2))
			return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: NCC has no second-order self Hessian (AppearanceModel.h:188-191)", fn);
		return MTFHIP_OK;
	}
	if (b->desc.am == MTFHIP_AM_MI) {
		/* fused MI iteration: every first-order Jacobian / Hessian type of the three search methods; with sec_ord_hess the Std types
		 * (MI.cc:659-695: cmptInitHessian / cmptCurrHessian + sum_p df_dI(p) d2I_dp2(p)) and the self types (MI.cc:697-735: the
		 * current pixel Hessian under the self gradient factor; the initial self Hessian takes its second-order part at
		 * initialize / setRegion).  Eight bins (the weights are read from the 8-bin gradient-factor tables). */
		return MTFHIP_OK;
	}
	/* Second-order Hessians of SPSS, SSIM, CCRE and the SCV family: CCRE's forms (CCRE.cc:797-865) weight the pixel Hessian by gradients no
	 * pass of this path hands on, SSIM's by df_dI (SSIM.cc:187-198, 256-268), which no pass accumulates for it; SCV is SSD on the re-mapped
	 * template, first order.  First order: CCRE has every type MI's materialising iteration serves (SumOfStd as two Hessian passes), SSIM
	 * every type NCC has, from the same rows (ssim_h, mtfhip_sm_system.h) */
	if (sm->sec_ord_hess) TRY(am_refuse(b, fn, AM_AT_SEC_ORD_HESS));
	/* SPSS: the pass fills ONE weighted Gram matrix per row (kernels_fused_spss.hip), and ESM's SumOfStd is the mean of two with different
	 * weights and rows (cmptInitHessian(J0) + cmptCurrHessian(Jt), AppearanceModel.h:194-206) */
	if (spss_am(b) && sm->sm == MTFHIP_SM_ESM && sm->hess_type == 4)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: SPSS with ESM hess_type SumOfStd needs two weighted Gram matrices in one pass and is not available on the fused entry points "
			"(cmpt_sum_of_hessians serves it)" MTFHIP_FIRST_ORDER_SERVED, fn);
	return MTFHIP_OK;   /* (every model mtfhip_batch_create accepts has its row of traits) */
}

/* inverse of a definite S x S matrix (column-major) by Gauss-Jordan on the diagonally scaled system */
static bool invert_definite(int S, const double *H, double *Hinv) {
	double A[8][16], sc[8];
	for (int i = 0; i < S; ++i) { double d = std::fabs(H[i * S + i]); sc[i] = d > 0 ? 1.0 / std::sqrt(d) : 1.0; }
	for (int i = 0; i < S; ++i)
		for (int j = 0; j < S; ++j) { A[i][j] = H[j * S + i] * sc[i] * sc[j]; A[i][S + j] = i == j ? 1.0 : 0.0; }
	for (int k = 0; k < S; ++k) {
		int piv = k;
		for (int i = k + 1; i < S; ++i) if (std::fabs(A[i][k]) > std::fabs(A[piv][k])) piv = i;
		if (A[piv][k] == 0) return false;
		if (piv != k) for (int j = 0; j < 2 * S; ++j) std::swap(A[piv][j], A[k][j]);
		const double p = A[k][k];
		for (int j = 0; j < 2 * S; ++j) A[k][j] /= p;
		for (int i = 0; i < S; ++i) {
			if (i == k) continue;
			const double f = A[i][k];
			if (f == 0) continue;
			for (int j = 0; j < 2 * S; ++j) A[i][j] -= f * A[k][j];
		}
	}
	for (int i = 0; i < S; ++i)
		for (int j = 0; j < S; ++j) Hinv[j * S + i] = A[i][S + j] * sc[i] * sc[j];
	return true;
}

/* th[].h0 <- H0 ([B][S x S], column-major), padded to 8 x 8 for d_h0; d_h0inv <- its inverse (zero for a flat template: no update) or, without,
 * zero.  The copies are only ENQUEUED, from thread-local staging: every caller synchronises the stream before it returns */
int store_h0(mtfhip_batch *b, const double *H0, bool with_inverse) {
	static thread_local std::vector<double> h0dev, hinv;
	const int S2 = b->S * b->S;
	h0dev.assign((size_t)b->B * 64, 0.0);
	for (int t = 0; t < b->B; ++t) {
		std::memset(b->th[t].h0, 0, sizeof(b->th[t].h0));
		std::memcpy(b->th[t].h0, H0 + (size_t)t * S2, sizeof(double) * S2);
		std::memcpy(&h0dev[(size_t)t * 64], b->th[t].h0, sizeof(double) * 64);
	}
	HIP_TRY(hipMemcpyAsync(b->d_h0, h0dev.data(), sizeof(double) * h0dev.size(), hipMemcpyHostToDevice, b->ctx->stream));
	if (!with_inverse) {
		HIP_TRY(hipMemsetAsync(b->d_h0inv, 0, sizeof(double) * 64 * (size_t)b->B, b->ctx->stream));
		return MTFHIP_OK;
	}
	hinv.assign((size_t)b->B * 64, 0.0);
	for (int t = 0; t < b->B; ++t)
		if (!invert_definite(b->S, b->th[t].h0, &hinv[(size_t)t * 64]))
			std::fill(hinv.begin() + (size_t)t * 64, hinv.begin() + (size_t)(t + 1) * 64, 0.0);   /* flat template: no update */
	HIP_TRY(hipMemcpyAsync(b->d_h0inv, hinv.data(), sizeof(double) * hinv.size(), hipMemcpyHostToDevice, b->ctx->stream));
	return MTFHIP_OK;
}

/* the initial self Hessian a search method keeps (NT/ESM.cc:133-141, NT/FCLK.cc:120-128, NT/ICLK.cc:96-118).  MI with sec_ord_hess: its
 * second-order form (MI.cc:697-735) over the template's pixel Hessian, which is materialised for this one call. */
static int init_self_hessian(mtfhip_batch *b, const mtfhip_sm_desc *sm, double *H0) {
	if (b->desc.am == MTFHIP_AM_MI && sm->sec_ord_hess && b->C == 1) {
		TRY(mtfhip_ssm_cmpt_pix_hessian(b, b->d0_variant, MTFHIP_BUF_D2I0_DX2, MTFHIP_BUF_DI0_DX, MTFHIP_BUF_D2I0_DP2));
		return mtfhip_am_cmpt_self_hessian2(b, MTFHIP_BUF_J0, MTFHIP_BUF_D2I0_DP2, H0);
	}
	/* SPSS: the constant Hessian of InitialSelf is cmptSelfHessian at It = I0 (SPSS.cc:91-101, :221-225).  At initialize the It buffer holds I0;
	 * a setRegion that refreshes H0 comes behind a loop whose last pass may or may not have materialised It, so the weight is taken from I0
	 * itself: the same H0 whatever the loop wrote */
	if (spss_am(b)) { FLUSH_AM(b); return spss_weighted_hessian(b, MTFHIP_BUF_J0, SPSS_W_SELF0, H0); }
	/* SSIM: cmptSelfHessian(J0) at It = I0 (SSIM.cc:270-287) is a function of the template's moments (every caller takes them in front: th[].ncc_tm
	 * is current); no pixel pass of its own, and the same H0 whatever a loop left in the It buffer */
	if (ssim_am(b)) return ssim_h0(b, H0);
	return mtfhip_am_cmpt_self_hessian(b, MTFHIP_BUF_J0, H0);
}
/* A low-order SSM's template in affine coordinates (mtfhip_batch::lo_ssm), behind the interface's own N x S Jacobian: the affine rows of dI0_dx
 * at the embedded state -- the six-column J0 the pass reads, J_S = J_aff M -- then, as for an affine batch, the constant self Hessian over
 * them (with_h0) and NCC's template moments.  The finish projects what comes out of these (M^T H M, g M) in front of its solve. */
static int lowdof_template(mtfhip_batch *b, const mtfhip_sm_desc *sm, int variant, bool with_h0) {
	PassMode pm(b);
	TRY(do_cmpt_pix_jacobian(b, variant, MTFHIP_BUF_DI0_DX, MTFHIP_BUF_J0));
	if (ncc_rows(b)) TRY(ncc_template_moments(b));   /* (in front of H0: SSIM's is a function of them) */
	if (with_h0) {
		std::vector<double> H0((size_t)b->B * b->S * b->S);
		TRY(init_self_hessian(b, sm, H0.data()));
		TRY(store_h0(b, H0.data(), true));
		HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	}
	return MTFHIP_OK;
}
/* nt::ICLK::initialize of small single-channel SSD / NCC patches in ONE launch (kernels_init.hip): the grid tracker re-initialises its
 * 256 patch trackers after every frame with the shipped reset_at_each_frame = 1 (GridTracker.cc:273-274, 345-392), and call by call
 * that was 385 us per frame against 42 us for tracking them (r05, tools/grid_modes_probe.py).  Nothing is waited for: the small
 * results the host mirrors hold (H0, NCC scalars, template moments) arrive in a pinned record and are folded in by the next entry
 * point that flushes (pull_init_mirrors).  MTFHIP_INIT_FUSED=0 keeps the call-by-call form (A/B and the equality test). */
bool template_init_fused_ok(const mtfhip_batch *b, const mtfhip_sm_desc *sm) {
	const char *e = std::getenv("MTFHIP_INIT_FUSED");   /* (read per call: the tests flip it) */
	if (e && e[0] == '0') return false;
	if (b->lo_ssm) return false;   /* (k_template_init writes the SSM's own rows and Hessian: the low-order models keep theirs in affine coordinates) */
	const int am = b->desc.am;
	if (am != MTFHIP_AM_SSD && am != MTFHIP_AM_NCC) return false;   /* (SSIM: k_template_init writes NCC's H0, not cmptSelfHessian of SSIM.cc) */
	const bool const_h = sm->hess_type == 0 || (sm->hess_type == 2 && am == MTFHIP_AM_SSD);
	return sm->sm == MTFHIP_SM_ICLK && const_h && sm->chained_warp && !sm->sec_ord_hess && b->C == 1 && b->N <= kTemplateInitMaxPix &&
		b->h_flag_dev != nullptr && b->ctx->img.data != nullptr && b->ctx->img.channels == 1;
}
int init_template_fused(mtfhip_batch *b, const mtfhip_sm_desc *sm, const RegionIngest *rg, bool publish_host) {
	(void)sm;
	hipStream_t st = b->ctx->stream;
	const bool ncc = b->desc.am == MTFHIP_AM_NCC;
	TRY(need_image(b));
	for (int id : {MTFHIP_BUF_I0, MTFHIP_BUF_IT, MTFHIP_BUF_DI0_DX, MTFHIP_BUF_DIT_DX, MTFHIP_BUF_J0, MTFHIP_BUF_DF_DI0, MTFHIP_BUF_DF_DIT}) TRY(ensure_buf(b, id));
	if (!b->h_init_flag_dev) {   /* (the last of the record's four words to be set: while it is null a failed call is simply repeated) */
		HIP_TRY(b->h_init_rec.reserve(kInitRec * (size_t)b->B));
		HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&b->h_init_rec_dev), b->h_init_rec, 0));
		HIP_TRY(b->h_init_flag.reserve(1));
		*b->h_init_flag = 0;
		HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&b->h_init_flag_dev), b->h_init_flag, 0));
	}
	if (ncc) HIP_TRY(b->d_ncc_tm.reserve(NCC_TM_COUNT * (size_t)b->B));
	++b->frame_count;   /* ImageBase.cc:74 */
	const unsigned long long seq = ++b->init_seq;
	{
		TimedScope tsc(b->ctx, "template_init");
		launch_template_init(b->view(), b->ctx->img, b->desc.grad_eps, b->norm_mult, b->norm_add, b->d_h0, b->d_h0inv, ncc ? b->d_ncc : nullptr,
			ncc ? b->d_ncc_tm : nullptr, publish_host ? InitPublish{b->h_init_rec_dev, b->d_fin_count, b->h_init_flag_dev, seq, publish_fenced()} : InitPublish{nullptr, nullptr, nullptr, 0, 0},
			rg ? *rg : RegionIngest{}, st);
	}
	/* (the kernel also zeroes the gradient vectors df_dI0 / df_dIt: initializeSimilarity / initializeGrad) */
	touch(b, MTFHIP_BUF_DI0_DX); touch(b, MTFHIP_BUF_J0);
	b->init_pix_vals = b->it_valid = true;
	b->init_pix_grad = b->dit_valid = true;
	b->init_sim = b->init_grad = true;
	for (auto &h : b->th) h.f = ncc ? 1.0 : 0.0;
	b->ncc_host_newer = false;       /* (the kernel wrote d_ncc itself) */
	b->init_mirror_seq = seq;
	b->init_rec_device = !publish_host;
	b->j0_is_template = true;
	b->j0_template_corners_epoch = b->corners_epoch;
	b->j0_variant = MTFHIP_JAC_WARPED;
	b->template_corners.resize(8 * (size_t)b->B);
	for (int t = 0; t < b->B; ++t) std::memcpy(&b->template_corners[8 * t], b->th[t].init_corners, sizeof(double) * 8);
	return MTFHIP_OK;
}
int mtfhip_batch_init_template(mtfhip_batch *b, const mtfhip_sm_desc *sm) {
	TRY(lowdof_sm_refuse(b, sm, "init_template"));
	if (sm && alk_sm(sm->sm)) return alk_init_template(b, sm);
	FLUSH(b);
	TRY(begin_entry(b));
	TRY(check_sm(b, sm, "init_template"));
	if (!b->have_corners) return fail(MTFHIP_ERR_LOGIC, "init_template before set_corners");
	/* am->clearInitStatus() (NT/ESM.cc:113, NT/FCLK.cc:105, NT/ICLK.cc:74) */
	b->init_pix_vals = b->init_pix_grad = b->init_sim = b->init_grad = false;
	/* k_template_init samples INIT_PTS and builds J0 at the identity warp: that is the current image at the current points only while no
	 * setState / compositionalUpdate / update() has moved the warp since set_corners (the mirrors are exact: set_corners_core stores the
	 * identity itself, and every state change goes through them) */
	bool at_identity = true;
	{
		const M3 I = m3_identity();
		for (const TargetHost &h : b->th) if (std::memcmp(h.warp.m, I.m, sizeof(I.m)) != 0) { at_identity = false; break; }
	}
	if (at_identity && template_init_fused_ok(b, sm)) return init_template_fused(b, sm);
	TRY(mtfhip_am_initialize_pix_vals(b, nullptr));
	if (sm->chained_warp) {
		TRY(mtfhip_am_initialize_pix_grad(b, nullptr));
		TRY(mtfhip_ssm_cmpt_pix_jacobian(b, MTFHIP_JAC_WARPED, MTFHIP_BUF_DI0_DX, MTFHIP_BUF_J0));
	} else {
		TRY(mtfhip_ssm_update_grad_pts(b, b->desc.grad_eps));
		TRY(mtfhip_am_initialize_pix_grad_warped(b, nullptr));
		TRY(mtfhip_ssm_cmpt_pix_jacobian(b, MTFHIP_JAC_INIT, MTFHIP_BUF_DI0_DX, MTFHIP_BUF_J0));
	}
	if (sm->sec_ord_hess) {   /* initializePixHess, NT/ESM.cc:406-416 ; the template's pixel Hessian is rebuilt per pixel from
	                           * d2I0_dx2 and dI0_dx inside k_second_order_ssd instead of being stored as an S^2 x N matrix */
		b->init_pix_hess = false;
		if (sm->chained_warp) TRY(mtfhip_am_initialize_pix_hess(b, nullptr));
		else { TRY(mtfhip_ssm_update_hess_pts(b, b->hess_eps)); TRY(mtfhip_am_initialize_pix_hess_warped(b, nullptr, nullptr)); }
		b->d0_variant = sm->chained_warp ? MTFHIP_JAC_WARPED : MTFHIP_JAC_INIT;
	}
	TRY(mtfhip_am_initialize_similarity(b));
	TRY(mtfhip_am_initialize_grad(b));
	TRY(mtfhip_am_initialize_hess(b));
	if (b->lo_ssm) TRY(lowdof_template(b, sm, sm->chained_warp ? MTFHIP_JAC_WARPED : MTFHIP_JAC_INIT, true));
	else {
		if (ncc_rows(b)) TRY(ncc_template_moments(b));   /* (in front of H0: SSIM's is a function of them) */
		std::vector<double> H0((size_t)b->B * b->S * b->S);
		TRY(init_self_hessian(b, sm, H0.data()));
		TRY(store_h0(b, H0.data(), true));
		HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	}
	b->j0_is_template = true;
	b->j0_template_corners_epoch = b->corners_epoch;
	b->j0_variant = sm->chained_warp ? MTFHIP_JAC_WARPED : MTFHIP_JAC_INIT;
	b->template_corners.resize(8 * (size_t)b->B);
	for (int t = 0; t < b->B; ++t) std::memcpy(&b->template_corners[8 * t], b->th[t].init_corners, sizeof(double) * 8);
	return MTFHIP_OK;
}

/* nt::ESM::setRegion NT/ESM.cc:148-168, nt::FCLK::setRegion NT/FCLK.cc:360-376, nt::ICLK::setRegion NT/ICLK.cc:131-157 (update_ssm
 * off): the SSM is reset to the new corners; ESM (and FCLK with the InitialSelf Hessian) recompute init_pix_jacobian with
 * cmptInitPixJacobian on the new grid and, for the Hessian types that use it, the constant self Hessian; ICLK keeps its
 * template Jacobian.  The template (I0, dI0_dx) is kept in every case. */
int mtfhip_batch_set_region(mtfhip_batch *b, const double *corners, const mtfhip_sm_desc *sm) { return set_region_core(b, corners, sm, false); }

int set_region_core(mtfhip_batch *b, const double *corners, const mtfhip_sm_desc *sm, bool for_track, bool defer_grid, bool layout_later) {
	FLUSH_AM(b);   /* (the current points are about to be replaced: only pending calls need them brought up to date) */
	TRY(begin_entry(b));
	TRY(check_sm(b, sm, "set_region"));
	if (!b->init_pix_vals) return fail(MTFHIP_ERR_LOGIC, "set_region before init_template");
	TRY(set_corners_core(b, corners, for_track, defer_grid, layout_later));
	const bool refresh = region_refreshes(sm);
	if (layout_later) {
		if (refresh) return fail(MTFHIP_ERR_LOGIC, "set_region: a layout behind the launch with a search method that refreshes its template Jacobian");
		b->deferred_template_check = true;   /* (the comparison below, once the host has the corners: set_corners_finish_deferred) */
		return MTFHIP_OK;
	}
	if (!refresh) {
		/* back on exactly the grid the kept template Jacobian was computed on: its rows can still be rebuilt from dI0_dx */
		if (b->j0_is_template && b->template_corners.size() == 8 * (size_t)b->B &&
			std::memcmp(b->template_corners.data(), corners, sizeof(double) * 8 * b->B) == 0)
			b->j0_template_corners_epoch = b->corners_epoch;
		return MTFHIP_OK;
	}
	TRY(mtfhip_ssm_cmpt_pix_jacobian(b, MTFHIP_JAC_INIT, MTFHIP_BUF_DI0_DX, MTFHIP_BUF_J0));
	const bool need_h0 = sm->hess_type == 0 || (sm->sm == MTFHIP_SM_ESM && sm->hess_type == 2);
	/* (the template moments in front of H0: SSIM's is a function of them; a low-order SSM's are taken over its affine rows, lowdof_template) */
	if (ncc_rows(b) && !b->lo_ssm) TRY(ncc_template_moments(b));
	if (b->lo_ssm) TRY(lowdof_template(b, sm, MTFHIP_JAC_INIT, need_h0));
	else if (need_h0) {
		std::vector<double> H0((size_t)b->B * b->S * b->S);
		if (b->desc.am == MTFHIP_AM_MI && sm->sec_ord_hess) b->d0_variant = MTFHIP_JAC_INIT;   /* (setRegion: cmptInitPixHessian, NT/ESM.cc:160-163) */
		TRY(init_self_hessian(b, sm, H0.data()));
		TRY(store_h0(b, H0.data(), true));
		HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	}
	b->j0_is_template = true;
	b->j0_template_corners_epoch = b->corners_epoch;
	b->j0_variant = MTFHIP_JAC_INIT;
	b->template_corners.assign(corners, corners + 8 * (size_t)b->B);
	return MTFHIP_OK;
}

int fused_args(const mtfhip_batch *b, const mtfhip_sm_desc *sm, FusedArgs &fa) {
	fa.chained = sm->chained_warp ? 1 : 0;
	fa.materialize = sm->materialize ? 1 : 0;
	fa.hess_mean = 0;
	fa.j0_recompute = (b->j0_is_template && b->j0_recompute_enabled && b->j0_template_corners_epoch == b->corners_epoch) ? 1 : 0;
	fa.j0_init_variant = b->j0_variant == MTFHIP_JAC_INIT ? 1 : 0;
	fa.grad_eps = b->desc.grad_eps;
	fa.norm_mult = b->norm_mult; fa.norm_add = b->norm_add;
	fa.active = nullptr;
	fa.inline_warp = 0;
	fa.fast_math = (b->math_mode == MTFHIP_MATH_FAST && !fa.materialize) ? 1 : 0;
	{ int nb; fused_decomposition(b->N, b->B, nb, fa.rows_per_block); }
	/* the template grid rebuilt in the kernel (16 B per point less): the grid is still the one k_init_grid laid out from d_w0 for these
	 * corners (grid_w0_epoch; a caller write to INIT_PTS / INIT_Z / INIT_HXY clears grid_from_corners), the maps divide by nothing, and
	 * the launch is the materialising SSD one -- the only instantiation with the rebuild (fused_lk_body, GR_OK), whose lattice products
	 * launch_fused_ssd gives (resx + resy) double2 of LDS */
	fa.grid_regen = (b->unit_z && b->grid_from_corners && b->grid_w0_epoch == b->corners_epoch && b->grid_w0_affine && b->C == 1 &&
		b->d_w0 && b->desc.resx + b->desc.resy <= kGridTabMax) ? 1 : 0;
	fa.w0 = b->d_w0;
	{
		const RegionIngest rg = region_geometry(b);
		fa.g_resx = rg.resx; fa.g_resy = rg.resy;
		fa.g_lo_x = rg.lo_x; fa.g_lo_y = rg.lo_y; fa.g_hi_x = rg.hi_x; fa.g_hi_y = rg.hi_y;
		fa.g_step_x = (fa.g_hi_x - fa.g_lo_x) / (b->desc.resx - 1); fa.g_step_y = (fa.g_hi_y - fa.g_lo_y) / (b->desc.resy - 1);
	}
	switch (sm->sm) {
	case MTFHIP_SM_FCLK: fa.mode = 0; break;
	case MTFHIP_SM_ESM: fa.mode = 1; fa.hess_mean = sm->hess_type == 3; break;
	default:
		if (sm->hess_type == 1) return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "fused ICLK with hess_type CurrentSelf: use the un-fused entry points");
		fa.mode = 2;
	}
	if (!grid_regen_kernel(b->desc.am, b->desc.ssm, fa.chained != 0, fa.mode, fa.materialize != 0) || fa.rows_per_block < kGridRegenMinRows)
		fa.grid_regen = 0;
	if (b->lo_ssm) fa.grid_regen = 0;   /* (a low-order SSM's lattice is not the affine one the pass would rebuild: set_corners_core's extents) */
	return MTFHIP_OK;
}

int mtfhip_batch_grid_regen(mtfhip_batch *b, const mtfhip_sm_desc *sm) {
	if (!b || !sm) return 0;
	FusedArgs fa;
	return fused_args(b, sm, fa) == MTFHIP_OK && fa.grid_regen ? 1 : 0;
}

/* The second-order term an SSD search method adds to its Hessian (k_second_order_ssd's `term`), -1 for none:
 * SSD's self Hessians are first order by definition (SSDBase.h:95-98) and InitialSelf never looks at the frame. */
/* MI (am = MTFHIP_AM_MI): its self Hessian has a second-order form of its own (MI.cc:697-735) -- term 4, the current pixel Hessian
 * weighted by sum_r gradIt(r) sum_t matIt(t) self_grad_factor(r, t) -- for CurrentSelf and ESM's SumOfSelf (whose other half, the
 * initial self Hessian, carries its second-order part since initialize / setRegion). */
int second_order_term(const mtfhip_sm_desc *sm, int am) {
	if (!sm->sec_ord_hess) return -1;
	if (am == MTFHIP_AM_MI && (sm->hess_type == 1 || (sm->sm == MTFHIP_SM_ESM && sm->hess_type == 2))) return 4;
	switch (sm->sm) {
	case MTFHIP_SM_FCLK: return sm->hess_type == 2 ? 0 : -1;
	case MTFHIP_SM_ESM: return sm->hess_type == 5 ? 0 : (sm->hess_type == 4 ? 1 : (sm->hess_type == 3 ? 2 : -1));
	default: return sm->hess_type == 2 ? 3 : -1;
	}
}

/* the reduced rows of a fused pass -> every target's f, g and H of the search method before damping: loops over the entries of mtfhip_sm_system.h,
 * the statement the device-side finish reads as well (NT/FCLK.cc:260-288 ; NT/ESM.cc:298-377 with SSDBase.cc:169-191,287-311 ; NT/ICLK.cc:206-251).
 * so: [B][S x S] second-order sums (x so_scale) or NULL */
int assemble_rows(mtfhip_batch *b, const mtfhip_sm_desc *sm, bool hess_mean, int nblk, const double *so, double so_scale, double *f, double *g, double *H) {
	const bool ncc = ncc_rows(b), spss = spss_am(b), ssim = ssim_am(b);   /* (ncc: the rows are NCC's moments -- NCC itself and SSIM) */
	const int S = b->S, S2 = S * S, RL = ncc ? NCC_ACC_COUNT : ACC_COUNT;
	TRY(read_rows(b, nblk, RL));
	if (ncc && !ncc_has_gram(ncc_h_which(*sm), hess_mean)) return fail(MTFHIP_ERR_LOGIC, "fused NCC: the Gram matrix this Hessian needs was not accumulated");
	for (int t = 0; t < b->B; ++t) {
		TargetHost &h = b->th[t];
		const double *row = b->h_acc + (size_t)t * RL, *sot = so ? so + (size_t)t * S2 : nullptr;
		double *gt = g + (size_t)t * S, *Ht = H + (size_t)t * S2;
		if (ssim) {
			/* SSIM over NCC's row: entry (r, c) of the constant Hessian and of the row's own, never a triangle (ssim_hess is not symmetric) */
			const SsimSys sq = ssim_host_sys(b, h, row);
			ssim_refresh_mirrors(h, sq, row);
			if (f) f[t] = h.f;
			for (int s = 0; s < S; ++s) gt[s] = ssim_g(*sm, sq, s);
			for (int c = 0; c < S; ++c)
				for (int r = 0; r < S; ++r) Ht[c * S + r] = ssim_h(*sm, sq, h.h0[c * S + r], r, c);
			continue;
		}
		if (ncc) ncc_refresh_mirrors(b, h, row); else h.f = ssd_f(spss, row);
		NccSys q = NccSys();
		if (ncc) q = ncc_host_sys(b, h, row);
		if (f) f[t] = h.f;
		for (int s = 0; s < S; ++s) gt[s] = ncc ? ncc_g(*sm, q, s) : ssd_g(*sm, spss, row, s);
		for (int c = 0; c < S; ++c)
			for (int r = 0; r < S; ++r) {
				/* (ncc_h leaves ex out of InitialSelf and ESM's SumOfSelf: second_order_term is -1 for exactly those, so `so` is NULL there) */
				const double ex = sot ? so_scale * sot[c * S + r] : 0.0;
				if (ncc) Ht[c * S + r] = ncc_h(*sm, q, h.h0[(r < c ? c : r) * S + (r < c ? r : c)], ex, r, c);
				else { double v = ssd_h(*sm, false, spss, row, h.h0, S, r, c); if (sot) v += ex; Ht[c * S + r] = v; }
			}
	}
	if (ncc) b->ncc_host_newer = true;
	return MTFHIP_OK;
}

static int iterate_core(mtfhip_batch *b, const mtfhip_sm_desc *sm, double *f, double *g, double *H);
int mtfhip_batch_iterate(mtfhip_batch *b, const mtfhip_sm_desc *sm, double *f, double *g, double *H) {
	TRY(lowdof_sm_refuse(b, sm, "iterate"));
	if (sm && alk_sm(sm->sm)) return alk_iterate(b, sm, f, g, H);
	if (!b || !b->lo_ssm) return iterate_core(b, sm, f, g, H);
	/* a low-order SSM: the affine pass and its host-side assembly in affine coordinates, then the projection; a materialising launch left
	 * its six Jacobian columns in the scratch planes -- the interface's N x S curr_pix_jacobian is formed from the materialised dIt_dx by
	 * the model's own expressions (k_pix_jacobian), and ESM's mean_pix_jacobian from that and J0, where the search method keeps one */
	/* (the checks of iterate_core, in its order and with its answers: the outputs here are this function's own staging arrays) */
	TRY(check_sm(b, sm, "iterate"));
	if (!g || !H) return fail(MTFHIP_ERR_INVALID_ARG, "iterate: NULL output");
	TRY(lowdof_template_current(b, "iterate"));
	std::vector<double> g6((size_t)6 * b->B), H6((size_t)36 * b->B);
	{
		PassMode pm(b);
		TRY(ensure_buf(b, MTFHIP_BUF_J0));
		TRY(ensure_buf(b, MTFHIP_BUF_JT));   /* (the pass's six-column planes) */
		TRY(iterate_core(b, sm, f, g6.data(), H6.data()));
	}
	const int SS = b->S;
	/* g_S = g_aff M, H_S = M^T H_aff M (lowdof_g / lowdof_h, mtfhip_sm_system.h) over the column-major 6 x 6 of each target */
	for (int t = 0; t < b->B; ++t) {
		const double *gt6 = &g6[(size_t)6 * t], *Ht6 = &H6[(size_t)36 * t];
		for (int c = 0; c < SS; ++c) {
			g[(size_t)t * SS + c] = lowdof_g(b->lo_ssm, c, [&](int a) { return gt6[a]; });
			for (int r = 0; r < SS; ++r) H[(size_t)t * SS * SS + c * SS + r] = lowdof_h(b->lo_ssm, r, c, [&](int rr, int cc) { return Ht6[cc * 6 + rr]; });
		}
	}
	if (sm->materialize && sm->sm != MTFHIP_SM_ICLK) {
		TRY(do_cmpt_pix_jacobian(b, sm->chained_warp ? MTFHIP_JAC_WARPED : MTFHIP_JAC_INIT, MTFHIP_BUF_DIT_DX, MTFHIP_BUF_JT));
		if (sm->sm == MTFHIP_SM_ESM && (sm->jac_type == 0 || sm->hess_type == 3)) TRY(mtfhip_sm_mean_jacobian(b));   /* NT/ESM.cc:239-242 */
	}
	return MTFHIP_OK;
}
static int iterate_core(mtfhip_batch *b, const mtfhip_sm_desc *sm, double *f, double *g, double *H) {
	FLUSH_AM(b);   /* the fused kernels derive the sample points from the warp: CURR_PTS may stay stale */
	TRY(begin_entry(b));
	TRY(check_sm(b, sm, "iterate"));
	if (b->C != 1 && sm->sec_ord_hess) return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "iterate: second-order Hessians of the multi-channel models use the per-function entry points");
	if (!g || !H) return fail(MTFHIP_ERR_INVALID_ARG, "iterate: NULL output");
	if (!b->init_pix_vals) return fail(MTFHIP_ERR_LOGIC, "iterate before init_template");
	TRY(need_image(b));
	if (b->desc.am == MTFHIP_AM_MI) return mi_iterate(b, sm, f, g, H);
	if (ccre_am(b)) return ccre_iterate(b, sm, f, g, H);
	if (second_order_term(sm) >= 0) TRY(ensure_pts(b));   /* k_second_order_ssd reads the current points */
	FusedArgs fa;
	TRY(fused_args(b, sm, fa));
	/* the SCV family at the current warp: SCV / LSCV::updateSimilarity re-map the template, then the SSD iteration on it; RSCV /
	 * LRSCV::updatePixVals build the map(s) of the current patch, which the fused pass applies to every sample (an LRSCV pass without
	 * them is the SSD pass on the raw patch) */
	FusedMaps maps;
	TRY(imap_before_pass(b, nullptr, 0, nullptr, &fa, 0, b->first_iter != 0, b->ctx->stream, &maps));
	int nblk = fused_blocks_per_target(b->N, b->B);
	{
		TimedScope ts(b->ctx, "fused_lk");
		const SpssArgs sp = spss_am(b) ? spss_args(b, sm) : SpssArgs{};
		launch_fused_ssd(fused_view(b, fa), b->ctx->img, fa, b->d_partials, nblk, b->ctx->stream, &maps, spss_am(b) ? &sp : nullptr);
	}
	b->it_valid = fa.materialize;
	b->dit_valid = fa.materialize && fa.mode != 2;
	b->jt_valid = fa.materialize && fa.mode != 2;
	const bool ncc = b->desc.am == MTFHIP_AM_NCC;   /* (the second-order pass's NCC form: SSIM's second-order types are refused, check_sm) */
	const int term = second_order_term(sm);
	const int S2 = b->S * b->S;
	std::vector<double> so;
	if (term >= 0) {
		if (term != 0 && !b->init_pix_hess) return fail(MTFHIP_ERR_LOGIC, "iterate: init_template was run without sec_ord_hess");
		const int nb2 = simple_blocks_per_target(b->N);
		TRY(ensure_second_order_scratch(b));
		if (ncc) TRY(push_ncc(b));   /* mean(I0), |I0 - mean| of the template */
		{
			TimedScope ts(b->ctx, "second_order");
			launch_second_order_ssd(b->view(), b->ctx->img, term, fa.chained, b->d0_variant, fa.grad_eps, b->hess_eps, b->norm_mult,
				b->norm_add, b->d_d2_part, nb2, b->d_d2_out, b->ctx->stream, 0,
				ncc ? SecondOrderNcc{b->d_partials, nblk, b->d_ncc} : SecondOrderNcc{nullptr, 0, nullptr});
		}
		so.resize((size_t)S2 * b->B);
		HIP_TRY(hipMemcpyAsync(so.data(), b->d_d2_out, sizeof(double) * so.size(), hipMemcpyDeviceToHost, b->ctx->stream));
	}
	/* (SumOfStd halves the whole sum, NT/ESM.cc:339) */
	return assemble_rows(b, sm, fa.hess_mean != 0, nblk, term >= 0 ? so.data() : nullptr, term == 1 ? 0.5 : 1.0, f, g, H);
}

} /* extern "C" */

#ifdef MTFHIP_FIN_TRACE
namespace mtfhip { void debug_fin_trace(unsigned long long *out); }
extern "C" void mtfhip_debug_fin_trace(unsigned long long *out) { mtfhip::debug_fin_trace(out); }
#endif
