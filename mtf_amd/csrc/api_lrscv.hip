/*
 * api_lrscv.hip -- the Localized Reversed SCV appearance model's own state (AM/src/LRSCV.cc): its configuration, the per-iteration maps
 * of the current patch (C-ABI implementation, include/mtfhip.h; the kernels: kernels_lrscv.hip, kernels_fused_lrscv.hip)
 *
 * LRSCV is an SSDBase whose updatePixVals samples It and, unless once_per_frame and not the first iteration (LRSCV.cc:234-235: then It
 * stays raw), maps it through one E[I0 | It] per overlapping sub-region and blends the images with per-pixel weights (LRSCV.cc:224-292).
 * It borrows the state of its two parents: RSCV's code plane ((int)I0) and per-function It_orig buffer (d_rscv_code, d_rscv_it), and
 * LSCV's sub-region geometry, weights, sums, maps and affine parameters (d_lscv_*, lscv_geometry).  The per-function route keeps the
 * reference's split literally (lrscv_update_pix_vals writes MTFHIP_BUF_IT); the fused route enqueues pass 1 in front of the fused pass
 * (lrscv_enqueue), which blends every sample itself.  A pass that does not map is an SSD pass on the raw patch.
 *
 * Accepted and ignored: LRSCVParams::pre_seed (updatePixVals passes pre-seeds of 0 to getDiracJointHist, LRSCV.cc:240-243),
 * show_subregions (an OpenCV window), debug_mode.
 */
#include "mtfhip_api_internal.h"

int lrscv_capture(mtfhip_batch *b) {
	/* the maps live in the fused pass's dynamic LDS beside its static arrays */
	TRY(lscv_geometry(b, (size_t)kLscvLdsBudget - kLrscvFusedStaticLds));
	const size_t B = (size_t)b->B, N = (size_t)b->N;
	hipStream_t st = b->ctx->stream;
	HIP_TRY(b->d_rscv_it.reserve(N * B));
	HIP_TRY(b->d_rscv_code.reserve(N * B));   /* (last: lrscv_update_pix_vals and lrscv_enqueue take it for "captured") */
	/* LRSCV::initializePixVals, first call: It = I0 (LRSCV.cc:208-210) */
	HIP_TRY(hipMemcpyAsync(b->d_rscv_it, b->buf[MTFHIP_BUF_I0], sizeof(double) * N * B, hipMemcpyDeviceToDevice, st));
	/* the template's columns of the joint histograms: (int)I0 */
	launch_rscv_codes(b->N, b->B, b->lscv_nb, b->buf[MTFHIP_BUF_I0], b->d_rscv_code, st);
	return MTFHIP_OK;
}

static LrscvArgs lrscv_args(mtfhip_batch *b, int t0, const int *active, const FusedArgs *fa) {
	const size_t N = (size_t)b->N, nb = (size_t)b->lscv_nb, R = (size_t)b->lscv_nx * b->lscv_ny, E = (size_t)b->lscv_ncell * nb;
	LrscvArgs a;
	a.nb = b->lscv_nb; a.kind = rscv_it_kind(fa);
	a.nx = b->lscv_nx; a.ny = b->lscv_ny; a.ncx = b->lscv_ncx; a.ncell = b->lscv_ncell;
	a.affine = b->lscv_affine;
	a.norm_mult = b->norm_mult; a.norm_add = b->norm_add; a.grad_eps = b->desc.grad_eps;
	a.code = b->d_rscv_code + (size_t)t0 * N;
	a.it_orig = fa ? nullptr : b->d_rscv_it + (size_t)t0 * N;
	a.cell = b->d_lscv_cell; a.crng = b->d_lscv_crng;
	a.active = active;
	a.tot = b->d_lscv_tot + (size_t)t0 * 2 * E;
	a.arrive = b->d_lscv_arrive + t0;
	a.map = b->d_lscv_map + (size_t)t0 * R * nb;
	a.aff = b->d_lscv_aff + (size_t)t0 * 2 * R;
	return a;
}

/* the blend's arguments for the targets from t0 on */
static LrscvMap lrscv_map(const mtfhip_batch *b, int t0) {
	const size_t R = (size_t)b->lscv_nx * b->lscv_ny;
	LrscvMap lm;
	lm.map = b->lscv_affine ? b->d_lscv_aff + (size_t)t0 * 2 * R : b->d_lscv_map + (size_t)t0 * R * b->lscv_nb;
	lm.wts = b->d_lscv_w;
	lm.nb = b->lscv_nb; lm.R = (int)R; lm.affine = b->lscv_affine; lm.linear = b->lscv_linear;
	return lm;
}

int lrscv_enqueue(mtfhip_batch *b, const BatchView &bv, int t0, const int *active, const FusedArgs &fa, hipStream_t st, LrscvMap *lm) {
	if (!b->d_rscv_code) return fail(MTFHIP_ERR_LOGIC, "lrscv :: updatePixVals before initializePixVals");
	if (fa.grad_eps != b->desc.grad_eps || fa.norm_mult != b->norm_mult || fa.norm_add != b->norm_add)
		return fail(MTFHIP_ERR_LOGIC, "lrscv :: the fused launch's normalisation is not the batch's");
	{
		TimedScope ts(b->ctx, "lrscv_map", st);
		launch_lrscv_hist(bv, b->ctx->img, lrscv_args(b, t0, active, &fa), st);
	}
	*lm = lrscv_map(b, t0);
	return MTFHIP_OK;
}

int lrscv_update_pix_vals(mtfhip_batch *b, const double *dp) {
	if (!b->d_rscv_code) return fail(MTFHIP_ERR_LOGIC, "lrscv :: updatePixVals before initializePixVals");
	hipStream_t st = b->ctx->stream;
	TimedScope ts(b->ctx, "sample");
	const BatchView bv = b->view();
	/* It at the current points (LRSCV.cc:226-232); once_per_frame and not the first iteration: that is all (LRSCV.cc:234-235) */
	if (!lrscv_due(b)) {
		launch_sample(bv, b->ctx->img, dp, b->buf[MTFHIP_BUF_IT], b->norm_mult, b->norm_add, st);
		return MTFHIP_OK;
	}
	/* It_orig, the sub-region maps (LRSCV.cc:237-247) and the blend (:249-254) */
	launch_sample(bv, b->ctx->img, dp, b->d_rscv_it, b->norm_mult, b->norm_add, st);
	launch_lrscv_hist(bv, b->ctx->img, lrscv_args(b, 0, nullptr, nullptr), st);
	launch_lrscv_apply(b->N, b->B, lrscv_map(b, 0), b->d_rscv_it, b->buf[MTFHIP_BUF_IT], st);
	return MTFHIP_OK;
}

extern "C" {

int mtfhip_batch_set_lrscv(mtfhip_batch *b, int n_sub_regions_x, int n_sub_regions_y, int spacing_x, int spacing_y, int affine_mapping,
	int once_per_frame, int weighted_mapping) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "set_lrscv: NULL batch");
	if (b->desc.am != MTFHIP_AM_LRSCV) return fail(MTFHIP_ERR_INVALID_ARG, "set_lrscv: the batch's appearance model is %d, not LRSCV", b->desc.am);
	if (b->d_lscv_cell) return fail(MTFHIP_ERR_LOGIC, "set_lrscv: call it before init_template (the sub-region geometry is fixed there)");
	if ((affine_mapping != 0 && affine_mapping != 1) || (once_per_frame != 0 && once_per_frame != 1) || (weighted_mapping != 0 && weighted_mapping != 1))
		return fail(MTFHIP_ERR_INVALID_ARG, "set_lrscv: affine_mapping, once_per_frame and weighted_mapping must be 0 or 1 (got %d, %d, %d)", affine_mapping,
			once_per_frame, weighted_mapping);
	TRY(lscv_check_geometry(b, n_sub_regions_x, n_sub_regions_y, spacing_x, spacing_y, "set_lrscv"));
	b->lscv_nx = n_sub_regions_x; b->lscv_ny = n_sub_regions_y;
	b->lscv_sx = spacing_x; b->lscv_sy = spacing_y;
	b->lscv_affine = affine_mapping; b->lscv_once = once_per_frame; b->lscv_linear = weighted_mapping;
	return MTFHIP_OK;
}

int mtfhip_batch_lrscv_intensity_maps(mtfhip_batch *b, double *dst) {
	if (!b || !dst) return fail(MTFHIP_ERR_INVALID_ARG, "lrscv_intensity_maps: NULL argument");
	if (b->desc.am != MTFHIP_AM_LRSCV) return fail(MTFHIP_ERR_INVALID_ARG, "lrscv_intensity_maps: the batch's appearance model is %d, not LRSCV", b->desc.am);
	FLUSH(b);
	if (!b->d_lscv_map) return fail(MTFHIP_ERR_LOGIC, "lrscv_intensity_maps before initializePixVals");
	HIP_TRY(hipMemcpyAsync(dst, b->d_lscv_map, sizeof(double) * (size_t)b->lscv_nx * b->lscv_ny * b->lscv_nb * b->B, hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	return MTFHIP_OK;
}

} /* extern "C" */
