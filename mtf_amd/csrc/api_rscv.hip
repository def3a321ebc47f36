/*
 * api_rscv.hip -- the Reversed SCV appearance model's own state (AM/src/RSCV.cc): the template's code plane, the intensity maps, the
 * per-function It_orig, its configuration (C-ABI implementation, include/mtfhip.h; the kernels: kernels_rscv.hip, kernels_fused_rscv.hip)
 *
 * RSCV is an SSDBase whose updatePixVals maps the current patch through the conditional expectation E[I0 | It] (RSCV.cc:170-238).
 * Everything behind updatePixVals is SSD on the mapped It.  The per-function route keeps that split literally (rscv_update_pix_vals
 * writes MTFHIP_BUF_IT = map(It_orig)); the fused route enqueues pass 1 + the map in front of the fused pass (rscv_enqueue), which
 * applies the map to every sample itself.
 */
#include "mtfhip_api_internal.h"

int rscv_capture(mtfhip_batch *b) {
	const size_t B = (size_t)b->B, N = (size_t)b->N, nb = (size_t)b->rscv_nb;
	hipStream_t st = b->ctx->stream;
	/* (d_rscv_code, which everything else takes for "captured", arrives last: while it is null a failed call is simply repeated, and what
	 * belongs to the first call runs once the whole group is there) */
	const bool first = !b->d_rscv_code;
	HIP_TRY(b->d_rscv_part.reserve((size_t)rscv_hist_blocks(b->N) * 2 * nb * B));
	HIP_TRY(b->d_rscv_arrive.reserve(B));
	HIP_TRY(b->d_rscv_map.reserve(nb * B));
	HIP_TRY(b->d_rscv_it.reserve(N * B));
	if (first) {
		HIP_TRY(hipMemsetAsync(b->d_rscv_arrive, 0, sizeof(unsigned) * B, st));
		/* RSCV::initializePixVals, first call: It = I0, It_orig = It (RSCV.cc:158-162) */
		HIP_TRY(hipMemcpyAsync(b->d_rscv_it, b->buf[MTFHIP_BUF_I0], sizeof(double) * N * B, hipMemcpyDeviceToDevice, st));
	}
	HIP_TRY(b->d_rscv_code.reserve(N * B));
	/* the template's columns of the joint histogram: (int)I0 */
	launch_rscv_codes(b->N, b->B, b->rscv_nb, b->buf[MTFHIP_BUF_I0], b->d_rscv_code, st);
	/* before the first updatePixVals the map is the identity of the bins (what the empty-bin rule gives) */
	std::vector<double> id(nb * B);
	for (size_t t = 0; t < B; ++t)
		for (size_t k = 0; k < nb; ++k) id[t * nb + k] = (double)k;
	HIP_TRY(hipMemcpyAsync(b->d_rscv_map, id.data(), sizeof(double) * id.size(), hipMemcpyHostToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));   /* (id is a stack-lifetime buffer) */
	return MTFHIP_OK;
}

/* the It_orig expression of the fused launch fa selects (launch_fused_rscv / launch_fused_lrscv: the same for either model and SSM) */
int rscv_it_kind(const FusedArgs *fa) {
	if (!fa) return RSCV_IT_FROM_BUF;
	return fused_it_kind(fused_select(FUSED_ROUTE_LOOP, MTFHIP_AM_RSCV, 1, MTFHIP_SSM_HOMOGRAPHY, fa->mode, fa->chained, fa->materialize, fa->fast_math));
}

static RscvArgs rscv_args(mtfhip_batch *b, int t0, const int *active, const FusedArgs *fa) {
	const size_t N = (size_t)b->N, nb = (size_t)b->rscv_nb;
	RscvArgs a;
	a.nb = b->rscv_nb; a.kind = rscv_it_kind(fa);
	a.norm_mult = b->norm_mult; a.norm_add = b->norm_add; a.grad_eps = b->desc.grad_eps;
	a.code = b->d_rscv_code + (size_t)t0 * N;
	a.it_orig = fa ? nullptr : b->d_rscv_it + (size_t)t0 * N;
	a.active = active;
	a.part = b->d_rscv_part + (size_t)t0 * rscv_hist_blocks(b->N) * 2 * nb;
	a.arrive = b->d_rscv_arrive + t0;
	a.map = b->d_rscv_map + (size_t)t0 * nb;
	return a;
}

int rscv_enqueue(mtfhip_batch *b, const BatchView &bv, int t0, const int *active, const FusedArgs &fa, hipStream_t st, RscvMap *rm) {
	if (!b->d_rscv_code) return fail(MTFHIP_ERR_LOGIC, "rscv :: updatePixVals before initializePixVals");
	if (fa.grad_eps != b->desc.grad_eps || fa.norm_mult != b->norm_mult || fa.norm_add != b->norm_add)
		return fail(MTFHIP_ERR_LOGIC, "rscv :: the fused launch's normalisation is not the batch's");
	{
		TimedScope ts(b->ctx, "rscv_map", st);
		launch_rscv_hist(bv, b->ctx->img, rscv_args(b, t0, active, &fa), st);
	}
	rm->map = b->d_rscv_map + (size_t)t0 * b->rscv_nb;
	rm->nb = b->rscv_nb;
	rm->linear = b->rscv_linear;
	return MTFHIP_OK;
}

int rscv_update_pix_vals(mtfhip_batch *b, const double *dp) {
	if (!b->d_rscv_code) return fail(MTFHIP_ERR_LOGIC, "rscv :: updatePixVals before initializePixVals");
	hipStream_t st = b->ctx->stream;
	TimedScope ts(b->ctx, "sample");
	const BatchView bv = b->view();
	/* It_orig at the current points (RSCV.cc:171-189), the joint histogram and the map (RSCV.cc:204-229), It = map(It_orig) (:230-234) */
	launch_sample(bv, b->ctx->img, dp, b->d_rscv_it, b->norm_mult, b->norm_add, st);
	launch_rscv_hist(bv, b->ctx->img, rscv_args(b, 0, nullptr, nullptr), st);
	launch_rscv_apply(b->N, b->B, b->rscv_nb, b->rscv_linear, b->d_rscv_map, b->d_rscv_it, b->buf[MTFHIP_BUF_IT], st);
	return MTFHIP_OK;
}

extern "C" {

int mtfhip_batch_set_rscv(mtfhip_batch *b, int use_bspl, int weighted_mapping, int mapped_gradient) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "set_rscv: NULL batch");
	if (b->desc.am != MTFHIP_AM_RSCV) return fail(MTFHIP_ERR_INVALID_ARG, "set_rscv: the batch's appearance model is %d, not RSCV", b->desc.am);
	if (use_bspl)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "set_rscv: RSCV use_bspl = 1 (BSpline histograms) is not available on the device path (Dirac histograms are)");
	if (mapped_gradient)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "set_rscv: RSCV mapped_gradient = 1 (the current gradient taken through the intensity map) is not available on the device path");
	if (weighted_mapping != 0 && weighted_mapping != 1) return fail(MTFHIP_ERR_INVALID_ARG, "set_rscv: weighted_mapping must be 0 or 1 (got %d)", weighted_mapping);
	b->rscv_linear = weighted_mapping;
	return MTFHIP_OK;
}

int mtfhip_batch_rscv_intensity_map(mtfhip_batch *b, double *dst) {
	if (!b || !dst) return fail(MTFHIP_ERR_INVALID_ARG, "rscv_intensity_map: NULL argument");
	if (b->desc.am != MTFHIP_AM_RSCV) return fail(MTFHIP_ERR_INVALID_ARG, "rscv_intensity_map: the batch's appearance model is %d, not RSCV", b->desc.am);
	FLUSH(b);
	if (!b->d_rscv_map) return fail(MTFHIP_ERR_LOGIC, "rscv_intensity_map before initializePixVals");
	HIP_TRY(hipMemcpyAsync(dst, b->d_rscv_map, sizeof(double) * (size_t)b->rscv_nb * b->B, hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	return MTFHIP_OK;
}

} /* extern "C" */
