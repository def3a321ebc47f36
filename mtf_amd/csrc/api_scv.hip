/*
 * api_scv.hip -- the SCV appearance model's own state (AM/src/SCV.cc): I0_orig, the per-iteration template re-map, its configuration
 * (C-ABI implementation, include/mtfhip.h; the kernels: kernels_scv.hip)
 *
 * SCV is an SSDBase whose updateSimilarity first re-maps the template through the conditional expectation E[It | I0_orig] (SCV.cc:194-230).
 * The device path keeps that split: scv_enqueue re-maps MTFHIP_BUF_I0 in place, and the SSD code behind it (the per-function
 * entry points, the fused SSD kernels) runs unchanged on it.  J0 / dI0_dx stay those of the original template (mapped_gradient 0).
 */
#include "mtfhip_api_internal.h"

int scv_capture(mtfhip_batch *b) {
	const size_t B = (size_t)b->B, N = (size_t)b->N, nb = (size_t)b->scv_nb;
	hipStream_t st = b->ctx->stream;
	/* (d_scv_i0, which scv_enqueue takes for "captured", arrives last: while it is null a failed call is simply repeated) */
	HIP_TRY(b->d_scv_code.reserve(N * B));
	HIP_TRY(b->d_scv_part.reserve((size_t)scv_hist_blocks(b->N) * 2 * nb * B));
	HIP_TRY(b->d_scv_map.reserve(nb * B));
	HIP_TRY(b->d_scv_i0.reserve(N * B));
	/* I0_orig = I0 (SCV.cc:166) */
	HIP_TRY(hipMemcpyAsync(b->d_scv_i0, b->buf[MTFHIP_BUF_I0], sizeof(double) * N * B, hipMemcpyDeviceToDevice, st));
	launch_scv_codes(b->N, b->B, b->scv_nb, b->d_scv_i0, b->d_scv_code, st);
	/* before the first update the map is the identity of the bins (what the empty-bin rule gives) */
	std::vector<double> id(nb * B);
	for (size_t t = 0; t < B; ++t)
		for (size_t k = 0; k < nb; ++k) id[t * nb + k] = (double)k;
	HIP_TRY(hipMemcpyAsync(b->d_scv_map, id.data(), sizeof(double) * id.size(), hipMemcpyHostToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));   /* (id is a stack-lifetime buffer) */
	return MTFHIP_OK;
}

int scv_enqueue(mtfhip_batch *b, const BatchView &bv, int t0, const int *active, int from_it, hipStream_t st) {
	if (!b->d_scv_i0) return fail(MTFHIP_ERR_LOGIC, "scv :: updateSimilarity before initializePixVals");
	const size_t N = (size_t)b->N, nb = (size_t)b->scv_nb;
	ScvArgs a;
	a.nb = b->scv_nb; a.hist = b->scv_hist; a.linear = b->scv_linear; a.from_it = from_it;
	a.norm_mult = b->norm_mult; a.norm_add = b->norm_add;
	a.code = b->d_scv_code + (size_t)t0 * N;
	a.i0o = b->d_scv_i0 + (size_t)t0 * N;
	a.active = active;
	{
		TimedScope ts(b->ctx, "scv_remap", st);
		launch_scv_update(bv, b->ctx->img, a, b->d_scv_part + (size_t)t0 * scv_hist_blocks(b->N) * 2 * nb, b->d_scv_map + (size_t)t0 * nb,
			bv.buf[MTFHIP_BUF_I0], st);
	}
	touch(b, MTFHIP_BUF_I0);
	return MTFHIP_OK;
}

int scv_refuse(const mtfhip_batch *b, const char *fn, int sec_ord_hess) {
	if (!b || !intensity_mapped(b)) return MTFHIP_OK;
	if (sec_ord_hess)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: %s with second-order Hessians is not available on the device path (first-order only)", fn,
			intensity_mapped_name(b));
	return MTFHIP_OK;
}

extern "C" {

int mtfhip_batch_set_scv(mtfhip_batch *b, int hist_type, int weighted_mapping, int mapped_gradient) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "set_scv: NULL batch");
	if (b->desc.am != MTFHIP_AM_SCV) return fail(MTFHIP_ERR_INVALID_ARG, "set_scv: the batch's appearance model is %d, not SCV", b->desc.am);
	if (hist_type == MTFHIP_SCV_HIST_BSPLINE)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "set_scv: SCV hist_type BSpline is not available on the device path (Dirac and Bilinear are)");
	if (hist_type != MTFHIP_SCV_HIST_DIRAC && hist_type != MTFHIP_SCV_HIST_BILINEAR)
		return fail(MTFHIP_ERR_INVALID_ARG, "set_scv: Invalid histogram type provided (%d)", hist_type);
	if (mapped_gradient)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "set_scv: SCV mapped_gradient = 1 (the template gradient re-mapped through the intensity map) is not available on the device path");
	if (weighted_mapping != 0 && weighted_mapping != 1) return fail(MTFHIP_ERR_INVALID_ARG, "set_scv: weighted_mapping must be 0 or 1 (got %d)", weighted_mapping);
	b->scv_hist = hist_type;
	b->scv_linear = weighted_mapping;
	b->scv_mapped_grad = 0;
	return MTFHIP_OK;
}

int mtfhip_batch_scv_intensity_map(mtfhip_batch *b, double *dst) {
	if (!b || !dst) return fail(MTFHIP_ERR_INVALID_ARG, "scv_intensity_map: NULL argument");
	if (b->desc.am != MTFHIP_AM_SCV) return fail(MTFHIP_ERR_INVALID_ARG, "scv_intensity_map: the batch's appearance model is %d, not SCV", b->desc.am);
	FLUSH(b);
	if (!b->d_scv_map) return fail(MTFHIP_ERR_LOGIC, "scv_intensity_map before initializePixVals");
	HIP_TRY(hipMemcpyAsync(dst, b->d_scv_map, sizeof(double) * (size_t)b->scv_nb * b->B, hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	return MTFHIP_OK;
}

} /* extern "C" */
