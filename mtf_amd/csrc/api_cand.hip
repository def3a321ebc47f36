/*
 * api_cand.hip -- candidate scoring (shared with the particle filter), candidate sampling and the NN dataset rows
 * (C-ABI implementation, include/mtfhip.h; shared declarations: mtfhip_api_internal.h; no CPU fallback: HIP kernels or an error)
 */
#include "mtfhip_api_internal.h"

extern "C" {

/* The template's own corners (set_corners lays a unit-z grid out INSIDE them: the lattice's end points are the corners), or NULL where they are
 * not the hull of the sample points: the scorer and the NN rows skip the border test of a candidate whose warped corners are inside the frame */
static const double *template_hull(const mtfhip_batch *b, double *hull_buf) {
	if (!b->unit_z || !b->grid_from_corners || b->B < 1) return nullptr;
	const double *ic = b->th[0].init_corners_hm;
	for (int q = 0; q < 4; ++q) {
		if (ic[3 * q + 2] != 1.0) return nullptr;
		hull_buf[2 * q] = ic[3 * q]; hull_buf[2 * q + 1] = ic[3 * q + 1];
	}
	return hull_buf;
}

/* ------------------------------------------------------------------ candidate scoring */
/* candidates [lo, lo + cnt) of dev_states: weight (the AM's likelihood, or PF's Gaussian / reciprocal mapping of the similarity) and
 * similarity at their global indices.  SSD / NCC (also multi-channel): k_pf_score; MI (8 bins): the histogram pass over the candidate
 * axis + k_mi_cand_score.  Shared by mtfhip_score_candidates_dev and the particle filter. */
int score_block_dev(mtfhip_batch *b, const double *dev_states, int lo, int cnt, double *wts, double *sim, int likelihood_func,
	double measurement_sigma, double max_similarity, const PfPeerPush *peer) {
	hipStream_t st = b->ctx->stream;
	if (b->desc.am == MTFHIP_AM_MI) {
		if (!(b->desc.mi_n_bins == 8 || (b->desc.mi_n_bins <= 10 && b->C == 1)))
			return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "score_candidates: MI candidates are scored with up to 10 bins (multi-channel: 8, the reference's default, parameters.h:344)");
		if (!b->init_sim) return fail(MTFHIP_ERR_LOGIC, "score_candidates before initializeSimilarity");
		const int nblk = 1;
		const size_t need = (size_t)std::max(cnt, 1) * nblk * b->mi_row_len;
		if (need > b->d_cand_mi.capacity()) {
			HIP_TRY(hipStreamSynchronize(st));
			HIP_TRY(b->d_cand_mi.reserve(need));
		}
		MiFastPlan fp;
		fp.nb = b->desc.mi_n_bins;
		fp.hk = 0; fp.hrow = 0; fp.j0_mode = 0; fp.j0_init_variant = 0; fp.need_dft = 0; fp.need_df0 = 0; fp.g_mean = 0;
		fp.grad_eps = b->desc.grad_eps; fp.norm_mult = b->norm_mult; fp.norm_add = b->norm_add; fp.hist_norm = b->mi_hist_norm;
		fp.active = nullptr; fp.tb = b->d_mi_tb;
		launch_mi_score_candidates(b->view_raw(), b->ctx->img, fp, dev_states, lo, cnt, b->d_cand_mi, nblk, b->mi_row_len, b->desc.mi_pre_seed,
			b->desc.likelihood_alpha, likelihood_func, measurement_sigma, max_similarity, wts, sim, st);
		if (peer && cnt > 0) launch_pf_peer_push(*peer, wts, lo, cnt, st);   /* (the MI scorer does not store to the peers itself) */
		return MTFHIP_OK;
	}
	const double *ncc_sc = nullptr;
	if (b->desc.am == MTFHIP_AM_NCC) {   /* mean(I0), |I0 - mean| of the template, as the un-fused NCC kernels read them */
		if (!b->init_sim) return fail(MTFHIP_ERR_LOGIC, "score_candidates before initializeSimilarity");
		TRY(push_ncc(b));
		ncc_sc = b->d_ncc;
	}
	double hull_buf[8];
	const double *hull = template_hull(b, hull_buf);
	/* (view_raw: the candidates bring their own warps; a stale device copy of the batch's warp is not uploaded for them) */
	launch_score_block(b->view_raw(), b->ctx->img, dev_states, lo, cnt, b->desc.likelihood_alpha, b->norm_mult, b->norm_add, ncc_sc, wts, sim,
		likelihood_func, measurement_sigma, max_similarity, b->math_mode == MTFHIP_MATH_FAST, peer, hull,
		(b->math_mode == MTFHIP_MATH_FAST && b->C == 1) ? pair_image_if_it_pays(b->ctx, cnt) : nullptr, st);
	return MTFHIP_OK;
}
int mtfhip_score_candidates_dev(mtfhip_batch *b, const double *dev_states, int C, double *dev_lik, double *dev_sim) {
	FLUSH_AM(b);   /* (every candidate warps the template grid itself: CURR_PTS are not read) */
	if (!b || !dev_states) return fail(MTFHIP_ERR_INVALID_ARG, "score_candidates: NULL argument");
	TRY(lowdof_refuse(b, "score_candidates"));
	TRY(am_refuse(b, "score_candidates", AM_AT_SCORE_CANDIDATES));
	if (C <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "score_candidates: n_candidates must be positive");
	if (!b->init_pix_vals) return fail(MTFHIP_ERR_LOGIC, "score_candidates before the template was initialised");
	TRY(need_image(b));
	TimedScope ts(b->ctx, "score_candidates");
	return score_block_dev(b, dev_states, 0, C, dev_lik, dev_sim, 0, 1.0, 0.0);
}

int mtfhip_score_candidates(mtfhip_batch *b, const double *states, int C, double *lik, double *sim) {
	FLUSH(b);
	if (!b || !states) return fail(MTFHIP_ERR_INVALID_ARG, "score_candidates: NULL argument");
	TRY(lowdof_refuse(b, "score_candidates"));
	TRY(am_refuse(b, "score_candidates", AM_AT_SCORE_CANDIDATES));
	if (C <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "score_candidates: n_candidates must be positive");
	size_t need = (size_t)C * (b->S + 2);
	HIP_TRY(b->d_cand.reserve(need));
	double *d_states = b->d_cand, *d_lik = b->d_cand + (size_t)C * b->S, *d_sim = d_lik + C;
	HIP_TRY(hipMemcpyAsync(d_states, states, sizeof(double) * C * b->S, hipMemcpyHostToDevice, b->ctx->stream));
	TRY(mtfhip_score_candidates_dev(b, d_states, C, d_lik, d_sim));
	if (lik) HIP_TRY(hipMemcpyAsync(lik, d_lik, sizeof(double) * C, hipMemcpyDeviceToHost, b->ctx->stream));
	if (sim) HIP_TRY(hipMemcpyAsync(sim, d_sim, sizeof(double) * C, hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	return MTFHIP_OK;
}

/* ------------------------------------------------------------------ NN dataset generation */
int mtfhip_sample_candidates_dev(mtfhip_batch *b, const double *dev_states, int C, double *dev_features) {
	FLUSH(b);
	if (!b || !dev_states || !dev_features) return fail(MTFHIP_ERR_INVALID_ARG, "sample_candidates: NULL argument");
	TRY(lowdof_refuse(b, "sample_candidates"));
	TRY(am_refuse(b, "sample_candidates", AM_AT_SAMPLE_CANDIDATES));
	if (C <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "sample_candidates: n_samples must be positive");
	if (b->desc.am == MTFHIP_AM_MI) return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "sample_candidates: MI distance features (5 x N B-spline rows) are not available");
	TRY(single_channel(b, "sample_candidates"));
	if (!b->have_corners) return fail(MTFHIP_ERR_LOGIC, "sample_candidates before set_corners");
	TRY(need_image(b));
	TimedScope ts(b->ctx, "sample_candidates");
	launch_sample_candidates(b->view_raw(), b->ctx->img, dev_states, C, b->norm_mult, b->norm_add, dev_features, b->ctx->stream);
	return MTFHIP_OK;
}
int mtfhip_sample_candidates(mtfhip_batch *b, const double *states, int C, double *features) {
	FLUSH(b);
	if (!b || !states || !features) return fail(MTFHIP_ERR_INVALID_ARG, "sample_candidates: NULL argument");
	TRY(lowdof_refuse(b, "sample_candidates"));
	TRY(am_refuse(b, "sample_candidates", AM_AT_SAMPLE_CANDIDATES));
	if (C <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "sample_candidates: n_samples must be positive");
	Dev<double> d_states, d_feat;   /* (released on every return; the release waits for what is in flight) */
	HIP_TRY(d_states.reserve((size_t)C * b->S));
	if (d_feat.reserve((size_t)C * b->N) != hipSuccess) return fail(MTFHIP_ERR_HIP, "device allocation of the %d x %d feature matrix failed", C, b->N);
	HIP_TRY(hipMemcpyAsync(d_states, states, sizeof(double) * C * b->S, hipMemcpyHostToDevice, b->ctx->stream));
	TRY(mtfhip_sample_candidates_dev(b, d_states, C, d_feat));
	HIP_TRY(hipMemcpyAsync(features, d_feat, sizeof(double) * (size_t)C * b->N, hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	return MTFHIP_OK;
}

/* NN::generateDataset (SM/src/NT/NN.cc:131-191) */
int mtfhip_nn_feature_size(mtfhip_batch *b, int *feat_size) {
	if (!b || !feat_size) return fail(MTFHIP_ERR_INVALID_ARG, "nn_feature_size: NULL argument");
	*feat_size = b->desc.am == MTFHIP_AM_MI ? 5 * b->N : b->N;   /* MI.cc:122: feat_size = 5 * patch_size; SSDBase.h:116-125, NCC.cc:530-537: patch_size */
	return MTFHIP_OK;
}
/* the launch behind mtfhip_nn_dataset_dev; base_dev / done (api_nn.hip: the query feature of the NN tracker's loop): the warp is read from
 * device memory instead of the host mirror, and the kernels return at once when *done is set */
int nn_dataset_enqueue(mtfhip_batch *b, const mtfhip_nn_desc *d, const double *dev_perturbations_in, double *dev_perturbations_out, double *dev_features,
	int row_lo, int row_count, const double *base_dev, const int *done) {
	FLUSH(b);
	if (!b || !d || !dev_features) return fail(MTFHIP_ERR_INVALID_ARG, "nn_dataset: NULL argument");
	TRY(lowdof_refuse(b, "nn_dataset"));
	TRY(am_refuse(b, "nn_dataset", AM_AT_NN_DATASET));
	if (d->n_samples <= 0 || row_lo < 0 || row_count < 0 || row_lo + row_count > d->n_samples)
		return fail(MTFHIP_ERR_INVALID_ARG, "nn_dataset: rows [%d, %d) of %d samples", row_lo, row_lo + row_count, d->n_samples);
	if (d->additive_update) return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "nn_dataset: additive_update (NNParams, NT/NN.cc:150-152): the compositional form only");
	if (!b->have_corners) return fail(MTFHIP_ERR_LOGIC, "nn_dataset before set_corners");
	if (b->B != 1) return fail(MTFHIP_ERR_INVALID_ARG, "nn_dataset: one template per batch (the batch has %d targets)", b->B);
	TRY(need_image(b));
	for (int s = 0; s < b->S; ++s) if (!(d->sigma[s] >= 0)) return fail(MTFHIP_ERR_INVALID_ARG, "nn_dataset: sigma[%d] = %g", s, d->sigma[s]);
	NnArgs a;
	a.perts_in = dev_perturbations_in; a.perts_out = dev_perturbations_out;
	a.base_dev = base_dev; a.done = done;
	for (int s = 0; s < 8; ++s) { a.sigma[s] = s < b->S ? d->sigma[s] : 0.0; a.mean[s] = s < b->S ? d->mean[s] : 0.0; }
	a.seed = d->seed;
	std::memcpy(a.base, b->th[0].warp.m, sizeof(a.base));
	a.row_lo = row_lo; a.norm_mult = b->norm_mult; a.norm_add = b->norm_add;
	double hull_buf[8];
	const double *hull = template_hull(b, hull_buf);
	/* tolerance mode: the samples' warps go through a scratch array (k_nn_warps -> k_nn_rows), grown to the largest launch so far */
	double *warps = nullptr;
	if (nn_two_launch_ok(b->view_raw(), b->ctx->img, b->math_mode == MTFHIP_MATH_FAST)) {
		const size_t need = nn_warps_bytes(row_count) / sizeof(double);
		if (need > b->d_nn_warps.capacity()) {
			HIP_TRY(hipStreamSynchronize(b->ctx->stream));
			HIP_TRY(b->d_nn_warps.reserve(need));
		}
		warps = b->d_nn_warps;
	}
	TimedScope ts(b->ctx, "nn_dataset");
	const hipError_t le = launch_nn_dataset(b->view_raw(), b->ctx->img, a, row_count, dev_features, warps, hull, b->ctx->stream);
	if (le != hipSuccess) return fail(MTFHIP_ERR_HIP, "nn_dataset: the row kernel could not be set up: %s", hipGetErrorString(le));
	return launch_error_pending();   /* a launch the runtime refused (its dynamic LDS, its grid) is this call's error, not a later one's */
}
int mtfhip_nn_dataset_dev(mtfhip_batch *b, const mtfhip_nn_desc *d, const double *dev_perturbations_in, double *dev_perturbations_out, double *dev_features,
	int row_lo, int row_count) {
	return nn_dataset_enqueue(b, d, dev_perturbations_in, dev_perturbations_out, dev_features, row_lo, row_count, nullptr, nullptr);
}
int mtfhip_nn_dataset(mtfhip_batch *b, const mtfhip_nn_desc *d, const double *perturbations_in, double *perturbations_out, double *features) {
	if (!b || !d || !features) return fail(MTFHIP_ERR_INVALID_ARG, "nn_dataset: NULL argument");
	TRY(lowdof_refuse(b, "nn_dataset"));
	TRY(am_refuse(b, "nn_dataset", AM_AT_NN_DATASET));
	if (d->n_samples <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "nn_dataset: n_samples must be positive");
	int F = 0;
	TRY(mtfhip_nn_feature_size(b, &F));
	const size_t C = (size_t)d->n_samples;
	Dev<double> d_p, d_feat;   /* (released on every return; the release waits for what is in flight) */
	HIP_TRY(d_p.reserve(C * b->S));
	if (d_feat.reserve(C * F) != hipSuccess) return fail(MTFHIP_ERR_HIP, "device allocation of the %d x %d feature matrix failed", d->n_samples, F);
	hipStream_t st = b->ctx->stream;
	if (perturbations_in) HIP_TRY(hipMemcpyAsync(d_p, perturbations_in, sizeof(double) * C * b->S, hipMemcpyHostToDevice, st));
	TRY(mtfhip_nn_dataset_dev(b, d, perturbations_in ? d_p.get() : nullptr, d_p, d_feat, 0, d->n_samples));
	if (perturbations_out) HIP_TRY(hipMemcpyAsync(perturbations_out, d_p, sizeof(double) * C * b->S, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(features, d_feat, sizeof(double) * C * F, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return MTFHIP_OK;
}

} /* extern "C" */
