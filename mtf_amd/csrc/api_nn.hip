/*
 * api_nn.hip -- mtfhip_nn: nt::NN's per-frame half (SM/src/NT/NN.cc:236-277) over a dataset resident on the device (C-ABI implementation,
 * include/mtfhip.h; the kernels: kernels_nn_search.hip, and kernels_nn.hip for the query feature)
 */
#include "mtfhip_api_internal.h"
#include "mtfhip_nn_handle.h"

static int nn_ensure_partials(mtfhip_nn *nn, int Q) {
	const size_t need = (size_t)Q * nn->nblk;
	if (need <= nn->d_part.capacity()) return MTFHIP_OK;
	HIP_TRY(hipStreamSynchronize(nn->b->ctx->stream));
	HIP_TRY(nn->d_part.reserve(need));
	return MTFHIP_OK;
}
static int nn_ensure_state(mtfhip_nn *nn, int max_iters) {
	if (nn->d_state && max_iters <= nn->log_cap) return MTFHIP_OK;
	HIP_TRY(hipStreamSynchronize(nn->b->ctx->stream));
	nn->d_state.reset(); nn->log_cap = 0;   /* (log_cap is the block's layout, not only its size: nn_walk_log) */
	HIP_TRY(nn->d_state.reserve(kNnStateDoubles + 1 + 4 * (size_t)max_iters));
	nn->log_cap = max_iters;
	return MTFHIP_OK;
}
static int nn_usable(const mtfhip_nn *nn, const char *fn) {
	if (!nn) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL handle", fn);
	return MTFHIP_OK;
}
static int nn_need_dataset(const mtfhip_nn *nn, const char *fn) {
	if (!nn->have_dataset) return fail(MTFHIP_ERR_LOGIC, "%s before nn_build / nn_set_dataset", fn);
	return MTFHIP_OK;
}

extern "C" {

int mtfhip_nn_create(mtfhip_batch *b, int n_samples, mtfhip_nn **out) {
	if (!b || !out) return fail(MTFHIP_ERR_INVALID_ARG, "nn_create: NULL argument");
	*out = nullptr;
	TRY(lowdof_refuse(b, "nn_create"));
	TRY(am_refuse(b, "nn_create", AM_AT_NN_CREATE));
	if (n_samples <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "nn_create: n_samples must be positive");
	if (b->B != 1) return fail(MTFHIP_ERR_INVALID_ARG, "nn_create: one template per batch (the batch has %d targets)", b->B);
	if (b->desc.am == MTFHIP_AM_MI)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "nn_create: MI is not available on the NN search (MIDist, MI.cc:749, is a joint histogram per dataset row)");
	int F = 0;
	TRY(mtfhip_nn_feature_size(b, &F));
	if (F > kNnSearchMaxFeat)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "nn_create: feat_size %d exceeds %d, what the search's LDS staging of the query holds", F, (int)kNnSearchMaxFeat);
	HIP_TRY(hipSetDevice(b->ctx->device));
	mtfhip_nn *nn = new mtfhip_nn();
	nn->b = b; nn->device = b->ctx->device; nn->n = n_samples; nn->F = F; nn->S = b->S; nn->ncc = b->desc.am == MTFHIP_AM_NCC ? 1 : 0;
	const char *hs = std::getenv("MTFHIP_NN_HOST_STEPPED");
	nn->host_stepped = hs && hs[0] == '1';
	nn->resident = nn_search_resident(nn->ncc, F);
	nn->nblk = nn_search_blocks(n_samples, nn->resident);
	auto cleanup = [&](int rc) { (void)mtfhip_nn_destroy(nn); return rc; };
	if (nn->d_feat.reserve((size_t)n_samples * F) != hipSuccess)
		return cleanup(fail(MTFHIP_ERR_HIP, "nn_create: device allocation of the %d x %d feature matrix failed", n_samples, F));
	if (nn->d_perts.reserve((size_t)n_samples * nn->S) != hipSuccess || nn->d_query.reserve((size_t)F) != hipSuccess)
		return cleanup(fail(MTFHIP_ERR_HIP, "nn_create: device allocation failed"));
	int rc = nn_ensure_partials(nn, 1);
	if (rc == MTFHIP_OK) rc = nn_ensure_state(nn, 8);
	if (rc != MTFHIP_OK) return cleanup(rc);
	*out = nn;
	return MTFHIP_OK;
}

int mtfhip_nn_destroy(mtfhip_nn *nn) {
	if (!nn) return fail(MTFHIP_ERR_INVALID_ARG, "nn_destroy: NULL handle");
	try {
		if (hipSetDevice(nn->device) == hipSuccess) (void)hipDeviceSynchronize();
		delete nn;   /* the members, the graph index's included, release what they own */
	} catch (...) {
	}
	return MTFHIP_OK;
}

int mtfhip_nn_build(mtfhip_nn *nn, const mtfhip_nn_desc *desc, int n_distr) {
	TRY(nn_usable(nn, "nn_build"));
	if (!desc || n_distr <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "nn_build: no distribution given");
	long total = 0;
	for (int k = 0; k < n_distr; ++k) {
		if (desc[k].additive_update) return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "nn_build: additive_update (NNParams, NT/NN.cc:255-257): the compositional form only");
		if (desc[k].n_samples < 0) return fail(MTFHIP_ERR_INVALID_ARG, "nn_build: distribution %d has %d samples", k, desc[k].n_samples);
		total += desc[k].n_samples;
	}
	if (total != nn->n) return fail(MTFHIP_ERR_INVALID_ARG, "nn_build: the distributions hold %ld samples, the handle %d", total, nn->n);
	nn->have_dataset = false; nn->g.valid = false;   /* (a graph belongs to the rows it was built over) */
	size_t lo = 0;
	for (int k = 0; k < n_distr; ++k) {
		const int cnt = desc[k].n_samples;
		if (cnt == 0) continue;
		/* (the kernel indexes the perturbations by the sample's index in ITS distribution: block k's land behind the rows before it) */
		TRY(nn_dataset_enqueue(nn->b, &desc[k], nullptr, nn->d_perts + lo * nn->S, nn->d_feat + lo * nn->F, 0, cnt, nullptr, nullptr));
		lo += (size_t)cnt;
	}
	nn->have_dataset = true;
	return MTFHIP_OK;
}

int mtfhip_nn_set_dataset_dev(mtfhip_nn *nn, const double *dev_features, const double *dev_perturbations) {
	TRY(nn_usable(nn, "nn_set_dataset_dev"));
	if (!dev_features || !dev_perturbations) return fail(MTFHIP_ERR_INVALID_ARG, "nn_set_dataset_dev: NULL argument");
	hipStream_t st = nn->b->ctx->stream;
	nn->g.valid = false;
	HIP_TRY(hipMemcpyAsync(nn->d_feat, dev_features, sizeof(double) * (size_t)nn->n * nn->F, hipMemcpyDeviceToDevice, st));
	HIP_TRY(hipMemcpyAsync(nn->d_perts, dev_perturbations, sizeof(double) * (size_t)nn->n * nn->S, hipMemcpyDeviceToDevice, st));
	nn->have_dataset = true;
	return MTFHIP_OK;
}
int mtfhip_nn_set_dataset(mtfhip_nn *nn, const double *features, const double *perturbations) {
	TRY(nn_usable(nn, "nn_set_dataset"));
	if (!features || !perturbations) return fail(MTFHIP_ERR_INVALID_ARG, "nn_set_dataset: NULL argument");
	hipStream_t st = nn->b->ctx->stream;
	nn->g.valid = false;
	HIP_TRY(hipMemcpyAsync(nn->d_feat, features, sizeof(double) * (size_t)nn->n * nn->F, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(nn->d_perts, perturbations, sizeof(double) * (size_t)nn->n * nn->S, hipMemcpyHostToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));   /* the caller's arrays are free again */
	nn->have_dataset = true;
	return MTFHIP_OK;
}
int mtfhip_nn_get_dataset_dev(mtfhip_nn *nn, double *dev_features, double *dev_perturbations) {
	TRY(nn_usable(nn, "nn_get_dataset_dev"));
	TRY(nn_need_dataset(nn, "nn_get_dataset_dev"));
	hipStream_t st = nn->b->ctx->stream;
	if (dev_features) HIP_TRY(hipMemcpyAsync(dev_features, nn->d_feat, sizeof(double) * (size_t)nn->n * nn->F, hipMemcpyDeviceToDevice, st));
	if (dev_perturbations) HIP_TRY(hipMemcpyAsync(dev_perturbations, nn->d_perts, sizeof(double) * (size_t)nn->n * nn->S, hipMemcpyDeviceToDevice, st));
	return MTFHIP_OK;
}
int mtfhip_nn_get_dataset(mtfhip_nn *nn, double *features, double *perturbations) {
	TRY(nn_usable(nn, "nn_get_dataset"));
	TRY(nn_need_dataset(nn, "nn_get_dataset"));
	hipStream_t st = nn->b->ctx->stream;
	if (features) HIP_TRY(hipMemcpyAsync(features, nn->d_feat, sizeof(double) * (size_t)nn->n * nn->F, hipMemcpyDeviceToHost, st));
	if (perturbations) HIP_TRY(hipMemcpyAsync(perturbations, nn->d_perts, sizeof(double) * (size_t)nn->n * nn->S, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return MTFHIP_OK;
}

int mtfhip_nn_search_dev(mtfhip_nn *nn, const double *dev_queries, int n_queries, int *dev_idx, double *dev_dist) {
	TRY(nn_usable(nn, "nn_search_dev"));
	if (n_queries <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "nn_search_dev: n_queries must be positive");
	if (n_queries > 65535) return fail(MTFHIP_ERR_INVALID_ARG, "nn_search_dev: at most 65535 queries per call");
	if (!dev_queries || !dev_idx || !dev_dist) return fail(MTFHIP_ERR_INVALID_ARG, "nn_search_dev: NULL argument");
	TRY(nn_need_dataset(nn, "nn_search_dev"));
	TRY(nn_ensure_partials(nn, n_queries));
	hipStream_t st = nn->b->ctx->stream;
	{
		TimedScope ts(nn->b->ctx, "nn_search");
		launch_nn_search(nn->ncc, nn->d_feat, nn->n, nn->F, dev_queries, n_queries, nn->d_part, nn->nblk, nullptr, st);
	}
	launch_nn_search_finish(nn->d_part, nn->nblk, n_queries, dev_idx, dev_dist, st);
	return launch_error_pending();
}
int mtfhip_nn_search(mtfhip_nn *nn, const double *queries, int n_queries, int *idx, double *dist) {
	TRY(nn_usable(nn, "nn_search"));
	if (n_queries <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "nn_search: n_queries must be positive");
	if (!queries || !idx || !dist) return fail(MTFHIP_ERR_INVALID_ARG, "nn_search: NULL argument");
	TRY(nn_need_dataset(nn, "nn_search"));
	hipStream_t st = nn->b->ctx->stream;
	const size_t Q = (size_t)n_queries;
	/* (every member is asked: one that a failed grow left empty is allocated again whatever the others hold) */
	if (Q * nn->F > nn->d_q.capacity() || Q > nn->d_idx.capacity() || Q > nn->d_dist.capacity())
		HIP_TRY(hipStreamSynchronize(st));   /* what is about to be released may still be read */
	HIP_TRY(nn->d_q.reserve(Q * nn->F));
	HIP_TRY(nn->d_idx.reserve(Q));
	HIP_TRY(nn->d_dist.reserve(Q));
	HIP_TRY(hipMemcpyAsync(nn->d_q, queries, sizeof(double) * (size_t)n_queries * nn->F, hipMemcpyHostToDevice, st));
	TRY(mtfhip_nn_search_dev(nn, nn->d_q, n_queries, nn->d_idx, nn->d_dist));
	HIP_TRY(hipMemcpyAsync(idx, nn->d_idx, sizeof(int) * (size_t)n_queries, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(dist, nn->d_dist, sizeof(double) * (size_t)n_queries, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return MTFHIP_OK;
}

int mtfhip_nn_update(mtfhip_nn *nn, int max_iters, double epsilon, double *corners_out, int *n_iters, double *log_out) {
	TRY(nn_usable(nn, "nn_update"));
	if (max_iters <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "nn_update: max_iters must be positive");
	if (!corners_out || !n_iters) return fail(MTFHIP_ERR_INVALID_ARG, "nn_update: NULL argument");
	TRY(nn_need_dataset(nn, "nn_update"));
	const bool gnn = nn->g.index_type == MTFHIP_NN_INDEX_GNN;
	if (gnn) TRY(gnn_need_graph(nn, "nn_update"));
	mtfhip_batch *b = nn->b;
	FLUSH(b);
	if (!b->have_corners) return fail(MTFHIP_ERR_LOGIC, "nn_update before set_corners");
	TRY(need_image(b));
	TRY(nn_ensure_state(nn, max_iters));
	if (gnn) TRY(gnn_prepare_update(nn, max_iters));
	hipStream_t st = b->ctx->stream;
	TargetHost &h = b->th[0];
	/* the state block goes up from the host mirrors: the batch's SSM may have been moved by any other entry point since the last frame */
	std::vector<double> up(kNnStateDoubles + 1, 0.0), down(kNnStateDoubles + 1 + (gnn ? 3 * (size_t)nn->log_cap + (size_t)max_iters : 3 * (size_t)max_iters));
	std::memcpy(&up[0], h.warp.m, sizeof(double) * 9);
	std::memcpy(&up[9], h.corners, sizeof(double) * 8);
	std::memcpy(&up[17], h.init_corners_hm, sizeof(double) * 12);
	HIP_TRY(hipMemcpyAsync(nn->d_state, up.data(), sizeof(double) * up.size(), hipMemcpyHostToDevice, st));
	int *d_ctl = reinterpret_cast<int *>(nn->d_state + kNnStateDoubles);
	double *d_log = nn->d_state + kNnStateDoubles + 1;
	mtfhip_nn_desc qd{};   /* the query feature: one sample, the zero perturbation (given, so nothing is drawn) */
	qd.n_samples = 1;
	auto iteration = [&](int it) -> int {
		TRY(nn_dataset_enqueue(b, &qd, nn->d_state + kNnZeroPert, nullptr, nn->d_query, 0, 1, nn->d_state, d_ctl));
		if (gnn) TRY(gnn_enqueue_update_walk(nn, it, d_ctl));   /* searchGraph (NT/NN.cc:250-251) -> the one partial the pick reads */
		else {
			TimedScope ts(b->ctx, "nn_search");
			launch_nn_search(nn->ncc, nn->d_feat, nn->n, nn->F, nn->d_query, 1, nn->d_part, nn->nblk, d_ctl, st);
		}
		launch_nn_pick_update(b->desc.ssm, nn->d_part, gnn ? 1 : nn->nblk, nn->d_perts, nn->n, nn->d_state, d_ctl, d_log, it, epsilon, st);
		return launch_error_pending();
	};
	if (nn->host_stepped) {
		for (int it = 0; it < max_iters; ++it) {
			TRY(iteration(it));
			int ctl[2] = {0, 0};
			HIP_TRY(hipMemcpyAsync(ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			if (ctl[0]) break;
		}
	} else {
		for (int it = 0; it < max_iters; ++it) TRY(iteration(it));
	}
	HIP_TRY(hipMemcpyAsync(down.data(), nn->d_state, sizeof(double) * down.size(), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	int ctl[2];
	std::memcpy(ctl, &down[kNnStateDoubles], sizeof(ctl));
	const int ran = ctl[1];
	if (gnn) gnn_finish_update(nn, reinterpret_cast<const int *>(&down[kNnStateDoubles + 1 + 3 * (size_t)nn->log_cap]), ran < max_iters ? ran : max_iters);
	/* the batch's SSM follows: mirrors from the device's warp and corners, the device copy of the batch refreshed as after compositionalUpdate */
	++b->lz.epoch;
	std::memcpy(h.warp.m, &down[0], sizeof(double) * 9);
	state_from_warp(b->desc.ssm, h.state, h.warp);
	std::memcpy(h.corners, &down[9], sizeof(double) * 8);
	b->fresh_reinit = false;
	if (b->inline_warp_ok) b->warps_dirty = true;
	else TRY(push_warps(b));
	b->pts_stale = true;
	std::memcpy(corners_out, h.corners, sizeof(double) * 8);
	*n_iters = ran;
	if (log_out) std::memcpy(log_out, &down[kNnStateDoubles + 1], sizeof(double) * 3 * (size_t)(ran < max_iters ? ran : max_iters));
	return MTFHIP_OK;
}

} /* extern "C" */
