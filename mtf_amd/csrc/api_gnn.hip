/*
 * api_gnn.hip -- nt::NN's graph index gnn::GNN over a mtfhip_nn handle's resident dataset (SM/src/NT/GNN.cc:30-241; C-ABI implementation,
 * include/mtfhip.h; the kernels: kernels_gnn.hip)
 */
#include "mtfhip_api_internal.h"
#include "mtfhip_nn_handle.h"

namespace {
constexpr size_t kGnnScratchBytes = (size_t)256 << 20;   /* the panel of distances a build keeps at a time */

int gnn_handle(const mtfhip_nn *nn, const char *fn) {
	if (!nn) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL handle", fn);
	return MTFHIP_OK;
}
/* GNN's constructor (GNN.cc:15-19), then at most n_samples - 1: see include/mtfhip.h */
int gnn_effective_degree(int degree, int n) {
	if (degree == 0 || degree > n) degree = n;
	else if (degree < 0) degree = -n / degree;
	return degree > n - 1 ? n - 1 : degree;
}
int gnn_check_desc(const mtfhip_nn *nn, const mtfhip_gnn_desc *d, const char *fn, int *degree) {
	if (!d) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);
	if (d->max_steps < 0) return fail(MTFHIP_ERR_INVALID_ARG, "%s: max_steps %d is negative", fn, d->max_steps);
	const int deg = gnn_effective_degree(d->degree, nn->n);
	if (deg + 1 > kGnnMaxList)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: degree %d (effective %d): the degree + 1 nearest rows of a node are sorted in LDS, at most %d", fn,
			d->degree, deg, (int)kGnnMaxList);
	*degree = deg;
	return MTFHIP_OK;
}
/* the start node and the search count: made with the handle's first GNN call, start node 0 */
int gnn_ensure_ctl(mtfhip_nn *nn) {
	NnGraph &g = nn->g;
	if (g.d_count) return MTFHIP_OK;
	HIP_TRY(g.d_count.reserve(2));
	g.d_start = reinterpret_cast<int *>(g.d_count + 1);
	const hipError_t e = hipMemsetAsync(g.d_count, 0, 16, nn->b->ctx->stream);
	if (e != hipSuccess) { g.d_count.reset(); g.d_start = nullptr; }   /* (not zeroed is not there: the next call starts over) */
	HIP_TRY(e);
	return MTFHIP_OK;
}
int gnn_ensure_graph(mtfhip_nn *nn, int degree) {
	NnGraph &g = nn->g;
	const size_t want = (size_t)nn->n * (size_t)(degree > 0 ? degree : 1);
	if (want > g.d_graph.capacity()) {
		HIP_TRY(hipStreamSynchronize(nn->b->ctx->stream));
		HIP_TRY(g.d_graph.reserve(want));
	}
	return MTFHIP_OK;
}
int gnn_ensure_walks(mtfhip_nn *nn, int Q) {
	NnGraph &g = nn->g;
	const size_t nq = (size_t)Q, part = nq * g.nper;
	if (nq <= g.d_walks.capacity() && part <= g.d_part.capacity() && nq <= g.d_tickets.capacity()) return MTFHIP_OK;
	HIP_TRY(hipStreamSynchronize(nn->b->ctx->stream));
	HIP_TRY(g.d_walks.reserve(nq));
	HIP_TRY(g.d_part.reserve(part));
	if (nq > g.d_tickets.capacity()) {   /* the tickets return to zero behind every walk: zeroed once, when they are allocated */
		HIP_TRY(g.d_tickets.reserve(nq));
		const hipError_t e = hipMemsetAsync(g.d_tickets, 0, sizeof(unsigned) * nq, nn->b->ctx->stream);
		if (e != hipSuccess) g.d_tickets.reset();   /* (not zeroed is not there: the next call starts over) */
		HIP_TRY(e);
	}
	return MTFHIP_OK;
}
void gnn_adopt(mtfhip_nn *nn, const mtfhip_gnn_desc *d, int degree) {
	NnGraph &g = nn->g;
	g.desc = *d; g.degree = degree; g.nper = gnn_step_blocks(degree); g.valid = true;
}
/* searchGraph (GNN.cc:115-203) for Q queries side by side: the start nodes, their distances, max_steps steps, all enqueued back to back */
void gnn_enqueue_walks(mtfhip_nn *nn, const double *dev_queries, int Q, const int *dev_start_nodes, const int *d_done) {
	NnGraph &g = nn->g;
	hipStream_t st = nn->b->ctx->stream;
	launch_gnn_init(g.d_walks, Q, dev_start_nodes, g.d_start, g.desc.random_start, g.desc.seed, g.d_count, nn->n, d_done, st);
	TimedScope ts(nn->b->ctx, "gnn_walk");
	launch_gnn_rows(nn->ncc, nn->d_feat, nn->n, nn->F, dev_queries, Q, g.d_graph, g.degree, g.d_walks, g.d_part, g.d_tickets, 1, g.desc.max_steps, 1, d_done, st);
	if (g.degree <= 0) return;
	for (int s = 0; s < g.desc.max_steps; ++s)
		launch_gnn_rows(nn->ncc, nn->d_feat, nn->n, nn->F, dev_queries, Q, g.d_graph, g.degree, g.d_walks, g.d_part, g.d_tickets, g.nper, g.desc.max_steps, 0, d_done, st);
}
} // namespace

int gnn_need_graph(const mtfhip_nn *nn, const char *fn) {
	if (!nn->g.valid) return fail(MTFHIP_ERR_LOGIC, "%s with the GNN index before nn_gnn_build / nn_gnn_set_graph (a new dataset invalidates the graph)", fn);
	return MTFHIP_OK;
}
int gnn_prepare_update(mtfhip_nn *nn, int max_iters) {
	NnGraph &g = nn->g;
	TRY(gnn_ensure_ctl(nn));
	TRY(gnn_ensure_walks(nn, 1));
	g.last_walks.clear();
	return MTFHIP_OK;
}
int gnn_enqueue_update_walk(mtfhip_nn *nn, int it, const int *d_done) {
	NnGraph &g = nn->g;
	gnn_enqueue_walks(nn, nn->d_query, 1, nullptr, d_done);
	launch_gnn_to_update(g.d_walks, nn->d_part, g.d_start, nn_walk_log(nn), it, d_done, nn->b->ctx->stream);
	return launch_error_pending();
}
void gnn_finish_update(mtfhip_nn *nn, const int *walk_log, int ran) {
	nn->g.last_walks.assign(walk_log, walk_log + 2 * (size_t)(ran > 0 ? ran : 0));
}

extern "C" {

int mtfhip_nn_gnn_build(mtfhip_nn *nn, const mtfhip_gnn_desc *d) {
	TRY(gnn_handle(nn, "nn_gnn_build"));
	int degree = 0;
	TRY(gnn_check_desc(nn, d, "nn_gnn_build", &degree));
	if (!nn->have_dataset) return fail(MTFHIP_ERR_LOGIC, "nn_gnn_build before nn_build / nn_set_dataset");
	HIP_TRY(hipSetDevice(nn->device));
	nn->g.valid = false;
	TRY(gnn_ensure_ctl(nn));
	TRY(gnn_ensure_graph(nn, degree));
	if (degree > 0) {
		/* the panel: as many rows of distances as the scratch budget holds (whole 64-row blocks where it holds that many); never n x n */
		size_t budget = kGnnScratchBytes;
		if (const char *e = std::getenv("MTFHIP_GNN_SCRATCH_BYTES")) {   /* (for the tests of the panel seam) */
			const long long v = std::atoll(e);
			if (v > 0) budget = (size_t)v;
		}
		size_t P = budget / (sizeof(double) * (size_t)nn->n);
		if (P >= (size_t)kGnnTile) P -= P % kGnnTile;
		if (P < 1) P = 1;
		if (P > (size_t)nn->n) P = (size_t)nn->n;
		if (P > 65535u * (size_t)kGnnTile) P = 65535u * (size_t)kGnnTile;
		Dev<double> scratch;
		if (scratch.reserve(P * (size_t)nn->n) != hipSuccess)
			return fail(MTFHIP_ERR_HIP, "nn_gnn_build: device allocation of the %zu x %d distance panel failed", P, nn->n);
		hipStream_t st = nn->b->ctx->stream;
		{
			TimedScope ts(nn->b->ctx, "gnn_build");
			for (size_t lo = 0; lo < (size_t)nn->n; lo += P) {
				const int rows = (int)((size_t)nn->n - lo < P ? (size_t)nn->n - lo : P);
				launch_gnn_dist(nn->ncc, nn->d_feat, nn->n, nn->F, (int)lo, rows, scratch, st);
				launch_gnn_select(scratch, nn->n, (int)lo, rows, degree, nn->g.d_graph, st);
			}
		}
		HIP_TRY(hipStreamSynchronize(st));
		TRY(launch_error_pending());
	}
	gnn_adopt(nn, d, degree);
	return MTFHIP_OK;
}

int mtfhip_nn_gnn_get_graph(mtfhip_nn *nn, int *degree, int *nns_inds) {
	TRY(gnn_handle(nn, "nn_gnn_get_graph"));
	TRY(gnn_need_graph(nn, "nn_gnn_get_graph"));
	if (degree) *degree = nn->g.degree;
	if (nns_inds && nn->g.degree > 0) {
		hipStream_t st = nn->b->ctx->stream;
		HIP_TRY(hipMemcpyAsync(nns_inds, nn->g.d_graph, sizeof(int) * (size_t)nn->n * nn->g.degree, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	return MTFHIP_OK;
}

int mtfhip_nn_gnn_set_graph(mtfhip_nn *nn, const mtfhip_gnn_desc *d, const int *nns_inds) {
	TRY(gnn_handle(nn, "nn_gnn_set_graph"));
	int degree = 0;
	TRY(gnn_check_desc(nn, d, "nn_gnn_set_graph", &degree));
	if (!nn->have_dataset) return fail(MTFHIP_ERR_LOGIC, "nn_gnn_set_graph before nn_build / nn_set_dataset");
	if (degree > 0 && !nns_inds) return fail(MTFHIP_ERR_INVALID_ARG, "nn_gnn_set_graph: NULL argument");
	for (size_t k = 0; k < (size_t)nn->n * (size_t)degree; ++k)
		if (nns_inds[k] < 0 || nns_inds[k] >= nn->n)
			return fail(MTFHIP_ERR_INVALID_ARG, "nn_gnn_set_graph: entry %zu is %d, not a row of the %d", k, nns_inds[k], nn->n);
	HIP_TRY(hipSetDevice(nn->device));
	nn->g.valid = false;
	TRY(gnn_ensure_ctl(nn));
	TRY(gnn_ensure_graph(nn, degree));
	if (degree > 0) {
		hipStream_t st = nn->b->ctx->stream;
		HIP_TRY(hipMemcpyAsync(nn->g.d_graph, nns_inds, sizeof(int) * (size_t)nn->n * degree, hipMemcpyHostToDevice, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	gnn_adopt(nn, d, degree);
	return MTFHIP_OK;
}

int mtfhip_nn_gnn_search_dev(mtfhip_nn *nn, const double *dev_queries, int n_queries, const int *dev_start_nodes, int *dev_idx, double *dev_dist,
	int *dev_n_steps) {
	TRY(gnn_handle(nn, "nn_gnn_search_dev"));
	if (n_queries <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "nn_gnn_search_dev: n_queries must be positive");
	if (n_queries > 65535) return fail(MTFHIP_ERR_INVALID_ARG, "nn_gnn_search_dev: at most 65535 queries per call");
	if (!dev_queries || !dev_idx || !dev_dist) return fail(MTFHIP_ERR_INVALID_ARG, "nn_gnn_search_dev: NULL argument");
	if (!nn->have_dataset) return fail(MTFHIP_ERR_LOGIC, "nn_gnn_search_dev before nn_build / nn_set_dataset");
	TRY(gnn_need_graph(nn, "nn_gnn_search_dev"));
	TRY(gnn_ensure_walks(nn, n_queries));
	gnn_enqueue_walks(nn, dev_queries, n_queries, dev_start_nodes, nullptr);
	launch_gnn_results(nn->g.d_walks, n_queries, dev_idx, dev_dist, dev_n_steps, nn->b->ctx->stream);
	return launch_error_pending();
}

int mtfhip_nn_gnn_search(mtfhip_nn *nn, const double *queries, int n_queries, const int *start_nodes, int *idx, double *dist, int *n_steps) {
	TRY(gnn_handle(nn, "nn_gnn_search"));
	if (n_queries <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "nn_gnn_search: n_queries must be positive");
	if (!queries || !idx || !dist) return fail(MTFHIP_ERR_INVALID_ARG, "nn_gnn_search: NULL argument");
	if (!nn->have_dataset) return fail(MTFHIP_ERR_LOGIC, "nn_gnn_search before nn_build / nn_set_dataset");
	TRY(gnn_need_graph(nn, "nn_gnn_search"));
	if (start_nodes)
		for (int q = 0; q < n_queries; ++q)
			if (start_nodes[q] < 0 || start_nodes[q] >= nn->n)
				return fail(MTFHIP_ERR_INVALID_ARG, "nn_gnn_search: start node %d of query %d is not a row of the %d", start_nodes[q], q, nn->n);
	NnGraph &g = nn->g;
	hipStream_t st = nn->b->ctx->stream;
	const size_t Q = (size_t)n_queries;
	/* (every member is asked: one that a failed grow left empty is allocated again whatever the others hold) */
	if (Q * nn->F > g.d_q.capacity() || Q > g.d_starts.capacity() || Q > g.d_idx.capacity() || Q > g.d_steps.capacity() || Q > g.d_dist.capacity())
		HIP_TRY(hipStreamSynchronize(st));   /* what is about to be released may still be read */
	HIP_TRY(g.d_q.reserve(Q * nn->F));
	HIP_TRY(g.d_starts.reserve(Q));
	HIP_TRY(g.d_idx.reserve(Q));
	HIP_TRY(g.d_steps.reserve(Q));
	HIP_TRY(g.d_dist.reserve(Q));
	HIP_TRY(hipMemcpyAsync(g.d_q, queries, sizeof(double) * (size_t)n_queries * nn->F, hipMemcpyHostToDevice, st));
	if (start_nodes) HIP_TRY(hipMemcpyAsync(g.d_starts, start_nodes, sizeof(int) * (size_t)n_queries, hipMemcpyHostToDevice, st));
	TRY(mtfhip_nn_gnn_search_dev(nn, g.d_q, n_queries, start_nodes ? g.d_starts.get() : nullptr, g.d_idx, g.d_dist, g.d_steps));
	HIP_TRY(hipMemcpyAsync(idx, g.d_idx, sizeof(int) * (size_t)n_queries, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(dist, g.d_dist, sizeof(double) * (size_t)n_queries, hipMemcpyDeviceToHost, st));
	if (n_steps) HIP_TRY(hipMemcpyAsync(n_steps, g.d_steps, sizeof(int) * (size_t)n_queries, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return MTFHIP_OK;
}

int mtfhip_nn_set_index(mtfhip_nn *nn, int index_type) {
	TRY(gnn_handle(nn, "nn_set_index"));
	if (index_type != MTFHIP_NN_INDEX_EXACT && index_type != MTFHIP_NN_INDEX_GNN)
		return fail(MTFHIP_ERR_INVALID_ARG, "nn_set_index: index type %d", index_type);
	nn->g.index_type = index_type;
	return MTFHIP_OK;
}

int mtfhip_nn_gnn_set_start(mtfhip_nn *nn, int node) {
	TRY(gnn_handle(nn, "nn_gnn_set_start"));
	if (node < 0 || node >= nn->n) return fail(MTFHIP_ERR_INVALID_ARG, "nn_gnn_set_start: node %d is not a row of the %d", node, nn->n);
	HIP_TRY(hipSetDevice(nn->device));
	TRY(gnn_ensure_ctl(nn));
	hipStream_t st = nn->b->ctx->stream;
	HIP_TRY(hipMemcpyAsync(nn->g.d_start, &node, sizeof(int), hipMemcpyHostToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));
	return MTFHIP_OK;
}

int mtfhip_nn_gnn_get_start(mtfhip_nn *nn, int *node) {
	TRY(gnn_handle(nn, "nn_gnn_get_start"));
	if (!node) return fail(MTFHIP_ERR_INVALID_ARG, "nn_gnn_get_start: NULL argument");
	*node = 0;
	if (!nn->g.d_count) return MTFHIP_OK;
	hipStream_t st = nn->b->ctx->stream;
	HIP_TRY(hipMemcpyAsync(node, nn->g.d_start, sizeof(int), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return MTFHIP_OK;
}

int mtfhip_nn_gnn_last_walks(mtfhip_nn *nn, int *start_nodes, int *n_steps) {
	TRY(gnn_handle(nn, "nn_gnn_last_walks"));
	const std::vector<int> &w = nn->g.last_walks;
	for (size_t k = 0; k < w.size() / 2; ++k) {
		if (start_nodes) start_nodes[k] = w[2 * k];
		if (n_steps) n_steps[k] = w[2 * k + 1];
	}
	return MTFHIP_OK;
}

} /* extern "C" */
