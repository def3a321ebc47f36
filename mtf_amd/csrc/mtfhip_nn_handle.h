/*
 * mtfhip_nn_handle.h -- the mtfhip_nn handle, shared by the two units that implement its entry points: api_nn.hip (the dataset, the exhaustive
 * search, NN::update) and api_gnn.hip (the graph index gnn::GNN: build, walk, and the walk inside NN::update).
 */
#pragma once
#include "mtfhip_api_internal.h"
#include <vector>

namespace {
constexpr int kNnStateDoubles = 40;   /* W 9 | corners 8 | init_corners_hm 12 | the zero perturbation 8 | pad 3 */
constexpr int kNnZeroPert = 29;
}

/* the graph index of a handle (api_gnn.hip) */
struct NnGraph {
	int index_type = MTFHIP_NN_INDEX_EXACT;   /* what mtfhip_nn_update searches with */
	bool valid = false;                       /* a graph of the CURRENT dataset is resident */
	mtfhip_gnn_desc desc{};                   /* as given; `degree` below is the effective one */
	int degree = 0, nper = 1;                 /* neighbours per node | workgroups of a step launch per walk */
	Dev<int> d_graph;                         /* [n][degree] */
	Dev<unsigned long long> d_count;          /* [2] device: searches begun (what random_start's draws are keyed by), then the start node (an int) */
	int *d_start = nullptr;                   /* a view: the second word of d_count */
	Dev<GnnWalk> d_walks; Dev<NnBest> d_part; Dev<unsigned> d_tickets;
	std::vector<int> last_walks;                            /* of the last update(): start, steps per iteration run */
	Dev<double> d_q, d_dist; Dev<int> d_starts, d_idx, d_steps;   /* staging of the host form of the search */
};

struct mtfhip_nn {
	mtfhip_batch *b = nullptr;
	int device = 0;                       /* (destroy does not reach through the batch: it may be gone) */
	int n = 0, F = 0, S = 0, ncc = 0;
	bool host_stepped = false, have_dataset = false;
	int resident = 0, nblk = 0;           /* workgroups of a search launch */
	Dev<double> d_feat, d_perts;
	Dev<NnBest> d_part;                   /* [queries][nblk] */
	Dev<double> d_query;                  /* the tracker's query feature, feat_size */
	/* W | corners | init_corners_hm | zero perturbation | pad, then ctl (done, n_iters: two ints in one double's place), then the log
	 * (log_cap x 3), then the GNN walks' log (log_cap x two ints: start node, steps): one read-back brings all of it */
	Dev<double> d_state; int log_cap = 0;
	Dev<double> d_q, d_dist; Dev<int> d_idx;   /* staging of the host form of the search */
	NnGraph g;
};

static inline int *nn_walk_log(const mtfhip_nn *nn) { return reinterpret_cast<int *>(nn->d_state + kNnStateDoubles + 1 + 3 * (size_t)nn->log_cap); }

/* api_gnn.hip, for mtfhip_nn_update and the handle's life cycle */
int gnn_need_graph(const mtfhip_nn *nn, const char *fn);    /* MTFHIP_ERR_LOGIC without a valid graph */
int gnn_prepare_update(mtfhip_nn *nn, int max_iters);       /* the walk's buffers, before the first launch of an update */
/* iteration `it` of NN::update with the graph index: the walk from the handle's start node for nn->d_query, its result as the one partial
 * (nn->d_part[0]) that k_nn_pick_update reads */
int gnn_enqueue_update_walk(mtfhip_nn *nn, int it, const int *d_done);
void gnn_finish_update(mtfhip_nn *nn, const int *walk_log, int ran);   /* keeps the walks' log of the `ran` iterations run (read back with the state block) */
