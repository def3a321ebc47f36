/*
 * NNParams.h -- the parameters of nt::NN (SM/include/mtf/SM/NNParams.h, defaults SM/src/NNParams.cc:6-18) with the reference's field names,
 * for mtf::hip::NN.  index_type selects the exhaustive search on the device (the default: what FLANN's Linear index computes) or the
 * reference's own graph index gnn::GNN with `gnn` (GNNParams.h); FLANN's other index parameters and the index files have no
 * counterpart.  additive_update defaults to true in the reference (NNParams.cc:10); the device path implements the compositional form
 * only, so the default here is false and hip::NN refuses true.
 */
#ifndef MTF_AMD_HOST_NN_PARAMS_H
#define MTF_AMD_HOST_NN_PARAMS_H

#include <vector>

#include "GNNParams.h"

namespace mtf {

struct NNParams {
	int n_samples = 1000;                        /* NNParams.cc:8 */
	int max_iters = 1;                           /* NNParams.cc:6 */
	double epsilon = 0.01;                       /* NNParams.cc:7 */
	std::vector<std::vector<double>> ssm_sigma;  /* one row per sampler distribution (NT/NN.cc:56-84); a row of one value serves every state component */
	std::vector<std::vector<double>> ssm_mean;   /* rows as ssm_sigma; empty: zero means */
	std::vector<double> pix_sigma;               /* not used by the device path (sigmas are given per state component) */
	bool additive_update = false;                /* must stay false: see above */
	std::vector<int> distr_n_samples;            /* samples per distribution (NT/NN.cc:60-73); empty: equal shares, the remainder to the last */
	unsigned long long seed = 0;                 /* distribution k draws with seed + k */
	bool debug_mode = false;
	enum IndexType { EXACT = 0, GNN = 1 };
	IndexType index_type = EXACT;                /* EXACT: hip::NN as it was; GNN: buildGraph behind the dataset, searchGraph per iteration (NT/NN.cc:110-124, 250-251) */
	GNNParams gnn;
};

} // namespace mtf
#endif
