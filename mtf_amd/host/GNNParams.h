/*
 * GNNParams.h -- the parameters of nt::NN's graph index gnn::GNN (SM/include/mtf/SM/GNNParams.h, defaults SM/src/GNNParams.cc:3-7) with the
 * reference's field names, for mtf::hip::NN.  cmpt_dist_thresh only decides in the reference whether the all-pairs distances are cached
 * (NT/GNN.cc:60-64); the device build computes them in panels whatever it says.  seed and start_node are additions: the reference draws
 * its start nodes with an unseeded rand() (NT/GNN.cc:28, 123-125); here the first search starts at start_node, and with random_start
 * every search draws from a counter-based generator keyed by (seed, the running search count).
 */
#ifndef MTF_AMD_HOST_GNN_PARAMS_H
#define MTF_AMD_HOST_GNN_PARAMS_H

namespace mtf {

struct GNNParams {
	int degree = 250;               /* GNNParams.cc:3; 0 or > n_samples: n_samples; negative: -n_samples / degree (NT/GNN.cc:15-19); then at most n_samples - 1 */
	int max_steps = 10;             /* GNNParams.cc:4 */
	int cmpt_dist_thresh = 10000;   /* GNNParams.cc:5; accepted, ignored */
	bool random_start = false;      /* GNNParams.cc:6 */
	bool verbose = false;           /* GNNParams.cc:7 */
	unsigned long long seed = 0;
	int start_node = 0;
};

} // namespace mtf
#endif
