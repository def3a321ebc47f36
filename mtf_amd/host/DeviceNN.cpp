/* DeviceNN.cpp -- see DeviceNN.h */
#include "DeviceNN.h"

#include <algorithm>
#include <cstring>

namespace mtf {

namespace hip {
NN::NN(std::shared_ptr<HipAM> a, std::shared_ptr<HipSSM> s, const NNParams &np) : nt::SearchMethod(a, s, nt::SMParams()), ham(a), hssm(s), nn(np) {
	name = "nn_hip";
	if (a->pair().get() != s->pair().get()) throw utils::InvalidArgument("hip::NN :: the AM and the SSM must share one HipPair");
	/* everything that can be refused is refused BEFORE the device handle exists (a constructor that throws runs no destructor) */
	if (nn.additive_update) throw utils::FunctonNotImplemented("hip::NN :: additive_update: the compositional form only");
	if (nn.ssm_sigma.empty()) throw utils::InvalidArgument("hip::NN :: ssm_sigma is empty");
	if (nn.max_iters <= 0 || nn.n_samples <= 0) throw utils::InvalidArgument("hip::NN :: n_samples and max_iters must be positive");
	const int k = (int)nn.ssm_sigma.size();
	if (nn.distr_n_samples.empty()) {
		nn.distr_n_samples.assign((size_t)k, nn.n_samples / k);
		nn.distr_n_samples.back() += nn.n_samples - k * (nn.n_samples / k);
	}
	int total = 0;
	for (int c : nn.distr_n_samples) total += c;
	if ((int)nn.distr_n_samples.size() != k || total != nn.n_samples) throw utils::InvalidArgument("hip::NN :: distr_n_samples does not match ssm_sigma / n_samples");
	HipPair::check(mtfhip_nn_create(a->pair()->b, nn.n_samples, &h));
	if (nn.index_type == NNParams::GNN) {   /* (the handle exists: a refusal from here on must release it) */
		int rc = mtfhip_nn_set_index(h, MTFHIP_NN_INDEX_GNN);
		if (rc == MTFHIP_OK && nn.gnn.start_node != 0) rc = mtfhip_nn_gnn_set_start(h, nn.gnn.start_node);
		if (rc != MTFHIP_OK) { mtfhip_nn_destroy(h); h = nullptr; }
		HipPair::check(rc);
	}
}
NN::~NN() { if (h) mtfhip_nn_destroy(h); }
void NN::initialize(const CornersT &corners) {
	am->clearInitStatus(); ssm->clearInitStatus();
	ssm->initialize(corners, am->getNChannels());
	am->initializePixVals(ssm->getPts());
	const int S = ssm_state_size;
	auto entry = [](const std::vector<double> &row, int k, double fallback) { return row.empty() ? fallback : (row.size() == 1 ? row[0] : row.at((size_t)k)); };
	std::vector<mtfhip_nn_desc> d(nn.ssm_sigma.size());
	for (size_t i = 0; i < d.size(); ++i) {
		std::memset(&d[i], 0, sizeof(d[i]));
		d[i].n_samples = nn.distr_n_samples[i];
		d[i].seed = nn.seed + i;
		const std::vector<double> empty;
		const std::vector<double> &mean = nn.ssm_mean.empty() ? empty : nn.ssm_mean[std::min(i, nn.ssm_mean.size() - 1)];
		for (int k = 0; k < S; ++k) { d[i].sigma[k] = entry(nn.ssm_sigma[i], k, 0.0); d[i].mean[k] = entry(mean, k, 0.0); }
	}
	HipPair::check(mtfhip_nn_build(h, d.data(), (int)d.size()));
	if (nn.index_type == NNParams::GNN) {   /* NT/NN.cc:110-124: gnn_index->buildGraph(eig_dataset.data()) */
		mtfhip_gnn_desc g;
		std::memset(&g, 0, sizeof(g));
		g.degree = nn.gnn.degree; g.max_steps = nn.gnn.max_steps; g.cmpt_dist_thresh = nn.gnn.cmpt_dist_thresh;
		g.random_start = nn.gnn.random_start ? 1 : 0; g.seed = nn.gnn.seed;
		HipPair::check(mtfhip_nn_gnn_build(h, &g));
	}
}
void NN::setRegion(const CornersT &corners) {
	ssm->setCorners(corners);
	hssm->markMoved();
}
void NN::update() {
	am->setFirstIter();
	log.assign(3 * (size_t)nn.max_iters, 0.0);
	HipPair::check(mtfhip_nn_update(h, nn.max_iters, nn.epsilon, region.data(), &iters_done, log.data()));
	log.resize(3 * (size_t)iters_done);
	walk_starts.assign((size_t)iters_done, 0); walk_steps.assign((size_t)iters_done, 0);
	if (nn.index_type == NNParams::GNN && iters_done > 0) HipPair::check(mtfhip_nn_gnn_last_walks(h, walk_starts.data(), walk_steps.data()));
	hssm->markMoved();
}
const CornersT &NN::getRegion() {
	HipPair::check(mtfhip_ssm_get_corners(ham->pair()->b, region.data()));
	return region;
}
} // namespace hip
} // namespace mtf
