/*
 * DeviceNN.h -- mtf::hip::NN: the nearest-neighbour search method (SM/include/mtf/SM/NT/NN.h, SM/src/NT/NN.cc:85-277) with the
 * reference's parameters over the device tracker of the C ABI (mtfhip_nn_*): the dataset is built and stays on the device, the index is
 * the exhaustive search or -- NNParams::index_type = GNN -- the reference's graph index gnn::GNN (mtfhip_nn_gnn_*: initialize() builds the
 * graph behind the dataset, NT/NN.cc:110-124), and update() is ONE mtfhip_nn_update call, as hip::LK makes one mtfhip_batch_track.  What a maintainer
 * registers next to nt::NN for HipAM / HipSSM pairs.
 */
#ifndef MTF_AMD_HOST_DEVICE_NN_H
#define MTF_AMD_HOST_DEVICE_NN_H

#include "HipModels.h"
#include "NNParams.h"
#include "SearchMethod.h"

namespace mtf {

namespace hip {
class NN : public nt::SearchMethod {
public:
	NN(std::shared_ptr<HipAM> am, std::shared_ptr<HipSSM> ssm, const NNParams &params);
	~NN() override;
	void initialize(const CornersT &corners) override;   /* NT/NN.cc:85-124: the template, generateDataset and, with the GNN index, buildGraph */
	void update() override;                               /* NT/NN.cc:236-277 */
	void setRegion(const CornersT &corners) override;
	const CornersT &getRegion() override;
	mtfhip_nn *handle() { return h; }
	/* best_idx, best_dist, update_norm of every iteration of the last update() */
	const std::vector<double> &getLog() const { return log; }
	/* with the GNN index: the start node and the step count of every iteration's walk of the last update() */
	const std::vector<int> &getWalkStarts() const { return walk_starts; }
	const std::vector<int> &getWalkSteps() const { return walk_steps; }
private:
	std::shared_ptr<HipAM> ham;
	std::shared_ptr<HipSSM> hssm;
	NNParams nn;
	mtfhip_nn *h = nullptr;
	CornersT region;
	std::vector<double> log;
	std::vector<int> walk_starts, walk_steps;
};
} // namespace hip

} // namespace mtf
#endif
