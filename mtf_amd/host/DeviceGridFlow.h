/*
 * DeviceGridFlow.h -- mtf::hip::GridFlow: nt::GridTrackerFlow (SM/src/NT/GridTrackerFlow.cc:74-126, `grid_sm flow`) on the device.  The
 * grid_size_x * grid_size_y points of the grid SSM are tracked from the previous frame to the current one by NCC::estimateOpticalFlow
 * (AM/src/NCC.cc:412-526: mtfhip_ncc_estimate_optical_flow, every point's whole flow in one launch), the grid SSM is fitted to
 * prev_pts -> curr_pts and the region warped by the fit; afterwards prev_pts = curr_pts (the points drift; setRegion puts them back on the
 * grid) and the current frame becomes the previous one (mtfhip_image_keep_prev: the two frames alternate between two device buffers).
 * TrackerBase-shaped, like mtf::hip::Grid: setImage / initialize / update / setRegion / getRegion with the reference's parameter block.
 *
 * The fit -- ssm.estimateWarpFromPts -- runs on the device once setEstimatorParams() has been called (with the reference's pix_mask);
 * without that call it is a std::function (setEstimator) whose default is hip::Grid's all-points least-squares fit.
 * A point whose flow is not finite (its window is flat in either frame) makes update() throw LogicError before the fit sees it,
 * with the tracker's state unchanged.
 */
#ifndef MTF_AMD_HOST_DEVICE_GRID_FLOW_H
#define MTF_AMD_HOST_DEVICE_GRID_FLOW_H

#include "DeviceGrid.h"
#include "GridTrackerFlowParams.h"

namespace mtf {
namespace hip {

class GridFlow {
public:
	typedef Grid::Estimator Estimator;
	std::string name = "grid_flow_hip";

	GridFlow(const GridTrackerFlowParams &params, int grid_ssm = MTFHIP_SSM_HOMOGRAPHY, int math_mode = MTFHIP_MATH_FAST, int device = 0, void *stream = nullptr);
	~GridFlow();
	GridFlow(const GridFlow &) = delete;
	GridFlow &operator=(const GridFlow &) = delete;

	void setImage(const ImageView &img);
#ifdef MTF_AMD_USE_OPENCV
	void setImage(const cv::Mat &img) { setImage(imageView(img)); }
#endif
	void initialize(const CornersT &corners);   /* GridTrackerFlow.cc:74-86 */
	void update();                              /* :88-105 */
	void setRegion(const CornersT &corners);    /* :119-126 */
	const CornersT &getRegion() { return region; }
	void setEstimator(Estimator e) { estimator = e; }
	void setEstimatorParams(const SSMEstimatorParams &est_params, unsigned long long seed = 1);
	const std::vector<unsigned char> &getPixMask() const { return pix_mask; }   /* all ones before the first update (:57-58) */
	bool estimatorOk() const { return est_info.ok; }
	const std::vector<GridPt> &getPrevPts() const { return prev_pts; }
	const std::vector<GridPt> &getCurrPts() const { return curr_pts; }
	const VectorXd &getSSMUpdate() const { return ssm_update; }
	const std::vector<int> &getIters() const { return n_iters; }
	const std::vector<int> &getStatus() const { return status; }    /* MTFHIP_FLOW_* per point */
private:
	GridTrackerFlowParams params;
	mtfhip_grid_desc gd;
	mtfhip_flow_desc fd;
	mtfhip_ctx *ctx = nullptr;
	int n, grid_ssm;
	bool initialized = false;
	CornersT region;
	std::vector<GridPt> prev_pts, curr_pts, flow_pts;
	std::vector<int> n_iters, status;
	std::vector<double> grid_pts, patch_corners;
	VectorXd ssm_update;
	Estimator estimator;
	bool device_estimator = false;
	SSMEstimatorParams est_params;
	unsigned long long est_seed = 1;
	EstimatorInfo est_info;
	std::vector<unsigned char> pix_mask, pix_mask_est;
	void pointsToGrid();
};

} // namespace hip
} // namespace mtf
#endif
