/* DeviceGridFlow.cpp -- see DeviceGridFlow.h */
#include "DeviceGridFlow.h"

#include <cmath>
#include <cstring>

namespace mtf {
namespace hip {

GridFlow::GridFlow(const GridTrackerFlowParams &gp, int _grid_ssm, int math_mode, int device, void *stream) :
	params(gp), n(gp.grid_size_x * gp.grid_size_y), grid_ssm(_grid_ssm) {
	if (gp.grid_size_x <= 0 || gp.grid_size_y <= 0) throw utils::InvalidArgument("GridTrackerFlow :: grid sizes must be positive");
	if (grid_ssm == MTFHIP_SSM_SIMILITUDE || grid_ssm == MTFHIP_SSM_ISOMETRY || grid_ssm == MTFHIP_SSM_TRANSLATION)
		throw utils::FunctonNotImplemented("GridTrackerFlow :: the Similitude / Isometry / Translation state space models are not served as grid SSM");
	if (grid_ssm != MTFHIP_SSM_HOMOGRAPHY && grid_ssm != MTFHIP_SSM_AFFINE) throw utils::InvalidArgument("GridTrackerFlow :: unknown grid SSM");
	/* the grid SSM's points alone: a layout whose sampling resolution is the grid's (GridTrackerFlowParams.cc:24-25) */
	gd = mtfhip_grid_desc{gp.grid_size_x, gp.grid_size_y, 1, 1, 0, 0, 0};
	fd = mtfhip_flow_desc{gp.search_window_x, gp.search_window_y, gp.max_iters, gp.epsilon, gp.use_const_grad ? 1 : 0, 1e-8, math_mode};
	HipPair::check(mtfhip_ctx_create(device, stream, &ctx));
	prev_pts.resize(n); curr_pts.resize(n); flow_pts.resize(n); n_iters.assign(n, 0); status.assign(n, 0);
	grid_pts.assign(2 * (size_t)n, 0.0); patch_corners.assign(8 * (size_t)n, 0.0);
	ssm_update.resize(grid_ssm == MTFHIP_SSM_HOMOGRAPHY ? 8 : 6);
	pix_mask.assign(n, 1);   /* :57-58 */
	const int gs = grid_ssm;
	estimator = [gs](VectorXd &u, const std::vector<GridPt> &a, const std::vector<GridPt> &c) { Grid::leastSquaresFit(gs, u, a, c); };
}

GridFlow::~GridFlow() {
	if (ctx) mtfhip_ctx_destroy(ctx);
}

void GridFlow::setImage(const ImageView &img) {
	if (img.channels != 1)   /* NCC.cc:416-420 */
		throw utils::FunctonNotImplemented("NCC::estimateOpticalFlow::Image type 32FC3 is currently not supported");
	HipPair::check(mtfhip_image_upload(ctx, img.data, img.rows, img.cols, img.step));
}

/* prev_pts = ssm.getPts() rounded to float (:77-81, :121-124) */
void GridFlow::pointsToGrid() {
	HipPair::check(mtfhip_grid_layout(&gd, region.data(), grid_pts.data(), patch_corners.data()));
	for (int k = 0; k < n; ++k) { prev_pts[k].x = static_cast<float>(grid_pts[2 * k]); prev_pts[k].y = static_cast<float>(grid_pts[2 * k + 1]); }
}

void GridFlow::initialize(const CornersT &corners) {
	region = corners;
	pointsToGrid();
	HipPair::check(mtfhip_image_keep_prev(ctx));   /* am->getCurrImg().copyTo(prev_img) :82 */
	initialized = true;
}

void GridFlow::setRegion(const CornersT &corners) {
	region = corners;
	pointsToGrid();
}

void GridFlow::setEstimatorParams(const SSMEstimatorParams &ep, unsigned long long seed) {
	const int min_mp = grid_ssm == MTFHIP_SSM_HOMOGRAPHY ? 4 : 3;
	if (ep.n_model_pts < min_mp || ep.n_model_pts > MTFHIP_EST_MAX_MODEL_PTS) throw utils::InvalidArgument("GridTrackerFlow :: est_params.n_model_pts out of range");
	if (n > MTFHIP_EST_MAX_PTS) throw utils::InvalidArgument("GridTrackerFlow :: more points than the device estimator fits in one set");
	if (n < ep.n_model_pts) throw utils::InvalidArgument("GridTrackerFlow :: fewer points than est_params.n_model_pts");
	est_params = ep; est_seed = seed; device_estimator = true;
}

void GridFlow::update() {
	if (!initialized) throw utils::LogicError("GridTrackerFlow :: update before initialize");
	/* am->estimateOpticalFlow(curr_pts, prev_img, prev_pts, search_window, n_pts, max_iters, epsilon, use_const_grad) :89-90 */
	static_assert(sizeof(GridPt) == 2 * sizeof(float), "cv::Point2f layout");
	HipPair::check(mtfhip_ncc_estimate_optical_flow(ctx, &fd, n, &prev_pts[0].x, &flow_pts[0].x, n_iters.data(), status.data()));
	for (int k = 0; k < n; ++k)
		if (status[k] == MTFHIP_FLOW_NONFINITE || !std::isfinite(flow_pts[k].x) || !std::isfinite(flow_pts[k].y))
			throw utils::LogicError("GridTrackerFlow :: the optical flow of point " + std::to_string(k) + " is not finite");
	curr_pts = flow_pts;
	/* ssm->estimateWarpFromPts(ssm_update, pix_mask, prev_pts, curr_pts, est_params) :91 */
	if (device_estimator) {
		pix_mask_est.resize(n);
		estimateWarpFromPts(ctx, grid_ssm, ssm_update.data(), pix_mask_est.data(), prev_pts.data(), curr_pts.data(), n, est_params, est_seed++, &est_info);
		pix_mask = pix_mask_est;
	} else estimator(ssm_update, prev_pts, curr_pts);
	/* :93-95 */
	CornersT warped;
	HipPair::check(mtfhip_ssm_apply_warp_to_pts(grid_ssm, region.data(), 4, ssm_update.data(), warped.data()));
	region = warped;
	prev_pts = curr_pts;                               /* :97-100 */
	HipPair::check(mtfhip_image_keep_prev(ctx));       /* :102 */
}

} // namespace hip
} // namespace mtf
