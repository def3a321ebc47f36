/*
 * GridTrackerFlowParams.h -- the parameter block of nt::GridTrackerFlow (SM/include/mtf/SM/GridTrackerFlowParams.h) with the reference's
 * field names and defaults (:6-17).  pyramid_levels and min_eig_thresh are carried as the reference carries them: it prints them
 * (NT/GridTrackerFlow.cc:20-22) and never reads them; show_trackers and debug_mode have no meaning here.
 */
#ifndef MTF_AMD_HOST_GRID_TRACKER_FLOW_PARAMS_H
#define MTF_AMD_HOST_GRID_TRACKER_FLOW_PARAMS_H

namespace mtf {

struct GridTrackerFlowParams {
	int grid_size_x = 10, grid_size_y = 10;
	int search_window_x = 10, search_window_y = 10;
	int pyramid_levels = 0;          /* unused */
	bool use_const_grad = false;
	double min_eig_thresh = 1e-4;    /* unused */
	int max_iters = 30;
	double epsilon = 0.01;
	bool show_trackers = false;
	bool debug_mode = false;
	int getResX() const { return grid_size_x; }   /* GridTrackerFlowParams.cc:24-25: the grid SSM samples the grid itself */
	int getResY() const { return grid_size_y; }
};

} // namespace mtf
#endif
