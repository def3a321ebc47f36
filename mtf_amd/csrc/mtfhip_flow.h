/*
 * mtfhip_flow.h -- what kernels_flow.hip (k_ncc_flow: NCC::estimateOpticalFlow, AM/src/NCC.cc:412-526, a point's whole flow in one
 * launch) and api_flow.hip (its C-ABI entry points) share.
 */
#ifndef MTFHIP_FLOW_H
#define MTFHIP_FLOW_H
#include "mtfhip_internal.h"

namespace mtfhip {

constexpr int kFlowMaxWin = MTFHIP_FLOW_MAX_WIN;       /* samples of a window: 4 per thread of a kBlock workgroup */
constexpr int kFlowTraceStride = MTFHIP_FLOW_TRACE_STRIDE;

struct FlowArgs {
	ImgView prev, cur;     /* the template's image and the one the loop samples */
	int win_w, win_h, max_iters, const_grad, fast_math;
	double epsilon, grad_eps;
	const float *prev_pts; /* [n_pts][2] */
	float *curr_pts;       /* [n_pts][2] */
	int *n_iters, *status; /* [n_pts] */
	double *trace;         /* [n_pts][trace_cap][kFlowTraceStride] or NULL */
	int trace_cap;
};

/* one workgroup per point; win_w * win_h <= kFlowMaxWin is the caller's to check */
void launch_ncc_flow(int n_pts, const FlowArgs &a, hipStream_t st);

} // namespace mtfhip
#endif
