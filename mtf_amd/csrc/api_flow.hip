/*
 * api_flow.hip -- mtfhip_ncc_estimate_optical_flow[_dev|_trace]: am.estimateOpticalFlow (AM/src/NCC.cc:412-526) on the device
 * (C-ABI implementation, include/mtfhip.h; the kernel: kernels_flow.hip)
 */
#include "mtfhip_api_internal.h"
#include "mtfhip_flow.h"

/* the argument checks every entry point shares, all before any launch; fills the launch arguments that do not depend on where the arrays live */
static int flow_prepare(const char *fn, mtfhip_ctx *c, const mtfhip_flow_desc *d, int n_pts, FlowArgs &a) {
	if (!d) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);
	if (n_pts <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "%s: n_pts must be positive (got %d)", fn, n_pts);
	if (d->win_w < 2 || d->win_h < 2)   /* LinSpaced over one entry has no step; the reference's default is 10 x 10 */
		return fail(MTFHIP_ERR_INVALID_ARG, "%s: search window %d x %d: both sides must be at least 2", fn, d->win_w, d->win_h);
	if (d->max_iters <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "%s: max_iters must be positive (got %d)", fn, d->max_iters);
	if (d->math_mode != MTFHIP_MATH_REPLAY && d->math_mode != MTFHIP_MATH_FAST) return fail(MTFHIP_ERR_INVALID_ARG, "%s: unknown math mode %d", fn, d->math_mode);
	if (!(d->grad_eps > 0)) return fail(MTFHIP_ERR_INVALID_ARG, "%s: grad_eps must be positive", fn);
	if ((double)d->win_w * d->win_h > (double)kFlowMaxWin)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: search window %d x %d has %.0f samples; the kernel keeps a window in the registers of one workgroup and supports at most %d",
			fn, d->win_w, d->win_h, (double)d->win_w * d->win_h, kFlowMaxWin);
	if (!c) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);   /* (behind the descriptor's own refusals: those need no device) */
	if (!c->img.data) return fail(MTFHIP_ERR_LOGIC, "%s: no current image: call mtfhip_image_upload/borrow first", fn);
	if (!c->prev.data) return fail(MTFHIP_ERR_LOGIC, "%s: no previous image (mtfhip_image_keep_prev)", fn);
	if (c->img.channels != 1 || c->prev.channels != 1)   /* NCC.cc:416-420 */
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: NCC::estimateOpticalFlow::Image type 32FC3 is currently not supported", fn);
	if (c->img.h != c->prev.h || c->img.w != c->prev.w)
		return fail(MTFHIP_ERR_INVALID_ARG, "%s: the previous image is %d x %d, the current one %d x %d", fn, c->prev.h, c->prev.w, c->img.h, c->img.w);
	a.prev = c->prev; a.cur = c->img;
	a.win_w = d->win_w; a.win_h = d->win_h; a.max_iters = d->max_iters; a.const_grad = d->const_grad ? 1 : 0;
	a.fast_math = d->math_mode == MTFHIP_MATH_FAST ? 1 : 0;
	a.epsilon = d->epsilon; a.grad_eps = d->grad_eps;
	a.trace = nullptr; a.trace_cap = 0;
	return MTFHIP_OK;
}

static size_t flow_align16(size_t v) { return (v + 15) & ~(size_t)15; }

/* the host-pointer forms: one upload, one launch, one download, one synchronisation; the staging is the context's (est_ws: both users
 * leave it idle when they return) */
static int flow_host(const char *fn, mtfhip_ctx *c, const mtfhip_flow_desc *d, int n_pts, const float *prev_pts, float *curr_pts, int *n_iters, int *status,
	double *trace, int trace_cap, bool want_trace) {
	if (!prev_pts || !curr_pts || !n_iters || !status || (want_trace && !trace)) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);
	FlowArgs a{};
	TRY(flow_prepare(fn, c, d, n_pts, a));
	if (want_trace && trace_cap < d->max_iters) return fail(MTFHIP_ERR_INVALID_ARG, "%s: trace_cap %d is less than max_iters %d", fn, trace_cap, d->max_iters);
	const size_t P = (size_t)n_pts;
	const size_t o_prev = 0, o_curr = flow_align16(o_prev + sizeof(float) * 2 * P), o_n = flow_align16(o_curr + sizeof(float) * 2 * P),
		o_st = flow_align16(o_n + sizeof(int) * P), o_tr = flow_align16(o_st + sizeof(int) * P),
		total = flow_align16(o_tr + (want_trace ? sizeof(double) * P * trace_cap * kFlowTraceStride : 0));
	HIP_TRY(hipSetDevice(c->device));
	if (c->est_ws.capacity() < total) {
		HIP_TRY(hipStreamSynchronize(c->stream));
		HIP_TRY(c->est_ws.reserve(total));
	}
	hipStream_t st = c->stream;
	HIP_TRY(hipMemcpyAsync(c->est_ws + o_prev, prev_pts, sizeof(float) * 2 * P, hipMemcpyHostToDevice, st));
	a.prev_pts = (const float *)(c->est_ws + o_prev); a.curr_pts = (float *)(c->est_ws + o_curr);
	a.n_iters = (int *)(c->est_ws + o_n); a.status = (int *)(c->est_ws + o_st);
	if (want_trace) {
		a.trace = (double *)(c->est_ws + o_tr); a.trace_cap = trace_cap;
		HIP_TRY(hipMemsetAsync(a.trace, 0, sizeof(double) * P * trace_cap * kFlowTraceStride, st));
	}
	{
		TimedScope ts(c, "flow", st);
		launch_ncc_flow(n_pts, a, st);
	}
	HIP_TRY(hipGetLastError());
	std::vector<unsigned char> down(total - o_curr);
	HIP_TRY(hipMemcpyAsync(down.data(), c->est_ws + o_curr, total - o_curr, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	TRY(launch_error_pending());
	std::memcpy(curr_pts, down.data(), sizeof(float) * 2 * P);
	std::memcpy(n_iters, down.data() + (o_n - o_curr), sizeof(int) * P);
	std::memcpy(status, down.data() + (o_st - o_curr), sizeof(int) * P);
	if (want_trace) std::memcpy(trace, down.data() + (o_tr - o_curr), sizeof(double) * P * trace_cap * kFlowTraceStride);
	return MTFHIP_OK;
}

extern "C" {

int mtfhip_ncc_estimate_optical_flow(mtfhip_ctx *c, const mtfhip_flow_desc *d, int n_pts, const float *prev_pts, float *curr_pts, int *n_iters, int *status) {
	return flow_host("ncc_estimate_optical_flow", c, d, n_pts, prev_pts, curr_pts, n_iters, status, nullptr, 0, false);
}

int mtfhip_ncc_estimate_optical_flow_trace(mtfhip_ctx *c, const mtfhip_flow_desc *d, int n_pts, const float *prev_pts, float *curr_pts, int *n_iters,
	int *status, double *trace, int trace_cap) {
	return flow_host("ncc_estimate_optical_flow_trace", c, d, n_pts, prev_pts, curr_pts, n_iters, status, trace, trace_cap, true);
}

int mtfhip_ncc_estimate_optical_flow_dev(mtfhip_ctx *c, const mtfhip_flow_desc *d, int n_pts, const float *dev_prev_pts, float *dev_curr_pts,
	int *dev_n_iters, int *dev_status) {
	const char *fn = "ncc_estimate_optical_flow_dev";
	if (!dev_prev_pts || !dev_curr_pts || !dev_n_iters || !dev_status) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);
	FlowArgs a{};
	TRY(flow_prepare(fn, c, d, n_pts, a));
	a.prev_pts = dev_prev_pts; a.curr_pts = dev_curr_pts; a.n_iters = dev_n_iters; a.status = dev_status;
	HIP_TRY(hipSetDevice(c->device));
	{
		TimedScope ts(c, "flow", c->stream);
		launch_ncc_flow(n_pts, a, c->stream);
	}
	HIP_TRY(hipGetLastError());
	return MTFHIP_OK;
}

} /* extern "C" */
