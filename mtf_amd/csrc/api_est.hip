/*
 * api_est.hip -- mtfhip_ssm_estimate_from_pts[_dev]: ssm.estimateWarpFromPts (SSM/src/Homography.cc:885-897, Affine.cc:359-369) on the
 * device (C-ABI implementation, include/mtfhip.h; the kernel: kernels_est.hip)
 */
#include "mtfhip_api_internal.h"
#include "mtfhip_est.h"

/* the argument checks both entry points share; fills the launch arguments that do not depend on where the arrays live */
static int est_prepare(const char *fn, mtfhip_ctx *c, int ssm, const mtfhip_est_params *p, int n_sets, const int *host_n_pts, int max_pts, int n_hyp,
	unsigned long long seed, EstArgs &a) {
	if (!c || !p) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);
	if (ssm_lowdof(ssm))
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: the robust estimator of the %s state space model is not available (homography and affine only)", fn, ssm_name(ssm));
	if (ssm != MTFHIP_SSM_HOMOGRAPHY && ssm != MTFHIP_SSM_AFFINE) return fail(MTFHIP_ERR_INVALID_ARG, "%s: unknown state space model %d", fn, ssm);
	if (p->method != MTFHIP_EST_RANSAC && p->method != MTFHIP_EST_LMEDS && p->method != MTFHIP_EST_LEAST_SQUARES)
		return fail(MTFHIP_ERR_INVALID_ARG, "%s: Invalid estimation method specified (%d)", fn, p->method);   /* SSMEstimatorParams.cc:26,38 */
	const int min_mp = ssm == MTFHIP_SSM_HOMOGRAPHY ? 4 : 3;   /* HomographyEstimator.cc:12, AffineEstimator.cc:13 */
	if (p->n_model_pts < min_mp || p->n_model_pts > MTFHIP_EST_MAX_MODEL_PTS)
		return fail(MTFHIP_ERR_INVALID_ARG, "%s: n_model_pts %d outside [%d, %d]", fn, p->n_model_pts, min_mp, (int)MTFHIP_EST_MAX_MODEL_PTS);
	if (n_sets <= 0 || max_pts <= 0 || n_hyp <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "%s: n_sets, max_pts and n_hyp must be positive", fn);
	if (max_pts > MTFHIP_EST_MAX_PTS)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: %d points per set; the kernel holds a set in LDS and supports at most %d", fn, max_pts, (int)MTFHIP_EST_MAX_PTS);
	if (p->max_iters <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "%s: max_iters must be positive", fn);
	if ((double)n_sets * n_hyp * p->n_model_pts >= 2147483648.0) return fail(MTFHIP_ERR_INVALID_ARG, "%s: %d sets x %d hypotheses exceed 2^31 subset entries", fn, n_sets, n_hyp);
	if (host_n_pts)
		for (int s = 0; s < n_sets; ++s) {
			if (host_n_pts[s] < p->n_model_pts)   /* CV_Assert(n_pts >= params.n_model_pts) HomographyEstimator.cc:177 */
				return fail(MTFHIP_ERR_INVALID_ARG, "%s: set %d has %d points, fewer than n_model_pts = %d", fn, s, host_n_pts[s], p->n_model_pts);
			if (host_n_pts[s] > max_pts) return fail(MTFHIP_ERR_INVALID_ARG, "%s: set %d has %d points, more than max_pts = %d", fn, s, host_n_pts[s], max_pts);
		}
	a.method = p->method;
	a.n_model_pts = p->n_model_pts; a.max_iters = p->max_iters; a.max_subset_attempts = p->max_subset_attempts;
	a.refine = p->refine ? 1 : 0; a.lm_max_iters = p->lm_max_iters;
	a.thresh = p->ransac_reproj_thresh <= 0 ? 3.0 : p->ransac_reproj_thresh;   /* SSMEstimatorParams.cc:54-56 */
	a.confidence = p->confidence;
	{   /* SSMEstimator.cc:145,172-173 */
		const double outlier_ratio = 0.45;
		const double r = std::log(1 - p->confidence) / std::log(1 - std::pow(1 - outlier_ratio, (double)p->n_model_pts));
		int niters = std::isfinite(r) ? (int)std::nearbyint(std::min(std::max(r, -1e9), 1e9)) : p->max_iters;   /* cvRound: half to even */
		a.lmeds_niters = std::min(std::max(niters, 3), p->max_iters);
	}
	a.n_hyp = n_hyp; a.seed = seed; a.max_pts = max_pts;
	return MTFHIP_OK;
}

static size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

extern "C" {

int mtfhip_ssm_estimate_from_pts(mtfhip_ctx *c, int ssm, const mtfhip_est_params *p, int n_sets, const int *n_pts, int max_pts, const float *in_pts,
	const float *out_pts, const int *subsets, int n_hyp, unsigned long long seed, double *state_update, unsigned char *mask, int *info, double *stats,
	int *subsets_used) {
	const char *fn = "ssm_estimate_from_pts";
	if (!n_pts || !in_pts || !out_pts || !state_update || !mask || !info || !stats) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);
	EstArgs a{};
	TRY(est_prepare(fn, c, ssm, p, n_sets, n_pts, max_pts, n_hyp, seed, a));
	const size_t S = (size_t)n_sets, mp = (size_t)p->n_model_pts;
	if (subsets)
		for (size_t s = 0; s < S; ++s)
			for (size_t q = 0; q < (size_t)n_hyp * mp; ++q) {
				const int id = subsets[s * n_hyp * mp + q];
				if (id < 0 || id >= n_pts[s]) return fail(MTFHIP_ERR_INVALID_ARG, "%s: subset index %d of set %zu outside [0, %d)", fn, id, s, n_pts[s]);
			}
	/* device staging: [n_pts | in_pts | out_pts | subsets] up, [subsets | update | stats | info | mask] down */
	const size_t o_n = 0, o_in = align16(o_n + sizeof(int) * S), o_out = align16(o_in + sizeof(float) * 2 * S * max_pts),
		o_sub = align16(o_out + sizeof(float) * 2 * S * max_pts), o_upd = align16(o_sub + sizeof(int) * S * n_hyp * mp), o_stats = align16(o_upd + sizeof(double) * 8 * S),
		o_info = align16(o_stats + sizeof(double) * 2 * S), o_mask = align16(o_info + sizeof(int) * 4 * S), total = align16(o_mask + S * max_pts);
	HIP_TRY(hipSetDevice(c->device));
	if (c->est_ws.capacity() < total) {
		HIP_TRY(hipStreamSynchronize(c->stream));
		HIP_TRY(c->est_ws.reserve(total));
	}
	std::vector<unsigned char> up(subsets ? o_upd : o_sub, 0), down(total - o_sub);
	std::memcpy(up.data() + o_n, n_pts, sizeof(int) * S);
	std::memcpy(up.data() + o_in, in_pts, sizeof(float) * 2 * S * max_pts);
	std::memcpy(up.data() + o_out, out_pts, sizeof(float) * 2 * S * max_pts);
	if (subsets) std::memcpy(up.data() + o_sub, subsets, sizeof(int) * S * n_hyp * mp);
	hipStream_t st = c->stream;
	HIP_TRY(hipMemcpyAsync(c->est_ws, up.data(), up.size(), hipMemcpyHostToDevice, st));
	if (!subsets) HIP_TRY(hipMemsetAsync(c->est_ws + o_sub, 0xFF, sizeof(int) * S * n_hyp * mp, st));
	a.subsets_given = subsets ? 1 : 0;
	a.n_pts = (const int *)(c->est_ws + o_n); a.in_pts = (const float *)(c->est_ws + o_in); a.out_pts = (const float *)(c->est_ws + o_out);
	a.subsets = (int *)(c->est_ws + o_sub); a.update = (double *)(c->est_ws + o_upd); a.stats = (double *)(c->est_ws + o_stats);
	a.info = (int *)(c->est_ws + o_info); a.mask = c->est_ws + o_mask;
	{
		TimedScope ts(c, "est", st);
		launch_est(ssm, n_sets, a, st);
	}
	HIP_TRY(hipGetLastError());
	const size_t from = subsets_used ? o_sub : o_upd;
	HIP_TRY(hipMemcpyAsync(down.data() + (from - o_sub), c->est_ws + from, total - from, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	auto at = [&](size_t off) { return down.data() + (off - o_sub); };
	if (subsets_used) std::memcpy(subsets_used, at(o_sub), sizeof(int) * S * n_hyp * mp);
	std::memcpy(state_update, at(o_upd), sizeof(double) * 8 * S);
	std::memcpy(stats, at(o_stats), sizeof(double) * 2 * S);
	std::memcpy(info, at(o_info), sizeof(int) * 4 * S);
	std::memcpy(mask, at(o_mask), S * max_pts);
	return MTFHIP_OK;
}

int mtfhip_ssm_estimate_from_pts_dev(mtfhip_ctx *c, int ssm, const mtfhip_est_params *p, int n_sets, const int *dev_n_pts, const int *host_n_pts,
	int max_pts, const float *dev_in_pts, const float *dev_out_pts, int *dev_subsets, int subsets_given, int n_hyp, unsigned long long seed,
	double *dev_state_update, unsigned char *dev_mask, int *dev_info, double *dev_stats) {
	const char *fn = "ssm_estimate_from_pts_dev";
	if (!dev_n_pts || !dev_in_pts || !dev_out_pts || !dev_subsets || !dev_state_update || !dev_mask || !dev_info || !dev_stats)
		return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);
	EstArgs a{};
	TRY(est_prepare(fn, c, ssm, p, n_sets, host_n_pts, max_pts, n_hyp, seed, a));
	a.subsets_given = subsets_given ? 1 : 0;
	a.n_pts = dev_n_pts; a.in_pts = dev_in_pts; a.out_pts = dev_out_pts; a.subsets = dev_subsets;
	a.update = dev_state_update; a.stats = dev_stats; a.info = dev_info; a.mask = dev_mask;
	HIP_TRY(hipSetDevice(c->device));
	{
		TimedScope ts(c, "est", c->stream);
		launch_est(ssm, n_sets, a, c->stream);
	}
	HIP_TRY(hipGetLastError());
	return MTFHIP_OK;
}

} /* extern "C" */
