/*
 * SSMEstimatorParams.h -- SSMEstimatorParams (SSM/include/mtf/SSM/SSMEstimatorParams.h:8-37, SSM/src/SSMEstimatorParams.cc) with the
 * reference's field names, EstType and defaults: the parameter block of ssm.estimateWarpFromPts, which mtf::hip::HipSSM and mtf::hip::Grid
 * run on the device (mtfhip_ssm_estimate_from_pts).
 */
#ifndef MTF_AMD_HOST_SSM_ESTIMATOR_PARAMS_H
#define MTF_AMD_HOST_SSM_ESTIMATOR_PARAMS_H

#include "../../include/mtfhip.h"

namespace mtf {

#ifdef MTF_AMD_USE_OPENCV
typedef cv::Point2f EstPt;
#else
struct EstPt { float x = 0, y = 0; };   /* cv::Point2f */
#endif

struct SSMEstimatorParams {
	enum class EstType { RANSAC, LeastMedian, LeastSquares };   /* SSMEstimatorParams.h:11 */
	EstType method = EstType::RANSAC;      /* SSMEstimatorParams.cc:5 */
	double ransac_reproj_thresh = 10.0;    /* :9 */
	int n_model_pts = 4;                   /* :10 */
	int max_iters = 2000;                  /* :6 */
	int max_subset_attempts = 300;         /* :7 */
	bool use_boost_rng = false;            /* :8; the device draws from Philox4x32-10 either way (the reference seeds from random_device) */
	double confidence = 0.995;             /* :13 */
	bool refine = true;                    /* :11 */
	int lm_max_iters = 10;                 /* :12 */

	SSMEstimatorParams() {}
	SSMEstimatorParams(EstType _method, double _ransac_reproj_thresh, int _n_model_pts, bool _refine, int _max_iters, int _max_subset_attempts,
		bool _use_boost_rng, double _confidence, int _lm_max_iters) :   /* :42-58 */
		method(_method), ransac_reproj_thresh(_ransac_reproj_thresh <= 0 ? 3 : _ransac_reproj_thresh), n_model_pts(_n_model_pts), max_iters(_max_iters),
		max_subset_attempts(_max_subset_attempts), use_boost_rng(_use_boost_rng), confidence(_confidence), refine(_refine), lm_max_iters(_lm_max_iters) {}
	static const char *toString(EstType t) {   /* :17-28 */
		return t == EstType::LeastSquares ? "LeastSquares" : t == EstType::RANSAC ? "RANSAC" : "LeastMedian";
	}
	mtfhip_est_params desc() const {
		mtfhip_est_params d;
		d.method = method == EstType::RANSAC ? MTFHIP_EST_RANSAC : method == EstType::LeastMedian ? MTFHIP_EST_LMEDS : MTFHIP_EST_LEAST_SQUARES;
		d.ransac_reproj_thresh = ransac_reproj_thresh; d.n_model_pts = n_model_pts; d.max_iters = max_iters; d.max_subset_attempts = max_subset_attempts;
		d.confidence = confidence; d.refine = refine ? 1 : 0; d.lm_max_iters = lm_max_iters;
		return d;
	}
};
typedef SSMEstimatorParams EstimatorParams;   /* Affine.cc:361 */

namespace hip {
/* what one call of the device estimator reports beside the state update and the mask */
struct EstimatorInfo {
	bool ok = false;
	int winner = -1, n_walked = 0, n_inliers = 0;
	double min_median = 0, sigma = 0;
};
/* ssm.estimateWarpFromPts (Homography.cc:885-897, Affine.cc:359-369) over mtfhip_ssm_estimate_from_pts: one point set, subsets drawn on the
 * device from `seed`.  state_update: 8 (homography) or 6 (affine) doubles; mask: one byte per point.  Throws on an argument error; a failed
 * fit is info.ok == false with the zero matrix's update. */
void estimateWarpFromPts(mtfhip_ctx *ctx, int ssm, double *state_update, unsigned char *mask, const EstPt *in_pts, const EstPt *out_pts, int n_pts,
	const SSMEstimatorParams &est_params, unsigned long long seed, EstimatorInfo *info = nullptr);
}

} // namespace mtf
#endif
