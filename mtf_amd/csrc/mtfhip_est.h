/*
 * mtfhip_est.h -- what kernels_est.hip (the device RANSAC / LMedS / least-squares estimator of the grid SSM,
 * SSM/src/{SSMEstimator,HomographyEstimator,AffineEstimator}.cc) and api_est.hip (its C-ABI entry points) share.
 */
#ifndef MTFHIP_EST_H
#define MTFHIP_EST_H
#include <hip/hip_runtime.h>

namespace mtfhip {

constexpr int kEstBlock = 256;        /* threads of the one workgroup that fits a point set */
constexpr int kEstChunk = 64;         /* hypotheses evaluated between two walks of the sequential rule (one per lane of wave 0) */
constexpr int kEstMaxPts = 1024;      /* points per set (LDS: 2 x 4 float arrays of this length) */
constexpr int kEstMaxModelPts = 8;    /* n_model_pts */

struct EstArgs {
	int method;            /* MTFHIP_EST_* */
	int n_model_pts, max_iters, max_subset_attempts, refine, lm_max_iters;
	double thresh, confidence;
	int lmeds_niters;      /* SSMEstimator.cc:172-173, evaluated on the host */
	int n_hyp;             /* rows of `subsets` per set: the walk never goes past it */
	int subsets_given;     /* 1: `subsets` holds the caller's rows; 0: the kernel draws and writes them */
	unsigned long long seed;
	int max_pts;           /* stride of the per-set arrays */
	const int *n_pts;      /* [n_sets] */
	const float *in_pts, *out_pts;   /* [n_sets][max_pts][2] */
	int *subsets;          /* [n_sets][n_hyp][n_model_pts] */
	double *update;        /* [n_sets][8] */
	unsigned char *mask;   /* [n_sets][max_pts] */
	int *info;             /* [n_sets][4]: ok, winning hypothesis, hypotheses walked, inliers */
	double *stats;         /* [n_sets][2]: minMedian, sigma (LMedS) */
};

void launch_est(int ssm, int n_sets, const EstArgs &a, hipStream_t st);

} // namespace mtfhip
#endif
