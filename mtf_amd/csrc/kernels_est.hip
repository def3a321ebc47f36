/*
 * kernels_est.hip -- ssm.estimateWarpFromPts on the device: the robust fit of the grid SSM (homography / affine) to point pairs that ends
 * GridTracker::update (SM/src/GridTracker.cc:267,333-341 -> SSM/src/Homography.cc:885-897, Affine.cc:359-369 -> estimateHomography /
 * estimateAffine, HomographyEstimator.cc:166-228, AffineEstimator.cc:127-190): RANSAC / LMedS / least squares, the re-fit on the inliers and
 * the Levenberg-Marquardt refinement (SSMEstimator.cc).
 *
 * One workgroup of 256 threads fits one point set; one launch fits several independent sets.  Per set:
 *   - the points sit in LDS as the floats they arrive as (cv::Point2f) and are widened on use (HomographyEstimator.cc:179-183);
 *   - hypotheses are evaluated in chunks of 64.  Lane l of wave 0 owns hypothesis base + l: it draws (or loads) its subset and fits its
 *     model -- for the homography a cyclic Jacobi on the 9 x 9 LtL held in LDS with the lane as the fastest index (conflict-free; ~160
 *     doubles per hypothesis would not fit the register file).  The four waves then score the chunk's models, a wave per model over all
 *     points (RANSAC: a ballot count; LMedS: the exact median by bisection on the float's bit pattern);
 *   - thread 0 walks the chunk's results with the reference's sequential rule (SSMEstimator.cc:101-128, 175-203), so hypotheses past the
 *     stopping index never influence anything: they are evaluated at most to the end of their chunk and never looked at;
 *   - the tail (mask, compaction in point order, re-fit, LM) uses all threads for the sums over the points -- per-thread partial sums,
 *     a shuffle tree per wave and a fixed-order sum of the four waves: no floating-point atomics, so a call is bit-reproducible --
 *     and thread 0 for the small dense algebra.
 * Everything is FP64 except the reprojection errors, which the reference itself rounds to float.
 */
#include "mtfhip_est.h"
#include "mtfhip_rng_device.h"

#include <cfloat>

namespace mtfhip {

namespace {

constexpr int EST_RED_MAX = 45;   /* the widest reduced row: LtL's upper triangle; the homography's JtJ (36) + JtErr (8) + errNorm */

struct EstShared {
	float in_x[kEstMaxPts], in_y[kEstMaxPts], out_x[kEstMaxPts], out_y[kEstMaxPts];       /* the set's points */
	float cin_x[kEstMaxPts], cin_y[kEstMaxPts], cout_x[kEstMaxPts], cout_y[kEstMaxPts];   /* the inliers, compacted in point order */
	double A[81 * kEstChunk], V[81 * kEstChunk];   /* Jacobi: entry-major, hypothesis (lane) fastest */
	double model[kEstChunk][9];
	double score[kEstChunk];                       /* RANSAC: inlier count; LMedS: median */
	int found[kEstChunk], has_model[kEstChunk];
	unsigned char pmask[kEstMaxPts];
	int seg_cnt[kEstMaxPts / 64];
	double red[4][EST_RED_MAX], sum[EST_RED_MAX];
	/* the walk's state (thread 0) */
	double best[9], H[9], Hfit[9];
	double min_median, sigma;
	int niters, max_good, winner, walked, stop, fail, fit_ok, n_compact, n_inl, result;
	/* LM (thread 0) */
	double param[8], prev[8], JtJ[64], JtErr[8], N[64], rhs[8];
	double err_norm, prev_err_norm, mask_thr;
	int mask_go;
	int lambda_lg10, lm_iters, lm_go, lm_done;
};

/* a workgroup-uniform control word read from LDS, as a scalar: every branch that leads to a barrier is taken on such a value, so the
 * compiler lowers it to a scalar branch and all four waves provably execute the same barriers */
__device__ __forceinline__ int uniform_dev(const int &v) { return __builtin_amdgcn_readfirstlane(v); }

/* cvRound: round half to even (the default rounding mode) */
__device__ __forceinline__ int cv_round_dev(double v) { return (int)rint(v); }

/* cvRANSACUpdateNumIters SSMEstimator.cc:50-71 */
__device__ int ransac_update_num_iters_dev(double p, double ep, int model_points, int max_iters) {
	p = fmax(p, 0.); p = fmin(p, 1.);
	ep = fmax(ep, 0.); ep = fmin(ep, 1.);
	double num = fmax(1. - p, DBL_MIN);
	double denom = 1. - pow(1. - ep, (double)model_points);
	if (denom < DBL_MIN) return 0;
	num = log(num);
	denom = log(denom);
	return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : cv_round_dev(num / denom);
}

/* checkSubset with checkPartialSubsets == false SSMEstimator.cc:262-296: no three points of the subset on one line */
__device__ bool check_subset_dev(const double *x, const double *y, int count) {
	for (int i = 0; i < count; ++i)
		for (int j = 0; j < i; ++j) {
			const double dx1 = x[j] - x[i], dy1 = y[j] - y[i];
			for (int k = 0; k < j; ++k) {
				const double dx2 = x[k] - x[i], dy2 = y[k] - y[i];
				if (fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return false;
			}
		}
	return true;
}

/* Cyclic Jacobi on the symmetric 9 x 9 matrix A (destroyed), eigenvectors in the columns of V; entry (i, j) lives at [(9 i + j) * stride].
 * The off-diagonal mass falls quadratically and has no rounding floor of its own (a rotation mixes off-diagonal entries only with each
 * other), so it is driven to 1e-20 of the matrix norm.  Returns the column of the smallest eigenvalue (cvEigenVV sorts descending and
 * the reference takes V[8], HomographyEstimator.cc:25,75). */
__device__ int jacobi9_dev(double *A, double *V, int stride) {
#define A_(i, j) A[((i) * 9 + (j)) * stride]
#define V_(i, j) V[((i) * 9 + (j)) * stride]
	for (int i = 0; i < 9; ++i)
		for (int j = 0; j < 9; ++j) V_(i, j) = i == j ? 1.0 : 0.0;
	for (int sweep = 0; sweep < 40; ++sweep) {
		double off = 0, all = 0;
		for (int i = 0; i < 9; ++i)
			for (int j = 0; j < 9; ++j) {
				const double v = A_(i, j);
				all += v * v;
				if (i != j) off += v * v;
			}
		if (!(off > 1e-40 * all)) break;
		for (int p = 0; p < 8; ++p)
			for (int q = p + 1; q < 9; ++q) {
				const double apq = A_(p, q);
				if (apq == 0.0) continue;
				const double theta = (A_(q, q) - A_(p, p)) / (2.0 * apq);
				const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
				const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
				for (int k = 0; k < 9; ++k) {
					const double akp = A_(k, p), akq = A_(k, q);
					A_(k, p) = c * akp - s * akq;
					A_(k, q) = s * akp + c * akq;
				}
				for (int k = 0; k < 9; ++k) {
					const double apk = A_(p, k), aqk = A_(q, k);
					A_(p, k) = c * apk - s * aqk;
					A_(q, k) = s * apk + c * aqk;
				}
				A_(p, q) = 0.0; A_(q, p) = 0.0;
				for (int k = 0; k < 9; ++k) {
					const double vkp = V_(k, p), vkq = V_(k, q);
					V_(k, p) = c * vkp - s * vkq;
					V_(k, q) = s * vkp + c * vkq;
				}
			}
	}
	int best = 0;
	for (int i = 1; i < 9; ++i)
		if (A_(i, i) < A_(best, best)) best = i;
	return best;
#undef A_
#undef V_
}

/* the second half of HomographyEstimator::runKernel (:48-80) once LtL's upper triangle is in A: the scale test, the eigenvector,
 * de-normalisation, division by H[8].  cm / sm: mean and summed absolute deviation of the output points, cM / sM: of the input points. */
__device__ bool hom_finish_dev(double *A, double *V, int stride, int count, double cmx, double cmy, double cMx, double cMy, double smx, double smy,
	double sMx, double sMy, double *H) {
	if (fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON) return false;
	smx = count / smx; smy = count / smy; sMx = count / sMx; sMy = count / sMy;
	for (int j = 0; j < 9; ++j)
		for (int k = 0; k < j; ++k) A[(j * 9 + k) * stride] = A[(k * 9 + j) * stride];   /* cvCompleteSymm */
	const int col = jacobi9_dev(A, V, stride);
	double h0[9];
	for (int k = 0; k < 9; ++k) h0[k] = V[(k * 9 + col) * stride];
	const double inv_hnorm[9] = {1. / smx, 0, cmx, 0, 1. / smy, cmy, 0, 0, 1};
	const double hnorm2[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
	double tmp[9], h1[9];
	m3_mul_dev(inv_hnorm, h0, tmp);
	m3_mul_dev(tmp, hnorm2, h1);
	const double sc = 1. / h1[8];
	for (int k = 0; k < 9; ++k) H[k] = h1[k] * sc;
	return true;
}

/* one point's rows of L (HomographyEstimator.cc:63-70) added to the upper triangle acc[45] (row j, column k >= j, row-major) */
__device__ __forceinline__ void ltl_accumulate_dev(double *acc, double x, double y, double X, double Y) {
	const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x};
	const double Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
	int e = 0;
#pragma unroll
	for (int j = 0; j < 9; ++j)
#pragma unroll
		for (int k = j; k < 9; ++k) { acc[e] += Lx[j] * Lx[k] + Ly[j] * Ly[k]; ++e; }
}

/* the affine least-squares fit from the sums over the points (AffineEstimator.cc:17-46 -> utils::computeAffineDLT warpUtils.cc:344-377: the
 * 2n x 6 system splits into two 3-unknown systems with one matrix).  Normal equations like Grid::leastSquaresFit, on input points centred at
 * their mean (mx, my) so that the 3 x 3 matrix is diag-dominant: s = {sxx, sxy, syy, sxX, syX, sX, sxY, syY, sY} over the centred inputs. */
__device__ void aff_solve_dev(const double *s, int count, double mx, double my, double *H) {
	const double sxx = s[0], sxy = s[1], syy = s[2];
	const double det = sxx * syy - sxy * sxy;
	const double inv = 1.0 / det;
	/* centred: sum x = sum y = 0, so the translation decouples */
	const double a00 = (syy * s[3] - sxy * s[4]) * inv, a01 = (sxx * s[4] - sxy * s[3]) * inv;
	const double a10 = (syy * s[6] - sxy * s[7]) * inv, a11 = (sxx * s[7] - sxy * s[6]) * inv;
	const double tx = s[5] / count, ty = s[8] / count;
	H[0] = a00; H[1] = a01; H[2] = tx - (a00 * mx + a01 * my);
	H[3] = a10; H[4] = a11; H[5] = ty - (a10 * mx + a11 * my);
	H[6] = 0; H[7] = 0; H[8] = 1;
}

/* Gaussian elimination with partial pivoting, n x n row-major, in place; a zero pivot leaves its unknown at zero (the reference's SVD
 * back-substitution drops the singular direction, SSMEstimator.cc:512-513) */
__device__ void solve_dev(int n, double *A, double *b) {
	for (int i = 0; i < n; ++i) {
		int piv = i;
		for (int r = i + 1; r < n; ++r)
			if (fabs(A[r * n + i]) > fabs(A[piv * n + i])) piv = r;
		if (A[piv * n + i] == 0.0) continue;
		if (piv != i) {
			for (int c = 0; c < n; ++c) { const double t = A[i * n + c]; A[i * n + c] = A[piv * n + c]; A[piv * n + c] = t; }
			const double t = b[i]; b[i] = b[piv]; b[piv] = t;
		}
		for (int r = i + 1; r < n; ++r) {
			const double f = A[r * n + i] / A[i * n + i];
			for (int c = i; c < n; ++c) A[r * n + c] -= f * A[i * n + c];
			b[r] -= f * b[i];
		}
	}
	for (int i = n - 1; i >= 0; --i) {
		double s = b[i];
		for (int c = i + 1; c < n; ++c) s -= A[i * n + c] * b[c];
		b[i] = A[i * n + i] != 0.0 ? s / A[i * n + i] : 0.0;
	}
}

/* sum of v[0 .. NV) over the workgroup into sh.sum, the same order on every run: shuffle tree per wave, then the four waves in order */
template <int NV>
__device__ __forceinline__ void block_sum_dev(EstShared &sh, double *v) {
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
		for (int e = 0; e < NV; ++e) v[e] += __shfl_down(v[e], off, 64);
	__syncthreads();   /* (the previous sum has been read) */
	if (lane == 0)
#pragma unroll
		for (int e = 0; e < NV; ++e) sh.red[w][e] = v[e];
	__syncthreads();
	if ((int)threadIdx.x < NV) sh.sum[threadIdx.x] = ((sh.red[0][threadIdx.x] + sh.red[1][threadIdx.x]) + sh.red[2][threadIdx.x]) + sh.red[3][threadIdx.x];
	__syncthreads();
}

/* computeReprojError HomographyEstimator.cc:84-98, AffineEstimator.cc:49-62: double arithmetic, rounded to float */
template <int SSM>
__device__ __forceinline__ float reproj_err_dev(const double *H, double Mx, double My, double mx, double my) {
	if constexpr (SSM == MTFHIP_SSM_HOMOGRAPHY) {
		const double ww = 1. / (H[6] * Mx + H[7] * My + 1.);
		const double dx = (H[0] * Mx + H[1] * My + H[2]) * ww - mx;
		const double dy = (H[3] * Mx + H[4] * My + H[5]) * ww - my;
		return (float)(dx * dx + dy * dy);
	} else {
		const double dx = (H[0] * Mx + H[1] * My + H[2]) - mx;
		const double dy = (H[3] * Mx + H[4] * My + H[5]) - my;
		return (float)(dx * dx + dy * dy);
	}
}

/* runKernel on m points held in four float arrays, by the whole workgroup: sh.fit_ok, sh.Hfit.  The same expressions as the per-lane fit
 * of a subset; the sums over the points are reduced in the workgroup's fixed order. */
template <int SSM>
__device__ void fit_all_dev(EstShared &sh, const float *ix, const float *iy, const float *ox, const float *oy, int m) {
	const int tid = threadIdx.x;
	if constexpr (SSM == MTFHIP_SSM_HOMOGRAPHY) {
		double v4[4] = {0, 0, 0, 0};
		for (int i = tid; i < m; i += kEstBlock) { v4[0] += (double)ox[i]; v4[1] += (double)oy[i]; v4[2] += (double)ix[i]; v4[3] += (double)iy[i]; }
		block_sum_dev<4>(sh, v4);
		const double cmx = sh.sum[0] / m, cmy = sh.sum[1] / m, cMx = sh.sum[2] / m, cMy = sh.sum[3] / m;
		double d4[4] = {0, 0, 0, 0};
		for (int i = tid; i < m; i += kEstBlock) {
			d4[0] += fabs((double)ox[i] - cmx); d4[1] += fabs((double)oy[i] - cmy); d4[2] += fabs((double)ix[i] - cMx); d4[3] += fabs((double)iy[i] - cMy);
		}
		block_sum_dev<4>(sh, d4);
		const double smx = sh.sum[0], smy = sh.sum[1], sMx = sh.sum[2], sMy = sh.sum[3];
		const bool scales_ok = !(fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON);
		double acc[45];
#pragma unroll
		for (int e = 0; e < 45; ++e) acc[e] = 0;
		if (scales_ok) {
			const double kx = m / smx, ky = m / smy, kX = m / sMx, kY = m / sMy;
			for (int i = tid; i < m; i += kEstBlock)
				ltl_accumulate_dev(acc, ((double)ox[i] - cmx) * kx, ((double)oy[i] - cmy) * ky, ((double)ix[i] - cMx) * kX, ((double)iy[i] - cMy) * kY);
		}
		block_sum_dev<45>(sh, acc);
		if (tid == 0) {
			int e = 0;
			for (int j = 0; j < 9; ++j)
				for (int k = j; k < 9; ++k) sh.A[(j * 9 + k) * kEstChunk] = sh.sum[e++];
			sh.fit_ok = hom_finish_dev(sh.A, sh.V, kEstChunk, m, cmx, cmy, cMx, cMy, smx, smy, sMx, sMy, sh.Hfit) ? 1 : 0;
		}
	} else {
		double v2[2] = {0, 0};
		for (int i = tid; i < m; i += kEstBlock) { v2[0] += (double)ix[i]; v2[1] += (double)iy[i]; }
		block_sum_dev<2>(sh, v2);
		const double mx = sh.sum[0] / m, my = sh.sum[1] / m;
		double s[9];
#pragma unroll
		for (int e = 0; e < 9; ++e) s[e] = 0;
		for (int i = tid; i < m; i += kEstBlock) {
			const double x = (double)ix[i] - mx, y = (double)iy[i] - my, X = (double)ox[i], Y = (double)oy[i];
			s[0] += x * x; s[1] += x * y; s[2] += y * y; s[3] += x * X; s[4] += y * X; s[5] += X; s[6] += x * Y; s[7] += y * Y; s[8] += Y;
		}
		block_sum_dev<9>(sh, s);
		if (tid == 0) { aff_solve_dev(sh.sum, m, mx, my, sh.Hfit); sh.fit_ok = 1; }
	}
	__syncthreads();
}

/* one pass of refine()'s loop over the points (HomographyEstimator.cc:117-139, AffineEstimator.cc:81-100) at sh.param: with_j = JtJ's upper
 * triangle, JtErr and errNorm into sh.sum (in that order), else errNorm alone into sh.sum[0] */
template <int SSM, bool WITH_J>
__device__ void lm_pass_dev(EstShared &sh, int m) {
	constexpr int NP = SSM == MTFHIP_SSM_HOMOGRAPHY ? 8 : 6;
	constexpr int NT = NP * (NP + 1) / 2;
	constexpr int NV = WITH_J ? NT + NP + 1 : 1;
	double h[8];
#pragma unroll
	for (int k = 0; k < NP; ++k) h[k] = sh.param[k];
	double acc[NV];
#pragma unroll
	for (int e = 0; e < NV; ++e) acc[e] = 0;
	for (int i = threadIdx.x; i < m; i += kEstBlock) {
		const double Mx = (double)sh.cin_x[i], My = (double)sh.cin_y[i];
		double J0[NP], J1[NP], e0, e1;
		if constexpr (SSM == MTFHIP_SSM_HOMOGRAPHY) {
			double ww = h[6] * Mx + h[7] * My + 1.;
			ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
			const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww, yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
			e0 = xi - (double)sh.cout_x[i]; e1 = yi - (double)sh.cout_y[i];
			J0[0] = Mx * ww; J0[1] = My * ww; J0[2] = ww; J0[3] = 0; J0[4] = 0; J0[5] = 0; J0[6] = -Mx * ww * xi; J0[7] = -My * ww * xi;
			J1[0] = 0; J1[1] = 0; J1[2] = 0; J1[3] = Mx * ww; J1[4] = My * ww; J1[5] = ww; J1[6] = -Mx * ww * yi; J1[7] = -My * ww * yi;
		} else {
			const double xi = h[0] * Mx + h[1] * My + h[2], yi = h[3] * Mx + h[4] * My + h[5];
			e0 = xi - (double)sh.cout_x[i]; e1 = yi - (double)sh.cout_y[i];
			J0[0] = Mx; J0[1] = My; J0[2] = 1; J0[3] = 0; J0[4] = 0; J0[5] = 0;
			J1[0] = 0; J1[1] = 0; J1[2] = 0; J1[3] = Mx; J1[4] = My; J1[5] = 1;
		}
		if constexpr (WITH_J) {
			int e = 0;
#pragma unroll
			for (int j = 0; j < NP; ++j)
#pragma unroll
				for (int k = j; k < NP; ++k) { acc[e] += J0[j] * J0[k] + J1[j] * J1[k]; ++e; }
#pragma unroll
			for (int j = 0; j < NP; ++j) acc[NT + j] += J0[j] * e0 + J1[j] * e1;
		}
		acc[NV - 1] += e0 * e0 + e1 * e1;
	}
	block_sum_dev<NV>(sh, acc);
}

/* LevMarq::step SSMEstimator.cc:489-516 (thread 0): the upper triangle mirrored, the diagonal scaled by 1 + lambda, param = prevParam - x */
template <int NP>
__device__ void lm_step_dev(EstShared &sh) {
	const double lambda = exp(sh.lambda_lg10 * log(10.));
	for (int i = 0; i < NP; ++i) {
		for (int j = 0; j < NP; ++j) sh.N[i * NP + j] = j >= i ? sh.JtJ[i * NP + j] : sh.JtJ[j * NP + i];
		sh.rhs[i] = sh.JtErr[i];
	}
	for (int i = 0; i < NP; ++i) sh.N[(NP + 1) * i] *= 1. + lambda;
	solve_dev(NP, sh.N, sh.rhs);
	for (int i = 0; i < NP; ++i) sh.param[i] = sh.prev[i] - sh.rhs[i];
}

/* refine(): LevMarq(nparams, 0, ITER + EPS, lm_max_iters, DBL_EPSILON) driven through updateAlt (SSMEstimator.cc:329-359, 427-487) on
 * the m compacted points; sh.H's first NP entries in and out */
template <int SSM>
__device__ void lm_refine_dev(EstShared &sh, int m, int lm_max_iters) {
	constexpr int NP = SSM == MTFHIP_SSM_HOMOGRAPHY ? 8 : 6;
	constexpr int NT = NP * (NP + 1) / 2;
	const int tid = threadIdx.x;
	const int max_iter = min(max(lm_max_iters, 1), 1000);
	auto take_j = [&]() {   /* thread 0, after a WITH_J pass */
		int e = 0;
		for (int j = 0; j < NP; ++j)
			for (int k = j; k < NP; ++k) sh.JtJ[j * NP + k] = sh.sum[e++];
		for (int j = 0; j < NP; ++j) sh.JtErr[j] = sh.sum[NT + j];
	};
	if (tid == 0) {
		for (int k = 0; k < NP; ++k) sh.param[k] = sh.H[k];
		sh.lambda_lg10 = -3; sh.lm_iters = 0;
	}
	__syncthreads();
	lm_pass_dev<SSM, true>(sh, m);                       /* STARTED -> CALC_J */
	if (tid == 0) { take_j(); sh.err_norm = sh.sum[NT + NP]; }
	for (int it = 0; it < max_iter; ++it) {             /* (lm_done is raised at the latest when iters reaches max_iter: the count only makes the bound explicit) */
		if (tid == 0) {                                   /* CALC_J */
			for (int k = 0; k < NP; ++k) sh.prev[k] = sh.param[k];
			lm_step_dev<NP>(sh);
			sh.prev_err_norm = sh.err_norm;
		}
		__syncthreads();
		lm_pass_dev<SSM, false>(sh, m);
		if (tid == 0) sh.err_norm = sh.sum[0];
		for (int rej = 0; rej < 34; ++rej) {              /* CHECK_ERR: the rejection loop (lambdaLg10 climbs from >= -16 to 17 at most: the count only makes the bound explicit) */
			if (tid == 0) {
				sh.lm_go = (sh.err_norm > sh.prev_err_norm && ++sh.lambda_lg10 <= 16) ? 1 : 0;
				if (sh.lm_go) lm_step_dev<NP>(sh);
			}
			__syncthreads();
			if (!uniform_dev(sh.lm_go)) break;
			lm_pass_dev<SSM, false>(sh, m);
			if (tid == 0) sh.err_norm = sh.sum[0];
		}
		if (tid == 0) {
			sh.lambda_lg10 = max(sh.lambda_lg10 - 1, -16);
			double d2 = 0, p2 = 0;
			for (int k = 0; k < NP; ++k) { const double d = sh.param[k] - sh.prev[k]; d2 += d * d; p2 += sh.prev[k] * sh.prev[k]; }
			/* cvNorm(param, prevParam, CV_RELATIVE_L2) = |param - prevParam| / (|prevParam| + DBL_EPSILON) */
			sh.lm_done = (++sh.lm_iters >= max_iter || sqrt(d2) / (sqrt(p2) + DBL_EPSILON) < DBL_EPSILON) ? 1 : 0;
		}
		__syncthreads();
		if (uniform_dev(sh.lm_done)) break;
		lm_pass_dev<SSM, true>(sh, m);                   /* back to CALC_J: JtJ and JtErr anew, errNorm kept */
		if (tid == 0) take_j();
	}
	if (tid == 0)
		for (int k = 0; k < NP; ++k) sh.H[k] = sh.param[k];
	__syncthreads();
}

/* the k-th smallest (0-based) of the wave's non-negative floats e[j] (point 64 j + lane; bits 0xFFFFFFFF past the end): their order is the order
 * of their bit patterns (the reference sorts them as ints, SSMEstimator.cc:193), so the largest v with #{x < v} <= k is found bit by bit */
__device__ __forceinline__ unsigned wave_select_dev(const unsigned (&e)[kEstMaxPts / 64], int nj, int k) {
	unsigned prefix = 0;
	for (int bit = 30; bit >= 0; --bit) {
		const unsigned cand = prefix | (1u << bit);
		int cnt = 0;
#pragma unroll
		for (int j = 0; j < kEstMaxPts / 64; ++j)
			if (j < nj) cnt += __popcll(__ballot(e[j] < cand));
		if (cnt <= k) prefix = cand;
	}
	return prefix;
}

template <int SSM>
__global__ __launch_bounds__(kEstBlock) void est_kernel(EstArgs a) {
	__shared__ EstShared sh;
	const int set = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int mp = a.n_model_pts;
	const int n = min(max(a.n_pts[set], 0), min(a.max_pts, kEstMaxPts));   /* (the host entry point has checked it; device-side callers are held to the arrays' bounds here) */
	const float *gin = a.in_pts + (size_t)set * a.max_pts * 2, *gout = a.out_pts + (size_t)set * a.max_pts * 2;
	int *subsets = a.subsets + (size_t)set * a.n_hyp * mp;
	unsigned char *gmask = a.mask + (size_t)set * a.max_pts;
	constexpr int NS = SSM == MTFHIP_SSM_HOMOGRAPHY ? 8 : 6;

	for (int i = tid; i < n; i += kEstBlock) {
		sh.in_x[i] = gin[2 * i]; sh.in_y[i] = gin[2 * i + 1]; sh.out_x[i] = gout[2 * i]; sh.out_y[i] = gout[2 * i + 1];
		gmask[i] = 1;                                          /* tempMask = all ones HomographyEstimator.cc:190-193 */
	}
	if (n < mp) {   /* CV_Assert(n_pts >= params.n_model_pts) :177 -- an argument error at the API; from device-side counts: a failed fit */
		if (tid == 0) {
			for (int q = 0; q < 8; ++q) a.update[(size_t)set * 8 + q] = 0.0;
			if constexpr (SSM == MTFHIP_SSM_HOMOGRAPHY) { a.update[(size_t)set * 8] = -1; a.update[(size_t)set * 8 + 4] = -1; }
			else { a.update[(size_t)set * 8 + 2] = -1; a.update[(size_t)set * 8 + 5] = -1; }
			int *info = a.info + (size_t)set * 4;
			info[0] = 0; info[1] = -1; info[2] = 0; info[3] = n;
			a.stats[(size_t)set * 2] = 0; a.stats[(size_t)set * 2 + 1] = 0;
		}
		return;
	}
	const int method = n == mp ? MTFHIP_EST_LEAST_SQUARES : a.method;   /* :196 */
	if (tid == 0) {
		sh.min_median = DBL_MAX; sh.sigma = 0;
		sh.niters = min(method == MTFHIP_EST_LMEDS ? a.lmeds_niters : a.max_iters, a.n_hyp);
		sh.max_good = 0; sh.winner = -1; sh.walked = 0; sh.stop = 0; sh.fail = 0; sh.result = 0; sh.n_compact = 0; sh.n_inl = n;
		for (int k = 0; k < 9; ++k) { sh.best[k] = 0; sh.H[k] = 0; }
	}
	__syncthreads();

	if (method != MTFHIP_EST_LEAST_SQUARES) {
		const double thr2 = a.thresh * a.thresh;
		const int nj = (n + 63) >> 6;
		for (int base = 0;; base += kEstChunk) {
			if (uniform_dev(sh.stop) || base >= uniform_dev(sh.niters)) break;   /* (written before the last barrier) */
			const int cnt = min(kEstChunk, a.n_hyp - base);
			/* ---- phase 1: subset and model, one hypothesis per lane of wave 0 ---- */
			if (tid < cnt) {
				const int k = base + tid;
				int idx[kEstMaxModelPts];
				double sx[kEstMaxModelPts], sy[kEstMaxModelPts], dx[kEstMaxModelPts], dy[kEstMaxModelPts];
				bool found;
				if (a.subsets_given) {
					for (int i = 0; i < mp; ++i) idx[i] = min(max(subsets[(size_t)k * mp + i], 0), n - 1);
					found = true;
				} else {
					/* getSubset with checkPartialSubsets == false SSMEstimator.cc:219-259; draw d of attempt t of hypothesis k is word d & 3 of
					 * Philox4x32-10 at counter (k, t, d >> 2, "ESTS") under the seed */
					int iters = 0, i = 0;
					for (; iters < a.max_subset_attempts; ++iters) {
						unsigned d = 0;
						Philox4 r{{0, 0, 0, 0}};
						for (i = 0; i < mp;) {
							if ((d & 3) == 0) r = philox4x32_10((unsigned)k, (unsigned)iters, d >> 2, 0x45535453u, (unsigned)a.seed, (unsigned)(a.seed >> 32));
							const int id = (int)(r.c[d & 3] % (unsigned)n);
							++d;
							int j = 0;
							for (; j < i; ++j)
								if (idx[j] == id) break;
							if (j < i) continue;
							idx[i++] = id;
						}
						for (int q = 0; q < mp; ++q) { sx[q] = (double)sh.in_x[idx[q]]; sy[q] = (double)sh.in_y[idx[q]]; dx[q] = (double)sh.out_x[idx[q]]; dy[q] = (double)sh.out_y[idx[q]]; }
						if (!check_subset_dev(sx, sy, mp) || !check_subset_dev(dx, dy, mp)) continue;
						break;
					}
					found = i == mp && iters < a.max_subset_attempts;
					if (found)
						for (int q = 0; q < mp; ++q) subsets[(size_t)k * mp + q] = idx[q];
				}
				bool has = false;
				if (found) {
					for (int q = 0; q < mp; ++q) { sx[q] = (double)sh.in_x[idx[q]]; sy[q] = (double)sh.in_y[idx[q]]; dx[q] = (double)sh.out_x[idx[q]]; dy[q] = (double)sh.out_y[idx[q]]; }
					double H[9];
					if constexpr (SSM == MTFHIP_SSM_HOMOGRAPHY) {
						/* HomographyEstimator::runKernel :29-71 in the subset's order */
						double cmx = 0, cmy = 0, cMx = 0, cMy = 0, smx = 0, smy = 0, sMx = 0, sMy = 0;
						for (int q = 0; q < mp; ++q) { cmx += dx[q]; cmy += dy[q]; cMx += sx[q]; cMy += sy[q]; }
						cmx /= mp; cmy /= mp; cMx /= mp; cMy /= mp;
						for (int q = 0; q < mp; ++q) { smx += fabs(dx[q] - cmx); smy += fabs(dy[q] - cmy); sMx += fabs(sx[q] - cMx); sMy += fabs(sy[q] - cMy); }
						double acc[45];
#pragma unroll
						for (int e = 0; e < 45; ++e) acc[e] = 0;
						const bool scales_ok = !(fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON);
						if (scales_ok) {
							const double kx = mp / smx, ky = mp / smy, kX = mp / sMx, kY = mp / sMy;
							for (int q = 0; q < mp; ++q) ltl_accumulate_dev(acc, (dx[q] - cmx) * kx, (dy[q] - cmy) * ky, (sx[q] - cMx) * kX, (sy[q] - cMy) * kY);
							int e = 0;
#pragma unroll
							for (int j = 0; j < 9; ++j)
#pragma unroll
								for (int q = j; q < 9; ++q) { sh.A[(j * 9 + q) * kEstChunk + tid] = acc[e]; ++e; }
						}
						has = hom_finish_dev(sh.A + tid, sh.V + tid, kEstChunk, mp, cmx, cmy, cMx, cMy, smx, smy, sMx, sMy, H);
					} else {
						double mx = 0, my = 0;
						for (int q = 0; q < mp; ++q) { mx += sx[q]; my += sy[q]; }
						mx /= mp; my /= mp;
						double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
						for (int q = 0; q < mp; ++q) {
							const double x = sx[q] - mx, y = sy[q] - my;
							s[0] += x * x; s[1] += x * y; s[2] += y * y; s[3] += x * dx[q]; s[4] += y * dx[q]; s[5] += dx[q]; s[6] += x * dy[q]; s[7] += y * dy[q]; s[8] += dy[q];
						}
						aff_solve_dev(s, mp, mx, my, H);
						has = true;
					}
					if (has)
						for (int q = 0; q < 9; ++q) sh.model[tid][q] = H[q];
				}
				sh.found[tid] = found ? 1 : 0;
				sh.has_model[tid] = has ? 1 : 0;
			}
			__syncthreads();
			/* ---- phase 2: a wave per model over all points ---- */
			for (int h = wave; h < cnt; h += 4) {
				if (!uniform_dev(sh.found[h]) || !uniform_dev(sh.has_model[h])) continue;
				double H[9];
#pragma unroll
				for (int q = 0; q < 9; ++q) H[q] = sh.model[h][q];
				unsigned eb[kEstMaxPts / 64];
				int good = 0;
#pragma unroll
				for (int j = 0; j < kEstMaxPts / 64; ++j) {
					eb[j] = 0xFFFFFFFFu;
					if (j < nj) {
						const int i = j * 64 + lane;
						bool in = false;
						if (i < n) {
							const float err = reproj_err_dev<SSM>(H, (double)sh.in_x[i], (double)sh.in_y[i], (double)sh.out_x[i], (double)sh.out_y[i]);
							eb[j] = __float_as_uint(err);
							in = (double)err <= thr2;                 /* findInliers SSMEstimator.cc:43-45 */
						}
						good += __popcll(__ballot(in));
					}
				}
				if (method == MTFHIP_EST_RANSAC) {
					if (lane == 0) sh.score[h] = (double)good;
				} else {
					/* the median of the sorted errors :193-196 */
					double median;
					if (n & 1) median = (double)__uint_as_float(wave_select_dev(eb, nj, n / 2));
					else {
						const float lo = __uint_as_float(wave_select_dev(eb, nj, n / 2 - 1)), hi = __uint_as_float(wave_select_dev(eb, nj, n / 2));
						median = (double)(lo + hi) * 0.5;
					}
					if (lane == 0) sh.score[h] = median;
				}
			}
			__syncthreads();
			/* ---- phase 3: the sequential rule over the chunk ---- */
			if (tid == 0) {
				int k = base;
				for (; k < base + cnt; ++k) {
					if (k >= sh.niters) { sh.stop = 1; break; }
					const int l = k - base;
					if (!sh.found[l]) {                          /* :104-109, 178-183 */
						if (k == 0) sh.fail = 1;
						sh.stop = 1;
						break;
					}
					if (!sh.has_model[l]) continue;             /* :112-114 */
					if (method == MTFHIP_EST_RANSAC) {
						const int good = (int)sh.score[l];
						if (good > max(sh.max_good, mp - 1)) {   /* :120-126 */
							for (int q = 0; q < 9; ++q) sh.best[q] = sh.model[l][q];
							sh.max_good = good; sh.winner = k;
							sh.niters = ransac_update_num_iters_dev(a.confidence, (double)(n - good) / n, mp, sh.niters);
						}
					} else if (sh.score[l] < sh.min_median) {    /* :198-201 */
						sh.min_median = sh.score[l]; sh.winner = k;
						for (int q = 0; q < 9; ++q) sh.best[q] = sh.model[l][q];
					}
				}
				sh.walked = k;                                   /* `iter` when the loop ends */
			}
			__syncthreads();
		}
		/* ---- the method's result and mask ---- */
		if (tid == 0) {
			double thr = 0;
			int go = 0;
			if (method == MTFHIP_EST_RANSAC) {
				if (!sh.fail && sh.max_good > 0) { thr = a.thresh; go = 1; }   /* :132-136: the accepted model's tmask */
			} else if (!sh.fail && sh.min_median < DBL_MAX) {                  /* :207-213 */
				thr = 2.5 * 1.4826 * (1 + 5. / (n - mp)) * sqrt(sh.min_median);
				thr = fmax(thr, 0.001);
				go = 1;
			}
			sh.mask_thr = thr; sh.mask_go = go;
		}
		__syncthreads();
		const bool mask_pass = uniform_dev(sh.mask_go) != 0;
		const double thr = sh.mask_thr;
		if (mask_pass) {
			const double t2 = thr * thr;
			double H[9];
			for (int q = 0; q < 9; ++q) H[q] = sh.best[q];
			int good = 0;
			for (int i0 = 0; i0 < n; i0 += kEstBlock) {
				const int i = i0 + tid;
				bool in = false;
				if (i < n) {
					const float err = reproj_err_dev<SSM>(H, (double)sh.in_x[i], (double)sh.in_y[i], (double)sh.out_x[i], (double)sh.out_y[i]);
					in = (double)err <= t2;
					sh.pmask[i] = in ? 1 : 0;
					gmask[i] = in ? 1 : 0;
				}
				good += __popcll(__ballot(in));
			}
			if (lane == 0) sh.seg_cnt[wave] = good;
			__syncthreads();
			if (tid == 0) {
				const int total = sh.seg_cnt[0] + sh.seg_cnt[1] + sh.seg_cnt[2] + sh.seg_cnt[3];
				sh.result = method == MTFHIP_EST_RANSAC ? 1 : (total >= mp ? 1 : 0);
				sh.n_inl = total;
				if (method == MTFHIP_EST_LMEDS) sh.sigma = thr;
				for (int q = 0; q < 9; ++q) sh.H[q] = sh.best[q];
			}
		}
		__syncthreads();
	} else {
		/* LeastSquares, and every method at n_pts == n_model_pts: runKernel on all points, the mask stays all ones */
		for (int i = tid; i < n; i += kEstBlock) sh.pmask[i] = 1;
		fit_all_dev<SSM>(sh, sh.in_x, sh.in_y, sh.out_x, sh.out_y, n);
		if (tid == 0) {
			sh.result = sh.fit_ok;
			for (int q = 0; q < 9; ++q) sh.H[q] = sh.Hfit[q];
		}
		__syncthreads();
	}

	/* ---- the tail HomographyEstimator.cc:206-215, AffineEstimator.cc:168-177 ---- */
	int n_in = n;
	if (uniform_dev(sh.result) && n > mp) {
		/* icvCompressPoints: the inliers in point order; 64-point segments, a ballot each */
		const int nseg = (n + 63) >> 6;
		for (int s = wave; s < nseg; s += 4) {
			const int i = s * 64 + lane;
			const unsigned long long b = __ballot(i < n && sh.pmask[i]);
			if (lane == 0) sh.seg_cnt[s] = __popcll(b);
		}
		__syncthreads();
		for (int s = wave; s < nseg; s += 4) {
			const int i = s * 64 + lane;
			const bool in = i < n && sh.pmask[i];
			const unsigned long long b = __ballot(in);
			int off = 0;
			for (int q = 0; q < s; ++q) off += sh.seg_cnt[q];
			if (in) {
				const int p = off + __popcll(b & ((1ull << lane) - 1ull));
				sh.cin_x[p] = sh.in_x[i]; sh.cin_y[p] = sh.in_y[i]; sh.cout_x[p] = sh.out_x[i]; sh.cout_y[p] = sh.out_y[i];
			}
		}
		if (tid == 0) {
			int total = 0;
			for (int q = 0; q < nseg; ++q) total += sh.seg_cnt[q];
			sh.n_compact = total;
		}
		__syncthreads();
		n_in = uniform_dev(sh.n_compact);
		if (method == MTFHIP_EST_RANSAC) {               /* the re-fit on the inliers; its return value is not looked at (:210-211) */
			fit_all_dev<SSM>(sh, sh.cin_x, sh.cin_y, sh.cout_x, sh.cout_y, n_in);
			if (tid == 0 && sh.fit_ok)
				for (int q = 0; q < 9; ++q) sh.H[q] = sh.Hfit[q];
			__syncthreads();
		}
		if (a.refine) lm_refine_dev<SSM>(sh, n_in, a.lm_max_iters);
	}
	__syncthreads();

	/* ---- outputs: the update in the SSM's own parameterisation (Homography.cc:889-896, Affine.cc:363-368); a failed fit is the zero matrix ---- */
	if (tid == 0) {
		double W[9];
		for (int q = 0; q < 9; ++q) W[q] = sh.result ? sh.H[q] : 0.0;
		double p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		if constexpr (SSM == MTFHIP_SSM_HOMOGRAPHY) { p[0] = W[0] - 1; p[1] = W[1]; p[2] = W[2]; p[3] = W[3]; p[4] = W[4] - 1; p[5] = W[5]; p[6] = W[6]; p[7] = W[7]; }
		else { p[0] = W[2]; p[1] = W[5]; p[2] = W[0] - 1; p[3] = W[1]; p[4] = W[3]; p[5] = W[4] - 1; }
		for (int q = 0; q < 8; ++q) a.update[(size_t)set * 8 + q] = q < NS ? p[q] : 0.0;
		int *info = a.info + (size_t)set * 4;
		info[0] = sh.result; info[1] = sh.winner; info[2] = sh.walked;
		info[3] = sh.n_inl;
		a.stats[(size_t)set * 2] = sh.min_median < DBL_MAX ? sh.min_median : 0.0;
		a.stats[(size_t)set * 2 + 1] = sh.sigma;
	}
}

} // namespace

void launch_est(int ssm, int n_sets, const EstArgs &a, hipStream_t st) {
	if (ssm == MTFHIP_SSM_HOMOGRAPHY) hipLaunchKernelGGL(est_kernel<MTFHIP_SSM_HOMOGRAPHY>, dim3(n_sets), dim3(kEstBlock), 0, st, a);
	else hipLaunchKernelGGL(est_kernel<MTFHIP_SSM_AFFINE>, dim3(n_sets), dim3(kEstBlock), 0, st, a);
}

} // namespace mtfhip
