/*
 * kernels_nn_search.hip -- nt::NN's per-frame half on the device (SM/src/NT/NN.cc:236-277): the exact nearest-neighbour search of the
 * current patch's distance feature over the resident n_samples x feat_size dataset (what FLANN's Linear index computes,
 * SM/include/mtf/SM/FLANNParams.h:13, and what GNN and the KD-trees approximate), and the compositional update with the winning
 * sample's perturbation.
 *   k_nn_search<NCC>      persistent workgroups; the query is staged once in LDS; a wave takes whole rows (row r of wave w of workgroup g:
 *                         r = 4 g + w, then steps of 4 gridDim.x), a lane the element pairs lane, lane + 64, ... of the row, read as 16
 *                         bytes where the row starts on a 16-byte boundary and as two 8-byte loads where it does not (rows of odd feat_size
 *                         alternate); the distance functors are SSDBaseDist (AM/src/SSDBase.cc:576-603: sum (a - b)^2; its worst_dist early
 *                         return does not change the argmin) and NCCDist (AM/src/NCC.cc:568-591: -sum a b on the centred unit-norm rows).
 *                         The order of a row's sum depends on feat_size alone -- four accumulators per lane, a fixed DPP tree -- so equal rows
 *                         have equal distances wherever they are stored, and a wave keeps its running best (dist, index); a workgroup
 *                         writes the best of its four waves to a partials array.  No atomics.
 *   k_nn_search_finish    one wave per query: the minimum of the partials, ties to the lower index -> idx[q], dist[q].
 *   k_nn_pick_update<SSM> one wave: the same minimum, the log entry (best_idx, best_dist, update_norm), W <- W * W(perturbations[best_idx])
 *                         as compositionalUpdate does (Homography.cc:73-92, Affine.cc:87-109), the corners, update_norm =
 *                         ||prev_corners - corners||^2 (NN.cc:263) and the `done` flag (NN.cc:268).
 * (dist, index) pairs ordered lexicographically have an exact minimum, so no reduction order shows in the result: a call is bit-reproducible.
 * One of the translation units of libmtfhip.so.
 */
#include "mtfhip_device.h"
#include "mtfhip_rng_device.h"
#include "mtfhip_nn_search_device.h"

namespace mtfhip {

template <bool NCC>
__global__ __launch_bounds__(kBlock) void k_nn_search(const double *feat, int n_samples, int F, const double *queries, NnBest *partials, const int *done) {
	extern __shared__ nns_d2 nns_q[];   /* the query: (F + 1) / 2 pairs, a zero behind an odd row */
	__shared__ NnBest wbest[4];
	if (done && *done) return;          /* (uniform, in front of every barrier) */
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	double *sq = reinterpret_cast<double *>(nns_q);
	const double *q = queries + (size_t)blockIdx.y * F;
	for (int i = threadIdx.x; i < F; i += kBlock) sq[i] = q[i];
	if (threadIdx.x == 0 && (F & 1)) sq[F] = 0.0;
	__syncthreads();
	double best = __builtin_inf();
	int bidx = INT_MAX;
	for (int r = (int)blockIdx.x * 4 + wave; r < n_samples; r += (int)gridDim.x * 4) {
		const double d = nn_row_dist<NCC>(feat, r, F, lane, nns_q);   /* (mtfhip_nn_search_device.h: the graph walk's rows take the same body) */
		if (d < best) { best = d; bidx = r; }   /* (a wave's rows ascend: the first of equal distances stays) */
	}
	if (lane == 0) { wbest[wave].dist = best; wbest[wave].idx = bidx; }
	__syncthreads();
	if (threadIdx.x == 0) {
		NnBest o = wbest[0];
#pragma unroll
		for (int w = 1; w < 4; ++w) if (nn_better(wbest[w].dist, wbest[w].idx, o.dist, o.idx)) o = wbest[w];
		o.pad = 0;
		partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = o;
	}
}

__global__ __launch_bounds__(64) void k_nn_search_finish(const NnBest *partials, int nblk, int *idx, double *dist) {
	double d; int i;
	nn_reduce_partials(partials + (size_t)blockIdx.x * nblk, nblk, d, i);
	if (threadIdx.x == 0) { idx[blockIdx.x] = i == INT_MAX ? -1 : i; dist[blockIdx.x] = i == INT_MAX ? __builtin_nan("") : d; }
}

/* st: W (9) | corners x0 y0 .. x3 y3 (8) | init_corners_hm (12); ctl: done | n_iters; log[it]: best_idx | best_dist | update_norm */
template <int SSM>
__global__ __launch_bounds__(64) void k_nn_pick_update(const NnBest *partials, int nblk, const double *perts, int n_samples, double *st, int *ctl,
	double *log, int it, double epsilon) {
	constexpr int S = SSM == MTFHIP_SSM_HOMOGRAPHY ? 8 : 6;
	if (ctl[0]) return;
	double d; int bi;
	nn_reduce_partials(partials, nblk, d, bi);
	if (threadIdx.x != 0) return;
	if (bi < 0 || bi >= n_samples) {   /* no row compared below infinity (a feature that is not a number): the loop stops where it is */
		log[3 * it] = -1.0; log[3 * it + 1] = __builtin_nan(""); log[3 * it + 2] = 0.0;
		ctl[1] = it + 1; ctl[0] = 1;
		return;
	}
	double p[8], P[9], W[9], Wn[9];
#pragma unroll
	for (int q = 0; q < 8; ++q) p[q] = q < S ? perts[(size_t)bi * S + q] : 0.0;
#pragma unroll
	for (int q = 0; q < 9; ++q) W[q] = st[q];
	warp_from_state_dev<SSM>(p, P);
	m3_mul_dev(W, P, Wn);
	if constexpr (SSM == MTFHIP_SSM_HOMOGRAPHY) {
		const double n22 = Wn[8];
#pragma unroll
		for (int q = 0; q < 9; ++q) Wn[q] /= n22;
	}
	double un = 0.0;
#pragma unroll
	for (int c = 0; c < 4; ++c) {   /* corners = dehomogenise(curr_warp * init_corners_hm) (Homography.cc:87-90) / the affine top rows (Affine.cc:105) */
		const double *ic = st + 17 + 3 * c;
		double x = Wn[0] * ic[0] + Wn[1] * ic[1] + Wn[2] * ic[2];
		double y = Wn[3] * ic[0] + Wn[4] * ic[1] + Wn[5] * ic[2];
		if constexpr (SSM == MTFHIP_SSM_HOMOGRAPHY) {
			const double dd = Wn[6] * ic[0] + Wn[7] * ic[1] + Wn[8] * ic[2];
			x = x / dd; y = y / dd;
		}
		const double ex = st[9 + 2 * c] - x, ey = st[9 + 2 * c + 1] - y;
		un += ex * ex; un += ey * ey;
		st[9 + 2 * c] = x; st[9 + 2 * c + 1] = y;
	}
#pragma unroll
	for (int q = 0; q < 9; ++q) st[q] = Wn[q];
	log[3 * it] = (double)bi; log[3 * it + 1] = d; log[3 * it + 2] = un;
	ctl[1] = it + 1;
	if (un < epsilon) ctl[0] = 1;
}

/* the LDS a search launch asks for */
static size_t nn_search_lds(int F) { return sizeof(double) * (size_t)(F + 2); }

/* workgroups a search launch of this feature size may keep resident: occupancy x compute units, at most 8 per compute unit */
int nn_search_resident(int ncc, int F) {
	int dev = 0, per_cu = 0, n_cu = 0;
	if (hipGetDevice(&dev) != hipSuccess) return 256;
	const void *fn = ncc ? reinterpret_cast<const void *>(&k_nn_search<true>) : reinterpret_cast<const void *>(&k_nn_search<false>);
	if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0) return 256;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kBlock, nn_search_lds(F)) != hipSuccess || per_cu <= 0) per_cu = 1;
	return n_cu * (per_cu < 8 ? per_cu : 8);
}
int nn_search_blocks(int n_samples, int resident) {
	const int want = (n_samples + 3) / 4;
	return want < resident ? (want > 0 ? want : 1) : resident;
}
/* partials: [Q][nblk] */
void launch_nn_search(int ncc, const double *feat, int n_samples, int F, const double *queries, int Q, NnBest *partials, int nblk, const int *done, hipStream_t st) {
	const dim3 g((unsigned)nblk, (unsigned)Q), blk(kBlock);
	if (ncc) MTFHIP_LAUNCH((k_nn_search<true>), g, blk, nn_search_lds(F), st, feat, n_samples, F, queries, partials, done);
	else MTFHIP_LAUNCH((k_nn_search<false>), g, blk, nn_search_lds(F), st, feat, n_samples, F, queries, partials, done);
}
void launch_nn_search_finish(const NnBest *partials, int nblk, int Q, int *idx, double *dist, hipStream_t st) {
	MTFHIP_LAUNCH(k_nn_search_finish, dim3((unsigned)Q), dim3(64), 0, st, partials, nblk, idx, dist);
}
void launch_nn_pick_update(int ssm, const NnBest *partials, int nblk, const double *perts, int n_samples, double *state, int *ctl, double *log, int it,
	double epsilon, hipStream_t st) {
	if (ssm == MTFHIP_SSM_HOMOGRAPHY) MTFHIP_LAUNCH((k_nn_pick_update<MTFHIP_SSM_HOMOGRAPHY>), dim3(1), dim3(64), 0, st, partials, nblk, perts, n_samples, state, ctl, log, it, epsilon);
	else MTFHIP_LAUNCH((k_nn_pick_update<MTFHIP_SSM_AFFINE>), dim3(1), dim3(64), 0, st, partials, nblk, perts, n_samples, state, ctl, log, it, epsilon);
}

} // namespace mtfhip
