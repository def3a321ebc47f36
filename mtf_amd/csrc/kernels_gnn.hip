/*
 * kernels_gnn.hip -- nt::NN's graph index gnn::GNN on the device (SM/src/NT/GNN.cc:30-203; defaults SM/src/GNNParams.cc:3-7).
 *   k_gnn_dist<NCC>    computeDistances (GNN.cc:30-57) for a panel of rows against every row: a workgroup owns a 64 x 64 block of (i, j)
 *                      pairs, both operand panels staged in LDS sixteen columns at a time (16-byte loads where the row starts on a
 *                      16-byte boundary, 8-byte loads where it does not: rows of odd feat_size alternate), a thread a 4 x 4 block of pairs
 *                      in registers.  Plain FP64 vector arithmetic, one accumulator per pair, the columns in ascending order: SSD in the
 *                      difference form sum (a - b)^2 (SSDBase.cc:576-603; dataset rows are small perturbations of one patch, so the Gram
 *                      form would cancel exactly where the neighbour order is decided), NCC -sum a b (NCC.cc:568-591).  (a - b)^2 and a b
 *                      are symmetric in their operands and the order of a pair's sum depends on feat_size alone, so d(i, j) and d(j, i)
 *                      have the same bits and a row's distances do not depend on the panel it fell into.  Both halves of the matrix are
 *                      computed: a panel's rows are complete without a transposed write into panels that do not exist yet.
 *   k_gnn_select       buildGraph's insertion loop (GNN.cc:71-101) for one row per workgroup: the degree + 1 smallest entries under the
 *                      total order (dist ascending, index ascending), sorted; the first is dropped whatever it is (GNN.cc:98-101: usually the
 *                      row itself, but an identical row at a lower index takes that place and the row keeps itself as a neighbour).  An
 *                      order-preserving 64-bit key of the double, an eight-pass radix select for the (degree + 1)-th key, ties at that key
 *                      to the lower indices, compaction into LDS, a bitonic sort of at most 1024 (key, index) pairs.
 *   k_gnn_init / k_gnn_rows<NCC>
 *                      searchGraph with K = 1 (GNN.cc:115-203).  k_gnn_rows is k_nn_search through an index indirection: the query in
 *                      LDS, a wave per neighbour row, nn_row_dist (mtfhip_nn_search_device.h) -- the exhaustive search's own row sum, so a
 *                      row's distance has the same bits under either index --, the best under (dist, position in the neighbour list) per
 *                      workgroup into a partials array.  The workgroup that finishes last takes their minimum and applies the reference's rule: the best joins
 *                      the visited set; parent_dist <= best ends the walk (GNN.cc:180-183), else the walk moves there (GNN.cc:184-185);
 *                      max_steps ends it too.  Of the visited nodes the one of smallest distance is the answer, of equal distances the one
 *                      visited first (the reference's qsort, GNN.cc:191, leaves that order open).  Every launch returns at once for a walk
 *                      that is done.  No floating-point atomics anywhere: a build and a walk are bit-reproducible.
 * One of the translation units of libmtfhip.so.
 */
#include "mtfhip_device.h"
#include "mtfhip_rng_device.h"
#include "mtfhip_nn_search_device.h"

namespace mtfhip {

constexpr int kGnnKc = 16;   /* columns of the operand panels in LDS at a time */

template <bool NCC>
__global__ __launch_bounds__(kBlock) void k_gnn_dist(const double *feat, int n, int F, int row_lo, int rows, double *out) {
	__shared__ double sA[kGnnTile][kGnnKc + 1], sB[kGnnTile][kGnnKc + 1];   /* (a row stride of 17 doubles: the reads below do not collide) */
	const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
	const int i0 = row_lo + (int)blockIdx.y * kGnnTile, j0 = (int)blockIdx.x * kGnnTile;
	const int i_end = min(n, row_lo + rows);
	double acc[4][4];
#pragma unroll
	for (int r = 0; r < 4; ++r)
#pragma unroll
		for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
	/* entries k, k + 1 of row r; past the row's end and past the last row: zeros, whose terms are +0 for both functors */
	auto stage = [&](double (*s)[kGnnKc + 1], int base, int limit, int k0) {
#pragma unroll
		for (int e = tid; e < kGnnTile * (kGnnKc / 2); e += kBlock) {
			const int rr = e / (kGnnKc / 2), p = e % (kGnnKc / 2), r = base + rr, k = k0 + 2 * p;
			double v0 = 0.0, v1 = 0.0;
			if (r < limit) {
				const size_t at = (size_t)r * (size_t)F + (size_t)k;
				if (k + 1 < F && (at & 1) == 0) { const nns_d2 v = *reinterpret_cast<const nns_d2 *>(feat + at); v0 = v.x; v1 = v.y; }
				else { if (k < F) v0 = feat[at]; if (k + 1 < F) v1 = feat[at + 1]; }
			}
			s[rr][2 * p] = v0; s[rr][2 * p + 1] = v1;
		}
	};
	for (int k0 = 0; k0 < F; k0 += kGnnKc) {
		stage(sA, i0, i_end, k0);
		stage(sB, j0, n, k0);
		__syncthreads();
#pragma unroll
		for (int kk = 0; kk < kGnnKc; ++kk) {
			double a[4], b[4];
#pragma unroll
			for (int r = 0; r < 4; ++r) a[r] = sA[ty + 16 * r][kk];
#pragma unroll
			for (int c = 0; c < 4; ++c) b[c] = sB[tx + 16 * c][kk];
#pragma unroll
			for (int r = 0; r < 4; ++r)
#pragma unroll
				for (int c = 0; c < 4; ++c) {
					if constexpr (NCC) acc[r][c] += a[r] * b[c];
					else { const double d = a[r] - b[c]; acc[r][c] += d * d; }
				}
		}
		__syncthreads();
	}
#pragma unroll
	for (int r = 0; r < 4; ++r) {
		const int i = i0 + ty + 16 * r;
		if (i >= i_end) continue;
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			const int j = j0 + tx + 16 * c;
			if (j < n) out[(size_t)(i - row_lo) * (size_t)n + (size_t)j] = NCC ? -acc[r][c] : acc[r][c];
		}
	}
}

/* keys ascend as the doubles do (-0 and +0, equal as doubles, share a key) */
__device__ __forceinline__ unsigned long long gnn_key(double d) {
	if (d == 0.0) d = 0.0;
	const unsigned long long u = (unsigned long long)__double_as_longlong(d);
	return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__global__ __launch_bounds__(kBlock) void k_gnn_select(const double *dist, int n, int row_lo, int degree, int *graph) {
	__shared__ unsigned hist[256];
	__shared__ unsigned long long skey[kGnnMaxList];
	__shared__ int sidx[kGnnMaxList];
	__shared__ unsigned s_sel, s_rem, s_bucket, s_cnt;
	const int tid = threadIdx.x;
	const double *row = dist + (size_t)blockIdx.x * (size_t)n;
	const int id1 = row_lo + (int)blockIdx.x;
	const unsigned K = (unsigned)degree + 1u;   /* (the launcher: 2 <= K <= min(n, kGnnMaxList)) */
	/* the K-th smallest key, eight bits at a time from the top */
	unsigned long long prefix = 0;
	unsigned remaining = K, bucket = 0;
	for (int pass = 0; pass < 8; ++pass) {
		const int shift = 56 - 8 * pass;
		const unsigned long long hi_mask = pass ? (~0ull << (shift + 8)) : 0ull;
		hist[tid] = 0;
		__syncthreads();
		for (int j = tid; j < n; j += kBlock) {
			const unsigned long long key = gnn_key(row[j]);
			if ((key & hi_mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
		}
		__syncthreads();
		if (tid == 0) {
			unsigned cum = 0, b = 0;
			for (; b < 255; ++b) {
				if (cum + hist[b] >= remaining) break;
				cum += hist[b];
			}
			s_sel = b; s_rem = remaining - cum; s_bucket = hist[b];
		}
		__syncthreads();
		prefix |= (unsigned long long)s_sel << shift;
		remaining = s_rem; bucket = s_bucket;
		__syncthreads();
	}
	/* prefix: the K-th key; `remaining` of the `bucket` entries equal to it belong to the list, those of the lowest indices */
	const bool take_all = remaining == bucket;
	if (tid == 0) s_cnt = 0;
	__syncthreads();
	for (int j = tid; j < n; j += kBlock) {
		const unsigned long long key = gnn_key(row[j]);
		if (key < prefix || (take_all && key == prefix)) {
			const unsigned slot = atomicAdd(&s_cnt, 1u);
			if (slot < (unsigned)kGnnMaxList) { skey[slot] = key; sidx[slot] = j; }
		}
	}
	__syncthreads();
	if (!take_all && tid < 64) {   /* (rare: equal distances across the list's end) one wave walks the row in index order */
		const unsigned base = K - remaining;
		unsigned taken = 0;
		for (int j0 = 0; j0 < n && taken < remaining; j0 += 64) {
			const int j = j0 + tid;
			const bool eq = j < n && gnn_key(row[j]) == prefix;
			const unsigned long long m = __builtin_amdgcn_ballot_w64(eq);
			const unsigned rank = taken + (unsigned)__popcll(m & ((1ull << tid) - 1ull));
			if (eq && rank < remaining) { skey[base + rank] = prefix; sidx[base + rank] = j; }
			taken += (unsigned)__popcll(m);
		}
	}
	unsigned M = 2;
	while (M < K) M <<= 1;
	__syncthreads();
	for (unsigned t = K + tid; t < M; t += kBlock) { skey[t] = ~0ull; sidx[t] = INT_MAX; }
	__syncthreads();
	for (unsigned k = 2; k <= M; k <<= 1)
		for (unsigned j = k >> 1; j > 0; j >>= 1) {
			for (unsigned t = tid; t < (M >> 1); t += kBlock) {
				const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
				const bool up = (i & k) == 0;
				const unsigned long long ka = skey[i], kb = skey[l];
				const int ia = sidx[i], ib = sidx[l];
				const bool a_after_b = ka > kb || (ka == kb && ia > ib);
				if (a_after_b == up) { skey[i] = kb; skey[l] = ka; sidx[i] = ib; sidx[l] = ia; }
			}
			__syncthreads();
		}
	for (int p = tid; p < degree; p += kBlock) graph[(size_t)id1 * (size_t)degree + p] = sidx[p + 1];
}

__global__ __launch_bounds__(kBlock) void k_gnn_init(GnnWalk *walks, int Q, const int *start_nodes, const int *handle_start, int random_start,
	unsigned long long seed, unsigned long long *count, int n, const int *done) {
	if (done && *done) return;
	const unsigned long long c0 = *count;
	__syncthreads();
	for (int q = threadIdx.x; q < Q; q += kBlock) {
		int s;
		if (start_nodes) s = start_nodes[q];
		else if (random_start) s = (int)(philox_uniform(seed, 0x474E4E53u /* "GNNS" */, (unsigned)(c0 + (unsigned long long)q)) * (double)n);
		else s = *handle_start;
		s = s < 0 ? 0 : (s > n - 1 ? n - 1 : s);
		GnnWalk w;
		w.parent_dist = __builtin_inf(); w.best_dist = __builtin_inf();
		w.cur = s; w.best_idx = s; w.start = s; w.n_steps = 0; w.done = 0; w.pad = 0;
		walks[q] = w;
	}
	if (threadIdx.x == 0) *count = c0 + (unsigned long long)Q;
}

/* the rule of one step (or, begin: of the start node), by one thread: (d, pos) the best of the neighbour list under (dist, position) */
__device__ __forceinline__ void gnn_pick(GnnWalk &w, double d, int pos, const int *graph, int degree, int max_steps, int begin) {
	if (begin) {   /* GNN.cc:127-132: the start node is the first visited node */
		w.parent_dist = d; w.best_dist = d;
		w.done = (pos == INT_MAX || degree <= 0 || max_steps <= 0) ? 1 : 0;   /* (no distance below infinity | a node without neighbours) */
		return;
	}
	w.n_steps += 1;
	if (pos == INT_MAX) { w.done = 1; return; }
	const int node = graph[(size_t)w.cur * (size_t)degree + pos];
	if (d < w.best_dist) { w.best_dist = d; w.best_idx = node; }   /* GNN.cc:174-178, 191: the visited node of smallest distance, the earliest of equals */
	if (w.parent_dist <= d) w.done = 1;                            /* GNN.cc:180-183 */
	else { w.cur = node; w.parent_dist = d; }                      /* GNN.cc:184-185 */
	if (w.n_steps >= max_steps) w.done = 1;                        /* GNN.cc:134 */
}

/* One launch per step.  The workgroup that finishes last -- an integer ticket per walk, no floating-point atomics -- takes the minimum of the
 * partials and applies the rule, so a step is one launch; every workgroup has read the walk's state before it draws its ticket, so the
 * last one may overwrite it.  The ticket is back at zero when the launch ends. */
template <bool NCC>
__global__ __launch_bounds__(kBlock) void k_gnn_rows(const double *feat, int n, int F, const double *queries, const int *graph, int degree,
	GnnWalk *walks, NnBest *partials, unsigned *tickets, int max_steps, int begin, const int *done) {
	extern __shared__ nns_d2 gnn_q[];   /* the query, as k_nn_search stages it */
	__shared__ NnBest wbest[4];
	__shared__ int s_last;
	if (done && *done) return;          /* (uniform, in front of every barrier) */
	const int q = blockIdx.y;
	const int cur = walks[q].cur;
	if (!begin && walks[q].done) return;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	nn_stage_query(queries + (size_t)q * F, F, gnn_q);
	__syncthreads();
	const int count = begin ? 1 : degree;
	const int *list = graph + (size_t)cur * (size_t)degree;
	double best = __builtin_inf();
	int bpos = INT_MAX;
	for (int pos = (int)blockIdx.x * 4 + wave; pos < count; pos += (int)gridDim.x * 4) {
		const int r = begin ? cur : list[pos];   /* (uniform per wave) */
		if ((unsigned)r >= (unsigned)n) continue;
		const double d = nn_row_dist<NCC>(feat, r, F, lane, gnn_q);
		if (d < best) { best = d; bpos = pos; }   /* (a wave's positions ascend: the first of equal distances stays) */
	}
	if (lane == 0) { wbest[wave].dist = best; wbest[wave].idx = bpos; }
	__syncthreads();
	NnBest *mine = partials + (size_t)q * gridDim.x;
	if (threadIdx.x == 0) {
		NnBest o = wbest[0];
#pragma unroll
		for (int w = 1; w < 4; ++w) if (nn_better(wbest[w].dist, wbest[w].idx, o.dist, o.idx)) o = wbest[w];
		o.pad = 0;
		mine[blockIdx.x] = o;
		__threadfence();
		s_last = atomicAdd(&tickets[q], 1u) == gridDim.x - 1u ? 1 : 0;
	}
	__syncthreads();
	if (!s_last || threadIdx.x >= 64) return;
	__threadfence();
	const volatile NnBest *vp = mine;   /* (written by other workgroups of this launch) */
	double d = __builtin_inf();
	int pos = INT_MAX;
	for (int k = lane; k < (int)gridDim.x; k += 64) {
		const double pd = vp[k].dist;
		const int pi = vp[k].idx;
		if (nn_better(pd, pi, d, pos)) { d = pd; pos = pi; }
	}
	nn_wave_min(d, pos);
	if (lane != 0) return;
	GnnWalk w = walks[q];
	gnn_pick(w, d, pos, graph, degree, max_steps, begin);
	walks[q] = w;
	tickets[q] = 0u;
}

__global__ __launch_bounds__(kBlock) void k_gnn_results(const GnnWalk *walks, int Q, int *idx, double *dist, int *n_steps) {
	const int q = blockIdx.x * kBlock + threadIdx.x;
	if (q >= Q) return;
	const GnnWalk w = walks[q];
	idx[q] = w.best_idx; dist[q] = w.best_dist;
	if (n_steps) n_steps[q] = w.n_steps;
}

__global__ void k_gnn_to_update(const GnnWalk *walk, NnBest *partial, int *handle_start, int *walk_log, int it, const int *done) {
	if (done && *done) return;
	const GnnWalk w = *walk;
	NnBest o; o.dist = w.best_dist; o.idx = w.best_idx; o.pad = 0;
	*partial = o;
	*handle_start = w.best_idx;   /* GNN.cc:198: the next search starts where this one ended */
	walk_log[2 * it] = w.start; walk_log[2 * it + 1] = w.n_steps;
}

void launch_gnn_dist(int ncc, const double *feat, int n, int F, int row_lo, int rows, double *dist, hipStream_t st) {
	const dim3 g((unsigned)((n + kGnnTile - 1) / kGnnTile), (unsigned)((rows + kGnnTile - 1) / kGnnTile)), blk(kBlock);
	if (ncc) MTFHIP_LAUNCH((k_gnn_dist<true>), g, blk, 0, st, feat, n, F, row_lo, rows, dist);
	else MTFHIP_LAUNCH((k_gnn_dist<false>), g, blk, 0, st, feat, n, F, row_lo, rows, dist);
}
void launch_gnn_select(const double *dist, int n, int row_lo, int rows, int degree, int *graph, hipStream_t st) {
	if (degree < 1 || degree + 1 > kGnnMaxList || degree + 1 > n || rows <= 0) return;
	MTFHIP_LAUNCH(k_gnn_select, dim3((unsigned)rows), dim3(kBlock), 0, st, dist, n, row_lo, degree, graph);
}
/* workgroups of a step: a wave per neighbour row, at most 256 workgroups per walk */
int gnn_step_blocks(int degree) {
	const int want = (degree + 3) / 4;
	return want < 1 ? 1 : (want > 256 ? 256 : want);
}
void launch_gnn_init(GnnWalk *walks, int Q, const int *start_nodes, const int *handle_start, int random_start, unsigned long long seed,
	unsigned long long *count, int n, const int *done, hipStream_t st) {
	MTFHIP_LAUNCH(k_gnn_init, dim3(1), dim3(kBlock), 0, st, walks, Q, start_nodes, handle_start, random_start, seed, count, n, done);
}
void launch_gnn_rows(int ncc, const double *feat, int n, int F, const double *queries, int Q, const int *graph, int degree, GnnWalk *walks,
	NnBest *partials, unsigned *tickets, int nper, int max_steps, int begin, const int *done, hipStream_t st) {
	const dim3 g((unsigned)nper, (unsigned)Q), blk(kBlock);
	const size_t lds = sizeof(double) * (size_t)(F + 2);
	if (ncc) MTFHIP_LAUNCH((k_gnn_rows<true>), g, blk, lds, st, feat, n, F, queries, graph, degree, walks, partials, tickets, max_steps, begin, done);
	else MTFHIP_LAUNCH((k_gnn_rows<false>), g, blk, lds, st, feat, n, F, queries, graph, degree, walks, partials, tickets, max_steps, begin, done);
}
void launch_gnn_results(const GnnWalk *walks, int Q, int *idx, double *dist, int *n_steps, hipStream_t st) {
	MTFHIP_LAUNCH(k_gnn_results, dim3((unsigned)((Q + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, walks, Q, idx, dist, n_steps);
}
void launch_gnn_to_update(const GnnWalk *walk, NnBest *partial, int *handle_start, int *walk_log, int it, const int *done, hipStream_t st) {
	MTFHIP_LAUNCH(k_gnn_to_update, dim3(1), dim3(1), 0, st, walk, partial, handle_start, walk_log, it, done);
}

} // namespace mtfhip
