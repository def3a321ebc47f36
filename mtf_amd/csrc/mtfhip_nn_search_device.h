/*
 * mtfhip_nn_search_device.h -- what nt::NN's two indices share on the device (kernels_nn_search.hip: the exhaustive search; kernels_gnn.hip:
 * the graph walk): the distance of one stored row to the query staged in LDS, by one wave, and the exact minimum of (dist, index) pairs.
 * ONE body for both, so that a row has the same distance bits whichever index asks for it.
 */
#pragma once
#include "mtfhip_device.h"
#include <climits>
#include <type_traits>

namespace mtfhip {

typedef double nns_d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool nn_better(double d, int i, double bd, int bi) { return d < bd || (d == bd && i < bi); }

/* the wave's minimum of (d, i), in every lane */
__device__ __forceinline__ void nn_wave_min(double &d, int &i) {
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) {
		const double od = __shfl_xor(d, m);
		const int oi = __shfl_xor(i, m);
		if (nn_better(od, oi, d, i)) { d = od; i = oi; }
	}
}
/* the minimum of n partials, by one wave */
__device__ __forceinline__ void nn_reduce_partials(const NnBest *part, int n, double &d, int &i) {
	d = __builtin_inf(); i = INT_MAX;
	for (int k = (int)(threadIdx.x & 63); k < n; k += 64) {
		const NnBest p = part[k];
		if (nn_better(p.dist, p.idx, d, i)) { d = p.dist; i = p.idx; }
	}
	nn_wave_min(d, i);
}

/* The distance functor of row r (F entries at `row`) to the query in LDS -- nns_q: (F + 1) / 2 pairs, a zero behind an odd row --, by one
 * wave, in every lane: SSDBaseDist (AM/src/SSDBase.cc:576-603: sum (a - b)^2) or NCCDist (AM/src/NCC.cc:568-591: -sum a b).  A lane takes
 * the element pairs lane, lane + 64, ... of the row, read as 16 bytes where the row starts on a 16-byte boundary and as two 8-byte loads
 * where it does not.  The order of the sum depends on F alone: four accumulators per lane, a fixed DPP tree. */
template <bool NCC>
__device__ __forceinline__ double nn_row_dist(const double *feat, int r, int F, int lane, const nns_d2 *nns_q) {
	const double *sq = reinterpret_cast<const double *>(nns_q);
	const double *row = feat + (size_t)r * F;
	const int P = F >> 1;               /* whole pairs of a row */
	auto term = [](double a, double b) { if constexpr (NCC) return a * b; else { const double d = a - b; return d * d; } };
	/* ONE body for both alignments: only the loads differ, the arithmetic and its order do not */
	auto body = [&](auto wide_tag) -> double {
		constexpr bool WIDE = decltype(wide_tag)::value;
		auto ld = [&](int p) -> nns_d2 {
			if constexpr (WIDE) return reinterpret_cast<const nns_d2 *>(row)[p];
			else { nns_d2 v; v.x = row[2 * p]; v.y = row[2 * p + 1]; return v; }
		};
		double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
		int p = lane;
		for (; p + 192 < P; p += 256) {   /* four loads in flight per lane */
			const nns_d2 v0 = ld(p), v1 = ld(p + 64), v2 = ld(p + 128), v3 = ld(p + 192);
			const nns_d2 q0 = nns_q[p], q1 = nns_q[p + 64], q2 = nns_q[p + 128], q3 = nns_q[p + 192];
			a0 += term(v0.x, q0.x); a0 += term(v0.y, q0.y);
			a1 += term(v1.x, q1.x); a1 += term(v1.y, q1.y);
			a2 += term(v2.x, q2.x); a2 += term(v2.y, q2.y);
			a3 += term(v3.x, q3.x); a3 += term(v3.y, q3.y);
		}
		for (; p < P; p += 64) {
			const nns_d2 v0 = ld(p), q0 = nns_q[p];
			a0 += term(v0.x, q0.x); a0 += term(v0.y, q0.y);
		}
		if ((F & 1) && lane == (P & 63)) a0 += term(row[F - 1], sq[F - 1]);   /* the last entry of an odd row */
		return (a0 + a1) + (a2 + a3);
	};
	const bool wide = (((size_t)r * (size_t)F) & 1) == 0;   /* (uniform per wave) the row starts on a 16-byte boundary */
	double s = wide ? body(std::true_type{}) : body(std::false_type{});
	s = wave_sum_dpp(s);
	return NCC ? -s : s;
}

/* the query into LDS as nn_row_dist reads it (every thread of the workgroup; a barrier behind it is the caller's) */
__device__ __forceinline__ void nn_stage_query(const double *q, int F, nns_d2 *nns_q) {
	double *sq = reinterpret_cast<double *>(nns_q);
	for (int i = threadIdx.x; i < F; i += blockDim.x) sq[i] = q[i];
	if (threadIdx.x == 0 && (F & 1)) sq[F] = 0.0;
}

} // namespace mtfhip
