/*
 * mtfhip_lscv_device.h -- the hand-over that ends the localized pass 1 of LSCV (kernels_lscv.hip) and LRSCV (kernels_lrscv.hip): a
 * workgroup adds its (cell, bin) table to the target's u32 sums; the last one of the target to arrive adds the cells of each sub-region,
 * writes the maps (map[b] = sum / count, or b where the count is 0), zeroes the sums for the next launch and, with affine_mapping, fits
 * map_r[k] ~ a_r k + c_r over k = 0 .. n_bins - 1 in FP64.  Which bin keys the table (the template's for LSCV, the current patch's for
 * LRSCV) and which value is summed is the caller's; the arithmetic here is the same for both.
 */
#ifndef MTFHIP_LSCV_DEVICE_H
#define MTFHIP_LSCV_DEVICE_H
#include "mtfhip_device.h"

namespace mtfhip {

/* s_tab: the workgroup's [2][ncell nb] table (sums, then counts), complete (after a __syncthreads); A: LscvArgs or LrscvArgs (nb, nx, ny,
 * ncx, ncell, affine, crng, tot, arrive, map, aff) */
template <class A>
__device__ __forceinline__ void lscv_hand_over(const A &a, int t, int nblk, unsigned *s_tab, int &s_last) {
	const int nb = a.nb, E = a.ncell * nb;
	unsigned *s_sum = s_tab, *s_cnt = s_tab + E;
	unsigned *tot = a.tot + (size_t)t * 2 * E;
	for (int e = threadIdx.x; e < 2 * E; e += kBlock) {
		const unsigned v = s_tab[e];
		if (v) __hip_atomic_fetch_add(tot + e, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	/* the last workgroup of the target to arrive builds the maps (acknowledged sums, then an agent-scope arrival) */
	wait_stores_acked();
	__syncthreads();
	if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(a.arrive + t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nblk - 1u;
	__syncthreads();
	if (!s_last) return;
	if (threadIdx.x == 0) st_coh(a.arrive + t, 0u);
	for (int e = threadIdx.x; e < 2 * E; e += kBlock) { s_tab[e] = ld_coh(tot + e); st_coh(tot + e, 0u); }
	__syncthreads();
	/* LSCV.cc:274-285 / LRSCV.cc:263-277: intensity_map(b) = (the bin's sum) / (its count), or b where the count is 0 */
	const int nx = a.nx, R = a.nx * a.ny;
	double *map = a.map + (size_t)t * R * nb;
	for (int e = threadIdx.x; e < R * nb; e += kBlock) {
		const int r = e / nb, b = e - r * nb, idx = r % nx, idy = r / nx;
		const int cx0 = a.crng[2 * idx], cx1 = a.crng[2 * idx + 1], cy0 = a.crng[2 * nx + 2 * idy], cy1 = a.crng[2 * nx + 2 * idy + 1];
		unsigned long long s = 0, c = 0;
		for (int cy = cy0; cy <= cy1; ++cy)
			for (int cx = cx0; cx <= cx1; ++cx) {
				const int k = (cy * a.ncx + cx) * nb + b;
				s += s_sum[k]; c += s_cnt[k];
			}
		st_coh(map + e, c == 0 ? (double)b : (double)s / (double)c);
	}
	if (!a.affine) return;
	wait_stores_acked();
	__syncthreads();
	/* affine_mapping (LSCV.cc:286-288, LRSCV.cc:279-281): least squares of map against [k, 1], k = 0 .. n_bins - 1, by the normal equations; sum k and
	 * sum k^2 are exact integers */
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (int r = wave; r < R; r += kBlock / 64) {
		double sm = 0.0, skm = 0.0;
		for (int k = lane; k < nb; k += 64) { const double m = ld_coh(map + (size_t)r * nb + k); sm += m; skm += (double)k * m; }
#pragma unroll
		for (int off = 32; off >= 1; off >>= 1) { sm += __shfl_xor(sm, off); skm += __shfl_xor(skm, off); }
		if (lane == 0) {
			const double n = (double)nb, sk = (double)nb * (nb - 1) / 2, skk = (double)(nb - 1) * nb * (2 * nb - 1) / 6;
			const double det = n * skk - sk * sk;
			a.aff[((size_t)t * R + r) * 2] = (n * skm - sk * sm) / det;
			a.aff[((size_t)t * R + r) * 2 + 1] = (skk * sm - sk * skm) / det;
		}
	}
}

} // namespace mtfhip
#endif
