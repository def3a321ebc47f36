/*
 * mtfhip_ccre_device.h -- device helpers of the CCRE translation unit (kernels_ccre.hip): the table block's layout and algebra
 * (mtfhip_ccre_tables.h, shared with the host) and the per-pixel expressions of CCRE.cc over the windows of mtfhip_mi_device.h
 */
#ifndef MTFHIP_CCRE_DEVICE_H
#define MTFHIP_CCRE_DEVICE_H
#include "mtfhip_mi_device.h"
#include "mtfhip_ccre_tables.h"

namespace mtfhip {

static_assert(CCRE_NB == MI_NB && CCRE_SIZE <= MI_SIZE, "a CCRE batch keeps its tables in the block an MI batch has");

/* sum_i C_i(p) (1 + ccre_log_term(i, j)) over ALL bins i, for one template bin j (CCRE.cc:440-457, :552-555): the rows below the window,
 * where C = 1, come from the prefix table P; above the window C = 0 (what the reference leaves there is state: include/mtfhip.h).
 * a: cum_window of It(p); L, P: the [CCRE_NB][CCRE_NB] tables in LDS */
__device__ __forceinline__ double ccre_cum_dot(const BsplWin &a, const double *L, const double *P, int j) {
	double s = P[min(a.lo, CCRE_NB - 1) * CCRE_NB + j];   /* (the clamp: a value past the last bin reads inside the table) */
#pragma unroll
	for (int r = 0; r < 4; ++r) if (r < a.n) s += a.w[r] * (1 + L[(a.lo + r) * CCRE_NB + j]);
	return s;
}

} // namespace mtfhip
#endif
