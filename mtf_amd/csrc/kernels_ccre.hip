/*
 * kernels_ccre.hip -- Cross Cumulative Residual Entropy (AM/src/CCRE.cc, first order, symmetrical_grad = 0, true cumulative histograms):
 * the tables, both gradient vectors with their Jacobian products, and the three first-order Hessians
 * (one of the translation units of libmtfhip.so; conventions and the shared device helpers: mtfhip_device.h)
 *
 * The histogram pass is k_mi_hist<.., CUM> (kernels_mi.hip): the joint histogram of CCRE is the product MI's dense slabs already form, with the
 * cumulative weights of the current patch in the A operand.  Everything here reads the per-target table block of mtfhip_ccre_tables.h.
 */
#include "mtfhip_ccre_device.h"

namespace mtfhip {

/* the block rows of up to three histogram passes summed in a fixed order, then ccre_tables (mtfhip_ccre_tables.h) by the whole workgroup:
 * pre-seeding, logs, ccre_log_term, f, the column sums of the cumulative joint histogram and the prefix table the init-side passes read.
 * Row: [nb | nb*nb] cumulative (A, I0)  |  [nb | nb*nb] cumulative (It, It), with_self  |  [nb | .] the plain histogram of I0 / of It */
__global__ __launch_bounds__(kBlock) void k_ccre_tables(int nb, double pre_seed, double norm_mult, int mode, int with_self, const double *partials,
	int nblk, int row_len, double *tb_all, double *f_out) {
	__shared__ double raw[3 * (CCRE_NB + CCRE_NB * CCRE_NB)];
	__shared__ double red[kBlock];
	const int t = blockIdx.x, R = nb + nb * nb;
	const double *p = partials + (size_t)t * nblk * row_len;
	for (int k = threadIdx.x; k < 3 * R; k += kBlock) {
		const int seg = k / R;
		const bool need = seg == 0 ? mode != CCRE_TB_HIST0 : (seg == 1 ? with_self != 0 : ((mode != CCRE_TB_UPDATE || with_self) && k - 2 * R < nb));
		raw[k] = need ? column_sum(p + k, nblk, row_len) : 0.0;
	}
	__syncthreads();
	ccre_tables(threadIdx.x, kBlock, [] { __syncthreads(); }, nb, pre_seed, norm_mult, mode, with_self, raw, tb_all + (size_t)t * MI_SIZE, red, f_out + t);
}

/* Both gradient vectors per pixel and their Jacobian products in one pass (the shape of k_mi_grad_gemv):
 *   df_dIt = sum_{i, j in the two windows} C'_i(It) beta_j(I0) L(i, j)                                         updateCurrGrad CCRE.cc:465-476
 *   df_dI0 = sum_{j in window} beta'_j(I0) [ sum_i C_i(It) (1 + L(i, j)) - cum_joint_hist_sum(j) / init_hist(j) ]  updateInitGrad :425-464
 * and df_dIt . Jt, df_dI0 . J0 (AppearanceModel's cmptCurrJacobian / cmptInitJacobian).  Jt / J0 / the outputs may be NULL.
 * Block partial rows: [8 | 8]. */
__global__ __launch_bounds__(kBlock) void k_ccre_grad_gemv(int N, int S, int nb, double norm_mult, const double *It_all, const double *I0_all,
	const double *tb_all, const double *Jt_all, const double *J0_all, MiJ0Rebuild rb, double *dft_out, double *df0_out, double *partials, int nblk) {
	__shared__ double L[CCRE_NB * CCRE_NB], P[CCRE_NB * CCRE_NB], Rt[CCRE_NB];
	__shared__ double lds[4 * 16];
	const int t = blockIdx.y;
	const double *tb = tb_all + (size_t)t * MI_SIZE;
	for (int k = threadIdx.x; k < CCRE_NB * CCRE_NB; k += kBlock) { L[k] = tb[CCRE_L + k]; P[k] = tb[CCRE_P + k]; }
	if (threadIdx.x < CCRE_NB) Rt[threadIdx.x] = tb[CCRE_RATIO + threadIdx.x];
	__syncthreads();
	const double *It = It_all + (size_t)t * N, *I0 = I0_all + (size_t)t * N;
	const double *Jt = Jt_all ? Jt_all + (size_t)t * N * S : nullptr, *J0 = J0_all ? J0_all + (size_t)t * N * S : nullptr;
	double acc[16];
#pragma unroll
	for (int k = 0; k < 16; ++k) acc[k] = 0.0;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
		double jt[kMaxS], j0[kMaxS];
#pragma unroll
		for (int s = 0; s < kMaxS; ++s) { jt[s] = (Jt && s < S) ? Jt[(size_t)s * N + i] : 0.0; j0[s] = (J0 && !rb.dI0 && s < S) ? J0[(size_t)s * N + i] : 0.0; }
		if (J0 && rb.dI0) {
			/* the template's steepest-descent row rebuilt from dI0_dx and the grid point, as k_mi_grad_gemv does (kernels_mi.hip) */
			const double *g0 = rb.dI0 + (size_t)t * 2 * N;
			const double g0x = g0[i], g0y = g0[(size_t)N + i];
			const double2 p0 = reinterpret_cast<const double2 *>(rb.pts + (size_t)t * 2 * N)[i];
			if (rb.hom) {
				double Ix0 = g0x, Iy0 = g0y;
				if (!rb.init_variant) { const double inv = 1.0 / (rb.z ? rb.z[(size_t)t * N + i] : 1.0); Ix0 = g0x * inv; Iy0 = g0y * inv; }
				hom_row(j0, Ix0, Iy0, p0.x, p0.y, p0.x, p0.y);
			} else {
				j0[0] = g0x; j0[1] = g0y; j0[2] = g0x * p0.x; j0[3] = g0x * p0.y; j0[4] = g0y * p0.x; j0[5] = g0y * p0.y; j0[6] = j0[7] = 0.0;
			}
		}
		const BsplWin a = cum_window(It[i], nb, norm_mult);
		const BsplWin c0 = bspl_window(I0[i], nb, norm_mult, false);
		double dft = 0, df0 = 0;
#pragma unroll
		for (int r = 0; r < 4; ++r)
#pragma unroll
			for (int c = 0; c < 4; ++c)
				if (r < a.n && c < c0.n) dft += a.d[r] * c0.w[c] * L[(a.lo + r) * CCRE_NB + c0.lo + c];
#pragma unroll
		for (int c = 0; c < 4; ++c)
			if (c < c0.n) df0 += c0.d[c] * (ccre_cum_dot(a, L, P, c0.lo + c) - Rt[c0.lo + c]);
		if (dft_out) dft_out[(size_t)t * N + i] = dft;
		if (df0_out) df0_out[(size_t)t * N + i] = df0;
#pragma unroll
		for (int s = 0; s < kMaxS; ++s) { acc[s] = fma(dft, jt[s], acc[s]); acc[8 + s] = fma(df0, j0[s], acc[8 + s]); }
	}
	block_reduce_store<16>(acc, partials + ((size_t)t * nblk + blockIdx.x) * 16, lds);
}

/* The first-order Hessians on k_mi_hess's slab scheme (pixel mode: lane p writes its pixel's dense bin vectors; bin mode: lane q owns the bin
 * pairs q, q + 64 .. and walks the 64 staged pixels -- no atomics, a fixed order).
 *  !INIT  cmptCurrHessian (CCRE.cc:564-602; B = I0, table CCRE_L) and cmptSelfHessian (:644-678; B = It, table CCRE_SELF_L):
 *           Hsum += [sum_i C''_i sum_j beta_j(B) T(i, j)] Jrow Jrow^T,   Q[(i, j)] += C'_i(It) beta_j(B) Jrow
 *   INIT  cmptInitHessian (:521-560; B = I0, J = J0):
 *           Hsum += [sum_j beta''_j (sum_i C_i (1 + L(i, j)) - cum_joint_hist_sum(j) / init_hist(j))] Jrow Jrow^T,
 *           Q[(i, j)] += C_i(It) beta'_j(I0) Jrow with C DENSE (1 below the window: cum_fill),   G[j] += beta'_j(I0) Jrow
 * Block partial rows: [36 Hsum | nb*nb*S Q | nb*S G (INIT)] */
template <bool INIT>
__global__ __launch_bounds__(kBlock) void k_ccre_hess(int N, int S, int nb, double norm_mult, const double *It_all, const double *B_all,
	const double *tb_all, int table_off, const double *J_all, double *partials, int nblk, int row_len) {
	extern __shared__ __attribute__((aligned(16))) double dyn[];
	constexpr int RS = kMiRow;
	double *T = dyn;                                     /* CCRE_NB^2: ccre_log_term / self_ccre_log_term */
	double *P = T + CCRE_NB * CCRE_NB;                   /* CCRE_NB^2 prefix table (INIT) */
	double *Rt = P + CCRE_NB * CCRE_NB;                  /* CCRE_NB (INIT) */
	double *red = Rt + CCRE_NB;                          /* 4 * 36 */
	double *slabs = red + 4 * 36;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int slab = RS * (2 * nb + kMaxS);
	double *gd = slabs + (size_t)wave * slab;            /* [nb][65] the cumulative side: C' (window), or C (dense) for INIT */
	double *wd = gd + nb * RS;                           /* [nb][65] the plain side: beta, or beta' for INIT */
	double *rw = wd + nb * RS;                           /* [kMaxS][65] J rows */
	const int t = blockIdx.y;
	const double *tb = tb_all + (size_t)t * MI_SIZE;
	for (int k2 = threadIdx.x; k2 < CCRE_NB * CCRE_NB; k2 += kBlock) { T[k2] = tb[table_off + k2]; P[k2] = INIT ? tb[CCRE_P + k2] : 0.0; }
	if (threadIdx.x < CCRE_NB) Rt[threadIdx.x] = INIT ? tb[CCRE_RATIO + threadIdx.x] : 0.0;
	__syncthreads();
	const double *A = It_all + (size_t)t * N, *Bv = B_all + (size_t)t * N;
	const double *J = J_all + (size_t)t * N * S;
	double acc[36];
#pragma unroll
	for (int k2 = 0; k2 < 36; ++k2) acc[k2] = 0.0;
	double accq[kMiPairs][kMaxS], accg[kMaxS];
	int pr[kMiPairs], pc[kMiPairs];
#pragma unroll
	for (int m = 0; m < kMiPairs; ++m) {
		const int q = lane + 64 * m;
		pr[m] = q < nb * nb ? q / nb : -1; pc[m] = q < nb * nb ? q % nb : 0;
#pragma unroll
		for (int s = 0; s < kMaxS; ++s) accq[m][s] = 0.0;
	}
#pragma unroll
	for (int s = 0; s < kMaxS; ++s) accg[s] = 0.0;
	for (int base = (blockIdx.x * (kBlock / 64) + wave) * 64; base < N; base += nblk * kBlock) {
		const int i = base + lane;
		double row[kMaxS];
#pragma unroll
		for (int s = 0; s < kMaxS; ++s) row[s] = (i < N && s < S) ? J[(size_t)s * N + i] : 0.0;
		for (int k2 = 0; k2 < nb; ++k2) { gd[k2 * RS + lane] = 0.0; wd[k2 * RS + lane] = 0.0; }
		if (i < N) {
			const BsplWin a = cum_window(A[i], nb, norm_mult);
			const BsplWin b = bspl_window(Bv[i], nb, norm_mult, INIT);
			double hess_term = 0;
			if constexpr (INIT) {
				/* scalar_term, CCRE.cc:550-557 */
#pragma unroll
				for (int c = 0; c < 4; ++c) if (c < b.n) hess_term += b.h[c] * (ccre_cum_dot(a, T, P, b.lo + c) - Rt[b.lo + c]);
				cum_fill<RS>(gd, lane, a, nb);
#pragma unroll
				for (int c = 0; c < 4; ++c) if (c < b.n) wd[(b.lo + c) * RS + lane] = b.d[c];
			} else {
				/* hist_hess_term, CCRE.cc:580-591, :658-668 */
#pragma unroll
				for (int r = 0; r < 4; ++r) {
					if (r < a.n) {
						double inner = 0;
#pragma unroll
						for (int c = 0; c < 4; ++c) if (c < b.n) inner += b.w[c] * T[(a.lo + r) * CCRE_NB + b.lo + c];
						hess_term += a.h[r] * inner;
						gd[(a.lo + r) * RS + lane] = a.d[r];
					}
				}
#pragma unroll
				for (int c = 0; c < 4; ++c) if (c < b.n) wd[(b.lo + c) * RS + lane] = b.w[c];
			}
			int k2 = 0;
#pragma unroll
			for (int x = 0; x < kMaxS; ++x) {
				const double hx = hess_term * row[x];
#pragma unroll
				for (int y = x; y < kMaxS; ++y) { acc[k2] = fma(hx, row[y], acc[k2]); ++k2; }
			}
		}
#pragma unroll
		for (int s = 0; s < kMaxS; ++s) rw[s * RS + lane] = row[s];
		__builtin_amdgcn_wave_barrier();
#pragma unroll 4
		for (int p = 0; p < 64; ++p) {
			double jr[kMaxS];
#pragma unroll
			for (int s = 0; s < kMaxS; ++s) jr[s] = rw[s * RS + p];
#pragma unroll
			for (int m = 0; m < kMiPairs; ++m) {
				if (pr[m] >= 0) {
					const double gr = gd[pr[m] * RS + p] * wd[pc[m] * RS + p];
#pragma unroll
					for (int s = 0; s < kMaxS; ++s) accq[m][s] = fma(gr, jr[s], accq[m][s]);
				}
			}
			if constexpr (INIT) {
				if (lane < nb) {
					const double g = wd[lane * RS + p];
#pragma unroll
					for (int s = 0; s < kMaxS; ++s) accg[s] = fma(g, jr[s], accg[s]);
				}
			}
		}
		__builtin_amdgcn_wave_barrier();
	}
	double *dst = partials + ((size_t)t * nblk + blockIdx.x) * row_len;
	const int ql = nb * nb * S + (INIT ? nb * S : 0);
	block_reduce_store<36>(acc, dst, red);
	__syncthreads();
	/* the four waves' Q (and G) blocks through the (now free) slabs: [4][ql], summed in wave order */
	double *qred = slabs;
#pragma unroll
	for (int m = 0; m < kMiPairs; ++m) {
		if (pr[m] >= 0) {
#pragma unroll
			for (int s = 0; s < kMaxS; ++s) if (s < S) qred[wave * ql + (pr[m] * nb + pc[m]) * S + s] = accq[m][s];
		}
	}
	if constexpr (INIT) {
		if (lane < nb) {
#pragma unroll
			for (int s = 0; s < kMaxS; ++s) if (s < S) qred[wave * ql + nb * nb * S + lane * S + s] = accg[s];
		}
	}
	__syncthreads();
	for (int k2 = threadIdx.x; k2 < ql; k2 += kBlock)
		dst[36 + k2] = (qred[k2] + qred[ql + k2]) + (qred[2 * ql + k2] + qred[3 * ql + k2]);
}
/* one reduced row per target -> the S x S Hessian (column-major, as k_mi_hess_finish): Hsum + the bin-pair terms
 * (CCRE.cc:595-601, :671-677; init: :532-545 through ccre_init_pair / ccre_init_bin, which is not symmetric) */
__global__ __launch_bounds__(kBlock) void k_ccre_hess_finish(int S, int nb, int init, const double *rows, int row_len, const double *tb_all,
	int joint_off, double *out) {
	const int t = blockIdx.x;
	const double *p = rows + (size_t)t * row_len, *tb = tb_all + (size_t)t * MI_SIZE;
	const double *Q = p + 36, *G = Q + (size_t)nb * nb * S;
	if (threadIdx.x < 64) {
		const int r2 = threadIdx.x >> 3, c2 = threadIdx.x & 7;
		if (r2 < S && c2 < S) {
			const int a = r2 < c2 ? r2 : c2, b2 = r2 < c2 ? c2 : r2;
			double h = p[a * 8 - (a * (a - 1)) / 2 + (b2 - a)];
			for (int i = 0; i < nb; ++i)
				for (int j = 0; j < nb; ++j) {
					const double jv = tb[joint_off + i * CCRE_NB + j];
					const double *q = Q + (size_t)(i * nb + j) * S;
					if (init) h += ccre_init_pair(q[r2], q[c2], G[j * S + c2], jv, tb[CCRE_HIST_0 + j]);
					else h += q[r2] * q[c2] * ccre_hess_factor(jv, tb[CCRE_CUM_T + i]);
				}
			if (init)
				for (int j = 0; j < nb; ++j) h += ccre_init_bin(G[j * S + r2], G[j * S + c2], tb[CCRE_COLSUM + j], tb[CCRE_HIST_0 + j]);
			out[(size_t)t * 64 + c2 * S + r2] = h;
		}
	}
}

/* ===================================================================== */
/* launchers                                                              */
/* ===================================================================== */
void launch_ccre_tables(const BatchView &bv, int nb, double pre_seed, double norm_mult, int mode, int with_self, const double *partials, int nblk,
	int row_len, double *tb, double *f_out, hipStream_t st) {
	MTFHIP_LAUNCH(k_ccre_tables, dim3(bv.B), dim3(kBlock), 0, st, nb, pre_seed, norm_mult, mode, with_self, partials, nblk, row_len, tb, f_out);
}
void launch_ccre_grad_gemv(const BatchView &bv, int nb, double norm_mult, const double *It, const double *I0, const double *tb,
	const double *Jt, const double *J0, const MiJ0Rebuild &rb, double *df_dIt, double *df_dI0, double *partials, int nblk, hipStream_t st) {
	MTFHIP_LAUNCH(k_ccre_grad_gemv, grid2(nblk, bv.B), dim3(kBlock), 0, st, bv.N, bv.S, nb, norm_mult, It, I0, tb, Jt, J0, rb, df_dIt, df_dI0,
		partials, nblk);
}
/* kind 0 init (J = J0), 1 curr, 2 self */
void launch_ccre_hess(const BatchView &bv, int nb, double norm_mult, int kind, const double *It, const double *I0, const double *tb, const double *J,
	double *partials, int nblk, int row_len, hipStream_t st) {
	const int ql = nb * nb * bv.S + nb * bv.S;
	const size_t slabs = std::max<size_t>((size_t)4 * kMiRow * (2 * nb + kMaxS), (size_t)4 * ql);
	const size_t lds = sizeof(double) * (2 * CCRE_NB * CCRE_NB + CCRE_NB + 4 * 36 + slabs);
	static bool attr_set = false;
	if (!attr_set) {   /* 16 bins need more dynamic LDS than the default 64 KB cap (as k_mi_hess) */
		(void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_ccre_hess<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
		(void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_ccre_hess<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
		attr_set = true;
	}
	if (kind == 0)
		MTFHIP_LAUNCH(k_ccre_hess<true>, grid2(nblk, bv.B), dim3(kBlock), lds, st, bv.N, bv.S, nb, norm_mult, It, I0, tb, (int)CCRE_L, J, partials, nblk, row_len);
	else
		MTFHIP_LAUNCH(k_ccre_hess<false>, grid2(nblk, bv.B), dim3(kBlock), lds, st, bv.N, bv.S, nb, norm_mult, It, kind == 1 ? I0 : It, tb,
			(int)(kind == 1 ? CCRE_L : CCRE_SELF_L), J, partials, nblk, row_len);
}
void launch_ccre_hess_finish(const BatchView &bv, int nb, int kind, const double *rows, int row_len, const double *tb, double *out, hipStream_t st) {
	MTFHIP_LAUNCH(k_ccre_hess_finish, dim3(bv.B), dim3(kBlock), 0, st, bv.S, nb, kind == 0 ? 1 : 0, rows, row_len, tb,
		(int)(kind == 2 ? CCRE_SELF_JOINT : CCRE_JOINT), out);
}

} // namespace mtfhip
