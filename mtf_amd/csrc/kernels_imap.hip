/*
 * kernels_imap.hip -- the intensity maps of the SCV family (AM/src/SCV.cc, RSCV.cc, LSCV.cc, LRSCV.cc): four models that are SSD behind
 * a map built from per-bin histogram sums.  SCV and LSCV re-map the template through E[It | I0_orig] in front of
 * SSDBase::updateSimilarity (SCV.cc:194-230, LSCV.cc:263-304), so everything behind these kernels is the SSD path (the fused SSD kernels
 * of kernels_fused.hip, unchanged, read the re-mapped I0 from MTFHIP_BUF_I0).  RSCV and LRSCV map the current patch through E[I0 | It]
 * in updatePixVals (RSCV.cc:170-238, LRSCV.cc:224-292); their maps are applied inside the fused pass (kernels_fused_rscv.hip,
 * kernels_fused_lrscv.hip) or, on the per-function path, by k_rscv_apply / k_lrscv_apply.
 *
 * Pass 1 is one mechanism (mtfhip_imap_device.h: imap_walk): It of every pixel -- sampled at the current warp with the arithmetic of the
 * pass that follows, or read from a buffer on the per-function path -- and two sums per bin, so the n_bins^2 joint histogram never
 * exists.  Reads 16 B/px (grid point) + 4 texels + the code plane.  The four endings:
 *
 *   k_scv_hist    map[b] = sum_i i joint(i, b) / init_hist(b), per template bin b:
 *                   Dirac:    sum over the pixels of template bin b of (int)It, and their count (code plane, 2 B/px);
 *                   Bilinear: t_wt It and t_wt into column b_0, b_wt It and b_wt into column b_0 + 1 (l p + r (p + 1) = It; I0_orig, 8 B/px).
 *                 One row of 2 n_bins sums per workgroup; k_scv_map sums the rows in workgroup order and divides, with the reference's
 *                 empty-bin rule (map[b] = b where init_hist(b) == 0); k_scv_remap: I0 = map(I0_orig), nearest (map[(int)rint(x)]) from
 *                 the code plane (2 B/px) or linear from I0_orig (8 B/px); 8 B/px out.
 *   k_rscv_hist   map[b] = sum_j j joint(b, j) / curr_hist(b), per CURRENT bin b: sum over the pixels of bin (int)It_orig of (int)I0
 *                 (code plane, 1 B/px), and their count.  LDS u32 atomics, one row of 2 n_bins sums per workgroup; the last workgroup
 *                 of a target to arrive sums the rows into 64-bit integers and writes the map (map[b] = b where curr_hist(b) == 0).
 *   k_lscv_hist   SCV's Dirac sums per sub-region r.  The sub-region boundaries cut the patch into at most (2 n_x - 1)(2 n_y - 1) cells,
 *                 and every pixel of a cell lies in the same sub-regions (cell plane, 2 B/px, one per batch): a workgroup adds one u32
 *                 pair per pixel into its (cell, template bin) table in LDS, then lscv_hand_over -- the target's u32 sums by agent-scope
 *                 atomics, the last-arriving workgroup's maps, the FP64 affine fit with affine_mapping, the sums zeroed for the next
 *                 launch.  k_lscv_remap: I0 = sum over idx (outer), idy (inner) of w(i, r) mapped_r(I0_orig), each product rounded, no
 *                 FMA: the reference's order and rounding.  Nearest reads the code plane, linear and affine I0_orig; the weights are one
 *                 [n_sub][N] table per batch (8 n_sub B/px, shared by the batch's targets); 8 B/px out.
 *   k_lrscv_hist  RSCV's sums per sub-region r, keyed by (cell, current bin) on LSCV's cell plane, then lscv_hand_over.
 *
 * Reproducibility.  Dirac sums are integers, exact in any order (u32 per workgroup: at most 255 x 2^26 / 64 < 2^32 per bin; the localized
 * models' u32 per target: imap_capture refuses patches where (n_bins - 1) N could overflow one; u64 across RSCV's workgroups), and stay
 * exact as doubles.  SCV's Bilinear sums have a fixed order: the 256 pixels of a chunk are staged in LDS, wave w owns the pixels
 * [64 w, 64 w + 64) of the chunk and lane l the bins l, l + 64, l + 128, l + 192, and adds its pixels in pixel order; the four waves'
 * tables are summed in wave order at the end, and the workgroup rows by k_scv_map in workgroup order.  The affine fit sums in a fixed
 * order (lane l takes k = l, l + 64, ..., in order; then a xor butterfly, whose every step adds the same two values on both lanes).  So
 * every map is identical run to run, and the Dirac ones equal the float64 reference's.
 */
#include "mtfhip_imap_device.h"

namespace mtfhip {

/* per pixel of I0_orig: (int)I0_orig (the Dirac / Bilinear template bin) | (int)rint(I0_orig) << 8 (the nearest mapping's index) */
__global__ __launch_bounds__(kBlock) void k_scv_codes(int N, int nb, const double *i0o, unsigned short *code) {
	const int t = blockIdx.y;
	const double *x = i0o + (size_t)t * N;
	unsigned short *c = code + (size_t)t * N;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
		const double v = x[i];
		c[i] = (unsigned short)(imap_bin((int)v, nb) | (imap_bin((int)rint(v), nb) << 8));
	}
}

/* per pixel of I0: (int)I0, the template's column of the joint histogram */
__global__ __launch_bounds__(kBlock) void k_rscv_codes(int N, int nb, const double *i0, unsigned char *code) {
	const int t = blockIdx.y;
	const double *x = i0 + (size_t)t * N;
	unsigned char *c = code + (size_t)t * N;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) c[i] = (unsigned char)imap_bin((int)x[i], nb);
}

template <int SSM, int KIND>
__global__ __launch_bounds__(kBlock) void k_scv_hist(BatchView bv, ImgView im, ImapArgs a, int nblk) {
	__shared__ int s_bin[kBlock];
	__shared__ double s_v0[kBlock], s_w0[kBlock], s_v1[kBlock], s_w1[kBlock];
	__shared__ double s_tab[4][2][kImapMaxBins];
	__shared__ unsigned s_isum[kImapMaxBins], s_icnt[kImapMaxBins];   /* Dirac: integer sums, exact in any order */
	const int t = blockIdx.y;
	if (a.active && !a.active[t]) return;
	const int N = bv.N, nb = a.nb, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const bool bil = a.hist == 1;
	const unsigned short *code = a.code16 + (size_t)t * N;
	const double *i0o = a.i0o + (size_t)t * N;
	double s[4] = {0.0, 0.0, 0.0, 0.0}, w[4] = {0.0, 0.0, 0.0, 0.0};
	const int nk = (nb + 63) >> 6;   /* bin slots per lane in use */
	if (!bil) {
		for (int b = threadIdx.x; b < kImapMaxBins; b += kBlock) { s_isum[b] = 0u; s_icnt[b] = 0u; }
		__syncthreads();
	}
	imap_walk<SSM, KIND>(bv, im, a, t, nblk, [&](int i, auto it) {
		int bin = -2;   /* (no bin: a padding pixel of the last chunk) */
		double v0 = 0.0, w0 = 0.0, v1 = 0.0, w1 = 0.0;
		if (i < N) {
			const double itv = it();
			if (bil) {
				/* getBilinearJointHist (histUtils.cc:421-461) with I0_orig as the second image */
				const double x0 = i0o[i];
				const int b0 = (int)x0;
				const double b_wt = x0 - b0, t_wt = 1 - b_wt;
				bin = imap_bin(b0, nb);
				v0 = t_wt * itv; w0 = t_wt;
				if (b_wt != 0 && bin + 1 < nb) { v1 = b_wt * itv; w1 = b_wt; }
			} else {
				/* getDiracJointHist (histUtils.cc:370-394): joint((int)It, (int)I0_orig) += 1 */
				bin = code[i] & 0xff;
				v0 = (double)imap_bin((int)itv, nb); w0 = 1.0;
			}
		}
		if (!bil) {
			/* (a workgroup sums at most 255 x 2^26 / 64 < 2^32: no u32 overflow) */
			if (bin >= 0) { atomicAdd(&s_isum[bin], (unsigned)v0); atomicAdd(&s_icnt[bin], 1u); }
			return;
		}
		/* every chunk needs all 256 threads at its two barriers, the padding lanes included */
		s_bin[threadIdx.x] = bin; s_v0[threadIdx.x] = v0; s_w0[threadIdx.x] = w0; s_v1[threadIdx.x] = v1; s_w1[threadIdx.x] = w1;
		__syncthreads();
		const int j0 = wave * 64;
		for (int j = j0; j < j0 + 64; ++j) {
			const int bj = s_bin[j];   /* (one LDS broadcast per pixel) */
			const double a0 = s_v0[j], c0 = s_w0[j];
			const double a1 = s_v1[j], c1 = s_w1[j];
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				if (k >= nk) break;   /* (uniform) */
				if (bj == lane + 64 * k) { s[k] += a0; w[k] += c0; }
				if (bj + 1 == lane + 64 * k) { s[k] += a1; w[k] += c1; }
			}
		}
		__syncthreads();
	});
	double *row = a.part_f + ((size_t)t * nblk + blockIdx.x) * 2 * nb;
	if (!bil) {
		__syncthreads();
		for (int b = threadIdx.x; b < nb; b += kBlock) { row[b] = (double)s_isum[b]; row[nb + b] = (double)s_icnt[b]; }
		return;
	}
#pragma unroll
	for (int k = 0; k < 4; ++k) { s_tab[wave][0][lane + 64 * k] = s[k]; s_tab[wave][1][lane + 64 * k] = w[k]; }
	__syncthreads();
	for (int b = threadIdx.x; b < nb; b += kBlock) {
		double ss = s_tab[0][0][b], ww = s_tab[0][1][b];
		for (int q = 1; q < 4; ++q) { ss += s_tab[q][0][b]; ww += s_tab[q][1][b]; }
		row[b] = ss; row[nb + b] = ww;
	}
}

/* SCV::updateSimilarity SCV.cc:208-229: intensity_map(b) = wt_sum / init_hist(b), or b where init_hist(b) == 0 */
__global__ __launch_bounds__(kBlock) void k_scv_map(int nb, const int *active, const double *part, int nblk, double *map) {
	const int t = blockIdx.x;
	if (active && !active[t]) return;
	for (int b = threadIdx.x; b < nb; b += kBlock) {
		const double *col = part + (size_t)t * nblk * 2 * nb + b;
		double ss = 0.0, ww = 0.0;
		for (int k = 0; k < nblk; ++k) { ss += col[(size_t)k * 2 * nb]; ww += col[(size_t)k * 2 * nb + nb]; }
		map[(size_t)t * nb + b] = ww == 0 ? (double)b : ss / ww;
	}
}

/* utils::mapPixVals<Nearest / Linear> (imgUtils.h:682-703): I0 = map(I0_orig) */
__global__ __launch_bounds__(kBlock) void k_scv_remap(int N, int nb, int linear, const int *active, const double *map, const unsigned short *code,
	const double *i0o, double *I0) {
	__shared__ double s_map[kImapMaxBins];
	const int t = blockIdx.y;
	if (active && !active[t]) return;
	for (int b = threadIdx.x; b < nb; b += kBlock) s_map[b] = map[(size_t)t * nb + b];
	__syncthreads();
	const unsigned short *c = code + (size_t)t * N;
	const double *x = i0o + (size_t)t * N;
	double *out = I0 + (size_t)t * N;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
		if (linear) {
			const double v = x[i];
			const int lx = imap_bin((int)v, nb);
			const double dx = v - (int)v;
			const int ux = lx + 1 < nb ? lx + 1 : nb - 1;
			out[i] = dx == 0 ? s_map[lx] : (1 - dx) * s_map[lx] + dx * s_map[ux];
		} else {
			out[i] = s_map[c[i] >> 8];
		}
	}
}

template <int SSM, int KIND>
__global__ __launch_bounds__(kBlock) void k_rscv_hist(BatchView bv, ImgView im, ImapArgs a, int nblk) {
	__shared__ unsigned s_sum[kImapMaxBins], s_cnt[kImapMaxBins];
	__shared__ int s_last;
	const int t = blockIdx.y;
	if (a.active && !a.active[t]) return;   /* (uniform over the target's workgroups: nobody counts itself in) */
	const int N = bv.N, nb = a.nb;
	const unsigned char *code = a.code8 + (size_t)t * N;
	for (int b = threadIdx.x; b < kImapMaxBins; b += kBlock) { s_sum[b] = 0u; s_cnt[b] = 0u; }
	__syncthreads();
	imap_walk<SSM, KIND>(bv, im, a, t, nblk, [&](int i, auto it) {
		if (i >= N) return;
		/* getDiracJointHist (histUtils.cc:370-394): joint((int)It_orig, (int)I0) += 1, curr_hist((int)It_orig) += 1 */
		const int bt = imap_bin((int)it(), nb);
		atomicAdd(&s_sum[bt], (unsigned)code[i]);
		atomicAdd(&s_cnt[bt], 1u);
	});
	__syncthreads();
	unsigned *part = a.part_u + (size_t)t * nblk * 2 * nb;
	unsigned *row = part + (size_t)blockIdx.x * 2 * nb;
	for (int b = threadIdx.x; b < nb; b += kBlock) { st_coh(row + b, s_sum[b]); st_coh(row + nb + b, s_cnt[b]); }
	/* the last workgroup of the target to arrive builds the map (kernels_step.hip's hand-over: write-through rows, acknowledged, then an
	 * agent-scope arrival) */
	wait_stores_acked();
	__syncthreads();
	if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(a.arrive + t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nblk - 1u;
	__syncthreads();
	if (!s_last) return;
	if (threadIdx.x == 0) st_coh(a.arrive + t, 0u);
	/* RSCV::updatePixVals RSCV.cc:211-229: intensity_map(b) = sum_j j joint(b, j) / curr_hist(b), or b where curr_hist(b) == 0 */
	for (int b = threadIdx.x; b < nb; b += kBlock) {
		unsigned long long s = 0, c = 0;
		for (int k0 = 0; k0 < nblk; k0 += 8) {
			unsigned vs[8], vc[8];
#pragma unroll
			for (int j = 0; j < 8; ++j) {
				const bool in = k0 + j < nblk;
				const unsigned *r = part + (size_t)(in ? k0 + j : 0) * 2 * nb;
				vs[j] = in ? ld_coh(r + b) : 0u;
				vc[j] = in ? ld_coh(r + nb + b) : 0u;
			}
#pragma unroll
			for (int j = 0; j < 8; ++j) { s += vs[j]; c += vc[j]; }
		}
		a.map[(size_t)t * nb + b] = c == 0 ? (double)b : (double)s / (double)c;
	}
}

/* utils::mapPixVals<Nearest / Linear> (imgUtils.h:696-703): It = map(It_orig) */
__global__ __launch_bounds__(kBlock) void k_rscv_apply(int N, int nb, int linear, const double *map, const double *ito, double *It) {
	__shared__ double s_map[kImapMaxBins];
	const int t = blockIdx.y;
	for (int b = threadIdx.x; b < nb; b += kBlock) s_map[b] = map[(size_t)t * nb + b];
	__syncthreads();
	const double *x = ito + (size_t)t * N;
	double *out = It + (size_t)t * N;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) out[i] = rscv_map_val(s_map, nb, linear, x[i]);
}

/* the localized pass 1; REV: LRSCV (the table is keyed by the current bin and sums (int)I0), else LSCV (keyed by the template's bin, sums
 * (int)It) */
template <int SSM, int KIND, bool REV>
__device__ __forceinline__ void localized_hist(const BatchView &bv, const ImgView &im, const ImapArgs &a, int nblk, unsigned *s_tab, int &s_last) {
	const int t = blockIdx.y;
	if (a.active && !a.active[t]) return;   /* (uniform over the target's workgroups: nobody counts itself in) */
	const int N = bv.N, nb = a.nb, E = a.ncell * nb;
	unsigned *s_sum = s_tab, *s_cnt = s_tab + E;
	for (int e = threadIdx.x; e < 2 * E; e += kBlock) s_tab[e] = 0u;
	__syncthreads();
	/* getDiracJointHist over a sub-region (histUtils.cc:396-419): LSCV.cc:272-275 joint((int)It, (int)I0_orig) += 1, init_hist((int)I0_orig) += 1;
	 * LRSCV.cc:240-243 with the current patch first, joint((int)It, (int)I0) += 1, curr_hist((int)It) += 1 */
	imap_walk<SSM, KIND>(bv, im, a, t, nblk, [&](int i, auto it) {
		if (i >= N) return;
		if constexpr (REV) {
			/* (the fast kinds' interior test is per wave, so every lane samples, whether or not its pixel lies in a sub-region) */
			const int bt = imap_bin((int)it(), nb);
			const unsigned cl = a.cell[i];
			if (cl == 0xffffu) return;   /* (in no sub-region: no histogram counts it) */
			const int e = (int)cl * nb + bt;
			atomicAdd(&s_sum[e], (unsigned)a.code8[(size_t)t * N + i]);
			atomicAdd(&s_cnt[e], 1u);
		} else {
			const unsigned cl = a.cell[i];
			if (cl == 0xffffu) return;   /* (... and replay has no wave-wide step: it is not sampled either) */
			const int e = (int)cl * nb + (a.code16[(size_t)t * N + i] & 0xff);
			atomicAdd(&s_sum[e], (unsigned)imap_bin((int)it(), nb));
			atomicAdd(&s_cnt[e], 1u);
		}
	});
	__syncthreads();
	lscv_hand_over(a, t, nblk, s_tab, s_last);
}
template <int SSM, int KIND>
__global__ __launch_bounds__(kBlock) void k_lscv_hist(BatchView bv, ImgView im, ImapArgs a, int nblk) {
	extern __shared__ unsigned s_tab[];   /* [2][ncell nb]: the sums of (int)It, then the counts, keyed by (cell, template bin) */
	__shared__ int s_last;
	localized_hist<SSM, KIND, false>(bv, im, a, nblk, s_tab, s_last);
}
template <int SSM, int KIND>
__global__ __launch_bounds__(kBlock) void k_lrscv_hist(BatchView bv, ImgView im, ImapArgs a, int nblk) {
	extern __shared__ unsigned s_tab[];   /* [2][ncell nb]: the sums of (int)I0, then the counts, keyed by (cell, current bin) */
	__shared__ int s_last;
	localized_hist<SSM, KIND, true>(bv, im, a, nblk, s_tab, s_last);
}

/* LSCV.cc:286-300: I0_mapped through sub-region r's map (affine, utils::mapPixVals<Linear / Nearest>, imgUtils.h:682-703), then
 * I0 += I0_mapped * sub_region_wts(pix, r) for idx outer, idy inner */
__global__ __launch_bounds__(kBlock) void k_lscv_remap(int N, ImapArgs a, double *I0) {
	extern __shared__ double s_map[];   /* affine: [R][2] (a_r, c_r); else [R][nb] */
	const int t = blockIdx.y;
	if (a.active && !a.active[t]) return;
	const int nb = a.nb, nx = a.nx, ny = a.ny, R = nx * ny;
	const int M = a.affine ? 2 * R : R * nb;
	const double *src = a.affine ? a.aff + (size_t)t * 2 * R : a.map + (size_t)t * R * nb;
	for (int e = threadIdx.x; e < M; e += kBlock) s_map[e] = src[e];
	__syncthreads();
	const unsigned short *c = a.code16 + (size_t)t * N;
	const double *x = a.i0o + (size_t)t * N;
	double *out = I0 + (size_t)t * N;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
		double v = 0.0, dx = 0.0;
		int lx = 0, ux = 0, nr = 0;
		if (a.affine || a.linear) {
			v = x[i];
			dx = v - (int)v;
			lx = imap_bin((int)v, nb);
			ux = lx + 1 < nb ? lx + 1 : nb - 1;
		} else {
			nr = c[i] >> 8;
		}
		double acc = 0.0;
		for (int idx = 0; idx < nx; ++idx)
			for (int idy = 0; idy < ny; ++idy) {
				const int r = idy * nx + idx;
				double m;
				if (a.affine) {
					m = s_map[2 * r] * v + s_map[2 * r + 1];
				} else if (a.linear) {
					const double *mr = s_map + r * nb;
					m = dx == 0 ? mr[lx] : (1 - dx) * mr[lx] + dx * mr[ux];
				} else {
					m = s_map[r * nb + nr];
				}
				acc += m * a.wts[(size_t)r * N + i];
			}
		out[i] = acc;
	}
}

/* LRSCV.cc:249-254: It = the blend of It_orig's images through the sub-region maps */
__global__ __launch_bounds__(kBlock) void k_lrscv_apply(int N, LrscvMap lm, const double *ito, double *It) {
	extern __shared__ double s_map[];   /* affine: [R][2] (a_r, c_r); else [R][nb] */
	const int t = blockIdx.y;
	const int M = lm.affine ? 2 * lm.R : lm.R * lm.nb;
	for (int e = threadIdx.x; e < M; e += kBlock) s_map[e] = lm.map[(size_t)t * M + e];
	__syncthreads();
	const double *x = ito + (size_t)t * N;
	double *out = It + (size_t)t * N;
	for (int i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) out[i] = lrscv_blend(s_map, lm, lm.wts + i, (unsigned)N, x[i]);
}

/* the kinds a model's pass 1 is instantiated for: SCV and LSCV run in front of an SSD pass (replay, or the buffer); the reversed models in
 * front of every fused form */
template <int... KINDS> struct ImapKinds {};
using ImapKindsSsd = ImapKinds<RSCV_IT_REPLAY, RSCV_IT_FROM_BUF>;
using ImapKindsAll = ImapKinds<RSCV_IT_REPLAY, RSCV_IT_FAST_ICLK, RSCV_IT_FAST_CHAINED, RSCV_IT_FAST_QSTEP, RSCV_IT_FROM_BUF>;
/* calls f(SSM, KIND) -- std::integral_constant tags -- for the pass-1 instantiation of (ssm, kind) */
template <int... KINDS, class F>
static void imap_visit(ImapKinds<KINDS...>, int ssm, int kind, F &&f) {
	auto with_ssm = [&](auto K) {
		if (ssm == MTFHIP_SSM_HOMOGRAPHY) f(std::integral_constant<int, MTFHIP_SSM_HOMOGRAPHY>{}, K);
		else f(std::integral_constant<int, MTFHIP_SSM_AFFINE>{}, K);
		return true;
	};
	if (!((kind == KINDS && with_ssm(std::integral_constant<int, KINDS>{})) || ...))
		note_launch_error(hipErrorInvalidDeviceFunction, __FILE__, __LINE__);   /* (no kernel for this launch: an error, not a skipped pass) */
}

void launch_scv_codes(int N, int B, int nb, const double *i0o, unsigned short *code, hipStream_t st) {
	MTFHIP_LAUNCH(k_scv_codes, grid2(simple_blocks_per_target(N), B), dim3(kBlock), 0, st, N, nb, i0o, code);
}
void launch_rscv_codes(int N, int B, int nb, const double *i0, unsigned char *code, hipStream_t st) {
	MTFHIP_LAUNCH(k_rscv_codes, grid2(simple_blocks_per_target(N), B), dim3(kBlock), 0, st, N, nb, i0, code);
}
void launch_scv_update(const BatchView &bv, const ImgView &im, const ImapArgs &a, double *I0, hipStream_t st) {
	const int nblk = imap_hist_blocks(bv.N, kImapChunks);
	imap_visit(ImapKindsSsd{}, bv.ssm, a.kind, [&](auto SSM, auto KIND) {
		MTFHIP_LAUNCH((k_scv_hist<SSM(), KIND()>), grid2(nblk, bv.B), dim3(kBlock), 0, st, bv, im, a, nblk);
	});
	MTFHIP_LAUNCH(k_scv_map, dim3(bv.B), dim3(kBlock), 0, st, a.nb, a.active, (const double *)a.part_f, nblk, a.map);
	MTFHIP_LAUNCH(k_scv_remap, grid2(simple_blocks_per_target(bv.N), bv.B), dim3(kBlock), 0, st, bv.N, a.nb, a.linear, a.active, (const double *)a.map,
		a.code16, a.i0o, I0);
}
void launch_rscv_hist(const BatchView &bv, const ImgView &im, const ImapArgs &a, hipStream_t st) {
	const int nblk = imap_hist_blocks(bv.N, kImapChunks);
	imap_visit(ImapKindsAll{}, bv.ssm, a.kind, [&](auto SSM, auto KIND) {
		MTFHIP_LAUNCH((k_rscv_hist<SSM(), KIND()>), grid2(nblk, bv.B), dim3(kBlock), 0, st, bv, im, a, nblk);
	});
}
void launch_rscv_apply(int N, int B, int nb, int linear, const double *map, const double *it_orig, double *It, hipStream_t st) {
	MTFHIP_LAUNCH(k_rscv_apply, grid2(simple_blocks_per_target(N), B), dim3(kBlock), 0, st, N, nb, linear, map, it_orig, It);
}
void launch_lscv_update(const BatchView &bv, const ImgView &im, const ImapArgs &a, double *I0, hipStream_t st) {
	const int nblk = imap_hist_blocks(bv.N, kImapChunksLocal);
	const size_t lds_hist = sizeof(unsigned) * 2 * (size_t)a.ncell * a.nb;
	imap_visit(ImapKindsSsd{}, bv.ssm, a.kind, [&](auto SSM, auto KIND) {
		MTFHIP_LAUNCH((k_lscv_hist<SSM(), KIND()>), grid2(nblk, bv.B), dim3(kBlock), lds_hist, st, bv, im, a, nblk);
	});
	const size_t lds_map = sizeof(double) * (a.affine ? 2 * (size_t)a.nx * a.ny : (size_t)a.nx * a.ny * a.nb);
	MTFHIP_LAUNCH(k_lscv_remap, grid2(simple_blocks_per_target(bv.N), bv.B), dim3(kBlock), lds_map, st, bv.N, a, I0);
}
void launch_lrscv_hist(const BatchView &bv, const ImgView &im, const ImapArgs &a, hipStream_t st) {
	const int nblk = imap_hist_blocks(bv.N, kImapChunksLocal);
	const size_t lds = sizeof(unsigned) * 2 * (size_t)a.ncell * a.nb;
	imap_visit(ImapKindsAll{}, bv.ssm, a.kind, [&](auto SSM, auto KIND) {
		MTFHIP_LAUNCH((k_lrscv_hist<SSM(), KIND()>), grid2(nblk, bv.B), dim3(kBlock), lds, st, bv, im, a, nblk);
	});
}
void launch_lrscv_apply(int N, int B, const LrscvMap &lm, const double *it_orig, double *It, hipStream_t st) {
	const size_t lds = sizeof(double) * (size_t)(lm.affine ? 2 * lm.R : lm.R * lm.nb);
	MTFHIP_LAUNCH(k_lrscv_apply, grid2(simple_blocks_per_target(N), B), dim3(kBlock), lds, st, N, lm, it_orig, It);
}

} // namespace mtfhip
