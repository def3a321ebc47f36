/*
 * kernels_alk.hip -- the additive Lucas-Kanade search methods on the device: nt::FALK (SM/src/NT/FALK.cc) and nt::IALK
 * (SM/src/NT/IALK.cc).  One iteration is two launches for every target of the batch: k_alk_pass (the pixel pass) and k_alk_finish
 * (row sums, Hessian choice, Levenberg-Marquardt, solve, StateSpaceModel::additiveUpdate, convergence test).
 * (one of the translation units of libmtfhip.so; conventions and the shared device helpers: mtfhip_device.h)
 */
#include "mtfhip_finish_device.h"

namespace mtfhip {

/* The pixel pass of one FALK / IALK iteration in replay arithmetic: every per-pixel expression is the one the per-function kernels
 * evaluate (k_apply_warp, k_sample, k_img_grad, k_pix_jacobian: kernels_interface.hip), in the reference's operation order, so what
 * MAT stores is bit-identical to the per-function route.
 *   both : curr_pt = W(p) init_pt (ProjectiveBase.cc:41-49), It = getPixVal<Linear, Constant>(curr_pt) (border value 128)
 *   FALK : dIt_dx = the finite-difference gradient at the CURRENT point (ImageBase.cc:292 -> imgUtils.cc:233-254), row = cmptPixJacobian
 *          (Homography.cc:193-229; Affine.h:35-37: cmptInitPixJacobian)
 *   IALK : row = cmptApproxPixJacobian of the STORED dI0_dx (Homography.cc:296-358, Affine.cc:184-211); no gradient is sampled
 * Sums (the fused kernel's FCLK-type row, so the host's and the finish's assembly of g and H serve unchanged):
 *   SSD  : ACC_H += row (x) row, ACC_G += -(It - I0) row, ACC_RR += (It - I0)^2
 *   NCC  : NCC_GRAM += row (x) row, NCC_SJ += row, NCC_ITJ += It row, NCC_I0J += I0 row, NCC_IT / _IT2 / _I0IT
 * Fixed order: a thread walks its pixels in increasing order, the workgroup reduces with the halving butterfly (block_reduce_store) and
 * writes one partial row; no floating-point atomics.  A workgroup serves rows_per_block 256-pixel rows of one target
 * (fused_decomposition); the only branch in front of the reduction's barrier is the target's live flag, uniform over the workgroup. */
template <int SSM, int AM, bool IALK, bool MAT>
__global__ __launch_bounds__(kBlock) void k_alk_pass(BatchView bv, ImgView im, AlkArgs a, double *partials, int nblk) {
	constexpr int S = (SSM == MTFHIP_SSM_HOMOGRAPHY) ? 8 : 6;
	constexpr bool NCC = AM == MTFHIP_AM_NCC;
	constexpr int K = NCC ? NCC_ACC_COUNT : 48;
	constexpr int ROW_LEN = NCC ? NCC_ACC_COUNT : ACC_COUNT;
	__shared__ double lds[4 * K];
	const int t = blockIdx.y;
	if (a.active && a.active[t] == 0) return;
	const unsigned N = (unsigned)bv.N;
	const Warp9 W = load_warp(bv.warps + 9 * t);
	const double *st = bv.states + 8 * t;
	const double2 *__restrict__ ip = reinterpret_cast<const double2 *>(bv.buf[MTFHIP_BUF_INIT_PTS]) + (size_t)t * N;
	const double *__restrict__ iz = bv.buf[MTFHIP_BUF_INIT_Z] + (size_t)t * N;
	const double2 *__restrict__ ih = reinterpret_cast<const double2 *>(bv.buf[MTFHIP_BUF_INIT_HXY]) + (size_t)t * N;
	const double *__restrict__ I0 = bv.buf[MTFHIP_BUF_I0] + (size_t)t * N;
	const double *__restrict__ dI0 = bv.buf[MTFHIP_BUF_DI0_DX] + (size_t)t * N * 2;
	double *__restrict__ It = bv.buf[MTFHIP_BUF_IT] + (size_t)t * N;
	double *__restrict__ dIt = bv.buf[MTFHIP_BUF_DIT_DX] + (size_t)t * N * 2;
	double *__restrict__ Jt = bv.buf[MTFHIP_BUF_JT] + (size_t)t * N * S;
	const bool unit_z = bv.unit_z != 0;
	const double eps = a.grad_eps;
	const double gmult = a.norm_mult / (2 * eps);
	/* Affine.cc:186-187 */
	const double aa = st[2] + 1, ab = st[3], ac = st[4], ad = st[5] + 1;

	double acc[K];
#pragma unroll
	for (int k = 0; k < K; ++k) acc[k] = 0.0;

	const unsigned base = blockIdx.x * (unsigned)(kBlock * a.rows_per_block) + threadIdx.x;
	for (int rr = 0; rr < a.rows_per_block; ++rr) {
		const unsigned i = base + (unsigned)rr * kBlock;
		if (i >= N) break;
		const double2 p0 = ip[i];
		const double x = p0.x, y = p0.y;
		const double2 hp = unit_z ? p0 : ih[i];
		const double z = unit_z ? 1.0 : iz[i];
		double wx, wy, D = 1.0;
		if constexpr (SSM == MTFHIP_SSM_HOMOGRAPHY) {
			const double cx = W.m[0] * hp.x + W.m[1] * hp.y + W.m[2] * z;
			const double cy = W.m[3] * hp.x + W.m[4] * hp.y + W.m[5] * z;
			D = W.m[6] * hp.x + W.m[7] * hp.y + W.m[8] * z;
			wx = cx / D; wy = cy / D;
		} else {
			wx = W.m[0] * hp.x + W.m[1] * hp.y + W.m[2] * z;
			wy = W.m[3] * hp.x + W.m[4] * hp.y + W.m[5] * z;
		}
		const Cell c = load_cell(im, wx, wy);
		const double it = a.norm_mult * pix_val_cell(im, c, wx, wy) + a.norm_add;
		const double i0 = I0[i];
		double gx, gy;
		if constexpr (IALK) {
			gx = dI0[i]; gy = dI0[N + i];
		} else {
			double inc = pix_val_cell(im, c, wx + eps, wy);
			double dec = pix_val_cell(im, c, wx - eps, wy);
			gx = (inc - dec) * gmult;
			inc = pix_val_cell(im, c, wx, wy + eps);
			dec = pix_val_cell(im, c, wx, wy - eps);
			gy = (inc - dec) * gmult;
		}
		double row[S];
		if constexpr (SSM == MTFHIP_SSM_HOMOGRAPHY) {
			if constexpr (IALK) {
				const double a_ = (W.m[0] - W.m[6] * wx), b_ = (W.m[1] - W.m[7] * wx);
				const double c_ = (W.m[3] - W.m[6] * wy), d_ = (W.m[4] - W.m[7] * wy);
				const double inv_factor = 1.0 / (a_ * d_ - b_ * c_);
				const double Ix = (d_ * gx - c_ * gy) * inv_factor;
				const double Iy = (a_ * gy - b_ * gx) * inv_factor;
				hom_row(row, Ix, Iy, x, y, wx, wy);
			} else {
				const double inv_d = 1.0 / D;
				hom_row(row, gx * inv_d, gy * inv_d, x, y, wx, wy);
			}
		} else {
			const double Ixx = gx * x, Ixy = gx * y, Iyy = gy * y, Iyx = gy * x;
			if constexpr (IALK) {
				const double inv_det = 1.0 / (aa * ad - ab * ac);
				row[0] = (gx * ad - gy * ac) * inv_det; row[1] = (gy * aa - gx * ab) * inv_det;
				row[2] = (Ixx * ad - Iyx * ac) * inv_det; row[3] = (Ixy * ad - Iyy * ac) * inv_det;
				row[4] = (Iyx * aa - Ixx * ab) * inv_det; row[5] = (Iyy * aa - Ixy * ab) * inv_det;
			} else {
				row[0] = gx; row[1] = gy; row[2] = Ixx; row[3] = Ixy; row[4] = Iyx; row[5] = Iyy;
			}
		}
		if constexpr (MAT) {
			MAT_STORE(&It[i], it);
			if constexpr (!IALK) { MAT_STORE(&dIt[i], gx); MAT_STORE(&dIt[N + i], gy); }
#pragma unroll
			for (int s = 0; s < S; ++s) MAT_STORE(&Jt[(size_t)s * N + i], row[s]);
		}
		if constexpr (NCC) {
			acc[NCC_IT] += it; acc[NCC_IT2] = fma(it, it, acc[NCC_IT2]); acc[NCC_I0IT] = fma(i0, it, acc[NCC_I0IT]);
#pragma unroll
			for (int s = 0; s < S; ++s) {
				acc[NCC_SJ + s] += row[s];
				acc[NCC_ITJ + s] = fma(it, row[s], acc[NCC_ITJ + s]);
				acc[NCC_I0J + s] = fma(i0, row[s], acc[NCC_I0J + s]);
			}
		} else {
			const double r = it - i0;
			acc[ACC_RR] = fma(r, r, acc[ACC_RR]);
#pragma unroll
			for (int s = 0; s < S; ++s) acc[ACC_G + s] = fma(-r, row[s], acc[ACC_G + s]);
		}
#pragma unroll
		for (int p = 0; p < S; ++p)
#pragma unroll
			for (int q = p; q < S; ++q) {
				constexpr int H0 = NCC ? (int)NCC_GRAM : (int)ACC_H;
				const int k = H0 + p * 8 - (p * (p - 1)) / 2 + (q - p);
				acc[k] = fma(row[p], row[q], acc[k]);
			}
	}
	block_reduce_store<K>(acc, partials + ((size_t)t * nblk + blockIdx.x) * ROW_LEN, lds);
}

/* one workgroup per target: finish_track_body's additive form (mtfhip_finish_device.h).  `sm` arrives with sm.sm = MTFHIP_SM_FCLK: the
 * row is FCLK-type and hess_type keeps FCLK's numbering (FALKParams.h:9, IALKParams.h:9). */
__global__ __launch_bounds__(256) void k_alk_finish(BatchView bv, mtfhip_sm_desc sm, TrackState ts, const double *partials, int nblk) {
	finish_track_body<false, true>(bv, sm, ts, partials, nblk, blockIdx.x);
}

/* ===================================================================== */
/* launchers                                                              */
/* ===================================================================== */
template <int SSM, int AM>
static void launch_alk_pass_t(const BatchView &bv, const ImgView &im, const AlkArgs &a, double *partials, int nblk, hipStream_t st) {
	const dim3 g = grid2(nblk, bv.B);
	if (a.ialk) {
		if (a.materialize) MTFHIP_LAUNCH((k_alk_pass<SSM, AM, true, true>), g, dim3(kBlock), 0, st, bv, im, a, partials, nblk);
		else MTFHIP_LAUNCH((k_alk_pass<SSM, AM, true, false>), g, dim3(kBlock), 0, st, bv, im, a, partials, nblk);
	} else {
		if (a.materialize) MTFHIP_LAUNCH((k_alk_pass<SSM, AM, false, true>), g, dim3(kBlock), 0, st, bv, im, a, partials, nblk);
		else MTFHIP_LAUNCH((k_alk_pass<SSM, AM, false, false>), g, dim3(kBlock), 0, st, bv, im, a, partials, nblk);
	}
}
void launch_alk_pass(const BatchView &bv, const ImgView &im, const AlkArgs &a, double *partials, int nblk, hipStream_t st) {
	const bool hom = bv.ssm == MTFHIP_SSM_HOMOGRAPHY;
	if (bv.C != 1 || (bv.am != MTFHIP_AM_SSD && bv.am != MTFHIP_AM_NCC)) {   /* (no kernel for this launch: an error, not a skipped pass) */
		note_launch_error(hipErrorInvalidDeviceFunction, __FILE__, __LINE__);
		return;
	}
	if (bv.am == MTFHIP_AM_NCC) {
		if (hom) launch_alk_pass_t<MTFHIP_SSM_HOMOGRAPHY, MTFHIP_AM_NCC>(bv, im, a, partials, nblk, st);
		else launch_alk_pass_t<MTFHIP_SSM_AFFINE, MTFHIP_AM_NCC>(bv, im, a, partials, nblk, st);
	} else {
		if (hom) launch_alk_pass_t<MTFHIP_SSM_HOMOGRAPHY, MTFHIP_AM_SSD>(bv, im, a, partials, nblk, st);
		else launch_alk_pass_t<MTFHIP_SSM_AFFINE, MTFHIP_AM_SSD>(bv, im, a, partials, nblk, st);
	}
}
void launch_alk_finish(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts, const double *partials, int nblk, hipStream_t st) {
	/* (the workgroup sizes of launch_finish_track: NCC rows are 72 wide, many block rows are summed by 240 lanes) */
	MTFHIP_LAUNCH(k_alk_finish, dim3(bv.B), dim3(nblk > 8 ? 256 : (bv.am == MTFHIP_AM_NCC ? 128 : 64)), 0, st, bv, sm, ts, partials, nblk);
}

} // namespace mtfhip
