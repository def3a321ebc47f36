/*
 * kernels_flow.hip -- k_ncc_flow: NCC::estimateOpticalFlow (AM/src/NCC.cc:412-526), the translation-only NCC Gauss-Newton flow that
 * nt::GridTrackerFlow runs on its grid points (SM/src/NT/GridTrackerFlow.cc:88-91), a point's whole flow in ONE launch: the template from
 * the previous image, then up to max_iters passes on the current one, no host round trip and no per-pixel global traffic beside the texels.
 *
 * Decomposition: one point per workgroup of kBlock threads, PPT = ceil(N / kBlock) samples per thread (N = win_w win_h <= 1024, PPT 1 .. 4).
 * Sample i = threadIdx.x + k kBlock is lattice entry (i / win_w, i % win_w): y outer, x inner, as sc::getPixVals walks it
 * (imgUtils.h:319-334).  A thread keeps, per sample, the two lattice coordinates (the reference adds every pass's step to every element of
 * win_x / win_y in double, NCC.cc:518-519: the sum of the rounded additions cannot be rebuilt from the index, so it is carried), the centred
 * template value and -- under const_grad -- the two gradient components.  Like k_iclk_track this is a chain of dependent latencies per point,
 * not a bandwidth problem: the passes of one point cannot overlap, the points of a launch do.
 *
 * MTFHIP_MATH_REPLAY walks the reference's passes in its operation order (mean | centred sums | mean of df | gradient sums; four workgroup
 * reductions per pass), samples with pix_val's expressions (five samples per pixel, the 1e-8 central difference) and solves the 2 x 2 system
 * with the column-pivoted Householder QR the project's checker restates; only the order of the N-wide sums differs from a serial loop.
 * MTFHIP_MATH_FAST forms every quantity of a pass from twelve raw sums in ONE workgroup reduction (ncc_flow_assemble below), takes the
 * gradient from the closed-form derivative of the bilinear cell, and solves the system in closed form in every thread.
 */
#include "mtfhip_grid_device.h"
#include "mtfhip_flow.h"

namespace mtfhip {

__device__ __forceinline__ bool finite_d(double v) { return __builtin_isfinite(v); }

/* x = A^-1 b, A 2 x 2 column-major: the column-pivoted Householder QR standing in for colPivHouseholderQr().solve (NCC.cc:515), written
 * out for n = 2 step by step as the checker's restatement (mtfo_colpiv_qr_solve) and tests/helpers/flow_ref.py do it.  A rank-deficient
 * system gives the basic solution (zero for the zero matrix), as Eigen's solve does. */
__device__ __forceinline__ void colpiv_qr_solve2(double a00, double a10, double a01, double a11, double b0, double b1, double &x0, double &x1) {
	double p0 = a00, p1 = a10, q0 = a01, q1 = a11;   /* column k = (p), the other (q) */
	const double cn0 = a00 * a00 + a10 * a10, cn1 = a01 * a01 + a11 * a11;
	double max_norm0 = 0;
	if (max_norm0 < cn0) max_norm0 = cn0;
	if (max_norm0 < cn1) max_norm0 = cn1;
	/* k = 0 */
	double best = -1; bool swapped = false;
	if (cn0 > best) best = cn0;
	if (cn1 > best) { best = cn1; swapped = true; }
	x0 = 0; x1 = 0;
	if (best <= max_norm0 * 1e-300 || best == 0) return;   /* rank 0 */
	if (swapped) { p0 = a01; p1 = a11; q0 = a00; q1 = a10; }
	double r0 = b0, r1 = b1;
	{
		const double norm = sqrt(best), alpha = p0 > 0 ? -norm : norm;
		const double v0 = p0 - alpha, v1 = p1, vnorm2 = v0 * v0 + v1 * v1;
		if (vnorm2 > 0) {
			double f = 2 * (v0 * p0 + v1 * p1) / vnorm2;
			p0 -= f * v0; p1 -= f * v1;
			f = 2 * (v0 * q0 + v1 * q1) / vnorm2;
			q0 -= f * v0; q1 -= f * v1;
			f = 2 * (v0 * r0 + v1 * r1) / vnorm2;
			r0 -= f * v0; r1 -= f * v1;
		}
	}
	/* k = 1 */
	best = q1 * q1;
	const bool full = !(best <= max_norm0 * 1e-300 || best == 0);
	if (full) {
		const double norm = sqrt(best), alpha = q1 > 0 ? -norm : norm;
		const double v1 = q1 - alpha, vnorm2 = v1 * v1;
		if (vnorm2 > 0) {
			double f = 2 * (v1 * q1) / vnorm2;
			q1 -= f * v1;
			f = 2 * (v1 * r1) / vnorm2;
			r1 -= f * v1;
		}
	}
	const double y1 = full ? r1 / q1 : 0.0;
	const double y0 = (full ? r0 - q0 * y1 : r0) / p0;
	if (swapped) { x1 = y0; x0 = y1; } else { x0 = y0; x1 = y1; }
}

/* sc::getPixValsWithGrad for one lattice entry (imgUtils.h:337-366): the value and the central differences at x +- eps, y +- eps, each of
 * the five samples with getPixVal's expression (the cell's texels are fetched once: pix_val_cell) */
__device__ __forceinline__ void flow_sample_replay(const ImgView &im, double x, double y, bool grad, double eps, double gmult, double &v, double &gx,
	double &gy) {
	if (!grad) { v = pix_val(im, x, y); return; }
	const Cell c = load_cell(im, x, y);
	v = pix_val_cell(im, c, x, y);
	double inc = pix_val_cell(im, c, x + eps, y);
	double dec = pix_val_cell(im, c, x - eps, y);
	gx = (inc - dec) * gmult;
	inc = pix_val_cell(im, c, x, y + eps);
	dec = pix_val_cell(im, c, x, y - eps);
	gy = (inc - dec) * gmult;
}
/* Tolerance mode.  All five samples inside one interior cell (the common case): the value and the closed-form slopes of the cell
 * (bilin_fast), the slopes times the step the reference's difference really takes (fd_step).  Otherwise -- an integer coordinate, where
 * x - eps lies in the cell to the left and the difference straddles the texel edge, a coordinate within eps of an edge, the border, a
 * window off the frame -- the reference's five samples.  A coordinate is converted to an integer only after the range test has passed. */
__device__ __forceinline__ void flow_sample_fast(const ImgView &im, double x, double y, bool grad, double eps, double gmult, double &v, double &gx,
	double &gy) {
	if (!grad) { v = pix_val_fast(im, x, y); return; }
	const double w = (double)im.w, h = (double)im.h;
	if (x >= 1.0 && y >= 1.0 && x < w - 2.0 && y < h - 2.0) {
		const int lx = (int)x, ly = (int)y;
		const double lxd = (double)lx, lyd = (double)ly;
		if (x - eps >= lxd && x + eps < lxd + 1.0 && y - eps >= lyd && y + eps < lyd + 1.0) {
			const float *r0 = im.data + (size_t)ly * im.stride, *r1 = r0 + im.stride;
			double bgx, bgy;
			bilin_fast(r0[lx], r0[lx + 1], r1[lx], r1[lx + 1], x - lxd, y - lyd, v, bgx, bgy);
			gx = bgx * (fd_step(x, eps) * gmult);
			gy = bgy * (fd_step(y, eps) * gmult);
			return;
		}
	}
	flow_sample_replay(im, x, y, true, eps, gmult, v, gx, gy);
}

/* The twelve raw sums of a tolerance-mode pass and what NCC.cc:475-515 makes of them.  With n samples, I0c the centred template, c = |I0c|,
 * G = (Gx, Gy) the image gradient, m = S_It / n:
 *   a   = sum I0c (It - m)            = S_I0cIt - m S_I0c            (S_I0c = sum I0c ~ 0, a constant of the point)
 *   b^2 = sum (It - m)^2              = S_ItIt - m S_It
 *   f   = a / (b c)
 *   df_i = (I0c_i / c - f (It_i - m) / b) / b,  mean(df) = S_I0c / (c b n)                      (sum (It - m) = 0)
 *   e_k = sum G_k (It - m)            = S_GkIt - m S_Gk
 *   df_dx_k = sum (df_i - mean(df)) G_ik = (S_GkI0c / c - f e_k / b) / b - mean(df) S_Gk
 *   Gc = (G - mean(G)) / b:  (Gc^T Gc)_kl = (S_GkGl - S_Gk S_Gl / n) / b^2,   (Gc^T Itc / b)_k = e_k / b^2   (sum (G_k - mean) = 0)
 *   d2f_dx2 = -Gc^T Gc + (Gc^T Itc / b)(Gc^T Itc / b)^T,   opt_flow = -d2f_dx2^-1 df_dx  (closed form, one reciprocal)
 * Slots: 0 S_It, 1 S_ItIt, 2 S_I0cIt, 3 S_Gx, 4 S_Gy, 5 S_GxGx, 6 S_GxGy, 7 S_GyGy, 8 S_GxIt, 9 S_GyIt, 10 S_GxI0c, 11 S_GyI0c. */
struct FlowPass { double fx, fy, f, g0, g1, h00, h01, h11; };
__device__ __forceinline__ FlowPass ncc_flow_assemble(const double *S, double S_I0c, double inv_c, double inv_n) {
	FlowPass r;
	const double m = S[0] * inv_n;
	const double b2 = fma(-S[0], m, S[1]);
	const double a = fma(-m, S_I0c, S[2]);
	const double ib = rsq_fast(b2), ib2 = ib * ib;
	r.f = a * ib * inv_c;
	const double dfm = S_I0c * inv_c * ib * inv_n;
	const double e0 = fma(-m, S[3], S[8]), e1 = fma(-m, S[4], S[9]);
	r.g0 = fma(-dfm, S[3], ib * fma(S[10], inv_c, -(r.f * ib) * e0));
	r.g1 = fma(-dfm, S[4], ib * fma(S[11], inv_c, -(r.f * ib) * e1));
	const double v0 = e0 * ib2, v1 = e1 * ib2;
	const double sxx = fma(-S[3] * inv_n, S[3], S[5]) * ib2, sxy = fma(-S[3] * inv_n, S[4], S[6]) * ib2, syy = fma(-S[4] * inv_n, S[4], S[7]) * ib2;
	r.h00 = fma(v0, v0, -sxx); r.h01 = fma(v0, v1, -sxy); r.h11 = fma(v1, v1, -syy);
	const double idet = rcp_fast(fma(r.h00, r.h11, -(r.h01 * r.h01)));
	r.fx = -fma(r.h11, r.g0, -(r.h01 * r.g1)) * idet;
	r.fy = -fma(r.h00, r.g1, -(r.h01 * r.g0)) * idet;
	return r;
}

template <int PPT, bool FAST>
__global__ __launch_bounds__(kBlock) void k_ncc_flow(FlowArgs a) {
	__shared__ double lds[2][48];
	const int p = blockIdx.x, tid = threadIdx.x;
	const int N = a.win_w * a.win_h;
	const double n_d = (double)N;
	const float px = a.prev_pts[2 * p], py = a.prev_pts[2 * p + 1];
	const double eps = a.grad_eps, gmult = 1.0 / (2 * eps);   /* grad_mult_factor :426 */
	if (!(__builtin_isfinite(px) && __builtin_isfinite(py))) {   /* (uniform) no lattice to sample */
		if (tid == 0) {
			const float nanf_ = __builtin_nanf("");
			a.curr_pts[2 * p] = nanf_; a.curr_pts[2 * p + 1] = nanf_; a.n_iters[p] = 0; a.status[p] = MTFHIP_FLOW_NONFINITE;
		}
		return;
	}
	/* the lattice :427-433 */
	double X[PPT], Y[PPT], I0c[PPT], Gx[PPT], Gy[PPT];
	bool ok[PPT];
	{
		const double half_w = a.win_w / 2.0, half_h = a.win_h / 2.0;
		const double lo_x = px - half_w, hi_x = px + half_w, lo_y = py - half_h, hi_y = py + half_h;
#pragma unroll
		for (int k = 0; k < PPT; ++k) {
			const int i = tid + k * kBlock;
			ok[k] = i < N;
			const int row = ok[k] ? i / a.win_w : 0, col = ok[k] ? i % a.win_w : 0;
			X[k] = lin_spaced_hd(col, a.win_w, lo_x, hi_x);
			Y[k] = lin_spaced_hd(row, a.win_h, lo_y, hi_y);
			I0c[k] = 0; Gx[k] = 0; Gy[k] = 0;
		}
	}
	const bool cg = a.const_grad != 0;
	float cx = px, cy = py;     /* curr_pts[pt_id] = prev_pts[pt_id] :464 */
	int n_it = a.max_iters, status = MTFHIP_FLOW_MAX_ITERS;
	double *tr = a.trace ? a.trace + (size_t)p * a.trace_cap * kFlowTraceStride : nullptr;

	if constexpr (!FAST) {
		/* ---- the template :444-462 ---- */
		double I0cc[PPT];
		double gmx = 0, gmy = 0, c;
		{
			double s[3] = {0, 0, 0};
#pragma unroll
			for (int k = 0; k < PPT; ++k)
				if (ok[k]) {
					flow_sample_replay(a.prev, X[k], Y[k], cg, eps, gmult, I0c[k], Gx[k], Gy[k]);
					s[0] += I0c[k];
					if (cg) { s[1] += Gx[k]; s[2] += Gy[k]; }
				}
			block_allsum<3>(s, &lds[0][0]);
			const double I0_mean = s[0] / n_d;
			if (cg) { gmx = s[1] / n_d; gmy = s[2] / n_d; }
			double c2[1] = {0};
#pragma unroll
			for (int k = 0; k < PPT; ++k)
				if (ok[k]) { I0c[k] = I0c[k] - I0_mean; c2[0] += I0c[k] * I0c[k]; }
			block_allsum<1>(c2, &lds[0][0]);
			c = sqrt(c2[0]);
#pragma unroll
			for (int k = 0; k < PPT; ++k) I0cc[k] = I0c[k] / c;
		}
		/* ---- the loop :465-521 ---- */
		for (int it = 0; it < a.max_iters; ++it) {
			double It[PPT], D[PPT];
			double s[3] = {0, 0, 0};
#pragma unroll
			for (int k = 0; k < PPT; ++k) {
				It[k] = 0; D[k] = 0;
				if (ok[k]) {
					flow_sample_replay(a.cur, X[k], Y[k], !cg, eps, gmult, It[k], Gx[k], Gy[k]);
					s[0] += It[k];
					if (!cg) { s[1] += Gx[k]; s[2] += Gy[k]; }
				}
			}
			block_allsum<3>(s, &lds[0][0]);
			const double It_mean = s[0] / n_d;
			if (!cg) { gmx = s[1] / n_d; gmy = s[2] / n_d; }
			double ab[2] = {0, 0};
#pragma unroll
			for (int k = 0; k < PPT; ++k)
				if (ok[k]) { It[k] = It[k] - It_mean; ab[0] += I0c[k] * It[k]; ab[1] += It[k] * It[k]; }
			block_allsum<2>(ab, &lds[0][0]);
			const double b = sqrt(ab[1]);
			const double f = ab[0] / (b * c);
			double dm[1] = {0};
#pragma unroll
			for (int k = 0; k < PPT; ++k)
				if (ok[k]) { It[k] = It[k] / b; D[k] = (I0cc[k] - f * It[k]) / b; dm[0] += D[k]; }
			block_allsum<1>(dm, &lds[0][0]);
			const double df_mean = dm[0] / n_d;
			double q[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
			for (int k = 0; k < PPT; ++k)
				if (ok[k]) {
					const double wgt = D[k] - df_mean;
					q[0] += wgt * Gx[k]; q[1] += wgt * Gy[k];
					const double gcx = (Gx[k] - gmx) / b, gcy = (Gy[k] - gmy) / b;
					q[2] += gcx * gcx; q[3] += gcx * gcy; q[4] += gcy * gcy;
					q[5] += gcx * It[k]; q[6] += gcy * It[k];
				}
			block_allsum<7>(q, &lds[0][0]);
			const double h00 = -q[2] + q[5] * q[5], h01 = -q[3] + q[5] * q[6], h11 = -q[4] + q[6] * q[6];
			double fx, fy;
			if (finite_d(h00) && finite_d(h01) && finite_d(h11) && finite_d(q[0]) && finite_d(q[1])) {
				colpiv_qr_solve2(h00, h01, h01, h11, q[0], q[1], fx, fy);
				fx = -fx; fy = -fy;
			} else fx = fy = __builtin_nan("");
			if (tr && tid == 0 && it < a.trace_cap) {
				double *t = tr + (size_t)it * kFlowTraceStride;
				t[0] = fx; t[1] = fy; t[2] = f; t[3] = q[0]; t[4] = q[1]; t[5] = h00; t[6] = h01; t[7] = h11;
			}
			if (!(finite_d(fx) && finite_d(fy))) { status = MTFHIP_FLOW_NONFINITE; n_it = it + 1; break; }
			cx += (float)fx; cy += (float)fy;                                     /* :516-517, float32 */
#pragma unroll
			for (int k = 0; k < PPT; ++k) { X[k] += fx; Y[k] += fy; }             /* :518-519, double, element by element */
			if (fx * fx + fy * fy < a.epsilon) { status = MTFHIP_FLOW_CONVERGED; n_it = it + 1; break; }
		}
	} else {
		const double inv_n = 1.0 / n_d;
		int par = 0;
		double K[12];   /* const_grad: the gradient-only sums and the two against I0c, constants of the loop */
		double S_I0c, inv_c;
		{
			double s[12];
#pragma unroll
			for (int j = 0; j < 12; ++j) s[j] = 0;
#pragma unroll
			for (int k = 0; k < PPT; ++k)
				if (ok[k]) {
					flow_sample_fast(a.prev, X[k], Y[k], cg, eps, gmult, I0c[k], Gx[k], Gy[k]);
					s[0] += I0c[k];
				}
			block_allsum_h12(s, &lds[par][0]); par ^= 1;
			const double I0_mean = s[0] * inv_n;
#pragma unroll
			for (int j = 0; j < 12; ++j) s[j] = 0;
#pragma unroll
			for (int k = 0; k < PPT; ++k)
				if (ok[k]) {
					I0c[k] -= I0_mean;
					s[0] += I0c[k]; s[1] = fma(I0c[k], I0c[k], s[1]);
					if (cg) {
						s[3] += Gx[k]; s[4] += Gy[k];
						s[5] = fma(Gx[k], Gx[k], s[5]); s[6] = fma(Gx[k], Gy[k], s[6]); s[7] = fma(Gy[k], Gy[k], s[7]);
						s[10] = fma(Gx[k], I0c[k], s[10]); s[11] = fma(Gy[k], I0c[k], s[11]);
					}
				}
			block_allsum_h12(s, &lds[par][0]); par ^= 1;
			S_I0c = s[0]; inv_c = rsq_fast(s[1]);
#pragma unroll
			for (int j = 0; j < 12; ++j) K[j] = s[j];
		}
		for (int it = 0; it < a.max_iters; ++it) {
			double s[12];
#pragma unroll
			for (int j = 0; j < 12; ++j) s[j] = 0;
#pragma unroll
			for (int k = 0; k < PPT; ++k)
				if (ok[k]) {
					double v;
					flow_sample_fast(a.cur, X[k], Y[k], !cg, eps, gmult, v, Gx[k], Gy[k]);
					s[0] += v; s[1] = fma(v, v, s[1]); s[2] = fma(I0c[k], v, s[2]);
					s[8] = fma(Gx[k], v, s[8]); s[9] = fma(Gy[k], v, s[9]);
					if (!cg) {
						s[3] += Gx[k]; s[4] += Gy[k];
						s[5] = fma(Gx[k], Gx[k], s[5]); s[6] = fma(Gx[k], Gy[k], s[6]); s[7] = fma(Gy[k], Gy[k], s[7]);
						s[10] = fma(Gx[k], I0c[k], s[10]); s[11] = fma(Gy[k], I0c[k], s[11]);
					}
				}
			block_allsum_h12(s, &lds[par][0]); par ^= 1;
			if (cg) { s[3] = K[3]; s[4] = K[4]; s[5] = K[5]; s[6] = K[6]; s[7] = K[7]; s[10] = K[10]; s[11] = K[11]; }
			const FlowPass r = ncc_flow_assemble(s, S_I0c, inv_c, inv_n);   /* every thread: no thread-0 section, no broadcast */
			if (tr && tid == 0 && it < a.trace_cap) {
				double *t = tr + (size_t)it * kFlowTraceStride;
				t[0] = r.fx; t[1] = r.fy; t[2] = r.f; t[3] = r.g0; t[4] = r.g1; t[5] = r.h00; t[6] = r.h01; t[7] = r.h11;
			}
			if (!(finite_d(r.fx) && finite_d(r.fy))) { status = MTFHIP_FLOW_NONFINITE; n_it = it + 1; break; }
			cx += (float)r.fx; cy += (float)r.fy;
#pragma unroll
			for (int k = 0; k < PPT; ++k) { X[k] += r.fx; Y[k] += r.fy; }
			if (fma(r.fx, r.fx, r.fy * r.fy) < a.epsilon) { status = MTFHIP_FLOW_CONVERGED; n_it = it + 1; break; }
		}
	}
	if (tid == 0) {
		if (status == MTFHIP_FLOW_NONFINITE) cx = cy = __builtin_nanf("");
		a.curr_pts[2 * p] = cx; a.curr_pts[2 * p + 1] = cy; a.n_iters[p] = n_it; a.status[p] = status;
	}
}

void launch_ncc_flow(int n_pts, const FlowArgs &a, hipStream_t st) {
	const int N = a.win_w * a.win_h, ppt = (N + kBlock - 1) / kBlock;
	const dim3 grid((unsigned)n_pts), block(kBlock);
#define MTFHIP_FLOW_CASE(P) case P: \
		if (a.fast_math) MTFHIP_LAUNCH((k_ncc_flow<P, true>), grid, block, 0, st, a); \
		else MTFHIP_LAUNCH((k_ncc_flow<P, false>), grid, block, 0, st, a); \
		break;
	switch (ppt) {
		MTFHIP_FLOW_CASE(1) MTFHIP_FLOW_CASE(2) MTFHIP_FLOW_CASE(3) MTFHIP_FLOW_CASE(4)
	default: note_launch_error(hipErrorInvalidValue, __FILE__, __LINE__); break;   /* (the entry points refuse N > kFlowMaxWin) */
	}
#undef MTFHIP_FLOW_CASE
}

} // namespace mtfhip
