/*
 * api_imap.hip -- the SCV family's own state and hooks: SCV, RSCV, LSCV and LRSCV (AM/src/SCV.cc, RSCV.cc, LSCV.cc, LRSCV.cc), SSD behind an
 * intensity map (C-ABI implementation, include/mtfhip.h; the kernels: kernels_imap.hip, kernels_fused_rscv.hip, kernels_fused_lrscv.hip;
 * the state: IntensityMapState, mtfhip_api_internal.h)
 *
 * SCV and LSCV are SSDBase models whose updateSimilarity first re-maps the template through the conditional expectation E[It | I0_orig]
 * (SCV.cc:194-230; LSCV.cc:263-304: one per sub-region, blended with per-pixel weights).  The device path keeps that split: imap_before_pass
 * re-maps MTFHIP_BUF_I0 in place, and the SSD code behind it (the per-function entry points, the fused SSD kernels) runs unchanged on it.
 * J0 / dI0_dx stay those of the original template (mapped_gradient 0).
 *
 * RSCV and LRSCV are SSDBase models whose updatePixVals maps the current patch through E[I0 | It] (RSCV.cc:170-238; LRSCV.cc:224-292: one per
 * sub-region, blended).  Everything behind updatePixVals is SSD on the mapped It.  The per-function route keeps that split literally
 * (imap_update_pix_vals writes MTFHIP_BUF_IT); the fused route enqueues pass 1 + the maps in front of the fused pass (imap_before_pass), which
 * applies them to every sample itself.  An LRSCV pass that does not map is an SSD pass on the raw patch.
 *
 * once_per_frame (LSCV.cc:264-265, LRSCV.cc:234-235): the localized models map on the first iteration of a frame only.
 *
 * Accepted and ignored: LSCVParams / LRSCVParams::pre_seed (pre-seeds of 0 go to getDiracJointHist, LSCV.cc:272-275, LRSCV.cc:240-243),
 * approx_dist_feat (LSCVDist only), show_subregions (an OpenCV window), debug_mode.
 */
#include "mtfhip_api_internal.h"

static inline size_t imap_regions(const mtfhip_batch *b) { return imap_localized(b) ? (size_t)b->imap.nx * b->imap.ny : 1; }
static inline const char *imap_tag(const mtfhip_batch *b) {   /* (the reference's class names in its messages) */
	static const char *const tag[4] = {"scv", "rscv", "lscv", "lrscv"};
	return tag[b->desc.am - MTFHIP_AM_SCV];
}

/* the sub-region extents of LSCV.cc:146-167 (LRSCV.cc:122-147) and the reference's refusal (fn: the entry point) */
static int check_geometry(const mtfhip_batch *b, int nx, int ny, int sx, int sy, const char *fn) {
	const char *am = intensity_mapped_name(b);
	if (nx < 1 || ny < 1) return fail(MTFHIP_ERR_INVALID_ARG, "%s: %s needs at least one sub-region per axis (got %d x %d)", fn, am, nx, ny);
	if (sx < 0 || sy < 0) return fail(MTFHIP_ERR_INVALID_ARG, "%s: %s sub-region spacing must not be negative (got %d x %d)", fn, am, sx, sy);
	const long long size_x = (long long)b->desc.resx - (long long)(nx - 1) * sx, size_y = (long long)b->desc.resy - (long long)(ny - 1) * sy;
	if (size_x <= 0 || size_y <= 0)
		return fail(MTFHIP_ERR_INVALID_ARG, "%s :: Patch size : %dx%d is not enough to use the specified region spacing and / or count", am,
			b->desc.resx, b->desc.resy);
	return MTFHIP_OK;
}

/* the cells of one axis: the distinct non-empty sets of sub-regions its coordinates lie in (contiguous runs: the first and the last
 * sub-region containing a coordinate never decrease along the axis); cell[v] = -1 outside every sub-region; rng[2 k], rng[2 k + 1]: the
 * first and the last cell of sub-region k */
static int axis_cells(int res, int n, int spacing, std::vector<int> &cell, std::vector<int> &rng) {
	const int size = res - (n - 1) * spacing;
	cell.assign(res, -1);
	rng.assign(2 * n, -1);
	int nc = 0, plo = -1, phi = -1;
	for (int v = 0; v < res; ++v) {
		int lo = -1, hi = -1;
		for (int k = 0; k < n; ++k)
			if (k * spacing <= v && v <= k * spacing + size - 1) { if (lo < 0) lo = k; hi = k; }
		if (lo < 0) continue;
		if (lo != plo || hi != phi) { ++nc; plo = lo; phi = hi; }
		cell[v] = nc - 1;
		for (int k = lo; k <= hi; ++k) { if (rng[2 * k] < 0) rng[2 * k] = nc - 1; rng[2 * k + 1] = nc - 1; }
	}
	return nc;
}

/* what imap_capture uploads from the host: alive until it has synchronised the stream */
struct ImapStage {
	std::vector<unsigned short> cell;
	std::vector<int> crng;
	std::vector<double> w, id, aff;
};

/* the sub-region geometry of LSCV and LRSCV at initializePixVals: the cell plane, the cells of each sub-region, the weights, the sums and
 * counters -- refused when the pass-1 table or the maps (map_lds_budget) exceed their LDS.  The uploads are enqueued only. */
static int imap_geometry(mtfhip_batch *b, size_t map_lds_budget, ImapStage &hs) {
	IntensityMapState &m = b->imap;
	const int nx = m.nx, ny = m.ny, R = nx * ny, resx = b->desc.resx, resy = b->desc.resy;
	const char *am = intensity_mapped_name(b);
	TRY(check_geometry(b, nx, ny, m.sx, m.sy, "init_template"));
	std::vector<int> cx, cy, rx, ry;
	const int ncx = axis_cells(resx, nx, m.sx, cx, rx), ncy = axis_cells(resy, ny, m.sy, cy, ry);
	const size_t B = (size_t)b->B, N = (size_t)b->N, nb = (size_t)m.nb, ncell = (size_t)ncx * ncy;
	if (ncell >= 0xffff) return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "init_template: %s with %zu sub-region cells (at most 65534)", am, ncell);
	const size_t lds_hist = 2 * sizeof(unsigned) * ncell * nb, lds_map = sizeof(double) * (size_t)R * nb;
	if (lds_hist > (size_t)kLscvLdsBudget - 64 || lds_map > map_lds_budget)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED,
			"init_template: %s with %d x %d sub-regions (%zu cells) at %zu bins needs %zu B of LDS for its histograms and %zu B for its maps "
			"(the limits are %d B and %zu B per workgroup)", am, nx, ny, ncell, nb, lds_hist, lds_map, kLscvLdsBudget - 64, map_lds_budget);
	if ((double)(nb - 1) * (double)N >= 4294967296.0)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "init_template: %s with %zu sample points at %zu bins could overflow its u32 histogram sums", am, N, nb);
	hipStream_t st = b->ctx->stream;
	/* (the cell plane arrives last: the sums and counters are zeroed once the whole group is there) */
	const bool first = !m.cell;
	HIP_TRY(m.crng.reserve(2 * (size_t)(nx + ny)));
	HIP_TRY(m.w.reserve((size_t)R * N));
	HIP_TRY(m.tot.reserve(2 * ncell * nb * B));
	HIP_TRY(m.arrive.reserve(B));
	HIP_TRY(m.map.reserve((size_t)R * nb * B));
	HIP_TRY(m.aff.reserve(2 * (size_t)R * B));
	if (first) {
		HIP_TRY(hipMemsetAsync(m.tot, 0, sizeof(unsigned) * 2 * ncell * nb * B, st));
		HIP_TRY(hipMemsetAsync(m.arrive, 0, sizeof(unsigned) * B, st));
	}
	HIP_TRY(m.cell.reserve(N));
	m.ncx = ncx; m.ncell = (int)ncell;
	/* pixel i at (i % resx, i / resx): its cell, and sub_region_wts (LSCV.cc:170-197), computed as the reference does -- the centre
	 * (start + end) / 2.0, the difference truncated toward zero, 1 / (1 + dx^2 + dy^2), each row divided by its sum taken idy outer,
	 * idx inner */
	hs.cell.resize(N);
	hs.w.resize((size_t)R * N);
	std::vector<double> cen_x(nx), cen_y(ny), row(R);
	const int size_x = resx - (nx - 1) * m.sx, size_y = resy - (ny - 1) * m.sy;
	for (int idx = 0; idx < nx; ++idx) cen_x[idx] = static_cast<double>(idx * m.sx + idx * m.sx + size_x - 1) / 2.0;
	for (int idy = 0; idy < ny; ++idy) cen_y[idy] = static_cast<double>(idy * m.sy + idy * m.sy + size_y - 1) / 2.0;
	for (size_t i = 0; i < N; ++i) {
		const unsigned px = (unsigned)(i % resx), py = (unsigned)(i / resx);
		hs.cell[i] = (cx[px] < 0 || cy[py] < 0) ? (unsigned short)0xffff : (unsigned short)(cy[py] * ncx + cx[px]);
		double sum = 0;
		for (int idy = 0; idy < ny; ++idy)
			for (int idx = 0; idx < nx; ++idx) {
				const int dx = static_cast<int>(px - cen_x[idx]), dy = static_cast<int>(py - cen_y[idy]);
				const double pw = 1.0 / static_cast<double>(1.0 + dx * dx + dy * dy);
				sum += row[idy * nx + idx] = pw;
			}
		for (int r = 0; r < R; ++r) hs.w[(size_t)r * N + i] = row[r] / sum;
	}
	hs.crng = rx;
	hs.crng.insert(hs.crng.end(), ry.begin(), ry.end());
	HIP_TRY(hipMemcpyAsync(m.cell, hs.cell.data(), sizeof(unsigned short) * N, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(m.crng, hs.crng.data(), sizeof(int) * hs.crng.size(), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(m.w, hs.w.data(), sizeof(double) * hs.w.size(), hipMemcpyHostToDevice, st));
	return MTFHIP_OK;
}

int imap_capture(mtfhip_batch *b) {
	if (!intensity_mapped(b)) return MTFHIP_OK;
	IntensityMapState &m = b->imap;
	const bool local = imap_localized(b), rev = imap_reversed(b);
	const size_t B = (size_t)b->B, N = (size_t)b->N, nb = (size_t)m.nb, R = imap_regions(b);
	hipStream_t st = b->ctx->stream;
	ImapStage hs;
	/* (LRSCV's maps live in the fused pass's dynamic LDS beside its static arrays) */
	if (local) TRY(imap_geometry(b, (size_t)kLscvLdsBudget - (rev ? kLrscvFusedStaticLds : 0), hs));
	const bool first = !m.captured();
	if (!local) {
		const size_t rows = (size_t)imap_hist_blocks(b->N, kImapChunks) * 2 * nb * B;
		if (rev) { HIP_TRY(m.part_u.reserve(rows)); HIP_TRY(m.arrive.reserve(B)); }
		else HIP_TRY(m.part_f.reserve(rows));
		HIP_TRY(m.map.reserve(nb * B));
	}
	HIP_TRY(m.orig.reserve(N * B));
	if (rev && !local && first) HIP_TRY(hipMemsetAsync(m.arrive, 0, sizeof(unsigned) * B, st));
	/* I0_orig = I0 (SCV.cc:166, LSCV.cc:232); the reversed models' first call: It = I0, It_orig = It (RSCV.cc:158-162, LRSCV.cc:208-210) */
	if (!rev || local || first) HIP_TRY(hipMemcpyAsync(m.orig, b->buf[MTFHIP_BUF_I0], sizeof(double) * N * B, hipMemcpyDeviceToDevice, st));
	/* the template's bins: of I0_orig, or the reversed models' columns of the joint histogram (int)I0 */
	if (rev) {
		HIP_TRY(m.code8.reserve(N * B));
		launch_rscv_codes(b->N, b->B, m.nb, b->buf[MTFHIP_BUF_I0], m.code8, st);
	} else {
		HIP_TRY(m.code16.reserve(N * B));
		launch_scv_codes(b->N, b->B, m.nb, m.orig, m.code16, st);
	}
	/* before the first update the maps are the identity of the bins (what the empty-bin rule gives), the affine fits a = 1, c = 0 */
	hs.id.resize(R * nb * B);
	for (size_t k = 0; k < hs.id.size(); ++k) hs.id[k] = (double)(k % nb);
	HIP_TRY(hipMemcpyAsync(m.map, hs.id.data(), sizeof(double) * hs.id.size(), hipMemcpyHostToDevice, st));
	if (local) {
		hs.aff.resize(2 * R * B);
		for (size_t k = 0; k < hs.aff.size(); ++k) hs.aff[k] = k % 2 == 0 ? 1.0 : 0.0;
		HIP_TRY(hipMemcpyAsync(m.aff, hs.aff.data(), sizeof(double) * hs.aff.size(), hipMemcpyHostToDevice, st));
	}
	HIP_TRY(hipStreamSynchronize(st));   /* (hs is a stack-lifetime buffer) */
	return MTFHIP_OK;
}

/* the argument block of the model's pass 1 and what follows it, for the targets [t0, t0 + bv.B); kind: how pass 1 obtains It (RSCV_IT_*) */
static ImapArgs imap_args(const mtfhip_batch *b, const BatchView &bv, int t0, const int *active, int kind) {
	const IntensityMapState &m = b->imap;
	const size_t N = (size_t)b->N, nb = (size_t)m.nb, R = imap_regions(b), E = (size_t)m.ncell * nb;
	const size_t rows = (size_t)imap_hist_blocks(b->N, kImapChunks) * 2 * nb;
	ImapArgs a;
	a.nb = m.nb; a.kind = kind;
	a.hist = m.hist; a.linear = m.linear; a.affine = m.affine;
	a.nx = m.nx; a.ny = m.ny; a.ncx = m.ncx; a.ncell = m.ncell;
	a.norm_mult = b->norm_mult; a.norm_add = b->norm_add; a.grad_eps = b->desc.grad_eps;
	/* (the buffers a model does not have are null, and stay so) */
	a.src = kind != RSCV_IT_FROM_BUF ? nullptr : (imap_reversed(b) ? m.orig + (size_t)t0 * N : bv.buf[MTFHIP_BUF_IT]);
	a.code16 = m.code16 ? m.code16 + (size_t)t0 * N : nullptr;
	a.code8 = m.code8 ? m.code8 + (size_t)t0 * N : nullptr;
	a.i0o = m.orig + (size_t)t0 * N;
	a.cell = m.cell; a.crng = m.crng; a.wts = m.w;
	a.active = active;
	a.part_f = m.part_f ? m.part_f + (size_t)t0 * rows : nullptr;
	a.part_u = m.part_u ? m.part_u + (size_t)t0 * rows : nullptr;
	a.tot = m.tot ? m.tot + (size_t)t0 * 2 * E : nullptr;
	a.arrive = m.arrive ? m.arrive + t0 : nullptr;
	a.map = m.map + (size_t)t0 * R * nb;
	a.aff = m.aff ? m.aff + (size_t)t0 * 2 * R : nullptr;
	return a;
}

/* SCV / LSCV: I0 = map(I0_orig) for the targets [t0, t0 + bv.B) */
static void remap_template(mtfhip_batch *b, const BatchView &bv, int t0, const int *active, int from_it, hipStream_t st) {
	const ImapArgs a = imap_args(b, bv, t0, active, from_it ? RSCV_IT_FROM_BUF : RSCV_IT_REPLAY);
	TimedScope ts(b->ctx, imap_localized(b) ? "lscv_remap" : "scv_remap", st);
	if (imap_localized(b)) launch_lscv_update(bv, b->ctx->img, a, bv.buf[MTFHIP_BUF_I0], st);
	else launch_scv_update(bv, b->ctx->img, a, bv.buf[MTFHIP_BUF_I0], st);
	touch(b, MTFHIP_BUF_I0);
}

/* the It_orig expression (RSCV_IT_*) of the fused launch fa selects (launch_fused_rscv / launch_fused_lrscv: the same for either model and
 * SSM); RSCV_IT_FROM_BUF without one (the per-function route) */
static int rscv_it_kind(const FusedArgs *fa) {
	if (!fa) return RSCV_IT_FROM_BUF;
	return fused_it_kind(fused_select(FUSED_ROUTE_LOOP, MTFHIP_AM_RSCV, 1, MTFHIP_SSM_HOMOGRAPHY, fa->mode, fa->chained, fa->materialize, fa->fast_math));
}

/* RSCV / LRSCV: pass 1 and the maps of the current patch for the targets [t0, t0 + bv.B) */
static void map_current(mtfhip_batch *b, const BatchView &bv, int t0, const int *active, const FusedArgs *fa, hipStream_t st) {
	const ImapArgs a = imap_args(b, bv, t0, active, rscv_it_kind(fa));
	if (imap_localized(b)) launch_lrscv_hist(bv, b->ctx->img, a, st);
	else launch_rscv_hist(bv, b->ctx->img, a, st);
}

/* ... and what applies them from the target t0 on: the map (RSCV), the blend (LRSCV) */
static FusedMaps current_maps(const mtfhip_batch *b, int t0) {
	const IntensityMapState &m = b->imap;
	const size_t R = imap_regions(b);
	FusedMaps fm;
	if (imap_localized(b)) {
		fm.lm.map = m.affine ? m.aff + (size_t)t0 * 2 * R : m.map + (size_t)t0 * R * m.nb;
		fm.lm.wts = m.w;
		fm.lm.nb = m.nb; fm.lm.R = (int)R; fm.lm.affine = m.affine; fm.lm.linear = m.linear;
	} else {
		fm.rm.map = m.map + (size_t)t0 * m.nb;
		fm.rm.nb = m.nb; fm.rm.linear = m.linear;
	}
	return fm;
}

int imap_before_pass(mtfhip_batch *b, const BatchView *chunk, int t0, const int *active, const FusedArgs *fa, int from_it, bool first_pass,
	hipStream_t st, FusedMaps *out) {
	if (!intensity_mapped(b)) return MTFHIP_OK;
	const bool rev = imap_reversed(b);
	if (rev && !fa) return MTFHIP_OK;
	/* once_per_frame: only on the first iteration of a frame (LSCV.cc:264-265, LRSCV.cc:234-235) */
	if (imap_localized(b) && b->imap.once && !first_pass) return MTFHIP_OK;
	if (!b->imap.captured()) return fail(MTFHIP_ERR_LOGIC, "%s :: %s before initializePixVals", imap_tag(b), rev ? "updatePixVals" : "updateSimilarity");
	const BatchView bv = chunk ? *chunk : b->view();
	if (!rev) { remap_template(b, bv, t0, active, from_it, st); return MTFHIP_OK; }
	if (fa->grad_eps != b->desc.grad_eps || fa->norm_mult != b->norm_mult || fa->norm_add != b->norm_add)
		return fail(MTFHIP_ERR_LOGIC, "%s :: the fused launch's normalisation is not the batch's", imap_tag(b));
	{
		TimedScope ts(b->ctx, imap_localized(b) ? "lrscv_map" : "rscv_map", st);
		map_current(b, bv, t0, active, fa, st);
	}
	*out = current_maps(b, t0);
	return MTFHIP_OK;
}

int imap_update_pix_vals(mtfhip_batch *b, const double *dp) {
	if (!imap_reversed(b)) return IMAP_NOT_MINE;
	if (!b->imap.captured()) return fail(MTFHIP_ERR_LOGIC, "%s :: updatePixVals before initializePixVals", imap_tag(b));
	const IntensityMapState &m = b->imap;
	hipStream_t st = b->ctx->stream;
	TimedScope ts(b->ctx, "sample");
	const BatchView bv = b->view();
	/* LRSCV under once_per_frame and not on the first iteration: It at the current points is all (LRSCV.cc:226-235) */
	if (imap_localized(b) && m.once && !b->first_iter) {
		launch_sample(bv, b->ctx->img, dp, b->buf[MTFHIP_BUF_IT], b->norm_mult, b->norm_add, st);
		return MTFHIP_OK;
	}
	/* It_orig at the current points (RSCV.cc:171-189, LRSCV.cc:226-232), the joint histograms and the maps (RSCV.cc:204-229, LRSCV.cc:237-247),
	 * It = map(It_orig) (RSCV.cc:230-234) or the blend (LRSCV.cc:249-254) */
	launch_sample(bv, b->ctx->img, dp, m.orig, b->norm_mult, b->norm_add, st);
	map_current(b, bv, 0, nullptr, nullptr, st);
	if (imap_localized(b)) launch_lrscv_apply(b->N, b->B, current_maps(b, 0).lm, m.orig, b->buf[MTFHIP_BUF_IT], st);
	else launch_rscv_apply(b->N, b->B, m.nb, m.linear, m.map, m.orig, b->buf[MTFHIP_BUF_IT], st);
	return MTFHIP_OK;
}

/* mtfhip_batch_set_lscv / _set_lrscv for the model am, named fn in the messages */
static int set_localized(mtfhip_batch *b, int am, const char *fn, int nx, int ny, int sx, int sy, int affine_mapping, int once_per_frame,
	int weighted_mapping) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL batch", fn);
	if (b->desc.am != am) return fail(MTFHIP_ERR_INVALID_ARG, "%s: the batch's appearance model is %d, not %s", fn, b->desc.am, am_traits(am).name);
	if (b->imap.cell) return fail(MTFHIP_ERR_LOGIC, "%s: call it before init_template (the sub-region geometry is fixed there)", fn);
	if ((affine_mapping != 0 && affine_mapping != 1) || (once_per_frame != 0 && once_per_frame != 1) || (weighted_mapping != 0 && weighted_mapping != 1))
		return fail(MTFHIP_ERR_INVALID_ARG, "%s: affine_mapping, once_per_frame and weighted_mapping must be 0 or 1 (got %d, %d, %d)", fn, affine_mapping,
			once_per_frame, weighted_mapping);
	TRY(check_geometry(b, nx, ny, sx, sy, fn));
	IntensityMapState &m = b->imap;
	m.nx = nx; m.ny = ny; m.sx = sx; m.sy = sy;
	m.affine = affine_mapping; m.once = once_per_frame; m.linear = weighted_mapping;
	return MTFHIP_OK;
}

/* the four *_intensity_map(s) getters for the model am, named fn in the messages: [B][R][nb] */
static int get_maps(mtfhip_batch *b, int am, const char *fn, double *dst) {
	if (!b || !dst) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);
	if (b->desc.am != am) return fail(MTFHIP_ERR_INVALID_ARG, "%s: the batch's appearance model is %d, not %s", fn, b->desc.am, am_traits(am).name);
	FLUSH(b);
	if (!b->imap.map) return fail(MTFHIP_ERR_LOGIC, "%s before initializePixVals", fn);
	HIP_TRY(hipMemcpyAsync(dst, b->imap.map, sizeof(double) * imap_regions(b) * b->imap.nb * b->B, hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	return MTFHIP_OK;
}

extern "C" {

int mtfhip_batch_set_scv(mtfhip_batch *b, int hist_type, int weighted_mapping, int mapped_gradient) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "set_scv: NULL batch");
	if (b->desc.am != MTFHIP_AM_SCV) return fail(MTFHIP_ERR_INVALID_ARG, "set_scv: the batch's appearance model is %d, not SCV", b->desc.am);
	if (hist_type == MTFHIP_SCV_HIST_BSPLINE)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "set_scv: SCV hist_type BSpline is not available on the device path (Dirac and Bilinear are)");
	if (hist_type != MTFHIP_SCV_HIST_DIRAC && hist_type != MTFHIP_SCV_HIST_BILINEAR)
		return fail(MTFHIP_ERR_INVALID_ARG, "set_scv: Invalid histogram type provided (%d)", hist_type);
	if (mapped_gradient)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "set_scv: SCV mapped_gradient = 1 (the template gradient re-mapped through the intensity map) is not available on the device path");
	if (weighted_mapping != 0 && weighted_mapping != 1) return fail(MTFHIP_ERR_INVALID_ARG, "set_scv: weighted_mapping must be 0 or 1 (got %d)", weighted_mapping);
	b->imap.hist = hist_type;
	b->imap.linear = weighted_mapping;
	b->imap.mapped_grad = 0;
	return MTFHIP_OK;
}

int mtfhip_batch_set_rscv(mtfhip_batch *b, int use_bspl, int weighted_mapping, int mapped_gradient) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "set_rscv: NULL batch");
	if (b->desc.am != MTFHIP_AM_RSCV) return fail(MTFHIP_ERR_INVALID_ARG, "set_rscv: the batch's appearance model is %d, not RSCV", b->desc.am);
	if (use_bspl)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "set_rscv: RSCV use_bspl = 1 (BSpline histograms) is not available on the device path (Dirac histograms are)");
	if (mapped_gradient)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "set_rscv: RSCV mapped_gradient = 1 (the current gradient taken through the intensity map) is not available on the device path");
	if (weighted_mapping != 0 && weighted_mapping != 1) return fail(MTFHIP_ERR_INVALID_ARG, "set_rscv: weighted_mapping must be 0 or 1 (got %d)", weighted_mapping);
	b->imap.linear = weighted_mapping;
	return MTFHIP_OK;
}

int mtfhip_batch_set_lscv(mtfhip_batch *b, int n_sub_regions_x, int n_sub_regions_y, int spacing_x, int spacing_y, int affine_mapping,
	int once_per_frame, int weighted_mapping) {
	return set_localized(b, MTFHIP_AM_LSCV, "set_lscv", n_sub_regions_x, n_sub_regions_y, spacing_x, spacing_y, affine_mapping, once_per_frame, weighted_mapping);
}
int mtfhip_batch_set_lrscv(mtfhip_batch *b, int n_sub_regions_x, int n_sub_regions_y, int spacing_x, int spacing_y, int affine_mapping,
	int once_per_frame, int weighted_mapping) {
	return set_localized(b, MTFHIP_AM_LRSCV, "set_lrscv", n_sub_regions_x, n_sub_regions_y, spacing_x, spacing_y, affine_mapping, once_per_frame, weighted_mapping);
}

int mtfhip_batch_scv_intensity_map(mtfhip_batch *b, double *dst) { return get_maps(b, MTFHIP_AM_SCV, "scv_intensity_map", dst); }
int mtfhip_batch_rscv_intensity_map(mtfhip_batch *b, double *dst) { return get_maps(b, MTFHIP_AM_RSCV, "rscv_intensity_map", dst); }
int mtfhip_batch_lscv_intensity_maps(mtfhip_batch *b, double *dst) { return get_maps(b, MTFHIP_AM_LSCV, "lscv_intensity_maps", dst); }
int mtfhip_batch_lrscv_intensity_maps(mtfhip_batch *b, double *dst) { return get_maps(b, MTFHIP_AM_LRSCV, "lrscv_intensity_maps", dst); }

int mtfhip_batch_set_first_iter(mtfhip_batch *b, int on) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "set_first_iter: NULL batch");
	b->first_iter = on ? 1 : 0;
	return MTFHIP_OK;
}

int mtfhip_batch_first_iter(const mtfhip_batch *b) { return b && b->first_iter ? 1 : 0; }

} /* extern "C" */
