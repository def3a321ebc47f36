/*
 * api_lscv.hip -- the Localized SCV appearance model's own state (AM/src/LSCV.cc): I0_orig, the sub-region geometry, the per-iteration
 * localized template re-map, its configuration (C-ABI implementation, include/mtfhip.h; the kernels: kernels_lscv.hip)
 *
 * LSCV is an SSDBase whose updateSimilarity first re-maps the template through one conditional expectation E[It | I0_orig] per
 * sub-region and blends the re-mapped templates with per-pixel weights (LSCV.cc:263-304).  As SCV, the device path keeps that split:
 * lscv_enqueue re-maps MTFHIP_BUF_I0 in place, and the SSD code behind it (the per-function entry points, the fused SSD kernels) runs
 * unchanged on it.  J0 / dI0_dx stay those of the original template.
 *
 * Accepted and ignored: LSCVParams::pre_seed (updateSimilarity passes pre-seeds of 0 to getDiracJointHist, LSCV.cc:272-275),
 * approx_dist_feat (LSCVDist only, LSCV.cc:322-...), show_subregions (an OpenCV window, LSCV.cc:243-245, :306-...).
 */
#include "mtfhip_api_internal.h"

#include <climits>

/* the sub-region extents of LSCV.cc:146-167 (LRSCV.cc:122-147) and the reference's refusal */
int lscv_check_geometry(const mtfhip_batch *b, int nx, int ny, int sx, int sy, const char *fn) {
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
static int lscv_axis_cells(int res, int n, int spacing, std::vector<int> &cell, std::vector<int> &rng) {
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

int lscv_geometry(mtfhip_batch *b, size_t map_lds_budget) {
	const int nx = b->lscv_nx, ny = b->lscv_ny, R = nx * ny, resx = b->desc.resx, resy = b->desc.resy;
	const char *am = intensity_mapped_name(b);
	TRY(lscv_check_geometry(b, nx, ny, b->lscv_sx, b->lscv_sy, "init_template"));
	std::vector<int> cx, cy, rx, ry;
	const int ncx = lscv_axis_cells(resx, nx, b->lscv_sx, cx, rx), ncy = lscv_axis_cells(resy, ny, b->lscv_sy, cy, ry);
	const size_t B = (size_t)b->B, N = (size_t)b->N, nb = (size_t)b->lscv_nb, ncell = (size_t)ncx * ncy;
	if (ncell >= 0xffff) return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "init_template: %s with %zu sub-region cells (at most 65534)", am, ncell);
	const size_t lds_hist = 2 * sizeof(unsigned) * ncell * nb, lds_map = sizeof(double) * (size_t)R * nb;
	if (lds_hist > (size_t)kLscvLdsBudget - 64 || lds_map > map_lds_budget)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED,
			"init_template: %s with %d x %d sub-regions (%zu cells) at %zu bins needs %zu B of LDS for its histograms and %zu B for its maps "
			"(the limits are %d B and %zu B per workgroup)", am, nx, ny, ncell, nb, lds_hist, lds_map, kLscvLdsBudget - 64, map_lds_budget);
	if ((double)(nb - 1) * (double)N >= 4294967296.0)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "init_template: %s with %zu sample points at %zu bins could overflow its u32 histogram sums", am, N, nb);
	hipStream_t st = b->ctx->stream;
	/* (d_lscv_cell, which set_lscv / set_lrscv take for "the geometry is fixed", arrives last: while it is null a failed call is simply
	 * repeated, and the sums and counters are zeroed once the whole group is there) */
	const bool first = !b->d_lscv_cell;
	HIP_TRY(b->d_lscv_crng.reserve(2 * (size_t)(nx + ny)));
	HIP_TRY(b->d_lscv_w.reserve((size_t)R * N));
	HIP_TRY(b->d_lscv_tot.reserve(2 * ncell * nb * B));
	HIP_TRY(b->d_lscv_arrive.reserve(B));
	HIP_TRY(b->d_lscv_map.reserve((size_t)R * nb * B));
	HIP_TRY(b->d_lscv_aff.reserve(2 * (size_t)R * B));
	if (first) {
		HIP_TRY(hipMemsetAsync(b->d_lscv_tot, 0, sizeof(unsigned) * 2 * ncell * nb * B, st));
		HIP_TRY(hipMemsetAsync(b->d_lscv_arrive, 0, sizeof(unsigned) * B, st));
	}
	HIP_TRY(b->d_lscv_cell.reserve(N));
	b->lscv_ncx = ncx; b->lscv_ncell = (int)ncell;
	/* pixel i at (i % resx, i / resx): its cell, and sub_region_wts (LSCV.cc:170-197), computed as the reference does -- the centre
	 * (start + end) / 2.0, the difference truncated toward zero, 1 / (1 + dx^2 + dy^2), each row divided by its sum taken idy outer,
	 * idx inner */
	std::vector<unsigned short> cell(N);
	std::vector<double> w((size_t)R * N), cen_x(nx), cen_y(ny);
	const int size_x = resx - (nx - 1) * b->lscv_sx, size_y = resy - (ny - 1) * b->lscv_sy;
	for (int idx = 0; idx < nx; ++idx) cen_x[idx] = static_cast<double>(idx * b->lscv_sx + idx * b->lscv_sx + size_x - 1) / 2.0;
	for (int idy = 0; idy < ny; ++idy) cen_y[idy] = static_cast<double>(idy * b->lscv_sy + idy * b->lscv_sy + size_y - 1) / 2.0;
	std::vector<double> row(R);
	for (size_t i = 0; i < N; ++i) {
		const unsigned px = (unsigned)(i % resx), py = (unsigned)(i / resx);
		cell[i] = (cx[px] < 0 || cy[py] < 0) ? (unsigned short)0xffff : (unsigned short)(cy[py] * ncx + cx[px]);
		double sum = 0;
		for (int idy = 0; idy < ny; ++idy)
			for (int idx = 0; idx < nx; ++idx) {
				const int dx = static_cast<int>(px - cen_x[idx]), dy = static_cast<int>(py - cen_y[idy]);
				const double pw = 1.0 / static_cast<double>(1.0 + dx * dx + dy * dy);
				sum += row[idy * nx + idx] = pw;
			}
		for (int r = 0; r < R; ++r) w[(size_t)r * N + i] = row[r] / sum;
	}
	std::vector<int> crng(rx);
	crng.insert(crng.end(), ry.begin(), ry.end());
	/* before the first update the maps are the identity of the bins (what the empty-bin rule gives), the affine fits a = 1, c = 0 */
	std::vector<double> id((size_t)R * nb * B), aff(2 * (size_t)R * B);
	for (size_t k = 0; k < id.size(); ++k) id[k] = (double)(k % nb);
	for (size_t k = 0; k < aff.size(); ++k) aff[k] = k % 2 == 0 ? 1.0 : 0.0;
	HIP_TRY(hipMemcpyAsync(b->d_lscv_cell, cell.data(), sizeof(unsigned short) * N, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(b->d_lscv_crng, crng.data(), sizeof(int) * crng.size(), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(b->d_lscv_w, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(b->d_lscv_map, id.data(), sizeof(double) * id.size(), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(b->d_lscv_aff, aff.data(), sizeof(double) * aff.size(), hipMemcpyHostToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));   /* (stack-lifetime buffers) */
	return MTFHIP_OK;
}

int lscv_capture(mtfhip_batch *b) {
	TRY(lscv_geometry(b, (size_t)kLscvLdsBudget));
	const size_t B = (size_t)b->B, N = (size_t)b->N;
	hipStream_t st = b->ctx->stream;
	HIP_TRY(b->d_lscv_code.reserve(N * B));
	HIP_TRY(b->d_lscv_i0.reserve(N * B));   /* (last: lscv_enqueue takes it for "captured") */
	/* I0_orig = I0 (LSCV.cc:232) and its bins */
	HIP_TRY(hipMemcpyAsync(b->d_lscv_i0, b->buf[MTFHIP_BUF_I0], sizeof(double) * N * B, hipMemcpyDeviceToDevice, st));
	launch_scv_codes(b->N, b->B, b->lscv_nb, b->d_lscv_i0, b->d_lscv_code, st);
	return MTFHIP_OK;
}

int lscv_enqueue(mtfhip_batch *b, const BatchView &bv, int t0, const int *active, int from_it, hipStream_t st) {
	if (!b->d_lscv_i0) return fail(MTFHIP_ERR_LOGIC, "lscv :: updateSimilarity before initializePixVals");
	const size_t N = (size_t)b->N, nb = (size_t)b->lscv_nb, R = (size_t)b->lscv_nx * b->lscv_ny, E = (size_t)b->lscv_ncell * nb;
	LscvArgs a;
	a.nb = b->lscv_nb; a.nx = b->lscv_nx; a.ny = b->lscv_ny; a.ncx = b->lscv_ncx; a.ncell = b->lscv_ncell;
	a.from_it = from_it; a.affine = b->lscv_affine; a.linear = b->lscv_linear;
	a.norm_mult = b->norm_mult; a.norm_add = b->norm_add;
	a.code = b->d_lscv_code + (size_t)t0 * N;
	a.i0o = b->d_lscv_i0 + (size_t)t0 * N;
	a.cell = b->d_lscv_cell; a.crng = b->d_lscv_crng; a.wts = b->d_lscv_w;
	a.active = active;
	a.tot = b->d_lscv_tot + (size_t)t0 * 2 * E;
	a.arrive = b->d_lscv_arrive + t0;
	a.map = b->d_lscv_map + (size_t)t0 * R * nb;
	a.aff = b->d_lscv_aff + (size_t)t0 * 2 * R;
	{
		TimedScope ts(b->ctx, "lscv_remap", st);
		launch_lscv_update(bv, b->ctx->img, a, bv.buf[MTFHIP_BUF_I0], st);
	}
	touch(b, MTFHIP_BUF_I0);
	return MTFHIP_OK;
}

extern "C" {

int mtfhip_batch_set_lscv(mtfhip_batch *b, int n_sub_regions_x, int n_sub_regions_y, int spacing_x, int spacing_y, int affine_mapping,
	int once_per_frame, int weighted_mapping) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "set_lscv: NULL batch");
	if (b->desc.am != MTFHIP_AM_LSCV) return fail(MTFHIP_ERR_INVALID_ARG, "set_lscv: the batch's appearance model is %d, not LSCV", b->desc.am);
	if (b->d_lscv_cell) return fail(MTFHIP_ERR_LOGIC, "set_lscv: call it before init_template (the sub-region geometry is fixed there)");
	if ((affine_mapping != 0 && affine_mapping != 1) || (once_per_frame != 0 && once_per_frame != 1) || (weighted_mapping != 0 && weighted_mapping != 1))
		return fail(MTFHIP_ERR_INVALID_ARG, "set_lscv: affine_mapping, once_per_frame and weighted_mapping must be 0 or 1 (got %d, %d, %d)", affine_mapping,
			once_per_frame, weighted_mapping);
	TRY(lscv_check_geometry(b, n_sub_regions_x, n_sub_regions_y, spacing_x, spacing_y, "set_lscv"));
	b->lscv_nx = n_sub_regions_x; b->lscv_ny = n_sub_regions_y;
	b->lscv_sx = spacing_x; b->lscv_sy = spacing_y;
	b->lscv_affine = affine_mapping; b->lscv_once = once_per_frame; b->lscv_linear = weighted_mapping;
	return MTFHIP_OK;
}

int mtfhip_batch_lscv_intensity_maps(mtfhip_batch *b, double *dst) {
	if (!b || !dst) return fail(MTFHIP_ERR_INVALID_ARG, "lscv_intensity_maps: NULL argument");
	if (b->desc.am != MTFHIP_AM_LSCV) return fail(MTFHIP_ERR_INVALID_ARG, "lscv_intensity_maps: the batch's appearance model is %d, not LSCV", b->desc.am);
	FLUSH(b);
	if (!b->d_lscv_map) return fail(MTFHIP_ERR_LOGIC, "lscv_intensity_maps before initializePixVals");
	HIP_TRY(hipMemcpyAsync(dst, b->d_lscv_map, sizeof(double) * (size_t)b->lscv_nx * b->lscv_ny * b->lscv_nb * b->B, hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	return MTFHIP_OK;
}

int mtfhip_batch_set_first_iter(mtfhip_batch *b, int on) {
	if (!b) return fail(MTFHIP_ERR_INVALID_ARG, "set_first_iter: NULL batch");
	b->lscv_first_iter = on ? 1 : 0;
	return MTFHIP_OK;
}

int mtfhip_batch_first_iter(const mtfhip_batch *b) { return b && b->lscv_first_iter ? 1 : 0; }

} /* extern "C" */
