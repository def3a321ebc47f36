/*
 * api_grid.hip -- the grid tracker: the fused re-initialisation of its patches, mtfhip_grid_update / _frame / _fb_mask / _backward / _frame_fb / _reset
 * (C-ABI implementation, include/mtfhip.h; shared declarations: mtfhip_api_internal.h; no CPU fallback: HIP kernels or an error)
 */
#include "mtfhip_api_internal.h"

extern "C" {

/* resetTrackers(reinit) for the patches of a grid: setCorners + initialize of every patch tracker in ONE launch -- the host half of the
 * reset (mirrors, staged corners; set_corners_core deferred) and k_template_init in region mode, which reads the patch corners from the
 * pinned staging buffer and lays out its own grid (as k_iclk_track does for the per-frame setRegion) */
static int grid_reinit_fused(mtfhip_batch *b, const mtfhip_sm_desc *sm, const double *patches, bool layout_later = false) {
	const bool dbg = g_track_dbg_timing;
	const auto t0 = std::chrono::steady_clock::now();
	/* a record of the PREVIOUS fused initialisation that nobody has asked for (reset-every-frame mode: mtfhip_grid_frame holds it back) is
	 * superseded by this one: every mirror it would fill is rewritten by the new record -- not folding it in saves the host 1 KB per patch of
	 * cold reads (12 us per frame at 256 patches).  With recorded interface calls pending the flush below still wants it. */
	/* (r05 advisor: a call that fails before the new launch is enqueued -- check_sm, need_image, degenerate corners in set_corners_core -- must not
	 * leave the mirrors older than d_h0 / d_ncc / d_ncc_tm with nothing pending: the dropped record is put back on those paths) */
	const unsigned long long dropped_seq = (b->init_mirror_seq && !b->lz.any()) ? b->init_mirror_seq : 0;
	const bool dropped_dev = b->init_rec_device;
	if (dropped_seq) b->init_mirror_seq = 0;
#define REINIT_TRY(expr) do { const int _rc = (expr); if (_rc != MTFHIP_OK) { if (dropped_seq && !b->init_mirror_seq) { b->init_mirror_seq = dropped_seq; b->init_rec_device = dropped_dev; } return _rc; } } while (0)
	REINIT_TRY(lazy_flush(b, false));   /* (the current points are about to be replaced: no apply_warp for them -- 7 us per frame when this was FLUSH) */
	REINIT_TRY(begin_entry(b));
	REINIT_TRY(check_sm(b, sm, "init_template"));
	REINIT_TRY(need_image(b));
	const auto t1 = std::chrono::steady_clock::now();
	REINIT_TRY(set_corners_core(b, layout_later ? nullptr : patches, false, true, layout_later));   /* (layout_later: b->deferred_gdesc / _region / _region_map are set, mtfhip_grid_reset) */
#undef REINIT_TRY
	const auto t2 = std::chrono::steady_clock::now();
	b->init_pix_vals = b->init_pix_grad = b->init_sim = b->init_grad = false;
	RegionIngest rg = region_geometry(b);
	const double *stage = reinterpret_cast<const double *>(b->h_stage_a_dev);
	rg.corners = stage + 17 * (size_t)b->B; rg.ncc = nullptr;
	rg.d_ncc = b->d_ncc; rg.d_w0 = b->d_w0; rg.d_init_corners_hm = b->d_init_corners_hm;
	if (layout_later) region_deferred_layout(b, rg);
	/* (no host publish: a grid re-initialises every frame and its records are superseded unread -- the pinned stores and their acknowledgement
	 * were ~2 us at the tail of every workgroup; a caller that does read the mirrors copies d_h0 / d_ncc / d_ncc_tm, pull_init_mirrors) */
	static const bool rec_pinned = std::getenv("MTFHIP_GRID_INIT_PUBLISH") && std::getenv("MTFHIP_GRID_INIT_PUBLISH")[0] == '1';
	const int rc = init_template_fused(b, sm, &rg, rec_pinned);
	const auto t3 = std::chrono::steady_clock::now();
	set_corners_finish_deferred(b);   /* the host half of a deferred reset (a no-op when nothing was deferred): under the kernel */
	if (dbg) {
		const auto t4 = std::chrono::steady_clock::now();
		auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point c) { return std::chrono::duration<double, std::micro>(c - a).count(); };
		static double a1 = 0, a2 = 0, a3 = 0, a4 = 0; static int n = 0;
		a1 += us(t0, t1); a2 += us(t1, t2); a3 += us(t2, t3); a4 += us(t3, t4);
		if (++n % 100 == 0) { std::fprintf(stderr, "[grid_reinit] flush + checks %.1f us, set_corners (deferred) %.1f, init_template_fused (launch) %.1f, deferred host half %.1f (mean of 100)\n", a1 / 100, a2 / 100, a3 / 100, a4 / 100); a1 = a2 = a3 = a4 = 0; }
	}
	/* (init_template_fused took the template corners from the mirrors, which the deferred half has only now brought up to date) */
	for (int t = 0; t < b->B; ++t) std::memcpy(&b->template_corners[8 * t], b->th[t].init_corners, sizeof(double) * 8);
	b->warps_dirty = true;   /* the device slab still holds the previous frame's warps: whoever needs them next uploads the (identity) mirrors */
	/* ... except the one-launch loop kernels, which start a freshly re-initialised patch from init_corners_hm (TrackState::fresh_reset) */
	b->fresh_reinit = rc == MTFHIP_OK && !(std::getenv("MTFHIP_GRID_FRESH") && std::getenv("MTFHIP_GRID_FRESH")[0] == '0');
	if (rc == MTFHIP_OK) { HIP_TRY(hipEventRecord(b->ev_a, b->ctx->stream)); b->stage_a_busy = true; }   /* the kernel reads the staging buffer */
	return rc;
}

/* GridTracker::update's patch half as ONE call (SM/src/GridTracker.cc:345-363): every patch tracker is reset to its region and
 * runs its update(); regions and corners in the reference's CornersT layout as a row-major host array sees it (2 x 4: the x row,
 * then the y row), plus the patch centroids utils::getCentroid (miscUtils.h:473-480: the mean of the four corners) hands to the
 * robust estimator.  (The layout conversion and the centroids were ~9 of the ~14 us a frame spent in the Python layer.) */
int mtfhip_grid_update(mtfhip_batch *b, const mtfhip_sm_desc *sm, const double *regions_2x4, int *n_iters, double *corners_2x4, double *centroids) {
	if (!b || !sm || !regions_2x4) return fail(MTFHIP_ERR_INVALID_ARG, "grid_update: NULL argument");
	TRY(lowdof_refuse(b, "grid_update"));
	TRY(am_refuse(b, "grid_update", AM_AT_GRID));
	const size_t B = (size_t)b->B;
	static thread_local std::vector<double> in, out;
	in.resize(8 * B); out.resize(8 * B);
	for (size_t t = 0; t < B; ++t)
		for (int q = 0; q < 4; ++q) { in[8 * t + 2 * q] = regions_2x4[8 * t + q]; in[8 * t + 2 * q + 1] = regions_2x4[8 * t + 4 + q]; }
	TRY(mtfhip_batch_track_region(b, sm, in.data(), n_iters, out.data()));
	for (size_t t = 0; t < B; ++t) {
		const double *c = &out[8 * t];
		if (corners_2x4)
			for (int q = 0; q < 4; ++q) { corners_2x4[8 * t + q] = c[2 * q]; corners_2x4[8 * t + 4 + q] = c[2 * q + 1]; }
		if (centroids) { centroids[2 * t] = (c[0] + c[2] + c[4] + c[6]) * 0.25; centroids[2 * t + 1] = (c[1] + c[3] + c[5] + c[7]) * 0.25; }
	}
	return MTFHIP_OK;
}

/* utils::getCentroid(cv::Point2f &, corners) miscUtils.h:472-480: the mean of the four corners, rounded to float */
static inline void centroid_f(float *dst, const double *c) {
	dst[0] = static_cast<float>((c[0] + c[2] + c[4] + c[6]) / 4.0);
	dst[1] = static_cast<float>((c[1] + c[3] + c[5] + c[7]) / 4.0);
}
static int grid_batch_ok(const mtfhip_batch *b, const mtfhip_grid_desc *g, const char *fn) {
	if (!b || !g) return fail(MTFHIP_ERR_INVALID_ARG, "%s: NULL argument", fn);
	TRY(lowdof_refuse(b, fn));   /* (the grid tracker's one-launch kernels solve what they accumulate: no projection) */
	TRY(am_refuse(b, fn, AM_AT_GRID));
	if (g->grid_size_x <= 0 || g->grid_size_y <= 0 || g->grid_size_x * g->grid_size_y != b->B)   /* GridTracker.cc:124-129 */
		return fail(MTFHIP_ERR_INVALID_ARG, "%s: mismatch between the grid dimensions (%d x %d) and the batch's %d patch trackers", fn, g->grid_size_x, g->grid_size_y, b->B);
	return MTFHIP_OK;
}
/* every patch tracker's update() behind a reset that may still be running (mtfhip_grid_frame without a region; the backward pass) */
static int grid_track_plain(mtfhip_batch *b, const mtfhip_sm_desc *sm, int *n_iters, double *out) {
	/* reset-every-frame mode: this call follows mtfhip_grid_reset(reinit), whose k_template_init may still be running.  The one-launch
	 * loop kernel reads nothing of that kernel's host record, so it is enqueued behind it right away (r05: the host used to wait for the
	 * record and copy 1 KB per patch first -- launch latency + 256 KB of memcpy exposed in every frame); the record is folded into the
	 * mirrors by the next call that flushes without this flag.  MTFHIP_GRID_HOLD_PULL=0: the r05 first form. */
	if (alk_sm(sm->sm)) TRY(check_sm(b, sm, "grid_frame"));   /* (mtfhip_batch_track itself serves the additive search methods: the grid frames do not) */
	const size_t B = (size_t)b->B;
	const char *e_hp = std::getenv("MTFHIP_GRID_HOLD_PULL");
	const bool hold = b->init_mirror_seq != 0 && !(e_hp && e_hp[0] == '0') && b->h_stage_b_dev && b->h_pub_dev && b->desc.am != MTFHIP_AM_MI && !sm->leven_marq &&
		iclk_one_launch(b, sm) && second_order_term(sm, b->desc.am) < 0 && ((37 * sizeof(double) * B) % 16) == 0;
	b->hold_init_pull = hold;
	const int rc = mtfhip_batch_track(b, sm, n_iters, out);
	b->hold_init_pull = false;
	return rc;
}
/* GridTracker::update's patch loop (GridTracker.cc:254-261), with the reset that preceded it folded in when a region is given */
int mtfhip_grid_frame(mtfhip_batch *b, const mtfhip_sm_desc *sm, const mtfhip_grid_desc *g, const double *region, int *n_iters, double *corners, float *centroids) {
	if (!sm) return fail(MTFHIP_ERR_INVALID_ARG, "grid_frame: NULL argument");
	TRY(grid_batch_ok(b, g, "grid_frame"));
	const size_t B = (size_t)b->B;
	static thread_local std::vector<double> out;
	static thread_local std::vector<int> iters;
	out.resize(8 * B); iters.resize(B);
	if (region) TRY(track_region_impl(b, sm, region, n_iters ? n_iters : iters.data(), out.data(), g));
	else TRY(grid_track_plain(b, sm, n_iters ? n_iters : iters.data(), out.data()));
	if (corners) std::memcpy(corners, out.data(), sizeof(double) * 8 * B);
	if (centroids) for (size_t t = 0; t < B; ++t) centroid_f(centroids + 2 * t, &out[8 * t]);
	return MTFHIP_OK;
}

/* ---- forward-backward error estimation (GridTracker.cc:186-190, 263-266, 294-343) ---- */
/* the mask half of backwardEstimation (:307-332): host arithmetic, no device */
int mtfhip_grid_fb_mask(int n, const float *prev_pts, const float *curr_pts, const float *fb_prev_pts, const mtfhip_grid_fb_desc *fb,
	unsigned char *fb_err_mask, float *prev_masked, float *curr_masked, int *n_masked) {
	if (n < 0 || !prev_pts || !curr_pts || !fb_prev_pts || !fb || !fb_err_mask || !n_masked) return fail(MTFHIP_ERR_INVALID_ARG, "grid_fb_mask: NULL argument");
	int cnt = 0;
	auto keep = [&](int id) {
		if (prev_masked) { prev_masked[2 * cnt] = prev_pts[2 * id]; prev_masked[2 * cnt + 1] = prev_pts[2 * id + 1]; }
		if (curr_masked) { curr_masked[2 * cnt] = curr_pts[2 * id]; curr_masked[2 * cnt + 1] = curr_pts[2 * id + 1]; }
		++cnt;
	};
	for (int id = 0; id < n; ++id) {
		/* cv::Point2f members: the difference is a float, the squares and their sum doubles (:309-312) */
		const float dxf = fb_prev_pts[2 * id] - prev_pts[2 * id], dyf = fb_prev_pts[2 * id + 1] - prev_pts[2 * id + 1];
		const double dx = dxf, dy = dyf;
		if (dx * dx + dy * dy > fb->fb_err_thresh) fb_err_mask[id] = 0;
		else { fb_err_mask[id] = 1; keep(id); }
	}
	if (cnt < fb->n_model_pts) {   /* :321-332: filled up in tracker order to what the estimator needs */
		for (int id = 0; id < n; ++id) {
			if (fb_err_mask[id]) continue;
			keep(id);
			fb_err_mask[id] = 1;
			if (cnt == fb->n_model_pts) break;
		}
	}
	*n_masked = cnt;
	return MTFHIP_OK;
}
/* the patch half of backwardEstimation (:295-306) for every patch tracker of the batch at once: re-initialised at its tracked location on the
 * current frame (fb_reinit), run on the PREVIOUS frame (mtfhip_image_keep_prev), centroid of where it arrives, then back on the current
 * frame and setRegion(location) */
static int grid_backward_impl(mtfhip_batch *b, const mtfhip_sm_desc *sm, const mtfhip_grid_desc *g, const mtfhip_grid_fb_desc *fb, int *n_iters, double *fb_corners,
	float *fb_prev_pts, bool restore) {
	if (!sm || !fb) return fail(MTFHIP_ERR_INVALID_ARG, "grid_backward: NULL argument");
	TRY(grid_batch_ok(b, g, "grid_backward"));
	if (!b->init_pix_vals) return fail(MTFHIP_ERR_LOGIC, "grid_backward before the patch trackers were initialised");
	mtfhip_ctx *c = b->ctx;
	if (!c->prev.data) return fail(MTFHIP_ERR_LOGIC, "grid_backward: no previous image (mtfhip_image_keep_prev)");
	if (c->prev.h != c->img.h || c->prev.w != c->img.w || c->prev.channels != c->img.channels)
		return fail(MTFHIP_ERR_INVALID_ARG, "grid_backward: the previous image is %dx%dx%d, the current one %dx%dx%d", c->prev.h, c->prev.w, c->prev.channels, c->img.h, c->img.w, c->img.channels);
	TRY(track_validate(b, sm));
	const size_t B = (size_t)b->B;
	static thread_local std::vector<double> loc, out;
	static thread_local std::vector<int> iters;
	loc.resize(8 * B); out.resize(8 * B); iters.resize(B);
	FLUSH(b);
	for (size_t t = 0; t < B; ++t) std::memcpy(&loc[8 * t], b->th[t].corners, sizeof(double) * 8);   /* tracker_location = getRegion().clone() :296 */
	if (fb->fb_reinit) {                                                                               /* tracker->initialize(tracker_location) :297-299 */
		const char *e_gf = std::getenv("MTFHIP_GRID_FUSED");
		const bool fused = !(e_gf && e_gf[0] == '0') && b->h_stage_a_dev && template_init_fused_ok(b, sm);
		if (fused) TRY(grid_reinit_fused(b, sm, loc.data()));
		else {
			TRY(mtfhip_ssm_set_corners(b, loc.data()));
			TRY(mtfhip_batch_init_template(b, sm));
		}
	}
	TRY(mtfhip_image_swap_prev(c));                                                                    /* tracker->setImage(prev_img) :300 */
	const int rc = grid_track_plain(b, sm, n_iters ? n_iters : iters.data(), out.data());              /* tracker->update() :301 */
	const int rs = mtfhip_image_swap_prev(c);                                                          /* tracker->setImage(curr_img) :304 */
	if (rc != MTFHIP_OK) return rc;
	if (rs != MTFHIP_OK) return rs;
	if (fb_corners) std::memcpy(fb_corners, out.data(), sizeof(double) * 8 * B);
	if (fb_prev_pts) for (size_t t = 0; t < B; ++t) centroid_f(fb_prev_pts + 2 * t, &out[8 * t]);      /* getCentroid(fb_prev_pts[id], getRegion()) :302 */
	if (!restore) return MTFHIP_OK;
	return mtfhip_batch_set_region(b, loc.data(), sm);                                                 /* tracker->setRegion(tracker_location) :305 */
}
int mtfhip_grid_backward(mtfhip_batch *b, const mtfhip_sm_desc *sm, const mtfhip_grid_desc *g, const mtfhip_grid_fb_desc *fb, int *n_iters, double *fb_corners,
	float *fb_prev_pts) {
	return grid_backward_impl(b, sm, g, fb, n_iters, fb_corners, fb_prev_pts, true);
}
/* GridTracker::update's patch loop followed by backwardEstimation (:254-266): mtfhip_grid_frame, mtfhip_grid_backward and the mask in one call */
int mtfhip_grid_frame_fb(mtfhip_batch *b, const mtfhip_sm_desc *sm, const mtfhip_grid_desc *g, const mtfhip_grid_fb_desc *fb, const double *region,
	const float *prev_pts, int *n_iters, double *corners, float *centroids, float *fb_prev_pts, unsigned char *fb_err_mask, float *prev_masked, float *curr_masked,
	int *n_masked) {
	if (!fb || !prev_pts || !fb_prev_pts || !fb_err_mask || !n_masked) return fail(MTFHIP_ERR_INVALID_ARG, "grid_frame_fb: NULL argument");
	if (!(fb->fb_err_thresh > 0)) return fail(MTFHIP_ERR_INVALID_ARG, "grid_frame_fb: fb_err_thresh must be positive (GridTracker.cc:186: the estimation is off otherwise; use mtfhip_grid_frame)");
	TRY(grid_batch_ok(b, g, "grid_frame_fb"));
	static thread_local std::vector<float> cen;
	cen.resize(2 * (size_t)b->B);
	static const bool always_restore = std::getenv("MTFHIP_GRID_FB_RESTORE") && std::getenv("MTFHIP_GRID_FB_RESTORE")[0] == '1';
	/* The shipped configuration (reset_at_each_frame 1, fb_reinit 1; Config/modules.cfg:80-82) in ONE launch: k_grid_fb runs a patch's update(), its
	 * initialize(tracker_location) and its update() on the previous frame back to back in the patch's workgroup and leaves the trackers as the
	 * forward pass left them -- the caller's resetTrackers(reinit) (:273-274) re-initialises them next.  Tolerance mode, ICLK with a constant
	 * Hessian over SSD / NCC, an affine patch SSM (a tracked patch stays a parallelogram: a unit-z lattice), <= 1024 pixels.  MTFHIP_GRID_FB_FUSED=0:
	 * the three launches. */
	{
		const char *e_ff = std::getenv("MTFHIP_GRID_FB_FUSED");   /* (read per call: the tests compare the two forms in one process) */
		mtfhip_ctx *c = b->ctx;
		const bool reinit_ok = !fb->fb_reinit || (b->desc.ssm == MTFHIP_SSM_AFFINE && template_init_fused_ok(b, sm));   /* (fb_reinit 0: the backward loop keeps the forward pass's template and state) */
		/* reset_at_each_frame 1: the caller's reset follows, nothing to restore.  0 without fb_reinit: the template is untouched, setRegion(tracker_location)
		 * (:305) is one more call behind the launch.  (0 with fb_reinit would have to keep the backward template: the launch-by-launch form.) */
		const bool restore_after = g->reset_at_each_frame == 0 && !fb->fb_reinit;
		const bool fused = !(e_ff && e_ff[0] == '0') && !region && reinit_ok && (g->reset_at_each_frame == 1 || restore_after) && !always_restore &&
			b->math_mode == MTFHIP_MATH_FAST && (b->desc.am == MTFHIP_AM_SSD || b->desc.am == MTFHIP_AM_NCC) && b->C == 1 && sm->sm == MTFHIP_SM_ICLK && iclk_one_launch(b, sm) && !sm->leven_marq &&
			second_order_term(sm, b->desc.am) < 0 && b->N <= 4 * kBlock && b->h_pub_dev && !b->d_trace && b->init_pix_vals &&
			(b->desc.am != MTFHIP_AM_NCC || b->d_ncc_tm) && c->prev.data && c->img.data && c->prev.h == c->img.h && c->prev.w == c->img.w &&
			c->prev.channels == c->img.channels;
		if (fused) {
			const size_t B = (size_t)b->B;
			if (!b->d_fb) {   /* (the last of the three to arrive: while it is null a failed call is simply repeated) */
				HIP_TRY(b->h_fb.reserve(9 * B));
				HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&b->h_fb_dev), b->h_fb, 0));
				HIP_TRY(b->d_fb.reserve(9 * B));
			}
			b->fb_fused_req = true; b->fb_fused_reinit = fb->fb_reinit != 0;
			const int rc = mtfhip_grid_frame(b, sm, g, nullptr, n_iters, corners, cen.data());
			b->fb_fused_req = false;
			if (rc != MTFHIP_OK) return rc;
			if (centroids) std::memcpy(centroids, cen.data(), sizeof(float) * cen.size());
			for (size_t t = 0; t < B; ++t) {
				if (b->h_fb[9 * t + 8] < 0) return fail(MTFHIP_ERR_INVALID_ARG, "grid_frame_fb: degenerate tracked corners for patch %d", (int)t);
				centroid_f(fb_prev_pts + 2 * t, b->h_fb + 9 * t);                                        /* getCentroid(fb_prev_pts[id], getRegion()) :302 */
			}
			if (restore_after) {                                                                           /* tracker->setRegion(tracker_location) :305 */
				static thread_local std::vector<double> loc;
				loc.resize(8 * B);
				for (size_t t = 0; t < B; ++t) std::memcpy(&loc[8 * t], b->th[t].corners, sizeof(double) * 8);   /* (the forward pass's: what the kernel left) */
				TRY(mtfhip_batch_set_region(b, loc.data(), sm));
			}
			return mtfhip_grid_fb_mask(b->B, prev_pts, cen.data(), fb_prev_pts, fb, fb_err_mask, prev_masked, curr_masked, n_masked);
		}
	}
	TRY(mtfhip_grid_frame(b, sm, g, region, n_iters, corners, cen.data()));
	if (centroids) std::memcpy(centroids, cen.data(), sizeof(float) * cen.size());
	/* GridTracker::update goes on to resetTrackers when reset_at_each_frame != 0 (:273-274): every patch tracker is then initialize()d or
	 * setRegion()ed on the new grid, which replaces all that setRegion(tracker_location) (:305) would leave -- the SSM's state; with fb_reinit
	 * the template is the backward pass's either way -- so that call is left out here (MTFHIP_GRID_FB_RESTORE=1 keeps it) */
	TRY(grid_backward_impl(b, sm, g, fb, nullptr, nullptr, fb_prev_pts, always_restore || g->reset_at_each_frame == 0));
	return mtfhip_grid_fb_mask(b->B, prev_pts, cen.data(), fb_prev_pts, fb, fb_err_mask, prev_masked, curr_masked, n_masked);
}
/* GridTracker::resetTrackers(reinit) GridTracker.cc:345-392 */
int mtfhip_grid_reset(mtfhip_batch *b, const mtfhip_sm_desc *sm, const mtfhip_grid_desc *g, const double *region, int reinit, double *patch_corners, float *prev_pts) {
	if (!sm || !region) return fail(MTFHIP_ERR_INVALID_ARG, "grid_reset: NULL argument");
	TRY(grid_batch_ok(b, g, "grid_reset"));
	if (alk_sm(sm->sm)) TRY(check_sm(b, sm, "grid_reset"));   /* (before anything is laid out: an additive search method has no grid frame) */
	const size_t B = (size_t)b->B;
	static thread_local std::vector<double> patches;
	patches.resize(8 * B);
	const char *e_gf = std::getenv("MTFHIP_GRID_FUSED"), *e_ld = std::getenv("MTFHIP_GRID_LAYOUT_DEV");
	const bool fused = reinit && !(e_gf && e_gf[0] == '0') && b->h_stage_a_dev && template_init_fused_ok(b, sm);
	/* fixed-size patches of an affine patch SSM: k_template_init lays its patch out itself and the host layout runs behind the launch */
	const bool layout_later = fused && b->desc.ssm != MTFHIP_SSM_HOMOGRAPHY && !g->dyn_patch_size && !(e_ld && e_ld[0] == '0');
	if (layout_later) {
		M3 Wr;
		if (!rect_to_quad(-0.5, -0.5, 0.5, 0.5, region, Wr)) return fail(MTFHIP_ERR_INVALID_ARG, "grid_layout: degenerate region corners");
		b->deferred_gdesc = *g;
		std::memcpy(b->deferred_region, region, sizeof(b->deferred_region));
		std::memcpy(b->deferred_region_map, Wr.m, sizeof(b->deferred_region_map));
		const int rc = grid_reinit_fused(b, sm, nullptr, true);
		if (rc != MTFHIP_OK) { b->deferred_layout = false; return rc; }
		if (b->deferred_patches.size() != 8 * B) return fail(MTFHIP_ERR_LOGIC, "grid_reset: the deferred layout did not run");
		std::memcpy(patches.data(), b->deferred_patches.data(), sizeof(double) * 8 * B);
	} else {
		TRY(mtfhip_grid_layout(g, region, nullptr, patches.data()));
		if (!reinit) TRY(mtfhip_batch_set_region(b, patches.data(), sm));   /* tracker->setRegion(patch_corners) */
		else if (fused) TRY(grid_reinit_fused(b, sm, patches.data()));       /* tracker->initialize(patch_corners): NT/ICLK.cc:71-128 etc. */
		else {
			TRY(mtfhip_ssm_set_corners(b, patches.data()));
			TRY(mtfhip_batch_init_template(b, sm));
		}
	}
	if (patch_corners) std::memcpy(patch_corners, patches.data(), sizeof(double) * 8 * B);
	/* :387 getCentroid(prev_pts[id], tracker->getRegion()): both resets leave the tracker's region = the patch corners */
	if (prev_pts) for (size_t t = 0; t < B; ++t) centroid_f(prev_pts + 2 * t, &patches[8 * t]);
	return MTFHIP_OK;
}

} /* extern "C" */
