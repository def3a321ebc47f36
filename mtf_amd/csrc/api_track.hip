/*
 * api_track.hip -- the device-side loop: the skeleton every loop shares (slab upload, Levenberg-Marquardt state, flag poll, read-back), track_core and
 * its one-launch, persistent and chunked drivers, mtfhip_batch_track / _track_region, the debug trace and the two query entry points
 * (C-ABI implementation, include/mtfhip.h; shared declarations: mtfhip_api_internal.h; no CPU fallback: HIP kernels or an error)
 */
#include "mtfhip_api_internal.h"

extern "C" {

/* active = 1, iters = 0, corners, warps, states, NCC scalars (unless keep_ncc): one pinned async copy of the whole slab (w0 is copied along:
 * init_grid consumed it long ago).  h_stage_b needs no guard: every return path of a loop has waited for its results, i.e. the stream has drained or
 * -- the chunked loop's in-loop delivery -- all B targets have arrived, so the head of the call, which reads the buffer, has run. */
/* lw (the chunked driver's fused head, track_core): the same launch also sets the loop's words (k_track_prologue); the copy fallback -- no host-visible
 * staging buffer -- keeps its copy and sets them with that kernel behind it */
int loop_upload_slab(mtfhip_batch *b, hipStream_t st, bool keep_ncc, const LoopWords *lw) {
	const size_t Bt = (size_t)b->B;
	std::memcpy(b->h_stage_b + 45 * sizeof(double) * Bt, b->h_stage_a + 45 * sizeof(double) * Bt, 9 * sizeof(double) * Bt);
	fill_stage(b, b->h_stage_b, nullptr, 1, true);
	const size_t skip_off = keep_ncc ? 37 * sizeof(double) * Bt : 0, skip_len = keep_ncc ? 8 * sizeof(double) * Bt : 0;
	if (b->h_stage_b_dev && lw) { TimedScope tsc(b->ctx, "track_prologue", st); launch_track_prologue(b->h_stage_b_dev, b->d_slab, b->slab_bytes, skip_off, skip_len, *lw, st); }
	else if (b->h_stage_b_dev) launch_ingest_host(b->h_stage_b_dev, b->d_slab, b->slab_bytes, st, skip_off, skip_len);
	else if (keep_ncc) return fail(MTFHIP_ERR_LOGIC, "track: a held template-initialisation record needs the host-visible staging buffer");
	else {
		HIP_TRY(hipMemcpyAsync(b->d_slab, b->h_stage_b, b->slab_bytes, hipMemcpyHostToDevice, st));
		if (lw) { TimedScope tsc(b->ctx, "track_prologue", st); launch_track_prologue(nullptr, nullptr, 0, 0, 0, *lw, st); }
	}
	b->warps_dirty = false;   /* the slab carries the warps */
	return MTFHIP_OK;
}
/* per-target LM state: prev_similarity 0, leven_marq_delta = lm_delta_init, no pending reset, iteration 0 */
int loop_lm_state(mtfhip_batch *b, const mtfhip_sm_desc *sm, hipStream_t st, double **lm) {
	HIP_TRY(b->d_lm.reserve(kLmStride * (size_t)b->B));
	std::vector<double> lm0((size_t)kLmStride * b->B, 0.0);
	for (int t = 0; t < b->B; ++t) lm0[(size_t)kLmStride * t + 1] = sm->lm_delta_init;
	HIP_TRY(hipMemcpyAsync(b->d_lm, lm0.data(), sizeof(double) * lm0.size(), hipMemcpyHostToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));   /* lm0 is a stack-lifetime buffer */
	*lm = b->d_lm;
	return MTFHIP_OK;
}
/* A loop is enqueued without waiting for the device, so passes after the last target has stopped would still be launched (a few microseconds
 * each).  With a reachable convergence test the flags are looked at every eighth pass: one small copy + sync against up to seven idle passes.
 * A copy that fails: track_core's drivers take it as "not stopped" (err == NULL), alk_track makes it the call's error -- kept as they were. */
bool loop_all_stopped(const mtfhip_sm_desc *sm, int max_passes, int it, const int *d_flags, int n, hipStream_t on, std::vector<int> &h_flags, hipError_t *err) {
	if (!(sm->epsilon > 0) || (it + 1) % 8 != 0 || it + 1 >= max_passes) return false;
	h_flags.resize(n);
	hipError_t e = hipMemcpyAsync(h_flags.data(), d_flags, sizeof(int) * n, hipMemcpyDeviceToHost, on);
	if (e == hipSuccess) e = hipStreamSynchronize(on);
	if (e != hipSuccess) { if (err) *err = e; return false; }
	for (int v : h_flags) if (v) return false;
	return true;
}
/* the slab comes back through a kernel that writes it into host-coherent memory and raises a flag the host spins on -- the loop's own (pub_seq)
 * or k_publish_host -- or as one copy + one sync (MTFHIP_ZERO_COPY=0); then into the mirrors and the caller's arrays.  *h_res: the slab as read */
int loop_read_back(mtfhip_batch *b, hipStream_t st, unsigned long long pub_seq, int *n_iters, double *corners, const char **h_res) {
	*h_res = b->h_pub;
	if (pub_seq) TRY(wait_host_flag(b, pub_seq));
	else if (b->h_pub_dev) {
		const unsigned long long seq = ++b->acc_seq;
		{ TimedScope tsc(b->ctx, "publish_host", st); launch_publish_host(b->d_slab, b->h_pub_dev, b->slab_bytes, b->d_fin_count, b->h_flag_dev, seq, st); }
		TRY(wait_host_flag(b, seq));
	} else {
		HIP_TRY(hipMemcpyAsync(b->h_stage_b, b->d_slab, b->slab_bytes, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		*h_res = b->h_stage_b;
	}
	const size_t Bt = (size_t)b->B;
	const double *p = reinterpret_cast<const double *>(*h_res);
	const double *w = p, *s = p + 9 * Bt, *cr = p + 17 * Bt;
	const int *iters = reinterpret_cast<const int *>(*h_res + b->slab_dbl_bytes) + Bt;
	for (int t = 0; t < b->B; ++t) {
		std::memcpy(b->th[t].warp.m, w + 9 * t, sizeof(double) * 9);
		/* (a low-order SSM's slab holds the affine embedding of the warp: its own state is getStateFromWarp of the warp, as its
		 * compositionalUpdate leaves it -- Similitude.cc:111-121, Isometry.cc:56-66; Translation's state is the warp's last column) */
		if (b->lo_ssm) state_from_warp(b->lo_ssm, b->th[t].state, b->th[t].warp);
		else std::memcpy(b->th[t].state, s + 8 * t, sizeof(double) * 8);
		std::memcpy(b->th[t].corners, cr + 8 * t, sizeof(double) * 8);
		if (n_iters) n_iters[t] = iters[t];
		if (corners) std::memcpy(corners + 8 * t, cr + 8 * t, sizeof(double) * 8);
	}
	return MTFHIP_OK;
}
/* the one-launch grid kernel (k_iclk_track: a patch's whole ICLK update() in one workgroup) takes ICLK with a constant Hessian -- up to
 * four pixels per thread, where every per-pixel operand of the loop stays in registers: 3.1-4.4 us per iteration at 25 x 25 and
 * 32 x 32 against 8.8-12 for a launch per pass.  Above that the template Jacobian is re-read in every iteration and the kernel
 * falls behind the launch-per-pass loop (40 x 40: 11.3-16.9 against 9.9-13.7 us; 50 x 50 x 256: 35.3 against 14.9;
 * profiles/r03_experiments.md), so larger patches take that loop.  MTFHIP_ICLK_ONE_LAUNCH_MAX moves the boundary (experiments). */
static int iclk_one_launch_max_pix() {
	static const int v = std::getenv("MTFHIP_ICLK_ONE_LAUNCH_MAX") ? std::atoi(std::getenv("MTFHIP_ICLK_ONE_LAUNCH_MAX")) : 4 * kBlock;
	return v < kIclkTrackMaxPix ? v : kIclkTrackMaxPix;
}
bool iclk_one_launch(const mtfhip_batch *b, const mtfhip_sm_desc *sm) {
	/* (SCV re-maps its template, RSCV rebuilds its map between the passes: they take the fused launch + finish per pass) */
	/* (a low-order SSM takes the two-launch loop, whose finish projects the affine system: the one-launch kernels solve what they accumulate) */
	/* (SPSS: the one-launch kernels accumulate SSD's or NCC's sums; SSIM: NCC's sums, but they solve NCC's system) */
	return b->C == 1 && !b->lo_ssm && !loop_only(b) && sm->sm == MTFHIP_SM_ICLK && (sm->hess_type == 0 || (sm->hess_type == 2 && b->desc.am == MTFHIP_AM_SSD)) &&
		b->N <= iclk_one_launch_max_pix();
}

/* Targets per launch of the device-side loop.  Chunking pays where an iteration both re-reads a large constant operand
 * set and writes as much again (ESM with materialisation: 88 B/px read, 88 B/px written): +15-17 % at B = 128-256.
 * FCLK reads only 24 B/px (fits anyway) and the lean / ICLK variants barely write, so for them a chunk only multiplies
 * the per-iteration finish launches (measured 7-20 % slower) and they keep one launch for all targets.
 * MTFHIP_TRACK_CHUNK_PX overrides the pixel budget (tests force tiny chunks with it, in every mode). */
static int track_chunk(const mtfhip_batch *b, const mtfhip_sm_desc *sm, const FusedArgs &fa) {
	const char *env_px = std::getenv("MTFHIP_TRACK_CHUNK_PX");
	if (!env_px && !(fa.mode == 1 && fa.materialize)) return b->B;
	const double chunk_px = env_px ? std::atof(env_px) : 2.6e6;
	int chunk = (int)(chunk_px / (double)b->N);
	if (chunk < 1) chunk = 1;
	if (chunk >= b->B || sm->max_iters == 1) return b->B;
	const int n_chunks = (b->B + chunk - 1) / chunk;
	return (b->B + n_chunks - 1) / n_chunks;   /* balanced: 100 targets -> 50 + 50, not 65 + 35 */
}
/* Queues of the device-side loop.  Two for the launches that materialise the interface arrays (HBM-bound: ESM / FCLK full mode, NCC,
 * the multi-channel models): the solve + update of one chunk of targets -- one-wave workgroups, a 6.5 us chain of dependent
 * latencies -- and the fill / drain of its pixel pass then run under the other chunk's pixel pass.  Measured at 200 x 200 x 64 (one
 * call): 61.5 -> 49-52 us per step in calls of >= 100 iterations, 64.5 -> 59-63 at 20; the lean / ICLK launches (issue-bound) gain
 * 0-4 %, small patches lose (50 x 50: -7 %): they keep one queue.  MTFHIP_TRACK_STREAMS=1 selects the single queue, 3 / 4 more
 * queues (measured slower), 12 two queues for every launch kind (A/B knob). */
static int track_queues(const mtfhip_batch *b, const FusedArgs &fa) {
	const char *e_want = std::getenv("MTFHIP_TRACK_STREAMS");   /* (read per call: the tests switch it) */
	const int want = e_want ? std::atoi(e_want) : 2;
	if (want < 2 || b->B < 2 || b->d_trace) return 1;
	/* launches that write nothing are issue-bound: ESM's lean pass gains 3-6 % in 200-iteration calls and loses 4-5 % in 20-iteration
	 * ones, FCLK's and ICLK's gain nothing */
	if (!fa.materialize && want < 12) return 1;
	/* small passes are launch- and latency-sized, not bandwidth-sized: 8 x 200 x 200 and 64 x 50 x 50 measured 5-14 % slower on two queues
	 * in 20-iteration calls, 16 / 32 / 48 x 200 x 200 6-22 % faster */
	static const double min_rows = std::getenv("MTFHIP_TRACK_STREAMS_MIN_ROWS") ? std::atof(std::getenv("MTFHIP_TRACK_STREAMS_MIN_ROWS")) : 0.5e6;
	if ((double)b->B * b->N < min_rows && want < 12) return 1;
	return std::min(std::min(want % 10, 4), b->B);
}
int mtfhip_batch_track_targets_per_launch(mtfhip_batch *b, const mtfhip_sm_desc *sm) {
	FLUSH(b);
	if (check_sm(b, sm, "track_targets_per_launch") != MTFHIP_OK) return 0;
	if (iclk_one_launch(b, sm)) return b->B;
	FusedArgs fa;
	if (fused_args(b, sm, fa) != MTFHIP_OK) return 0;
	const int chunk = track_chunk(b, sm, fa), nq = track_queues(b, fa);
	return nq >= 2 ? std::min(chunk, (b->B + nq - 1) / nq) : chunk;
}
int mtfhip_batch_track_queues(mtfhip_batch *b, const mtfhip_sm_desc *sm) {
	FLUSH(b);
	if (check_sm(b, sm, "track_queues") != MTFHIP_OK) return 0;
	if (hist_am(b)) return 1;
	if (iclk_one_launch(b, sm)) return 1;
	FusedArgs fa;
	if (fused_args(b, sm, fa) != MTFHIP_OK) return 0;
	return track_queues(b, fa);
}

/* Deferred materialisation of the two-launch loop.  A materialising pass stores It, dIt_dx and Jt (88 B/px) that the next pass overwrites
 * and nothing in between reads: only what a target's last executed pass wrote can be seen after the call.  Where this predicate holds, the
 * passes before the one the host knows to be the last run the non-materialising kernel in the same (replay) arithmetic on the same cut of
 * the pixel pass -- the same partial rows, so H, g, the update, the corners and n_iters are the parent loop's bits -- the last pass
 * materialises as before, and a target the finish stops earlier (change < epsilon) gets one trailing materialising launch at the warp of
 * its last pass (TrackState::warp_last / need_mat).  MTFHIP_TRACK_DEFER_MAT=0 (read per call) keeps every pass materialising. */
static bool track_defers_materialisation(const mtfhip_batch *b, const mtfhip_sm_desc *sm, const FusedArgs &fa, int so_term, bool resume, bool use_step) {
	const char *e = std::getenv("MTFHIP_TRACK_DEFER_MAT");   /* (read per call: the tests and the A/B measurement flip it) */
	if (e && e[0] == '0') return false;
	if (!fa.materialize) return false;          /* nothing is stored that could be deferred */
	if (fa.mode == 2) return false;             /* ICLK stores It only (8 B/px): a trailing launch would cost more than it saves */
	if (sm->max_iters < 3) return false;        /* one or two passes: a lean pass + a trailing pass can cost more than the stores saved */
	if (sm->leven_marq) return false;           /* an undo pass, FCLK's 2 x max_iters passes: the host does not know the last pass, and the
	                                             * finish also stops a target on a counter of its own */
	if (b->d_trace) return false;               /* the debug trace is compared pass by pass against loops that materialise every pass */
	if (so_term >= 0) return false;             /* the second-order pass runs between the pixel pass and the finish, beside the stored arrays */
	if (b->desc.am != MTFHIP_AM_SSD && b->desc.am != MTFHIP_AM_NCC) return false;   /* MI has its own loop; SCV / RSCV / LSCV / LRSCV re-map from It between the passes */
	if (b->C != 1) return false;                /* the multi-channel kernels are an instantiation set of their own: not measured */
	if (use_step) return false;                 /* the one-launch-per-pass form (MTFHIP_STEP=1) has no lean / full pair */
	if (resume) return false;                   /* the rest of a persistent launch: the iteration counters do not start at zero */
	return true;
}

static int track_core(mtfhip_batch *b, const mtfhip_sm_desc *sm, int *n_iters, double *corners, bool slab_uploaded, bool resume = false, bool region_mode = false);
/* ---- the persistent one-launch loop (kernels_persist.hip) ---- */
/* rows per workgroup so that every target's workgroups are resident together: the default decomposition when it fits, else the
 * smallest number of rows that does */
static void persist_decomposition(const mtfhip_batch *b, int &nblk, int &rows) {
	fused_decomposition(b->N, b->B, nblk, rows);
	const int per_target = b->ctx->n_cus / b->B;
	if (per_target >= 1 && nblk > per_target) {
		const int total_rows = (b->N + kBlock - 1) / kBlock;
		rows = (total_rows + per_target - 1) / per_target;
		nblk = (total_rows + rows - 1) / rows;
	}
	static const int forced = std::getenv("MTFHIP_PERSIST_NBLK") ? std::atoi(std::getenv("MTFHIP_PERSIST_NBLK")) : 0;   /* experiments */
	if (forced > 0 && forced < nblk) {
		const int total_rows = (b->N + kBlock - 1) / kBlock;
		rows = (total_rows + forced - 1) / forced;
		nblk = (total_rows + rows - 1) / rows;
	}
}
/* the arrival / barrier words of the persistent and the one-launch-per-pass kernels: zero between launches */
static int ensure_persist_words(mtfhip_batch *b, hipStream_t st) {
	if (b->d_persist) return MTFHIP_OK;
	HIP_TRY(b->d_persist.reserve(2 * (size_t)b->B));
	const hipError_t e = hipMemsetAsync(b->d_persist, 0, 2 * sizeof(int) * (size_t)b->B, st);
	if (e != hipSuccess) b->d_persist.reset();   /* (not zeroed is not there: the next call starts over) */
	HIP_TRY(e);
	return MTFHIP_OK;
}
static unsigned long long persist_timeout_ticks() {   /* 100 MHz ticks; MTFHIP_PERSIST_TIMEOUT_US for tests (default 20 ms) */
	const char *e = std::getenv("MTFHIP_PERSIST_TIMEOUT_US");
	const double us = e ? std::atof(e) : 20000.0;
	return (unsigned long long)(us * 100.0);
}
/* Opt-in (MTFHIP_PERSIST=1).  Measured on MI355X (profiles/README.md, r02): a hand-over between workgroups through memory costs what
 * the gap between two dependent launches costs (~2 us), so one launch per loop does not beat two launches per iteration --
 * 200 x 200 x 1: 17.1 us per iteration against 13.0, 50 x 50 x 1: 12.3 against 12.3 -- and the per-iteration time is the solve's
 * latency either way. */
static bool persist_fits(const mtfhip_batch *b, const mtfhip_sm_desc *sm, const FusedArgs &fa) {
	const char *e = std::getenv("MTFHIP_PERSIST");
	if (!(e && e[0] == '1') || !b->persist_ok || fa.materialize || b->ctx->n_cus <= 0 || b->B > b->ctx->n_cus || !b->h_pub_dev) return false;
	if (b->C != 1) return false;   /* (no multi-channel instantiation of the persistent kernel) */
	if (b->lo_ssm) return false;   /* (the low-order SSMs are served by the two-launch loop only) */
	if (loop_only(b)) return false;   /* (the SCV family: a re-map runs between the passes; SPSS; SSIM: NCC's pass, but its own finish) */
	if (b->B > 8) return false;   /* a batch is better served by its own decomposition (eight workgroups per target) */
	if (sm->max_iters < 2) return false;
	int nblk, rows;
	persist_decomposition(b, nblk, rows);
	return (long)nblk * b->B <= b->ctx->n_cus && nblk <= b->nblk_max;
}
/* LSCV / LRSCV: update() sets first_iter in front of its loop and every completed iteration clears it (NT/ESM.cc:178, :291): the device
 * loop maps in front of its first pass (track_core) and leaves the batch's flag clear */
static int lscv_after_track(mtfhip_batch *b, int rc) {
	if (rc == MTFHIP_OK && b && imap_localized(b)) b->first_iter = 0;
	return rc;
}
int mtfhip_batch_track(mtfhip_batch *b, const mtfhip_sm_desc *sm, int *n_iters, double *corners) {
	TRY(lowdof_sm_refuse(b, sm, "track"));
	if (sm && alk_sm(sm->sm)) return alk_track(b, sm, n_iters, corners);
	return lscv_after_track(b, track_core(b, sm, n_iters, corners, false));
}

/* setRegion + update of one frame in one call: what GridTracker::update does with every patch tracker (GridTracker.cc:345-363:
 * tracker->setRegion(patch corners); tracker->update()) and a pyramid level with the level above's result.  For the search
 * methods that keep their template Jacobian (ICLK; FCLK without the InitialSelf Hessian) the reset state and the loop's
 * active flags / iteration counts travel in ONE staged copy; the others take the two steps one after the other. */
/* MTFHIP_TRACK_DEBUG_TIMING: host-side stamps of a one-launch frame (before the launch call | after it | after the deferred host half) */
const bool g_track_dbg_timing = std::getenv("MTFHIP_TRACK_DEBUG_TIMING") != nullptr;
static thread_local std::chrono::steady_clock::time_point g_track_dbg_t[3];
/* grid != NULL (mtfhip_grid_frame): region_corners is the GRID's region (8 doubles) and the patches are laid over it -- by the kernel
 * itself where the one-launch region mode applies and the patches are fixed-size rectangles (the host layout then runs behind the launch),
 * by mtfhip_grid_layout in front of the call otherwise */
int track_region_impl(mtfhip_batch *b, const mtfhip_sm_desc *sm, const double *region_corners, int *n_iters, double *corners, const mtfhip_grid_desc *grid) {
	if (!b || !sm || !region_corners) return fail(MTFHIP_ERR_INVALID_ARG, "track_region: NULL argument");
	/* everything track_core would refuse is refused before the SSM is reset (the folded upload reads the pinned staging buffer
	 * without an event guard: the loop that follows is what the host waits for) */
	TRY(track_validate(b, sm));
	const bool folded = !region_refreshes(sm);
	const bool dbg = g_track_dbg_timing;
	/* r04: in front of the one-launch ICLK kernel (the grid tracker's patches) the reset needs no launch of its own -- every workgroup
	 * ingests its patch's corners from the pinned staging buffer and lays out its own grid (RegionIngest, k_iclk_track).
	 * MTFHIP_GRID_FUSED=0 keeps the ingest + k_init_grid launch in front of the loop (A/B, and the bit-identity test). */
	const char *e_gf = std::getenv("MTFHIP_GRID_FUSED");   /* (read per call: the A/B test flips it) */
	const bool fused_ok = !(e_gf && e_gf[0] == '0');
	const bool region_mode = fused_ok && folded && !hist_am(b) && !sm->leven_marq && iclk_one_launch(b, sm) && second_order_term(sm, b->desc.am) < 0 &&
		b->h_stage_a_dev && b->h_pub_dev;
	const auto t0 = std::chrono::steady_clock::now();
	static thread_local std::vector<double> patches;
	bool layout_later = false;
	if (grid) {
		const char *e_ld = std::getenv("MTFHIP_GRID_LAYOUT_DEV");   /* (=0: the host lays the patches out in front of the launch, the r05 first form) */
		layout_later = region_mode && b->desc.ssm != MTFHIP_SSM_HOMOGRAPHY && !grid->dyn_patch_size && !(e_ld && e_ld[0] == '0');
		if (layout_later) {
			M3 Wr;
			if (!rect_to_quad(-0.5, -0.5, 0.5, 0.5, region_corners, Wr)) return fail(MTFHIP_ERR_INVALID_ARG, "grid_layout: degenerate region corners");
			b->deferred_gdesc = *grid;
			std::memcpy(b->deferred_region, region_corners, sizeof(b->deferred_region));
			std::memcpy(b->deferred_region_map, Wr.m, sizeof(b->deferred_region_map));
		} else {
			patches.resize(8 * (size_t)b->B);
			TRY(mtfhip_grid_layout(grid, region_corners, nullptr, patches.data()));
			region_corners = patches.data();
		}
	}
	{
		const int rs = set_region_core(b, layout_later ? nullptr : region_corners, sm, folded, region_mode, layout_later);
		if (rs != MTFHIP_OK) { b->deferred_layout = false; b->deferred_template_check = false; set_corners_finish_deferred(b); return rs; }
	}
	const auto t1 = std::chrono::steady_clock::now();
	const int r = lscv_after_track(b, track_core(b, sm, n_iters, corners, folded, false, region_mode));
	set_corners_finish_deferred(b);   /* (a call that failed before its launch: nothing stays pending on the caller's buffer) */
	if (dbg) {
		const auto t2 = std::chrono::steady_clock::now();
		static double acc1 = 0, acc2 = 0, acc3 = 0, acc4 = 0, acc5 = 0, acc6 = 0; static int n = 0;
		auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point c) { return std::chrono::duration<double, std::micro>(c - a).count(); };
		acc1 += us(t0, t1); acc2 += us(t1, t2); acc3 += us(t1, g_track_dbg_t[0]); acc4 += us(g_track_dbg_t[0], g_track_dbg_t[1]); acc5 += us(g_track_dbg_t[1], g_track_dbg_t[2]); acc6 += us(g_track_dbg_t[2], t2);
		if (++n % 100 == 0) {
			std::fprintf(stderr, "[track_region] set_region %.1f us, track %.1f us = before the launch %.1f + launch call %.1f + deferred host half %.1f + wait and copy-out %.1f (mean of 100)\n",
				acc1 / 100, acc2 / 100, acc3 / 100, acc4 / 100, acc5 / 100, acc6 / 100);
			acc1 = acc2 = acc3 = acc4 = acc5 = acc6 = 0;
		}
	}
	return r;
}
int mtfhip_batch_track_region(mtfhip_batch *b, const mtfhip_sm_desc *sm, const double *region_corners, int *n_iters, double *corners) {
	return track_region_impl(b, sm, region_corners, n_iters, corners, nullptr);
}

/* the argument / state checks of the device loop, without side effects (track_region runs them before it resets the SSM) */
int track_validate(mtfhip_batch *b, const mtfhip_sm_desc *sm) {
	TRY(check_sm(b, sm, "track"));
	if (sm->max_iters <= 0) return fail(MTFHIP_ERR_INVALID_ARG, "track: max_iters must be positive");
	const int so_term = second_order_term(sm, b->desc.am);
	if (b->desc.am == MTFHIP_AM_MI && so_term >= 0 && b->desc.mi_n_bins != 8)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "track: second-order MI Hessians with other than 8 bins go through the per-function entry points");
	if (so_term >= 0 && b->C != 1) return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "track: second-order Hessians of the multi-channel models use the per-function entry points");
	if (so_term > 0 && so_term != 4 && !b->init_pix_hess) return fail(MTFHIP_ERR_LOGIC, "track: init_template was run without sec_ord_hess");
	if (!b->init_pix_vals) return fail(MTFHIP_ERR_LOGIC, "track before init_template");
	/* (a rejected Levenberg-Marquardt step of FCLK repeats a pass within one iteration of its while loop: the passes do not tell which
	 * iteration is the first) */
	if (imap_localized(b) && b->imap.once && sm->leven_marq && sm->sm == MTFHIP_SM_FCLK)
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "track: %s once_per_frame with Levenberg-Marquardt FCLK is not available on the device loop (use the per-function entry points)",
			intensity_mapped_name(b));
	return need_image(b);
}
/* track_core's drivers.  ICLK with a constant Hessian on small patches: a patch's whole update() in one workgroup of ONE launch (k_iclk_track), which
 * also delivers the slab to the host (pub_seq) and in region mode ingests the staged corners of the setRegion; fb_fused_req: k_grid_fb */
static int track_loop_one_launch(mtfhip_batch *b, const mtfhip_sm_desc *sm, const TrackState &ts, const TrackCtx &cx, unsigned long long &pub_seq) {
	hipStream_t st = b->ctx->stream;
	const BatchView bv = b->view();
	const bool fb_fused = b->fb_fused_req;
	TimedScope tsc(b->ctx, fb_fused ? "grid_fb" : "iclk_track");
	HostPublish pub{nullptr, 0, 0, nullptr, nullptr, 0, 0};
	if (b->h_pub_dev) {
		pub_seq = ++b->acc_seq;
		pub = HostPublish{b->h_pub_dev, b->slab_dbl_bytes, b->B, b->d_fin_count, b->h_flag_dev, pub_seq, publish_fenced()};
	}
	RegionIngest rg{};
	if (cx.region_mode) {
		/* (the staging slab of set_corners_core: w 9 | s 8 | corners 8 | init_corners_hm 12 | NCC scalars 8 | w0 9 per target) */
		const double *stage = reinterpret_cast<const double *>(b->h_stage_a_dev);
		rg = region_geometry(b);
		rg.corners = stage + 17 * (size_t)b->B; rg.ncc = stage + 37 * (size_t)b->B;
		rg.d_ncc = b->d_ncc; rg.d_w0 = b->d_w0; rg.d_init_corners_hm = b->d_init_corners_hm;
		if (b->deferred_layout) region_deferred_layout(b, rg);   /* the kernel lays its patches out itself (track_region_impl) */
	}
	const bool dbg_t = g_track_dbg_timing;
	if (dbg_t) g_track_dbg_t[0] = std::chrono::steady_clock::now();
	if (fb_fused) {
		if (cx.region_mode || !pub.host) return fail(MTFHIP_ERR_LOGIC, "track: the one-launch forward-backward frame takes the plain mode with a host record");
		/* (the template lattice's geometry: what grid_reinit_fused hands k_template_init) */
		if (!launch_grid_fb(bv, b->ctx->img, b->ctx->prev, *sm, ts, b->d_h0inv, b->d_ncc, b->norm_mult, b->norm_add, b->desc.grad_eps, pub,
				GridFbOut{b->h_fb_dev, b->d_fb, b->fb_fused_reinit ? 1 : 0}, region_geometry(b), st))
			return fail(MTFHIP_ERR_LOGIC, "track: patch too large for the one-launch forward-backward frame");
	} else
		launch_iclk_track(bv, b->ctx->img, *sm, ts, b->d_h0inv, b->d_ncc, b->norm_mult, b->norm_add, b->math_mode == MTFHIP_MATH_FAST, pub, rg, st);
	if (dbg_t) g_track_dbg_t[1] = std::chrono::steady_clock::now();
	set_corners_finish_deferred(b);   /* the host half of a deferred reset, under the kernel */
	if (dbg_t) g_track_dbg_t[2] = std::chrono::steady_clock::now();
	return MTFHIP_OK;
}
/* a grid that fits the device at one workgroup per CU (a single large target, a few small ones): every pass of the loop in ONE launch, the
 * workgroups meeting at an in-kernel barrier between the pixel pass and the solve (kernels_persist.hip) */
static int track_loop_persist(mtfhip_batch *b, const mtfhip_sm_desc *sm, const FusedArgs &fa, const TrackState &ts, const TrackCtx &cx) {
	hipStream_t st = b->ctx->stream;
	TRY(ensure_persist_words(b, st));
	int nblk_p, rows_p;
	persist_decomposition(b, nblk_p, rows_p);
	FusedArgs fp = fa;
	fp.rows_per_block = rows_p;
	PersistState ps{b->d_persist, reinterpret_cast<unsigned *>(b->d_persist.get()) + b->B, b->persist_gen, persist_timeout_ticks()};
	b->persist_gen += (unsigned)cx.max_passes + 1u;
	TimedScope tsc(b->ctx, "track_persist");
	launch_track_persist(b->view(), b->ctx->img, fp, *sm, ts, b->d_partials, nblk_p, ps, cx.max_passes, st);
	return MTFHIP_OK;
}

/* the chunked driver's chunk of targets: its views, its cut of the pixel pass, its queue.  fl / tl: the arguments of a pass that does not materialise
 * (replay arithmetic whatever the batch's math mode: a call that asks for the interface arrays has asked for it; no grid rebuild) */
struct ChunkRun { BatchView bc; FusedArgs fc, fl; TrackState tc, tl; int nblk_c, t0, nt; double *part; hipStream_t s; bool done; };
static void track_chunk_runs(mtfhip_batch *b, const FusedArgs &fa, const TrackState &ts, int chunk, int n_streams, bool defer, std::vector<ChunkRun> &runs) {
	const BatchView bv = b->view();
	const bool ncc = ncc_rows(b);
	const size_t RL = ncc ? NCC_ACC_COUNT : ACC_COUNT;   /* partial / reduced row length */
	for (int t0 = 0; t0 < b->B; t0 += chunk) {
		const int nt = std::min(chunk, b->B - t0);
		BatchView bc = bv;
		bc.B = nt;
		for (int i = 0; i < MTFHIP_BUF_COUNT; ++i)
			if (bc.buf[i]) bc.buf[i] += (size_t)t0 * b->per_target[i];
		bc.warps += 9 * (size_t)t0; bc.states += 8 * (size_t)t0;
		FusedArgs fc = fa;
		fc.active = fa.active + t0;
		if (fc.w0) fc.w0 += 9 * (size_t)t0;
		TrackState tc{ts.acc + (size_t)t0 * RL, ts.h0 + (size_t)t0 * 64, ts.corners + 8 * (size_t)t0,
			ts.init_corners_hm + 12 * (size_t)t0, ts.active + t0, ts.n_iters + t0, ncc ? ts.ncc + 8 * (size_t)t0 : nullptr,
			ncc ? ts.ncc_tm + NCC_TM_COUNT * (size_t)t0 : nullptr, 0, ts.lm ? ts.lm + (size_t)kLmStride * t0 : nullptr, nullptr,
			ts.trace ? ts.trace + (size_t)t0 * ts.trace_cap * kTraceStride : nullptr, ts.trace_cap,
			ts.h_extra ? ts.h_extra + (size_t)t0 * b->S * b->S : nullptr, ts.h_extra_scale, ts.fast_finish};
		int nblk_c; { int rows; fused_decomposition(b->N, nt, nblk_c, rows, MTFHIP_SLOTS / n_streams); fc.rows_per_block = rows; }
		if (nblk_c > b->nblk_max) { int rows; fused_decomposition(b->N, nt, nblk_c, rows); fc.rows_per_block = rows; }
		if (fc.rows_per_block < kGridRegenMinRows) fc.grid_regen = 0;   /* (fused_args' test, for the chunk's own cut) */
		double *part = b->d_partials + (size_t)t0 * b->nblk_max * RL;
		/* MTFHIP_TRACK_SERIALIZE=1: the same chunks and the same cut of the pixel pass, one queue -- for the PMC passes, whose
		 * per-dispatch counters are device-wide and would include the launch in flight on the other queue */
		static const bool serialize = std::getenv("MTFHIP_TRACK_SERIALIZE") && std::getenv("MTFHIP_TRACK_SERIALIZE")[0] == '1';
		const int q = serialize ? n_streams - 1 : (int)(runs.size() % (size_t)n_streams);
		FusedArgs fl = fc;
		fl.materialize = 0; fl.fast_math = 0; fl.grid_regen = 0;
		tc.keep_last = ts.keep_last; tc.lo_ssm = ts.lo_ssm; tc.SS = ts.SS;
		if (defer || ts.keep_last) { tc.warp_last = b->d_last_ws + 9 * (size_t)t0; tc.state_last = b->d_last_ws + 9 * (size_t)b->B + 8 * (size_t)t0; tc.need_mat = b->d_need_mat + t0; }
		TrackState tl = tc;
		tl.lean_pass = 1;
		runs.push_back(ChunkRun{bc, fc, fl, tc, tl, nblk_c, t0, nt, part, q == n_streams - 1 ? b->ctx->stream : b->ctx->extra_streams[q], false});
	}
}
/* deferred materialisation: targets that stopped behind a lean pass get the materialising kernel once more at the warp of that pass (the same
 * pass again: the partial rows it rewrites are the ones already there; no finish follows).  A target whose flag is clear costs an idle pass. */
static void track_materialise_stopped(mtfhip_batch *b, const ChunkRun &r) {
	BatchView bm = r.bc;
	bm.warps = r.tc.warp_last; bm.states = r.tc.state_last;
	FusedArgs fm = r.fc;
	fm.active = r.tc.need_mat;
	TimedScope tsc(b->ctx, "fused_lk", r.s);
	launch_fused_ssd(bm, b->ctx->img, fm, r.part, r.nblk_c, r.s);
}
/* the extra queues of the loop and the phase stamps that keep two of them apart (PhaseCtl); what cannot be created leaves one queue.
 * MTFHIP_TRACK_PHASE: the fraction of a period the queues are kept apart; 0 = no control */
static double track_phase_frac() {
	const char *e_ph = std::getenv("MTFHIP_TRACK_PHASE");
	return e_ph ? std::atof(e_ph) : 0.35;
}
static void track_phase_words(mtfhip_ctx *c) {
	if (c->d_phase.reserve(4) != hipSuccess) (void)hipGetLastError();
}
static int track_open_queues(mtfhip_batch *b, int n_streams, double &phase_frac) {
	mtfhip_ctx *c = b->ctx;
	if (n_streams >= 2) {
		if (!c->ev_fork && c->ev_fork.create(hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); n_streams = 1; }
		for (int q = 0; q + 1 < n_streams; ++q)
			if (!(c->extra_streams[q] && c->ev_join[q]) && (c->extra_streams[q].create(hipStreamNonBlocking) != hipSuccess ||
				c->ev_join[q].create(hipEventDisableTiming) != hipSuccess)) { (void)hipGetLastError(); n_streams = 1; break; }
	}
	phase_frac = track_phase_frac();
	if (n_streams == 2 && phase_frac > 0) {
		track_phase_words(c);
	}
	return n_streams;
}
/* Every way out of the chunked driver joins the extra queues: the normal path with an event the context's stream waits on; an early return
 * (a failed launch or copy: TRY / HIP_TRY) by draining them here -- kernels still in flight on an extra queue would otherwise race with
 * whatever the caller enqueues next on the context's stream (r03 advisor finding). */
struct QueueJoin {
	mtfhip_ctx *c; int n; bool joined = false;
	~QueueJoin() { if (!joined) for (int q = 0; q + 1 < n; ++q) if (c->extra_streams[q]) (void)hipStreamSynchronize(c->extra_streams[q]); }
};
/* Small batches (a single tracker's target, a handful of them): one launch per pass instead of two -- the pixel pass's last workgroup runs
 * the finish (kernels_step.hip).  MEASURED r05 (one box, ESM + SSD + homography, 200 iterations per call): 200 x 200 full 12.22 -> 12.54 us
 * per iteration, lean 10.92 -> 10.79, 50 x 50 lean 10.55 -> 10.44: nothing.  The r04 verdict's estimate (a launch boundary = the finish
 * kernel's 4.9 us) does not hold: the in-kernel hand-over -- acknowledged stores, an agent-scope arrival, ~160 rows read back past the L2
 * -- costs what the boundary cost, as the persistent loop's did in r03.  Opt-in (MTFHIP_STEP=1) and bit-identical to the two-launch loop
 * (test_one_launch_per_pass_equals_two_launch_loop); MTFHIP_STEP_MAX_TARGETS bounds the batch size it takes (default 8). */
static bool track_takes_step(const mtfhip_batch *b, const FusedArgs &fa, int so_term, int n_streams) {
	const char *e_st = std::getenv("MTFHIP_STEP");   /* (read per call: the tests flip it) */
	const char *e_mx = std::getenv("MTFHIP_STEP_MAX_TARGETS");
	const int max_t = e_mx ? std::atoi(e_mx) : 8;
	return (e_st && e_st[0] == '1') && so_term < 0 && !b->lo_ssm && !loop_only(b) && n_streams == 1 && b->B <= max_t && track_step_available(b->view(), fa);
}
/* one pass of one chunk on its queue: the intensity re-maps, the pixel pass (lean: the non-materialising one), the second-order pass, the finish */
struct FinishCtl { PhaseCtl pc; HostPublish pub; int prio; };
static int track_chunk_pass(mtfhip_batch *b, const mtfhip_sm_desc *sm, const FusedArgs &fa, const TrackCtx &cx, const ChunkRun &r, int it, bool lean, bool use_step,
	const FinishCtl &fc) {
	if (use_step) {
		TimedScope tsc(b->ctx, "track_step", r.s);
		launch_track_step(r.bc, b->ctx->img, r.fc, *sm, r.tc, r.part, r.nblk_c, b->d_persist + r.t0, r.s);
		return MTFHIP_OK;
	}
	/* (the SCV family: the chunk's template re-map or current maps -- the loop's first pass is the frame's first iteration) */
	FusedMaps maps;
	TRY(imap_before_pass(b, &r.bc, r.t0, r.fc.active, &r.fc, 0, it == 0, r.s, &maps));
	{
		TimedScope tsc(b->ctx, "fused_lk", r.s);
		const SpssArgs sp = spss_am(b) ? spss_args(b, sm) : SpssArgs{};
		launch_fused_ssd(r.bc, b->ctx->img, lean ? r.fl : r.fc, r.part, r.nblk_c, r.s, &maps, spss_am(b) ? &sp : nullptr);
	}
	if (cx.so_term >= 0) {
		TimedScope tsc(b->ctx, "second_order", r.s);
		launch_second_order_ssd(r.bc, b->ctx->img, cx.so_term, fa.chained, b->d0_variant, fa.grad_eps, b->hess_eps, b->norm_mult, b->norm_add,
			b->d_d2_part + (size_t)r.t0 * cx.nb2 * 64, cx.nb2, b->d_d2_out + (size_t)r.t0 * b->S * b->S, r.s, 1,
			b->desc.am == MTFHIP_AM_NCC ? SecondOrderNcc{r.part, r.nblk_c, r.tc.ncc} : SecondOrderNcc{nullptr, 0, nullptr});
	}
	TimedScope tsc(b->ctx, "finish_track", r.s);
	TrackState tf = lean ? r.tl : r.tc;
	tf.last_pass = it + 1 == cx.max_passes ? 1 : 0;
	tf.finish_prio = fc.prio;
	/* (SSIM: the finish that reads NCC's rows as SSIM does, with the model's constants -- kernels_ssim.hip) */
	if (ssim_am(b)) launch_finish_track_ssim(r.bc, *sm, tf, r.part, r.nblk_c, r.s, fc.pc, fc.pub, r.t0, b->ssim_c1, b->ssim_c2);
	else launch_finish_track(r.bc, *sm, tf, r.part, r.nblk_c, r.s, fc.pc, fc.pub, r.t0);
	return MTFHIP_OK;
}
/* Targets are independent, so the loops commute: all passes of a chunk of targets (track_chunk) run before the next chunk starts, two
 * chunks at a time where two queues pay (track_queues).  The queues start a quarter of a period apart (a spinning one-wave kernel in front of the later one; the period is estimated from
 * the bytes a pass moves): started together they stay in lockstep on some boxes -- the fill and drain phases of the two pixel
 * passes coincide and so do the two solves, 55 us per step of 64 x 200 x 200 against 49 out of phase (from there on the solve
 * kernels keep them apart, PhaseCtl).  A/B at that size, three boxes: no delay 1.05-1.10 M iters/s in 20-iteration calls and
 * 1.13-1.19 M in 200-iteration ones, 15 us 1.13-1.15 M and 1.28-1.30 M, 25 / 30 / 35 us in between and less repeatable.
 * MTFHIP_TRACK_STAGGER_US: > 0 that many microseconds, 0 none.
 * The context's own stream takes the LATER chunk of a pair: it is then the last to finish, and the join at the end of the call finds
 * the other queue's event already signalled instead of paying a cross-queue wait (~12 us) in front of the result read-back. */
/* The end of a call (cx.fused_io): the finish that stops a target, or the last one enqueued, hands the target to the host (k_finish_track's HostPublish), so
 * the host neither waits for the queues' join nor launches k_publish_host: it is released when the last of the B targets has arrived.  The join
 * events are still recorded and waited on the context's stream before the host starts to wait: whatever is enqueued there next runs behind
 * both queues, and wait_host_flag's fall-back synchronisation covers them.  The trailing materialising launches of an epsilon > 0 call may
 * end after the flag: they are in front of that join too, i.e. stream-ordered in front of everything that can read It / dIt_dx / Jt.  That
 * covers the arrays, not the image those launches sample: the context's own image is only replaced by work on the context's stream, a
 * BORROWED one is the caller's to rewrite from any stream after the call, so epsilon > 0 on a borrowed image keeps the old delivery (below).
 * A set trace (one queue, compared pass by pass), the one-launch-per-pass form, the rest of a persistent launch (targets that are no longer
 * active would never arrive) and a batch without host-coherent mirrors (MTFHIP_ZERO_COPY=0) keep k_publish_host / the copy. */
static int track_loop_chunked(mtfhip_batch *b, const mtfhip_sm_desc *sm, const FusedArgs &fa, const TrackState &ts, const TrackCtx &cx, unsigned long long &pub_seq) {
	hipStream_t st = b->ctx->stream;
	int chunk = track_chunk(b, sm, fa);
	double phase_frac;
	const int n_streams = track_open_queues(b, track_queues(b, fa), phase_frac);
	/* (words_ready: the head of the call has zeroed the stamps and the flags -- k_track_prologue, track_core) */
	if (!cx.words_ready && n_streams == 2 && phase_frac > 0 && b->ctx->d_phase) HIP_TRY(hipMemsetAsync(b->ctx->d_phase, 0, sizeof(unsigned long long) * 4, st));
	const bool use_step = track_takes_step(b, fa, cx.so_term, n_streams);
	if (use_step) TRY(ensure_persist_words(b, st));
	/* deferred materialisation (track_defers_materialisation): the passes before the last run the lean kernel */
	const bool defer = track_defers_materialisation(b, sm, fa, cx.so_term, cx.resume, use_step);
	if (defer || ts.keep_last) {
		HIP_TRY(b->d_last_ws.reserve(17 * (size_t)b->B));
		HIP_TRY(b->d_need_mat.reserve((size_t)b->B));
		if (!cx.words_ready) HIP_TRY(hipMemsetAsync(b->d_need_mat, 0, sizeof(int) * (size_t)b->B, st));
	}
	/* the later queue's start-up delay: a quarter of the period of the pass kind that runs.  Materialising passes are store-bound (130 B per pixel
	 * at 6.5 TB/s + the solve); the lean passes of a deferred call are issue-bound: 30.4 us per step of 64 x 200 x 200 on two queues
	 * (profiles/track_call_cost.md), i.e. 8.75 us per million pixels + the same 8 */
	const char *e_sg = std::getenv("MTFHIP_TRACK_STAGGER_US");   /* (read per call: the A/B and the tests flip it) */
	double stagger_us = e_sg ? std::atof(e_sg) : -1.0;
	if (stagger_us < 0) stagger_us = 0.25 * ((double)b->B * b->N * (defer ? 8.75e-6 : 130.0 / 6.5e6) + 8.0) * (2.0 / n_streams);
	FinishCtl fin{PhaseCtl{nullptr, nullptr, 0.0}, HostPublish{nullptr, 0, 0, nullptr, nullptr, 0, 0}, 0};
	{
		const char *e_pr = std::getenv("MTFHIP_FINISH_PRIO");   /* (read per call) */
		fin.prio = (e_pr && e_pr[0] == '0') ? 0 : 1;
	}
	/* a borrowed image may be rewritten by its owner, on a stream of the owner's, once a call that returns results has returned (mtfhip.h).  With a
	 * reachable epsilon, pixel passes follow the delivery -- the trailing materialising launches, which sample the image, and passes enqueued
	 * for targets that have all stopped -- so such a call keeps the delivery behind the join, which waits for them */
	const mtfhip_ctx *c = b->ctx;
	const bool borrowed = c->img.data != c->img_owned && c->img.data != c->prev_owned;
	if (cx.fused_io && b->h_pub_dev && !b->d_trace && !use_step && !cx.resume && !(borrowed && sm->epsilon > 0)) {
		pub_seq = ++b->acc_seq;
		fin.pub = HostPublish{b->h_pub_dev, b->slab_dbl_bytes, b->B, b->d_fin_count, b->h_flag_dev, pub_seq, publish_fenced()};
	}
	if (n_streams >= 2) {
		const int part_sz = (b->B + n_streams - 1) / n_streams;
		if (chunk > part_sz) chunk = part_sz;
		HIP_TRY(hipEventRecord(b->ctx->ev_fork, st));   /* the slab upload */
		for (int q = 0; q + 1 < n_streams; ++q) HIP_TRY(hipStreamWaitEvent(b->ctx->extra_streams[q], b->ctx->ev_fork, 0));
	}
	std::vector<ChunkRun> runs;
	track_chunk_runs(b, fa, ts, chunk, n_streams, defer, runs);
	const auto dbg_t0 = std::chrono::steady_clock::now();
	QueueJoin queue_join{b->ctx, n_streams};
	std::vector<int> h_flags;
	/* the chunks of a group (one per queue) advance together, pass by pass, so that both queues are fed from the start */
	for (size_t g0 = 0; g0 < runs.size(); g0 += (size_t)n_streams) {
		const size_t g1 = std::min(runs.size(), g0 + (size_t)n_streams);
		for (int it = 0; it < cx.max_passes; ++it) {
			bool all_done = true;
			const bool lean = defer && it + 1 < cx.max_passes;   /* (the pass the host knows to be the last materialises) */
			for (size_t k = g0; k < g1; ++k) {
				ChunkRun &r = runs[k];
				if (r.done) continue;
				if (n_streams >= 2 && it == 0 && k > g0 && stagger_us > 0) launch_queue_delay(stagger_us * (double)(k - g0), r.s);
				fin.pc = PhaseCtl{nullptr, nullptr, 0.0};
				if (n_streams == 2 && phase_frac > 0 && b->ctx->d_phase) {
					const int qi = (int)((k - g0) & 1);
					fin.pc = PhaseCtl{b->ctx->d_phase + qi, b->ctx->d_phase + (1 - qi), phase_frac};
				}
				TRY(track_chunk_pass(b, sm, fa, cx, r, it, lean, use_step, fin));
				if (loop_all_stopped(sm, cx.max_passes, it, r.tc.active, r.nt, r.s, h_flags)) r.done = true;
				all_done = all_done && r.done;
			}
			if (all_done) break;
		}
		if (defer && sm->epsilon > 0)
			for (size_t k = g0; k < g1; ++k) track_materialise_stopped(b, runs[k]);
	}
	if (g_track_dbg_timing)
		std::fprintf(stderr, "[track] %d queues, %d passes enqueued in %.1f us\n", n_streams, cx.max_passes,
			std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - dbg_t0).count());
	for (int q = 0; q + 1 < n_streams; ++q) {
		HIP_TRY(hipEventRecord(b->ctx->ev_join[q], b->ctx->extra_streams[q]));
		HIP_TRY(hipStreamWaitEvent(st, b->ctx->ev_join[q], 0));
	}
	queue_join.joined = true;
	return MTFHIP_OK;
}

/* validation, the driver's choice, the slab upload, the loop state, the driver, the read-back, and what follows a persistent launch cut short */
static int track_core_impl(mtfhip_batch *b, const mtfhip_sm_desc *sm, int *n_iters, double *corners, bool slab_uploaded, bool resume, bool region_mode);
/* A low-order SSM (mtfhip_batch::lo_ssm): the loop runs on the batch as an affine one (PassMode) -- the affine pixel pass, the finish that
 * projects its system -- on the two-launch route.  A materialising loop leaves six Jacobian columns in the scratch planes; the interface's
 * N x S curr_pix_jacobian is written behind the loop by the model's own expressions from the materialised dIt_dx, at the warp every
 * target's last pass ran at (TrackState::keep_last), and ESM's mean_pix_jacobian from that and J0 where the search method keeps one. */
static int track_core(mtfhip_batch *b, const mtfhip_sm_desc *sm, int *n_iters, double *corners, bool slab_uploaded, bool resume, bool region_mode) {
	if (!b || !b->lo_ssm || b->pass_mode) return track_core_impl(b, sm, n_iters, corners, slab_uploaded, resume, region_mode);
	TRY(lowdof_template_current(b, "track"));
	{
		PassMode pm(b);
		TRY(ensure_buf(b, MTFHIP_BUF_J0));
		TRY(ensure_buf(b, MTFHIP_BUF_JT));   /* (the pass's six-column planes) */
		TRY(track_core_impl(b, sm, n_iters, corners, slab_uploaded, resume, region_mode));
	}
	if (sm->materialize && sm->sm != MTFHIP_SM_ICLK) {
		BatchView v = b->view();
		v.warps = b->d_last_ws; v.states = b->d_last_ws + 9 * (size_t)b->B;
		{
			TimedScope ts(b->ctx, "pix_jacobian");
			launch_pix_jacobian(v, sm->chained_warp ? MTFHIP_JAC_WARPED : MTFHIP_JAC_INIT, b->buf[MTFHIP_BUF_DIT_DX], b->buf[MTFHIP_BUF_JT], b->ctx->stream);
		}
		touch(b, MTFHIP_BUF_JT);
		b->jt_valid = true;
		if (sm->sm == MTFHIP_SM_ESM && (sm->jac_type == 0 || sm->hess_type == 3)) TRY(mtfhip_sm_mean_jacobian(b));   /* NT/ESM.cc:239-242 */
	}
	return MTFHIP_OK;
}
static int track_core_impl(mtfhip_batch *b, const mtfhip_sm_desc *sm, int *n_iters, double *corners, bool slab_uploaded, bool resume, bool region_mode) {
	FLUSH_AM(b);   /* (none of the loop's kernels reads CURR_PTS: they warp the template grid themselves) */
	TRY(begin_entry(b));
	TRY(track_validate(b, sm));
	/* passes to enqueue: a rejected Levenberg-Marquardt step does not consume an iteration of FCLK's while loop (NT/FCLK.cc:193-223),
	 * and two rejections never follow each other (the pass after an undo skips the test) */
	TrackCtx cx{second_order_term(sm, b->desc.am), (sm->leven_marq && sm->sm == MTFHIP_SM_FCLK) ? 2 * sm->max_iters : sm->max_iters, 0, resume, region_mode};
	hipStream_t st = b->ctx->stream;
	const bool mi = hist_am(b), ncc = ncc_rows(b);   /* (mi: MI or CCRE, a driver of their own; ncc: the pass reduces NCC's rows -- NCC itself and SSIM) */
	/* (the one-launch grid kernel has no Levenberg-Marquardt: with it ICLK takes the fused launch + finish per pass) */
	const bool one_launch = !mi && !sm->leven_marq && iclk_one_launch(b, sm) && cx.so_term < 0;
	FusedArgs fa;
	if (!one_launch && !mi) TRY(fused_args(b, sm, fa));
	else { fa.materialize = 0; fa.mode = 2; fa.active = nullptr; fa.rows_per_block = 1; fa.j0_recompute = 0; fa.inline_warp = 0; fa.fast_math = 0; fa.grid_regen = 0; fa.w0 = nullptr; }
	/* right behind a fused grid re-initialisation the one-launch kernels need nothing of the slab's warps / states / corners (identity, zero, the
	 * templates' own corners: TrackState::fresh_reset): no fill_stage, no ingest launch (5 us + its gap per frame of a reset-every-frame loop) */
	const bool fresh = b->fresh_reinit && one_launch && !region_mode && !slab_uploaded && !resume && b->h_pub_dev && b->d_trace == nullptr;
	b->fresh_reinit = false;
	/* (a pending fused initialisation, hold_init_pull: the mirrors' NCC scalars are older than d_ncc, which k_template_init wrote) */
	/* the chunked driver's call path: one launch in front of the loop -- the slab ingest, the deferred-materialisation flags, the queues' phase stamps
	 * and the Levenberg-Marquardt start state (k_track_prologue) instead of the ingest, two memsets and a pageable copy + synchronisation -- and the
	 * delivery from inside the loop (track_loop_chunked).  MTFHIP_TRACK_FUSED_IO=0 (read per call) keeps the separate steps (A/B, the tests).
	 * Where the slab is on the device already (a folded track_region) the kernel runs without the ingest: still one launch for all the words. */
	const bool persisted = !mi && !one_launch && cx.so_term < 0 && persist_fits(b, sm, fa);
	{
		const char *e_io = std::getenv("MTFHIP_TRACK_FUSED_IO");
		cx.fused_io = !mi && !one_launch && !persisted && !(e_io && e_io[0] == '0');
	}
	LoopWords lw{nullptr, 0, nullptr, nullptr, 0, 0.0, nullptr};
	if (cx.fused_io && !resume) {
		/* (the flags only for a call that can defer -- the one-launch-per-pass form, decided with the queues, may still turn it down: the
		 * flags are then zeroed for nothing; the stamps only where two queues will use them; words that exist from earlier calls cost nothing) */
		if (track_defers_materialisation(b, sm, fa, cx.so_term, resume, false)) {
			HIP_TRY(b->d_last_ws.reserve(17 * (size_t)b->B));
			HIP_TRY(b->d_need_mat.reserve((size_t)b->B));
		}
		if (sm->leven_marq) HIP_TRY(b->d_lm.reserve(kLmStride * (size_t)b->B));
		if (track_queues(b, fa) == 2 && track_phase_frac() > 0) track_phase_words(b->ctx);
		lw = LoopWords{b->d_need_mat, b->d_need_mat ? b->B : 0, b->ctx->d_phase, sm->leven_marq ? b->d_lm : nullptr, b->B, sm->lm_delta_init, b->d_fin_count};
		cx.words_ready = true;
	}
	if (!slab_uploaded && !fresh) TRY(loop_upload_slab(b, st, b->hold_init_pull && b->init_mirror_seq != 0, cx.words_ready ? &lw : nullptr));
	else {
		b->warps_dirty = false;   /* the slab on the device carries the warps */
		if (cx.words_ready) { TimedScope tsc(b->ctx, "track_prologue", st); launch_track_prologue(nullptr, nullptr, 0, 0, 0, lw, st); }
	}
	fa.active = b->d_active;
	if (ncc && !one_launch && !b->d_ncc_tm) return fail(MTFHIP_ERR_LOGIC, "track before init_template");
	TrackState ts{b->d_acc, b->d_h0, b->d_corners, b->d_init_corners_hm, b->d_active, b->d_iters, ncc ? b->d_ncc : nullptr, ncc ? b->d_ncc_tm : nullptr, 0, nullptr, nullptr,
		b->d_trace, b->trace_cap};
	ts.fresh_reset = fresh ? 1 : 0;
	if (b->d_trace && !resume) HIP_TRY(hipMemsetAsync(b->d_trace, 0, sizeof(double) * kTraceStride * (size_t)b->trace_cap * b->B, st));
	if (mi && b->d_trace) ts.f_ext = b->d_mi_f;   /* (the trace records the similarity; Levenberg-Marquardt sets it below as well) */
	if (sm->leven_marq) {
		if (resume || cx.words_ready) ts.lm = b->d_lm;   /* (words_ready: the head of the call has written the start state) */
		else TRY(loop_lm_state(b, sm, st, &ts.lm));
		if (mi) ts.f_ext = b->d_mi_f;
	}
	if (cx.so_term >= 0) {
		/* second-order term of SSD's Hessian inside the loop: one more pixel pass per iteration (k_second_order_ssd, the points
		 * re-derived from the warp), its S x S sums added by the finish, which then solves with pivoting */
		cx.nb2 = simple_blocks_per_target(b->N);
		TRY(ensure_second_order_scratch(b));
		/* (halved with the rest of the sum: ESM SumOfStd, NT/ESM.cc:339; MI's SumOfSelf, NT/ESM.cc:333) */
		ts.h_extra = b->d_d2_out; ts.h_extra_scale = (cx.so_term == 1 || (cx.so_term == 4 && sm->sm == MTFHIP_SM_ESM && sm->hess_type == 2)) ? 0.5 : 1.0;
	}
	{
		/* tolerance mode + a definite first-order system: the register-resident finish (finish_track_fast_body) */
		const char *e = std::getenv("MTFHIP_FAST_FINISH");   /* (read per call: the tests compare the two bodies in one process) */
		const bool enabled = !(e && e[0] == '0');
		ts.fast_finish = (enabled && b->math_mode == MTFHIP_MATH_FAST && ssd_like(b) && cx.so_term < 0) ? 1 : 0;   /* (SSD's rows: NCC, MI and CCRE, SPSS and SSIM each have a finish of their own) */
		/* a low-order SSM: the projection lives in finish_track_body alone (the register-resident body would index its rows at run time);
		 * its materialising loop keeps every target's last warp for the Jacobian written behind the loop (track_core) */
		if (b->lo_ssm) { ts.fast_finish = 0; ts.keep_last = (fa.materialize && fa.mode != 2) ? 1 : 0; ts.lo_ssm = b->lo_ssm; ts.SS = ssm_state_size(b->lo_ssm); }
	}
	unsigned long long pub_seq = 0;   /* non-zero: the loop's own kernel delivers the results to the host */
	if (ccre_am(b)) TRY(track_loop_ccre(b, sm, ts, cx));
	else if (mi) TRY(track_loop_mi(b, sm, ts, cx));
	else if (one_launch) TRY(track_loop_one_launch(b, sm, ts, cx, pub_seq));
	else if (persisted) TRY(track_loop_persist(b, sm, fa, ts, cx));
	else TRY(track_loop_chunked(b, sm, fa, ts, cx, pub_seq));
	const char *h_res;
	TRY(loop_read_back(b, st, pub_seq, n_iters, corners, &h_res));
	const int *act = reinterpret_cast<const int *>(h_res + b->slab_dbl_bytes), *iters = act + b->B;
	if (region_mode)
		for (int t = 0; t < b->B; ++t)
			if (iters[t] < 0) return fail(MTFHIP_ERR_INVALID_ARG, "track_region: degenerate corners for target %d", t);
	if (persisted) {
		/* a workgroup that could not wait any longer for its peers (CUs held by another process) leaves its target active with
		 * iterations to go: the two-launch loop takes the call from where the device stopped, and this batch stays with it */
		bool cut = false;
		for (int t = 0; t < b->B; ++t) cut = cut || act[t] != 0;
		if (cut) {
			b->persist_ok = false;
			HIP_TRY(hipStreamSynchronize(st));
			HIP_TRY(hipMemsetAsync(b->d_persist, 0, 2 * sizeof(int) * (size_t)b->B, st));
			return track_core(b, sm, n_iters, corners, true, true);   /* (the slab on the device is current: warps, flags, iteration counts) */
		}
	}
	if (!mi) {   /* (mi_enqueue keeps the flags of its own passes) */
		b->it_valid = fa.materialize;
		b->dit_valid = b->jt_valid = fa.materialize && fa.mode != 2;
	}
	loop_done(b);
	return MTFHIP_OK;
}

/* debug trace of the device-side loop: with max_passes > 0 every pass of mtfhip_batch_track / _track_region also records what it
 * solved (H, g, the state update, the corners it produced, f) -- the per-iteration quantities the parity tests compare with the
 * CPU trackers' traces; 0 switches it off (the default: a NULL test per pass) */
int mtfhip_batch_track_trace(mtfhip_batch *b, int max_passes) {
	if (!b || max_passes < 0) return fail(MTFHIP_ERR_INVALID_ARG, "track_trace: invalid argument");
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	b->d_trace.reset(); b->trace_cap = 0;
	if (max_passes > 0) {
		HIP_TRY(b->d_trace.reserve(kTraceStride * (size_t)max_passes * b->B));
		b->trace_cap = max_passes;
		HIP_TRY(hipMemsetAsync(b->d_trace, 0, sizeof(double) * kTraceStride * (size_t)max_passes * b->B, b->ctx->stream));
	}
	return MTFHIP_OK;
}
int mtfhip_batch_track_trace_read(mtfhip_batch *b, double *dst) {
	if (!b || !dst) return fail(MTFHIP_ERR_INVALID_ARG, "track_trace_read: NULL argument");
	if (!b->d_trace) return fail(MTFHIP_ERR_LOGIC, "track_trace_read: tracing is off (mtfhip_batch_track_trace)");
	HIP_TRY(hipMemcpyAsync(dst, b->d_trace, sizeof(double) * kTraceStride * (size_t)b->trace_cap * b->B, hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	return MTFHIP_OK;
}

} /* extern "C" */
