/*
 * mtfhip_api_internal.h -- what the translation units of the C-ABI implementation share: error plumbing, the small
 * host-side math (3x3 warps, 4-corner DLT), the context / batch handles and their helpers, and the declarations of
 * the functions that cross unit boundaries (the per-function entry points and kAmOps live in api_am.hip, each appearance model's own code in
 * a unit of its name, the deferred-fusion layer in api_lazy.hip, the skeleton of the device-side loops in api_track.hip).  Not installed:
 * include/mtfhip.h is the public contract.
 */
#ifndef MTFHIP_API_INTERNAL_H
#define MTFHIP_API_INTERNAL_H
#include "mtfhip_internal.h"
#include "mtfhip_am_served.h"

#include <algorithm>
#include <chrono>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace mtfhip;

namespace mtfhip {
void launch_init_grid(const BatchView &bv, const double *dev_w0, int resx, int resy, double lo_x, double lo_y,
	double hi_x, double hi_y, int force_unit_z, hipStream_t st);
}

/* ------------------------------------------------------------------ errors */
extern thread_local std::string g_last_error;   /* one per thread for the whole library; defined in api_core.hip */
constexpr size_t kErrMsgCap = 512;
static int fail(int code, const char *fmt, ...) {
	char buf[kErrMsgCap];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	g_last_error = buf;
	return code;
}
#define HIP_TRY(expr)                                                                        \
	do {                                                                                     \
		hipError_t _e = (expr);                                                              \
		if (_e != hipSuccess)                                                                \
			return fail(MTFHIP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
	} while (0)
#define TRY(expr)                  \
	do {                           \
		int _r = (expr);           \
		if (_r != MTFHIP_OK) return _r; \
	} while (0)

/* ------------------------------------------------------------------ small host math */
struct M3 {
	double m[9];
};
static M3 m3_identity() { return M3{{1, 0, 0, 0, 1, 0, 0, 0, 1}}; }
static M3 m3_mul(const M3 &a, const M3 &b) {
	M3 c;
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j)
			c.m[3 * i + j] = a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j] + a.m[3 * i + 2] * b.m[6 + j];
	return c;
}
/* Matrix3d::inverse() as Eigen evaluates it for fixed 3x3: cofactors / determinant */
static M3 m3_inverse(const M3 &a) {
	const double *u = a.m;
	M3 c;
	c.m[0] = u[4] * u[8] - u[5] * u[7]; c.m[1] = u[2] * u[7] - u[1] * u[8]; c.m[2] = u[1] * u[5] - u[2] * u[4];
	c.m[3] = u[5] * u[6] - u[3] * u[8]; c.m[4] = u[0] * u[8] - u[2] * u[6]; c.m[5] = u[2] * u[3] - u[0] * u[5];
	c.m[6] = u[3] * u[7] - u[4] * u[6]; c.m[7] = u[1] * u[6] - u[0] * u[7]; c.m[8] = u[0] * u[4] - u[1] * u[3];
	double det = u[0] * c.m[0] + u[1] * c.m[3] + u[2] * c.m[6];
	double inv_det = 1.0 / det;
	for (int i = 0; i < 9; ++i) c.m[i] *= inv_det;
	return c;
}
/* the low-order rigid models: Similitude (S = 4), Isometry (3), Translation (2) */
static inline bool ssm_lowdof(int ssm) { return ssm == MTFHIP_SSM_SIMILITUDE || ssm == MTFHIP_SSM_ISOMETRY || ssm == MTFHIP_SSM_TRANSLATION; }
static inline bool ssm_known(int ssm) { return ssm == MTFHIP_SSM_HOMOGRAPHY || ssm == MTFHIP_SSM_AFFINE || ssm_lowdof(ssm); }
static inline int ssm_state_size(int ssm) {
	switch (ssm) {
	case MTFHIP_SSM_HOMOGRAPHY: return 8;
	case MTFHIP_SSM_SIMILITUDE: return 4;
	case MTFHIP_SSM_ISOMETRY: return 3;
	case MTFHIP_SSM_TRANSLATION: return 2;
	default: return 6;
	}
}
static inline const char *ssm_name(int ssm) {
	switch (ssm) {
	case MTFHIP_SSM_HOMOGRAPHY: return "homography";
	case MTFHIP_SSM_AFFINE: return "affine";
	case MTFHIP_SSM_SIMILITUDE: return "similitude";
	case MTFHIP_SSM_ISOMETRY: return "isometry";
	case MTFHIP_SSM_TRANSLATION: return "translation";
	default: return "unknown";
	}
}
/* getWarpFromState: Homography.cc:94-107, Affine.cc:116-130, Similitude.cc:123-141, Isometry.cc:68-86, Translation.cc:86-93 */
static M3 warp_from_state(int ssm, const double *p) {
	M3 W;
	if (ssm == MTFHIP_SSM_HOMOGRAPHY) {
		W.m[0] = 1 + p[0]; W.m[1] = p[1]; W.m[2] = p[2];
		W.m[3] = p[3]; W.m[4] = 1 + p[4]; W.m[5] = p[5];
		W.m[6] = p[6]; W.m[7] = p[7]; W.m[8] = 1;
	} else if (ssm == MTFHIP_SSM_SIMILITUDE) {
		W.m[0] = 1 + p[2]; W.m[1] = -p[3]; W.m[2] = p[0];
		W.m[3] = p[3]; W.m[4] = 1 + p[2]; W.m[5] = p[1];
		W.m[6] = 0; W.m[7] = 0; W.m[8] = 1;
	} else if (ssm == MTFHIP_SSM_ISOMETRY) {
		const double cos_theta = std::cos(p[2]), sin_theta = std::sin(p[2]);
		W.m[0] = cos_theta; W.m[1] = -sin_theta; W.m[2] = p[0];
		W.m[3] = sin_theta; W.m[4] = cos_theta; W.m[5] = p[1];
		W.m[6] = 0; W.m[7] = 0; W.m[8] = 1;
	} else if (ssm == MTFHIP_SSM_TRANSLATION) {
		W = M3{{1, 0, p[0], 0, 1, p[1], 0, 0, 1}};
	} else {
		W.m[0] = 1 + p[2]; W.m[1] = p[3]; W.m[2] = p[0];
		W.m[3] = p[4]; W.m[4] = 1 + p[5]; W.m[5] = p[1];
		W.m[6] = 0; W.m[7] = 0; W.m[8] = 1;
	}
	return W;
}
/* getStateFromWarp: Homography.cc:116-132, Affine.cc:132-143, Similitude.cc:144-153, Isometry.cc:88-97, Translation.cc:95-101 */
static void state_from_warp(int ssm, double *p, const M3 &W) {
	if (ssm == MTFHIP_SSM_HOMOGRAPHY) {
		p[0] = W.m[0] - 1; p[1] = W.m[1]; p[2] = W.m[2]; p[3] = W.m[3]; p[4] = W.m[4] - 1; p[5] = W.m[5];
		p[6] = W.m[6]; p[7] = W.m[7];
	} else if (ssm_lowdof(ssm)) {
		for (int k = 0; k < 8; ++k) p[k] = 0;
		p[0] = W.m[2]; p[1] = W.m[5];
		if (ssm == MTFHIP_SSM_SIMILITUDE) { p[2] = W.m[0] - 1; p[3] = W.m[3]; }
		else if (ssm == MTFHIP_SSM_ISOMETRY) p[2] = std::atan2(W.m[3], W.m[0]);
	} else {
		p[0] = W.m[2]; p[1] = W.m[5]; p[2] = W.m[0] - 1; p[3] = W.m[1]; p[4] = W.m[3]; p[5] = W.m[4] - 1;
		p[6] = p[7] = 0;
	}
}
/* The homography that maps the corners of the axis-aligned rectangle [lo_x, hi_x] x [lo_y, hi_y] (TL, TR, BR, BL) onto
 * four given corners -- what the reference obtains from the 4-point DLT (utils::computeHomographyDLT,
 * Utilities/src/warpUtils.cc:171-224, JacobiSVD of the 8 x 9 system).  Four point pairs determine the matrix uniquely up
 * to scale, so the closed form of the square-to-quadrilateral map (Heckbert 1989, eq. 2.12), composed with the
 * rectangle's normalisation and scaled to m[8] = 1, is the same matrix to rounding -- ~40 flops instead of an 8 x 8
 * elimination per target (GridTracker sets 256 of them per frame).  false: degenerate corners. */
static bool rect_to_quad(double lo_x, double lo_y, double hi_x, double hi_y, const double *q, M3 &H) {
	return rect_to_quad_hd(lo_x, lo_y, hi_x, hi_y, q, H.m);   /* (one set of expressions for host and device: mtfhip_internal.h) */
}

/* ------------------------------------------------------------------ handles */
struct Timer {
	std::vector<std::pair<Event, Event>> pending;
	double total_ms = 0;
	int n = 0;
	long launches = 0;
	/* [start, end) of every timed launch in ms since the context's reference event: launches of one family can overlap when the
	 * device-side loop runs on two queues, and the time the family was executing is then the union, not the sum */
	std::vector<std::pair<double, double>> spans;
};

struct mtfhip_ctx {
	int device = 0;
	Stream stream;   /* the caller's (borrowed) or the library's own */
	/* second queue of the device-side loop (track_loop_chunked: two chunks of independent targets in flight, one's solve + update under the
	 * other's pixel pass); created on first use, ordered against `stream` by the two events */
	Stream extra_streams[3];
	Event ev_fork, ev_join[3];
	Dev<unsigned long long> d_phase;   /* [4] wall-clock stamps of the queues' last solve (PhaseCtl) */
	ImgView img{nullptr, 0, 0, 0};   /* img, prev: views -- into img_owned / prev_owned, or of a borrowed image */
	Dev<float> img_owned;
	/* the previous frame (GridTracker's prev_img = curr_img.clone(), SM/src/GridTracker.cc:241-243, 266): mtfhip_image_keep_prev.  An image
	 * the context owns is kept by exchanging the two owned buffers (the next upload fills the other one: no copy); a borrowed one is copied. */
	ImgView prev{nullptr, 0, 0, 0};
	Dev<float> prev_owned;
	Dev<unsigned char> raw;      /* staging of the raw frame (pre-processing) */
	Dev<float> tmp_a, tmp_b;     /* gray / row-pass intermediates */
	/* The current image with every texel next to the one BELOW it -- pair[2 (y W + x)] = I[y][x], pair[2 (y W + x) + 1] = I[y + 1][x] -- so that
	 * the four texels of a bilinear cell are 16 contiguous bytes: ONE gather per sample instead of two for the kernels that sit on the vector
	 * memory path (the candidate scorer; r06 -- the NN rows kernel gained nothing from it).  Built on demand (ensure_pair_image) for images the context owns (an uploaded or derived
	 * image cannot change behind the library's back; a borrowed one can), rebuilt when img_serial has moved. */
	Dev<float> pair_owned;
	unsigned long long img_serial = 1, pair_serial = 0, pair_demand_serial = 0;
	size_t pair_demand = 0;   /* candidates scored on the current image so far without the copy (pair_image_if_it_pays) */
	int n_cus = 0;   /* compute units: the persistent loop needs its whole grid resident */
	bool timing = false;
	int timing_stride = 1;   /* events are recorded around every timing_stride-th launch of a family */
	std::map<std::string, Timer> timers;
	Event ev_ref;   /* recorded by timing_reset: origin of Timer::spans */
	std::vector<Event> free_events;
	std::vector<struct mtfhip_batch *> batches;   /* live batches: deferred work is flushed before the image changes */
	Dev<unsigned char> est_ws;   /* mtfhip_ssm_estimate_from_pts: device staging of its arguments and results */
};

struct TimedScope {
	mtfhip_ctx *ctx;
	Event a, b;
	Timer *tm = nullptr;
	hipStream_t on;
	TimedScope(mtfhip_ctx *c, const char *family, hipStream_t stream = nullptr) : ctx(c), on(stream ? stream : c->stream) {
		if (!ctx->timing) return;
		Timer *cand = &ctx->timers[family];
		if ((cand->launches++ % ctx->timing_stride) != 0) return;
		tm = cand;
		auto get = [&]() {
			Event e;
			if (!ctx->free_events.empty()) { e = std::move(ctx->free_events.back()); ctx->free_events.pop_back(); }
			else (void)e.create();
			return e;
		};
		a = get(); b = get();
		(void)hipEventRecord(a, on);
	}
	~TimedScope() {
		if (!tm) return;
		(void)hipEventRecord(b, on);
		tm->pending.emplace_back(std::move(a), std::move(b));
	}
};

constexpr int kAccRowMax = NCC_ACC_COUNT > ACC_COUNT ? NCC_ACC_COUNT : ACC_COUNT;   /* widest partial / reduced row */

struct TargetHost {
	M3 warp;
	double state[8];
	double corners[8], init_corners[8];
	double init_corners_hm[12];
	double f;
	/* NCC scalars (AM/src/NCC.cc members) */
	double I0_mean, It_mean, a, b, c, gmean;
	double i0_ss;   /* sum (I0 - I0_mean)^2 itself (c is its root): slot 6 of the device scalars, read by the SSIM finish */
	double it_ss;   /* SSIM: sum (It - It_mean)^2 of the last similarity update (a holds sum (I0 - I0_mean)(It - It_mean), as for NCC) */
	double h0[64]; /* constant self Hessian of the template (column-major), set by init_template */
	/* NCC, fused path: moments of the template's pixel Jacobian (constant while J0 is): sum J0, sum I0 J0, Gram(J0) */
	double ncc_tm[NCC_TM_COUNT];
};

/* (the bin limits of kAmTraits, mtfhip_am_served.h, are the kernels' own) */
static_assert(kAmTraits[MTFHIP_AM_MI].max_bins == MI_NB && kAmTraits[MTFHIP_AM_CCRE].max_bins == MI_NB && kAmTraits[MTFHIP_AM_SCV].max_bins == kImapMaxBins &&
	kAmTraits[MTFHIP_AM_RSCV].max_bins == kImapMaxBins && kAmTraits[MTFHIP_AM_LSCV].max_bins == kImapMaxBins && kAmTraits[MTFHIP_AM_LRSCV].max_bins == kImapMaxBins,
	"kAmTraits::max_bins");

/* The SCV family (SCV, RSCV, LSCV, LRSCV: SSD behind an intensity map) keeps ONE state: a batch has one appearance model for life.  SCV and
 * LSCV re-map the template (I0 = map(I0_orig)) in front of a similarity update; the reversed models RSCV and LRSCV map the current patch; the
 * localized models LSCV and LRSCV keep one map per overlapping sub-region and blend them per pixel (api_imap.hip). */
struct IntensityMapState {
	/* *Params: n_bins, weighted_mapping, SCV's hist_type and mapped_gradient; the localized models' n_sub_regions_x / _y, spacing_x / _y,
	 * affine_mapping, once_per_frame; the cell columns and cells their geometry has */
	int nb = 0, linear = 0, hist = 0, mapped_grad = 0;
	int nx = 3, ny = 3, sx = 10, sy = 10, affine = 0, once = 0;
	int ncx = 0, ncell = 0;
	Dev<double> orig;             /* [B][N] I0_orig (SCV, LSCV); It_orig of the per-function route (RSCV, LRSCV) */
	/* the template's code plane [B][N], one per kernel family: (int)I0_orig | (int)rint(I0_orig) << 8 (SCV, LSCV), (int)I0 (RSCV, LRSCV).
	 * It ARRIVES LAST at initializePixVals and is what everything takes for "captured": while it is null a failed call is simply repeated,
	 * and what belongs to the first call runs once the whole group is there */
	Dev<unsigned short> code16;
	Dev<unsigned char> code8;
	Dev<double> part_f;           /* [B][imap_hist_blocks][2 nb] pass-1 rows (SCV) */
	Dev<unsigned> part_u;         /* ... (RSCV) */
	Dev<unsigned> arrive;         /* [B] arrival counters (RSCV, LSCV, LRSCV) */
	Dev<double> map, aff;         /* [B][R][nb] the intensity maps, [B][R][2] the affine fits (localized; R = nx ny, else 1) */
	/* the sub-region geometry, one copy per batch: the cell plane [N] -- it arrives last of these and is what set_lscv / set_lrscv take for
	 * "the geometry is fixed" --, the cells of each sub-region [2 nx + 2 ny], the weights [R][N]; and the per-target sums [B][2][ncell nb] */
	Dev<unsigned short> cell;
	Dev<int> crng;
	Dev<double> w;
	Dev<unsigned> tot;
	bool captured() const { return code16 || code8; }
};

struct mtfhip_batch;
static int push_warps(mtfhip_batch *b);
struct mtfhip_batch {
	mtfhip_ctx *ctx;
	mtfhip_patch_desc desc;
	int B, N, S;          /* N = patch_size = NP * C (rows of the per-pixel AM arrays) */
	int NP = 0, C = 1;    /* sample points per target, channels */
	/* The low-order models (lo_ssm = MTFHIP_SSM_SIMILITUDE / _ISOMETRY / _TRANSLATION, else 0) on the fused path run the AFFINE pixel pass and
	 * keep everything upstream of the solve in affine coordinates.  While a fused entry point works (PassMode, below) the batch IS an
	 * affine one -- S = 6, desc.ssm = MTFHIP_SSM_AFFINE, buf[J0 / JT / JM] the six-column scratch planes pass_j[] that no entry point
	 * exposes -- so the template's constant Hessian th[].h0 / d_h0 and the NCC template moments are the affine ones; outside, S and
	 * desc.ssm are the model's own and the three buffers the interface's N x S arrays. */
	int lo_ssm = 0;
	bool pass_mode = false;
	Dev<double> pass_j[3];
	size_t pass_j_per_target[3] = {0, 0, 0};
	double norm_mult = 1, norm_add = 0;
	/* Every Dev<>, Pinned<> and Event member owns what it names and releases it with the batch.  The raw pointers are VIEWS: d_warps,
	 * d_states, d_corners, d_init_corners_hm, d_ncc, d_w0, d_active and d_iters point into d_slab, and every *_dev is the device address of
	 * the pinned buffer it is named after. */
	Dev<double> buf[MTFHIP_BUF_COUNT];
	size_t per_target[MTFHIP_BUF_COUNT];
	double *d_warps = nullptr, *d_states = nullptr, *d_w0 = nullptr, *d_corners = nullptr, *d_init_corners_hm = nullptr;   /* views into d_slab */
	double *d_ncc = nullptr;   /* [B][8] NCC scalars: a view into d_slab */
	Dev<double> d_partials, d_acc, d_scratch_pts, d_h0, d_cand;
	Dev<double> d_colmean; /* [B][8] column means */
	/* MI: per-target table block, block partial rows, similarity and Hessian outputs */
	Dev<double> d_mi_tb, d_mi_part, d_mi_f, d_mi_H;
	Dev<double> d_mi_poly;   /* [B][mi_poly_size()], allocated by the first recompute iteration */
	/* the fused template initialisation (kernels_init.hip, init_template's ICLK fast path): its small results arrive in this pinned
	 * record (kInitRec doubles per target) behind init_flag; init_mirror_seq != 0: the host mirrors (th[].h0, NCC scalars and template
	 * moments) are older than the device copies until pull_init_mirrors() has folded the record in (lazy_flush does) */
	Pinned<double, hipHostMallocMapped> h_init_rec;
	double *h_init_rec_dev = nullptr;
	Pinned<unsigned long long, hipHostMallocMapped> h_init_flag;
	unsigned long long *h_init_flag_dev = nullptr, init_seq = 0, init_mirror_seq = 0;
	bool init_rec_device = false;   /* the pending record was NOT published to pinned memory (grid re-initialisations, r05): pull_init_mirrors copies d_h0 / d_ncc / d_ncc_tm instead */
	Dev<double> d_mi_red;   /* [B][mi_row_len] block rows summed (the Hessian assembly then reads one row per target) */
	Dev<double> d_h0inv; /* [B][64] inverse of the constant Hessian (one-launch ICLK) */
	Dev<double> d_d2_part, d_d2_out, d_d2_w; /* second-order term: block rows, [B][64] sums, MI self weights */
	double hess_eps = 1.0;
	/* MTFHIP_MATH_*: arithmetic of the non-materialising kernels (include/mtfhip.h) */
	int math_mode = (std::getenv("MTFHIP_MATH") && (std::getenv("MTFHIP_MATH")[0] == 'r' || std::getenv("MTFHIP_MATH")[0] == '0')) ? MTFHIP_MATH_REPLAY : MTFHIP_MATH_FAST;
	bool init_pix_hess = false;
	/* J0 and dI0_dx are still exactly what init_template produced (no setter / pixel-Jacobian call touched them since): the
	 * fused kernel may then rebuild J0's rows from dI0_dx instead of reading them (MTFHIP_J0_RECOMPUTE=0 disables) */
	unsigned int frame_count = 0;   /* ImageBase::frame_count: ++ in initializePixVals and updateModel (ImageBase.cc:74, SSD.cc:51) */
	bool j0_is_template = false;
	long corners_epoch = 0, j0_template_corners_epoch = -1;   /* set_corners moves the grid: J0 rows depend on init_pts */
	/* the corners epoch whose grid k_init_grid laid out from the slab's w0 (what the staged slab keeps re-uploading), and whether every
	 * target's map had W0[6] = W0[7] = 0 there: FusedArgs::grid_regen */
	long grid_w0_epoch = -1;
	bool grid_w0_affine = false;
	int j0_variant = MTFHIP_JAC_WARPED;
	std::vector<double> template_corners;   /* [B][8] corners the stored J0 was computed on */
	bool j0_recompute_enabled = !(std::getenv("MTFHIP_J0_RECOMPUTE") && std::getenv("MTFHIP_J0_RECOMPUTE")[0] == '0');
	int d0_variant = MTFHIP_JAC_WARPED; /* how the template's pixel Hessian was formed (fused second-order path) */
	int mi_row_len = 0;
	std::vector<double> ccre_f_max;   /* CCRE: max_similarity, f of initializeSimilarity (CCRE.cc:261), per target */
	double mi_hist_norm = 0;
	IntensityMapState imap;   /* SCV, RSCV, LSCV, LRSCV: the model's own state (api_imap.hip) */
	int first_iter = 0;       /* AppearanceModel::first_iter (mtfhip_batch_set_first_iter; the localized models' once_per_frame reads it) */
	/* SPSS (am = MTFHIP_AM_SPSS): SPSSParams k and c = (k (PIX_MAX - PIX_MIN))^2 (SPSS.cc:37-38) */
	double spss_k = 0.01, spss_c = (0.01 * 255.0) * (0.01 * 255.0);
	/* SSIM (am = MTFHIP_AM_SSIM): SSIMParams k1, k2 and c1 = (k1 (PIX_MAX - PIX_MIN))^2, c2 likewise (SSIM.cc:36-39) */
	double ssim_k1 = 0.01, ssim_k2 = 0.03, ssim_c1 = (0.01 * 255.0) * (0.01 * 255.0), ssim_c2 = (0.03 * 255.0) * (0.03 * 255.0);
	Dev<double> d_cand_mi;   /* MI candidate scoring: histogram rows per candidate */
	int *d_active = nullptr, *d_iters = nullptr;   /* views into d_slab */
	/* The small per-target state lives in ONE device allocation (warps | states | corners | init_corners_hm | ncc | w0 |
	 * active | iters) mirrored by two pinned staging buffers, so that set_corners and track each move it with a single
	 * copy (a grid frame used to cost 14 small copies and 4 stream syncs around a 100 us kernel). */
	Dev<char> d_slab;
	Pinned<char> h_stage_a, h_stage_b;
	Event ev_a, ev_b;
	/* k_track_persist: barrier words, the generation counter the host advances per launch; persist_ok is cleared for good when a
	 * launch could not keep its workgroups resident (the two-launch loop finishes the call and serves the later ones) */
	Dev<int> d_persist;
	/* deferred materialisation of the device-side loop (track_loop_chunked): warp [B][9] | state [B][8] of the last pass of a target that stopped
	 * behind a non-materialising pass, and the per-target flags of the trailing materialising launch */
	Dev<double> d_last_ws;
	Dev<int> d_need_mat;
	unsigned persist_gen = 0;
	bool persist_ok = true;
	bool stage_a_busy = false;   /* ev_a guards an upload from h_stage_a that may still be in flight */
	/* warp + state of every target after setState / compositionalUpdate: one copy from a pinned double buffer, no sync */
	Pinned<double> h_wstage[2];
	Event ev_w[2];
	int wflip = 0;
	/* CURR_PTS / CURR_HXY / CURR_Z lag behind the warp: only the un-fused kernels read them, so k_apply_warp runs when
	 * one of those is about to be launched (lazy_flush) or the arrays are read, not after every update */
	bool pts_stale = false;
	Dev<double> d_it_shadow;
	Dev<double> d_ncc_tm;   /* [B][52] NCC template moments for the device-side finish */
	/* the one-launch forward-backward frame (k_grid_fb): requested by mtfhip_grid_frame_fb around its track call */
	/* set by a fused grid re-initialisation (grid_reinit_fused: identity warps, zero states, corners = the templates' corners on host AND device),
	 * cleared by whatever changes the mirrors' warps / states / corners next (set_corners_core, apply_states) and consumed by the next track_core:
	 * its one-launch kernel then starts from init_corners_hm and the slab is not uploaded (TrackState::fresh_reset) */
	bool fresh_reinit = false;
	bool fb_fused_req = false, fb_fused_reinit = true;
	Pinned<double, hipHostMallocMapped> h_fb;
	double *h_fb_dev = nullptr;
	Dev<double> d_fb;   /* [B][9] the backward pass's corners | iteration count: pinned host copy, device copy */
	Dev<double> d_nn_warps;   /* NN dataset, tolerance mode: the samples' warps between k_nn_warps and k_nn_rows */
	Dev<double> d_lm;       /* [B][kLmStride] Levenberg-Marquardt state of the device-side loop */
	Dev<double> d_trace; int trace_cap = 0;   /* [B][trace_cap][kTraceStride] debug trace of the device-side loop, or NULL */
	/* NCC: a fused iteration updated the scalars (It_mean, a, b, f) on the host only; the un-fused kernels read d_ncc */
	bool ncc_host_newer = false;
	/* mtfhip_grid_frame behind a fused re-initialisation (reset-every-frame mode): the loop kernel is ENQUEUED behind k_template_init instead
	 * of the host first waiting for that kernel's record and folding 1 KB per patch into its mirrors -- lazy_flush leaves the record
	 * pending while this is set, and the slab upload of the call leaves the device's NCC scalars (the kernel's own) alone */
	bool hold_init_pull = false;
	size_t slab_bytes = 0, slab_dbl_bytes = 0;
	Pinned<double, hipHostMallocMapped | hipHostMallocCoherent> h_acc;
	/* Zero-copy read-back of the reduced rows: h_acc is host-coherent pinned memory the reduction kernel writes directly
	 * (h_acc_dev = its device address) followed by a sequence number in h_flag; the host spins on the flag instead of
	 * paying a copy command plus a stream synchronisation per iteration (MTFHIP_ZERO_COPY=0: copy + sync) */
	double *h_acc_dev = nullptr;
	Pinned<unsigned long long, hipHostMallocMapped | hipHostMallocCoherent> h_flag;
	unsigned long long *h_flag_dev = nullptr, acc_seq = 0;
	char *h_stage_a_dev = nullptr, *h_stage_b_dev = nullptr;   /* device addresses of the staging buffers when kernels may read them (k_ingest_host), else NULL */
	Pinned<char, hipHostMallocMapped | hipHostMallocCoherent> h_pub;
	char *h_pub_dev = nullptr;   /* host-coherent mirror of the state slab, written by k_publish_host (track's read-back) */
	Dev<int> d_fin_count;
	int nblk_max;
	int unit_z = 1;
	/* INIT_PTS is the lattice set_corners (or the grid kernel's region mode) laid out INSIDE init_corners: what lets the candidate scorer
	 * trust the corners as the hull of the sample points.  Cleared when the caller writes a grid of its own (mtfhip_batch_write /
	 * mtfhip_batch_device_ptr of INIT_PTS / INIT_HXY / INIT_Z). */
	bool grid_from_corners = false;
	/* a deferred affine reset whose host half is still to be written (set_corners_core / set_corners_finish_deferred): the caller's
	 * corners, valid for the duration of the C-ABI call that deferred them */
	const double *deferred_corners = nullptr;
	bool deferred_for_track = false;
	/* mtfhip_grid_frame, fixed-size patches (r05): the kernel lays its patches out itself from the grid's region (RegionIngest::layout),
	 * so the HOST layout -- for the mirrors, the staged slab and the template-grid comparison -- is also deferred behind the launch:
	 * set_corners_finish_deferred runs mtfhip_grid_layout into deferred_patches first */
	bool deferred_layout = false, deferred_template_check = false;
	mtfhip_grid_desc deferred_gdesc{};
	double deferred_region[8] = {0, 0, 0, 0, 0, 0, 0, 0}, deferred_region_map[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	std::vector<double> deferred_patches;
	bool have_corners = false, init_pix_vals = false, init_pix_grad = false, init_sim = false, init_grad = false;
	bool it_valid = false, dit_valid = false, jt_valid = false;
	std::vector<TargetHost> th;

	/* Deferred fusion of the per-function entry points (SSD, single channel; DESIGN.md "drop-in path").  The pixel-level
	 * producers of an iteration (updatePixVals, updatePixGrad, cmpt*PixJacobian, updateSimilarity, update*Grad,
	 * mean Jacobian) only RECORD themselves; the first call that needs a number on the host (cmpt*Jacobian) runs the
	 * fused kernel with materialize=1 when the recorded set is one of the ESM / FCLK / ICLK call sequences, and every
	 * other entry point first replays what is pending through the un-fused kernels, in the recorded order -- so the
	 * buffers and results are those of the call-by-call execution either way. */
	struct Lazy {
		bool enabled = false;
		long seq = 0;
		long pv = 0;            /* update_pix_vals(NULL) */
		long gp = 0;            /* ssm_update_grad_pts(grad_eps) */
		long pg = 0; int pg_kind = 0;   /* update_pix_grad(NULL) = 1, update_pix_grad_warped(NULL) = 2 */
		long pj = 0; int pj_variant = -1;   /* ssm_cmpt_pix_jacobian(variant, DIT_DX -> JT) */
		long sim = 0, cg = 0, ig = 0, jm = 0;
		bool any() const { return pv || gp || pg || pj || sim || cg || ig || jm; }
		bool sim_need_f = false;
		/* DF_DI0 (updateSimilarity) / DF_DIT (updateCurrGrad) were skipped by a fused launch: refreshed from IT / I0 on
		 * first use, and in any case before IT is overwritten by something that does not overwrite them as well */
		bool df0_stale = false, dft_stale = false;
		/* ...and when IT has to change first, the old IT is kept instead of being consumed: the launch writes the other
		 * of two IT buffers (pointer swap, no copy) and the stale vector remembers that it refers to the shadow */
		bool df0_sh = false, dft_sh = false, shadow_valid = false;
		struct NccSave { double It_mean, a, b, f; };
		std::vector<NccSave> ncc_shadow;   /* NCC scalars that belong to the shadow IT */
		bool no_cache = false;
		/* Levenberg-Marquardt reads f in the middle of the iteration (NT/ESM.cc:186-204), which replays updatePixVals +
		 * updateSimilarity un-fused; the fused launch may still serve the rest when IT and DF_DI0 are known to belong to
		 * the current warp and image (it recomputes the same IT bits): epoch counts warp / image changes */
		long epoch = 0, it_epoch = -1, df0_it_ver = -1;
		/* NCC: the moment rows of the last fused launch ([B][NCC_ACC_COUNT]); Hessian requests are answered from them while
		 * IT and the Jacobian they were taken from are unchanged.  ncc_tm_ver: J0 version of the template moments. */
		std::vector<double> ncc_M; bool ncc_M_mean = false; long ncc_M_it = -1, ncc_M_jt = -1, ncc_M_jm = -1, ncc_tm_ver = -1;
		/* SSD: sum r J0 of the lean launch that served getSimilarity() -- it IS cmptInitJacobian(J0) for this IT and J0 */
		std::vector<double> sim_g; long sim_g_it = -1, sim_g_j0 = -1;
		/* MI: IT version the self joint histogram / its factor table belong to, and whether the search method has been
		 * asking for the self Hessian (then the fused histogram pass takes the self histogram along) */
		long mi_self_it = -1; bool mi_want_self = false;
		/* Gram matrices that are already on the host: [B][36] upper triangles, valid while version matches */
		long ver[MTFHIP_BUF_COUNT] = {0};
		int gram_buf = -1; long gram_ver = -1; std::vector<double> gram;
		long gram0_ver = -1; std::vector<double> gram0;   /* J0: constant between template changes */
	} lz;

	/* Single-target batches (the literal drop-in shape): set_state / compositional_update only mark the device copy of the warp
	 * stale.  The fused launch that normally follows carries the warp in its kernel arguments (fused_view) and refreshes the
	 * device copy itself; anything else that builds a BatchView uploads it first (view).  MTFHIP_INLINE_WARP=0: always upload. */
	mutable bool warps_dirty = false;
	bool inline_warp_ok = false;
	BatchView view() const {
		if (warps_dirty) { warps_dirty = false; (void)push_warps(const_cast<mtfhip_batch *>(this)); }
		return view_raw();
	}
	BatchView view_raw() const {
		BatchView v;
		v.B = B; v.N = N; v.S = S; v.ssm = desc.ssm; v.am = desc.am; v.unit_z = unit_z; v.NP = NP; v.C = C;
		for (int i = 0; i < MTFHIP_BUF_COUNT; ++i) v.buf[i] = buf[i];
		v.warps = d_warps; v.states = d_states;
		return v;
	}
};

static int ensure_buf(mtfhip_batch *b, int id) {
	if (b->buf[id]) return MTFHIP_OK;
	HIP_TRY(b->buf[id].reserve(b->per_target[id] * b->B));
	HIP_TRY(hipMemsetAsync(b->buf[id], 0, sizeof(double) * b->per_target[id] * b->B, b->ctx->stream));
	return MTFHIP_OK;
}

/* the second-order term's block rows and [B][64] sums (k_second_order_ssd, k_weighted_plane_sum), allocated by the first call that needs them */
static int ensure_second_order_scratch(mtfhip_batch *b) {
	HIP_TRY(b->d_d2_part.reserve(64 * (size_t)simple_blocks_per_target(b->N) * b->B));
	HIP_TRY(b->d_d2_out.reserve(64 * (size_t)b->B));
	return MTFHIP_OK;
}

/* A fused entry point of a low-order SSM works on the batch as an affine one (mtfhip_batch::lo_ssm): the guard turns it into that for its
 * scope and back.  Nothing for homography / affine batches, and nothing when an outer scope already holds it. */
struct PassMode {
	mtfhip_batch *b;
	bool on;
	explicit PassMode(mtfhip_batch *b_) : b(b_), on(b_ && b_->lo_ssm && !b_->pass_mode) { if (on) flip(); }
	~PassMode() { if (on) flip(); }
	PassMode(const PassMode &) = delete;
	PassMode &operator=(const PassMode &) = delete;
	void flip() {
		static const int ids[3] = {MTFHIP_BUF_J0, MTFHIP_BUF_JT, MTFHIP_BUF_JM};
		for (int k = 0; k < 3; ++k) { b->buf[ids[k]].swap(b->pass_j[k]); std::swap(b->per_target[ids[k]], b->pass_j_per_target[k]); }
		b->pass_mode = !b->pass_mode;
		b->S = b->pass_mode ? 6 : ssm_state_size(b->lo_ssm);
		b->desc.ssm = b->pass_mode ? (int)MTFHIP_SSM_AFFINE : b->lo_ssm;
	}
};
/* what a low-order SSM is not served with: the entry point fn returns MTFHIP_ERR_NOT_IMPLEMENTED before any kernel of its own could read a
 * six- or eight-wide state */
static inline int lowdof_refuse(const mtfhip_batch *b, const char *fn) {
	if (!b || !b->lo_ssm) return MTFHIP_OK;
	return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: not available with the %s state space model (Similitude, Isometry and Translation are served by the "
		"StateSpaceModel and AppearanceModel entry points and by init_template / set_region / iterate / track / track_region with ESM, FCLK and ICLK, "
		"first-order Hessians)", fn, ssm_name(b->lo_ssm));
}
/* the affine pass of a low-order SSM reads the six-column template copy init_template / set_region left in scratch: a caller who has since
 * written the interface's N x S template Jacobian (mtfhip_batch_write, mtfhip_ssm_cmpt_pix_jacobian into J0) has a template the pass does not see */
static inline int lowdof_template_current(const mtfhip_batch *b, const char *fn) {
	if (b && b->lo_ssm && b->init_pix_vals && !b->j0_is_template)
		return fail(MTFHIP_ERR_LOGIC, "%s: the template Jacobian of this %s batch was overwritten since init_template / set_region; the fused path "
			"keeps its own affine-coordinate copy: call one of them again", fn, ssm_name(b->lo_ssm));
	return MTFHIP_OK;
}
/* the state as the device slab holds it: the SSM's own, or for a low-order SSM the affine embedding of its warp (BatchView::states) */
static inline void slab_state(const mtfhip_batch *b, const TargetHost &h, double *s8) {
	if (!b->lo_ssm) { std::memcpy(s8, h.state, sizeof(double) * 8); return; }
	const double *W = h.warp.m;
	s8[0] = W[2]; s8[1] = W[5]; s8[2] = W[0] - 1; s8[3] = W[1]; s8[4] = W[3]; s8[5] = W[4] - 1; s8[6] = s8[7] = 0;
}
/* host state of every target -> one staging image of the slab */
static void fill_stage(const mtfhip_batch *b, char *stage, const double *w0 /* [B][9] or NULL */, int active, bool zero_iters) {
	const size_t Bt = (size_t)b->B;
	double *p = reinterpret_cast<double *>(stage);
	double *w = p, *s = p + 9 * Bt, *cr = p + 17 * Bt, *ic = p + 25 * Bt, *nc = p + 37 * Bt, *pw0 = p + 45 * Bt;
	int *act = reinterpret_cast<int *>(stage + b->slab_dbl_bytes), *it = act + Bt;
	for (int t = 0; t < b->B; ++t) {
		const TargetHost &h = b->th[t];
		std::memcpy(w + 9 * t, h.warp.m, sizeof(double) * 9);
		slab_state(b, h, s + 8 * t);
		std::memcpy(cr + 8 * t, h.corners, sizeof(double) * 8);
		std::memcpy(ic + 12 * t, h.init_corners_hm, sizeof(double) * 12);
		double *q = nc + 8 * t;
		q[0] = h.I0_mean; q[1] = h.c; q[2] = h.It_mean; q[3] = h.b; q[4] = h.f; q[5] = h.gmean; q[6] = h.i0_ss; q[7] = 0;
		if (w0) std::memcpy(pw0 + 9 * t, w0 + 9 * t, sizeof(double) * 9);
		act[t] = active;
		if (zero_iters) it[t] = 0;
	}
}

static int push_warps(mtfhip_batch *b) {
	const int k = b->wflip; b->wflip ^= 1;
	HIP_TRY(hipEventSynchronize(b->ev_w[k]));   /* the copy that last read this buffer (two updates ago) is long done */
	double *w = b->h_wstage[k], *s = w + 9 * (size_t)b->B;   /* d_states follows d_warps in the slab */
	for (int t = 0; t < b->B; ++t) {
		std::memcpy(&w[9 * t], b->th[t].warp.m, sizeof(double) * 9);
		slab_state(b, b->th[t], &s[8 * t]);
	}
	HIP_TRY(hipMemcpyAsync(b->d_warps, w, sizeof(double) * 17 * (size_t)b->B, hipMemcpyHostToDevice, b->ctx->stream));
	HIP_TRY(hipEventRecord(b->ev_w[k], b->ctx->stream));
	return MTFHIP_OK;
}

/* the BatchView of a fused launch: a stale single-target warp goes into the kernel arguments instead of being uploaded */
/* SCV and LSCV are SSD on a re-mapped template, RSCV and LRSCV SSD on a mapped current patch: every SSD branch of the entry points serves
 * them */
static inline bool ssd_like(const mtfhip_batch *b) { return am_traits(b->desc.am).rows == AM_ROWS_SSD; }
/* SCV, RSCV, LSCV and LRSCV: an intensity map is rebuilt between the fused passes -- the one-launch, persistent and step loops do not take
 * them (fused_select, mtfhip_fused_dispatch.h) */
static inline bool intensity_mapped(const mtfhip_batch *b) { return am_traits(b->desc.am).intensity_mapped; }
/* the name of an intensity-mapped model, for the messages */
static inline const char *intensity_mapped_name(const mtfhip_batch *b) { return am_traits(b->desc.am).name; }
/* ... the localized ones (sub-regions, once_per_frame) and the reversed ones (the map is of the current patch) among them */
static inline bool imap_localized(const mtfhip_batch *b) { return am_traits(b->desc.am).localized; }
static inline bool imap_reversed(const mtfhip_batch *b) { return am_traits(b->desc.am).reversed; }
/* of the fused routes only the two-launch loop serves the model: the intensity-mapped ones (the template re-map / the current map runs
 * between the passes), SPSS (the one-launch kernels accumulate SSD's or NCC's sums) and SSIM (NCC's sums, but they solve NCC's system) */
static inline bool loop_only(const mtfhip_batch *b) { return am_traits(b->desc.am).loop_only; }
/* THE refusal of what depends on the model and the place (AM_AT_*) alone: the text of mtfhip_am_served.h for the entry point fn as
 * MTFHIP_ERR_NOT_IMPLEMENTED, MTFHIP_OK where the model is served (and for a NULL batch: the entry point's own check reports it) */
static inline int am_refuse(int am, const char *fn, int place, const char *extra = nullptr) {
	char text[kErrMsgCap];
	return am_refused(am, place, fn, extra, text, sizeof(text)) ? fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s", text) : MTFHIP_OK;
}
static inline int am_refuse(const mtfhip_batch *b, const char *fn, int place, const char *extra = nullptr) {
	return b ? am_refuse(b->desc.am, fn, place, extra) : MTFHIP_OK;
}
/* SPSS: a model of its own -- no SSD branch serves it, and of the fused routes only the two-launch loop does (fused_select) */
static inline bool spss_am(const mtfhip_batch *b) { return b->desc.am == MTFHIP_AM_SPSS; }
/* api_spss.hip.  spss_args: what a fused launch for the search method sm reads beside FusedArgs; SPSS's row of kAmOps (and
 * spss_weighted_hessian: weight SPSS_W_*) */
mtfhip::SpssArgs spss_args(const mtfhip_batch *b, const mtfhip_sm_desc *sm);
int spss_initialize_similarity(mtfhip_batch *b);
int spss_update_similarity(mtfhip_batch *b, int prereq_only);
int spss_update_grad(mtfhip_batch *b, int which);
int spss_weighted_hessian(mtfhip_batch *b, int j_buf, int weight, double *H);
int spss_hessian(mtfhip_batch *b, int j_buf, int kind, double *H);
int spss_likelihood(const mtfhip_batch *b, int t, double *l);
/* SSIM: every quantity of SSIM.cc is a function of the raw moments an NCC pass reduces (mtfhip_sm_system.h), so an SSIM batch launches NCC's
 * pass kernels (fused_select) on the two-launch loop, and its own finish (kernels_ssim.hip) */
static inline bool ssim_am(const mtfhip_batch *b) { return b->desc.am == MTFHIP_AM_SSIM; }
/* THE predicate of "this batch's fused passes reduce NCC's rows": the 72-wide partial / reduced row, the template moments th[].ncc_tm and their
 * upload d_ncc_tm, the per-target scalars d_ncc and their refresh.  (What solves NCC's own system -- the one-launch, step and persistent
 * kernels, the fused template initialisation, the second-order pass, the deferred-fusion layer -- asks for MTFHIP_AM_NCC by name.) */
static inline bool ncc_rows(const mtfhip_batch *b) { return am_traits(b->desc.am).rows == AM_ROWS_NCC; }
/* api_ssim.hip.  ssim_h0: the constant self Hessian from the template's moments (th[].ncc_tm must be current); SSIM's row of kAmOps
 * (its initializeSimilarity is NCC's, its likelihood NCC's form) */
int ssim_h0(const mtfhip_batch *b, double *H0);
int ssim_update_similarity(mtfhip_batch *b, int prereq_only);
int ssim_update_grad(mtfhip_batch *b, int which);
int ssim_hessian(mtfhip_batch *b, int j_buf, int kind, double *H);
/* CCRE (api_ccre.hip): MI's materialising iteration with cumulative weights on the current patch's side, in the buffers an MI batch has.
 * hist_am: the models whose iteration is a histogram pipeline of its own behind a materialising SSD pass (mi_enqueue / ccre_enqueue) and whose
 * device loop is their own driver (MI and CCRE).  CCRE's row of kAmOps follows */
static inline bool ccre_am(const mtfhip_batch *b) { return b->desc.am == MTFHIP_AM_CCRE; }
static inline bool hist_am(const mtfhip_batch *b) { return am_traits(b->desc.am).hist_driver; }
int ccre_initialize_similarity(mtfhip_batch *b);
int ccre_update_similarity(mtfhip_batch *b, int prereq_only);
int ccre_grad(mtfhip_batch *b, int which);
int ccre_hessian(mtfhip_batch *b, int j_buf, int kind, double *H);
int ccre_likelihood(const mtfhip_batch *b, int t, double *l);
/* What differs by model at the per-function AppearanceModel entry points (api_am.hip: kAmOps, one row per MTFHIP_AM_*):
 * initializeSimilarity (the model's own reads init_sim; the entry point sets it); updateSimilarity; grad, which 0 updateInitGrad into DF_DI0,
 * 1 updateCurrGrad into DF_DIT, 2 initializeGrad into both (the entry point asks once per batch); cmptInitHessian / cmptCurrHessian /
 * cmptSelfHessian, kind 0 / 1 / 2, into H [B][S x S]; getLikelihood of target t from th[t].f, no launch.  A null entry: the SSD body of
 * the entry point -- SSD and the SCV family */
struct AmOps {
	int (*initialize_similarity)(mtfhip_batch *b);
	int (*update_similarity)(mtfhip_batch *b, int prereq_only);
	int (*grad)(mtfhip_batch *b, int which);
	int (*hessian)(mtfhip_batch *b, int j_buf, int kind, double *H);
	int (*likelihood)(const mtfhip_batch *b, int t, double *l);
};
const AmOps &am_ops(const mtfhip_batch *b);
/* one target's reduced NCC row and template mirrors as the SSIM system of mtfhip_sm_system.h; and the host mirrors of SSIM.cc's members it leaves */
static inline mtfhip::SsimSys ssim_host_sys(const mtfhip_batch *b, const TargetHost &h, const double *M) {
	return mtfhip::ssim_sys(M, h.ncc_tm, h.I0_mean, h.i0_ss, (double)b->N, b->ssim_c1, b->ssim_c2);
}
static inline void ssim_refresh_mirrors(TargetHost &h, const mtfhip::SsimSys &q, const double *M) {
	h.It_mean = q.mt; h.it_ss = M[mtfhip::NCC_IT2] - q.N * q.mt * q.mt; h.a = M[mtfhip::NCC_I0IT] - q.N * q.m0 * q.mt; h.f = q.f;
}
/* api_imap.hip, the SCV family's hooks; each does nothing for a model outside the family.
 * imap_capture (initializePixVals): the template's code plane, I0_orig / It_orig, the identity maps, the localized models' geometry.
 * imap_before_pass: what the model runs in front of a pixel pass over the targets [t0, t0 + chunk->B) (chunk NULL: the whole batch) on st -- SCV / LSCV re-map I0 (from_it 1:
 * from MTFHIP_BUF_IT, the per-function route; 0: sampled at the current warp); with fa, the fused launch that follows, RSCV / LRSCV run pass 1
 * + the maps and hand what that launch applies to *out (without fa they have nothing to do: their updatePixVals has mapped It).
 * first_pass: the localized models under once_per_frame map in front of the first pass of a frame only.
 * imap_update_pix_vals: the per-function updatePixVals of RSCV / LRSCV, IMAP_NOT_MINE for every other model */
enum { IMAP_NOT_MINE = 1 };
int imap_capture(mtfhip_batch *b);
int imap_before_pass(mtfhip_batch *b, const BatchView *chunk, int t0, const int *active, const FusedArgs *fa, int from_it, bool first_pass,
	hipStream_t st, FusedMaps *out);
int imap_update_pix_vals(mtfhip_batch *b, const double *dp);
static inline BatchView fused_view(mtfhip_batch *b, FusedArgs &fa) {
	fa.inline_warp = 0;
	if (b->warps_dirty && b->B == 1) {
		b->warps_dirty = false;
		fa.inline_warp = 1;
		std::memcpy(fa.iw, b->th[0].warp.m, sizeof(double) * 9);
		std::memcpy(fa.is, b->th[0].state, sizeof(double) * 8);
		return b->view_raw();
	}
	return b->view();
}
/* corners = dehomogenise(curr_warp * init_corners_hm) (Homography.cc:87-90) / affine top rows (Affine.cc:105) */
static void update_corners(mtfhip_batch *b, int t) {
	TargetHost &h = b->th[t];
	for (int q = 0; q < 4; ++q) {
		const double *c = &h.init_corners_hm[3 * q];
		const double *W = h.warp.m;
		double x = W[0] * c[0] + W[1] * c[1] + W[2] * c[2];
		double y = W[3] * c[0] + W[4] * c[1] + W[5] * c[2];
		if (b->desc.ssm == MTFHIP_SSM_HOMOGRAPHY) {
			double d = W[6] * c[0] + W[7] * c[1] + W[8] * c[2];
			x = x / d; y = y / d;
		}
		h.corners[2 * q] = x; h.corners[2 * q + 1] = y;
	}
}

int launch_error_pending();   /* api_core.hip: the sticky status of MTFHIP_LAUNCH, cleared when reported */
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
	__builtin_ia32_pause();
#elif defined(__aarch64__)
	__asm__ __volatile__("yield");
#endif
}
/* wait until the kernel that was given `seq` has stored it behind its host-coherent writes.  The kernel normally reports within a
 * few microseconds of the launch that precedes this call, so the wait starts as a spin; when the stream is busy with longer
 * work (a whole device-side loop: tens to hundreds of microseconds) the spin gives the core away between polls after 200 us,
 * and after 50 ms the runtime's blocking synchronisation takes over (it costs ~100 us of its own, hence not earlier). */
static int wait_host_flag(mtfhip_batch *b, unsigned long long seq) {
	TRY(launch_error_pending());
	const auto t0 = std::chrono::steady_clock::now();
	bool yielding = false;
	for (unsigned spins = 0;; ++spins) {
		if (__atomic_load_n(b->h_flag.get(), __ATOMIC_ACQUIRE) == seq) return MTFHIP_OK;
		if (yielding) std::this_thread::yield(); else cpu_relax();
		if ((spins & 0x3ff) == 0x3ff || yielding) {
			const auto dt = std::chrono::steady_clock::now() - t0;
			if (dt > std::chrono::milliseconds(50)) break;
			if (dt > std::chrono::microseconds(1000)) yielding = true;
		}
	}
	/* the kernel did not report in: let the runtime tell why */
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	if (__atomic_load_n(b->h_flag.get(), __ATOMIC_ACQUIRE) == seq) return MTFHIP_OK;
	return fail(MTFHIP_ERR_HIP, "device results were not delivered to host memory");
}
/* fold the record of a fused template initialisation into the host mirrors (see mtfhip_batch::init_mirror_seq) */
static int pull_init_mirrors(mtfhip_batch *b) {
	if (!b->init_mirror_seq) return MTFHIP_OK;
	const bool ncc_am = b->desc.am == MTFHIP_AM_NCC;
	if (b->init_rec_device) {
		/* the kernel left its results on the device only (what it publishes otherwise is a copy of d_h0 | d_ncc | d_ncc_tm): three small copies and
		 * a synchronisation, paid by the rare caller that reads the mirrors behind a grid re-initialisation instead of by every frame */
		static thread_local std::vector<double> h0v, ncv, tmv;
		const size_t Bt = (size_t)b->B;
		h0v.resize(64 * Bt); ncv.resize(8 * Bt); tmv.resize(NCC_TM_COUNT * Bt);
		HIP_TRY(hipMemcpyAsync(h0v.data(), b->d_h0, sizeof(double) * 64 * Bt, hipMemcpyDeviceToHost, b->ctx->stream));
		if (ncc_am) {
			HIP_TRY(hipMemcpyAsync(ncv.data(), b->d_ncc, sizeof(double) * 8 * Bt, hipMemcpyDeviceToHost, b->ctx->stream));
			HIP_TRY(hipMemcpyAsync(tmv.data(), b->d_ncc_tm, sizeof(double) * NCC_TM_COUNT * Bt, hipMemcpyDeviceToHost, b->ctx->stream));
		}
		HIP_TRY(hipStreamSynchronize(b->ctx->stream));
		for (int t = 0; t < b->B; ++t) {
			TargetHost &h = b->th[t];
			std::memcpy(h.h0, &h0v[64 * (size_t)t], sizeof(double) * 64);
			if (ncc_am) {
				const double *r = &ncv[8 * (size_t)t], *m = &tmv[NCC_TM_COUNT * (size_t)t];
				h.I0_mean = r[0]; h.c = r[1]; h.It_mean = r[2]; h.b = r[3]; h.f = r[4]; h.gmean = r[5];
				std::memcpy(h.ncc_tm, m, sizeof(double) * NCC_TM_COUNT);
			}
		}
		b->init_mirror_seq = 0; b->init_rec_device = false;
		return MTFHIP_OK;
	}
	const unsigned long long seq = b->init_mirror_seq;
	const auto t0 = std::chrono::steady_clock::now();
	bool ok = false;
	for (unsigned spins = 0;; ++spins) {
		if (__atomic_load_n(b->h_init_flag.get(), __ATOMIC_ACQUIRE) == seq) { ok = true; break; }
		cpu_relax();
		if ((spins & 0x3ff) == 0x3ff && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
	}
	if (!ok) {
		HIP_TRY(hipStreamSynchronize(b->ctx->stream));
		if (__atomic_load_n(b->h_init_flag.get(), __ATOMIC_ACQUIRE) != seq) return fail(MTFHIP_ERR_HIP, "the template initialisation's results were not delivered to host memory");
	}
	const bool ncc = b->desc.am == MTFHIP_AM_NCC;
	for (int t = 0; t < b->B; ++t) {
		const double *r = b->h_init_rec + (size_t)t * mtfhip::kInitRec;
		TargetHost &h = b->th[t];
		std::memcpy(h.h0, r, sizeof(double) * 64);
		if (ncc) {
			h.I0_mean = r[64]; h.c = r[65]; h.It_mean = r[66]; h.b = r[67]; h.f = r[68]; h.gmean = r[69];
			std::memcpy(h.ncc_tm, r + 72, sizeof(double) * NCC_TM_COUNT);
		}
	}
	b->init_mirror_seq = 0;
	return MTFHIP_OK;
}
/* fixed-order sum of the per-workgroup rows -> h_acc ([B][row_len]) on the host, and wait for it */
static int read_rows(mtfhip_batch *b, int nblk, int row_len) {
	if (b->h_acc_dev) {
		const unsigned long long seq = ++b->acc_seq;
		launch_finish_host(b->d_partials, nblk, row_len, b->h_acc_dev, b->d_fin_count, b->h_flag_dev, seq, b->B, b->ctx->stream);
		return wait_host_flag(b, seq);
	}
	if (row_len == ACC_COUNT) launch_finish(b->d_partials, nblk, b->d_acc, b->B, b->ctx->stream);
	else launch_finish_rows(b->d_partials, nblk, row_len, b->d_acc, b->B, b->ctx->stream);
	HIP_TRY(hipMemcpyAsync(b->h_acc, b->d_acc, sizeof(double) * row_len * b->B, hipMemcpyDeviceToHost, b->ctx->stream));
	HIP_TRY(hipStreamSynchronize(b->ctx->stream));
	return MTFHIP_OK;
}
static int read_acc(mtfhip_batch *b, int nblk) { return read_rows(b, nblk, ACC_COUNT); }

static int need_image(mtfhip_batch *b) {
	if (!b->ctx->img.data) return fail(MTFHIP_ERR_LOGIC, "no current image: call mtfhip_image_upload/borrow first");
	if (b->ctx->img.channels != b->C)   /* ImageBase::setCurrImg: "Input image type does not match the required type" */
		return fail(MTFHIP_ERR_INVALID_ARG, "ImageBase::setCurrImg::Input image has %d channel(s), the appearance model expects %d", b->ctx->img.channels, b->C);
	return MTFHIP_OK;
}
/* the fused, one-launch and candidate kernels are single-channel; MCSSD / MCNCC / MCMI go through the per-function entry points */
static int single_channel(const mtfhip_batch *b, const char *fn) {
	if (b->C != 1) return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: multi-channel appearance models use the per-function entry points", fn);
	return MTFHIP_OK;
}
static int j_buf_ok(int id) { return id == MTFHIP_BUF_J0 || id == MTFHIP_BUF_JT || id == MTFHIP_BUF_JM; }

/* resolves a `pts` argument: NULL -> the batch's own device buffer, else upload into scratch */
static int resolve_pts(mtfhip_batch *b, const double *host, int own_buf, size_t per_target, const double **out) {
	if (!host) {
		if (!b->buf[own_buf]) return fail(MTFHIP_ERR_LOGIC, "device points not available yet");
		*out = b->buf[own_buf];
		return MTFHIP_OK;
	}
	HIP_TRY(hipMemcpyAsync(b->d_scratch_pts, host, sizeof(double) * per_target * b->B, hipMemcpyHostToDevice, b->ctx->stream));
	*out = b->d_scratch_pts;
	return MTFHIP_OK;
}

extern "C" {

/* ------------------------------------------------------------------ deferred fusion (see mtfhip_batch::Lazy) */
static inline void touch(mtfhip_batch *b, int id) { ++b->lz.ver[id]; }
static inline void touch_all(mtfhip_batch *b) { for (int i = 0; i < MTFHIP_BUF_COUNT; ++i) ++b->lz.ver[i]; }
int lazy_flush(mtfhip_batch *b, bool pts = true);
int ensure_df(mtfhip_batch *b);
/* what an entry point that rewrites the batch's arrays does behind its FLUSH / FLUSH_AM: every cached version is void */
static inline int begin_entry(mtfhip_batch *b) {
	if (b) { touch_all(b); b->lz.it_epoch = -1; TRY(ensure_df(b)); }
	return MTFHIP_OK;
}
int do_cmpt_pix_jacobian(mtfhip_batch *b, int variant, int grad_buf, int dst_buf);
static int lazy_flush_ctx(mtfhip_ctx *c) {   /* called by everything that replaces the current image */
	for (mtfhip_batch *b : c->batches) {
		/* the record of a fused template initialisation does not depend on the image any more (d_h0 / d_ncc / d_ncc_tm are written): with no
		 * recorded interface calls to replay it stays pending -- a reset-every-frame video loop (setImage, update, reset) would otherwise pay
		 * three device-to-host copies and a synchronisation per frame for mirrors the next re-initialisation supersedes unread */
		const bool hold = b->hold_init_pull;
		if (!b->lz.any()) b->hold_init_pull = true;
		const int rc = lazy_flush(b, false);   /* (pts = false: the current points follow the warp when an un-fused kernel next asks -- refreshing them at every setImage was one k_apply_warp launch per frame of a video loop; recorded calls that read them refresh them inside) */
		b->hold_init_pull = hold;
		if (rc) return rc;
		++b->lz.epoch;
	}
	return MTFHIP_OK;
}
#define FLUSH(b) do { if (b) { int _rc = lazy_flush(b); if (_rc) return _rc; } } while (0)
/* for entry points whose own kernels never read the current points (the AM's reductions over It / I0 / J buffers) */
#define FLUSH_AM(b) do { if (b) { int _rc = lazy_flush(b, false); if (_rc) return _rc; } } while (0)

/* MI gradient pass: rebuild the template rows instead of reading J0, under the conditions of FusedArgs::j0_recompute
 * (J0 is the search method's own template Jacobian on the current grid) */
static inline mtfhip::MiJ0Rebuild mi_j0_rebuild(const mtfhip_batch *b) {
	mtfhip::MiJ0Rebuild rb{nullptr, nullptr, nullptr, 0, 0};
	const bool ok = b->C == 1 && b->j0_is_template && b->j0_recompute_enabled && b->j0_template_corners_epoch == b->corners_epoch &&
		b->buf[MTFHIP_BUF_DI0_DX] && b->buf[MTFHIP_BUF_INIT_PTS] && (b->unit_z || b->buf[MTFHIP_BUF_INIT_Z]);
	if (ok) {
		rb.dI0 = b->buf[MTFHIP_BUF_DI0_DX]; rb.pts = b->buf[MTFHIP_BUF_INIT_PTS];
		rb.z = b->unit_z ? nullptr : b->buf[MTFHIP_BUF_INIT_Z];
		rb.hom = b->desc.ssm == MTFHIP_SSM_HOMOGRAPHY; rb.init_variant = b->j0_variant == MTFHIP_JAC_INIT;
	}
	return rb;
}

/* the template lattice's extents and resolution as the kernels that lay a grid out themselves take them (set_corners_core's extents:
 * ProjectiveBase.cc:14, Affine.cc:56-57); everything else of the record is zero */
static inline mtfhip::RegionIngest region_geometry(const mtfhip_batch *b) {
	/* (the model itself, also while a fused entry point has the batch in its affine form: PassMode) */
	const int ssm = b->lo_ssm ? b->lo_ssm : b->desc.ssm;
	const bool homg = ssm == MTFHIP_SSM_HOMOGRAPHY;
	const bool unit_sq = homg || ssm == MTFHIP_SSM_ISOMETRY || ssm == MTFHIP_SSM_TRANSLATION;   /* (set_corners_core's unit_square) */
	mtfhip::RegionIngest rg{};
	rg.lo_x = unit_sq ? -0.5 : 1 - b->desc.resx / 2.0; rg.lo_y = unit_sq ? -0.5 : 1 - b->desc.resy / 2.0;
	rg.hi_x = unit_sq ? 0.5 : b->desc.resx / 2.0; rg.hi_y = unit_sq ? 0.5 : b->desc.resy / 2.0;
	rg.resx = b->desc.resx; rg.resy = b->desc.resy; rg.force_unit_z = homg ? 0 : 1;
	return rg;
}
/* ... and the deferred layout (b->deferred_gdesc / _region_map): the kernel lays its patches out itself from the grid's region */
static inline void region_deferred_layout(const mtfhip_batch *b, mtfhip::RegionIngest &rg) {
	const mtfhip_grid_desc &gd = b->deferred_gdesc;
	rg.layout = 1;
	rg.grid = mtfhip::GridLayoutHD{gd.grid_size_x, gd.grid_size_y, gd.patch_size_x, gd.patch_size_y, gd.dyn_patch_size ? 1 : 0, gd.patch_centroid_inside ? 1 : 0};
	std::memcpy(rg.region_map, b->deferred_region_map, sizeof(rg.region_map));
}

/* ---- functions defined in one api_*.hip unit and used in another ---- */
enum { LAZY_CURR_JAC = 0, LAZY_DIFF_JAC = 1, LAZY_INIT_JAC = 2 };
int ensure_pts(mtfhip_batch *b);
const float *ensure_pair_image(mtfhip_ctx *c);   /* NULL: not applicable (borrowed / multi-channel / too large / MTFHIP_PAIR_IMAGE=0) */
const float *pair_image_if_it_pays(mtfhip_ctx *c, int n_candidates);
int set_corners_core(mtfhip_batch *b, const double *corners, bool for_track, bool defer_grid = false, bool layout_later = false);   /* api_core.hip */
void set_corners_finish_deferred(mtfhip_batch *b);
int do_update_grad_pts(mtfhip_batch *b, double grad_eps);
/* api_am.hip: the executors of the per-function calls the deferred layer records and replays (do_*, pix_grad_common), the gradient vectors'
 * common start, the Jacobian product */
int do_update_pix_vals(mtfhip_batch *b, const double *pts);
int pix_grad_common(mtfhip_batch *b, const double *pts, bool warped, bool init);
int do_update_similarity(mtfhip_batch *b, int prereq_only);
int do_update_curr_grad(mtfhip_batch *b);
int do_mean_jacobian(mtfhip_batch *b);
int zero_grad_vectors(mtfhip_batch *b);
int gemv_to_host(mtfhip_batch *b, const double *v1, int j1, const double *v2, int j2, int sum_mode, double *g, int diff);
/* api_lazy.hip (stale_clear: df_dI0 / df_dIt have just been written for the current IT; ensure_one: df_dI0 (curr 0) / df_dIt (1) derived if a
 * fused launch skipped it; protect_stale: see there; lazy_try_fused: trig LAZY_*, *done = 1 when one fused launch served the request) */
void stale_clear(mtfhip_batch *b, bool df0, bool dft);
int ensure_one(mtfhip_batch *b, bool curr);
int protect_stale(mtfhip_batch *b, bool w0, bool wt);
int lazy_try_fused(mtfhip_batch *b, int trig, int j_a, int j_b, double *g, int *done);
int lazy_try_similarity(mtfhip_batch *b);
/* api_mi.hip: MI's row of kAmOps, the pixel weights of its second-order self Hessian (into d_d2_w), its half of the deferred layer */
int mi_blocks(const mtfhip_batch *b);
int mi_initialize_similarity(mtfhip_batch *b);
int mi_update_similarity(mtfhip_batch *b, int prereq_only);
int mi_grad(mtfhip_batch *b, int which);
int mi_hessian(mtfhip_batch *b, int j_buf, int kind, double *H);
int mi_self_weight(mtfhip_batch *b);
int mi_lazy_similarity(mtfhip_batch *b);
int mi_lazy_fused(mtfhip_batch *b, int trig, int j_a, const mtfhip_sm_desc &sm, bool replay, double *g, int *done);
/* api_ncc.hip: NCC's row of kAmOps (ncc_initialize_similarity is SSIM's too); push_ncc: the host scalars -> d_ncc; the moment forms of the
 * fused path (ncc_host_sys: one target's reduced row and template mirrors as the NCC system of mtfhip_sm_system.h; ncc_refresh_mirrors: its
 * scalars -> It_mean / b / a / f) */
int push_ncc(mtfhip_batch *b);
int ncc_initialize_similarity(mtfhip_batch *b);
int ncc_update_similarity(mtfhip_batch *b, int prereq_only);
int ncc_grad(mtfhip_batch *b, int which);
int ncc_hessian(mtfhip_batch *b, int j_buf, int kind, double *H);
int ncc_template_moments(mtfhip_batch *b);
int ncc_lazy_outputs(mtfhip_batch *b, int trig, int j_a, bool hess_mean, double *g);
int ncc_hessian_from_cache(mtfhip_batch *b, int j_buf, int kind, double *H);
static inline NccSys ncc_host_sys(const mtfhip_batch *b, const TargetHost &h, const double *M) { return ncc_sys(M, h.ncc_tm, h.I0_mean, h.c, (double)b->N); }
void ncc_refresh_mirrors(const mtfhip_batch *b, TargetHost &h, const double *M);
/* api_fused.hip (second_order_term: -1 for none; assemble_rows: every target's reduced row of an SSD-family / SPSS / NCC pass -> f, g and H;
 * store_h0: th[].h0, d_h0 and d_h0inv from H0 [B][S x S] -- enqueued only: the caller synchronises the stream before it returns) */
int check_sm(const mtfhip_batch *b, const mtfhip_sm_desc *sm, const char *fn);
bool template_init_fused_ok(const mtfhip_batch *b, const mtfhip_sm_desc *sm);
int init_template_fused(mtfhip_batch *b, const mtfhip_sm_desc *sm, const mtfhip::RegionIngest *rg = nullptr, bool publish_host = true);
int set_region_core(mtfhip_batch *b, const double *corners, const mtfhip_sm_desc *sm, bool for_track, bool defer_grid = false, bool layout_later = false);
static inline bool region_refreshes(const mtfhip_sm_desc *sm) { return sm->sm == MTFHIP_SM_ESM || (sm->sm == MTFHIP_SM_FCLK && sm->hess_type == 0); }
int fused_args(const mtfhip_batch *b, const mtfhip_sm_desc *sm, FusedArgs &fa);
int second_order_term(const mtfhip_sm_desc *sm, int am = MTFHIP_AM_SSD);
int assemble_rows(mtfhip_batch *b, const mtfhip_sm_desc *sm, bool hess_mean, int nblk, const double *so, double so_scale, double *f, double *g, double *H);
int store_h0(mtfhip_batch *b, const double *H0, bool with_inverse);
/* api_mi_iter.hip.  What an MI iteration of the search method needs from the AM (NT/ESM.cc:315-377, NT/FCLK.cc:262-283, NT/ICLK.cc:204-252) */
struct MiPlan {
	enum { H_CONST, H_SELF_JT, H_CURR_JT, H_CURR_JM, H_SUM_STD, H_INIT_J0 };
	int hk;
	bool iclk, esm, fclk, self, need_jt, orig_jac, need_mean;
	explicit MiPlan(const mtfhip_sm_desc *sm) {
		iclk = sm->sm == MTFHIP_SM_ICLK; esm = sm->sm == MTFHIP_SM_ESM; fclk = sm->sm == MTFHIP_SM_FCLK;
		const int ht = sm->hess_type;
		hk = ht == 0 ? H_CONST
			: esm ? (ht <= 2 ? H_SELF_JT : (ht == 3 ? H_CURR_JM : (ht == 4 ? H_SUM_STD : H_CURR_JT)))
			: fclk ? (ht == 1 ? H_SELF_JT : H_CURR_JT)
			: (ht == 1 ? H_SELF_JT : H_INIT_J0);
		self = hk == H_SELF_JT;                /* cmptSelfHessian(Jt): the self histogram rides along with pass 1 */
		need_jt = !iclk || self;               /* ICLK's CurrentSelf refreshes the current pixel Jacobian (NT/ICLK.cc:215-237) */
		orig_jac = esm && sm->jac_type == 0;   /* cmptCurrJacobian(mean Jacobian) */
		need_mean = orig_jac || hk == H_CURR_JM;
	}
};
int mi_iterate(mtfhip_batch *b, const mtfhip_sm_desc *sm, double *f, double *g, double *H);
/* api_track.hip.  What track_core hands its drivers: second-order term or -1, passes to enqueue, block rows of the second-order pass, ... */
/* fused_io: the chunked driver's one-launch head and in-loop delivery (track_core; MTFHIP_TRACK_FUSED_IO=0: the memsets, the copy and the
 * k_publish_host launch); words_ready: the head has set the loop's words (need_mat, d_phase, the Levenberg-Marquardt state) */
struct TrackCtx { int so_term, max_passes, nb2; bool resume, region_mode; bool fused_io = false, words_ready = false; };
int track_loop_mi(mtfhip_batch *b, const mtfhip_sm_desc *sm, mtfhip::TrackState &ts, const TrackCtx &cx);   /* (api_mi_iter.hip) */
int ccre_iterate(mtfhip_batch *b, const mtfhip_sm_desc *sm, double *f, double *g, double *H);                  /* (api_ccre.hip) */
int track_loop_ccre(mtfhip_batch *b, const mtfhip_sm_desc *sm, mtfhip::TrackState &ts, const TrackCtx &cx);
/* ... and the skeleton every device-side loop shares (track_core, alk_track): the upload of the state slab, the initial Levenberg-Marquardt
 * state, the look at the stop flags every eighth pass, the read-back of the slab, the tail of a loop that ran to its read-back */
int loop_upload_slab(mtfhip_batch *b, hipStream_t st, bool keep_ncc, const LoopWords *lw = nullptr);
int loop_lm_state(mtfhip_batch *b, const mtfhip_sm_desc *sm, hipStream_t st, double **lm);
bool loop_all_stopped(const mtfhip_sm_desc *sm, int max_passes, int it, const int *d_flags, int n, hipStream_t on, std::vector<int> &h_flags, hipError_t *err = nullptr);
int loop_read_back(mtfhip_batch *b, hipStream_t st, unsigned long long pub_seq, int *n_iters, double *corners, const char **h_res);
static inline void loop_done(mtfhip_batch *b) {
	b->pts_stale = true;       /* CURR_PTS follow the final warp when an un-fused kernel next needs them */
	b->stage_a_busy = false;   /* the results have arrived, so the head of the call has run (the stream has drained, or -- the chunked loop's
	                            * in-loop delivery -- all B targets have reported in): whatever set_corners staged has been consumed */
}
bool iclk_one_launch(const mtfhip_batch *b, const mtfhip_sm_desc *sm);
int track_validate(mtfhip_batch *b, const mtfhip_sm_desc *sm);
int track_region_impl(mtfhip_batch *b, const mtfhip_sm_desc *sm, const double *region_corners, int *n_iters, double *corners, const mtfhip_grid_desc *grid);
extern const bool g_track_dbg_timing;   /* MTFHIP_TRACK_DEBUG_TIMING: host-side stamps of the loop and the grid frames on stderr */
/* api_alk.hip: MTFHIP_SM_FALK / _IALK behind mtfhip_batch_init_template / _iterate / _track */
static inline bool alk_sm(int sm) { return sm == MTFHIP_SM_FALK || sm == MTFHIP_SM_IALK; }
/* ... which a low-order SSM is not served with: refused before anything else looks at the call */
static inline int lowdof_sm_refuse(const mtfhip_batch *b, const mtfhip_sm_desc *sm, const char *fn) {
	if (b && b->lo_ssm && sm && alk_sm(sm->sm))
		return fail(MTFHIP_ERR_NOT_IMPLEMENTED, "%s: the additive search methods (FALK / IALK) are not available with the %s state space model", fn, ssm_name(b->lo_ssm));
	return MTFHIP_OK;
}
int alk_init_template(mtfhip_batch *b, const mtfhip_sm_desc *sm);
int alk_iterate(mtfhip_batch *b, const mtfhip_sm_desc *sm, double *f, double *g, double *H);
int alk_track(mtfhip_batch *b, const mtfhip_sm_desc *sm, int *n_iters, double *corners);
/* api_cand.hip (peer: also store the weights to the other ranks' mailboxes) */
int nn_dataset_enqueue(mtfhip_batch *b, const mtfhip_nn_desc *d, const double *dev_perturbations_in, double *dev_perturbations_out, double *dev_features,
	int row_lo, int row_count, const double *base_dev, const int *done);
int score_block_dev(mtfhip_batch *b, const double *dev_states, int lo, int cnt, double *wts, double *sim, int likelihood_func,
	double measurement_sigma, double max_similarity, const mtfhip::PfPeerPush *peer = nullptr);
} /* extern "C" */
#endif
