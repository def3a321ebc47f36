/*
 * mtfhip_internal.h -- shared between the HIP kernel translation units (kernels_*.hip) and the C-ABI
 * implementation (the api_*.hip units).  Not installed; the public contract is include/mtfhip.h.
 */
#ifndef MTFHIP_INTERNAL_H
#define MTFHIP_INTERNAL_H

#include <cstdlib>
#include <hip/hip_runtime.h>
#include "../../include/mtfhip.h"
#include "mtfhip_fused_dispatch.h"
#include "mtfhip_owned.h"
#include "mtfhip_sm_system.h"

namespace mtfhip {

/* The policies of the owner types (mtfhip_owned.h).  These are the library's only calls that obtain or release device memory, pinned host
 * memory, events and streams: a handle's member is an owner built on them, or a documented view. */
struct DeviceMem {
	static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
	static void release(void *p) { (void)hipFree(p); }
};
template <unsigned Flags = hipHostMallocDefault> struct PinnedMem {
	static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
	static void release(void *p) { (void)hipHostFree(p); }
};
struct FineGrainedMem {   /* device memory other devices' kernels may store into while ours polls it (the particle filter's mailbox) */
	static hipError_t alloc(void **p, size_t bytes) { return hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained); }
	static void release(void *p) { (void)hipFree(p); }
};
struct EventApi {
	typedef hipEvent_t handle;
	static hipError_t create(hipEvent_t *e) { return hipEventCreate(e); }
	static hipError_t create(hipEvent_t *e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
	static void destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
};
struct StreamApi {
	typedef hipStream_t handle;
	static hipError_t create(hipStream_t *s, unsigned flags) { return hipStreamCreateWithFlags(s, flags); }
	static void destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
};
template <class T> using Dev = Owned<T, DeviceMem>;
template <class T, unsigned Flags = hipHostMallocDefault> using Pinned = Owned<T, PinnedMem<Flags>>;
typedef OwnedHandle<EventApi> Event;
typedef OwnedHandle<StreamApi> Stream;

struct ImgView {
	const float *data;
	int h, w, stride;     /* stride in floats between rows */
	int channels = 1;     /* 1: CV_32FC1 ; 3: CV_32FC3, interleaved (the mc:: sampling path) */
};

/* POD view of a batch, passed by value to kernels.  Every buf[i] is [B][per-target size]. */
struct BatchView {
	int B, N, S, ssm, am; /* N = patch_size = NP * C rows of every per-pixel AM array; S = columns of the J planes this view addresses */
	int NP, C;            /* sample points per target, channels (MCSSD / MCNCC / MCMI: 3) */
	int unit_z;           /* 1: every init_z == 1 (affine SSM or parallelogram corners) */
	/* The low-order models (Similitude, Isometry, Translation) run the affine pixel pass: in a fused view ssm is MTFHIP_SSM_AFFINE and S
	 * the pass's row width 6 -- J planes, accumulator layout, the constant Hessian's stride; the model and the size of its solve travel
	 * with the finish alone (TrackState::lo_ssm / SS), so this struct -- the first kernel argument of every pixel pass -- is what it was.
	 * In a per-function view of such a batch ssm is the model itself and S its state size.
	 * `states` of a low-order batch holds, on the device, the affine embedding of its warp [W02, W12, W00 - 1, W01, W10, W11 - 1]:
	 * what the affine pass reads its 2 x 2 block from, and what the affine state update of the finish writes. */
	double *buf[MTFHIP_BUF_COUNT];
	double *warps;        /* [B][9] row-major curr_warp */
	double *states;       /* [B][8] curr_state */
};

/* (the accumulator slots ACC_* / NCC_* of the reducing kernels and tri8: mtfhip_sm_system.h) */

/* Every kernel launch of the library goes through this macro: the launch status (invalid configuration, missing code object,
 * out-of-resources ...) is read back at once and kept as a sticky error that the next C-ABI call which synchronises reports,
 * instead of surfacing as a timeout of the host-flag wait or at some later, unrelated call. */
void note_launch_error(hipError_t e, const char *file, int line);
#define MTFHIP_LAUNCH(...) do { hipLaunchKernelGGL(__VA_ARGS__); const hipError_t _le = hipGetLastError(); \
	if (_le != hipSuccess) ::mtfhip::note_launch_error(_le, __FILE__, __LINE__); } while (0)
constexpr int kBlock = 256;       /* threads per workgroup: 4 wave64 */
constexpr int kGridTabMax = 2048; /* FusedArgs::grid_regen: columns + rows of the lattice tabulated in LDS (32 KB) */
/* FusedArgs::grid_regen only when a workgroup walks at least this many rows: the map load, the table and its barrier stand in front of the
 * first row's loads, which pays off in a streaming launch (64 x 200 x 200: 20 rows, 54.4 -> 49.4 us) and not in a latency-bound one
 * (one 200 x 200 target, 4 rows: 12.2 -> 12.8 us per iteration with it) */
constexpr int kGridRegenMinRows = 8;
/* (which instantiations carry the rebuild: grid_regen_kernel, mtfhip_fused_dispatch.h) */
#ifndef MTFHIP_SLOTS
#define MTFHIP_SLOTS 512          /* resident workgroups of the fused kernel: 256 CUs x 2 (2 waves/SIMD, 4-wave groups) */
#endif
#ifndef MTFHIP_MIN_ROWS
#define MTFHIP_MIN_ROWS 4         /* at least this many 256-pixel rows per workgroup (amortises the reduction) */
#endif
constexpr int kMaxS = 8;

/* Work decomposition of the fused kernel: every target is cut into nblk chunks of `rows` 256-pixel rows so that
 * B * nblk is as close as possible to the number of resident workgroups -- one full round of workgroups, no
 * half-empty tail round (a 2.5-round grid costs ~8 % against a 2- or 1-round grid) */
inline void fused_decomposition(int N, int B, int &nblk, int &rows, int slots = MTFHIP_SLOTS) {
	const int total_rows = (N + kBlock - 1) / kBlock;
	int nb_max = (total_rows + MTFHIP_MIN_ROWS - 1) / MTFHIP_MIN_ROWS;
	if (nb_max < 1) nb_max = 1;
	if (B < 1) B = 1;
	/* cost model: rounds of resident workgroups x (rows per workgroup + the reduction epilogue, ~1.5 rows) */
	double best = 1e300;
	int best_nb = 1;
	for (int nb = 1; nb <= nb_max; ++nb) {
		const int r = (total_rows + nb - 1) / nb;
		const int real_nb = (total_rows + r - 1) / r;
		const long blocks = (long)B * real_nb;
		const long rounds = (blocks + slots - 1) / slots;
		const double cost = (double)rounds * (r + 1.5);
		if (cost < best - 1e-9) { best = cost; best_nb = real_nb; }
	}
	rows = (total_rows + best_nb - 1) / best_nb;
	nblk = (total_rows + rows - 1) / rows;
}
inline int fused_blocks_per_target(int N, int B) { int nb, r; fused_decomposition(N, B, nb, r); return nb; }
inline int simple_blocks_per_target(int N) {
	int nb = (N + kBlock * 4 - 1) / (kBlock * 4);
	return nb < 1 ? 1 : nb;
}

/* device-side solve + compositional update + convergence test for mtfhip_batch_track */
struct TrackState {
	double *acc;        /* [B][ACC_COUNT] reduced accumulators of this iteration */
	double *h0;         /* [B][64] constant (init) self Hessian, column-major, already negated sums */
	double *corners;    /* [B][8] current corners */
	double *init_corners_hm; /* [B][12] */
	int *active;        /* [B] 1 while the target still iterates */
	int *n_iters;       /* [B] */
	const double *ncc;    /* [B][8] NCC scalars (mean(I0), |I0 - mean|, ...), NULL for SSD */
	const double *ncc_tm; /* [B][52] NCC template moments: sum J0 | sum I0 J0 | Gram(J0) */
	int h_from_acc;       /* 1: every non-constant Hessian type reads the reduced row, ICLK's included (MI: k_finish_track_mi) */
	/* Levenberg-Marquardt (NT/ESM.cc:186-232, NT/FCLK.cc:205-250, NT/ICLK.cc:181-199) inside the device-side loop, per target:
	 * [0] prev_similarity [1] leven_marq_delta [2] state_reset [3] iter_id [4..11] the last state_update.  NULL: no LM. */
	double *lm;
	const double *f_ext;  /* [B] similarity of this pass when it is not a function of the reduced row (MI: d_mi_f), else NULL */
	/* debug trace of the device-side loop (mtfhip_batch_track_trace): record `pass` of target t at trace + (t cap + pass) kTraceStride:
	 * [0..63] H as the search method holds it before damping, row-major 8 x 8 | [64..71] g | [72..79] the state update applied |
	 * [80..87] corners after it | [88] f [89] pass [90] Levenberg-Marquardt undo [91] damping [92] 1 if H was recorded.  NULL: off. */
	double *trace;
	int trace_cap;
	/* second-order term of the Hessian (sec_ord_hess; k_second_order_ssd's output [B][S * S], entry (r, c) at c S + r), added to the
	 * first-order one times h_extra_scale (ESM SumOfStd halves the whole sum, NT/ESM.cc:339); the system is then solved with pivoting.
	 * NULL: none. */
	const double *h_extra;
	double h_extra_scale;
	int fast_finish;      /* tolerance mode, SSD family, first-order Hessian from the reduced row or the constant one: finish_track_fast_body */
	/* k_iclk_track / k_grid_fb, plain mode, right behind a fused re-initialisation (k_template_init in region mode, mtfhip_grid_reset): every patch
	 * starts from the identity warp and the zero state at its template's corners, which that kernel left in init_corners_hm -- the slab's warps /
	 * states / corners are not read, so the host does not upload them (one ingest launch and its gap less per frame, r06) */
	int fresh_reset;
	/* deferred materialisation (track_loop_chunked, api_track.hip): a pass launched with the non-materialising pixel kernel sets lean_pass; a target the finish
	 * stops after such a pass (change < epsilon) leaves the warp and the state that pass ran at in warp_last ([B][9]) / state_last
	 * ([B][8]) and raises need_mat[t]; one trailing launch of the materialising kernel at that warp then writes It / dIt_dx / Jt for
	 * it.  NULL / 0: off. */
	double *warp_last = nullptr;
	double *state_last = nullptr;
	int *need_mat = nullptr;
	int lean_pass = 0;
	/* the two-launch loop's finish (k_finish_track; the other routes leave both at 0).  last_pass: the host enqueues no pass behind this one, so a
	 * target that is still active after it is delivered to the host now (HostPublish of k_finish_track).  finish_prio: the finish waves raise
	 * their issue priority -- one wave per target beside the other queue's pixel pass, where it is always the younger wave of its SIMD */
	int last_pass = 0;
	int finish_prio = 0;
	/* a low-order SSM's materialising loop: the warp and the state a target's last pass ran at are kept in warp_last / state_last whatever the
	 * pass kind (need_mat is left alone), for the launch that writes the target's N x S Jacobian behind the loop (api_track.hip) */
	int keep_last = 0;
	/* the finish of a low-order SSM's batch (k_finish_track_lo): the model (MTFHIP_SSM_SIMILITUDE / _ISOMETRY / _TRANSLATION) and the size
	 * of its solve, 4 / 3 / 2 -- bv.S is then the affine pass's row width 6.  0: a homography / affine batch. */
	int lo_ssm = 0, SS = 0;
};
constexpr int kLmStride = 12;
constexpr int kTraceStride = 96;

/* k_track_persist: per-target arrival counter and generation number of the in-kernel barrier between the pixel pass and the solve */
struct PersistState {
	int *arrive;            /* [B] zero between launches */
	unsigned *gen;          /* [B] monotonic: gen_base + pass + 1 once pass `pass` has been solved */
	unsigned gen_base;
	unsigned long long timeout_ticks;   /* of the 100 MHz wall clock */
};

/* results of the one-launch loop delivered straight into the host-coherent mirror of the state slab (warps | states | corners |
 * ... | iteration counts) by the workgroup that produced them; the last workgroup to finish raises the flag the host spins on.
 * host == NULL: nothing is published (k_publish_host does it in a launch of its own). */
/* The square-to-quadrilateral map behind set_corners (see rect_to_quad, mtfhip_api_internal.h), as ONE set of expressions for the host
 * and for the kernel that lays out a patch's grid itself (k_iclk_track in region mode): both are compiled without contraction, so the
 * nine entries are the same bits on either side.  H: row-major 3 x 3, H[8] = 1; false: degenerate corners. */
__host__ __device__ inline bool rect_to_quad_hd(double lo_x, double lo_y, double hi_x, double hi_y, const double *q, double *H) {
	const double x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], x2 = q[4], y2 = q[5], x3 = q[6], y3 = q[7];
	const double dx1 = x1 - x2, dx2 = x3 - x2, sx = x0 - x1 + x2 - x3;
	const double dy1 = y1 - y2, dy2 = y3 - y2, sy = y0 - y1 + y2 - y3;
	double a, b, c, d, e, f, g, h;
	if (sx == 0 && sy == 0) {   /* parallelogram: affine */
		a = x1 - x0; b = x3 - x0; c = x0; d = y1 - y0; e = y3 - y0; f = y0; g = 0; h = 0;
		if (a * e - b * d == 0) return false;
	} else {
		const double den = dx1 * dy2 - dy1 * dx2;
		if (den == 0) return false;
		g = (sx * dy2 - dx2 * sy) / den; h = (dx1 * sy - sx * dy1) / den;
		a = x1 - x0 + g * x1; b = x3 - x0 + h * x3; c = x0;
		d = y1 - y0 + g * y1; e = y3 - y0 + h * y3; f = y0;
	}
	/* (u, v) = ((x - lo_x) / wx, (y - lo_y) / wy) */
	const double wx = hi_x - lo_x, wy = hi_y - lo_y;
	const double rows[3][3] = {{a, b, c}, {d, e, f}, {g, h, 1.0}};
	double m[9];
	for (int r = 0; r < 3; ++r) {
		m[3 * r] = rows[r][0] / wx; m[3 * r + 1] = rows[r][1] / wy;
		m[3 * r + 2] = rows[r][2] - rows[r][0] * lo_x / wx - rows[r][1] * lo_y / wy;
	}
	if (m[8] == 0 || !(m[8] - m[8] == 0)) return false;   /* zero, infinite or NaN */
	if (m[8] == 1.0) for (int i = 0; i < 9; ++i) H[i] = m[i];   /* (x / 1.0 == x: a parallelogram's nine divisions are skipped) */
	else for (int i = 0; i < 9; ++i) H[i] = m[i] / m[8];
	H[8] = 1;
	return true;
}

/* rect_to_quad_hd's first refusals alone (collinear / coincident corners), ~12 flops: what a deferred reset checks on the host BEFORE it
 * commits anything, so that degenerate corners are an error without a state change, as on the non-deferred path (the kernel's own
 * report through n_iters = -1 stays as the backstop for the map's remaining refusal, a vanishing m[8]) */
__host__ __device__ inline bool quad_degenerate_hd(const double *q) {
	const double x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], x2 = q[4], y2 = q[5], x3 = q[6], y3 = q[7];
	const double dx1 = x1 - x2, dx2 = x3 - x2, sx = x0 - x1 + x2 - x3;
	const double dy1 = y1 - y2, dy2 = y3 - y2, sy = y0 - y1 + y2 - y3;
	if (sx == 0 && sy == 0) return (x1 - x0) * (y3 - y0) - (x3 - x0) * (y1 - y0) == 0;
	return dx1 * dy2 - dy1 * dx2 == 0;
}

/* GridTracker::resetTrackers' geometry for ONE patch (SM/src/GridTracker.cc:345-380; mtfhip_grid_layout, api_core.hip, describes it): the
 * grid SSM's points are the resx x resy grid of the unit square through the region's 4-corner map Wr = rect_to_quad(-0.5 .. 0.5, region),
 * a patch is the cell spanned by four of them (dyn_patch_size), a fixed-size rectangle centred on its own point, or one centred on the
 * cell's centroid (patch_centroid_inside).  One set of expressions for the host layout and for the kernel that lays its own patch out
 * (k_iclk_track, RegionIngest::layout; both compiled without contraction: the same bits). */
struct GridLayoutHD { int grid_size_x, grid_size_y, patch_size_x, patch_size_y, dyn_patch_size, patch_centroid_inside; };
__host__ __device__ inline double lin_spaced_hd(int i, int n, double lo, double hi) { return (n == 1 || i == n - 1) ? hi : lo + i * ((hi - lo) / (n - 1)); }
__host__ __device__ inline void grid_pt_hd(const double *Wr, int resx, int resy, int idx, double *x, double *y) {
	const int r = idx / resx, c = idx % resx;
	const double ny = lin_spaced_hd(r, resy, -0.5, 0.5), nx = lin_spaced_hd(c, resx, -0.5, 0.5);
	const double X = Wr[0] * nx + Wr[1] * ny + Wr[2], Y = Wr[3] * nx + Wr[4] * ny + Wr[5], Z = Wr[6] * nx + Wr[7] * ny + Wr[8];
	*x = X / Z; *y = Y / Z;
}
__host__ __device__ inline void grid_patch_corners_hd(const GridLayoutHD &g, const double *Wr, int k, double *pc) {
	const int extra = (g.dyn_patch_size || g.patch_centroid_inside) ? 1 : 0;
	const int resx = g.grid_size_x + extra, resy = g.grid_size_y + extra;
	const bool surround = extra != 0;
	const int sub_x = g.grid_size_x + 1;   /* _linear_idx(idy, idx) = idy * (grid_size_x + 1) + idx, :139-146 */
	const int row = k / g.grid_size_x, col = k % g.grid_size_x;   /* :354-355 */
	for (int q = 0; q < 8; ++q) pc[q] = 0.0;
	if (surround) {   /* :357-367 TL, TR, BR, BL of the cell */
		const int id[4] = {row * sub_x + col, row * sub_x + col + 1, (row + 1) * sub_x + col + 1, (row + 1) * sub_x + col};
		for (int q = 0; q < 4; ++q) grid_pt_hd(Wr, resx, resy, id[q], pc + 2 * q, pc + 2 * q + 1);
	}
	if (!g.dyn_patch_size) {   /* :369-380 */
		double cx, cy;
		if (g.patch_centroid_inside) {   /* utils::getCentroid miscUtils.h:481-487 */
			cx = (pc[0] + pc[2] + pc[4] + pc[6]) / 4.0;
			cy = (pc[1] + pc[3] + pc[5] + pc[7]) / 4.0;
		} else grid_pt_hd(Wr, resx, resy, k, &cx, &cy);   /* ssm.getPts().col(tracker_id) */
		const double half_x = g.patch_size_x / 2.0, half_y = g.patch_size_y / 2.0;   /* centrod_dist_x / _y :156-157 */
		const double min_x = cx - half_x, min_y = cy - half_y;   /* utils::Corners(cv::Rect_<double>) miscUtils.h:42-52 */
		const double max_x = min_x + g.patch_size_x, max_y = min_y + g.patch_size_y;
		pc[0] = pc[6] = min_x; pc[2] = pc[4] = max_x;
		pc[1] = pc[3] = min_y; pc[5] = pc[7] = max_y;
	}
}

/* k_iclk_track in REGION mode (mtfhip_batch_track_region / mtfhip_grid_update, r04): the workgroup of a patch takes the patch's region
 * corners (and its template's NCC scalars) straight from the pinned staging buffer, derives the square-to-quadrilateral map, lays out
 * its own sample grid -- kept in registers for the loop, written to INIT_PTS / INIT_HXY / INIT_Z for whoever asks later -- and starts
 * from the identity warp: what set_corners' ingest + k_init_grid did in a launch of their own in front of the loop (7.8 us of a 64 us
 * frame, plus the gap).  corners == NULL: off (the slab and the grid are already on the device). */
struct RegionIngest {
	const double *corners;      /* device-visible pinned host memory: [B][8], (x, y) per corner, TL TR BR BL */
	const double *ncc;          /* likewise: [B][8] NCC scalars of the templates (slab layout) */
	double *d_ncc, *d_w0, *d_init_corners_hm;   /* the slab's device copies of what the workgroup derives */
	double lo_x, lo_y, hi_x, hi_y;
	int resx, resy, force_unit_z;
	/* layout != 0 (mtfhip_grid_frame with fixed-size patches, r05): the workgroup computes its patch's corners itself from the GRID's
	 * region (grid_patch_corners_hd over region_map = rect_to_quad(-0.5 .. 0.5, region), formed on the host once) -- `corners` is not
	 * read: no PCIe round trip in front of the grid layout, and the host lays the patches out for its mirrors AFTER the launch */
	int layout;
	GridLayoutHD grid;
	double region_map[9];
};

struct HostPublish {
	char *host;
	size_t dbl_bytes;   /* offset of the int part of the slab */
	int B;
	int *count;
	unsigned long long *flag, seq;
	int fenced;         /* publish_fenced(): the release / acquire form of the hand-over instead of acknowledged write-through stores */
};
/* How a kernel hands results to the host (k_finish_host, k_publish_host, publish_target, the particle filter's estimate).  Default:
 * relaxed system-scope (write-through) stores, s_waitcnt vmcnt(0), a relaxed agent-scope arrival counter, a relaxed system-scope flag
 * store by the last arriver -- what a release does in hardware minus the L2 write-backs (2.5 us each), but a data race under the
 * HIP / HSA memory model: it relies on the stores being write-through atomics, on per-wave vmcnt and on ordered posted writes
 * (r04 advisor).  MTFHIP_PUBLISH_FENCE=1 restores the model-conforming form at run time for every publisher: agent-scope release
 * before the counter, acq_rel on the counter, __threadfence_system() + a system-scope release store of the flag. */
inline int publish_fenced() {
	static const int v = [] { const char *e = std::getenv("MTFHIP_PUBLISH_FENCE"); return (e && e[0] == '1') ? 1 : 0; }();
	return v;
}

struct FusedArgs {
	int mode;          /* accumulation mode: 0 FCLK-type, 1 ESM-type, 2 ICLK-lite (see k_fused_ssd) */
	int chained;
	int materialize;
	int hess_mean;     /* ESM hess_type Original: outer products of (J0+Jt)/2 instead of Jt */
	int j0_init_variant; /* with j0_recompute: J0 is the Init variant (non-chained initialize, or refreshed by set_region), else Warped at identity */
	int j0_recompute;  /* 1: the template's SD rows are rebuilt from dI0_dx (bit-identical to the stored J0, 16 instead of 8 S bytes per pixel) */
	int rows_per_block; /* 256-pixel rows walked by one workgroup (fused_decomposition) */
	double grad_eps;
	double norm_mult, norm_add;
	const int *active; /* optional [B] mask: targets with 0 are skipped (device-side loop) */
	/* single-target batches: the warp and state travel in the kernel arguments (read from the kernarg segment instead of
	 * bv.warps / bv.states; the kernel stores them there afterwards) -- no separate upload in front of every launch */
	int inline_warp;
	double iw[9], is[8];
	/* 1: tolerance-mode arithmetic (mtfhip_device.h, "tolerance-mode arithmetic"); only with materialize == 0 -- the
	 * materialised arrays stay bit-identical to what the per-function kernels write */
	int fast_math;
	/* 1: the template grid point of a row is rebuilt from the target's map (w0 [B][9], the slab) and the lattice index instead of
	 * being read from INIT_PTS -- planned by fused_args only for a unit-z grid that k_init_grid laid out from these very maps with
	 * W0[6] = W0[7] = 0 (no division), single channel, no caller write to the grid since (grid_point_xy, mtfhip_grid_device.h) */
	int grid_regen;
	/* (planned for the materialising SSD launch only, lattices of at most kGridTabMax columns + rows: mtfhip_batch_grid_regen) */
	int g_resx, g_resy;
	double g_lo_x, g_lo_y, g_hi_x, g_hi_y;
	double g_step_x, g_step_y;   /* (hi - lo) / (res - 1), the layout's own step */
	const double *w0;
};

/* RSCV (am = MTFHIP_AM_RSCV): the intensity maps the fused pass applies to every sample (kernels_imap.hip builds them), an extra
 * argument behind the fused kernels' own -- map: [bv.B][nb], offset to bv's first target; linear: RSCVParams::weighted_mapping */
struct RscvMap {
	const double *map = nullptr;
	int nb = 0, linear = 0;
};
/* LRSCV (am = MTFHIP_AM_LRSCV): what the fused pass needs to blend every sample (kernels_imap.hip builds the maps) -- map: [bv.B][R][nb]
 * (affine_mapping: [bv.B][R][2], a_r and c_r), offset to bv's first target; wts: [R][N] sub_region_wts, one per batch, sub-region
 * idy nx + idx; R = nx ny; linear: weighted_mapping */
struct LrscvMap {
	const double *map = nullptr;
	const double *wts = nullptr;
	int nb = 0, R = 0, affine = 0, linear = 0;
};
/* what the pass in front of a fused launch hands it (imap_before_pass): the maps of the batch's model, or none */
struct FusedMaps {
	RscvMap rm;
	LrscvMap lm;
};

/* SPSS (am = MTFHIP_AM_SPSS): what the fused pass needs beside FusedArgs, an extra argument behind the fused kernels' own -- c = (255 k)^2
 * (SPSS.cc:37-38); weight: the per-pixel weight of the Gram matrix in ACC_H (SPSS_W_*: cmptSelfHessian SPSS.cc:221-225, cmptCurrHessian
 * :191-196, cmptInitHessian :160-165), taken over Jt (FCLK, ESM), Jm (ESM with FusedArgs::hess_mean) or J0 (ICLK); g_mean: ACC_G is
 * sum df_dIt Jm (ESM jac_type Original, NT/ESM.cc:246-249) instead of sum df_dIt Jt */
enum { SPSS_W_SELF = 0, SPSS_W_CURR = 1, SPSS_W_INIT = 2, SPSS_W_SELF0 = 3 };   /* SELF0 (per-function kernel only): the self weight at It = I0 */
struct SpssArgs {
	double c = 6.5025;
	int weight = SPSS_W_SELF, g_mean = 0;
};

/* one-time probe: does the kernel-argument segment hold (BatchView, ImgView, FusedArgs) where fused_lk_body's inline-warp path reads them? */
bool kernarg_layout_verified(hipStream_t st);
void launch_queue_delay(double microseconds, hipStream_t st);
/* ---- launchers (all asynchronous on `st`) ---- */
void launch_apply_warp(const BatchView &bv, hipStream_t st);
void launch_grad_pts(const BatchView &bv, double eps, hipStream_t st);
void launch_sample(const BatchView &bv, const ImgView &im, const double *pts, double *out,
	double mult, double add, hipStream_t st);
void launch_update_model(const BatchView &bv, const ImgView &im, const double *pts, double *I0, double mult, double add,
	double frame_count, double alpha, int running_avg, hipStream_t st);
void launch_img_grad(const BatchView &bv, const ImgView &im, const double *pts, double *grad,
	double eps, double mult, hipStream_t st);
void launch_warped_img_grad(const BatchView &bv, const ImgView &im, const double *grad_pts, double *grad,
	double eps, double mult, hipStream_t st);
void launch_pix_jacobian(const BatchView &bv, int variant, const double *grad, double *J, hipStream_t st);
void launch_mean_jacobian(const BatchView &bv, hipStream_t st);
/* MI device-side loop: g and H of the fused MI passes handed to the finish in one launch (k_finish_track_mi) */
void launch_finish_track_mi(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts, int sum_std, int gmode,
	const double *mi_H, const double *gpart, int ng, double *rows, hipStream_t st);
/* df_dI0 = It - I0 ; partial sums of r^2 into `partials` ([B][nblk][ACC_COUNT]) */
void launch_ssd_residual(const BatchView &bv, double *partials, int nblk, hipStream_t st);
void launch_negate(const double *src, double *dst, size_t n, hipStream_t st);
/* g-type partials: sum_i (v1[i]*J1[i,:] (+ v2[i]*J2[i,:] into ACC_G2, or + v1[i]*J2[i,:] into ACC_G when sum_mode)) */
void launch_gemv(const BatchView &bv, const double *v1, const double *J1, const double *v2, const double *J2,
	int sum_mode, double *partials, int nblk, hipStream_t st);
/* H-type partials: sum_i J[i,a] J[i,b] */
void launch_gram(const BatchView &bv, const double *J, double *partials, int nblk, hipStream_t st);
/* NCC pieces (see the kernel comments); `sc` is the [B][8] per-target scalar block */
void launch_vec_sum(const BatchView &bv, const double *v, double *partials, int nblk, hipStream_t st);
void launch_ncc_centered(const BatchView &bv, const double *sc, double *partials, int nblk, hipStream_t st);
void launch_ncc_grad(const BatchView &bv, const double *sc, int curr, double *out, double *partials, int nblk, hipStream_t st);
void launch_sub_mean(const BatchView &bv, double *v, const double *sc, hipStream_t st);
void launch_col_sum(const BatchView &bv, const double *J, double *partials, int nblk, hipStream_t st);
void launch_ncc_hess(const BatchView &bv, const double *sc, const double *colmean, const double *J, double *partials,
	int nblk, hipStream_t st);
/* MI pieces; table block offsets (doubles) of the per-target MI state, see kernels_mi.hip */
enum {
	MI_NB = 16,
	MI_HIST_INIT = 0, MI_HIST_CURR = 16, MI_LOG_INIT = 32, MI_LOG_CURR = 48,
	MI_JOINT = 64, MI_JOINT_LOG = 320, MI_T_CURR = 576, MI_T_INIT = 832,
	MI_SELF_JOINT = 1088, MI_T_SELF = 1344, MI_SIZE = 1600
};
void launch_mi_hist(const BatchView &bv, int nb, double norm_mult, const double *A, const double *Bv, double *partials,
	int nblk, int row_len, hipStream_t st);
void launch_mi_hist_finish(const BatchView &bv, int nb, double pre_seed, double norm_mult, int mode, int first_init,
	const double *partials, int nblk, int row_len, double *tb, double *f_out, hipStream_t st);
void launch_mi_factor(const BatchView &bv, int nb, int curr, double *tb, hipStream_t st);
void launch_mi_grad(const BatchView &bv, int nb, double norm_mult, const double *A, const double *Bv, const double *tb,
	int table_off, double *out, hipStream_t st);
void launch_mi_hess(const BatchView &bv, int nb, double norm_mult, const double *A, const double *Bv, const double *tb,
	int table_off, int transpose_q, const double *J, double *partials, int nblk, int row_len, hipStream_t st);
void launch_mi_hess_finish(const BatchView &bv, int nb, const double *partials, int nblk, int row_len, const double *tb,
	int joint_off, int hist_off, int transpose_q, double *out, hipStream_t st);
void launch_mi_tables_iter(const BatchView &bv, int nb, double pre_seed, double norm_mult, int with_self, const double *partials, int nblk,
	int row_len, double *tb, double *f_out, hipStream_t st);
void launch_mi_hist_self(const BatchView &bv, int nb, double norm_mult, const double *A, const double *Bv, double *partials,
	int nblk, int row_len, hipStream_t st);
/* dI0 != NULL: k_mi_grad_gemv rebuilds the template's steepest-descent row from dI0_dx [B][2][N], the grid points [B][N] x,y
 * (and z [B][N] of the homogeneous grid, NULL = 1) instead of reading J0 -- valid under the conditions of FusedArgs::j0_recompute */
struct MiJ0Rebuild { const double *dI0, *pts, *z; int hom, init_variant; };
void launch_mi_grad_gemv(const BatchView &bv, int nb, double norm_mult, const double *It, const double *I0, const double *tb,
	const double *Jt, const double *J0, const MiJ0Rebuild &rb, double *df_dIt, double *df_dI0, double *partials, int nblk, hipStream_t st);
/* CCRE pieces (kernels_ccre.hip; the table block and its modes: mtfhip_ccre_tables.h).  launch_ccre_hist is k_mi_hist with the cumulative fill
 * (kernels_mi.hip): rows [nb cumulative hist of A | nb*nb cumulative joint (A, B)].  launch_ccre_tables sums rows of
 * [nb + nb*nb (A, I0) | nb + nb*nb (It, It) | nb plain hist ..]; launch_ccre_hess: kind 0 init (J = J0), 1 curr, 2 self, rows
 * [36 | nb*nb*S | nb*S (init)], which launch_ccre_hess_finish reads summed to one row per target */
void launch_ccre_hist(const BatchView &bv, int nb, double norm_mult, const double *A, const double *Bv, double *partials,
	int nblk, int row_len, hipStream_t st);
void launch_ccre_tables(const BatchView &bv, int nb, double pre_seed, double norm_mult, int mode, int with_self, const double *partials, int nblk,
	int row_len, double *tb, double *f_out, hipStream_t st);
void launch_ccre_grad_gemv(const BatchView &bv, int nb, double norm_mult, const double *It, const double *I0, const double *tb,
	const double *Jt, const double *J0, const MiJ0Rebuild &rb, double *df_dIt, double *df_dI0, double *partials, int nblk, hipStream_t st);
void launch_ccre_hess(const BatchView &bv, int nb, double norm_mult, int kind, const double *It, const double *I0, const double *tb, const double *J,
	double *partials, int nblk, int row_len, hipStream_t st);
void launch_ccre_hess_finish(const BatchView &bv, int nb, int kind, const double *rows, int row_len, const double *tb, double *out, hipStream_t st);
/* ---- the recompute form of the MI iteration (kernels_mi_fused.hip; tolerance-mode arithmetic, 8 bins) ---- */
struct MiFastPlan {
	int nb = 8;           /* the AM's n_bins: 8 -> the NB = 8 kernels, otherwise (<= 10; hk 0 / 1) the NB = 10 ones */
	int hk;               /* Hessian pass: 0 none (constant Hessian), 1 self(Jt), 2 curr, 3 init(J0) */
	int hrow;             /* pixel Jacobian of the Hessian pass: 0 Jt, 1 J0, 2 (J0 + Jt) / 2 */
	int j0_mode;          /* 0 the template's row is not needed, 1 rebuilt from dI0_dx, 2 read from J0 */
	int j0_init_variant;
	int need_dft, need_df0, g_mean;
	int nonchained = 0;   /* the search method's chained_warp = 0: pass 2 takes the rounded steps of updateGradPts' four points (mi_finish) */
	int hist_from_joint = 0;   /* pass 1: the histogram of It as the row sums of the joint histogram (partition of unity: every window of I0 lies
	                              inside the bins and sums to one) instead of a block product of its own -- a third of the pass's matrix work */
	double grad_eps, norm_mult, norm_add, hist_norm;
	const int *active;    /* device flags, NULL = all */
	const double *tb;     /* [B][MI_SIZE] */
	const double *poly = nullptr;   /* [B][mi_poly_size()]: the tables as per-class polynomials (launch_mi_poly_tables), read by pass 2 */
};
void launch_mi_poly_tables(const BatchView &bv, const double *tb, double hist_norm, int with_self, double *poly, hipStream_t st);
/* launch_mi_tables_iter + launch_mi_poly_tables in one launch (hist_norm is the tables' norm_mult) */
void launch_mi_tables_poly(const BatchView &bv, int nb, double pre_seed, double norm_mult, int with_self, const double *partials, int nblk, int row_len,
	double *tb, double *f_out, double *poly, hipStream_t st);
int mi_poly_size(int nb = 8);
void launch_mi_pass_hist(const BatchView &bv, const ImgView &im, const MiFastPlan &pl, double *partials, int nblk, int row_len, hipStream_t st);
void launch_mi_pass_grad_hess(const BatchView &bv, const ImgView &im, const MiFastPlan &pl, double *partials, int nblk, hipStream_t st);
void launch_mi_finish_fast(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts, const MiFastPlan &pl, int gmode, int do_track,
	const double *partials, int nblk, double *out_H, double *out_g, double *rows, hipStream_t st);
void launch_mi_score_candidates(const BatchView &bv, const ImgView &im, const MiFastPlan &pl, const double *dev_states, int lo, int cnt,
	double *partials, int nblk, int row_len, double pre_seed, double alpha, int likelihood_func, double measurement_sigma, double max_similarity,
	double *wts, double *sim, hipStream_t st);
int mi_fast_row_len(int nb = 8);
/* ---- particle filter (kernels_pf.hip): proposal + scoring, cumulative weights, resampling + estimate ---- */
enum { PF_SAMPLER_STATE = 0,       /* one normal per state component (ProjectiveBase::generatePerturbation) */
	PF_SAMPLER_HOM_CORNERS = 1,    /* Homography, corner based: 10 normals (Homography.cc:899-911) */
	PF_SAMPLER_AFF_PTS1 = 2,       /* Affine, pt_based_sampling 1: 6 normals (Affine.cc:475-482) */
	PF_SAMPLER_AFF_PTS2 = 3,       /* Affine, pt_based_sampling 2: 8 normals (Affine.cc:483-491) */
	PF_SAMPLER_AFF_GEOM = 4 };     /* Affine, geometric: 6 normals through geomToState (Affine.cc:495-502) */
struct PfLaunch {
	int n, S;
	int dynamic_model, update_type, sampler, nz, likelihood_func, resampling_type, mean_type;
	double ar_coeff, measurement_sigma, max_similarity;
	double sigma[8], mean[8], init_corners[8], init_corners_hm[12], aux_inv[9], canon[6];
	unsigned long long seed;
	unsigned iter;
	const double *normals, *uniforms;   /* device arrays or NULL (Philox) */
	/* several sampler distributions (PF.cc:240-269, 345-369) and adaptive resampling (PF.cc:381-390); n_distr == 1 and
	 * min_eff_particles == 0: neither */
	int n_distr;
	const double *distr_uniforms;       /* [n] device array or NULL (Philox): the distribution draw of every particle */
	double min_distr_wt, min_eff_particles;
};
struct PfBuffers {
	double *st, *ar;            /* [n][S] the current (resampled) particle set */
	double *prop, *prop_ar;     /* [n][S] this iteration's proposals */
	double *next, *next_ar;     /* [n][S] where the selection pass leaves the proposals of the next iteration (look-ahead) */
	double *wts, *sim;          /* [>= n] weights at global particle indices; similarities or NULL */
	double *cum, *sub16, *chunk_tot, *chunk_incl;
	double *parts, *gparts, *out;   /* per-workgroup rows of the selection pass, their per-group folds, the estimate */
	int *res_order;             /* residual resampling: particle indices by weight, highest first (the last index stays last) */
	/* distributions / adaptive resampling (all NULL when neither is in use): [n_distr][8] sigmas and means, the cumulative distribution
	 * weights the ids are drawn from (rewritten by the scan for the next iteration), the weights themselves, the particles'
	 * distribution ids, per-chunk statistics of the scan [nch][17], the flag "this iteration resamples" */
	double *distr_sigma, *distr_mean, *distr_cum, *distr_wts, *scan_stats;
	int *distr_ids, *resample_flag;
	int *ids, *counters;        /* [0] the scan's arrival counter, [1] the selection pass's top-level counter, [2 ...] one per group of 64
	                               workgroups of the selection pass; zero between launches */
};
/* Peer-store exchange of the sharded filter's weights (the alternative to the all-gather, api_pf.hip: mtfhip_pf_set_exchange): every
 * rank owns a MAILBOX -- two weight vectors (the exchanges alternate between them, so a rank that runs one iteration ahead never
 * overwrites what a slower one still reads) and one arrival counter per source rank.  The scoring kernel stores every weight it
 * produces into every rank's mailbox (peer memory, mapped once at set-up); the last of its workgroups to finish adds 1 to its
 * rank's counter in every mailbox (release, system scope); the first kernel that reads the weights spins until every counter
 * has reached the count the host knows it must reach (acquire, system scope).  No host-enqueued collective, no extra launch. */
constexpr int kPfMaxPeers = 8;
struct PfPeerPush {
	int world, rank;                              /* world == 0: no peer stores */
	double *wts[kPfMaxPeers];                     /* every rank's weight vector of this exchange (own rank: unused, the scorer's wts) */
	unsigned long long *counters[kPfMaxPeers];    /* every rank's arrival counters [world]: this rank bumps entry `rank` */
	unsigned *arrive;                             /* this rank's own: the workgroups of the storing launch count themselves in; zero between launches */
};
struct PfPeerWait {
	int world, rank;                              /* world == 0: nothing to wait for */
	const unsigned long long *counters;           /* this rank's mailbox counters [world] */
	unsigned long long expected[kPfMaxPeers];     /* what each must have reached before the weights are complete */
	int *err;                                     /* host-mapped: set to 1 when the bounded spin gave up */
};
void launch_pf_propose(int ssm, const PfLaunch &p, const PfBuffers &bf, const double *st_in, const double *ar_in, double *st_out, double *ar_out, hipStream_t st);
void launch_score_block(const BatchView &bv, const ImgView &im, const double *states, int lo, int cnt, double alpha, double norm_mult,
	double norm_add, const double *ncc_sc, double *wts, double *sim, int likelihood_func, double measurement_sigma, double max_similarity,
	int fast_math, const PfPeerPush *peer /* or NULL */, const double *hull /* [8] host, or NULL: PfScoreArgs::hull */, const float *pair /* the row-pair copy of the frame, or NULL */, hipStream_t st);
/* weights [lo, lo + cnt) of `wts` -> every other rank's mailbox + the arrival: for scorers that do not store to the peers themselves */
void launch_pf_peer_push(const PfPeerPush &peer, const double *wts, int lo, int cnt, hipStream_t st);
void launch_pf_peer_wait(const PfPeerWait &w, hipStream_t st);   /* the wait in a launch of its own (no scan in this iteration) */
/* weights -> chunk-local cumulative weights + chunk table; wait != NULL: every workgroup first waits for the peers' weights */
void launch_pf_scan(const PfLaunch &p, const PfBuffers &bf, const PfPeerWait *wait, hipStream_t st);
/* local: no scan in front, the launch builds the cumulative weights in LDS itself (n <= pf_local_max(), multinomial resampling, no scan
 * statistics; wait: the peers' weights, as the scan's); pert_in: the perturbations of iteration p.iter + 1 drawn ahead (NULL: the
 * selection pass draws them itself); pert_out: where extra workgroups leave those of p.iter + 2 (NULL: none) -- [n][8] each */
struct PfSelectPlan { int local = 0; const PfPeerWait *wait = nullptr; const double *pert_in = nullptr; double *pert_out = nullptr; int estimate = 1; };
int pf_local_max();
void launch_pf_select(int ssm, const PfLaunch &p, const PfBuffers &bf, int lookahead, double *host_out /* or NULL */,
	unsigned long long *host_flag, unsigned long long seq, const PfSelectPlan &plan, hipStream_t st);
void launch_pf_fill(int n, int S, const double *dev_state, double *states, double *ars, hipStream_t st);
/* flag: NULL, or the scan's "this iteration resamples" (adaptive resampling): with 0 the residual kernels leave everything as it is */
void launch_pf_residual_prep(int n, const double *total, double *wts, double *keys, int *idx, const int *flag, hipStream_t st);
void launch_pf_residual_copies(int n, const double *wts, const int *order, int *copies, hipStream_t st);
void launch_pf_residual_map(int n, const int *order, const int *copies, const int *starts, int *ids, hipStream_t st);
int pf_parts_per_block();
int pf_chunk();
/* sums partials over blocks: out[B][ACC_COUNT] */
void launch_finish(double *partials, int nblk, double *out, int B, hipStream_t st);
void launch_finish_rows(double *partials, int nblk, int row_len, double *out, int B, hipStream_t st);
void launch_finish_host(double *partials, int nblk, int row_len, double *out_host, int *count, unsigned long long *flag_host,
	unsigned long long seq, int B, hipStream_t st);
void launch_publish_host(const void *src, void *dst_host, size_t bytes, int *count, unsigned long long *flag_host,
	unsigned long long seq, hipStream_t st);
/* the fused LK iteration for SSD (and RSCV: bv.am == MTFHIP_AM_RSCV takes the RSCV instantiations, which need rm; LRSCV: with lm and its
 * maps the LRSCV instantiations, without them -- a later pass of a frame under once_per_frame -- the SSD ones on the raw patch) */
void launch_fused_ssd(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials,
	int nblk, hipStream_t st, const FusedMaps *maps = nullptr, const SpssArgs *sp = nullptr);
/* kernels_fused_spss.hip: the SPSS instantiations of the fused body (replay and tolerance mode); and the finish that reads their rows,
 * k_finish_track_spss (launch_finish_track takes it for bv.am == MTFHIP_AM_SPSS) */
void launch_fused_spss(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const SpssArgs &sp,
	hipStream_t st);
/* kernels_spss.hip, the per-function entry points (SPSS.cc:116-225): f_vec summed into ACC_RR of the block rows (updateSimilarity); df_dIt
 * (curr = 1, updateCurrGrad) or df_dI0 (updateInitGrad) into `out`; the weighted Gram matrix sum w J J^T of a pixel Jacobian into ACC_H,
 * w = SPSS_W_* with df_dIt / df_dI0 read from their buffers as the reference reads its members */
void launch_spss_similarity(const BatchView &bv, double c, double *partials, int nblk, hipStream_t st);
void launch_spss_grad(const BatchView &bv, double c, int curr, double *out, hipStream_t st);
void launch_spss_hessian(const BatchView &bv, double c, int weight, const double *J, double *partials, int nblk, hipStream_t st);
/* kernels_fused_lrscv.hip: the LRSCV instantiations of the fused body (replay and tolerance mode) */
void launch_fused_lrscv(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const LrscvMap &lm,
	hipStream_t st);
/* kernels_fused_rscv.hip: the RSCV instantiations of the fused body (replay and tolerance mode) */
void launch_fused_rscv(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, const RscvMap &rm,
	hipStream_t st);
/* second-order path: hess_pts, image Hessians ([N][4]), SSM pixel Hessians ([S*S][N] planes), sum_p w[p] d2[:, p] */
void launch_hess_pts(const BatchView &bv, double eps, hipStream_t st);
void launch_img_hess(const BatchView &bv, const ImgView &im, const double *pts, double *hess, double eps, double mult, hipStream_t st);
void launch_warped_img_hess(const BatchView &bv, const ImgView &im, const double *pts, const double *hp, double *hess, double eps,
	double mult, hipStream_t st);
void launch_pix_hessian(const BatchView &bv, int variant, const double *hess, const double *grad, double *D, hipStream_t st);
void launch_weighted_plane_sum(const BatchView &bv, const double *d2a, const double *d2b, const double *w, double *partials, int nblk,
	double *out, hipStream_t st);
void launch_mean_planes(const double *a, const double *b, double *o, size_t n, hipStream_t st);
/* fused second-order term of the SSD Hessians, pixel-Hessian blocks in registers only; out[t][S*S] */
/* NCC weights for the fused second-order term: the fused NCC pass's partial rows of this iteration ([B][nblk][NCC_ACC_COUNT]) and
 * the template scalars ([B][8]: mean(I0), |I0 - mean|); rows == nullptr selects SSD's residual weights */
struct SecondOrderNcc { const double *rows; int nblk; const double *sc; };
/* MI weights for the fused second-order term (MI.cc:659-695: df_dI0 / df_dIt of the pixel): the gradient-factor tables of this
 * iteration ([B][MI_SIZE], k_mi_tables_iter) and the histogram normaliser; tb == nullptr: not MI.  Eight bins (the recompute passes). */
struct SecondOrderMi { const double *tb; double hist_norm; };
void launch_second_order_ssd(const BatchView &bv, const ImgView &im, int term, int chained, int d0_variant, double grad_eps,
	double hess_eps, double norm_mult, double norm_add, double *partials, int nblk, double *out, hipStream_t st, int own_pts = 0,
	SecondOrderNcc nc = SecondOrderNcc{nullptr, 0, nullptr}, SecondOrderMi mi = SecondOrderMi{nullptr, 0.0});
/* pre-processing / pyramid (float32 images) */
void launch_hist_eq(float *gray, int rows, int cols, unsigned *hist256, float *lut256, hipStream_t st);
void launch_to_gray(const void *raw, int rows, int cols, size_t stride_bytes, int channels, int depth_f32, float *out, hipStream_t st);
void launch_sym5(const float *src, float *tmp, float *dst, int rows, int cols, const float kx[3], const float ky[3], hipStream_t st);
void launch_pyr_down(const float *src, int srows, int scols, float *dst, int drows, int dcols, hipStream_t st);
void launch_resize_linear(const float *src, int srows, int scols, float *dst, int drows, int dcols, hipStream_t st);
/* NN dataset rows: features of C warped patches of target 0 (SSD: It, NCC: centred / normalised It) */
/* nt::NN's dataset generation in one launch (kernels_nn.hip) */
struct NnArgs {
	const double *perts_in;   /* [n_samples][S] device: the perturbations (any sampler of the SSM, made by the caller), or NULL: drawn on the device */
	double *perts_out;        /* [n_samples][S] device or NULL: the perturbations used (NN keeps them: ssm_perturbations, NT/NN.cc:141-147) */
	double sigma[8], mean[8]; /* ProjectiveBase::generatePerturbation: component k ~ N(mean_k, sigma_k) */
	unsigned long long seed;
	double base[9];           /* the SSM's current warp */
	int row_lo;               /* global index of the launch's first sample (row sharding: draws are keyed by the global index) */
	double norm_mult, norm_add;
	const double *base_dev;   /* device [9] or NULL: read the warp from here instead of `base` (the NN tracker's loop: the previous iteration moved it on the device) */
	const int *done;          /* device flag or NULL: every kernel of the launch returns at once when it is set (the NN tracker's loop) */
};
void launch_pair_image(const ImgView &im, float *pair /* [h][w][2] */, hipStream_t st);
hipError_t launch_nn_dataset(const BatchView &bv, const ImgView &im, const NnArgs &a, int count, double *feat, double *warps, const double *hull, hipStream_t st);
size_t nn_warps_bytes(int count);
bool nn_two_launch_ok(const BatchView &bv, const ImgView &im, int fast_math);
/* nt::NN's per-frame half (kernels_nn_search.hip): the exact search over the resident dataset, and the compositional update with the winner */
struct NnBest { double dist; int idx; int pad; };
constexpr int kNnSearchMaxFeat = 8000;   /* the query is staged in LDS: (feat_size + 2) doubles within the 64 KB a launch may ask for unasked */
int nn_search_resident(int ncc, int F);
int nn_search_blocks(int n_samples, int resident);
void launch_nn_search(int ncc, const double *feat, int n_samples, int F, const double *queries, int Q, NnBest *partials /* [Q][nblk] */, int nblk,
	const int *done, hipStream_t st);
void launch_nn_search_finish(const NnBest *partials, int nblk, int Q, int *idx, double *dist, hipStream_t st);
/* state: W (9) | corners (8) | init_corners_hm (12); ctl: done | n_iters; log[it]: best_idx | best_dist | update_norm */
void launch_nn_pick_update(int ssm, const NnBest *partials, int nblk, const double *perts, int n_samples, double *state, int *ctl, double *log, int it,
	double epsilon, hipStream_t st);
/* nt::NN's graph index gnn::GNN (kernels_gnn.hip; SM/src/NT/GNN.cc:30-203): the build -- all-pairs distances in row panels, the degree + 1
 * nearest of every row -- and the greedy walk, one step per launch pair */
struct GnnWalk { double parent_dist, best_dist; int cur, best_idx, start, n_steps, done, pad; };
constexpr int kGnnMaxList = 1024;   /* degree + 1 entries are sorted in LDS */
constexpr int kGnnTile = 64;        /* rows and columns of a workgroup's block of the distance matrix */
void launch_gnn_dist(int ncc, const double *feat, int n_samples, int F, int row_lo, int rows, double *dist /* [rows][n_samples] */, hipStream_t st);
void launch_gnn_select(const double *dist, int n_samples, int row_lo, int rows, int degree, int *graph /* [n_samples][degree] */, hipStream_t st);
int gnn_step_blocks(int degree);
/* start_nodes != NULL: walk q starts there; else random_start: drawn from (seed, *count + q); else at *handle_start.  *count += Q. */
void launch_gnn_init(GnnWalk *walks, int Q, const int *start_nodes, const int *handle_start, int random_start, unsigned long long seed,
	unsigned long long *count, int n_samples, const int *done, hipStream_t st);
/* begin: the start node's own distance (one row); else one step: the `degree` neighbours of the walk's node, and the reference's rule
 * applied by the workgroup that finishes last.  partials: [Q][nper]; tickets: [Q], zero between launches */
void launch_gnn_rows(int ncc, const double *feat, int n_samples, int F, const double *queries, int Q, const int *graph, int degree, GnnWalk *walks,
	NnBest *partials, unsigned *tickets, int nper, int max_steps, int begin, const int *done, hipStream_t st);
void launch_gnn_results(const GnnWalk *walks, int Q, int *idx, double *dist, int *n_steps, hipStream_t st);
/* the tracker's walk: (best_dist, best_idx) as the one partial k_nn_pick_update reads, the next search's start node, the log (start, n_steps) */
void launch_gnn_to_update(const GnnWalk *walk, NnBest *partial, int *handle_start, int *walk_log, int it, const int *done, hipStream_t st);
void launch_sample_candidates(const BatchView &bv, const ImgView &im, const double *dev_states, int C, double norm_mult,
	double norm_add, double *dev_feat, hipStream_t st);
/* whole ICLK loop in one launch, one workgroup per target (N <= 16 * kBlock); false if N is too large */
constexpr int kIclkTrackMaxPix = 8 * kBlock;   /* (the grid points of a thread's pixels stay in registers: k_iclk_track) */
/* k_grid_fb (kernels_grid_fb.hip): a frame's forward pass, the re-initialisation at the tracked location and the backward pass on the
 * previous frame in one launch; per patch the backward pass leaves 8 corners + its iteration count (-1: degenerate tracked corners) */
struct GridFbOut { double *host; double *dev; int reinit; };   /* [B][9] each: device-visible pinned memory | device memory (either may be NULL); reinit = fb_reinit: 0 = the backward pass keeps the forward pass's template and state (GridTracker.cc:297-299 skipped) */
bool launch_grid_fb(const BatchView &bv, const ImgView &im, const ImgView &imp, const mtfhip_sm_desc &sm, const TrackState &ts, const double *h0inv,
	const double *ncc_sc, double norm_mult, double norm_add, double grad_eps, const HostPublish &pub, const GridFbOut &fo, const RegionIngest &rg, hipStream_t st);
bool launch_iclk_track(const BatchView &bv, const ImgView &im, const mtfhip_sm_desc &sm, const TrackState &ts,
	const double *h0inv, const double *ncc_sc, double norm_mult, double norm_add, int fast_math, const HostPublish &pub, const RegionIngest &rg, hipStream_t st);
/* skip_off / skip_len (multiples of 16 bytes): a section that is left as it is on the device */
void launch_ingest_host(const void *src_host, void *dst, size_t bytes, hipStream_t st, size_t skip_off = 0, size_t skip_len = 0);
void launch_fused_mc(const BatchView &bv, const ImgView &im, const FusedArgs &fa, double *partials, int nblk, hipStream_t st);   /* bv.C > 1 */
/* a small patch's whole nt::ICLK::initialize in one launch (kernels_init.hip): template sample, gradient, steepest-descent rows,
 * moments, constant self Hessian and its inverse; the small results also go to a pinned host record of kInitRec doubles per target
 * (H0 64 | NCC scalars 8 | sum J0 8 | sum I0 J0 8 | Gram(J0) 36 | pad) behind the usual publish hand-over */
constexpr int kInitRec = 128;
constexpr int kTemplateInitMaxPix = 4 * 256;
struct InitPublish { double *host; int *count; unsigned long long *flag, seq; int fenced; };
void launch_template_init(const BatchView &bv, const ImgView &im, double grad_eps, double norm_mult, double norm_add, double *h0, double *h0inv,
	double *ncc, double *ncc_tm, const InitPublish &pub, const RegionIngest &rg, hipStream_t st);   /* rg.corners != NULL: the kernel lays out the grid itself */
/* one launch per pass with the finish folded in behind a last-arriver counter (kernels_step.hip); arrive: [B] ints, zero between launches */
bool track_step_available(const BatchView &bv, const FusedArgs &fa);
void launch_track_step(const BatchView &bv, const ImgView &im, const FusedArgs &fa, const mtfhip_sm_desc &sm, const TrackState &ts,
	double *partials, int nblk, int *arrive, hipStream_t st);
void launch_track_persist(const BatchView &bv, const ImgView &im, const FusedArgs &fa, const mtfhip_sm_desc &sm, const TrackState &ts,
	double *partials, int nblk, const PersistState &ps, int max_passes, hipStream_t st);
bool launch_init_grid_ingest(const BatchView &bv, const double *host_w0_dev, int resx, int resy, double lo_x, double lo_y,
	double hi_x, double hi_y, int force_unit_z, const void *src_host, void *dst, size_t bytes, int write_curr, hipStream_t st);
/* phase control of the two-queue loop (k_finish_track): this queue's and the other queue's time stamps, the fraction of a period to keep */
struct PhaseCtl { unsigned long long *mine; const unsigned long long *other; double frac; };
void launch_finish_track(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts, const double *partials,
	int nblk, hipStream_t st, PhaseCtl pc = PhaseCtl{nullptr, nullptr, 0.0}, const HostPublish &pub = HostPublish{nullptr, 0, 0, nullptr, nullptr, 0, 0}, int pub_t0 = 0);
/* the head of a chunked device-side loop in one launch (k_track_prologue): the slab ingest (src_host NULL: none; skip_*: launch_ingest_host's),
 * zero_i[n_zero_i] = 0, phase[0..3] = 0, the Levenberg-Marquardt start state lm[t] = {0, lm_delta_init, 0 ...} of n_lm targets, and the
 * arrival counter of the in-loop delivery *count = 0 (a call that failed between its passes can have left it part-counted)
 * (every pointer may be NULL) */
struct LoopWords { int *zero_i; int n_zero_i; unsigned long long *phase; double *lm; int n_lm; double lm_delta_init; int *count; };
void launch_track_prologue(const void *src_host, void *dst, size_t bytes, size_t skip_off, size_t skip_len, const LoopWords &lw, hipStream_t st);
/* kernels_fused_spss.hip: the finish over an SPSS pass's rows (launch_finish_track hands it bv.am == MTFHIP_AM_SPSS with its own block size) */
void launch_finish_track_spss(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts, const double *partials, int nblk,
	hipStream_t st, PhaseCtl pc, const HostPublish &pub, int pub_t0, dim3 block);

/* kernels_ssim.hip: the finish over an NCC pass's rows read as SSIM (mtfhip_sm_system.h: ssim_*), c1 and c2 the model's constants -- k_finish_track_ssim,
 * or k_finish_track_ssim_lo for ts.lo_ssm; the callers of launch_finish_track hand an SSIM batch's passes here instead.  And the kernels of
 * the per-function entry points (SSIM.cc:98-287): sum It, sum It^2, sum I0 It into ACC_G + 0 .. 2 of the block rows; df_dIt (curr = 1) or
 * df_dI0 into `out` from the per-target scalars sc ([B][8]: mo, mu, mult_factor, a, f c, grad_scal); the moments of the pixel Jacobian J
 * and of the current patch as a 72-wide NCC row per block */
void launch_finish_track_ssim(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts, const double *partials, int nblk,
	hipStream_t st, PhaseCtl pc, const HostPublish &pub, int pub_t0, double c1, double c2);
void launch_ssim_similarity(const BatchView &bv, double *partials, int nblk, hipStream_t st);
void launch_ssim_grad(const BatchView &bv, const double *sc, int curr, double *out, hipStream_t st);
void launch_ssim_hess(const BatchView &bv, const double *J, double *partials, int nblk, hipStream_t st);

/* ---- the additive search methods nt::FALK / nt::IALK (kernels_alk.hip) ---- */
struct AlkArgs {
	int ialk;            /* 0 FALK: gradient at the current points + cmptPixJacobian; 1 IALK: cmptApproxPixJacobian of dI0_dx */
	int materialize;     /* It, dIt_dx (FALK) and Jt are written to the interface buffers */
	int rows_per_block;  /* 256-pixel rows walked by one workgroup (fused_decomposition) */
	double grad_eps, norm_mult, norm_add;
	const int *active;   /* optional [B] mask: targets with 0 are skipped (device-side loop) */
};
/* the pixel pass: one partial row per workgroup, ACC_COUNT (SSD) or NCC_ACC_COUNT (NCC) wide, FCLK-type */
void launch_alk_pass(const BatchView &bv, const ImgView &im, const AlkArgs &a, double *partials, int nblk, hipStream_t st);
/* row sums, g and H by sm.hess_type (sm.sm = MTFHIP_SM_FCLK: the row's type), Levenberg-Marquardt, solve, additiveUpdate, convergence test */
void launch_alk_finish(const BatchView &bv, const mtfhip_sm_desc &sm, const TrackState &ts, const double *partials, int nblk, hipStream_t st);

/* ---- the SCV family's pass 1: workgroups per target, `chunks` 256-pixel chunks each, at most 64 (their rows are summed in order) ---- */
constexpr int kImapChunks = 8;         /* SCV, RSCV */
constexpr int kImapChunksLocal = 16;   /* LSCV, LRSCV: a workgroup zeroes and scans its whole (cell, bin) table */
inline int imap_hist_blocks(int N, int chunks) {
	const int nblk = ((N + kBlock - 1) / kBlock + chunks - 1) / chunks;
	return nblk < 1 ? 1 : (nblk > 64 ? 64 : nblk);
}

/* ---- the SCV family: SSD behind an intensity map (kernels_imap.hip) ---- */
constexpr int kImapMaxBins = 256;
/* LDS of a localized pass-1 workgroup: two u32 sums per (cell, bin); the re-map's maps, n_sub x n_bins doubles, stay within it too.  The
 * default dynamic-LDS limit: no kernel attribute raises it. */
constexpr int kLscvLdsBudget = 64 * 1024;
/* room left in the fused LRSCV pass's 64 KB of LDS for its own static arrays: the maps get the rest */
constexpr int kLrscvFusedStaticLds = 8 * 1024;
/* one argument block for the four models; every per-target pointer is offset to bv's first target.  SCV and LSCV key their sums by the
 * template's bin and re-map I0 (code16, i0o, wts); RSCV and LRSCV key them by the current patch's bin (code8).  The localized models add
 * the sub-region geometry (nx .. ncell, cell, crng) and sum per target (tot); SCV and RSCV sum per workgroup (part_f, part_u). */
struct ImapArgs {
	int nb, kind;                /* n_bins; how pass 1 obtains It: RSCV_IT_* (mtfhip_fused_dispatch.h) */
	int hist, linear, affine;    /* SCV's hist_type (0 Dirac, 1 Bilinear), weighted_mapping, affine_mapping */
	int nx, ny, ncx, ncell;      /* n_sub_regions_x / _y, cell columns, cells */
	double norm_mult, norm_add, grad_eps;
	const double *src;           /* [B][N] RSCV_IT_FROM_BUF (per-function path): MTFHIP_BUF_IT (SCV, LSCV), It_orig (RSCV, LRSCV) */
	const unsigned short *code16; /* [B][N] (int)I0_orig | (int)rint(I0_orig) << 8, clamped to [0, nb - 1] */
	const unsigned char *code8;  /* [B][N] (int)I0, clamped to [0, nb - 1] */
	const double *i0o;           /* [B][N] I0_orig */
	const unsigned short *cell;  /* [N] (one per batch) the pixel's cell, 0xffff outside every sub-region */
	const int *crng;             /* [2 nx + 2 ny] (one per batch) sub-region idx: cells cx in [crng[2 idx], crng[2 idx + 1]]; then idy: cy */
	const double *wts;           /* [nx ny][N] (one per batch) sub_region_wts, sub-region idy nx + idx */
	const int *active;           /* optional [B] mask: targets with 0 are skipped (device-side loop) */
	double *part_f;              /* [B][imap_hist_blocks(N, kImapChunks)][2 nb] per-workgroup sums (SCV) */
	unsigned *part_u;            /* ... (RSCV) */
	unsigned *tot;               /* [B][2][ncell nb] per-target sums, zero between launches */
	unsigned *arrive;            /* [B] arrival counters (0 between launches) */
	double *map;                 /* [B][nx ny][nb] (SCV, RSCV: [B][nb]) */
	double *aff;                 /* [B][nx ny][2] (affine_mapping) */
};
/* the template's bins, fixed until the template changes: ImapArgs::code16 of I0_orig, ::code8 of I0 */
void launch_scv_codes(int N, int B, int nb, const double *i0o, unsigned short *code, hipStream_t st);
void launch_rscv_codes(int N, int B, int nb, const double *i0, unsigned char *code, hipStream_t st);
/* SCV, LSCV: pass 1, the maps, then the re-map of I0 (MTFHIP_BUF_I0, offset to bv's first target) */
void launch_scv_update(const BatchView &bv, const ImgView &im, const ImapArgs &a, double *I0, hipStream_t st);
void launch_lscv_update(const BatchView &bv, const ImgView &im, const ImapArgs &a, double *I0, hipStream_t st);
/* RSCV, LRSCV: pass 1 and the maps (its last-arriving workgroup per target) */
void launch_rscv_hist(const BatchView &bv, const ImgView &im, const ImapArgs &a, hipStream_t st);
void launch_lrscv_hist(const BatchView &bv, const ImgView &im, const ImapArgs &a, hipStream_t st);
/* It = map(It_orig), or the blend of the mapped It_orig (the per-function route's updatePixVals); lm as the fused pass's, offset to target 0 */
void launch_rscv_apply(int N, int B, int nb, int linear, const double *map, const double *it_orig, double *It, hipStream_t st);
void launch_lrscv_apply(int N, int B, const LrscvMap &lm, const double *it_orig, double *It, hipStream_t st);

} // namespace mtfhip
#endif
