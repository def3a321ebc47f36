"""ctypes loader of libmtfhip.so (the C-ABI declared in include/mtfhip.h).

There is no fallback: if the shared library is missing or a call fails, an exception is raised.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MTFHIP_LIB", os.path.join(_HERE, "libmtfhip.so"))
CSRC = os.path.join(_HERE, "csrc")

AM_SSD, AM_NCC, AM_MI, AM_SCV, AM_RSCV, AM_LSCV, AM_LRSCV, AM_SPSS, AM_SSIM, AM_CCRE = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
SCV_HIST_DIRAC, SCV_HIST_BILINEAR, SCV_HIST_BSPLINE = 0, 1, 2
SSM_HOMOGRAPHY, SSM_AFFINE, SSM_SIMILITUDE, SSM_ISOMETRY, SSM_TRANSLATION = 0, 1, 2, 3, 4
# state sizes (StateSpaceModel::getStateSize): Homography.cc:36, Affine.cc:47, Similitude.cc:63, Isometry.cc:52, Translation.cc:48
SSM_STATE_SIZE = {SSM_HOMOGRAPHY: 8, SSM_AFFINE: 6, SSM_SIMILITUDE: 4, SSM_ISOMETRY: 3, SSM_TRANSLATION: 2}
SSM_LOW_ORDER = (SSM_SIMILITUDE, SSM_ISOMETRY, SSM_TRANSLATION)
SM_ESM, SM_FCLK, SM_ICLK, SM_FALK, SM_IALK = 0, 1, 2, 3, 4
JAC_INIT, JAC_PIX, JAC_WARPED, JAC_APPROX = 0, 1, 2, 3
MATH_REPLAY, MATH_FAST = 0, 1
EST_RANSAC, EST_LMEDS, EST_LEAST_SQUARES = 0, 1, 2     # EstType SSMEstimatorParams.h:11
EST_MAX_PTS, EST_MAX_MODEL_PTS = 1024, 8
(BUF_I0, BUF_IT, BUF_DI0_DX, BUF_DIT_DX, BUF_DF_DI0, BUF_DF_DIT, BUF_J0, BUF_JT, BUF_JM,
 BUF_INIT_PTS, BUF_CURR_PTS, BUF_GRAD_PTS, BUF_INIT_Z, BUF_CURR_Z, BUF_INIT_HXY, BUF_CURR_HXY,
 BUF_D2I0_DX2, BUF_D2IT_DX2, BUF_HESS_PTS, BUF_D2I0_DP2, BUF_D2IT_DP2, BUF_D2IM_DP2) = range(22)


class MtfHipError(RuntimeError):
    """Mirror of mtf::utils::Exception (Utilities/include/mtf/Utilities/excpUtils.h:8-55)."""

    def __init__(self, code, msg):
        super().__init__("mtfhip error %d: %s" % (code, msg))
        self.code = code


class InvalidArgument(MtfHipError):
    pass


class FunctionNotImplemented(MtfHipError):
    pass


class LogicError(MtfHipError):
    pass


_ERR = {-1: InvalidArgument, -2: FunctionNotImplemented, -3: LogicError}


def ssm_state_size(ssm):
    try:
        return SSM_STATE_SIZE[int(ssm)]
    except KeyError:
        raise InvalidArgument(-1, "unknown state space model %r" % (ssm,))


class PatchDesc(C.Structure):
    _fields_ = [("am", C.c_int), ("ssm", C.c_int), ("resx", C.c_int), ("resy", C.c_int),
                ("grad_eps", C.c_double), ("likelihood_alpha", C.c_double), ("mi_n_bins", C.c_int),
                ("mi_pre_seed", C.c_double), ("mi_partition_of_unity", C.c_int), ("hess_eps", C.c_double),
                ("n_channels", C.c_int)]


class SMDesc(C.Structure):
    _fields_ = [("sm", C.c_int), ("jac_type", C.c_int), ("hess_type", C.c_int), ("chained_warp", C.c_int),
                ("materialize", C.c_int), ("max_iters", C.c_int), ("epsilon", C.c_double),
                ("leven_marq", C.c_int), ("lm_delta_init", C.c_double), ("lm_delta_update", C.c_double),
                ("sec_ord_hess", C.c_int)]


class PFDesc(C.Structure):
    _fields_ = [("n_particles", C.c_int), ("max_iters", C.c_int), ("epsilon", C.c_double), ("dynamic_model", C.c_int),
                ("update_type", C.c_int), ("likelihood_func", C.c_int), ("resampling_type", C.c_int), ("mean_type", C.c_int),
                ("corner_based_sampling", C.c_int), ("reset_to_mean", C.c_int), ("measurement_sigma", C.c_double),
                ("ar_coeff", C.c_double), ("ssm_sigma", C.c_double * 8), ("ssm_mean", C.c_double * 8), ("seed", C.c_ulonglong),
                ("pt_based_sampling", C.c_int), ("adaptive_resampling_thresh", C.c_double), ("update_distr_wts", C.c_int),
                ("min_distr_wt", C.c_double)]


class GridDesc(C.Structure):
    """mtfhip_grid_desc = GridTrackerParams (SM/src/GridTracker.cc:20-94)"""
    _fields_ = [("grid_size_x", C.c_int), ("grid_size_y", C.c_int), ("patch_size_x", C.c_int), ("patch_size_y", C.c_int),
                ("reset_at_each_frame", C.c_int), ("dyn_patch_size", C.c_int), ("patch_centroid_inside", C.c_int)]


class GridFbDesc(C.Structure):
    """mtfhip_grid_fb_desc: GridTrackerParams::fb_err_thresh / fb_reinit (SM/src/GridTracker.cc:186-190, 294-343) and est_params.n_model_pts"""
    _fields_ = [("fb_err_thresh", C.c_double), ("fb_reinit", C.c_int), ("n_model_pts", C.c_int)]


class EstParams(C.Structure):
    """mtfhip_est_params = SSMEstimatorParams (SSM/include/mtf/SSM/SSMEstimatorParams.h:11-25, defaults SSMEstimatorParams.cc:5-13)"""
    _fields_ = [("method", C.c_int), ("ransac_reproj_thresh", C.c_double), ("n_model_pts", C.c_int), ("max_iters", C.c_int),
                ("max_subset_attempts", C.c_int), ("confidence", C.c_double), ("refine", C.c_int), ("lm_max_iters", C.c_int)]


def est_params(method=EST_RANSAC, ransac_reproj_thresh=10.0, n_model_pts=4, refine=True, max_iters=2000, max_subset_attempts=300,
               confidence=0.995, lm_max_iters=10):
    """SSMEstimatorParams with the class defaults (SSMEstimatorParams.cc:5-13, argument order :42-44 without use_boost_rng); the shipped
    configuration (Config/modules.cfg:37-45) is est_params(EST_LMEDS, 5, 4, True, 10000, 300, 0.995, 10)"""
    return EstParams(int(method), float(ransac_reproj_thresh), int(n_model_pts), int(max_iters), int(max_subset_attempts), float(confidence),
                     int(bool(refine)), int(lm_max_iters))


def est_n_hyp(p):
    """the number of hypotheses the reference's loop can reach: max_iters for RANSAC (SSMEstimator.cc:81), the up-front count of LMedS
    (:172-173, cvRound = round half to even), one for plain least squares"""
    import math
    if p.method == EST_RANSAC:
        return p.max_iters
    if p.method == EST_LMEDS:
        return min(max(round(math.log(1 - p.confidence) / math.log(1 - math.pow(1 - 0.45, p.n_model_pts))), 3), p.max_iters)
    return 1


class FlowDesc(C.Structure):
    """mtfhip_flow_desc: NCC::estimateOpticalFlow's arguments (AM/src/NCC.cc:412-414; defaults GridTrackerFlowParams.h:6-17)"""
    _fields_ = [("win_w", C.c_int), ("win_h", C.c_int), ("max_iters", C.c_int), ("epsilon", C.c_double), ("const_grad", C.c_int),
                ("grad_eps", C.c_double), ("math_mode", C.c_int)]


FLOW_MAX_WIN, FLOW_TRACE_STRIDE = 1024, 8
FLOW_NONFINITE, FLOW_CONVERGED, FLOW_MAX_ITERS = 0, 1, 2


def flow_desc(win=(10, 10), max_iters=30, epsilon=0.01, const_grad=False, grad_eps=1e-8, math=MATH_FAST):
    """win: (width, height) of the search window, or one number for both"""
    w, h = (win, win) if isinstance(win, int) else (win[0], win[1])
    return FlowDesc(int(w), int(h), int(max_iters), float(epsilon), int(bool(const_grad)), float(grad_eps), int(math))


class NnDesc(C.Structure):
    """mtfhip_nn_desc: NN::generateDataset's parameters (SM/src/NT/NN.cc:56-84, 131-191)"""
    _fields_ = [("n_samples", C.c_int), ("additive_update", C.c_int), ("sigma", C.c_double * 8), ("mean", C.c_double * 8), ("seed", C.c_ulonglong)]


class GnnDesc(C.Structure):
    """mtfhip_gnn_desc: gnn::GNNParams (SM/src/GNNParams.cc:3-7) plus the seed of random_start's draws"""
    _fields_ = [("degree", C.c_int), ("max_steps", C.c_int), ("cmpt_dist_thresh", C.c_int), ("random_start", C.c_int), ("seed", C.c_ulonglong)]


NN_INDEX_EXACT, NN_INDEX_GNN = 0, 1


def gnn_desc(degree=250, max_steps=10, cmpt_dist_thresh=10000, random_start=False, seed=0, **_ignored):
    """the reference's defaults (SM/src/GNNParams.cc:3-7); `start_node` and other keys a GNNParams dict may carry are not the descriptor's"""
    d = GnnDesc()
    d.degree, d.max_steps, d.cmpt_dist_thresh, d.random_start, d.seed = int(degree), int(max_steps), int(cmpt_dist_thresh), int(bool(random_start)), int(seed)
    return d


# every exported symbol of include/mtfhip.h (tests check that the library exports all of them)
SYMBOLS = [
    "mtfhip_last_error", "mtfhip_device_count", "mtfhip_ctx_create", "mtfhip_ctx_destroy",
    "mtfhip_ctx_synchronize", "mtfhip_ctx_stream", "mtfhip_image_upload", "mtfhip_image_upload_mc", "mtfhip_image_borrow",
    "mtfhip_image_preprocess", "mtfhip_image_pyramid_level", "mtfhip_image_download", "mtfhip_image_shape",
    "mtfhip_batch_create", "mtfhip_batch_destroy", "mtfhip_batch_n_targets", "mtfhip_batch_n_pix", "mtfhip_batch_patch_size",
    "mtfhip_batch_state_size", "mtfhip_batch_set_math_mode", "mtfhip_batch_get_math_mode", "mtfhip_batch_read", "mtfhip_batch_write", "mtfhip_batch_device_ptr",
    "mtfhip_ssm_set_corners", "mtfhip_ssm_set_state", "mtfhip_ssm_compositional_update",
    "mtfhip_ssm_invert_state", "mtfhip_ssm_update_grad_pts", "mtfhip_ssm_cmpt_pix_jacobian",
    "mtfhip_ssm_get_corners", "mtfhip_ssm_get_init_corners", "mtfhip_ssm_get_state", "mtfhip_ssm_get_warp",
    "mtfhip_ssm_apply_warp_to_corners", "mtfhip_ssm_identity_warp", "mtfhip_ssm_compose_warps",
    "mtfhip_ssm_estimate_warp_from_corners", "mtfhip_ssm_apply_warp_to_pts", "mtfhip_ssm_additive_update",
    "mtfhip_am_initialize_pix_vals", "mtfhip_am_update_pix_vals", "mtfhip_am_update_model", "mtfhip_am_initialize_pix_grad",
    "mtfhip_am_update_pix_grad", "mtfhip_am_initialize_pix_grad_warped", "mtfhip_am_update_pix_grad_warped",
    "mtfhip_am_initialize_similarity", "mtfhip_am_initialize_grad", "mtfhip_am_initialize_hess",
    "mtfhip_am_update_similarity", "mtfhip_am_update_curr_grad", "mtfhip_am_update_init_grad",
    "mtfhip_am_get_similarity", "mtfhip_am_get_likelihood",
    "mtfhip_am_cmpt_init_jacobian", "mtfhip_am_cmpt_curr_jacobian", "mtfhip_am_cmpt_difference_of_jacobians",
    "mtfhip_am_cmpt_init_hessian", "mtfhip_am_cmpt_curr_hessian", "mtfhip_am_cmpt_self_hessian",
    "mtfhip_am_cmpt_sum_of_hessians", "mtfhip_sm_mean_jacobian",
    "mtfhip_ssm_update_hess_pts", "mtfhip_am_initialize_pix_hess", "mtfhip_am_update_pix_hess",
    "mtfhip_am_initialize_pix_hess_warped", "mtfhip_am_update_pix_hess_warped", "mtfhip_ssm_cmpt_pix_hessian",
    "mtfhip_sm_mean_pix_hessian", "mtfhip_am_cmpt_init_hessian2", "mtfhip_am_cmpt_curr_hessian2",
    "mtfhip_am_cmpt_self_hessian2", "mtfhip_am_cmpt_sum_of_hessians2",
    "mtfhip_batch_init_template", "mtfhip_batch_set_region", "mtfhip_batch_iterate", "mtfhip_batch_track", "mtfhip_batch_track_region", "mtfhip_grid_update",
    "mtfhip_grid_res", "mtfhip_grid_layout", "mtfhip_grid_frame", "mtfhip_grid_reset",
    "mtfhip_image_keep_prev", "mtfhip_image_has_prev", "mtfhip_image_swap_prev", "mtfhip_grid_backward", "mtfhip_grid_fb_mask", "mtfhip_grid_frame_fb",
    "mtfhip_batch_track_targets_per_launch",
    "mtfhip_score_candidates", "mtfhip_score_candidates_dev",
    "mtfhip_sample_candidates", "mtfhip_sample_candidates_dev", "mtfhip_nn_feature_size", "mtfhip_nn_dataset", "mtfhip_nn_dataset_dev",
    "mtfhip_pf_create", "mtfhip_pf_destroy", "mtfhip_pf_initialize", "mtfhip_pf_set_region", "mtfhip_pf_set_sampler",
    "mtfhip_pf_iteration", "mtfhip_pf_update", "mtfhip_pf_get_particles", "mtfhip_pf_set_particles", "mtfhip_pf_max_similarity",
    "mtfhip_pf_set_max_similarity", "mtfhip_pf_set_distributions", "mtfhip_pf_set_distr_draws", "mtfhip_pf_get_distributions", "mtfhip_comm_create_loopback", "mtfhip_pf_shard_bounds",
    "mtfhip_batch_track_trace", "mtfhip_batch_track_trace_read", "mtfhip_image_preprocess_ex",
    "mtfhip_comm_unique_id", "mtfhip_comm_create", "mtfhip_comm_destroy", "mtfhip_comm_rank", "mtfhip_comm_world",
    "mtfhip_allgather_scores", "mtfhip_pf_set_comm", "mtfhip_pf_set_exchange", "mtfhip_pf_exchange_export", "mtfhip_pf_exchange_connect", "mtfhip_comm_create_detached",
    "mtfhip_timing_enable", "mtfhip_timing_reset", "mtfhip_timing_get", "mtfhip_timing_get_busy", "mtfhip_ssm_estimate_state_sigma", "mtfhip_batch_track_queues", "mtfhip_batch_inline_warp",
    "mtfhip_batch_grid_regen", "mtfhip_batch_set_scv", "mtfhip_batch_scv_intensity_map", "mtfhip_batch_set_rscv",
    "mtfhip_batch_rscv_intensity_map", "mtfhip_batch_set_lscv", "mtfhip_batch_lscv_intensity_maps", "mtfhip_batch_set_first_iter",
    "mtfhip_batch_first_iter", "mtfhip_batch_set_lrscv", "mtfhip_batch_lrscv_intensity_maps", "mtfhip_batch_set_spss", "mtfhip_batch_set_ssim",
    "mtfhip_ssm_estimate_from_pts", "mtfhip_ssm_estimate_from_pts_dev",
    "mtfhip_nn_create", "mtfhip_nn_destroy", "mtfhip_nn_build", "mtfhip_nn_set_dataset", "mtfhip_nn_set_dataset_dev", "mtfhip_nn_get_dataset",
    "mtfhip_nn_get_dataset_dev", "mtfhip_nn_search", "mtfhip_nn_search_dev", "mtfhip_nn_update",
    "mtfhip_nn_gnn_build", "mtfhip_nn_gnn_get_graph", "mtfhip_nn_gnn_set_graph", "mtfhip_nn_gnn_search", "mtfhip_nn_gnn_search_dev",
    "mtfhip_nn_set_index", "mtfhip_nn_gnn_set_start", "mtfhip_nn_gnn_get_start", "mtfhip_nn_gnn_last_walks",
    "mtfhip_ncc_estimate_optical_flow", "mtfhip_ncc_estimate_optical_flow_dev", "mtfhip_ncc_estimate_optical_flow_trace",
]


def build(force=False):
    """Compile libmtfhip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + \
           [os.path.join(_HERE, "..", "include", "mtfhip.h")]
    newest = max(os.path.getmtime(p) for p in srcs)
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < newest:
        subprocess.check_call(["make", "-C", CSRC, "-s", "-B", "-j%d" % min(8, os.cpu_count() or 1)])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libmtfhip.so is missing (%s); build it with `python -c 'import __graft_entry__ as g; "
                              "g.build()'` -- there is no CPU fallback" % LIB_PATH)
        try:
            # PyTorch-ROCm bundles its own libamdhip64 (SONAME libamdhip64.so.7, requested by torch as the
            # unversioned name): loaded first, it also satisfies libmtfhip's libamdhip64.so.7 dependency and the
            # process ends up with ONE HIP runtime.  The other order loads two runtimes that fight over the device.
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.mtfhip_last_error.restype = C.c_char_p
        L.mtfhip_ctx_stream.restype = C.c_void_p
        L.mtfhip_batch_device_ptr.restype = C.c_void_p
        L.mtfhip_pf_max_similarity.restype = C.c_double
        L.mtfhip_ctx_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.mtfhip_batch_create.argtypes = [C.c_void_p, C.POINTER(PatchDesc), C.c_int, C.POINTER(C.c_void_p)]
        L.mtfhip_image_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.mtfhip_image_borrow.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.mtfhip_image_upload_mc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.mtfhip_image_preprocess.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_double, C.c_double]
        L.mtfhip_image_preprocess_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_double, C.c_double, C.c_int, C.c_double]
        L.mtfhip_image_pyramid_level.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.mtfhip_image_download.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.mtfhip_image_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mtfhip_grid_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtfhip_grid_res.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtfhip_grid_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtfhip_grid_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtfhip_grid_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mtfhip_image_keep_prev.argtypes = [C.c_void_p]
        L.mtfhip_image_has_prev.argtypes = [C.c_void_p]
        L.mtfhip_image_swap_prev.argtypes = [C.c_void_p]
        L.mtfhip_grid_backward.argtypes = [C.c_void_p] * 7
        L.mtfhip_grid_fb_mask.argtypes = [C.c_int] + [C.c_void_p] * 8
        L.mtfhip_grid_frame_fb.argtypes = [C.c_void_p] * 14
        L.mtfhip_ssm_update_grad_pts.argtypes = [C.c_void_p, C.c_double]
        L.mtfhip_ssm_update_hess_pts.argtypes = [C.c_void_p, C.c_double]
        for fn in ("mtfhip_am_initialize_pix_hess", "mtfhip_am_update_pix_hess"):
            getattr(L, fn).argtypes = [C.c_void_p, C.c_void_p]
        for fn in ("mtfhip_am_initialize_pix_hess_warped", "mtfhip_am_update_pix_hess_warped"):
            getattr(L, fn).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtfhip_ssm_cmpt_pix_hessian.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        for fn in ("mtfhip_am_cmpt_init_hessian2", "mtfhip_am_cmpt_curr_hessian2", "mtfhip_am_cmpt_self_hessian2"):
            getattr(L, fn).argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.mtfhip_am_cmpt_sum_of_hessians2.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.mtfhip_score_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mtfhip_score_candidates_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mtfhip_sample_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.mtfhip_sample_candidates_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.mtfhip_nn_feature_size.argtypes = [C.c_void_p, C.c_void_p]
        L.mtfhip_nn_dataset.argtypes = [C.c_void_p] * 5
        L.mtfhip_nn_dataset_dev.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int]
        L.mtfhip_batch_device_ptr.argtypes = [C.c_void_p, C.c_int]
        L.mtfhip_batch_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.mtfhip_batch_write.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.mtfhip_timing_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.mtfhip_batch_inline_warp.argtypes = [C.c_void_p]
        L.mtfhip_batch_grid_regen.argtypes = [C.c_void_p, C.c_void_p]
        L.mtfhip_batch_set_scv.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.mtfhip_batch_scv_intensity_map.argtypes = [C.c_void_p, C.c_void_p]
        L.mtfhip_batch_set_rscv.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.mtfhip_batch_rscv_intensity_map.argtypes = [C.c_void_p, C.c_void_p]
        L.mtfhip_batch_set_lscv.argtypes = [C.c_void_p] + [C.c_int] * 7
        L.mtfhip_batch_lscv_intensity_maps.argtypes = [C.c_void_p, C.c_void_p]
        L.mtfhip_batch_set_first_iter.argtypes = [C.c_void_p, C.c_int]
        L.mtfhip_batch_first_iter.argtypes = [C.c_void_p]
        L.mtfhip_batch_set_lrscv.argtypes = [C.c_void_p] + [C.c_int] * 7
        L.mtfhip_batch_lrscv_intensity_maps.argtypes = [C.c_void_p, C.c_void_p]
        L.mtfhip_batch_set_spss.argtypes = [C.c_void_p, C.c_double]
        L.mtfhip_batch_set_ssim.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.mtfhip_ssm_estimate_state_sigma.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        L.mtfhip_pf_set_distributions.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mtfhip_pf_set_distr_draws.argtypes = [C.c_void_p, C.c_void_p]
        L.mtfhip_pf_get_distributions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtfhip_ssm_estimate_from_pts.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_int, C.c_ulonglong] + [C.c_void_p] * 5
        L.mtfhip_ssm_estimate_from_pts_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_int, C.c_int, C.c_ulonglong] + [C.c_void_p] * 4
        L.mtfhip_timing_get_busy.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.mtfhip_nn_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.mtfhip_nn_destroy.argtypes = [C.c_void_p]
        L.mtfhip_nn_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        for fn in ("mtfhip_nn_set_dataset", "mtfhip_nn_set_dataset_dev", "mtfhip_nn_get_dataset", "mtfhip_nn_get_dataset_dev"):
            getattr(L, fn).argtypes = [C.c_void_p] * 3
        for fn in ("mtfhip_nn_search", "mtfhip_nn_search_dev"):
            getattr(L, fn).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mtfhip_nn_update.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtfhip_nn_gnn_build.argtypes = [C.c_void_p, C.c_void_p]
        for fn in ("mtfhip_nn_gnn_get_graph", "mtfhip_nn_gnn_set_graph", "mtfhip_nn_gnn_last_walks"):
            getattr(L, fn).argtypes = [C.c_void_p] * 3
        for fn in ("mtfhip_nn_gnn_search", "mtfhip_nn_gnn_search_dev"):
            getattr(L, fn).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtfhip_nn_set_index.argtypes = [C.c_void_p, C.c_int]
        L.mtfhip_nn_gnn_set_start.argtypes = [C.c_void_p, C.c_int]
        L.mtfhip_nn_gnn_get_start.argtypes = [C.c_void_p, C.c_void_p]
        for fn in ("mtfhip_ncc_estimate_optical_flow", "mtfhip_ncc_estimate_optical_flow_dev"):
            getattr(L, fn).argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.mtfhip_ncc_estimate_optical_flow_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
        _lib = L
    return _lib


def check(code):
    if code != 0:
        msg = lib().mtfhip_last_error().decode("utf-8", "replace")
        raise _ERR.get(code, MtfHipError)(code, msg)
