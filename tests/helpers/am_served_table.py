"""Which appearance model is served where at the C ABI, as a literal table: one row per (model, place), typed from the refusal helpers and
their call sites as they stood before mtf_amd/csrc/mtfhip_am_served.h replaced them (spss_refuse / ssim_refuse / ccre_refuse, scv_refuse,
refuse_intensity_mapped, the hand-formatted SCV-family lines of api_grid / api_nn / api_alk, kAmTraits' no_3ch and no_update_model).
None: served.  Otherwise the exact bytes of mtfhip_last_error() for an entry point named "FN" (the n_channels 3 and update_model texts
carry no entry point), with "FALK" as the search method's name at the additive place.

Refusals that depend on more than the model and the place are not in it and stay at their sites: MI at alk_check, sample_candidates and
nn_create, NCC's missing second-order self Hessian, SPSS with ESM SumOfStd, the low-order SSMs."""

SSD, NCC, MI, SCV, RSCV, LSCV, LRSCV, SPSS, SSIM, CCRE = range(10)      # include/mtfhip.h
MODELS = (SSD, NCC, MI, SCV, RSCV, LSCV, LRSCV, SPSS, SSIM, CCRE)
# the places in the order of the header's enum
PLACES = ("3ch", "update_model", "sec_ord", "additive", "grid", "score_candidates", "sample_candidates", "nn_dataset", "nn_create", "pf_create")

# MTFHIP_FIRST_ORDER_SERVED: what SPSS, SSIM and CCRE append to every refusal
_S = (" (served: the first-order per-function AppearanceModel entry points and init_template / set_region / iterate / track / track_region "
      "with ESM, FCLK and ICLK)")

REFUSALS = {
    (SSD, "3ch"): None,
    (SSD, "update_model"): None,
    (SSD, "sec_ord"): None,
    (SSD, "additive"): None,
    (SSD, "grid"): None,
    (SSD, "score_candidates"): None,
    (SSD, "sample_candidates"): None,
    (SSD, "nn_dataset"): None,
    (SSD, "nn_create"): None,
    (SSD, "pf_create"): None,

    (NCC, "3ch"): None,
    (NCC, "update_model"): None,
    (NCC, "sec_ord"): None,
    (NCC, "additive"): None,
    (NCC, "grid"): None,
    (NCC, "score_candidates"): None,
    (NCC, "sample_candidates"): None,
    (NCC, "nn_dataset"): None,
    (NCC, "nn_create"): None,
    (NCC, "pf_create"): None,

    (MI, "3ch"): None,
    (MI, "update_model"): "updateModel :: MI has no online template update in the reference either",
    (MI, "sec_ord"): None,
    (MI, "additive"): None,
    (MI, "grid"): None,
    (MI, "score_candidates"): None,
    (MI, "sample_candidates"): None,
    (MI, "nn_dataset"): None,
    (MI, "nn_create"): None,
    (MI, "pf_create"): None,

    (SCV, "3ch"): "SCV with n_channels 3 (MCSCV) is not available on the device path (single channel only)",
    (SCV, "update_model"): "updateModel :: SCV is not available on this entry point (the template update would have to refresh I0_orig)",
    (SCV, "sec_ord"): "FN: SCV with second-order Hessians is not available on the device path (first-order only)",
    (SCV, "additive"): "FN: FALK with SCV is not available on the device route (use nt::FALK over the per-function entry points)",
    (SCV, "grid"): "FN: SCV is not available on the grid tracker",
    (SCV, "score_candidates"): "FN: SCV candidates are not available (SCVDist is a per-candidate intensity map)",
    (SCV, "sample_candidates"): "FN: SCV distance features are not available (SCVDist is a per-candidate intensity map)",
    (SCV, "nn_dataset"): "FN: SCV is not available on the NN dataset (SCVDist is a per-candidate intensity map)",
    (SCV, "nn_create"): "FN: SCV is not available on the NN search (its distance functor is a per-candidate intensity map)",
    (SCV, "pf_create"): "FN: SCV is not available on the particle filter (SCVDist is a per-candidate intensity map)",

    (RSCV, "3ch"): "RSCV with n_channels 3 (MCRSCV) is not available on the device path (single channel only)",
    (RSCV, "update_model"): "updateModel :: RSCV is not available on this entry point (the template update would have to refresh its code plane)",
    (RSCV, "sec_ord"): "FN: RSCV with second-order Hessians is not available on the device path (first-order only)",
    (RSCV, "additive"): "FN: FALK with RSCV is not available on the device route (use nt::FALK over the per-function entry points)",
    (RSCV, "grid"): "FN: RSCV is not available on the grid tracker",
    (RSCV, "score_candidates"): "FN: RSCV candidates are not available (RSCVDist is a per-candidate intensity map)",
    (RSCV, "sample_candidates"): "FN: RSCV distance features are not available (RSCVDist is a per-candidate intensity map)",
    (RSCV, "nn_dataset"): "FN: RSCV is not available on the NN dataset (RSCVDist is a per-candidate intensity map)",
    (RSCV, "nn_create"): "FN: RSCV is not available on the NN search (its distance functor is a per-candidate intensity map)",
    (RSCV, "pf_create"): "FN: RSCV is not available on the particle filter (RSCVDist is a per-candidate intensity map)",

    (LSCV, "3ch"): "LSCV with n_channels 3 (MCLSCV) is not available on the device path (single channel only)",
    (LSCV, "update_model"): "updateModel :: LSCV is not available on this entry point (the template update would have to refresh I0_orig)",
    (LSCV, "sec_ord"): "FN: LSCV with second-order Hessians is not available on the device path (first-order only)",
    (LSCV, "additive"): "FN: FALK with LSCV is not available on the device route (use nt::FALK over the per-function entry points)",
    (LSCV, "grid"): "FN: LSCV is not available on the grid tracker",
    (LSCV, "score_candidates"): "FN: LSCV candidates are not available (LSCVDist is a per-candidate intensity map)",
    (LSCV, "sample_candidates"): "FN: LSCV distance features are not available (LSCVDist is a per-candidate intensity map)",
    (LSCV, "nn_dataset"): "FN: LSCV is not available on the NN dataset (LSCVDist is a per-candidate intensity map)",
    (LSCV, "nn_create"): "FN: LSCV is not available on the NN search (its distance functor is a per-candidate intensity map)",
    (LSCV, "pf_create"): "FN: LSCV is not available on the particle filter (LSCVDist is a per-candidate intensity map)",

    (LRSCV, "3ch"): "LRSCV with n_channels 3 is not available (no multi-channel LRSCV exists in the reference either)",
    (LRSCV, "update_model"): "updateModel :: LRSCV is not available on this entry point (the template update would have to refresh its code plane)",
    (LRSCV, "sec_ord"): "FN: LRSCV with second-order Hessians is not available on the device path (first-order only)",
    (LRSCV, "additive"): "FN: FALK with LRSCV is not available on the device route (use nt::FALK over the per-function entry points)",
    (LRSCV, "grid"): "FN: LRSCV is not available on the grid tracker",
    (LRSCV, "score_candidates"): "FN: LRSCV candidates are not available (its maps are per-candidate intensity maps)",
    (LRSCV, "sample_candidates"): "FN: LRSCV distance features are not available (its maps are per-candidate intensity maps)",
    (LRSCV, "nn_dataset"): "FN: LRSCV is not available on the NN dataset (its maps are per-candidate intensity maps)",
    (LRSCV, "nn_create"): "FN: LRSCV is not available on the NN search (its distance functor is a per-candidate intensity map)",
    (LRSCV, "pf_create"): "FN: LRSCV is not available on the particle filter (its maps are per-candidate intensity maps)",

    (SPSS, "3ch"): "SPSS with n_channels 3 (MCSPSS) is not available on the device path (single channel only)",
    (SPSS, "update_model"): "updateModel: SPSS has no online template update on the device path" + _S,
    (SPSS, "sec_ord"): "FN: SPSS with second-order Hessians is not available on the device path (first-order only)" + _S,
    (SPSS, "additive"): "FN: SPSS is not available with the additive search methods (FALK / IALK)" + _S,
    (SPSS, "grid"): "FN: SPSS is not available on this entry point" + _S,
    (SPSS, "score_candidates"): "FN: SPSS is not available on this entry point" + _S,
    (SPSS, "sample_candidates"): "FN: SPSS is not available on this entry point" + _S,
    (SPSS, "nn_dataset"): "FN: SPSS is not available on this entry point" + _S,
    (SPSS, "nn_create"): "FN: SPSS is not available on this entry point" + _S,
    (SPSS, "pf_create"): "FN: SPSS is not available on this entry point" + _S,

    (SSIM, "3ch"): "SSIM with n_channels 3 (MCSSIM) is not available on the device path (single channel only)",
    (SSIM, "update_model"): "updateModel: SSIM has no online template update (SSIM.cc has none either)" + _S,
    (SSIM, "sec_ord"): "FN: SSIM with second-order Hessians is not available on the device path (first-order only)" + _S,
    (SSIM, "additive"): "FN: SSIM is not available with the additive search methods (FALK / IALK)" + _S,
    (SSIM, "grid"): "FN: SSIM is not available on this entry point" + _S,
    (SSIM, "score_candidates"): "FN: SSIM is not available on this entry point" + _S,
    (SSIM, "sample_candidates"): "FN: SSIM is not available on this entry point" + _S,
    (SSIM, "nn_dataset"): "FN: SSIM is not available on this entry point" + _S,
    (SSIM, "nn_create"): "FN: SSIM is not available on this entry point" + _S,
    (SSIM, "pf_create"): "FN: SSIM is not available on this entry point" + _S,

    (CCRE, "3ch"): "CCRE with n_channels 3 (MCCCRE) is not available on the device path (single channel only)",
    (CCRE, "update_model"): "updateModel: CCRE has no online template update (CCRE.cc has none either)" + _S,
    (CCRE, "sec_ord"): "FN: CCRE with second-order Hessians is not available on the device path (first-order only)" + _S,
    (CCRE, "additive"): "FN: CCRE is not available with the additive search methods (FALK / IALK)" + _S,
    (CCRE, "grid"): "FN: CCRE is not available on this entry point" + _S,
    (CCRE, "score_candidates"): "FN: CCRE is not available on this entry point (CCREDist is a per-candidate histogram)" + _S,
    (CCRE, "sample_candidates"): "FN: CCRE is not available on this entry point (CCREDist is a per-candidate histogram)" + _S,
    (CCRE, "nn_dataset"): "FN: CCRE is not available on this entry point (CCREDist is a per-candidate histogram)" + _S,
    (CCRE, "nn_create"): "FN: CCRE is not available on this entry point (CCREDist is a per-candidate histogram)" + _S,
    (CCRE, "pf_create"): "FN: CCRE is not available on this entry point (CCREDist is a per-candidate histogram)" + _S,
}

# what else the model alone decides: name, whose rows its fused passes fill (0 SSD's, 1 NCC's, 2 MI's, 3 SPSS's), intensity-mapped /
# localized / reversed (the SCV family and the two axes inside it), served by the two-launch loop only (iclk_one_launch, persist_fits and
# track_takes_step turned the intensity-mapped models, SPSS and SSIM away), its device loop is its own histogram driver (hist_am: MI and
# CCRE), the limit of n_bins where the model reads it, and whether n_bins <= 0 selects that limit
TRAITS = {
    SSD: ("SSD", 0, 0, 0, 0, 0, 0, 0, 0),
    NCC: ("NCC", 1, 0, 0, 0, 0, 0, 0, 0),
    MI: ("MI", 2, 0, 0, 0, 0, 1, 16, 0),
    SCV: ("SCV", 0, 1, 0, 0, 1, 0, 256, 1),
    RSCV: ("RSCV", 0, 1, 0, 1, 1, 0, 256, 1),
    LSCV: ("LSCV", 0, 1, 1, 0, 1, 0, 256, 1),
    LRSCV: ("LRSCV", 0, 1, 1, 1, 1, 0, 256, 1),
    SPSS: ("SPSS", 3, 0, 0, 0, 1, 0, 0, 0),
    SSIM: ("SSIM", 1, 0, 0, 0, 1, 0, 0, 0),
    CCRE: ("CCRE", 2, 0, 0, 0, 0, 1, 16, 0),
}


def text(am, place, fn):
    """the table's text for the entry point fn, None where served"""
    t = REFUSALS[(am, place)]
    return fn + t[2:] if t is not None and t.startswith("FN: ") else t
