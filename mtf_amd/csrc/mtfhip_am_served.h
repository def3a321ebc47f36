/*
 * mtfhip_am_served.h -- what the appearance model alone decides, stated once per model: its traits (kAmTraits, indexed by MTFHIP_AM_*) and
 * which places of the C ABI serve it or refuse it, with the refusal's text (am_refused).  Host-only and free of the HIP runtime (it needs
 * include/mtfhip.h for the enums and nothing else), so that the table can be checked by a stand-alone program
 * (tests/test_am_served_cpu.py, against the literal table of tests/helpers/am_served_table.py).
 *
 * A new appearance model adds its row here and a unit with its own code.  Refusals that depend on more than the model and the place stay
 * at their sites: NCC's missing second-order self Hessian and SPSS with ESM SumOfStd (check_sm), MI at alk_check, sample_candidates and
 * nn_create and its bin counts, LSCV / LRSCV once_per_frame with Levenberg-Marquardt FCLK, the low-order SSMs (lowdof_refuse).
 */
#ifndef MTFHIP_AM_SERVED_H
#define MTFHIP_AM_SERVED_H

#include <cstddef>
#include "../../include/mtfhip.h"

/* the places where a model can be refused: as many as the texts distinguish.  The first AM_AT_OWN_TEXTS have one text per model
 * (AmTraits::own_text), the others one format per way of refusing (kAmRefusal) */
enum {
	AM_AT_3_CHANNELS,          /* n_channels 3 at batch_create */
	AM_AT_UPDATE_MODEL,
	AM_AT_OWN_TEXTS,
	AM_AT_SEC_ORD_HESS = AM_AT_OWN_TEXTS,   /* check_sm with sec_ord_hess and the four *_hessian2 entry points */
	AM_AT_ADDITIVE_SM,         /* FALK / IALK (alk_check); the extra word is the search method's name */
	AM_AT_GRID,
	AM_AT_SCORE_CANDIDATES,
	AM_AT_SAMPLE_CANDIDATES,
	AM_AT_NN_DATASET,
	AM_AT_NN_CREATE,
	AM_AT_PF_CREATE,
	AM_AT_COUNT
};

#define MTFHIP_FIRST_ORDER_SERVED " (served: the first-order per-function AppearanceModel entry points and init_template / set_region / " \
	"iterate / track / track_region with ESM, FCLK and ICLK)"
/* The ways of refusing and their texts by place; NULL: served.  $f: the entry point, $a: the model's name, $x: the extra word,
 * $w: " (<AmTraits::no_candidates>)" where the model has one.  AM_REFUSES_AS_MAPPED: the SCV family, SSD behind an intensity map that has no
 * per-candidate form; AM_REFUSES_BUT_FIRST_ORDER: the models served by what MTFHIP_FIRST_ORDER_SERVED lists and nothing else */
enum { AM_REFUSES_NOTHING, AM_REFUSES_AS_MAPPED, AM_REFUSES_BUT_FIRST_ORDER };
constexpr const char *kAmRefusal[][AM_AT_COUNT - AM_AT_OWN_TEXTS] = {
	{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},
	{"$f: $a with second-order Hessians is not available on the device path (first-order only)",
		"$f: $x with $a is not available on the device route (use nt::$x over the per-function entry points)",
		"$f: $a is not available on the grid tracker",
		"$f: $a candidates are not available$w",
		"$f: $a distance features are not available$w",
		"$f: $a is not available on the NN dataset$w",
		"$f: $a is not available on the NN search (its distance functor is a per-candidate intensity map)",
		"$f: $a is not available on the particle filter$w"},
	{"$f: $a with second-order Hessians is not available on the device path (first-order only)" MTFHIP_FIRST_ORDER_SERVED,
		"$f: $a is not available with the additive search methods (FALK / IALK)" MTFHIP_FIRST_ORDER_SERVED,
		"$f: $a is not available on this entry point" MTFHIP_FIRST_ORDER_SERVED,
		"$f: $a is not available on this entry point$w" MTFHIP_FIRST_ORDER_SERVED,
		"$f: $a is not available on this entry point$w" MTFHIP_FIRST_ORDER_SERVED,
		"$f: $a is not available on this entry point$w" MTFHIP_FIRST_ORDER_SERVED,
		"$f: $a is not available on this entry point$w" MTFHIP_FIRST_ORDER_SERVED,
		"$f: $a is not available on this entry point$w" MTFHIP_FIRST_ORDER_SERVED},
};

/* rows: whose partial / reduced rows the model's fused passes fill.  intensity_mapped: an intensity map is rebuilt between the fused
 * passes (the SCV family); localized: one map per sub-region; reversed: the map is of the current patch.  loop_only: of the fused routes
 * only the two-launch loop serves it (fused_select), not the one-launch, persistent and step loops.  hist_driver: its iteration is a
 * histogram pipeline of its own behind a materialising SSD pass (mi_enqueue / ccre_enqueue) and its device loop is its own driver.
 * max_bins: the limit of mtfhip_patch_desc::mi_n_bins where the model reads it (0: it does not), bins_default: n_bins <= 0 selects
 * max_bins.  refuses: AM_REFUSES_*; own_text: the refusals at n_channels 3 and mtfhip_am_update_model (NULL: served); no_candidates: why the
 * model has no per-candidate form (candidates, particle filter, NN dataset), or NULL */
enum { AM_ROWS_SSD, AM_ROWS_NCC, AM_ROWS_MI, AM_ROWS_SPSS };
struct AmTraits {
	const char *name;
	int rows;
	bool intensity_mapped, localized, reversed, loop_only, hist_driver;
	int max_bins;
	bool bins_default;
	int refuses;
	const char *own_text[AM_AT_OWN_TEXTS], *no_candidates;
};
constexpr AmTraits kAmTraits[] = {
	{"SSD", AM_ROWS_SSD, false, false, false, false, false, 0, false, AM_REFUSES_NOTHING, {nullptr, nullptr}, nullptr},
	{"NCC", AM_ROWS_NCC, false, false, false, false, false, 0, false, AM_REFUSES_NOTHING, {nullptr, nullptr}, nullptr},
	{"MI", AM_ROWS_MI, false, false, false, false, true, 16, false, AM_REFUSES_NOTHING,
		{nullptr, "updateModel :: MI has no online template update in the reference either"}, nullptr},
	{"SCV", AM_ROWS_SSD, true, false, false, true, false, 256, true, AM_REFUSES_AS_MAPPED,
		{"SCV with n_channels 3 (MCSCV) is not available on the device path (single channel only)",
			"updateModel :: SCV is not available on this entry point (the template update would have to refresh I0_orig)"},
		"SCVDist is a per-candidate intensity map"},
	{"RSCV", AM_ROWS_SSD, true, false, true, true, false, 256, true, AM_REFUSES_AS_MAPPED,
		{"RSCV with n_channels 3 (MCRSCV) is not available on the device path (single channel only)",
			"updateModel :: RSCV is not available on this entry point (the template update would have to refresh its code plane)"},
		"RSCVDist is a per-candidate intensity map"},
	{"LSCV", AM_ROWS_SSD, true, true, false, true, false, 256, true, AM_REFUSES_AS_MAPPED,
		{"LSCV with n_channels 3 (MCLSCV) is not available on the device path (single channel only)",
			"updateModel :: LSCV is not available on this entry point (the template update would have to refresh I0_orig)"},
		"LSCVDist is a per-candidate intensity map"},
	{"LRSCV", AM_ROWS_SSD, true, true, true, true, false, 256, true, AM_REFUSES_AS_MAPPED,
		{"LRSCV with n_channels 3 is not available (no multi-channel LRSCV exists in the reference either)",
			"updateModel :: LRSCV is not available on this entry point (the template update would have to refresh its code plane)"},
		"its maps are per-candidate intensity maps"},
	{"SPSS", AM_ROWS_SPSS, false, false, false, true, false, 0, false, AM_REFUSES_BUT_FIRST_ORDER,
		{"SPSS with n_channels 3 (MCSPSS) is not available on the device path (single channel only)",
			"updateModel: SPSS has no online template update on the device path" MTFHIP_FIRST_ORDER_SERVED}, nullptr},
	{"SSIM", AM_ROWS_NCC, false, false, false, true, false, 0, false, AM_REFUSES_BUT_FIRST_ORDER,
		{"SSIM with n_channels 3 (MCSSIM) is not available on the device path (single channel only)",
			"updateModel: SSIM has no online template update (SSIM.cc has none either)" MTFHIP_FIRST_ORDER_SERVED}, nullptr},
	{"CCRE", AM_ROWS_MI, false, false, false, false, true, 16, false, AM_REFUSES_BUT_FIRST_ORDER,
		{"CCRE with n_channels 3 (MCCCRE) is not available on the device path (single channel only)",
			"updateModel: CCRE has no online template update (CCRE.cc has none either)" MTFHIP_FIRST_ORDER_SERVED},
		"CCREDist is a per-candidate histogram"},
};
static_assert(sizeof(kAmTraits) / sizeof(kAmTraits[0]) == MTFHIP_AM_CCRE + 1, "one row of traits per MTFHIP_AM_*");
static_assert(sizeof(kAmRefusal) / sizeof(kAmRefusal[0]) == AM_REFUSES_BUT_FIRST_ORDER + 1, "one row of formats per AM_REFUSES_*");
static inline const AmTraits &am_traits(int am) { return kAmTraits[am]; }   /* (am: a batch's, checked by mtfhip_batch_create) */

/* Is the model am (MTFHIP_AM_*) refused at place (AM_AT_*)?  false: served.  true: msg holds the refusal of the entry point fn, cut to
 * cap - 1 characters as a formatted print would cut it; extra: the place's extra word, or NULL */
static inline bool am_refused(int am, int place, const char *fn, const char *extra, char *msg, size_t cap) {
	const AmTraits &t = am_traits(am);
	const char *fmt = place < AM_AT_OWN_TEXTS ? t.own_text[place] : kAmRefusal[t.refuses][place - AM_AT_OWN_TEXTS];
	if (!fmt) return false;
	size_t n = 0;
	auto put = [&](const char *s) { for (; s && *s && n + 1 < cap; ++s) msg[n++] = *s; };
	for (const char *p = fmt; *p; ++p) {
		const char one[2] = {*p, 0};
		if (*p != '$') { put(one); continue; }
		switch (*++p) {
		case 'f': put(fn); break;
		case 'a': put(t.name); break;
		case 'x': put(extra); break;
		case 'w': if (t.no_candidates) { put(" ("); put(t.no_candidates); put(")"); } break;
		}
	}
	msg[n] = 0;
	return true;
}

#endif
