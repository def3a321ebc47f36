/*
 * FALKParams.h -- the parameters of nt::FALK (SM/include/mtf/SM/FALKParams.h, defaults SM/src/FALKParams.cc:3-15) with the reference's
 * field names, for mtf::hip::LK(MTFHIP_SM_FALK, ...) and the harness's nt::FALK.  The display switches (show_grid, show_patch,
 * patch_resize_factor, write_frames) have no counterpart.  The device loop serves SSD and NCC, single channel, first-order Hessians
 * (sec_ord_hess must stay false there; the harness class carries it).
 */
#ifndef MTF_AMD_HOST_FALK_PARAMS_H
#define MTF_AMD_HOST_FALK_PARAMS_H

#include "SearchMethod.h"

namespace mtf {

struct FALKParams {
	enum HessType { InitialSelf, CurrentSelf, Std };   /* FALKParams.h:9 */
	int max_iters = 10;                  /* FALKParams.cc:3 */
	double epsilon = 0.01;               /* FALKParams.cc:4 */
	HessType hess_type = InitialSelf;    /* FALKParams.cc:5 */
	bool sec_ord_hess = false;           /* FALKParams.cc:6 */
	bool enable_learning = false;        /* FALKParams.cc:11 */
	bool leven_marq = false;             /* FALKParams.cc:12 */
	double lm_delta_init = 0.01;         /* FALKParams.cc:13 */
	double lm_delta_update = 10;         /* FALKParams.cc:14 */
	bool debug_mode = false;
	/* the parameter block the search-method classes of this layer take */
	operator nt::SMParams() const {
		nt::SMParams p;
		p.max_iters = max_iters; p.epsilon = epsilon; p.hess_type = (int)hess_type; p.sec_ord_hess = sec_ord_hess;
		p.leven_marq = leven_marq; p.lm_delta_init = lm_delta_init; p.lm_delta_update = lm_delta_update; p.enable_learning = enable_learning;
		return p;
	}
};

} // namespace mtf
#endif
