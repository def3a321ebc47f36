/*
 * IALKParams.h -- the parameters of nt::IALK (SM/include/mtf/SM/IALKParams.h, defaults SM/src/IALKParams.cc:4-11) with the reference's
 * field names, for mtf::hip::LK(MTFHIP_SM_IALK, ...) and the harness's nt::IALK.  The device loop serves SSD and NCC, single channel,
 * first-order Hessians (sec_ord_hess must stay false there; the harness class carries it).
 */
#ifndef MTF_AMD_HOST_IALK_PARAMS_H
#define MTF_AMD_HOST_IALK_PARAMS_H

#include "SearchMethod.h"

namespace mtf {

struct IALKParams {
	enum HessType { InitialSelf, CurrentSelf, Std };   /* IALKParams.h:9 */
	int max_iters = 10;                  /* IALKParams.cc:4 */
	double epsilon = 0.01;               /* IALKParams.cc:5 */
	HessType hess_type = InitialSelf;    /* IALKParams.cc:6 */
	bool sec_ord_hess = false;           /* IALKParams.cc:7 */
	bool leven_marq = false;             /* IALKParams.cc:8 */
	double lm_delta_init = 0.01;         /* IALKParams.cc:9 */
	double lm_delta_update = 10;         /* IALKParams.cc:10 */
	bool debug_mode = false;
	/* the parameter block the search-method classes of this layer take */
	operator nt::SMParams() const {
		nt::SMParams p;
		p.max_iters = max_iters; p.epsilon = epsilon; p.hess_type = (int)hess_type; p.sec_ord_hess = sec_ord_hess;
		p.leven_marq = leven_marq; p.lm_delta_init = lm_delta_init; p.lm_delta_update = lm_delta_update;
		return p;
	}
};

} // namespace mtf
#endif
