/*
 * CCREParams.h -- the reference's names for the CCRE model (AM/include/mtf/AM/CCRE.h, AM/src/CCRE.cc:13-52): CCREParams with its fields and
 * class defaults -- the HipLink in place of the AMParams base -- and class CCRE with its ParamType and params.  A caller that wrote
 * `CCRE(&ccre_params)` constructs this one: the HipAM of an MTFHIP_AM_CCRE pair ("ccre") whose histogram parameters are the block's.
 * n_blocks is the TBB / OpenMP block count: carried and ignored.  symmetrical_grad = 1 (CCRE.cc:680-767) is not available on the device
 * path: the block is refused with FunctonNotImplemented before any device call.
 */
#ifndef MTF_AMD_HOST_CCRE_PARAMS_H
#define MTF_AMD_HOST_CCRE_PARAMS_H
#include "HipModels.h"

namespace mtf {
namespace hip {

struct CCREParams : HipAMParams {
	int n_bins = 8;                     /* CCRE_N_BINS */
	bool partition_of_unity = false;    /* CCRE_POU */
	double pre_seed = 10;               /* CCRE_PRE_SEED */
	bool symmetrical_grad = false;      /* CCRE_SYMMETRICAL_GRAD */
	int n_blocks = 0;                   /* CCRE_N_BLOCKS */
	bool debug_mode = false;            /* CCRE_DEBUG_MODE */
	CCREParams() = default;
	CCREParams(std::shared_ptr<HipLink> link_, int _n_bins, bool _partition_of_unity, double _pre_seed, bool _symmetrical_grad, int _n_blocks,
		bool _debug_mode) : n_bins(_n_bins), partition_of_unity(_partition_of_unity), pre_seed(_pre_seed), symmetrical_grad(_symmetrical_grad),
		n_blocks(_n_blocks), debug_mode(_debug_mode) { link = link_; }
};
class CCRE : public HipAM {
public:
	typedef CCREParams ParamType;
	explicit CCRE(const ParamType *ccre_params, int _n_channels = 1) : HipAM(linked(ccre_params), _n_channels), params(*ccre_params) {}
	const ParamType params;
	/* the link's appearance model and histogram parameters are the block's, set before the pair is created (a pair that exists keeps what it
	 * was created with) */
	static const HipAMParams *linked(const ParamType *cp) {
		if (!cp || !cp->link) throw utils::InvalidArgument("CCRE :: the parameter block carries no HipLink (the AM and the SSM of a tracker share one)");
		if (cp->symmetrical_grad)
			throw utils::FunctonNotImplemented("CCRE :: symmetrical_grad = 1 is not available on the device path (CCRE.cc:680-767 is not restated)");
		cp->link->am = MTFHIP_AM_CCRE;
		cp->link->ccre.n_bins = cp->n_bins; cp->link->ccre.partition_of_unity = cp->partition_of_unity; cp->link->ccre.pre_seed = cp->pre_seed;
		return cp;
	}
};

} // namespace hip
} // namespace mtf
#endif
