/*
 * HipModels.h -- AppearanceModel / StateSpaceModel subclasses whose data lives in HBM behind the C ABI
 * (include/mtfhip.h).  One HipPair (context + a batch of one target) is shared by the AM and the SSM of
 * a tracker.  References the two objects hand each other through the search method (PtsT, GradPtsT,
 * PixGradT, the SM-owned N x S Jacobians) are recognised BY ADDRESS: the bytes stay on the device and the
 * host objects are only keys; anything else is uploaded.  Host mirrors behind the getters are refreshed
 * lazily, when somebody actually asks ("host-resident interface vs device-resident data").
 */
#ifndef MTF_AMD_HOST_HIP_MODELS_H
#define MTF_AMD_HOST_HIP_MODELS_H

#include <map>
#include <memory>

#include "AppearanceModel.h"
#include "StateSpaceModel.h"
#include "SSMEstimatorParams.h"
#include "../../include/mtfhip.h"

namespace mtf {
namespace hip {

struct HipPair {
	mtfhip_ctx *ctx = nullptr;
	mtfhip_batch *b = nullptr;
	int am, ssm, resx, resy, N, S;   /* N = patch size = n_pix * n_channels */
	int n_pix, n_channels;
	double grad_eps, hess_eps = 1.0;
	/* addresses of host mirrors whose authoritative copy is a device buffer */
	const void *pts_key = nullptr, *grad_pts_key = nullptr, *init_grad_key = nullptr, *curr_grad_key = nullptr;
	const void *hess_pts_key = nullptr, *init_hess_key = nullptr, *curr_hess_key = nullptr;
	std::map<const void *, int> jac_keys;   /* SM-owned Jacobian matrices -> MTFHIP_BUF_J0 / _JT / _JM */
	std::map<const void *, int> hess_keys;  /* SM-owned pixel Hessians -> MTFHIP_BUF_D2I0_DP2 / _D2IT_DP2 / _D2IM_DP2 */
	int next_jac = 0, next_hess = 0;
	/* The host objects behind getPts(), getGradPts(), getCurrPixGrad() ... are keys: the adapters recognise them by address and
	 * their bytes stay on the device.  A reader that is NOT one of the adapters (the reference has a few: the SPI helpers next to
	 * NT/ESM.cc:466-472, NN's walk over ssm->getPts()) needs the bytes: with eager getters every such getter first reads its array
	 * back when a mutator has changed it since (a dirty flag per array) -- never stale, one D2H copy per changed array and getter
	 * call.  Off by default (the search methods call these getters every iteration only to pass the keys on);
	 * MTFHIP_EAGER_GETTERS=1 or setEagerGetters(true) turns it on. */
	bool eager_getters = false;
	void setEagerGetters(bool on) { eager_getters = on; }

	HipPair(int am, int ssm, int resx, int resy, double grad_eps, double likelihood_alpha, int mi_n_bins,
		double mi_pre_seed, int mi_pou, int device, void *stream, int n_channels = 1);
	~HipPair();
	static void check(int rc);               /* rethrows C-ABI failures as mtf::utils::Exception */
	int jacobianBuffer(const MatrixXd &J, bool may_register, int preferred = -1);
	void setSCV(int hist_type, bool weighted_mapping, bool mapped_gradient);   /* mtfhip_batch_set_scv (am = MTFHIP_AM_SCV) */
	void setRSCV(bool use_bspl, bool weighted_mapping, bool mapped_gradient);  /* mtfhip_batch_set_rscv (am = MTFHIP_AM_RSCV) */
	void setLSCV(int n_sub_regions_x, int n_sub_regions_y, int spacing_x, int spacing_y, bool affine_mapping, bool once_per_frame,
		bool weighted_mapping);                                                /* mtfhip_batch_set_lscv (am = MTFHIP_AM_LSCV) */
	void setLRSCV(int sub_regions_x, int sub_regions_y, int spacing_x, int spacing_y, bool affine_mapping, bool once_per_frame,
		bool weighted_mapping);                                                /* mtfhip_batch_set_lrscv (am = MTFHIP_AM_LRSCV) */
	void setSPSS(double k);                                                    /* mtfhip_batch_set_spss (am = MTFHIP_AM_SPSS) */
	void setSSIM(double k1, double k2);                                        /* mtfhip_batch_set_ssim (am = MTFHIP_AM_SSIM) */
	int hessianBuffer(const MatrixXd &D, bool may_register);
};

/* What the AM and the SSM of ONE tracker share, in the form the reference's templated search methods can carry it.
 * SearchMethod<AM, SSM> holds its models BY VALUE and builds them from `const AM::ParamType *` / `const SSM::ParamType *`
 * (SM/include/mtf/SM/SearchMethod.h:13-19, SM/src/ESM.cc:79-118; the models' own constructors: AM/include/mtf/AM/SSD.h
 * `SSD(const ParamType *ssd_params = nullptr, const int _n_channels = 1)`, SSM/include/mtf/SSM/Homography.h
 * `Homography(const ParamType *params_in = nullptr)`), so the two adapter objects cannot be handed a shared pair by the caller: both
 * parameter blocks point at one HipLink, and whichever model is constructed first creates the pair (context + one-target batch). */
/* SCVParams (AM/include/mtf/AM/SCV.h), the reference's field names and class defaults (SCV.cc:5-13).  n_bins <= 0 selects 256.
 * The device path serves hist_type Dirac (0) and Bilinear (1) with mapped_gradient off; pre_seed and partition_of_unity only act on the
 * BSpline histograms it refuses. */
struct HipSCVParams {
	int hist_type = 0; int n_bins = 256; double pre_seed = 0; bool partition_of_unity = false;
	bool weighted_mapping = false; bool mapped_gradient = false;
};
/* RSCVParams (AM/include/mtf/AM/RSCV.h), the reference's field names and class defaults (RSCV.cc:6-12).  n_bins <= 0 selects 256.
 * The device path serves use_bspl 0 (Dirac histograms) with mapped_gradient off; pre_seed and partition_of_unity only act on the BSpline
 * histograms it refuses, approx_dist_feat only on RSCVDist. */
struct HipRSCVParams {
	bool use_bspl = false; int n_bins = 256; double pre_seed = 0; bool partition_of_unity = false;
	bool weighted_mapping = false; bool mapped_gradient = false; bool approx_dist_feat = true;
};
/* LSCVParams (AM/include/mtf/AM/LSCV.h), the reference's field names and class defaults (LSCV.cc:8-16).  n_bins <= 0 selects 256.
 * pre_seed is accepted and ignored (updateSimilarity passes pre-seeds of 0, LSCV.cc:272-275), as are show_subregions (an OpenCV window)
 * and approx_dist_feat (LSCVDist only). */
struct HipLSCVParams {
	int n_sub_regions_x = 3, n_sub_regions_y = 3; int spacing_x = 10, spacing_y = 10;
	bool affine_mapping = false; bool once_per_frame = false; int n_bins = 256; double pre_seed = 0;
	bool weighted_mapping = false; bool show_subregions = false; bool approx_dist_feat = false;
};
/* LRSCVParams (AM/include/mtf/AM/LRSCV.h), the reference's field names and class defaults (LRSCV.cc:40-52).  n_bins <= 0 selects 256.
 * pre_seed is accepted and ignored (updatePixVals passes pre-seeds of 0, LRSCV.cc:240-243), as are show_subregions (an OpenCV window)
 * and debug_mode. */
struct HipLRSCVParams {
	int sub_regions_x = 3, sub_regions_y = 3; int spacing_x = 10, spacing_y = 10;
	bool affine_mapping = false; bool once_per_frame = false; int n_bins = 256; double pre_seed = 0;
	bool weighted_mapping = false; bool show_subregions = false; bool debug_mode = false;
};
/* SPSSParams (AM/include/mtf/AM/SPSS.h), the reference's field names; k: the shipped spss_k (Config/modules.cfg), c = (255 k)^2.  A
 * pix_mapper (an ImageBase the pixel values are taken through) is not available on the device path: SPSS reads the raw samples. */
struct HipSPSSParams {
	double k = 0.01;
};
/* SSIMParams (AM/include/mtf/AM/SSIM.h), the reference's field names and class defaults (SSIM.cc:4-5: the shipped ssim_k1, ssim_k2):
 * c1 = (255 k1)^2, c2 = (255 k2)^2 */
struct HipSSIMParams {
	double k1 = 0.01, k2 = 0.03;
};
/* the histogram parameters of CCREParams (CCREParams.h; AM/src/CCRE.cc:13-18) as they travel to mtfhip_patch_desc::mi_n_bins / mi_pre_seed /
 * mi_partition_of_unity */
struct HipCCREParams {
	int n_bins = 8; bool partition_of_unity = false; double pre_seed = 10;
};
struct HipLink {
	int am = MTFHIP_AM_SSD, ssm = MTFHIP_SSM_HOMOGRAPHY, resx = 50, resy = 50;   /* AMParams / SSMParams: resx, resy */
	double grad_eps = 1e-8, likelihood_alpha = 1.0;                           /* AMParams::grad_eps; SSDParams / NCCParams / MIParams::likelihood_alpha */
	int mi_n_bins = 8; double mi_pre_seed = 10; int mi_pou = 0;                /* MIParams */
	HipSCVParams scv;                                                          /* am = MTFHIP_AM_SCV ("scv") */
	HipRSCVParams rscv;                                                        /* am = MTFHIP_AM_RSCV ("rscv") */
	HipLSCVParams lscv;                                                        /* am = MTFHIP_AM_LSCV ("lscv") */
	HipLRSCVParams lrscv;                                                      /* am = MTFHIP_AM_LRSCV ("lrscv", "lrsc") */
	HipSPSSParams spss;                                                        /* am = MTFHIP_AM_SPSS ("spss") */
	HipSSIMParams ssim;                                                        /* am = MTFHIP_AM_SSIM ("ssim") */
	HipCCREParams ccre;                                                        /* am = MTFHIP_AM_CCRE ("ccre") */
	int device = 0; void *stream = nullptr;
	std::shared_ptr<HipPair> pair(int n_channels = 1) {
		if (!p && am == MTFHIP_AM_SCV) {
			p = std::make_shared<HipPair>(am, ssm, resx, resy, grad_eps, likelihood_alpha, scv.n_bins, scv.pre_seed, scv.partition_of_unity ? 1 : 0,
				device, stream, n_channels);
			p->setSCV(scv.hist_type, scv.weighted_mapping, scv.mapped_gradient);
		}
		if (!p && am == MTFHIP_AM_RSCV) {
			p = std::make_shared<HipPair>(am, ssm, resx, resy, grad_eps, likelihood_alpha, rscv.n_bins, rscv.pre_seed, rscv.partition_of_unity ? 1 : 0,
				device, stream, n_channels);
			p->setRSCV(rscv.use_bspl, rscv.weighted_mapping, rscv.mapped_gradient);
		}
		if (!p && am == MTFHIP_AM_LSCV) {
			p = std::make_shared<HipPair>(am, ssm, resx, resy, grad_eps, likelihood_alpha, lscv.n_bins, lscv.pre_seed, 0, device, stream, n_channels);
			p->setLSCV(lscv.n_sub_regions_x, lscv.n_sub_regions_y, lscv.spacing_x, lscv.spacing_y, lscv.affine_mapping, lscv.once_per_frame,
				lscv.weighted_mapping);
		}
		if (!p && am == MTFHIP_AM_LRSCV) {
			p = std::make_shared<HipPair>(am, ssm, resx, resy, grad_eps, likelihood_alpha, lrscv.n_bins, lrscv.pre_seed, 0, device, stream, n_channels);
			p->setLRSCV(lrscv.sub_regions_x, lrscv.sub_regions_y, lrscv.spacing_x, lrscv.spacing_y, lrscv.affine_mapping, lrscv.once_per_frame,
				lrscv.weighted_mapping);
		}
		if (!p && am == MTFHIP_AM_SPSS) {
			p = std::make_shared<HipPair>(am, ssm, resx, resy, grad_eps, likelihood_alpha, 0, 0.0, 0, device, stream, n_channels);
			p->setSPSS(spss.k);
		}
		if (!p && am == MTFHIP_AM_SSIM) {
			p = std::make_shared<HipPair>(am, ssm, resx, resy, grad_eps, likelihood_alpha, 0, 0.0, 0, device, stream, n_channels);
			p->setSSIM(ssim.k1, ssim.k2);
		}
		if (!p && am == MTFHIP_AM_CCRE)
			p = std::make_shared<HipPair>(am, ssm, resx, resy, grad_eps, likelihood_alpha, ccre.n_bins, ccre.pre_seed, ccre.partition_of_unity ? 1 : 0,
				device, stream, n_channels);
		if (!p) p = std::make_shared<HipPair>(am, ssm, resx, resy, grad_eps, likelihood_alpha, mi_n_bins, mi_pre_seed, mi_pou, device, stream, n_channels);
		else if (n_channels > 1 && n_channels != p->n_channels)   /* (SearchMethod<AM, SSM> constructs the AM first: it fixes the channel count) */
			throw utils::InvalidArgument("HipLink :: the pair exists with another channel count");
		return p;
	}
private:
	std::shared_ptr<HipPair> p;
};
struct HipAMParams { std::shared_ptr<HipLink> link; double learning_rate = 0.5; };
struct HipSSMParams { std::shared_ptr<HipLink> link; bool corner_based_sampling = true; int pt_based_sampling = 0; };

class HipAM : public AppearanceModel {
public:
	typedef HipAMParams ParamType;
	HipAM(std::shared_ptr<HipPair> pair);
	/* the constructor SearchMethod<AM, SSM> calls (am(am_params): n_channels defaults as in the reference's models) */
	explicit HipAM(const ParamType *params, int n_channels = 1);
	unsigned int getResX() const override { return p->resx; }
	unsigned int getResY() const override { return p->resy; }
	unsigned int getNPix() const override { return p->n_pix; }
	unsigned int getNChannels() const override { return p->n_channels; }   /* MCSSD / MCNCC / MCMI: 3 */
	unsigned int getPatchSize() const override { return p->N; }
	double getGradOffset() const override { return p->grad_eps; }
	double getHessOffset() const override { return p->hess_eps; }
	const PixValT &getInitPixVals() override;
	const PixValT &getCurrPixVals() override;
	const PixGradT &getInitPixGrad() override { return fresh(dI0_dx, MTFHIP_BUF_DI0_DX, d_dI0); }   /* key; bytes on the device unless eager */
	const PixGradT &getCurrPixGrad() override { return fresh(dIt_dx, MTFHIP_BUF_DIT_DX, d_dIt); }
	const PixHessT &getInitPixHess() override { return fresh(d2I0_dx2, MTFHIP_BUF_D2I0_DX2, d_h0); }
	const PixHessT &getCurrPixHess() override { return fresh(d2It_dx2, MTFHIP_BUF_D2IT_DX2, d_ht); }
	void syncPixGrad();                                               /* explicit read-back of both gradients */

	void setCurrImg(const ImageView &img) override;
#ifdef MTF_AMD_USE_OPENCV
	void setCurrImg(const cv::Mat &img) { setCurrImg(imageView(img)); }   /* the reference's signature (ImageBase.h:92) */
#endif
	void initializePixVals(const PtsT &init_pts) override;
	void initializePixGrad(const GradPtsT &warped_offset_pts) override;
	void initializePixGrad(const PtsT &init_pts) override;
	void updatePixVals(const PtsT &curr_pts) override;
	void updatePixGrad(const GradPtsT &warped_offset_pts) override;
	void updatePixGrad(const PtsT &curr_pts) override;
	void initializePixHess(const PtsT &init_pts, const HessPtsT &warped_offset_pts) override;
	void initializePixHess(const PtsT &init_pts) override;
	void updatePixHess(const PtsT &curr_pts, const HessPtsT &warped_offset_pts) override;
	void updatePixHess(const PtsT &curr_pts) override;

	double getSimilarity() const override;
	double getLikelihood() const override;
	void initializeSimilarity() override;
	void initializeGrad() override;
	void initializeHess() override;
	void updateSimilarity(bool prereq_only = true) override;
	void updateInitGrad() override;
	void updateCurrGrad() override;
	/* online template update (enable_learning of the search methods); learning_rate as SSDParams / NCCParams (default 0.5,
	 * Config/parameters.h:200), outside [0, 1] = running average */
	void updateModel(const PtsT &curr_pts) override;
	void setLearningRate(double lr) { learning_rate = lr; }
	/* NCC::estimateOpticalFlow (AM/src/NCC.cc:412-526; AppearanceModel.h:221-226 throws FunctonNotImplemented for every other model, and so
	 * does this): the translation-only NCC flow of prev_pts on a win_w x win_h lattice, all points in one launch (mtfhip_ncc_estimate_optical_flow).
	 * prev_img is not an argument: it is the frame keepPrevImg() kept on the device (prev_img = curr_img.clone() without the copy).
	 * A point whose step is not finite comes back as NaN; n_iters / status (may be NULL): passes run and MTFHIP_FLOW_* per point. */
	void estimateOpticalFlow(std::vector<EstPt> &curr_pts, const std::vector<EstPt> &prev_pts, int win_w, int win_h, unsigned int n_pts, int max_iters,
		double term_eps, bool const_grad, int math_mode = MTFHIP_MATH_FAST, std::vector<int> *n_iters = nullptr, std::vector<int> *status = nullptr) const;
	void keepPrevImg();
	/* NN / FLANN distance feature of the patch at the SSM's current state: SSD = the pixel values (SSDBase.h:116-125), NCC =
	 * centred and normalised (NCC.cc:530-537); computed on the device (mtfhip_sample_candidates), MI has none here */
	void initializeDistFeat() override { dist_feat.resize((int)p->N); }
	void updateDistFeat() override { if (dist_feat.size() != (int)p->N) dist_feat.resize((int)p->N); updateDistFeat(dist_feat.data()); }
	void updateDistFeat(double *feat_addr) override;
	const double *getDistFeat() override { return dist_feat.data(); }
	unsigned int getDistFeatSize() override { return p->N; }
	void cmptInitJacobian(RowVectorXd &df_dp, const MatrixXd &dI0_dpssm) override;
	void cmptCurrJacobian(RowVectorXd &df_dp, const MatrixXd &dIt_dpssm) override;
	void cmptDifferenceOfJacobians(RowVectorXd &df_dp_diff, const MatrixXd &dI0_dpssm, const MatrixXd &dIt_dpssm) override;
	void cmptInitHessian(MatrixXd &H, const MatrixXd &dI0_dpssm) override;
	void cmptCurrHessian(MatrixXd &H, const MatrixXd &dIt_dpssm) override;
	void cmptSelfHessian(MatrixXd &H, const MatrixXd &dIt_dpssm) override;
	void cmptSumOfHessians(MatrixXd &H, const MatrixXd &dI0_dpssm, const MatrixXd &dIt_dpssm) override;
	void cmptInitHessian(MatrixXd &H, const MatrixXd &dI0_dpssm, const MatrixXd &d2I0_dpssm2) override;
	void cmptCurrHessian(MatrixXd &H, const MatrixXd &dIt_dpssm, const MatrixXd &d2It_dpssm2) override;
	void cmptSelfHessian(MatrixXd &H, const MatrixXd &dIt_dpssm, const MatrixXd &d2It_dpssm2) override;
	void cmptSumOfHessians(MatrixXd &H, const MatrixXd &dI0_dpssm, const MatrixXd &dIt_dpssm, const MatrixXd &d2I0_dpssm2,
		const MatrixXd &d2It_dpssm2) override;
	void cmptMeanOf(MatrixXd &mean, const MatrixXd &a, const MatrixXd &b) override;
	void setFirstIter() override;
	void clearFirstIter() override;
	void clearInitStatus() override {}
private:
	double learning_rate = 0.5;
	VectorXd dist_feat;
	std::shared_ptr<HipPair> p;
public:
	const std::shared_ptr<HipPair> &pair() const { return p; }
	/* a device-side driver (hip::LK: mtfhip_batch_init_template / track / set_region) rewrote the AM's arrays behind this object */
	void markDeviceUpdated() { d_dI0 = d_dIt = d_h0 = d_ht = true; f_fresh = false; }
private:
	ImageView img{nullptr, 0, 0, 0};
	mutable double f = 0;
	mutable bool f_fresh = true;
	PixValT I0, It;
	PixGradT dI0_dx, dIt_dx;
	PixHessT d2I0_dx2, d2It_dx2;
	bool d_dI0 = false, d_dIt = false, d_h0 = false, d_ht = false;   /* host mirror older than the device array */
	template <typename T> const T &fresh(T &m, int buf, bool &dirty) {
		if (p->eager_getters && dirty) { HipPair::check(mtfhip_batch_read(p->b, buf, m.data())); dirty = false; }
		return m;
	}
	const double *hessPtsArg(const HessPtsT &pts) const;
	const double *ptsArg(const PtsT &pts) const;
	const double *gradPtsArg(const GradPtsT &pts) const;
	static void colMajorToHost(MatrixXd &H, const double *src, int S);
};

/* The reference's names for the SPSS model (AM/include/mtf/AM/SPSS.h): SPSSParams {k} -- with the HipLink every device parameter block
 * carries in place of the AMParams base -- and class SPSS with its ParamType, params and c = (k (PIX_MAX - PIX_MIN))^2 (SPSS.cc:37-38).  A caller that
 * wrote `SPSS(&spss_params)` constructs this one: the HipAM of an MTFHIP_AM_SPSS pair whose k is the block's.  No pix_mapper (not available on
 * the device path). */
struct SPSSParams : HipAMParams {
	double k = 0.01;
	SPSSParams() = default;
	SPSSParams(std::shared_ptr<HipLink> link_, double k_) : k(k_) { link = link_; }
};
class SPSS : public HipAM {
public:
	typedef SPSSParams ParamType;
	explicit SPSS(const ParamType *spss_params, int _n_channels = 1) : HipAM(linked(spss_params), _n_channels), params(*spss_params),
		c((params.k > 0 ? params.k : 0.01) * 255.0 * ((params.k > 0 ? params.k : 0.01) * 255.0)) {}
	const ParamType params;
	const double c;
private:
	/* the link's appearance model and k are the block's, set before the pair is created (a pair that exists keeps what it was created with) */
	static const HipAMParams *linked(const ParamType *sp) {
		if (!sp || !sp->link) throw utils::InvalidArgument("SPSS :: the parameter block carries no HipLink (the AM and the SSM of a tracker share one)");
		sp->link->am = MTFHIP_AM_SPSS;
		sp->link->spss.k = sp->k;
		return sp;
	}
};

/* The reference's names for the SSIM model (AM/include/mtf/AM/SSIM.h): SSIMParams {k1, k2} -- with the HipLink in place of the AMParams base --
 * and class SSIM with its ParamType, params and c1 = (k1 (PIX_MAX - PIX_MIN))^2, c2 likewise (SSIM.cc:36-39).  A caller that wrote
 * `SSIM(&ssim_params)` constructs this one: the HipAM of an MTFHIP_AM_SSIM pair whose constants are the block's. */
struct SSIMParams : HipAMParams {
	double k1 = 0.01, k2 = 0.03;
	SSIMParams() = default;
	SSIMParams(std::shared_ptr<HipLink> link_, double k1_, double k2_) : k1(k1_), k2(k2_) { link = link_; }
};
class SSIM : public HipAM {
public:
	typedef SSIMParams ParamType;
	explicit SSIM(const ParamType *ssim_params, int _n_channels = 1) : HipAM(linked(ssim_params), _n_channels), params(*ssim_params),
		c1(sq255(params.k1, 0.01)), c2(sq255(params.k2, 0.03)) {}
	const ParamType params;
	const double c1, c2;
private:
	static double sq255(double k, double dflt) { const double c = (k > 0 ? k : dflt) * 255.0; return c * c; }
	/* the link's appearance model and constants are the block's, set before the pair is created (a pair that exists keeps what it was created with) */
	static const HipAMParams *linked(const ParamType *sp) {
		if (!sp || !sp->link) throw utils::InvalidArgument("SSIM :: the parameter block carries no HipLink (the AM and the SSM of a tracker share one)");
		sp->link->am = MTFHIP_AM_SSIM;
		sp->link->ssim.k1 = sp->k1; sp->link->ssim.k2 = sp->k2;
		return sp;
	}
};

class HipSSM : public StateSpaceModel {
public:
	typedef HipSSMParams ParamType;
	HipSSM(std::shared_ptr<HipPair> pair);
	explicit HipSSM(const ParamType *params);   /* ssm(ssm_params) of SearchMethod<AM, SSM> */
	unsigned int getStateSize() override { return p->S; }
	unsigned int getResX() override { return p->resx; }
	unsigned int getResY() override { return p->resy; }
	unsigned int getNPts() override { return p->n_pix; }
	const PtsT &getPts() override { return fresh(curr_pts, MTFHIP_BUF_CURR_PTS, d_pts); }   /* key; syncPts() / eager getters refresh the bytes */
	const GradPtsT &getGradPts() override { return fresh(grad_pts, MTFHIP_BUF_GRAD_PTS, d_gpts); }
	const HessPtsT &getHessPts() override { return fresh(hess_pts, MTFHIP_BUF_HESS_PTS, d_hpts); }
	/* corners and state live in host memory behind the C ABI: always current, also after the device-side drivers
	 * (mtfhip_batch_track, mtfhip_pf_update) moved the SSM without going through this object */
	const CornersT &getCorners() override { syncSmall(); return curr_corners; }
	const VectorXd &getState() override { syncSmall(); return curr_state; }
	void syncPts();

	void setState(const VectorXd &ssm_state) override;
	void setCorners(const CornersT &corners) override;
	void compositionalUpdate(const VectorXd &state_update) override;
	void updateGradPts(double grad_eps) override;
	void updateHessPts(double hess_eps) override;
	void invertState(VectorXd &inv_state, const VectorXd &state) override;
	void cmptInitPixJacobian(MatrixXd &J, const PixGradT &g) override { jac(MTFHIP_JAC_INIT, J, g); }
	void cmptPixJacobian(MatrixXd &J, const PixGradT &g) override { jac(MTFHIP_JAC_PIX, J, g); }
	void cmptWarpedPixJacobian(MatrixXd &J, const PixGradT &g) override { jac(MTFHIP_JAC_WARPED, J, g); }
	void cmptApproxPixJacobian(MatrixXd &J, const PixGradT &g) override { jac(MTFHIP_JAC_APPROX, J, g); }
	void cmptInitPixHessian(MatrixXd &D, const PixHessT &h, const PixGradT &g) override { pixHess(MTFHIP_JAC_INIT, D, h, g); }
	void cmptPixHessian(MatrixXd &D, const PixHessT &h, const PixGradT &g) override { pixHess(MTFHIP_JAC_PIX, D, h, g); }
	void cmptWarpedPixHessian(MatrixXd &D, const PixHessT &h, const PixGradT &g) override { pixHess(MTFHIP_JAC_WARPED, D, h, g); }
	void cmptApproxPixHessian(MatrixXd &D, const PixHessT &h, const PixGradT &g) override { pixHess(MTFHIP_JAC_APPROX, D, h, g); }
	void applyWarpToCorners(CornersT &out, const CornersT &in, const VectorXd &state) override;
	/* 3 x 3 algebra on the host, no device work (ProjectiveBase.cc:51-55,142-160,321-331; Homography.cc:877-883; Affine.cc:352-357,382-393) */
	void additiveUpdate(const VectorXd &state_update) override;
	void applyWarpToPts(PtsT &out, const PtsT &in, const VectorXd &state) override;
	void getIdentityWarp(VectorXd &identity_warp) override;
	void composeWarps(VectorXd &composed, const VectorXd &state_1, const VectorXd &state_2) override;
	void estimateWarpFromCorners(VectorXd &state_update, const CornersT &in_corners, const CornersT &out_corners) override;
	/* the robust fit to point pairs (Homography.cc:885-897, Affine.cc:359-369) with the reference's signature, on the device
	 * (mtfhip_ssm_estimate_from_pts); every call draws its subsets from the next seed (setEstimatorSeed fixes the first) */
	void estimateWarpFromPts(VectorXd &state_update, std::vector<unsigned char> &mask, const std::vector<EstPt> &in_pts, const std::vector<EstPt> &out_pts,
		const SSMEstimatorParams &est_params);
	void setEstimatorSeed(unsigned long long seed) { est_seed = seed; }
	const EstimatorInfo &getEstimatorInfo() const { return est_info; }
	/* stochastic sampler (ProjectiveBase.cc:163-317, Homography.cc:899-942) on the host, one state per call as the interface
	 * has it -- what the literal nt::PF / nt::NN loops call.  The device filter (hip::PF, mtfhip_pf_*) generates all particles
	 * of an iteration in one launch instead.  The reference draws from boost::mt11213b seeded by random_device; here
	 * std::mt19937_64, seeded the same way unless setSamplerSeed() fixes it. */
	void initializeSampler(const VectorXd &state_sigma, const VectorXd &state_mean) override;
	void estimateStateSigma(VectorXd &state_sigma, double pix_sigma) override;   /* ProjectiveBase.cc:201-213 */
	void setSampler(const VectorXd &state_sigma, const VectorXd &state_mean) override;
	void setSamplerMean(const VectorXd &mean) override;
	void setSamplerSigma(const VectorXd &sigma) override;
	VectorXd getSamplerSigma() override { return sampler_sigma; }
	VectorXd getSamplerMean() override { return sampler_mean; }
	void compositionalRandomWalk(VectorXd &perturbed_state, const VectorXd &base_state) override;
	void additiveRandomWalk(VectorXd &perturbed_state, const VectorXd &base_state) override;
	void compositionalAutoRegression1(VectorXd &perturbed_state, VectorXd &perturbed_ar, const VectorXd &base_state,
		const VectorXd &base_ar, double a = 0.5) override;
	void additiveAutoRegression1(VectorXd &perturbed_state, VectorXd &perturbed_ar, const VectorXd &base_state,
		const VectorXd &base_ar, double a = 0.5) override;
	void generatePerturbation(VectorXd &perturbation) override;
	void estimateMeanOfSamples(VectorXd &sample_mean, const std::vector<VectorXd> &samples, int n_samples) override;
	void setSamplerSeed(unsigned long long seed);
	void markMoved() { d_pts = d_gpts = d_hpts = true; }   /* a device-side driver (hip::PF, mtfhip_batch_track) moved the SSM */
	void setCornerBasedSampling(bool on) { corner_based_sampling = on; }   /* HomographyParams::corner_based_sampling */
	bool getCornerBasedSampling() const { return corner_based_sampling; }
	void setPtBasedSampling(int mode) { pt_based_sampling = mode; }        /* AffineParams::pt_based_sampling (0 geometric, 1, 2) */
	int getPtBasedSampling() const { return pt_based_sampling; }
	const std::shared_ptr<HipPair> &pair() const { return p; }
private:
	std::shared_ptr<HipPair> p;
	bool d_pts = true, d_gpts = true, d_hpts = true;   /* host mirror older than the device array */
	template <typename T> const T &fresh(T &m, int buf, bool &dirty) {
		if (p->eager_getters && dirty) { HipPair::check(mtfhip_batch_read(p->b, buf, m.data())); dirty = false; }
		return m;
	}
	VectorXd sampler_sigma, sampler_mean;
	bool corner_based_sampling = true, sampler_ready = false;
	int pt_based_sampling = 0;
	unsigned long long est_seed = 1;
	EstimatorInfo est_info;
	[[noreturn]] void affineAdditiveRefused(const char *fn) const;
	struct Rng;
	std::shared_ptr<Rng> rng;
	double draw(int state_id);   /* one draw of N(mean[state_id], sigma[state_id]) */
	PtsT curr_pts;
	GradPtsT grad_pts;
	HessPtsT hess_pts;
	CornersT curr_corners;
	VectorXd curr_state;
	void syncSmall();
	void jac(int variant, MatrixXd &J, const PixGradT &g);
	void pixHess(int variant, MatrixXd &D, const PixHessT &h, const PixGradT &g);
	int gradBuffer(const PixGradT &g);
};

} // namespace hip
} // namespace mtf
#endif
