// What api.hip (the entry points) and the per-precision translation units share: the handle structs, the list of the typed bodies behind the
// entry points and the dispatch on a context's precision.  The build is split by explicit instantiation (lib.py builds the objects in parallel):
//   api.hip                 extern "C" entry points, argument checks, error plumbing -- instantiates NO kernel and nothing of Flow<T>, Bilinear<T>,
//                           PowerLens<T>, Projector<T>, Dataset<T>, EqDataset<T> or Drivers<T> (tests/test_boundary.py reads the object's symbols)
//   tu_main_{f32,f64}.hip   every body of CMBL_API_BODIES (api_body.hpp) and with them Ctx<T>, Flow<T> (engine.hpp), Bilinear<T>, PowerLens<T>, Dataset<T>
//                           (engine_dataset.hpp), Drivers<T> (drivers.hpp), their vtables and their kernels
//   tu_gen_{f32,f64}.hip    the host side of the any-size transform launches (engine_gen.hpp) and the run-time-plan kernels k_gen_dft*
//   tu_cty_{f32,f64}_{a,b}.hip   the compile-time-plan kernels of the column side and the plain transforms (engine_ct.hpp CtLaunchY: k_ct_dft,
//                           k_ct_dftx, k_ct_flow_y, k_ct_delta_y, k_ct_adj_y), lengths of CMBL_CT_LIST_A / _B (kernels_ct.hpp)
//   tu_ctx_{f32,f64}_{a,b}.hip   ... and of the row side of the fused stages (CtLaunchX: k_ct_adj_x, k_ct_adj_x_dx, k_ct_dft2)
//   tu_lensop_{f32,f64}.hip the fused column pass of a BilinearLens in a data set (engine_lensop.hpp: k_y_lens)
//   tu_small_{f32,f64}.hip  the one-launch flows of small maps (engine_small.hpp: k_small_flow, k_small_adj)
// An entry point reaches typed code in two ways only, and neither makes api.hip instantiate a member of a typed class (members defined in class
// are inline, and an explicit instantiation DECLARATION does not stop inline functions from being instantiated -- [temp.explicit]/10):
//   * a virtual member of the precision-free base its handle owns (CtxBase, FlowApi, DatasetApi, EqDatasetApi, BilinearApi, PowerLensApi, ProjectorApi): set_phi, apply, grad, ... and the
//     destructors.  The typed objects are made by the creators below, so their vtables are emitted in tu_main_* alone.
//   * BY_DTYPE(ctx, do_x, args...): a body of the list below, for what takes typed pointers or needs the typed object (which it gets back from
//     the handle with typed<Flow<T>>(L) etc., a static_cast).
#pragma once
#include "engine.hpp"
#include "engine_dataset.hpp"
#include "drivers.hpp"
#include "engine_ud.hpp"
#include "engine_cl.hpp"
#include "engine_bilinear.hpp"
#include "engine_powerlens.hpp"
#include "engine_mask.hpp"
#include "engine_equirect.hpp"
#include "engine_equirect_cov.hpp"
#include "engine_equirect_factor.hpp"
#include "engine_equirect_ds.hpp"
#include "engine_healpix.hpp"
#include "engine_nfft.hpp"
#include "../../include/cmblens.h"

struct cmbl_ctx { std::unique_ptr<cmbl::CtxBase> p; };
struct cmbl_clbins { std::unique_ptr<cmbl::ClBins> p; };
struct cmbl_flow { cmbl_ctx* ctx; std::unique_ptr<cmbl::FlowApi> p; };
struct cmbl_bilinear { cmbl_ctx* ctx; std::unique_ptr<cmbl::BilinearApi> p; };
struct cmbl_powerlens { cmbl_ctx* ctx; std::unique_ptr<cmbl::PowerLensApi> p; };
enum { LENSOP_FLOW = 0, LENSOP_BILINEAR = 1, LENSOP_POWERLENS = 2, LENSOP_IDENTITY = 3 };
// non-owning view: h is the cmbl_flow / cmbl_bilinear / cmbl_powerlens of `kind`.  LENSOP_IDENTITY has no handle behind it: h is the NoLens<T> that
// `own` keeps alive (made by do_lensop_identity, deleter and all)
struct cmbl_lensop { cmbl_ctx* ctx; int kind; void* h; std::shared_ptr<void> own; };
struct cmbl_projector { cmbl_ctx* ctx; std::unique_ptr<cmbl::ProjectorApi> p; };
struct cmbl_eqds { cmbl_ctx* ctx; std::unique_ptr<cmbl::EqDatasetApi> p; };
struct cmbl_dataset {
  cmbl_ctx* ctx; std::unique_ptr<cmbl::DatasetApi> p;
  std::map<const cmbl::FlowApi*, std::shared_ptr<void>> drv;                 // driver scratch (a Drivers<T>, deleter and all) per (dataset, flow) pair
  std::vector<std::unique_ptr<cmbl::DevBuf>> qe_pool;                        // legs and products of cmbl_quadratic_estimate, reused between calls
};

namespace cmbl {
// The typed bodies (api_body.hpp), one line each: their declarations and their explicit instantiations (tu_main_*) both come from this list.
#define CMBL_API_BODIES(X, T) \
  X(T, do_ctx_create, (cmbl_ctx* h, int Ny, int Nx, double theta, int device, void* stream)) \
  X(T, do_convert, (cmbl_ctx* ctx, int bi, const void* in, int bo, void* out, int P, int B)) \
  X(T, do_diag, (cmbl_ctx* ctx, int kind, int bd, const void* diag, int nplanes, bool transpose, int bi, const void* in, int bo, void* out, int P, int B)) \
  X(T, do_dot, (cmbl_ctx* ctx, int basis, const void* a, const void* b, int P, int B, double* out)) \
  X(T, do_diag_reduce, (cmbl_ctx* ctx, int which, int basis, const void* d, int P, int B, double* out)) \
  X(T, do_logdet, (cmbl_ctx* ctx, const void* d, int nplanes, double* out)) \
  X(T, do_axpby, (cmbl_ctx* ctx, const double* a, const void* x, const double* b, const void* y, void* out, long n, int B)) \
  X(T, do_qe_leg, (cmbl_ctx* ctx, const void* in_fourier, int n, int p1, int p2, void* out_map, int B)) \
  X(T, do_fourier_lmul, (cmbl_ctx* ctx, const void* in_map, int p1, int p2, int take_abs, void* out_fourier, int B)) \
  X(T, do_map_fma, (cmbl_ctx* ctx, const void* a, const void* b, double scale, void* out, int accumulate, long n)) \
  X(T, do_randn, (cmbl_ctx* ctx, const uint64_t* seeds, int nslots, uint64_t stream, void* out, long n_per_slot)) \
  X(T, do_flow_create, (cmbl_flow* h, int nsteps)) \
  X(T, do_dataset_create, (cmbl_dataset* h, int npol)) \
  X(T, do_bl_create, (cmbl_bilinear* h)) \
  X(T, do_pl_create, (cmbl_powerlens* h, int order, int kind)) \
  X(T, do_noise_inv, (cmbl_dataset* dsh, const void* in, void* out, int B)) \
  X(T, do_gradf_op, (cmbl_dataset* dsh, cmbl_lensop* Lh, const void* f, const void* d, int zero_d, void* out, int B)) \
  X(T, do_cg_op, (cmbl_dataset* dsh, cmbl_lensop* Lh, const void* d, const void* fstart, double tol, int maxit, void* f_out, double* hist, int* nit, int B)) \
  X(T, do_grad_lp_op, (cmbl_dataset* dsh, cmbl_lensop* Lh, const void* f, const void* phi, const void* d, double* lp, void* gf, void* gphi, int B, int quirk)) \
  X(T, do_lensop_identity, (cmbl_lensop* h)) \
  X(T, do_nolens_logpdf, (cmbl_dataset* dsh, const void* f, const void* d, double* lp, void* gf, int B)) \
  X(T, do_lpm, (cmbl_dataset* dsh, cmbl_flow* Lh, const void* fo, const void* phio, double* lp, void* gfo, void* gphio, int B, int quirk)) \
  X(T, do_theta_model, (cmbl_dataset* dsh, const ThetaModelArgs& a)) \
  X(T, do_lpm_theta, (cmbl_dataset* dsh, cmbl_flow* Lh, const void* fo, const void* phio, int B, int ntheta, const double* r, const double* aphi, const double* amps, int namps, double* lp)) \
  X(T, do_theta_ops, (cmbl_dataset* dsh, double r, double aphi, const double* amps, int namps, int which, void* out, double* sums)) \
  X(T, do_grad_theta, (cmbl_dataset* dsh, const void* f, const void* phi, int B, double r, double aphi, const double* amps, int namps, int want, double* grad)) \
  X(T, do_grad_theta_mixed, (cmbl_dataset* dsh, cmbl_flow* Lh, const void* fo, const void* phio, int B, double r, double aphi, const double* amps, int namps, int want, double* lp, double* grad)) \
  X(T, do_hmc,(cmbl_dataset* dsh, cmbl_flow* Lh, const void* fo, const void* phio, const void* mass, const void* white_p, const double* log_u, const uint64_t* seeds, uint64_t step, int nleap, double eps, int always, int quirk, int B, void* phio_out, double* dH, int* accept)) \
  X(T, do_map_step, (cmbl_dataset* dsh, cmbl_flow* Lh, const void* phi, const void* fstart, const void* hinv, double amax, double atol, double cg_tol, int cg_maxit, int quirk, int B, void* f_out, void* phi_out, double* logpdf, double* alpha, int* ncg, int* nls)) \
  X(T, do_qe, (cmbl_dataset* dsh, int which, const double* Cf, const double* Cft, const double* Cn, const double* TF, const double* Cphi, int wiener, const double* AL_in, void* phiqe_out, double* AL_out, int B)) \
  X(T, do_ud_grade, (cmbl_ctx* src, cmbl_ctx* dst, int mode, int deconv, int aa, int bi, const void* in, int bo, void* out, int P, int B)) \
  X(T, do_get_cl, (cmbl_ctx* ctx, cmbl_clbins* bins, int basis, const void* f1, const void* f2, int P, int B, const ClPairs& pr, int moments, double* out)) \
  X(T, do_edt_sq, (cmbl_ctx* ctx, const uint8_t* feat, int32_t* d2)) \
  X(T, do_make_mask, (cmbl_ctx* ctx, const MaskArgs& m, void* out)) \
  X(T, do_eq_convert, (cmbl_ctx* ctx, int bi, const void* in, int bo, void* out, int npol, int B)) \
  X(T, do_eq_apply, (cmbl_ctx* ctx, const void* blocks, bool cplx, int n, bool adjoint, const void* in, void* out, int B)) \
  X(T, do_eq_matmul, (cmbl_ctx* ctx, const void* A, bool adjA, const void* Bm, bool adjB, bool cplx, int n, void* out)) \
  X(T, do_eq_dot, (cmbl_ctx* ctx, const void* A, const void* Bm, bool cplx, int n, double* out)) \
  X(T, do_eq_scale_columns, (cmbl_ctx* ctx, void* blocks, bool cplx, int n, const double* w)) \
  X(T, do_eq_beam_pol, (cmbl_ctx* ctx, const void* blocksI, const double* omega, void* out)) \
  X(T, do_eq_cov, (cmbl_ctx* ctx, const double* tspan, const double* pspan, int pol, int lmax, const double* cl_a, const double* cl_b, int ngrid, void* blocks)) \
  X(T, do_eq_svd, (cmbl_ctx* ctx, const void* blocks, bool cplx, int n, double rtol, void* out_sqrt, void* out_pinv, double* sv, int* sweeps)) \
  X(T, do_eq_logabsdet, (cmbl_ctx* ctx, const void* blocks, bool cplx, int n, double* out)) \
  X(T, do_eq_solve, (cmbl_ctx* ctx, const void* A, bool acplx, int n, int side, const void* rhs, bool rcplx, int kind, void* out, int B)) \
  X(T, do_eqds_create, (cmbl_eqds* h, int npol)) \
  X(T, do_eq_field_dot, (cmbl_ctx* ctx, int basis, const void* a, const void* b, int npol, int B, double* out)) \
  X(T, do_projector_create, (cmbl_projector* h, int nside, int kind, const double* params, int method))

#define CMBL_API_DECLARE(T, name, params) template <typename T> void name params;
#define CMBL_API_INSTANTIATE(T, name, params) template void name<T> params;
CMBL_API_BODIES(CMBL_API_DECLARE, T)
#define CMBL_INSTANTIATE_API(T) CMBL_API_BODIES(CMBL_API_INSTANTIATE, T)
}  // namespace cmbl

// fn<T>(args...) with T the precision of a context (BY_DTYPE) or the one a dtype code names
#define BY_DTYPE_CODE(dtype, fn, ...) do { if ((dtype) == CMBL_F32) cmbl::fn<float>(__VA_ARGS__); else cmbl::fn<double>(__VA_ARGS__); } while (0)
#define BY_DTYPE(ctx, fn, ...) BY_DTYPE_CODE((ctx)->p->dtype, fn, __VA_ARGS__)
