// The typed bodies behind the C ABI (declared in api_decl.hpp); included by tu_main_{f32,f64}.hip only, which instantiate them.
#pragma once
#include "api_decl.hpp"

namespace cmbl {

// the typed object behind a handle: typed<Flow<T>>(L), typed<Dataset<T>>(ds) -- T is the precision of the handle's context (BY_DTYPE)
template <typename X, typename H> X& typed(H* h) { return *static_cast<X*>(h->p.get()); }
template <typename T> Ctx<T>* C(cmbl_ctx* c) { return &typed<Ctx<T>>(c); }

template <typename T> void do_convert(cmbl_ctx* ctx, int bi, const void* in, int bo, void* out, int P, int B) {
  Ctx<T>* c = C<T>(ctx);
  c->tmpA.ensure(sizeof(cx<T>) * (long)P * B * c->plane());              // (whatever the bases: the context's scratch exists after its first conversion)
  c->convert(bi, in, bo, out, P, B, c->tmpA);
}
template <typename T>
void do_diag(cmbl_ctx* ctx, int kind, int bd, const void* diag, int nplanes, bool transpose, int bi, const void* in, int bo, void* out, int P, int B) {
  Ctx<T>* c = C<T>(ctx);
  const long sl = (long)P * B;
  c->tmpA.ensure(sizeof(cx<T>) * sl * c->plane());
  c->tmpB.ensure(sizeof(T) * nplanes * c->plane());
  cx<T>* F = c->tmpA.template as<cx<T>>();
  T* dF = c->tmpB.template as<T>();
  c->ref2F_real((const T*)diag, dF, nplanes);
  const T* d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < nplanes; ++k) d[k] = dF + (size_t)k * c->plane();
  c->to_F(bi, in, F, bd, P, B);                       // B(f): convert to the operator's basis (src/specialops.jl:9)
  c->harm(F, F, P, B, kind, d, transpose, false, false);
  c->from_F(F, bd, bo, out, P, B);
}
template <typename T> void do_dot(cmbl_ctx* ctx, int basis, const void* a, const void* b, int P, int B, double* out) {
  Ctx<T>* c = C<T>(ctx);
  if (basis == B_MAP) { c->dot_map((const T*)a, (const T*)b, P, B, out); return; }
  // Fourier-type bases: the weighted sum is invariant under the internal permutation, but lam depends on ky, so
  // bring both operands to F layout (rotation QU<->EB is orthogonal entry by entry, any Fourier basis works as is)
  const long sl = (long)P * B;
  c->tmpA.ensure(sizeof(cx<T>) * 2 * sl * c->plane());
  cx<T>* Fa = c->tmpA.template as<cx<T>>(); cx<T>* Fb = Fa + sl * c->plane();
  c->ref2F((const cx<T>*)a, Fa, sl); c->ref2F((const cx<T>*)b, Fb, sl);
  c->dot_F(Fa, Fb, P, B, out);
}
// logdet / tr of Diagonal(field): which = 0 logdet, 1 tr
template <typename T> void do_diag_reduce(cmbl_ctx* ctx, int which, int basis, const void* d, int P, int B, double* out) {
  Ctx<T>* c = C<T>(ctx);
  if (basis == B_MAP) {
    if (which == 0) c->logdet_map((const T*)d, P, B, out); else c->tr_map((const T*)d, P, B, out);
    return;
  }
  const long sl = (long)P * B;
  c->tmpA.ensure(sizeof(cx<T>) * sl * c->plane());
  cx<T>* F = c->tmpA.template as<cx<T>>();
  c->ref2F((const cx<T>*)d, F, sl);                    // the lam-weighted sums are invariant under the internal permutation of x
  if (which == 0) c->logdet_Fc(F, P, B, out); else c->tr_Fc(F, P, B, out);
}
template <typename T> void do_logdet(cmbl_ctx* ctx, const void* d, int nplanes, double* out) {
  Ctx<T>* c = C<T>(ctx);
  c->tmpB.ensure(sizeof(T) * nplanes * c->plane());
  c->ref2F_real((const T*)d, c->tmpB.template as<T>(), nplanes);
  c->logdet_F(c->tmpB.template as<T>(), nplanes, out);
}
// the operator behind a view, as Dataset<T> sees it
template <typename T> LensOps<T>& lensop_of(cmbl_lensop* v) {
  if (v->kind == LENSOP_FLOW) return typed<Flow<T>>(static_cast<cmbl_flow*>(v->h));
  if (v->kind == LENSOP_BILINEAR) return typed<Bilinear<T>>(static_cast<cmbl_bilinear*>(v->h));
  if (v->kind == LENSOP_IDENTITY) return *static_cast<NoLens<T>*>(v->h);
  return typed<PowerLens<T>>(static_cast<cmbl_powerlens*>(v->h));
}
// the data of a call in the F layout: `d` (reference layout, converted into dF) or, d == NULL, what the data set holds
template <typename T> const cx<T>* data_of(Dataset<T>& ds, const void* d, cx<T>* dF, int B) {
  if (d) { ds.c->ref2F((const cx<T>*)d, dF, (long)ds.P * B); return dF; }
  CMBL_REQUIRE(ds.Bd == B, ERR_SHAPE, "dataset data batch size differs from nbatch");
  return ds.d_h.template as<cx<T>>();
}
// pinv(Cn) * z with whichever form of the noise operator the data set holds (reference layout in and out, in place allowed)
template <typename T>
void do_noise_inv(cmbl_dataset* dsh, const void* in, void* out, int B) {
  Dataset<T>& ds = typed<Dataset<T>>(dsh);
  Ctx<T>* c = ds.c;
  CMBL_REQUIRE(ds.has_noise(), ERR_STATE, "dataset_noise_inv: neither CMBL_OP_CN_INV nor CMBL_OP_CN_INV_PIX has been set");
  const long n = ds.fsize(B);
  ds.cvt.ensure(sizeof(cx<T>) * n);
  cx<T>* zF = ds.cvt.template as<cx<T>>();
  c->ref2F((const cx<T>*)in, zF, (long)ds.P * B);
  ds.apply_cn_inv(zF, zF, B);
  c->F2ref(zF, (cx<T>*)out, (long)ds.P * B);
}
// (cmbl_gradientf_logpdf and cmbl_wiener_cg come here too, with a view of their LenseFlow)
template <typename T>
void do_gradf_op(cmbl_dataset* dsh, cmbl_lensop* Lh, const void* f, const void* d, int zero_d, void* out, int B) {
  Dataset<T>& ds = typed<Dataset<T>>(dsh); LensOps<T>& L = lensop_of<T>(Lh);
  Ctx<T>* c = ds.c;
  L.op_check(B);
  const long n = ds.fsize(B);
  ds.cvt.ensure(sizeof(cx<T>) * 3 * n);
  cx<T>* fF = ds.cvt.template as<cx<T>>(); cx<T>* dF = fF + n; cx<T>* oF = dF + n;
  c->ref2F((const cx<T>*)f, fF, (long)ds.P * B);
  ds.gradientf(L, fF, zero_d ? nullptr : data_of(ds, d, dF, B), oF, B);
  c->F2ref(oF, (cx<T>*)out, (long)ds.P * B);
}
template <typename T>
void do_cg_op(cmbl_dataset* dsh, cmbl_lensop* Lh, const void* d, const void* fstart, double tol, int maxit, void* f_out, double* hist, int* nit, int B) {
  Dataset<T>& ds = typed<Dataset<T>>(dsh); LensOps<T>& L = lensop_of<T>(Lh);
  Ctx<T>* c = ds.c;
  L.op_check(B);
  const long n = ds.fsize(B);
  ds.cvt.ensure(sizeof(cx<T>) * 3 * n);
  cx<T>* dF = ds.cvt.template as<cx<T>>(); cx<T>* sF = dF + n; cx<T>* oF = sF + n;
  const cx<T>* dd = data_of(ds, d, dF, B);
  const cx<T>* fs = nullptr;
  if (fstart) { c->ref2F((const cx<T>*)fstart, sF, (long)ds.P * B); fs = sF; }
  *nit = ds.wiener_cg(L, dd, fs, tol, maxit, oF, hist, B);
  c->F2ref(oF, (cx<T>*)f_out, (long)ds.P * B);
  CMBL_HIP(hipStreamSynchronize(c->stream));
}
template <typename T>
void do_grad_lp_op(cmbl_dataset* dsh, cmbl_lensop* Lh, const void* f, const void* phi, const void* d, double* lp, void* gf, void* gphi, int B, int quirk) {
  Dataset<T>& ds = typed<Dataset<T>>(dsh); LensOps<T>& L = lensop_of<T>(Lh);
  Ctx<T>* c = ds.c;
  const long n = ds.fsize(B), pl = c->plane();
  // what the operator cannot give is refused before its phi is touched
  CMBL_REQUIRE(!gf || L.op_has_adjoint(), ERR_ARG, std::string(L.op_name()) + ": the gradient with respect to f needs L', which the reference does not define for this operator");
  CMBL_REQUIRE(!gphi || L.op_has_pullback(), ERR_ARG, std::string(L.op_name()) + ": the reference defines no pullback of L * f with respect to phi for this operator (gphi_out must be NULL)");
  L.op_set_phi(B_FOURIER, phi, 1);
  ds.cvt.ensure(sizeof(cx<T>) * (3 * n + (1 + B) * pl));
  cx<T>* fF = ds.cvt.template as<cx<T>>(); cx<T>* dF = fF + n; cx<T>* gF = dF + n; cx<T>* pF = gF + n; cx<T>* gpF = pF + pl;
  c->ref2F((const cx<T>*)f, fF, (long)ds.P * B);
  c->ref2F((const cx<T>*)phi, pF, 1);
  const cx<T>* dd = data_of(ds, d, dF, B);
  ds.grad_logpdf(L, fF, pF, dd, lp, gf ? gF : nullptr, gphi ? gpF : nullptr, B, quirk != 0);
  if (gf) c->F2ref(gF, (cx<T>*)gf, (long)ds.P * B);
  if (gphi) c->F2ref(gpF, (cx<T>*)gphi, B);
  CMBL_HIP(hipStreamSynchronize(c->stream));
}
// the identity for the L slot (cmbl_lensop_identity): the view owns its NoLens<T>
template <typename T> void do_lensop_identity(cmbl_lensop* h) {
  h->own = std::make_shared<NoLens<T>>(C<T>(h->ctx));
  h->h = h->own.get();
}
template <typename T>
void do_nolens_logpdf(cmbl_dataset* dsh, const void* f, const void* d, double* lp, void* gf, int B) {
  Dataset<T>& ds = typed<Dataset<T>>(dsh);
  Ctx<T>* c = ds.c;
  const long n = ds.fsize(B);
  ds.cvt.ensure(sizeof(cx<T>) * 3 * n);
  cx<T>* fF = ds.cvt.template as<cx<T>>(); cx<T>* dF = fF + n; cx<T>* gF = dF + n;
  c->ref2F((const cx<T>*)f, fF, (long)ds.P * B);
  ds.nolens_logpdf(fF, data_of(ds, d, dF, B), lp, gf ? gF : nullptr, B);
  if (gf) c->F2ref(gF, (cx<T>*)gf, (long)ds.P * B);
  CMBL_HIP(hipStreamSynchronize(c->stream));
}
template <typename T>
void do_lpm(cmbl_dataset* dsh, cmbl_flow* Lh, const void* fo, const void* phio, double* lp, void* gfo, void* gphio, int B, int quirk) {
  Dataset<T>& ds = typed<Dataset<T>>(dsh); Flow<T>& L = typed<Flow<T>>(Lh);
  Ctx<T>* c = ds.c;
  const long pl = c->plane();
  ds.cvt.ensure(sizeof(cx<T>) * 2 * B * pl);
  cx<T>* pF = ds.cvt.template as<cx<T>>(); cx<T>* gF = pF + (long)B * pl;
  c->ref2F((const cx<T>*)phio, pF, B);
  ds.logpdf_mixed(L, (const T*)fo, pF, lp, (T*)gfo, gfo ? gF : nullptr, B, quirk != 0);
  if (gfo) c->F2ref(gF, (cx<T>*)gphio, B);
  CMBL_HIP(hipStreamSynchronize(c->stream));
}
// the θ layer on the device (Dataset<T>::theta_*, kernels_theta.hpp)
template <typename T> void do_theta_model(cmbl_dataset* dsh, const ThetaModelArgs& a) {
  typed<Dataset<T>>(dsh).theta_install(a.cfs, a.nplanes, a.c0, a.nbands, a.band_planes, a.band_idx, a.band_nbins, a.cten, a.cn, a.s2len, a.r0, a.cphi0, a.aphi0,
                                       a.nphi, a.g, a.logdet_cn);
}
template <typename T>
void do_lpm_theta(cmbl_dataset* dsh, cmbl_flow* Lh, const void* fo, const void* phio, int B, int ntheta, const double* r, const double* aphi, const double* amps,
                  int namps, double* lp) {
  Dataset<T>& ds = typed<Dataset<T>>(dsh); Flow<T>& L = typed<Flow<T>>(Lh);
  Ctx<T>* c = ds.c;
  ds.cvt.ensure(sizeof(cx<T>) * 2 * B * c->plane());
  cx<T>* pF = ds.cvt.template as<cx<T>>();
  c->ref2F((const cx<T>*)phio, pF, B);
  ds.logpdf_mixed_theta(L, (const T*)fo, pF, B, ntheta, r, aphi, amps, namps, lp);
  CMBL_HIP(hipStreamSynchronize(c->stream));
}
template <typename T> void do_theta_ops(cmbl_dataset* dsh, double r, double aphi, const double* amps, int namps, int which, void* out, double* sums) {
  typed<Dataset<T>>(dsh).theta_readback(r, aphi, amps, namps, which, (T*)out, sums);
}
template <typename T>
void do_grad_theta(cmbl_dataset* dsh, const void* f, const void* phi, int B, double r, double aphi, const double* amps, int namps, int want, double* grad) {
  Dataset<T>& ds = typed<Dataset<T>>(dsh);
  Ctx<T>* c = ds.c;
  const long n = ds.fsize(B);
  ds.cvt.ensure(sizeof(cx<T>) * (n + B * c->plane()));
  cx<T>* fF = ds.cvt.template as<cx<T>>(); cx<T>* pF = fF + n;
  c->ref2F((const cx<T>*)f, fF, (long)ds.P * B);
  c->ref2F((const cx<T>*)phi, pF, B);
  ds.grad_theta_logpdf(fF, pF, B, r, aphi, amps, namps, want, grad);
}
template <typename T>
void do_grad_theta_mixed(cmbl_dataset* dsh, cmbl_flow* Lh, const void* fo, const void* phio, int B, double r, double aphi, const double* amps, int namps, int want,
                         double* lp, double* grad) {
  Dataset<T>& ds = typed<Dataset<T>>(dsh); Flow<T>& L = typed<Flow<T>>(Lh);
  Ctx<T>* c = ds.c;
  const long pl = c->plane();
  ds.cvt.ensure(sizeof(cx<T>) * 2 * B * pl);
  cx<T>* pF = ds.cvt.template as<cx<T>>(); cx<T>* gF = pF + (long)B * pl;
  c->ref2F((const cx<T>*)phio, pF, B);
  ds.grad_theta_logpdf_mixed(L, (const T*)fo, pF, gF, B, r, aphi, amps, namps, want, lp, grad);
}

template <typename T> Drivers<T>& drivers_of(cmbl_dataset* dsh, cmbl_flow* Lh) {
  auto& p = dsh->drv[Lh->p.get()];
  if (!p) p = std::make_shared<Drivers<T>>(typed<Dataset<T>>(dsh), typed<Flow<T>>(Lh));
  return *static_cast<Drivers<T>*>(p.get());
}
template <typename T>
void do_hmc(cmbl_dataset* dsh, cmbl_flow* Lh, const void* fo, const void* phio, const void* mass, const void* white_p, const double* log_u, const uint64_t* seeds,
                   uint64_t step, int nleap, double eps, int always, int quirk, int B, void* phio_out, double* dH, int* accept) {
  Drivers<T>& dr = drivers_of<T>(dsh, Lh);
  Dataset<T>& ds = dr.ds;
  Ctx<T>* c = ds.c;
  const long pl = c->plane(), np = c->npix();
  ds.cvt.ensure(sizeof(cx<T>) * 2 * B * pl + sizeof(T) * (pl + (long)B * np));
  cx<T>* pF = ds.cvt.template as<cx<T>>(); cx<T>* oF = pF + (long)B * pl;
  T* mF = reinterpret_cast<T*>(oF + (long)B * pl); T* w = mF + pl;
  c->ref2F((const cx<T>*)phio, pF, B);
  c->ref2F_real((const T*)mass, mF, 1);
  const T* wp = (const T*)white_p;
  if (!wp) {                                                             // randn!(rng, ...) with the drivers' stream convention (rng.py)
    CMBL_REQUIRE(seeds != nullptr, ERR_ARG, "white_p == NULL needs seeds_host");
    c->randn(w, seeds, B, stream_id(STREAM_P, step), np);
    wp = w;
  }
  std::vector<double> lu(B);
  for (int b = 0; b < B; ++b) {
    if (log_u) lu[b] = log_u[b];
    else { CMBL_REQUIRE(seeds != nullptr, ERR_ARG, "log_u_host == NULL needs seeds_host"); lu[b] = std::log(philox_uniform(seeds[b], stream_id(STREAM_U, step))); }
  }
  dr.hmc_step((const T*)fo, pF, mF, wp, lu.data(), nleap, eps, always != 0, quirk != 0, B, oF, dH, accept);
  c->F2ref(oF, (cx<T>*)phio_out, B);
  CMBL_HIP(hipStreamSynchronize(c->stream));
}
template <typename T>
void do_map_step(cmbl_dataset* dsh, cmbl_flow* Lh, const void* phi, const void* fstart, const void* hinv, double amax, double atol, double cg_tol, int cg_maxit, int quirk,
                        int B, void* f_out, void* phi_out, double* logpdf, double* alpha, int* ncg, int* nls) {
  Drivers<T>& dr = drivers_of<T>(dsh, Lh);
  Dataset<T>& ds = dr.ds;
  Ctx<T>* c = ds.c;
  const long pl = c->plane(), n = ds.fsize(B);
  CMBL_REQUIRE(ds.Bd == B, ERR_SHAPE, "dataset data batch size differs from nbatch");
  ds.cvt.ensure(sizeof(cx<T>) * (2 * B * pl + 2 * n) + sizeof(T) * 2 * pl);
  cx<T>* pF = ds.cvt.template as<cx<T>>(); cx<T>* oF = pF + (long)B * pl; cx<T>* sF = oF + (long)B * pl; cx<T>* fF = sF + n;
  T* hF = reinterpret_cast<T*>(fF + n); T* ones = hF + pl;
  c->ref2F((const cx<T>*)phi, pF, B);
  c->ref2F_real((const T*)hinv, hF, 1);
  const cx<T>* fs = nullptr;
  if (fstart) { c->ref2F((const cx<T>*)fstart, sF, (long)ds.P * B); fs = sF; }
  // G = I for the duration of the step (src/maximization.jl:146), whatever G the dataset carries
  std::vector<T> h1(pl, T(1));
  CMBL_HIP(hipMemcpyAsync(ones, h1.data(), sizeof(T) * pl, hipMemcpyHostToDevice, c->stream));
  CMBL_HIP(hipStreamSynchronize(c->stream));
  // (a dataset that never set G works as well: the slot is a one-plane diagonal for the duration of the call and is put back as it was)
  auto& g = ds.ops[OP_G_INV];
  struct Swap { decltype(g)& o; const T* d0; int np, kind; ~Swap() { o.d[0] = d0; o.nplanes = np; o.kind = kind; } } sw{g, g.d[0], g.nplanes, g.kind};
  if (g.nplanes == 0) { g.nplanes = 1; g.kind = 1; }
  g.d[0] = ones;
  std::vector<double> hist((size_t)cg_maxit * B);
  dr.map_joint_step(pF, fs, hF, amax, atol, cg_tol, cg_maxit, quirk != 0, B, fF, oF, logpdf, alpha, ncg, nls, hist.data());
  c->F2ref(fF, (cx<T>*)f_out, (long)ds.P * B);
  c->F2ref(oF, (cx<T>*)phi_out, B);
  CMBL_HIP(hipStreamSynchronize(c->stream));
}

template <typename T>
void do_qe(cmbl_dataset* dsh, int which, const double* Cf, const double* Cft, const double* Cn, const double* TF, const double* Cphi, int wiener,
                  const double* AL_in, void* phiqe_out, double* AL_out, int B) {
  Dataset<T>& ds = typed<Dataset<T>>(dsh); auto& pool = dsh->qe_pool;
  Ctx<T>* c = ds.c;
  const long pl = c->plane();
  CMBL_REQUIRE(ds.Bd == B, ERR_SHAPE, "dataset data batch size differs from nbatch");
  // data components the estimator uses: TT -> T; EE -> E; EB -> E, B  (component index inside the dataset's I / EB / IEB data)
  const int P = ds.P;
  int comp[2] = {0, 0};
  if (which == 0) { CMBL_REQUIRE(P == 1 || P == 3, ERR_ARG, "TT needs a dataset with temperature"); comp[0] = 0; }
  else { CMBL_REQUIRE(P >= 2, ERR_ARG, "EE / EB need a dataset with polarisation"); comp[0] = P - 2; comp[1] = P - 1; }
  const int ncomp = which == 2 ? 2 : 1;
  ds.cvt.ensure(sizeof(cx<T>) * (long)ncomp * B * pl);
  cx<T>* dr[2] = {ds.cvt.template as<cx<T>>(), ds.cvt.template as<cx<T>>() + (long)B * pl};
  for (int k = 0; k < ncomp; ++k)
    for (int b = 0; b < B; ++b) c->F2ref(ds.d_h.template as<cx<T>>() + ((long)b * P + comp[k]) * pl, dr[k] + (long)b * pl, 1);
  const cx<T>* drc[2] = {dr[0], dr[1]};
  quadratic_estimate<T>(c, pool, which, B, drc, Cf, Cft, Cn, TF, Cphi, wiener != 0, AL_in, (cx<T>*)phiqe_out, AL_out);
  // the legs and products stay allocated for the next call (a one-off estimator otherwise spends half its time in hipMalloc), unless
  // they are large relative to the device: ~100 maps, 3 GB at 2048^2 in double precision
  size_t held = 0, free_b = 0, total_b = 0;
  for (const auto& b : pool) held += b->bytes;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); total_b = (size_t)16 << 30; }
  if (held > total_b / 16) pool.clear();                                 // 18 GB on a 288 GB part (round 4 dropped the pool above 1 GB: re-allocated on every call at 2048^2)
}


// ---- the creators, and the members that take typed pointers (api.hip must not instantiate a launching member: see api_decl.hpp) ----------
template <typename T> void do_ctx_create(cmbl_ctx* h, int Ny, int Nx, double theta, int device, void* stream) { h->p = std::make_unique<Ctx<T>>(Ny, Nx, theta, device, stream); }
template <typename T> void do_flow_create(cmbl_flow* h, int nsteps) { h->p = std::make_unique<Flow<T>>(C<T>(h->ctx), nsteps); }
template <typename T> void do_dataset_create(cmbl_dataset* h, int npol) { h->p = std::make_unique<Dataset<T>>(C<T>(h->ctx), npol); }
template <typename T> void do_bl_create(cmbl_bilinear* h) { h->p = std::make_unique<Bilinear<T>>(C<T>(h->ctx)); }
template <typename T> void do_pl_create(cmbl_powerlens* h, int order, int kind) { h->p = std::make_unique<PowerLens<T>>(C<T>(h->ctx), order, kind); }
template <typename T> void do_projector_create(cmbl_projector* h, int nside, int kind, const double* params, int method) {
  if (method == PROJECT_NFFT) h->p = std::make_unique<NfftProjector<T>>(C<T>(h->ctx), nside, kind, params);
  else h->p = std::make_unique<Projector<T>>(C<T>(h->ctx), nside, kind, params);
}
template <typename T> void do_axpby(cmbl_ctx* ctx, const double* a, const void* x, const double* b, const void* y, void* out, long n, int B) {
  C<T>(ctx)->lincomb((T*)out, (const T*)x, (const T*)y, a, b, n, B);
}
template <typename T> void do_qe_leg(cmbl_ctx* ctx, const void* in_fourier, int n, int p1, int p2, void* out_map, int B) {
  C<T>(ctx)->qe_leg((const cx<T>*)in_fourier, (T*)out_map, n, p1, p2, B);
}
template <typename T> void do_fourier_lmul(cmbl_ctx* ctx, const void* in_map, int p1, int p2, int take_abs, void* out_fourier, int B) {
  C<T>(ctx)->fourier_lmul((const T*)in_map, (cx<T>*)out_fourier, p1, p2, take_abs != 0, B);
}
template <typename T> void do_map_fma(cmbl_ctx* ctx, const void* a, const void* b, double scale, void* out, int accumulate, long n) {
  C<T>(ctx)->map_fma((T*)out, (const T*)a, (const T*)b, scale, accumulate != 0, n);
}
template <typename T> void do_randn(cmbl_ctx* ctx, const uint64_t* seeds, int nslots, uint64_t stream, void* out, long n_per_slot) {
  C<T>(ctx)->randn((T*)out, seeds, nslots, stream, n_per_slot);
}
template <typename T> void do_ud_grade(cmbl_ctx* src, cmbl_ctx* dst, int mode, int deconv, int aa, int bi, const void* in, int bo, void* out, int P, int B) {
  ud_grade<T>(C<T>(src), C<T>(dst), mode, deconv != 0, aa != 0, bi, in, bo, out, P, B);
}
template <typename T> void do_get_cl(cmbl_ctx* ctx, cmbl_clbins* bins, int basis, const void* f1, const void* f2, int P, int B, const ClPairs& pr, int moments, double* out) {
  get_cl<T>(C<T>(ctx), *bins->p, basis, f1, f2, P, B, pr, moments, out);
}
template <typename T> void do_edt_sq(cmbl_ctx* ctx, const uint8_t* feat, int32_t* d2) { edt_sq_checked<T>(C<T>(ctx), feat, d2); }
template <typename T> void do_make_mask(cmbl_ctx* ctx, const MaskArgs& m, void* out) { make_mask<T>(C<T>(ctx), m, (T*)out); }
template <typename T> void do_eq_convert(cmbl_ctx* ctx, int bi, const void* in, int bo, void* out, int npol, int B) { equirect_convert<T>(C<T>(ctx), bi, in, bo, out, npol, B); }
template <typename T> void do_eq_apply(cmbl_ctx* ctx, const void* blocks, bool cplx, int n, bool adjoint, const void* in, void* out, int B) { equirect_block_apply<T>(C<T>(ctx), blocks, cplx, n, adjoint, in, out, B); }
template <typename T> void do_eq_matmul(cmbl_ctx* ctx, const void* A, bool adjA, const void* Bm, bool adjB, bool cplx, int n, void* out) { equirect_block_matmul<T>(C<T>(ctx), A, adjA, Bm, adjB, cplx, n, out); }
template <typename T> void do_eq_dot(cmbl_ctx* ctx, const void* A, const void* Bm, bool cplx, int n, double* out) { equirect_block_dot<T>(C<T>(ctx), A, Bm, cplx, n, out); }
template <typename T> void do_eq_scale_columns(cmbl_ctx* ctx, void* blocks, bool cplx, int n, const double* w) { equirect_scale_columns<T>(C<T>(ctx), blocks, cplx, n, w); }
template <typename T> void do_eq_beam_pol(cmbl_ctx* ctx, const void* blocksI, const double* omega, void* out) { equirect_beam_pol<T>(C<T>(ctx), blocksI, omega, out); }
template <typename T> void do_eq_svd(cmbl_ctx* ctx, const void* blocks, bool cplx, int n, double rtol, void* out_sqrt, void* out_pinv, double* sv, int* sweeps) { equirect_block_svd<T>(C<T>(ctx), blocks, cplx, n, rtol, out_sqrt, out_pinv, sv, sweeps); }
template <typename T> void do_eq_logabsdet(cmbl_ctx* ctx, const void* blocks, bool cplx, int n, double* out) { equirect_block_logabsdet<T>(C<T>(ctx), blocks, cplx, n, out); }
template <typename T> void do_eq_solve(cmbl_ctx* ctx, const void* A, bool acplx, int n, int side, const void* rhs, bool rcplx, int kind, void* out, int B) { equirect_block_solve<T>(C<T>(ctx), A, acplx, n, side, rhs, rcplx, kind, out, B); }
template <typename T> void do_eq_cov(cmbl_ctx* ctx, const double* tspan, const double* pspan, int pol, int lmax, const double* cl_a, const double* cl_b, int ngrid, void* blocks) { equirect_cov<T>(C<T>(ctx), tspan, pspan, pol, lmax, cl_a, cl_b, ngrid, blocks); }
template <typename T> void do_eqds_create(cmbl_eqds* h, int npol) { h->p = std::make_unique<EqDataset<T>>(C<T>(h->ctx), npol); }
template <typename T> void do_eq_field_dot(cmbl_ctx* ctx, int basis, const void* a, const void* b, int npol, int B, double* out) { equirect_field_dot<T>(C<T>(ctx), basis, a, b, npol, B, out); }

}  // namespace cmbl
