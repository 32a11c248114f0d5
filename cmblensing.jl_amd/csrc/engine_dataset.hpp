// The data model on top of Ctx<T> and a lensing operator (LensOps<T>): Dataset<T> with its operators, the Wiener filter and the posterior
// with its gradients.  Included by api_decl.hpp and drivers.hpp.
#pragma once
#include "engine.hpp"
#include "engine_cg.hpp"
#include "engine_nolens.hpp"
#include "kernels_theta.hpp"

namespace cmbl {

// =================================================================================================
// Data model, Wiener filter, posterior   (src/dataset.jl, src/maximization.jl, src/numerical_algorithms.jl)
enum OpId { OP_CF_INV = 0, OP_CN_INV, OP_B, OP_MF, OP_D, OP_D_INV, OP_PRECOND_INV, OP_CPHI_INV, OP_G_INV, OP_MPIX, OP_CN_INV_PIX, OP_COUNT };

struct DatasetApi {                        // what the C ABI (api.hip) holds of a dataset (see FlowApi)
  double logdet_sum = 0;
  virtual ~DatasetApi() = default;
  virtual void set_op(int which, const void* planes, int nplanes) = 0;
  virtual void set_data(const void* d_ref, int B) = 0;
};

template <typename T>
struct Dataset : DatasetApi {
  Ctx<T>* c;
  int P;
  struct Op { DevBuf buf; int nplanes = 0; const T* d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; int kind = 0; };
  Op ops[OP_COUNT];
  DevBuf d_h; int Bd = 0;                  // data, F layout harmonic
  // scratch
  DevBuf t1, t2, t3, mp, mp2, phiF, gphi, dphi1, dphi2, fh, fhat, ftil, cvt;

  Dataset(Ctx<T>* ctx, int npol) : c(ctx), P(npol), cg(ctx) { CMBL_REQUIRE(npol >= 1 && npol <= 3, ERR_ARG, "npol must be 1, 2 or 3"); }

  void set_op(int which, const void* planes, int nplanes) override {
    CMBL_REQUIRE(which >= 0 && which < OP_COUNT, ERR_ARG, "bad operator id");
    Op& o = ops[which];
    if (which == OP_MPIX) {
      CMBL_REQUIRE(nplanes == 1, ERR_ARG, "pixel mask is one map");
      o.buf.ensure(sizeof(T) * c->npix());
      CMBL_HIP(hipMemcpyAsync(o.buf.p, planes, sizeof(T) * c->npix(), hipMemcpyDeviceToDevice, c->stream));
      o.nplanes = 1; o.d[0] = o.buf.template as<T>(); o.kind = 1;
      return;
    }
    if (which == OP_CN_INV_PIX) {            // pinv of the variance maps of Cn = Diagonal(V): one plane for all pol slices or one each; 0 planes clears it
      CMBL_REQUIRE(nplanes == 0 || nplanes == 1 || nplanes == P, ERR_SHAPE, "the map-diagonal noise operator takes 1 or npol planes (0 clears it)");
      CMBL_REQUIRE(nplanes == 0 || planes != nullptr, ERR_ARG, "planes is NULL");
      o.nplanes = nplanes; o.kind = 1; o.d[0] = nullptr;
      if (nplanes == 0) return;
      o.buf.ensure(sizeof(T) * nplanes * c->npix());
      CMBL_HIP(hipMemcpyAsync(o.buf.p, planes, sizeof(T) * nplanes * c->npix(), hipMemcpyDeviceToDevice, c->stream));
      o.d[0] = o.buf.template as<T>();
      return;
    }
    const bool s0 = (which == OP_CPHI_INV || which == OP_G_INV);
    CMBL_REQUIRE(s0 ? nplanes == 1 : (nplanes == P || (P == 3 && nplanes == 5)), ERR_SHAPE, "wrong number of planes for this operator");
    o.buf.ensure(sizeof(T) * nplanes * c->plane());
    c->ref2F_real((const T*)planes, o.buf.template as<T>(), nplanes);
    o.nplanes = nplanes; o.kind = (nplanes == 5) ? 2 : 1;
    for (int k = 0; k < 5; ++k) o.d[k] = k < nplanes ? o.buf.template as<T>() + (size_t)k * c->plane() : nullptr;
  }
  const Op& op(int which) const {
    CMBL_REQUIRE(ops[which].nplanes > 0, ERR_STATE, "a required dataset operator has not been set");
    return ops[which];
  }
  bool has(int which) const { return ops[which].nplanes > 0; }
  void apply(int which, const cx<T>* in, cx<T>* out, int B, bool transpose = false, bool in_qu = false, bool out_qu = false,
             const cx<T>* z = nullptr, T alpha = 0, T beta = 1, int Pp = -1) {
    const Op& o = op(which);
    c->harm(in, out, Pp < 0 ? P : Pp, B, o.kind, o.d, transpose, in_qu, out_qu, z, alpha, beta);
  }
  void set_data(const void* d_ref, int B) override {
    d_h.ensure(sizeof(cx<T>) * (long)P * B * c->plane());
    c->ref2F((const cx<T>*)d_ref, d_h.template as<cx<T>>(), (long)P * B);
    Bd = B;
  }
  long fsize(int B) const { return (long)P * B * c->plane(); }

  // x (QU Fourier, F layout) <- rfft2(mask .* irfft2(x)): x pass, column kernel (c2r, mask, r2c in LDS), x pass
  void pixel_mask(cx<T>* x, long sl) {
    if (c->generic) {
      mp.ensure(sizeof(T) * sl * c->npix());
      c->F_to_map(x, mp.template as<T>(), sl); c->mask_mul(mp.template as<T>(), mp.template as<T>(), ops[OP_MPIX].d[0], sl); c->rfft2_F(mp.template as<T>(), x, sl);
      return;
    }
    cx<T>* m = c->mixed_scratch(sl);
    c->template x_pass<1>(x, m, sl); c->y_mask(m, m, ops[OP_MPIX].d[0], sl); c->template x_pass<0>(m, x, sl);
  }
  // out = beta * pinv(Cn) in, harmonic F in and out (in place allowed), with whichever form of the noise operator is set.  Fourier form
  // (OP_CN_INV): one launch.  Map-diagonal form (OP_CN_INV_PIX; Cn = Diagonal(V) in the I/QU map basis, src/dataset.jl:37-47): the sandwich
  // rfft2(w .* irfft2(.)) between the two basis changes.  Power-of-two maps: three launches -- EB -> QU with ifft_x (row carrier), the column
  // kernel (c2r, weight, r2c in LDS), fft_x with QU -> EB (row carrier).  Any size: five (basis change, irfft2, weight, rfft2, basis change).
  void apply_cn_inv(const cx<T>* in, cx<T>* out, int B, T beta = 1) {
    if (!has(OP_CN_INV_PIX)) { apply(OP_CN_INV, in, out, B, false, false, false, nullptr, 0, beta); return; }
    const Op& o = ops[OP_CN_INV_PIX];
    const long sl = (long)P * B;
    if (c->generic) {
      mp.ensure(sizeof(T) * sl * c->npix());
      c->harm(in, out, P, B, 0, nullptr, false, false, true);
      c->F_to_map(out, mp.template as<T>(), sl); c->weight_mul(mp.template as<T>(), mp.template as<T>(), o.d[0], o.nplanes, P, beta, sl); c->rfft2_F(mp.template as<T>(), out, sl);
      c->harm(out, out, P, B, 0, nullptr, false, true, false);
      return;
    }
    cx<T>* m = c->mixed_scratch(sl);
    by_pol([&](auto pp) {
      constexpr int PP = decltype(pp)::value;
      PwChain<T, PP> to_qu{c->geom(), {}, 0, 1, nullptr, T(0), nullptr, T(1)};
      c->template x_pw<PP, true>(in, m, to_qu, B);                                      // EB -> QU, ifft_x
      c->y_weight(m, m, o.d[0], o.nplanes, P, beta, sl);                                // x pinv(V) on the map
      PwChain<T, PP> to_eb{c->geom(), {}, 1, 0, nullptr, T(0), out, T(1)};
      c->template x_pw<PP, false>(m, nullptr, to_eb, B);                                // fft_x, QU -> EB, stored
    });
  }
  bool has_noise() const { return has(OP_CN_INV_PIX) || has(OP_CN_INV); }

  // x (harmonic F) -> M x = Mf * (Mpix * x) ; transpose: Mpix' * (Mf' * x)   (src/dataset.jl:279-285)
  // qu: the pixel side of M is exchanged in QU Fourier (x comes in QU Fourier for M, goes out in QU Fourier for M'), so that the beam
  // next to it does the basis change in its own launch instead of a launch of its own
  void apply_M(cx<T>* x, int B, bool transpose, bool qu = false) {
    const long sl = (long)P * B;
    if (!has(OP_MPIX)) { apply(OP_MF, x, x, B, transpose, qu && !transpose, qu && transpose); return; }
    if (!transpose) {
      if (!qu) c->harm(x, x, P, B, 0, nullptr, false, false, true);        // -> QU Fourier
      pixel_mask(x, sl);
      apply(OP_MF, x, x, B, false, true, false);
    } else {
      apply(OP_MF, x, x, B, true, false, true);
      pixel_mask(x, sl);
      if (!qu) c->harm(x, x, P, B, 0, nullptr, false, true, false);
    }
  }

  // ---- fused path (kernels_harm.hpp; power-of-two maps) ----------------------------------------------------------------------------
  bool fused() const { return !c->generic && c->opts.fused_harm && !has(OP_CN_INV_PIX); }
  OpRef<T> opref(int which, bool transpose = false) const {
    const Op& o = op(which);
    OpRef<T> r{};
    for (int k = 0; k < 5; ++k) r.d[k] = o.d[k];
    r.kind = o.kind; r.transpose = transpose ? 1 : 0;
    return r;
  }
  template <typename Fn> void by_pol(Fn&& fn) const { cmbl::by_pol(P, fn); }
  DevBuf m1;                                 // mixed-layout scratch of the data-space part
  // The harmonic chains of the model on either side of Cn^-1:  pre = [B,] Mf  and  post = Mf' [, B']
  void model_chains(HarmChain<T>& pre, HarmChain<T>& post, bool beam) const {
    if (beam) pre.push(opref(OP_B));
    pre.push(opref(OP_MF)); post.push(opref(OP_MF, true));
    if (beam) post.push(opref(OP_B, true));
  }
  // The middle of a pass through data space with a pixel mask, in place on `m` (mixed layout, QU, the beam applied): pixel mask; one row pass with
  // the Fourier mask, scale * (. - d), Cn^-1, the quadratic form and the Fourier mask'; pixel mask'.  store == false: the value alone, the pass
  // ends with the quadratic form and m keeps the masked input.  Returns where the partials of the quadratic form were left (PART_QN).
  template <int PP> DotOut masked_core(cx<T>* m, const cx<T>* dd, int dB, T scale, bool store, int B) {
    c->y_mask(m, m, ops[OP_MPIX].d[0], (long)P * B);                                    // pixel mask
    PwResid<T, PP> rs{c->geom(), {}, {}, opref(OP_CN_INV), dd, dB, scale, nullptr};
    model_chains(rs.pre, rs.post, false);
    const DotOut qn = c->template x_pw<PP, false>(m, store ? m : nullptr, rs, B, false, Ctx<T>::PART_QN);
    if (store) c->y_mask(m, m, ops[OP_MPIX].d[0], (long)P * B);                         // pixel mask'
    return qn;
  }
  // From rfft_y(L f) in `a_ftil` (mixed, left intact) to  w = scale * B'M' Cn^-1 (M B L f - d):  w in QU Fourier to `w_F` (F layout) and
  // ifft_x(w) to L.H (mixed), ready for an adjoint / delta flow with h_ready.  Returns where the
  // partial sums of (MBLf - d)' Cn^-1 (MBLf - d) were left.  value_only: stop after the quadratic form.  dd == nullptr: d = 0.   (src/dataset.jl:59-66,76-80)
  // H: the mixed-layout buffer ifft_x(w) goes to (the flow's hbuf_ensure; unused when value_only)
  DotOut data_space(cx<T>* H, const cx<T>* a_ftil, const cx<T>* dd, int dB, T scale, cx<T>* w_F, bool value_only, int B) {
    const long sl = (long)P * B;
    DotOut qn{};
    by_pol([&](auto pp) {
      constexpr int PP = decltype(pp)::value;
      const ModeGeom<T> g = c->geom();
      if (has(OP_MPIX)) {
        m1.ensure(sizeof(cx<T>) * sl * c->mplane());
        cx<T>* m = m1.template as<cx<T>>();
        PwChain<T, PP> b1{g, {}, 1, 1, nullptr, T(0), nullptr, T(1)};
        b1.ch.push(opref(OP_B));
        c->template x_pw<PP, false>(a_ftil, m, b1, B);                                  // beam
        qn = masked_core<PP>(m, dd, dB, T(1), !value_only, B);                          // mask, Fourier mask / residual / Cn^-1 / quadratic form / Fourier mask', mask'
        if (value_only) return;
        PwChain<T, PP> b2{g, {}, 1, 1, nullptr, T(0), w_F, scale};
        b2.ch.push(opref(OP_B, true));
        c->template x_pw<PP, false>(m, H, b2, B);                                       // beam', w stored, ifft_x(w) -> H
      } else {
        PwResid<T, PP> rs{g, {}, {}, opref(OP_CN_INV), dd, dB, scale, value_only ? nullptr : w_F};
        model_chains(rs.pre, rs.post, true);
        qn = c->template x_pw<PP, false>(a_ftil, H, rs, B, false, Ctx<T>::PART_QN);
      }
    });
    return qn;
  }
  // f (harmonic F) -> L f: leaves the lensed maps in `ftil` and rfft_y(L f) in L.A
  void lens_from_harmonic(Flow<T>& L, const cx<T>* f_h, T* ftil, int B) {
    const long sl = (long)P * B;
    mp2.ensure(sizeof(T) * sl * c->npix());
    cx<T>* a = L.abuf_ensure(L.A, sl);
    by_pol([&](auto pp) {
      constexpr int PP = decltype(pp)::value;
      PwChain<T, PP> r{c->geom(), {}, 0, 1, nullptr, T(0), nullptr, T(1)};
      c->template x_pw<PP, true>(f_h, a, r, B, true);                                   // EB -> QU, ifft_x, Hermitian rows projected
    });
    c->y_c2r(a, mp2.template as<T>(), sl);
    L.flow_map(mp2.template as<T>(), ftil, P, B, false, true, true, &L.A);
  }
  // Y = L'B'M'Cn^-1 (d - M B L f)   (QU Fourier, F layout; the data part of gradientf_logpdf)
  void model_adjoint(Flow<T>& L, const cx<T>* f_h, const cx<T>* dd, int dB, cx<T>* Y, int B) {
    const long sl = (long)P * B;
    ftil.ensure(sizeof(T) * sl * c->npix());
    lens_from_harmonic(L, f_h, ftil.template as<T>(), B);
    data_space(L.hbuf_ensure(sl), L.A.template as<cx<T>>(), dd, dB, T(-1), Y, false, B);
    L.flow_adj_F(Y, Y, P, B, false, true);
  }

  // mu = M B L f : harmonic F in (f may be nullptr == 0) -> harmonic F out (t2); uses mp2 for maps
  // `ftil_out`: where the lensed maps f~ = L f are left (default: the scratch mp2)
  void mean(LensOps<T>& L, const cx<T>* f_h, cx<T>* out, int B, T* ftil_out = nullptr) {
    const long sl = (long)P * B;
    mp2.ensure(sizeof(T) * sl * c->npix());
    c->harm(f_h, out, P, B, 0, nullptr, false, false, true);
    c->F_to_map(out, mp2.template as<T>(), sl);
    L.op_lens_F(mp2.template as<T>(), ftil_out, out, P, B);
    apply(OP_B, out, out, B, false, true, true);                          // QU Fourier -> (EB) x beam -> QU Fourier
    apply_M(out, B, false, true);
  }

  // gradientf_logpdf (src/dataset.jl:76-80): L'B'M'Cn^-1 (d - M B L f) - Cf^-1 f.  f_h == nullptr means f = 0;
  // d_h == nullptr means d = 0.  All harmonic F layout.  out must not alias f_h.  A LenseFlow on a power-of-two map runs the fused form;
  // any other operator with an adjoint (and f = 0) the composition around op_lens_F / op_adj_F
  void gradientf(LensOps<T>& L, const cx<T>* f_h, const cx<T>* dd, cx<T>* out, int B) {
    CMBL_REQUIRE(L.op_has_adjoint(), ERR_ARG, std::string(L.op_name()) + ": gradientf_logpdf / the Wiener filter need L', which the reference does not define for this operator");
    const long n = fsize(B);
    t2.ensure(sizeof(cx<T>) * n);
    cx<T>* r = t2.template as<cx<T>>();
    const Form fm = form(L);
    if (f_h && fm == FORM_IDENTITY) { nolens_adjoint(f_h, dd, B, out, B); return; }          // L = I: the flow-free form, Cf^-1 f included
    if (f_h && fm == FORM_FLOW) {
      model_adjoint(*L.as_flow(), f_h, dd, B, r, B);
    } else {
      if (f_h) {
        mean(L, f_h, r, B);
        if (dd) c->lincomb1((T*)r, (const T*)dd, (const T*)r, 1.0, -1.0, 2 * n / B, B);
      } else {
        CMBL_REQUIRE(dd != nullptr, ERR_ARG, "gradientf with f = 0 and d = 0 is identically zero");
        CMBL_HIP(hipMemcpyAsync(r, dd, sizeof(cx<T>) * n, hipMemcpyDeviceToDevice, c->stream));
      }
      if (f_h && !dd) apply_cn_inv(r, r, B, (T)-1);                        // d = 0: the sign of -(M B L f) rides along
      else apply_cn_inv(r, r, B);
      apply_M(r, B, true, true);
      apply(OP_B, r, r, B, true, true, true);                              // QU Fourier -> (EB) x beam' -> QU Fourier
      L.op_adj_F(r, r, P, B);
    }
    if (f_h) {
      c->harm(r, r, P, B, 0, nullptr, false, true, false);                 // -> harmonic
      apply(OP_CF_INV, f_h, out, B, false, false, false, r, (T)1, (T)-1);  // out = r - Cf^-1 f
    } else {
      c->harm(r, out, P, B, 0, nullptr, false, true, false);
    }
  }

  // conjugate_gradient (src/numerical_algorithms.jl:73-134) driving argmaxf_logpdf (src/maximization.jl:17-42).  a0 = gradientf(f=0,d=0) is identically
  // zero for this linear model (all operators finite), so it is not evaluated.  The scalars live on the device; both forms of the loop, their storage
  // and their end are CgSolver's (engine_cg.hpp).  Which form runs, here and in gradientf: the fused ones need fused() and the LenseFlow or the identity.
  enum Form { FORM_COMPOSED, FORM_FLOW, FORM_IDENTITY };
  Form form(LensOps<T>& L) const { return !fused() ? FORM_COMPOSED : L.as_flow() ? FORM_FLOW : L.as_identity() ? FORM_IDENTITY : FORM_COMPOSED; }
  DevBuf qdev;
  CgSolver<T> cg;
  // What the forms of the iteration share on top of the solver: b = -gradientf(f=0, d) = -L'B'M'Cn^-1 d, the start iterate x and r = b - A x
  // with A = gradientf(., d = 0): both sides carry the sign of the gradient.  Block: the scalar block of the form (CgStateBlock / CgScalBlock).
  auto cg_A(LensOps<T>& L, int B) { return [this, &L, B](const cx<T>* p, cx<T>* Ap, double* pAp) { gradientf(L, p, nullptr, Ap, B); if (pAp) c->dot_F_dev(p, Ap, P, B, pAp); }; }
  template <typename Block> typename CgSolver<T>::Vecs cg_problem(LensOps<T>& L, const cx<T>* dd, const cx<T>* fstart, int maxit, int B) {
    CMBL_REQUIRE(B <= MAXBATCH, ERR_ARG, "nbatch > 256 not supported in reductions");
    const auto v = cg.template begin<Block>(fsize(B), B, maxit);
    std::vector<double> mone(B, -1.0);
    gradientf(L, nullptr, dd, v.b, B);
    c->lincomb((T*)v.b, (T*)v.b, nullptr, mone.data(), nullptr, v.nr, B);
    cg.start(v, fstart, cg_A(L, B));
    return v;
  }
  // A p = -L'B'M'Cn^-1 M B L p - Cf^-1 p of the fused iteration with a LenseFlow; returns the partials of p'Ap.  The two flows, 7 launches between
  // them (basis change + ifft_x, c2r, beam, mask, Fourier mask / Cn^-1 / Fourier mask', mask', beam' + ifft_x) and one after.  Y: scratch.
  DotOut flow_Ap(Flow<T>& L, const cx<T>* p, cx<T>* Y, cx<T>* Ap, int B) {
    model_adjoint(L, p, nullptr, B, Y, B);                                  // Y = -L'B'M'Cn^-1 M B L p
    DotOut oA{};
    by_pol([&](auto pp) { oA = c->pw_flat(PwCgAp<T, decltype(pp)::value>{c->geom(), opref(OP_CF_INV), Y, p, Ap}, B, Ctx<T>::PART_CG_PAP); });   // A p = Y - Cf^-1 p
    return oA;
  }
  // ---- the no-lensing model d = M B f + n (NoLensingDataSet, src/dataset.jl:37-47, 68-73; L = I in the slot) -------------------------------
  // out = A f [+ B'M'Cn^-1 d] = B'M'Cn^-1 (d - M B f) - Cf^-1 f  (harmonic F; dd == nullptr: d = 0; out must not alias f_h), the fused form of
  // gradientf_logpdf (src/dataset.jl:76-80) with the flows taken out of model_adjoint.  With a pixel mask five launches: EB -> beam -> QU with
  // ifft_x (Hermitian rows projected, as in lens_from_harmonic), mask, Fourier mask / residual / Cn^-1 / Fourier mask', mask', beam' + QU -> EB +
  // the prior term (PwNlAp); without one a single flat launch (PwNlDiag).  Returns where the partials of f'(out) were left (PART_CG_PAP).
  DotOut nolens_adjoint(const cx<T>* f_h, const cx<T>* dd, int dB, cx<T>* out, int B) {
    const long sl = (long)P * B;
    DotOut pap{};
    by_pol([&](auto pp) {
      constexpr int PP = decltype(pp)::value;
      const ModeGeom<T> g = c->geom();
      if (!has(OP_MPIX)) {
        PwNlDiag<T, PP> nd{g, {}, {}, opref(OP_CN_INV), opref(OP_CF_INV), dd, dB, f_h, out};
        model_chains(nd.pre, nd.post, true);
        pap = c->pw_flat(nd, B, Ctx<T>::PART_CG_PAP);
        return;
      }
      m1.ensure(sizeof(cx<T>) * sl * c->mplane());
      cx<T>* m = m1.template as<cx<T>>();
      PwChain<T, PP> b1{g, {}, 0, 1, nullptr, T(0), nullptr, T(1)};
      b1.ch.push(opref(OP_B));
      c->template x_pw<PP, true>(f_h, m, b1, B, true);                                  // beam, EB -> QU, ifft_x, Hermitian rows projected
      masked_core<PP>(m, dd, dB, T(-1), true, B);                                       // mask, Fourier mask / residual / Cn^-1 / Fourier mask', mask'; the sign of the gradient
      PwNlAp<T, PP> ap{g, {}, opref(OP_CF_INV), f_h, out};
      ap.post.push(opref(OP_B, true));
      pap = c->template x_pw<PP, false>(m, nullptr, ap, B, false, Ctx<T>::PART_CG_PAP); // fft_x, QU -> EB, beam', - Cf^-1 f, stored; partials of f'(out)
    });
    return pap;
  }
  // The value pass of a log-posterior:  z = mean(f) - d,  w = Cn^-1 z  and  Cf^-1 f,  with z'w in qdev[2] and f'Cf^-1 f in qdev[0], which stay on
  // the device until read_logpdf.  mean_into(z, qdev) enqueues the model's mean of f into z (harmonic F) once the scratch is there.
  struct ValuePass { cx<T>*w, *cfif; double* qd; };
  template <typename MeanF> ValuePass value_pass(MeanF&& mean_into, const cx<T>* f_h, const cx<T>* dd, int B) {
    const long n = fsize(B);
    CMBL_REQUIRE(B <= MAXBATCH, ERR_ARG, "nbatch > 256 not supported in reductions");
    t1.ensure(sizeof(cx<T>) * n); t2.ensure(sizeof(cx<T>) * n); t3.ensure(sizeof(cx<T>) * n); qdev.ensure(sizeof(double) * 3 * MAXBATCH);
    cx<T>*z = t1.template as<cx<T>>(), *cfif = t2.template as<cx<T>>(), *w = t3.template as<cx<T>>();
    double* qd = qdev.template as<double>();
    mean_into(z, qd);
    c->lincomb1((T*)z, (const T*)z, (const T*)dd, 1.0, -1.0, 2 * n / B, B);
    apply_cn_inv(z, w, B);                    c->dot_F_dev(z, w, P, B, qd + 2 * MAXBATCH);
    apply(OP_CF_INV, f_h, cfif, B);           c->dot_F_dev(f_h, cfif, P, B, qd);
    return {w, cfif, qd};
  }
  // logpdf(ds; f) of the no-lensing model per batch slot, -1/2 [ f'Cf^-1 f + (M B f - d)'Cn^-1 (M B f - d) + logdet_sum ] with logdet_sum = logdet Cf +
  // logdet Cn (src/dataset.jl:68-73, src/distributions.jl:11-15), and with gf_h its gradient B'M'Cn^-1 (d - M B f) - Cf^-1 f (src/dataset.jl:76-80)
  // from the same pass through data space.  The sums are formed on the device in double, in a fixed order, and read back once (read_logpdf).
  // Any size, either form of the noise operator.  Reads nothing of phi: OP_CPHI_INV, OP_D*, OP_G_INV need not be set.
  void nolens_logpdf(const cx<T>* f_h, const cx<T>* dd, double* lp, cx<T>* gf_h, int B) {
    const ValuePass q = value_pass([&](cx<T>* z, double* qd) {
      CMBL_HIP(hipMemsetAsync(qd + MAXBATCH, 0, sizeof(double), c->stream)); // the slot of phi'Cphi^-1 phi: this model has none
      apply(OP_B, f_h, z, B);                                                // z = M B f
      apply_M(z, B, false);
    }, f_h, dd, B);
    if (gf_h) {
      apply_M(q.w, B, true);
      apply(OP_B, q.w, q.w, B, true, false, false, nullptr, 0, (T)-1);
      c->lincomb1((T*)gf_h, (const T*)q.w, (const T*)q.cfif, 1.0, -1.0, 2 * fsize(B) / B, B);
    }
    read_logpdf(lp, B, 0);
  }

  // The Wiener filter in the form of form(L).  Fused (CgSolver::solve_fused): A p is flow_Ap with a LenseFlow, nolens_adjoint with the identity (7
  // launches per iteration with a pixel mask, 3 without); the solver's z is free there and serves as flow_Ap's scratch.
  int wiener_cg(LensOps<T>& L, const cx<T>* dd, const cx<T>* fstart, double tol, int maxit, cx<T>* f_out, double* hist, int B) {
    const Form fm = form(L);
    if (fm == FORM_COMPOSED) {
      const auto v = cg_problem<CgStateBlock>(L, dd, fstart, maxit, B);
      cg.solve(v, cg_A(L, B), [&](const cx<T>* r, cx<T>* z, double* rz) { apply(OP_PRECOND_INV, r, z, B); c->dot_F_dev(r, z, P, B, rz); }, tol);
      return cg.template finish<CgStateBlock>(v, f_out, hist);
    }
    const auto v = cg_problem<CgScalBlock>(L, dd, fstart, maxit, B);
    cg.solve_fused(v, P, opref(OP_PRECOND_INV), tol, [&](const cx<T>* p, cx<T>* Ap) {
      return fm == FORM_FLOW ? flow_Ap(*L.as_flow(), p, v.z, Ap, B) : nolens_adjoint(p, nullptr, B, Ap, B);
    });
    return cg.template finish<CgScalBlock>(v, f_out, hist);
  }

  // What grad_logpdf and the composed logpdf_mixed share, for nphi planes of phi (1, or one per slot):  z = M B L f - d with f~ = L f left in
  // ftil;  w = Cn^-1 z,  Cf^-1 f  and  Cphi^-1 phi  with the three sets of quadratic forms in qdev, which stay on the device until read_logpdf.
  // adjoint: w <- -B'M'Cn^-1 z = d/df~ (QU Fourier).  The prior terms are only handed out: each caller forms its own sums with them.
  struct Posterior { cx<T>*w, *cfif, *cpip; };
  Posterior posterior(LensOps<T>& L, const cx<T>* f_h, const cx<T>* phi_F, int nphi, const cx<T>* dd, bool adjoint, int B) {
    ftil.ensure(sizeof(T) * (long)P * B * c->npix()); gphi.ensure(sizeof(cx<T>) * nphi * c->plane());
    const ValuePass q = value_pass([&](cx<T>* z, double*) { mean(L, f_h, z, B, ftil.template as<T>()); }, f_h, dd, B);   // leaves f~ = L f in ftil
    cx<T>*w = q.w, *cfif = q.cfif, *cpip = gphi.template as<cx<T>>();
    apply(OP_CPHI_INV, phi_F, cpip, nphi, false, false, false, nullptr, 0, 1, 1);
    c->dot_F_dev(phi_F, cpip, 1, nphi, q.qd + MAXBATCH);
    if (adjoint) {
      apply_M(w, B, true, true);
      apply(OP_B, w, w, B, true, true, true, nullptr, 0, (T)-1);
    }
    return {w, cfif, cpip};
  }
  // logpdf per slot from the three sets of sums in qdev, read back ONCE, after everything else of the call has been enqueued (a read-back
  // per term drained the stream three times in the middle of a gradient evaluation).  phi_stride: 1 with a phi per slot, 0 with one phi.
  // A NaN logpdf is a VALUE, not an error: MAP_joint's line search penalises it (src/maximization.jl:194-199) and hmc_step
  // rejects the proposal (log(rand()) < NaN is false, src/sampling.jl:414), so it must reach the caller.
  void read_logpdf(double* lp, int B, int phi_stride) {
    double q[3 * MAXBATCH];
    CMBL_HIP(hipMemcpyAsync(q, qdev.template as<double>(), sizeof(double) * 3 * MAXBATCH, hipMemcpyDeviceToHost, c->stream));
    CMBL_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < B; ++i) lp[i] = -0.5 * (q[i] + q[MAXBATCH + i * phi_stride] + q[2 * MAXBATCH + i] + logdet_sum);
  }

  // logpdf(ds; f, phi) (src/dataset.jl:59-66) per batch slot and, where asked for, its gradient with respect to f (harmonic) and phi (B planes,
  // F layout) at once, for any operator whose phi has been set from `phi_F` (one plane):  z = M B L f - d;  w = -B'M'Cn^-1 z;
  // grad_f = L' w - Cf^-1 f;  grad_phi = pullback(L f)(w) - Cphi^-1 phi -- what gradient(phi -> logpdf(ds; f, phi), phi) of MAP_marg evaluates
  // (src/maximization.jl:307).  One forward lens and one pass through data space serve the value and both gradients.
  void grad_logpdf(LensOps<T>& L, const cx<T>* f_h, const cx<T>* phi_F, const cx<T>* dd, double* lp, cx<T>* gf_h, cx<T>* gphi_F, int B, bool quirk) {
    const long n = fsize(B), pl = c->plane();
    CMBL_REQUIRE(!gf_h || L.op_has_adjoint(), ERR_ARG, std::string(L.op_name()) + ": the gradient with respect to f needs L', which the reference does not define for this operator");
    CMBL_REQUIRE(!gphi_F || L.op_has_pullback(), ERR_ARG, std::string(L.op_name()) + ": the reference defines no pullback of L * f with respect to phi for this operator");
    dphi1.ensure(sizeof(cx<T>) * B * pl);
    const Posterior q = posterior(L, f_h, phi_F, 1, dd, gf_h || gphi_F, B);
    cx<T>* w = q.w;
    if (gphi_F) {
      L.op_pullback(ftil.template as<T>(), w, dphi1.template as<cx<T>>(), P, B, quirk);
      for (int b = 0; b < B; ++b) c->lincomb1((T*)(gphi_F + b * pl), (const T*)(dphi1.template as<cx<T>>() + b * pl), (const T*)q.cpip, 1.0, -1.0, 2 * pl, 1);
    } else if (gf_h) L.op_adj_F(w, w, P, B);
    if (gf_h) {
      c->harm(w, w, P, B, 0, nullptr, false, true, false);                  // -> harmonic
      c->lincomb1((T*)gf_h, (const T*)w, (const T*)q.cfif, 1.0, -1.0, 2 * n / B, B);
    }
    read_logpdf(lp, B, 0);
  }

  // d/dfhat = D' \ g_f lives in `w` only between the two delta flows.  grad_theta_logpdf_mixed asks for a copy (QU Fourier, F layout) by setting
  // ghat_out for the duration of its call; nobody else pays for it
  cx<T>* ghat_out = nullptr;
  void keep_ghat(const cx<T>* w, long n) {
    if (ghat_out) CMBL_HIP(hipMemcpyAsync(ghat_out, w, sizeof(cx<T>) * n, hipMemcpyDeviceToDevice, c->stream));
  }

  // logpdf(Mixed(ds); f°, phi°) and optionally its gradient.  fo: map (reference layout == internal), phio: F layout S0.
  // gfo (map) / gphio (F) may be nullptr for value only.
  // Fused form (power-of-two maps).  Launches outside the four flows: phi prior (1), precompute (4), the y pass of f° (1), unmix + Cf^-1
  // + its quadratic form + ifft_x (1), c2r (1), the data-space part (5 with a pixel mask, 1 without), D'^-1 between the delta flows (1),
  // per delta flow the first d/dx pass and the delta-phi epilogue (1 + 3), the final irfft2 (2): 25 with a pixel mask.
  void logpdf_mixed_fused(Flow<T>& L, const T* fo, const cx<T>* phio_F, double* lp, T* gfo, cx<T>* gphio_F, int B, bool quirk) {
    const long sl = (long)P * B, n = fsize(B), np = c->npix(), pl = c->plane();
    phiF.ensure(sizeof(cx<T>) * B * pl); fhat.ensure(sizeof(T) * sl * np); ftil.ensure(sizeof(T) * sl * np);
    fh.ensure(sizeof(cx<T>) * n); t2.ensure(sizeof(cx<T>) * n); t3.ensure(sizeof(cx<T>) * n);
    gphi.ensure(sizeof(cx<T>) * B * pl); dphi1.ensure(sizeof(cx<T>) * B * pl);
    mp2.ensure(sizeof(T) * sl * np);
    cx<T>*phi = phiF.template as<cx<T>>(), *f_h = fh.template as<cx<T>>(), *w = t3.template as<cx<T>>(), *cfif = t2.template as<cx<T>>();
    cx<T>* cpip = gphi.template as<cx<T>>();
    CMBL_REQUIRE(B <= MAXBATCH, ERR_ARG, "nbatch > 256 not supported in reductions");
    qdev.ensure(sizeof(double) * 3 * MAXBATCH);
    double* qd = qdev.template as<double>();
    // phi = G \ phi° ; Cphi^-1 phi ; phi' Cphi^-1 phi
    DotOut parts[3];
    parts[1] = c->pw_flat(PwPhiPrior<T>{c->lam.template as<T>(), pl, op(OP_G_INV).d[0], op(OP_CPHI_INV).d[0], phio_F, phi, cpip}, B, Ctx<T>::PART_QP);
    L.set_phi_F(phi, B);
    // fhat = L \ f° (its y transform stays in A3) ; f = D \ fhat ; Cf^-1 f ; f' Cf^-1 f ; the y-transformed f goes straight into the forward flow
    L.flow_map(fo, fhat.template as<T>(), P, B, true, false, true, &L.A3);
    cx<T>* a = L.abuf_ensure(L.A, sl);
    by_pol([&](auto pp) {
      constexpr int PP = decltype(pp)::value;
      parts[0] = c->template x_pw<PP, false>(L.A3.template as<cx<T>>(), a, PwUnmixPrior<T, PP>{c->geom(), opref(OP_D_INV), opref(OP_CF_INV), f_h, cfif}, B, true, Ctx<T>::PART_QF);
    });
    c->y_c2r(a, mp2.template as<T>(), sl);
    L.flow_map(mp2.template as<T>(), ftil.template as<T>(), P, B, false, true, true, &L.A);       // f~ = L f in ftil, rfft_y(f~) in A
    // z = M B L f - d ; z' Cn^-1 z ; w = -B'M'Cn^-1 z  (QU Fourier) with ifft_x(w) ready in L.H
    parts[2] = data_space(gfo ? L.hbuf_ensure(sl) : nullptr, L.A.template as<cx<T>>(), d_h.template as<cx<T>>(), Bd, T(-1), w, gfo == nullptr, B);
    double* const outs[3] = {qd, qd + MAXBATCH, qd + 2 * MAXBATCH};
    c->finish_parts(parts, outs, 3, B);
    if (!gfo) { read_logpdf(lp, B, 1); return; }
    // pullback through f~ = L f : delta flow t 1->0 from (f~, w, 0)
    L.flow_delta(ftil.template as<T>(), w, dphi1.template as<cx<T>>(), P, B, true, quirk, true, &L.A, true);
    // g_f = df1 - Cf^-1 f (harmonic) ; d/dfhat = D' \ g_f -> QU Fourier, with its ifft_x in L.H
    by_pol([&](auto pp) {
      constexpr int PP = decltype(pp)::value;
      PwChain<T, PP> ch{c->geom(), {}, 1, 1, cfif, T(-1), w, T(1)};
      ch.ch.push(opref(OP_D_INV, true));
      c->template x_pw<PP, true>(w, L.hbuf_ensure(sl), ch, B);
    });
    keep_ghat(w, n);
    // pullback through fhat = L \ f° : delta flow t 0->1 from (fhat, w, 0); the epilogue forms d/dphi° = G' \ (dphi1 + dphi2 - Cphi^-1 phi)
    const DphiTail<T> tail{dphi1.template as<cx<T>>(), cpip, op(OP_G_INV).d[0]};
    L.flow_delta(fhat.template as<T>(), w, gphio_F, P, B, false, quirk, true, &L.A3, true, &tail);
    c->F_to_map(w, gfo, sl);                                                // d/df° in f°'s basis (QU map)
    read_logpdf(lp, B, 1);
  }
  void logpdf_mixed(Flow<T>& L, const T* fo, const cx<T>* phio_F, double* lp, T* gfo, cx<T>* gphio_F, int B, bool quirk) {
    CMBL_REQUIRE(Bd == B, ERR_SHAPE, "dataset data batch size differs from nbatch");
    if (fused()) return logpdf_mixed_fused(L, fo, phio_F, lp, gfo, gphio_F, B, quirk);
    const long sl = (long)P * B, n = fsize(B), np = c->npix(), pl = c->plane();
    phiF.ensure(sizeof(cx<T>) * B * pl); fhat.ensure(sizeof(T) * sl * np); fh.ensure(sizeof(cx<T>) * n);
    dphi1.ensure(sizeof(cx<T>) * B * pl); dphi2.ensure(sizeof(cx<T>) * B * pl);
    cx<T>*phi = phiF.template as<cx<T>>(), *f_h = fh.template as<cx<T>>();
    // phi = G \ phi°
    apply(OP_G_INV, phio_F, phi, B, false, false, false, nullptr, 0, 1, 1);
    L.set_phi_F(phi, B);
    // fhat = L \ f° ; f = D \ fhat
    L.flow_map(fo, fhat.template as<T>(), P, B, true);
    c->rfft2_F(fhat.template as<T>(), f_h, sl);
    apply(OP_D_INV, f_h, f_h, B, false, true, false);
    // z = M B L f - d ; the quadratic forms ; with a gradient, d/df~ = -B'M'Cn^-1 z -> QU Fourier
    const Posterior q = posterior(L, f_h, phi, B, d_h.template as<cx<T>>(), gfo != nullptr, B);
    cx<T>*w = q.w, *cfif = q.cfif, *cpip = q.cpip;
    if (!gfo) { read_logpdf(lp, B, 1); return; }
    // pullback through f~ = L f : delta flow t 1->0 from (f~, w, 0)
    L.flow_delta(ftil.template as<T>(), w, dphi1.template as<cx<T>>(), P, B, true, quirk);
    // g_f = df1 - Cf^-1 f   (harmonic) ; then d/dfhat = D' \ g_f  -> QU Fourier
    c->harm(w, w, P, B, 0, nullptr, false, true, false);
    c->lincomb1((T*)w, (const T*)w, (const T*)cfif, 1.0, -1.0, 2 * n / B, B);
    apply(OP_D_INV, w, w, B, true, false, true);
    keep_ghat(w, n);
    // pullback through fhat = L \ f° : delta flow t 0->1 from (fhat, w, 0)
    L.flow_delta(fhat.template as<T>(), w, dphi2.template as<cx<T>>(), P, B, false, quirk);
    // d/df° in f°'s basis (QU map)
    c->F_to_map(w, gfo, sl);
    // g_phi = dphi1 + dphi2 - Cphi^-1 phi ; d/dphi° = G' \ g_phi
    cx<T>* g = dphi1.template as<cx<T>>();
    c->lincomb1((T*)g, (const T*)g, (const T*)dphi2.p, 1.0, 1.0, 2 * pl, B);
    c->lincomb1((T*)g, (const T*)g, (const T*)cpip, 1.0, -1.0, 2 * pl, B);
    apply(OP_G_INV, g, gphio_F, B, true, false, false, nullptr, 0, 1, 1);
    read_logpdf(lp, B, 1);
  }

  // ---- θ layer on the device (kernels_theta.hpp): the model installed once per data set, the operators of one θ, the grid of logpdf(Mixed; θ) ----
  struct ThetaModel {
    bool set = false, has_c0 = false, has_g = false;
    int np = 0, nbands = 0, namps = 0;
    int bmask[TH_MAXBANDS] = {0, 0, 0}, bnb[TH_MAXBANDS] = {0, 0, 0}, boff[TH_MAXBANDS] = {0, 0, 0};
    double s2len = 0, r0 = 1, aphi0 = 1, logdet_cn = 0;
    DevBuf planes;                           // double, F layout: cfs, c0, cten, cn, d0inv (np planes each), cphi0, nphi, g0inv, guser
    DevBuf bidx;                             // int32, F layout: one bin-index plane per band
    DevBuf ops;                              // T, F layout: the scratch operator sets pinv(Cf) (np), pinv(D) (np), pinv(Cphi), pinv(G)
    DevBuf part, sums, amps;                 // partial sums [3][nblk], their totals [3], the amplitude vectors of a grid call
    // the θ-gradient (k_theta_grad): each band's modes sorted by bin (int32), the chunks of those lists (ThChunk), per amplitude its first
    // chunk (int32, namps + 1); per call the per-mode band terms, the partial sums of both stages, the result [nbatch][2 + namps], ĝ, ∇f°
    DevBuf glist, gchunks, gampchunk, gcontrib, gpart, gcpart, gout, ghat, gfo;
    int nchunks = 0;
  } th;
  T* th_op(int which) {
    T* o = th.ops.template as<T>(); const long pl = c->plane();
    return which == OP_CF_INV ? o : which == OP_D_INV ? o + th.np * pl : which == OP_CPHI_INV ? o + 2 * th.np * pl : o + (2 * th.np + 1) * pl;
  }
  // a reference-layout plane ([x][ky]) in the F layout ([ky][x slot]; the slot order of Ctx::build_geometry)
  template <typename V> void th_toF(const V* ref, V* out, int nplanes) const {
    const int Nx = c->Nx, Nyh = c->Nyh;
    std::vector<int> xf(Nx);
    for (int i = 0; i < Nx; ++i) { unsigned r = i; if (!c->generic) { r = 0; for (int b = 0; b < c->lgNx; ++b) r |= ((i >> b) & 1u) << (c->lgNx - 1 - b); } xf[i] = (int)r; }
    for (int p = 0; p < nplanes; ++p)
      for (int k = 0; k < Nyh; ++k)
        for (int i = 0; i < Nx; ++i) out[((size_t)p * Nyh + k) * Nx + i] = ref[((size_t)p * Nx + xf[i]) * Nyh + k];
  }
  // everything theta._ops reads, copied; D0 = D(r0) and g0 = G-numerator at Aphi0 do not depend on θ and are derived here, on the host, with
  // the very functions the kernel uses
  void theta_install(const double* cfs, int nplanes, const double* c0, int nbands, const int* band_planes, const int32_t* band_idx, const int* band_nbins,
                     const double* cten, const double* cn, double s2len, double r0, const double* cphi0, double aphi0, const double* nphi,
                     const double* g, double logdet_cn) {
    CMBL_REQUIRE(nplanes == (P == 3 ? 5 : P), ERR_SHAPE, "theta_model: the covariances take npol planes (5 for IQU)");
    CMBL_REQUIRE(nbands >= 0 && nbands <= TH_MAXBANDS, ERR_ARG, "theta_model: at most three bandpower bands (TT, TE, EE)");
    CMBL_REQUIRE(nbands == 0 || (c0 && band_planes && band_idx && band_nbins), ERR_ARG, "theta_model: bands need the base covariance, their planes, bin indices and bin counts");
    CMBL_REQUIRE(r0 != 0 && aphi0 != 0 && std::isfinite(r0) && std::isfinite(aphi0), ERR_ARG, "theta_model: r0 and Aphi0 must be finite and non-zero");
    const long pl = c->plane();
    const int np = nplanes;
    int namps = 0;
    for (int k = 0; k < nbands; ++k) {
      CMBL_REQUIRE(band_nbins[k] >= 1 && band_nbins[k] <= 65535, ERR_ARG, "theta_model: a band needs 1 ... 65535 bins");
      CMBL_REQUIRE(band_planes[k] > 0 && band_planes[k] < (1 << np) && (np != 5 || !(band_planes[k] & 16)), ERR_ARG, "theta_model: a band rescales planes of the covariance, never BB of the block form");
      for (long j = 0; j < pl; ++j) CMBL_REQUIRE(band_idx[(size_t)k * pl + j] >= 0 && band_idx[(size_t)k * pl + j] <= band_nbins[k], ERR_ARG, "theta_model: a bin index outside [0, nbins]");
      namps += band_nbins[k];
    }
    std::vector<double> h((size_t)(5 * np + 4) * pl, 0.0);
    double *hcfs = h.data(), *hc0 = hcfs + np * pl, *hcten = hc0 + np * pl, *hcn = hcten + np * pl, *hd0 = hcn + np * pl;
    double *hcphi = hd0 + np * pl, *hnphi = hcphi + pl, *hg0 = hnphi + pl, *hgu = hg0 + pl;
    th_toF(cfs, hcfs, np); th_toF(cten, hcten, np); th_toF(cn, hcn, np); th_toF(cphi0, hcphi, 1); th_toF(nphi, hnphi, 1);
    if (c0) th_toF(c0, hc0, np);
    if (g) th_toF(g, hgu, 1);
    for (long j = 0; j < pl; ++j) {
      if (np == 5) {
        auto at = [&](const double* a) { return ThBlk{a[j], a[pl + j], a[2 * pl + j], a[3 * pl + j], a[4 * pl + j]}; };
        const ThBlk d0i = th_pinv(th_mix(th_add(at(hcfs), at(hcten)), th_noise2(at(hcn), s2len)));
        hd0[j] = d0i.a; hd0[pl + j] = d0i.b; hd0[2 * pl + j] = d0i.c; hd0[3 * pl + j] = d0i.d; hd0[4 * pl + j] = d0i.e;
      } else {
        for (int p = 0; p < np; ++p) hd0[p * pl + j] = th_pinv(th_mix(hcfs[p * pl + j] + hcten[p * pl + j], hcn[p * pl + j], s2len));
      }
      hg0[j] = th_pinv(th_g(hnphi[j], hcphi[j]));
    }
    th.set = false;                            // a second install replaces the first; a failed one leaves none
    th.planes.ensure(sizeof(double) * h.size());
    CMBL_HIP(hipMemcpyAsync(th.planes.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
    th.nchunks = 0;
    if (nbands) {
      std::vector<int32_t> hb((size_t)nbands * pl);
      th_toF(band_idx, hb.data(), nbands);
      th.bidx.ensure(sizeof(int32_t) * hb.size());
      CMBL_HIP(hipMemcpyAsync(th.bidx.p, hb.data(), sizeof(int32_t) * hb.size(), hipMemcpyHostToDevice, c->stream));
      // the per-bin sums of the θ-gradient: per band the modes that lie in a bin, sorted by (bin, mode), cut into chunks of at most TH_CHUNK
      // entries that never straddle a bin; the chunks of one amplitude are consecutive (as ClBins orders its modes, kernels_cl.hpp)
      std::vector<int32_t> list; std::vector<ThChunk> chunks; std::vector<int32_t> ampchunk;
      for (int k = 0, off = 0; k < nbands; off += band_nbins[k], ++k) {
        std::vector<std::vector<int32_t>> bins(band_nbins[k]);
        for (long j = 0; j < pl; ++j) { const int32_t i = hb[(size_t)k * pl + j]; if (i < band_nbins[k]) bins[i].push_back((int32_t)j); }
        for (int i = 0; i < band_nbins[k]; ++i) {
          ampchunk.push_back((int32_t)chunks.size());
          for (size_t s = 0; s < bins[i].size(); s += TH_CHUNK)
            chunks.push_back(ThChunk{(int)(list.size() + s), (int)std::min<size_t>(TH_CHUNK, bins[i].size() - s), k, off + i});
          list.insert(list.end(), bins[i].begin(), bins[i].end());
        }
      }
      ampchunk.push_back((int32_t)chunks.size());
      th.nchunks = (int)chunks.size();
      th.glist.ensure(sizeof(int32_t) * std::max<size_t>(1, list.size())); th.gchunks.ensure(sizeof(ThChunk) * std::max<size_t>(1, chunks.size()));
      th.gampchunk.ensure(sizeof(int32_t) * ampchunk.size());
      if (!list.empty()) CMBL_HIP(hipMemcpyAsync(th.glist.p, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice, c->stream));
      if (!chunks.empty()) CMBL_HIP(hipMemcpyAsync(th.gchunks.p, chunks.data(), sizeof(ThChunk) * chunks.size(), hipMemcpyHostToDevice, c->stream));
      CMBL_HIP(hipMemcpyAsync(th.gampchunk.p, ampchunk.data(), sizeof(int32_t) * ampchunk.size(), hipMemcpyHostToDevice, c->stream));
      CMBL_HIP(hipStreamSynchronize(c->stream));   // hb and the lists go away
    }
    CMBL_HIP(hipStreamSynchronize(c->stream));     // ... and h
    th.ops.ensure(sizeof(T) * (2 * np + 2) * pl);
    th.part.ensure(sizeof(double) * 3 * TH_MAXBLK); th.sums.ensure(sizeof(double) * 3);
    th.np = np; th.nbands = nbands; th.namps = namps; th.has_c0 = c0 != nullptr; th.has_g = g != nullptr;
    for (int k = 0, off = 0; k < TH_MAXBANDS; ++k) {
      th.bmask[k] = k < nbands ? band_planes[k] : 0; th.bnb[k] = k < nbands ? band_nbins[k] : 0; th.boff[k] = off;
      off += th.bnb[k];
    }
    th.s2len = s2len; th.r0 = r0; th.aphi0 = aphi0; th.logdet_cn = logdet_cn;
    th.set = true;
  }
  // the operators of one θ into the scratch sets and the three sums into th.sums (device).  r / aphi NaN: not named.  amps_dev: this θ's
  // amplitude vectors on the device, or nullptr (ones)
  ThetaDev theta_dev() const {
    const long pl = c->plane();
    const double* d = th.planes.template as<double>();
    ThetaDev m{};
    m.cfs = d; m.c0 = th.has_c0 ? d + th.np * pl : nullptr; m.cten = d + 2 * th.np * pl; m.cn = d + 3 * th.np * pl; m.d0inv = d + 4 * th.np * pl;
    m.cphi0 = d + 5 * th.np * pl; m.nphi = m.cphi0 + pl; m.g0inv = m.nphi + pl; m.guser = th.has_g ? m.g0inv + pl : nullptr;
    for (int k = 0; k < TH_MAXBANDS; ++k) { m.bidx[k] = k < th.nbands ? th.bidx.template as<int>() + (size_t)k * pl : nullptr; m.bmask[k] = th.bmask[k]; m.bnb[k] = th.bnb[k]; m.boff[k] = th.boff[k]; }
    m.nbands = th.nbands; m.np = th.np; m.Nx = c->Nx; m.Ny = c->Ny; m.Nyh = c->Nyh; m.pl = pl; m.s2len = th.s2len; m.aphi0 = th.aphi0;
    return m;
  }
  ThetaPoint theta_point(double r, double aphi, const double* amps_dev) const {
    ThetaPoint t{};
    t.r_named = !std::isnan(r); t.s = (t.r_named ? r : th.r0) / th.r0;
    t.g_theta = !std::isnan(aphi) && !th.has_g; t.aphi = std::isnan(aphi) ? th.aphi0 : aphi;
    t.amps = amps_dev;
    return t;
  }
  void theta_eval(double r, double aphi, const double* amps_dev) {
    CMBL_REQUIRE(th.set, ERR_STATE, "no θ model has been installed on this data set (cmbl_dataset_theta_model)");
    const long pl = c->plane();
    const ThetaDev m = theta_dev();
    const ThetaPoint t = theta_point(r, aphi, amps_dev);
    const int nblk = (int)std::min<long>(TH_MAXBLK, (pl + NTP - 1) / NTP);
    double* part = th.part.template as<double>();
    if (th.np == 5) CMBL_LAUNCH(c, K_PWFLAT, (k_theta_ops<T, true>), dim3((unsigned)nblk), 0, c->stream, m, t, th_op(OP_CF_INV), th_op(OP_D_INV), th_op(OP_CPHI_INV), th_op(OP_G_INV), part);
    else CMBL_LAUNCH(c, K_PWFLAT, (k_theta_ops<T, false>), dim3((unsigned)nblk), 0, c->stream, m, t, th_op(OP_CF_INV), th_op(OP_D_INV), th_op(OP_CPHI_INV), th_op(OP_G_INV), part);
    CMBL_LAUNCH(c, K_REDUCE, k_theta_sum, dim3(1), 0, c->stream, (const double*)part, nblk, th.sums.template as<double>());
  }
  void theta_sums(double* s3) {
    CMBL_HIP(hipMemcpyAsync(s3, th.sums.p, sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
    CMBL_HIP(hipStreamSynchronize(c->stream));
  }
  const double* theta_amps(const double* amps_host, int namps, int ntheta) {
    CMBL_REQUIRE(th.set, ERR_STATE, "no θ model has been installed on this data set (cmbl_dataset_theta_model)");
    CMBL_REQUIRE(amps_host ? namps == th.namps : namps == 0, ERR_SHAPE, "the amplitude vectors of a θ hold one value per bin of every band of the installed model (or none at all)");
    if (!amps_host || namps == 0) return nullptr;
    th.amps.ensure(sizeof(double) * (size_t)namps * ntheta);
    CMBL_HIP(hipMemcpyAsync(th.amps.p, amps_host, sizeof(double) * (size_t)namps * ntheta, hipMemcpyHostToDevice, c->stream));
    CMBL_HIP(hipStreamSynchronize(c->stream));     // the caller's array may go away
    return th.amps.template as<double>();
  }
  // While one of these lives, the four θ-dependent operator sets of the data set point at the scratch sets; they and logdet_sum are put back
  // on every way out
  struct ThetaScratchOps {
    static constexpr int ids[4] = {OP_CF_INV, OP_D_INV, OP_CPHI_INV, OP_G_INV};
    struct Saved { int nplanes, kind; const T* d[5]; };
    Dataset* ds; Saved s[4]; double logdet;
    explicit ThetaScratchOps(Dataset* ds_) : ds(ds_), logdet(ds_->logdet_sum) {
      const long pl = ds->c->plane();
      for (int i = 0; i < 4; ++i) {
        Op& o = ds->ops[ids[i]];
        s[i].nplanes = o.nplanes; s[i].kind = o.kind; for (int k = 0; k < 5; ++k) s[i].d[k] = o.d[k];
        const int n = i < 2 ? ds->th.np : 1;
        o.nplanes = n; o.kind = n == 5 ? 2 : 1;
        for (int k = 0; k < 5; ++k) o.d[k] = k < n ? ds->th_op(ids[i]) + (size_t)k * pl : nullptr;
      }
    }
    ThetaScratchOps(const ThetaScratchOps&) = delete;
    ~ThetaScratchOps() { for (int i = 0; i < 4; ++i) { Op& o = ds->ops[ids[i]]; o.nplanes = s[i].nplanes; o.kind = s[i].kind; for (int k = 0; k < 5; ++k) o.d[k] = s[i].d[k]; } ds->logdet_sum = logdet; }
  };
  // lp[i * B + b] = logpdf(Mixed(ds); f°_b, phi°_b, θ_i) (src/dataset.jl:84-87).  The four θ-dependent operator sets and logdet_sum of the data set
  // point at the scratch sets while the grid runs and are put back on every way out.
  void logpdf_mixed_theta(Flow<T>& L, const T* fo, const cx<T>* phio_F, int B, int ntheta, const double* r, const double* aphi, const double* amps_host,
                          int namps, double* lp) {
    const double* ad = theta_amps(amps_host, namps, ntheta);
    const ThetaScratchOps keep(this);
    for (int i = 0; i < ntheta; ++i) {
      theta_eval(r[i], aphi[i], ad ? ad + (size_t)i * namps : nullptr);
      double s[3];
      theta_sums(s);
      logdet_sum = s[0] + th.logdet_cn;
      logpdf_mixed(L, fo, phio_F, lp + (size_t)i * B, nullptr, nullptr, B, false);
      for (int b = 0; b < B; ++b) lp[(size_t)i * B + b] -= s[1] + s[2];
    }
  }
  // testing aid: the scratch operator set `which` of one θ in the reference layout, and the three sums
  void theta_readback(double r, double aphi, const double* amps_host, int namps, int which, T* out_ref, double* sums_host) {
    CMBL_REQUIRE(which == OP_CF_INV || which == OP_D_INV || which == OP_CPHI_INV || which == OP_G_INV, ERR_ARG, "theta_ops: which is CMBL_OP_CF_INV, _D_INV, _CPHI_INV or _G_INV");
    const double* ad = theta_amps(amps_host, namps, 1);
    theta_eval(r, aphi, ad);
    if (out_ref) c->F2ref_real(th_op(which), out_ref, (which == OP_CF_INV || which == OP_D_INV) ? th.np : 1);
    double s[3];
    theta_sums(s);
    if (sums_host) for (int k = 0; k < 3; ++k) sums_host[k] = s[k];
  }

  // ---- the θ-gradient (k_theta_grad): grad[b][2 + namps] = (d/dr, d/dAphi, d/d amplitudes in install order) per slot; what `want` leaves out is 0 ----
  // a derivative is taken with respect to a parameter that θ names; the arguments are checked before anything is uploaded or enqueued
  // (a model installed, then want / NaN / NULL, then the amplitude count in theta_amps)
  const double* theta_grad_args(double r, double aphi, const double* amps_host, int namps, int want, int B) {
    CMBL_REQUIRE(th.set, ERR_STATE, "no θ model has been installed on this data set (cmbl_dataset_theta_model)");
    CMBL_REQUIRE(want > 0 && want < 8, ERR_ARG, "theta gradient: want is a non-empty mask of CMBL_THETA_R, CMBL_THETA_APHI, CMBL_THETA_AMPS");
    CMBL_REQUIRE(!(want & TH_WANT_R) || !std::isnan(r), ERR_ARG, "theta gradient: the derivative with respect to r needs r named in θ (not NaN)");
    CMBL_REQUIRE(!(want & TH_WANT_APHI) || !std::isnan(aphi), ERR_ARG, "theta gradient: the derivative with respect to Aphi needs Aphi named in θ (not NaN)");
    CMBL_REQUIRE(!(want & TH_WANT_AMPS) || (amps_host && namps != 0), ERR_ARG, "theta gradient: the derivative with respect to the amplitudes needs amps_host (and a model with bands)");
    CMBL_REQUIRE(B <= MAXBATCH, ERR_ARG, "nbatch > 256 not supported in reductions");
    return theta_amps(amps_host, namps, 1);
  }
  // grad_host is laid out with the CALLER's amplitude count: rows of 2 + th.namps doubles when the amplitudes were given, of 2 when they were
  // not (amps_dev == nullptr: a θ that names no band, whatever the model holds)
  template <bool MIXED> void theta_grad_run(const ThetaFields<T>& fl, double r, double aphi, const double* amps_dev, int want, int B, double* grad_host) {
    const long pl = c->plane();
    const int nblk = (int)std::min<long>(TH_MAXBLK, (pl + NTP - 1) / NTP), nout = 2 + (amps_dev ? th.namps : 0);
    th.gpart.ensure(sizeof(double) * 2 * TH_MAXBLK * MAXBATCH); th.gout.ensure(sizeof(double) * (2 + th.namps) * MAXBATCH);
    if (want & TH_WANT_AMPS) {
      th.gcontrib.ensure(sizeof(double) * (size_t)B * th.nbands * pl);
      th.gcpart.ensure(sizeof(double) * (size_t)B * std::max(1, th.nchunks));
    }
    const ThetaDev m = theta_dev();
    const ThetaPoint t = theta_point(r, aphi, amps_dev);
    double *part = th.gpart.template as<double>(), *contrib = th.gcontrib.template as<double>(), *cpart = th.gcpart.template as<double>();
    const dim3 grid((unsigned)nblk, (unsigned)B);
    if (th.np == 5) CMBL_LAUNCH(c, K_PWFLAT, (k_theta_grad<T, true, MIXED>), grid, 0, c->stream, m, t, fl, want, th.r0, part, contrib);
    else CMBL_LAUNCH(c, K_PWFLAT, (k_theta_grad<T, false, MIXED>), grid, 0, c->stream, m, t, fl, want, th.r0, part, contrib);
    if ((want & TH_WANT_AMPS) && th.nchunks > 0)
      CMBL_LAUNCH(c, K_REDUCE, k_theta_bins, dim3((unsigned)th.nchunks, (unsigned)B), 0, c->stream, th.gchunks.template as<ThChunk>(), th.glist.template as<int>(),
                  (const double*)contrib, th.nbands, pl, cpart);
    CMBL_LAUNCH(c, K_REDUCE, k_theta_grad_sum, dim3((unsigned)nout, (unsigned)B), 0, c->stream, (const double*)part, nblk, (const double*)cpart, th.nchunks,
                th.gampchunk.template as<int>(), want, th.gout.template as<double>());
    CMBL_HIP(hipMemcpyAsync(grad_host, th.gout.p, sizeof(double) * (size_t)nout * B, hipMemcpyDeviceToHost, c->stream));
    CMBL_HIP(hipStreamSynchronize(c->stream));
  }
  // ∇θ logpdf(ds; f, phi, θ) at fixed fields: f harmonic, phi Fourier with one plane per slot, both F layout.  No lensing operator, no data term
  void grad_theta_logpdf(const cx<T>* f_h, const cx<T>* phi_F, int B, double r, double aphi, const double* amps_host, int namps, int want, double* grad_host) {
    const double* ad = theta_grad_args(r, aphi, amps_host, namps, want, B);
    theta_grad_run<false>(ThetaFields<T>{f_h, phi_F, nullptr, nullptr, nullptr}, r, aphi, ad, want, B, grad_host);
  }
  // logpdf(Mixed(ds); f°, phi°, θ) and its θ-gradient at one θ: the operators of θ go to the scratch sets (as in logpdf_mixed_theta), the
  // library's own gradient of logpdf(Mixed) runs on them -- leaving f in fh, phi in phiF, d/dphi° in gphio_F and, through ghat_out, a copy
  // of d/dfhat -- and one pass forms the explicit, the cross and the log-determinant terms from them
  void grad_theta_logpdf_mixed(Flow<T>& L, const T* fo, const cx<T>* phio_F, cx<T>* gphio_F, int B, double r, double aphi, const double* amps_host,
                               int namps, int want, double* lp, double* grad_host) {
    const double* ad = theta_grad_args(r, aphi, amps_host, namps, want, B);
    const long n = fsize(B);
    th.ghat.ensure(sizeof(cx<T>) * n); th.gfo.ensure(sizeof(T) * (long)P * B * c->npix());
    double s[3];
    {
      const ThetaScratchOps keep(this);
      struct Unhook { Dataset* ds; ~Unhook() { ds->ghat_out = nullptr; } } unhook{this};
      theta_eval(r, aphi, ad);
      theta_sums(s);
      logdet_sum = s[0] + th.logdet_cn;
      ghat_out = th.ghat.template as<cx<T>>();
      logpdf_mixed(L, fo, phio_F, lp, th.gfo.template as<T>(), gphio_F, B, false);
    }
    for (int b = 0; b < B; ++b) lp[b] -= s[1] + s[2];
    cx<T>* gh = th.ghat.template as<cx<T>>();
    c->harm(gh, gh, P, B, 0, nullptr, false, true, false);                  // QU Fourier -> harmonic
    theta_grad_run<true>(ThetaFields<T>{fh.template as<cx<T>>(), phiF.template as<cx<T>>(), gh, phio_F, gphio_F}, r, aphi, ad, want, B, grad_host);
  }
};

}  // namespace cmbl
