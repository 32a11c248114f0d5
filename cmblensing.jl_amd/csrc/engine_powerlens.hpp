// Host side of cmbl_powerlens_*: PowerLens (src/powerlens.jl) and Taylens (src/taylens.jl) on the device.
// One deflection (the reference has require_unbatched on it, src/powerlens.jl:25), any number of (pol, batch) slices of f.  Per deflection: the
// table (pixel-unit displacement; for Taylens the source pixel and the residual).  Per apply and per total order n: one pointwise launch that
// makes the n + 1 planes of that order for all slices, one batched transform over them, one pointwise launch that folds them into the result --
// 1 + (order + 1)(order + 2) / 2 - 1 plane transforms per slice, scratch of (order + 1) S planes.  Every launch goes to the context's stream,
// nothing synchronises with the host and nothing uses atomics: results are bit-identical between runs.
#pragma once
#include <initializer_list>
#include "engine.hpp"
#include "kernels_powerlens.hpp"

namespace cmbl {

enum { PL_POWERLENS = 0, PL_TAYLENS = 1 };

struct PowerLensApi {                        // what the C ABI (api.hip) holds of a PowerLens / Taylens (see FlowApi in engine.hpp)
  virtual ~PowerLensApi() = default;
  virtual void set_phi(int basis, const void* phi, int nb) = 0;
  virtual void set_deflection(const void* dy_rad, const void* dx_rad) = 0;
  virtual void apply(int mode, int bi, const void* in, int bo, void* out, int P, int B) = 0;
};

#define CMBL_PL_ORDERS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)
// fn(integral_constant<int, n>) for a run-time order n in FIRST..12 (FIRST = 0: Taylens' bare permutation as well)
template <int FIRST, typename Fn> void by_order(int n, const char* who, Fn&& fn) {
  if constexpr (FIRST == 0) { if (n == 0) return fn(std::integral_constant<int, 0>{}); }
  switch (n) {
#define CMBL_X(N) case N: return fn(std::integral_constant<int, N>{});
    CMBL_PL_ORDERS(CMBL_X)
#undef CMBL_X
    default: fail(ERR_ARG, std::string(who) + ": order outside " + (FIRST ? "1" : "0") + "..12");
  }
}

template <typename T>
struct PowerLens : PowerLensApi, LensOps<T> {
  Ctx<T>* c;
  const int order;
  const bool taylens;
  bool ready = false;
  const T dx;                                // Δx in T
  DevBuf defl, u, src;                       // deflection maps [2][npix] (x then y, radians); the table
  DevBuf phiF, gF;                           // set_phi scratch
  DevBuf fF, dF, dmaps, inm, outm;           // F of the argument (the adjoint's result), the planes and maps of one order, boundary maps (Ctx::as_maps / map_dst)
  static constexpr int V = 16 / sizeof(T);   // reals per vector access

  PowerLens(Ctx<T>* ctx, int order_, int kind) : c(ctx), order(order_), taylens(kind == PL_TAYLENS), dx(ctx->dx()) {}
  PowerLens(const PowerLens&) = delete;
  PowerLens& operator=(const PowerLens&) = delete;

  static PlCoef<T> coef(int n) {             // 1 / (a! (n-a)!) in double
    double fact[PL_MAXORDER + 1] = {1};
    for (int k = 1; k <= PL_MAXORDER; ++k) fact[k] = fact[k - 1] * k;
    PlCoef<T> cf{};
    for (int a = 0; a <= n; ++a) cf.c[a] = (T)(1.0 / (fact[a] * fact[n - a]));
    return cf;
  }
  dim3 fgrid() const { return dim3(nblocks(c->plane())); }
  dim3 pgrid(int v) const { return dim3(nblocks(c->npix() / v)); }
  // V pixels per thread where every plane of every array starts on a 16-byte boundary
  bool vec(std::initializer_list<const void*> ps) const {
    if (c->npix() % V) return false;
    for (const void* p : ps) if ((uintptr_t)p % 16) return false;
    return true;
  }

  void table() {
    const long np = c->npix();
    u.ensure(sizeof(cx<T>) * np);
    if (taylens) src.ensure(sizeof(unsigned) * np);
    CMBL_LAUNCH(c, K_PL, (k_pl_table<T>), pgrid(1), 0, c->stream, (const T*)(defl.as<T>() + np), (const T*)defl.as<T>(), dx, taylens ? 1 : 0, u.as<cx<T>>(),
                src.as<unsigned>(), c->Ny, c->Nx);
    ready = true;
  }
  void set_phi(int basis, const void* phi, int nb) override {
    CMBL_REQUIRE(nb == 1, ERR_SHAPE, "PowerLens / Taylens with a batched phi is not implemented (require_unbatched, src/powerlens.jl:25, src/taylens.jl:27)");
    c->deflection_maps(basis, phi, phiF, gF, defl, K_PL);                   // d = ∇ϕ (src/powerlens.jl:23)
    table();
  }
  void set_deflection(const void* dy_rad, const void* dx_rad) override {
    c->deflection_maps(dy_rad, dx_rad, defl);
    table();
  }

  void mult(int n, const cx<T>* F, cx<T>* out, int S) {
    by_order<1>(n, "PowerLens", [&](auto o) {
      CMBL_LAUNCH(c, K_PL, (k_pl_mult<T, decltype(o)::value>), fgrid(), 0, c->stream, F, out, c->lx_r.template as<T>(), c->ly.template as<T>(), dx, c->Nx, c->plane(), S);
    });
  }
  void combine(int n, const cx<T>* G, cx<T>* r, int S) {
    by_order<1>(n, "PowerLens", [&](auto o) {
      CMBL_LAUNCH(c, K_PL, (k_pl_combine<T, decltype(o)::value>), fgrid(), 0, c->stream, G, r, c->lx_r.template as<T>(), c->ly.template as<T>(), dx, c->Nx, c->plane(), S);
    });
  }
  void premul(int n, const T* g, T* W, int S) {
    const bool v = vec({g, W});
    by_order<1>(n, "PowerLens", [&](auto o) {
      constexpr int N = decltype(o)::value;
      if (v) CMBL_LAUNCH(c, K_PL, (k_pl_premul<T, N, V>), pgrid(V), 0, c->stream, (const cx<T>*)u.as<cx<T>>(), g, W, coef(N), c->npix(), S);
      else CMBL_LAUNCH(c, K_PL, (k_pl_premul<T, N, 1>), pgrid(1), 0, c->stream, (const cx<T>*)u.as<cx<T>>(), g, W, coef(N), c->npix(), S);
    });
  }
  // out = base + the terms of total order n (n = 0: Taylens' permutation of base alone)
  void accum(int n, const T* D, const T* base, T* out, bool gather_base, int S) {
    const cx<T>* uu = u.as<cx<T>>(); const unsigned* sp = src.as<unsigned>();
    const long np = c->npix();
    if (taylens)
      return by_order<0>(n, "Taylens", [&](auto o) {
        CMBL_LAUNCH(c, K_PL, (k_pl_accum<T, decltype(o)::value, true, 1>), pgrid(1), 0, c->stream, uu, sp, D, base, out, coef(decltype(o)::value), gather_base ? 1 : 0, np, S);
      });
    const bool v = vec({D, base, out});
    by_order<1>(n, "PowerLens", [&](auto o) {
      constexpr int N = decltype(o)::value;
      if (v) CMBL_LAUNCH(c, K_PL, (k_pl_accum<T, N, false, V>), pgrid(V), 0, c->stream, uu, sp, D, base, out, coef(N), 0, np, S);
      else CMBL_LAUNCH(c, K_PL, (k_pl_accum<T, N, false, 1>), pgrid(1), 0, c->stream, uu, sp, D, base, out, coef(N), 0, np, S);
    });
  }

  void apply(int mode, int bi, const void* in, int bo, void* out, int P, int B) override {
    CMBL_REQUIRE(mode == F_FWD || mode == F_ADJ, ERR_ARG, "PowerLens / Taylens: the reference defines no inverse (src/powerlens.jl, src/taylens.jl): mode must be CMBL_FLOW_FWD or CMBL_FLOW_ADJ");
    CMBL_REQUIRE(!(taylens && mode == F_ADJ), ERR_ARG, "Taylens: the reference defines no adjoint (src/taylens.jl:51 is its only action)");
    CMBL_REQUIRE(ready, ERR_STATE, "cmbl_powerlens_set_phi / cmbl_powerlens_set_deflection has not been called");
    const int S = P * B;
    const long np = c->npix(), pl = c->plane(), sn = (long)S * np;
    // the loop of :44 is empty: a copy, with no transform where both sides are Fourier
    if (order == 0 && !taylens && mode == F_FWD) return c->convert(bi, in, bo, out, P, B, fF);
    // every buffer before the first launch: growing one frees it
    fF.ensure(sizeof(cx<T>) * S * pl);
    if (order > 0) { dF.ensure(sizeof(cx<T>) * (order + 1) * S * pl); dmaps.ensure(sizeof(T) * (order + 1) * sn); if (!c->generic) c->mixed_scratch((long)(order + 1) * S); }
    if (bi != B_MAP) inm.ensure(sizeof(T) * sn);
    outm.ensure(sizeof(T) * sn);
    cx<T>* F = fF.as<cx<T>>();
    // the argument as maps AND as QU Fourier planes: both sums need both (as_maps leaves the planes in fF)
    if (bi == B_MAP && (order > 0 || mode == F_ADJ)) c->to_F(bi, in, F, B_FOURIER, P, B);
    const T* fm = c->as_maps(bi, in, fF, inm, P, B);
    if (mode == F_ADJ) {                                                    // r = Ð(g) + ...  (src/powerlens.jl:54-57)
      for (int n = 1; n <= order; ++n) {
        premul(n, fm, dmaps.as<T>(), S);
        c->rfft2_F(dmaps.as<T>(), dF.as<cx<T>>(), (long)(n + 1) * S);
        combine(n, dF.as<cx<T>>(), F, S);
      }
      c->from_F(F, B_FOURIER, bo, out, P, B);
      return;
    }
    T* dst = c->map_dst(bo, out, fm, outm, S);                              // Taylens gathers from the argument
    if (order == 0) accum(0, nullptr, fm, dst, true, S);                    // Taylens(0): the loop of src/taylens.jl:62 is empty, the permutation stays
    for (int n = 1; n <= order; ++n) {
      mult(n, F, dF.as<cx<T>>(), S);
      c->F_to_map(dF.as<cx<T>>(), dmaps.as<T>(), (long)(n + 1) * S);
      accum(n, dmaps.as<T>(), n == 1 ? fm : dst, dst, n == 1, S);
    }
    c->map_finish(dst, bo, out, fF, P, B);
  }

  // ---- LensOps<T> (a PowerLens / Taylens in the L slot of a data set): the composition from the launches above, no kernel of its own ----
  const char* op_name() const override { return taylens ? "Taylens" : "PowerLens"; }
  void op_check(int) const override { CMBL_REQUIRE(ready, ERR_STATE, "cmbl_powerlens_set_phi / cmbl_powerlens_set_deflection has not been called"); }
  void op_set_phi(int basis, const void* phi, int nb) override { set_phi(basis, phi, nb); }
  void op_lens(const T* in, T* out, int P, int B) override { apply(F_FWD, B_MAP, in, B_MAP, out, P, B); }
  DevBuf opm;
  void op_lens_F(T* in, T* ftil, cx<T>* F, int P, int B) override {
    if (!ftil) { opm.ensure(sizeof(T) * P * B * c->npix()); ftil = opm.as<T>(); }
    op_lens(in, ftil, P, B);
    c->rfft2_F(ftil, F, (long)P * B);
  }
  bool op_has_adjoint() const override { return !taylens; }
  // r = Ð(g) + Σ_n ... (src/powerlens.jl:54-57) with g given as QU Fourier planes: the sum is accumulated onto them
  void op_adj_F(const cx<T>* in, cx<T>* out, int P, int B) override {
    CMBL_REQUIRE(!taylens, ERR_ARG, "Taylens: the reference defines no adjoint (src/taylens.jl:51 is its only action)");
    op_check(B);
    const int S = P * B;
    const long np = c->npix(), pl = c->plane();
    opm.ensure(sizeof(T) * S * np);
    if (order > 0) { dF.ensure(sizeof(cx<T>) * (order + 1) * S * pl); dmaps.ensure(sizeof(T) * (order + 1) * S * np); if (!c->generic) c->mixed_scratch((long)(order + 1) * S); }
    if (in != out) CMBL_HIP(hipMemcpyAsync(out, in, sizeof(cx<T>) * S * pl, hipMemcpyDeviceToDevice, c->stream));
    c->F_to_map(out, opm.as<T>(), S);
    for (int n = 1; n <= order; ++n) {
      premul(n, opm.as<T>(), dmaps.as<T>(), S);
      c->rfft2_F(dmaps.as<T>(), dF.as<cx<T>>(), (long)(n + 1) * S);
      combine(n, dF.as<cx<T>>(), out, S);
    }
  }
};

}  // namespace cmbl
