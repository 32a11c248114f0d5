// Host side of cmbl_bilinear_*: BilinearLens (src/bilinearlens.jl) and its gmres (src/numerical_algorithms.jl:193-214) on the device.
// One ϕ (a batched ϕ is refused like the reference's, :40), any number of (pol, batch) slices of f.  Per ϕ: the table of L (kernels_bilinear.hpp)
// at once; the CSR of L', the table of BilinearLens(-ϕ) and its CSR lazily, on first use, kept until ϕ changes (:92-97).  Every launch goes to
// the context's stream and nothing but set_phi's norm(ϕ) == 0 test synchronises: the Hessenberg entries of the Arnoldi process stay on the device.
//
// gmres as written builds K = [Pl b, (Pl A) Pl b, ...], α = argmin |K[:, 2:n+1] α - K[:, 1]|, x = K[:, 1:n] α: GMRES(n) from x0 = 0 on
// (Pl A) x = Pl b in exact arithmetic.  cond(K[:, 2:n+1]) is ~1e4 at 0.7 px rms, so the same minimiser is formed by Arnoldi with modified
// Gram-Schmidt: per-slice dots reduced in a fixed order in double (block_sum + k_reduce_final<SUM_FLOAT64>), the (n+1) x n least-squares problem
// solved by Givens rotations in one thread per slice, and a clean stop on breakdown (Pl A = I: the reference's QR would meet a rank-deficient K).
#pragma once
#include <limits>
#include "engine.hpp"
#include "kernels_bilinear.hpp"

namespace cmbl {

// the table of one operator and, once asked for, the CSR of its transpose
struct BlTab { DevBuf base, fr, rowstart, col, val; bool rows = false, csr = false; };

struct BilinearApi {                         // what the C ABI (api.hip) holds of a BilinearLens (see FlowApi in engine.hpp)
  virtual ~BilinearApi() = default;
  virtual void set_phi(int basis, const void* phi, int nb) = 0;
  virtual void set_deflection(const void* dy_px, const void* dx_px) = 0;
  virtual void apply(int mode, int bi, const void* in, int bo, void* out, int P, int B, int maxiter) = 0;
  virtual void grad(const void* f_lensed, int bdel, const void* delta, void* dphi, int bdf, void* df, int P, int B) = 0;
};

template <typename T>
struct Bilinear : BilinearApi, LensOps<T> {
  Ctx<T>* c;
  bool ready = false, identity = false;
  T div = 1;                                 // the deflection maps are divided by this (Δx for ∇ϕ, 1 for pixel-unit maps)
  DevBuf defl;                               // [2][npix]: x then y component
  BlTab fwd, anti;
  DevBuf cnt, blk, flag, phiF, gF;           // set-up scratch
  DevBuf inm, outm, cvt;                     // boundary scratch (Ctx::as_maps / map_dst / map_finish): argument maps, result maps, F planes
  DevBuf Q, tmp, H, y, part;                 // GMRES: the orthonormal basis [m+1][S][npix], A q, Hessenberg entries, coefficients, partial sums
  DevBuf gmaps, vmaps, vF, dF;               // pullback scratch
  static constexpr int RED = 256;

  explicit Bilinear(Ctx<T>* ctx) : c(ctx) {}
  Bilinear(const Bilinear&) = delete;
  Bilinear& operator=(const Bilinear&) = delete;

  unsigned pgrid() const { return nblocks(c->npix()); }
  void reset() { fwd.rows = fwd.csr = anti.rows = anti.csr = false; }

  void rows(BlTab& t, T sign) {
    if (t.rows) return;
    const long np = c->npix();
    t.base.ensure(sizeof(unsigned) * np); t.fr.ensure(sizeof(cx<T>) * np);
    CMBL_LAUNCH(c, K_BL, (k_bl_rows<T>), dim3(pgrid()), 0, c->stream, defl.as<T>() + np, defl.as<T>(), div, sign, t.base.as<unsigned>(), t.fr.as<cx<T>>(), c->Ny, c->Nx);
    t.rows = true;
  }
  void csr(BlTab& t) {
    if (t.csr) return;
    const long np = c->npix();
    const int nblk = (int)((np + BL_SCAN - 1) / BL_SCAN);
    t.rowstart.ensure(sizeof(unsigned) * (np + 1)); t.col.ensure(sizeof(unsigned) * 4 * np); t.val.ensure(sizeof(T) * 4 * np);
    cnt.ensure(sizeof(unsigned) * np); blk.ensure(sizeof(unsigned) * nblk);
    unsigned* n = cnt.as<unsigned>(); unsigned* rs = t.rowstart.as<unsigned>();
    CMBL_HIP(hipMemsetAsync(n, 0, sizeof(unsigned) * np, c->stream));
    CMBL_LAUNCH(c, K_BL, k_bl_count, dim3(pgrid()), 0, c->stream, t.base.as<unsigned>(), n, c->Ny, c->Nx);
    CMBL_LAUNCH(c, K_BL, k_bl_scan1, dim3((unsigned)nblk), 0, c->stream, n, rs, blk.as<unsigned>(), np);
    CMBL_LAUNCH(c, K_BL, k_bl_scan2, dim3(1), 0, c->stream, blk.as<unsigned>(), nblk);
    CMBL_LAUNCH(c, K_BL, k_bl_scan3, dim3(pgrid()), 0, c->stream, rs, blk.as<unsigned>(), np, (unsigned)(4 * np));
    CMBL_HIP(hipMemsetAsync(n, 0, sizeof(unsigned) * np, c->stream));
    CMBL_LAUNCH(c, K_BL, k_bl_fill, dim3(pgrid()), 0, c->stream, t.base.as<unsigned>(), rs, n, t.col.as<unsigned>(), c->Ny, c->Nx);
    CMBL_LAUNCH(c, K_BL, (k_bl_sort<T>), dim3(pgrid()), 0, c->stream, rs, t.col.as<unsigned>(), t.val.as<T>(), t.fr.as<cx<T>>(), np);
    t.csr = true;
  }
  BlTab& table(bool antilens, bool transposed) {
    BlTab& t = antilens ? anti : fwd;
    rows(t, antilens ? (T)-1 : (T)1);
    if (transposed) csr(t);
    return t;
  }
  // out = L in or L' in over S slices (in != out)
  void mul(bool antilens, bool transposed, const T* in, T* out, int S) {
    BlTab& t = table(antilens, transposed);
    if (transposed) CMBL_LAUNCH(c, K_BL, (k_bl_csr<T>), dim3(pgrid()), 0, c->stream, t.rowstart.as<unsigned>(), t.col.as<unsigned>(), t.val.as<T>(), in, out, c->npix(), S);
    else CMBL_LAUNCH(c, K_BL, (k_bl_gather<T>), dim3(pgrid()), 0, c->stream, t.base.as<unsigned>(), t.fr.as<cx<T>>(), in, out, c->Ny, c->Nx, S);
  }

  void set_phi(int basis, const void* phi, int nb) override {
    CMBL_REQUIRE(nb == 1, ERR_SHAPE, "BilinearLens with batched phi is not implemented (src/bilinearlens.jl:40)");
    const long n = basis == B_MAP ? c->npix() : 2 * c->plane();
    flag.ensure(sizeof(int));
    CMBL_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), c->stream));
    CMBL_LAUNCH(c, K_BL, (k_bl_anynz<T>), dim3(std::min(nblocks(n), 1024u)), 0, c->stream, (const T*)phi, n, flag.as<int>());
    int nz = 0;
    CMBL_HIP(hipMemcpyAsync(&nz, flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    CMBL_HIP(hipStreamSynchronize(c->stream));
    reset();
    identity = nz == 0;                                                     // norm(ϕ) == 0 (:34)
    ready = true;
    if (identity) return;
    c->deflection_maps(basis, phi, phiF, gF, defl, K_BL);
    div = c->dx();
    rows(fwd, (T)1);
  }
  void set_deflection(const void* dy_px, const void* dx_px) override {
    c->deflection_maps(dy_px, dx_px, defl);
    div = 1;
    reset();
    identity = false; ready = true;
    rows(fwd, (T)1);
  }

  // <w, qdot> (qdot null: <w, w>) of every slice -> out[S] (device doubles), after w -= hprev qprev when qprev is given
  void mgs(T* w, const T* qprev, const double* hprev, const T* qdot, double* out, int S) {
    const long np = c->npix();
    const unsigned nblk = std::min(nblocks(np), (unsigned)RED);
    CMBL_LAUNCH(c, K_BL, (k_bl_mgs<T>), dim3(nblk, (unsigned)S), 0, c->stream, w, qprev, hprev, qdot, part.as<double>(), np);
    CMBL_LAUNCH(c, K_REDUCE, (k_reduce_final<T, SUM_FLOAT64>), dim3((unsigned)S), 0, c->stream, part.as<double>(), out, (int)nblk, 1.0);
  }
  // x = gmres(A, b; Pl, maxiter = m) per slice with A = L (or L'), Pl = BilinearLens(-ϕ) (or its transpose)  (:127-151)
  void solve(bool transposed, const T* b, T* x, int m, int S) {
    const long np = c->npix(), sn = (long)S * np;
    Q.ensure(sizeof(T) * (m + 1) * sn); tmp.ensure(sizeof(T) * sn);
    H.ensure(sizeof(double) * ((long)(m + 1) * m + 1) * S); y.ensure(sizeof(double) * (long)m * S); part.ensure(sizeof(double) * (long)RED * S);
    T* q = Q.as<T>(); double* h = H.as<double>();
    auto slot = [&](int j, int k) { return h + ((long)j * m + k) * S; };
    // a direction whose norm is below 16 eps of its column's is rounding noise of the orthogonalisation
    const double thr = 16.0 * (double)std::numeric_limits<T>::epsilon(), thr2 = thr * thr;
    const dim3 sg(std::min(pgrid(), 1024u), (unsigned)S);
    mul(true, transposed, b, q, S);                                         // K1 = Pl b
    mgs(q, nullptr, nullptr, nullptr, slot(m + 1, 0), S);                   // beta^2
    CMBL_LAUNCH(c, K_BL, (k_bl_scale<T>), sg, 0, c->stream, q, (const double*)slot(m + 1, 0), (const double*)h, 0L, 0, thr2, np);
    for (int k = 0; k < m; ++k) {
      T* w = q + (long)(k + 1) * sn;
      mul(false, transposed, q + (long)k * sn, tmp.as<T>(), S);             // w = Pl A q_k
      mul(true, transposed, tmp.as<T>(), w, S);
      mgs(w, nullptr, nullptr, q, slot(0, k), S);
      for (int j = 1; j <= k; ++j) mgs(w, q + (long)(j - 1) * sn, slot(j - 1, k), q + (long)j * sn, slot(j, k), S);
      mgs(w, q + (long)k * sn, slot(k, k), nullptr, slot(k + 1, k), S);     // the last update carries |w|^2
      CMBL_LAUNCH(c, K_BL, (k_bl_scale<T>), sg, 0, c->stream, w, (const double*)slot(k + 1, k), (const double*)slot(0, k), (long)m * S, k + 1, thr2, np);
    }
    CMBL_LAUNCH_NT(c, K_BL, 64, k_bl_lsq, dim3((unsigned)((S + 63) / 64)), 0, c->stream, (const double*)h, y.as<double>(), m, S, thr2);
    CMBL_LAUNCH(c, K_BL, (k_bl_combine<T>), sg, 0, c->stream, (const T*)q, (const double*)y.as<double>(), x, m, S, np);
  }

  void check_ready() const { CMBL_REQUIRE(ready, ERR_STATE, "cmbl_bilinear_set_phi / cmbl_bilinear_set_deflection has not been called"); }

  void apply(int mode, int bi, const void* in, int bo, void* out, int P, int B, int maxiter) override {
    check_ready();
    if (identity) return c->convert(bi, in, bo, out, P, B, cvt);            // sparse_repr === I && return f (:108, 118, 128, 141)
    const int S = P * B;
    const T* src = c->as_maps(bi, in, cvt, inm, P, B);
    T* dst = c->map_dst(bo, out, src, outm, S);                             // the gathers cannot run in place
    if (mode == F_FWD) mul(false, false, src, dst, S);
    else if (mode == F_ADJ) mul(false, true, src, dst, S);
    else solve(mode == F_INVADJ, src, dst, maxiter, S);
    c->map_finish(dst, bo, out, cvt, P, B);
  }

  // δϕ of the pullback of L*f (:165-171): ∇'·(Σ_pol Ł(Δ) Ł(∇f̃)), a Fourier plane per batch slot, F layout, to dF
  void grad_phi(const T* f_lensed, const T* dm, int P, int B) {
    const int S = P * B;
    const long np = c->npix(), pl = c->plane();
    // ∇f̃ in Fourier space (the reference's choice), back to maps
    vF.ensure(sizeof(cx<T>) * 3 * S * pl); gmaps.ensure(sizeof(T) * 2 * S * np); vmaps.ensure(sizeof(T) * 2 * B * np); dF.ensure(sizeof(cx<T>) * B * pl);
    cx<T>* F = vF.as<cx<T>>(); cx<T>* G = F + (long)S * pl;
    const dim3 fg(nblocks(pl));
    c->rfft2_F(f_lensed, F, S);
    CMBL_LAUNCH(c, K_BL, (k_bl_gradmult<T>), fg, 0, c->stream, (const cx<T>*)F, G, c->lx_r.template as<T>(), c->ly.template as<T>(), c->Nx, pl, S);
    c->F_to_map(G, gmaps.as<T>(), 2L * S);
    CMBL_LAUNCH(c, K_BL, (k_bl_polsum<T>), dim3(std::min(pgrid(), 1024u), (unsigned)B), 0, c->stream, dm, (const T*)gmaps.as<T>(),
                vmaps.as<T>(), np, P, B);
    c->rfft2_F(vmaps.as<T>(), F, 2L * B);
    CMBL_LAUNCH(c, K_BL, (k_bl_div<T>), fg, 0, c->stream, (const cx<T>*)F, dF.as<cx<T>>(), c->lx_r.template as<T>(), c->ly.template as<T>(), c->Nx, pl, B);
  }
  // pullback of L*f (:165-171): δf = L'Δ in `bdf`; δϕ in the ABI layout
  void grad(const void* f_lensed, int bdel, const void* delta, void* dphi, int bdf, void* df, int P, int B) override {
    check_ready();
    const int S = P * B;
    const T* dm = c->as_maps(bdel, delta, cvt, inm, P, B);
    grad_phi((const T*)f_lensed, dm, P, B);
    c->F2ref(dF.as<cx<T>>(), (cx<T>*)dphi, B);
    // δf = B(Lϕ' * Δ)
    if (identity) return c->convert(B_MAP, dm, bdf, df, P, B, cvt);
    T* dst = c->map_dst(bdf, df, dm, outm, S);
    mul(false, true, dm, dst, S);
    c->map_finish(dst, bdf, df, cvt, P, B);
  }

  // ---- LensOps<T> (a BilinearLens in the L slot of a data set, src/dataset.jl:223) ----------------------------------------------------
  // Power-of-two maps with the option "lens_fused": the gather (the row sum over the CSR of L') runs inside the column pass of the transform
  // that follows it, Ctx::y_lens -- one launch instead of gather, map to HBM, y_r2c.  Any other size: the composition.
  bool lens_fused() const { return !c->generic && c->opts.lens_fused && !identity; }
  LensTab<T> tab(bool transposed) {
    BlTab& t = table(false, transposed);
    return LensTab<T>{t.base.as<unsigned>(), t.fr.as<cx<T>>(), t.rowstart.as<unsigned>(), t.col.as<unsigned>(), t.val.as<T>()};
  }
  // F = rfft2(L m) or rfft2(L' m) of S maps
  void mul_F(bool transposed, const T* m, cx<T>* F, int S) {
    if (lens_fused()) {
      const LensTab<T> t = tab(transposed);
      cx<T>* mx = c->mixed_scratch(S);
      c->y_lens(transposed, t, m, mx, S);
      c->template x_pass<0>(mx, F, S);
      return;
    }
    if (identity) return c->rfft2_F(m, F, S);
    outm.ensure(sizeof(T) * S * c->npix());
    mul(false, transposed, m, outm.as<T>(), S);
    c->rfft2_F(outm.as<T>(), F, S);
  }
  const char* op_name() const override { return "BilinearLens"; }
  void op_check(int) const override { check_ready(); }
  void op_set_phi(int basis, const void* phi, int nb) override { set_phi(basis, phi, nb); }
  void op_lens(const T* in, T* out, int P, int B) override {
    check_ready();
    if (identity) return c->copy_maps(in, out, (long)P * B);
    mul(false, false, in, out, P * B);
  }
  void op_lens_F(T* in, T* ftil, cx<T>* F, int P, int B) override {
    check_ready();
    if (!ftil) return mul_F(false, in, F, P * B);
    op_lens(in, ftil, P, B);
    c->rfft2_F(ftil, F, (long)P * B);
  }
  bool op_has_adjoint() const override { return true; }
  void op_adj_F(const cx<T>* in, cx<T>* out, int P, int B) override {
    check_ready();
    inm.ensure(sizeof(T) * P * B * c->npix());
    c->F_to_map(in, inm.as<T>(), (long)P * B);
    mul_F(true, inm.as<T>(), out, P * B);
  }
  bool op_has_pullback() const override { return true; }
  void op_pullback(T* ftil, cx<T>* w, cx<T>* dphi, int P, int B, bool) override {
    check_ready();
    inm.ensure(sizeof(T) * P * B * c->npix());
    c->F_to_map(w, inm.as<T>(), (long)P * B);
    grad_phi(ftil, inm.as<T>(), P, B);
    CMBL_HIP(hipMemcpyAsync(dphi, dF.p, sizeof(cx<T>) * B * c->plane(), hipMemcpyDeviceToDevice, c->stream));
    mul_F(true, inm.as<T>(), w, P * B);
  }
  bool op_has_inverse() const override { return true; }
  void op_inv(const T* in, T* out, int P, int B) override {
    check_ready();
    if (identity) return c->copy_maps(in, out, (long)P * B);
    solve(false, in, out, 5, P * B);
  }
};

}  // namespace cmbl
