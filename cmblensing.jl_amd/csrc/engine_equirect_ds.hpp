// Host side of cmbl_eqds_* and cmbl_equirect_field_dot: NoLensingDataSet (src/dataset.jl:37-47, 68-80) on ProjEquiRect,
//   d = M B f + noise,  f ~ N(0, Cf),  noise ~ N(0, Cn),
// with Cf^-1, B, the preconditioner (and Cn^-1 in its block form) BlockDiagEquiRect operators, M (and Cn^-1 in its pixel form) map-diagonal.  The
// reference's argmaxf_logpdf (src/maximization.jl:17-42) starts from zero(diag(ds.Cf)), and the reference defines no diag(::BlockDiagEquiRect): what
// runs here is its algorithm (conjugate_gradient, src/numerical_algorithms.jl:73-134) on its operators, with the zero field of Cf's basis.
//
// Fields are AZFOURIER arrays, data are MAP arrays (the mask and the pixel noise live there).  The CG vectors stay in the Az basis; their dot products
// are the map dot (src/proj_equirect.jl:355) formed there (kernels_equirect_ds.hpp has the weights).  PRECONDITION of every entry point: each block
// operator maps images of maps to images of maps -- spin-0 blocks are real at columns 0 and Nx/2, spin-2 blocks there commute with v -> S conj(v),
// S the swap of the two halves.  Cℓ_to_Cov and Cℓ_to_Beam produce such blocks; the Python constructor checks the two columns.
//
// One CG iteration with Cn map-diagonal (the launches, all on the context's stream, no host synchronisation):
//   t = B p                                  k_eqds_apply2                    |B|
//   t -> map, map *= W, map -> t             equirect_convert, k_eqds_pix, equirect_convert       (W = M Cn^-1 M, precombined)
//   Ap = Cf^-1 p + B' t, partials of p'Ap    k_eqds_apply2                    |Cf^-1| + |B|
//   p'Ap ; alpha                             k_eqds_dot_fin, k_cg_alpha
//   x += alpha p, r -= alpha Ap              k_cg_xr
//   z = P^-1 r, partials of r'z              k_eqds_apply2                    |P^-1|
//   r'z ; beta, history, stop and best flags k_eqds_dot_fin, k_cg_beta
//   p = z + beta p ; bestx = x if better     k_cg_p, k_cg_keep_best
// Cn block-diagonal: the middle line becomes  -> map, *= M, -> Az, Cn^-1 (k_eqds_apply2, |Cn^-1|), -> map, *= M, -> Az.  The loop, with its scalars, history and
// flags on the device, is CgSolver<T>::solve (engine_cg.hpp, shared with the flat-sky solver): this file forms b and supplies A p (hess) and z = P^-1 r (apply1) with their dots.
#pragma once
#include "engine.hpp"
#include "engine_equirect.hpp"
#include "engine_dataset.hpp"
#include "eqds_host.hpp"
#include "kernels_equirect_ds.hpp"

namespace cmbl {

struct EqDatasetApi {                      // what the C ABI (api.hip) holds of such a data set: precision-free, pointers untyped
  double logdet_sum = 0;
  virtual ~EqDatasetApi() = default;
  virtual void set_block_op(int which, const void* blocks, bool cplx, int n) = 0;
  virtual void set_pixel_op(int which, const void* map, int nplanes) = 0;
  virtual void mean(const void* f, void* d_out, int B) = 0;
  virtual void gradientf(const void* f, const void* d, void* out, int B) = 0;
  virtual void logpdf(const void* f, const void* d, double* lp, int B) = 0;
  virtual int wiener_cg(const void* d, const void* fstart, double tol, int maxit, void* f_out, double* hist, int B) = 0;
};

// per-slot dots of two fields in either basis, left on the device at out_dev[0 .. B).  wgt: a diagonal weight between two MAPS (wplanes = 1 or npol), or nullptr
template <typename T> void equirect_dot_dev(Ctx<T>* c, DevBuf& parts, int basis, const void* a, const void* b, const T* wgt, int wplanes, int npol, int B, double* out_dev) {
  const int Mh = c->Nx / 2 + 1, n = npol * c->Ny;
  const long len = basis == B_MAP ? c->npix() * npol : (long)n * Mh;
  const unsigned nb = (unsigned)std::min<long>((len + NTP - 1) / NTP, 256);
  parts.ensure(sizeof(double) * (size_t)nb * B);
  double* part = parts.template as<double>();
  if (basis == B_MAP) CMBL_LAUNCH(c, K_REDUCE, (k_eqds_dot_part<T, false>), dim3(nb, (unsigned)B), 0, c->stream, a, b, wgt, wplanes, part, len, n, c->Nx, npol == 2, c->npix());
  else CMBL_LAUNCH(c, K_REDUCE, (k_eqds_dot_part<T, true>), dim3(nb, (unsigned)B), 0, c->stream, a, b, wgt, wplanes, part, len, n, c->Nx, npol == 2, c->npix());
  CMBL_LAUNCH(c, K_REDUCE, k_eqds_dot_fin, dim3((unsigned)B), 0, c->stream, (const double*)part, (long)nb, out_dev);
}
// cmbl_equirect_field_dot: out_host[b] = dot(a_b, b_b) (src/proj_equirect.jl:355) of MAP arrays, or of AZFOURIER arrays that are images of maps
template <typename T> void equirect_field_dot(Ctx<T>* c, int basis, const void* a, const void* b, int npol, int B, double* out_host) {
  DevBuf parts, res;
  res.ensure(sizeof(double) * B);
  equirect_dot_dev<T>(c, parts, basis, a, b, nullptr, 0, npol, B, res.template as<double>());
  CMBL_HIP(hipMemcpyAsync(out_host, res.p, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
  CMBL_HIP(hipStreamSynchronize(c->stream));
}

template <typename T>
struct EqDataset : EqDatasetApi {
  Ctx<T>* c;
  EqdsBook bk;
  DevBuf pix[EQDS_NPIXOP], Wb, MCb;        // owned copies of the map-diagonal planes; W = M Cn^-1 M and M Cn^-1 (pixel form of Cn)
  DevBuf t1, t2, mp, parts, q2;            // scratch, grown on demand
  CgSolver<T> cg;                          // the CG vectors, scalars, flags and loop (engine_cg.hpp)

  EqDataset(Ctx<T>* ctx, int npol) : c(ctx), cg(ctx) { std::string m; const int rc = bk.init(ctx->Ny, ctx->Nx, npol, m); if (rc) fail(rc, m); }
  int P() const { return bk.P; }
  int n() const { return bk.n(); }
  int Mh() const { return c->Nx / 2 + 1; }
  long azsize(int B) const { return (long)n() * Mh() * B; }               // complex elements of a batch of fields
  long mapsize(int B) const { return c->npix() * P() * B; }
  void require(int B, bool need_cn, bool need_precond) const { std::string m; const int rc = bk.check(B, need_cn, need_precond, m); if (rc) fail(rc, m); }

  void set_block_op(int which, const void* blocks, bool cplx, int n_) override { std::string m; const int rc = bk.set_block(which, blocks, cplx, n_, m); if (rc) fail(rc, m); }
  void set_pixel_op(int which, const void* map, int nplanes) override {
    std::string m; const int rc = bk.set_pixel(which, map == nullptr, nplanes, m); if (rc) fail(rc, m);
    if (!map) return;
    pix[which].ensure(sizeof(T) * nplanes * c->npix());
    CMBL_HIP(hipMemcpyAsync(pix[which].p, map, sizeof(T) * nplanes * c->npix(), hipMemcpyDeviceToDevice, c->stream));
  }
  const T* mask() const { return bk.pix_planes[EQDS_MASK] ? pix[EQDS_MASK].template as<T>() : nullptr; }
  int mask_planes() const { return bk.pix_planes[EQDS_MASK]; }
  // W and M Cn^-1 of the pixel form, rebuilt after a map-diagonal operator changed
  int wplanes() const { return std::max(bk.pix_planes[EQDS_MASK], bk.pix_planes[EQDS_CN_INV_PIX]); }
  void weights() {
    if (!bk.dirty || !bk.cn_pix()) return;
    const long total = (long)wplanes() * c->npix();
    Wb.ensure(sizeof(T) * total); MCb.ensure(sizeof(T) * total);
    CMBL_LAUNCH(c, K_EQ_POINT, (k_eqds_wcomb<T>), dim3(eq_grid(total)), 0, c->stream, Wb.template as<T>(), MCb.template as<T>(), mask(), mask_planes(),
                (const T*)pix[EQDS_CN_INV_PIX].template as<T>(), bk.pix_planes[EQDS_CN_INV_PIX], c->npix(), total);
    bk.dirty = false;
  }

  // ---- launches
  // out = sa A x + sc C y (C == nullptr, y != nullptr: + sc y); dot_out != nullptr: dot_out[b] = dot(dotv, out) on the device
  // the forms an evaluation uses: one operator plain or adjoint, or a plain one plus an adjoint one
  template <bool CA, bool ADJA, bool CC, bool ADJC, bool TWO> void apply2_bc(const EqdsArgs<T>& a, int B) {
    const dim3 grid((unsigned)((a.n + EQ_TP - 1) / EQ_TP), (unsigned)a.Mh);
    if (B == 1) CMBL_LAUNCH(c, K_EQ_APPLY, (k_eqds_apply2<T, CA, ADJA, CC, ADJC, TWO, 1>), grid, 0, c->stream, a);
    else if (B <= 4) CMBL_LAUNCH(c, K_EQ_APPLY, (k_eqds_apply2<T, CA, ADJA, CC, ADJC, TWO, 4>), grid, 0, c->stream, a);
    else CMBL_LAUNCH(c, K_EQ_APPLY, (k_eqds_apply2<T, CA, ADJA, CC, ADJC, TWO, 8>), grid, 0, c->stream, a);
  }
  void apply2(int opA, bool adjA, T sa, const cx<T>* x, int opC, bool adjC, T sc, const cx<T>* y, cx<T>* out, const cx<T>* dotv, double* dot_out, int B) {
    EqdsArgs<T> a{};
    a.A = bk.blk[opA].p; a.x = x; a.sa = sa;
    a.C = opC >= 0 ? bk.blk[opC].p : nullptr; a.y = y; a.sc = sc;
    a.out = out; a.dotv = dotv; a.n = n(); a.Mh = Mh(); a.Nx = c->Nx; a.spin2 = P() == 2; a.nbatch = B;
    const long nper = (long)a.Mh * ((a.n + EQ_TP - 1) / EQ_TP);
    if (dot_out) { parts.ensure(sizeof(double) * (size_t)nper * B); a.part = parts.template as<double>(); }
    const bool ca = bk.blk[opA].cplx, cc = opC >= 0 && bk.blk[opC].cplx;
    if (opC < 0) {
      if (adjA) { if (ca) apply2_bc<true, true, false, false, false>(a, B); else apply2_bc<false, true, false, false, false>(a, B); }
      else { if (ca) apply2_bc<true, false, false, false, false>(a, B); else apply2_bc<false, false, false, false, false>(a, B); }
    } else {
      CMBL_REQUIRE(!adjA && adjC, ERR_ARG, "eqds: the two-operator apply is compiled for a plain first and an adjoint second operand");
      if (ca) { if (cc) apply2_bc<true, false, true, true, true>(a, B); else apply2_bc<true, false, false, true, true>(a, B); }
      else { if (cc) apply2_bc<false, false, true, true, true>(a, B); else apply2_bc<false, false, false, true, true>(a, B); }
    }
    if (dot_out) CMBL_LAUNCH(c, K_REDUCE, k_eqds_dot_fin, dim3((unsigned)B), 0, c->stream, (const double*)a.part, nper, dot_out);
  }
  void apply1(int op, bool adj, T s, const cx<T>* x, cx<T>* out, const cx<T>* dotv, double* dot_out, int B) { apply2(op, adj, s, x, -1, false, T(0), nullptr, out, dotv, dot_out, B); }
  void to_map(const cx<T>* az, T* map, int B) { equirect_convert<T>(c, B_AZFOURIER, az, B_MAP, map, P(), B); }
  void to_az(const T* map, cx<T>* az, int B) { equirect_convert<T>(c, B_MAP, map, B_AZFOURIER, az, P(), B); }
  void pixop(T* out, const T* in, const T* d, const T* wa, int npa, const T* wb, int npb, T sgn, int B) {
    const long total = mapsize(B);
    CMBL_LAUNCH(c, K_EQ_POINT, (k_eqds_pix<T>), dim3(eq_grid(total)), 0, c->stream, out, in, d, wa, npa, wb, npb, sgn, P(), c->npix(), total);
  }
  void copy_az(cx<T>* dst, const cx<T>* src, int B) { CMBL_HIP(hipMemcpyAsync(dst, src, sizeof(cx<T>) * azsize(B), hipMemcpyDeviceToDevice, c->stream)); }
  void scratch(int B) {
    t1.ensure(sizeof(cx<T>) * azsize(B)); t2.ensure(sizeof(cx<T>) * azsize(B)); mp.ensure(sizeof(T) * mapsize(B));
    q2.ensure(sizeof(double) * 2 * MAXBATCH);
  }
  // B f as a map (f == nullptr: nothing); returns the map scratch
  T* beamed_map(const cx<T>* f, int B) {
    T* map = mp.template as<T>();
    if (bk.has(EQDS_B)) { apply1(EQDS_B, false, T(1), f, t1.template as<cx<T>>(), nullptr, nullptr, B); to_map(t1.template as<cx<T>>(), map, B); }
    else to_map(f, map, B);
    return map;
  }
  // u (Az) = M' Cn^-1 applied to the residual map in `map` (overwritten): pixel form  map *= M Cn^-1, -> Az;  block form  -> Az, Cn^-1, -> map, *= M, -> Az
  void weigh_back(T* map, cx<T>* u, int B) {
    if (bk.cn_pix()) {
      pixop(map, map, nullptr, MCb.template as<T>(), wplanes(), nullptr, 0, T(1), B);
      to_az(map, u, B);
      return;
    }
    cx<T>* v = t2.template as<cx<T>>();
    to_az(map, u, B);
    apply1(EQDS_CN_INV, false, T(1), u, v, nullptr, nullptr, B);
    to_map(v, map, B);
    if (mask()) pixop(map, map, nullptr, mask(), mask_planes(), nullptr, 0, T(1), B);
    to_az(map, u, B);
  }
  // out = B' u, or u itself without a beam
  void beam_adj(const cx<T>* u, cx<T>* out, int B) {
    if (bk.has(EQDS_B)) apply1(EQDS_B, true, T(1), u, out, nullptr, nullptr, B); else copy_az(out, u, B);
  }
  // Ap = (Cf^-1 + B' M' Cn^-1 M B) p, and dot(p, Ap) when asked for
  void hess(const cx<T>* p, cx<T>* Ap, double* dot_out, int B) {
    T* map = beamed_map(p, B);
    cx<T>* u = t1.template as<cx<T>>();
    if (bk.cn_pix()) { pixop(map, map, nullptr, Wb.template as<T>(), wplanes(), nullptr, 0, T(1), B); to_az(map, u, B); }
    else { if (mask()) pixop(map, map, nullptr, mask(), mask_planes(), nullptr, 0, T(1), B); weigh_back(map, u, B); }
    if (bk.has(EQDS_B)) apply2(EQDS_CF_INV, false, T(1), p, EQDS_B, true, T(1), u, Ap, p, dot_out, B);
    else apply2(EQDS_CF_INV, false, T(1), p, -1, false, T(1), u, Ap, p, dot_out, B);
  }

  // mean = M B f (src/dataset.jl:68-73 without L)
  void mean(const void* f, void* d_out, int B) override {
    require(B, false, false); scratch(B);
    T* map = beamed_map((const cx<T>*)f, B);
    pixop((T*)d_out, map, nullptr, mask(), mask_planes(), nullptr, 0, T(1), B);
  }
  // B' M' Cn^-1 (d - M B f) - Cf^-1 f (src/dataset.jl:76-80 without L); f == nullptr: f = 0, d == nullptr: d = 0
  void gradientf(const void* fv, const void* dv, void* outv, int B) override {
    require(B, true, false); scratch(B); weights();
    const cx<T>* f = (const cx<T>*)fv; const T* d = (const T*)dv; cx<T>* out = (cx<T>*)outv;
    CMBL_REQUIRE(f || d, ERR_ARG, "eqds_gradientf_logpdf with f = 0 and d = 0 is identically zero");
    T* map = mp.template as<T>();
    if (f) { beamed_map(f, B); pixop(map, map, d, mask(), mask_planes(), nullptr, 0, d ? T(1) : T(-1), B); }      // d - M B f, or -(M B f)
    else CMBL_HIP(hipMemcpyAsync(map, d, sizeof(T) * mapsize(B), hipMemcpyDeviceToDevice, c->stream));
    cx<T>* u = t1.template as<cx<T>>();
    weigh_back(map, u, B);
    if (!f) { beam_adj(u, out, B); return; }
    if (bk.has(EQDS_B)) apply2(EQDS_CF_INV, false, T(-1), f, EQDS_B, true, T(1), u, out, nullptr, nullptr, B);
    else apply2(EQDS_CF_INV, false, T(-1), f, -1, false, T(1), u, out, nullptr, nullptr, B);
  }
  // -1/2 [ (d - MBf)' Cn^-1 (d - MBf) + f' Cf^-1 f + logdet_sum ] per slot (src/dataset.jl:59-66); synchronises
  void logpdf(const void* fv, const void* dv, double* lp, int B) override {
    require(B, true, false); scratch(B);
    const cx<T>* f = (const cx<T>*)fv; const T* d = (const T*)dv;
    double* q = q2.template as<double>();
    T* map = beamed_map(f, B);
    pixop(map, map, d, mask(), mask_planes(), nullptr, 0, T(1), B);
    if (bk.cn_pix()) equirect_dot_dev<T>(c, parts, B_MAP, map, map, pix[EQDS_CN_INV_PIX].template as<T>(), bk.pix_planes[EQDS_CN_INV_PIX], P(), B, q);
    else {
      cx<T>* z = t1.template as<cx<T>>();
      to_az(map, z, B);
      apply1(EQDS_CN_INV, false, T(1), z, t2.template as<cx<T>>(), z, q, B);
    }
    apply1(EQDS_CF_INV, false, T(1), f, t2.template as<cx<T>>(), f, q + MAXBATCH, B);
    std::vector<double> h(2 * (size_t)B);
    CMBL_HIP(hipMemcpyAsync(h.data(), q, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
    CMBL_HIP(hipMemcpyAsync(h.data() + B, q + MAXBATCH, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
    CMBL_HIP(hipStreamSynchronize(c->stream));
    for (int b = 0; b < B; ++b) lp[b] = -0.5 * (h[b] + h[B + b] + logdet_sum);
  }

  // conjugate_gradient (CgSolver, engine_cg.hpp) on A = Cf^-1 + B'M'Cn^-1 M B, b = B'M'Cn^-1 d, with the semantics of cmbl_wiener_cg:
  // res = dot(r, z), stop when all(res < tol), the best-res iterate is returned, a NaN residual is ERR_NAN.  Returns the length of the history.
  int wiener_cg(const void* dv, const void* fstart, double tol, int maxit, void* f_out, double* hist, int B) override {
    require(B, true, true); scratch(B); weights();
    const auto v = cg.template begin<CgStateBlock>(azsize(B), B, maxit);
    T* map = mp.template as<T>();                                            // b = B' M' Cn^-1 d
    CMBL_HIP(hipMemcpyAsync(map, dv, sizeof(T) * mapsize(B), hipMemcpyDeviceToDevice, c->stream));
    weigh_back(map, t1.template as<cx<T>>(), B);
    beam_adj(t1.template as<cx<T>>(), v.b, B);
    auto A = [&](const cx<T>* p, cx<T>* Ap, double* pAp) { hess(p, Ap, pAp, B); };
    cg.start(v, (const cx<T>*)fstart, A);
    cg.solve(v, A, [&](const cx<T>* r, cx<T>* z, double* rz) { apply1(EQDS_PRECOND_INV, false, T(1), r, z, r, rz, B); }, tol);
    return cg.template finish<CgStateBlock>(v, (cx<T>*)f_out, hist);
  }
};

}  // namespace cmbl
