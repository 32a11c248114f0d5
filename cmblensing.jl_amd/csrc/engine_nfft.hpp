// Host side of a Projector of method CMBL_PROJECT_NFFT: project(...; method = :fft) (src/proj_healpix.jl:229-236, 254-294, 314-325).
//
// What it computes.  I_N = {-N/2, ..., N/2 - 1}; grid nodes x_g = ((i - Ny/2 - 1) / Ny, (j - Nx/2 - 1) / Nx) at the integer pixels, HEALPix nodes
// x_p by the same formula at the fractional (i_p, j_p) of hpx_idxs_in_patch; K(x) = sum_{l in I_Ny x I_Nx} cos 2 pi l.x.
//   Cartesian -> HEALPix   h_p = 1 / (Ny Nx)  sum_g m_g K(x_g - x_p)   on the patch, exactly 0 elsewhere
//   HEALPix -> Cartesian   m_g = 1 / Npatch   sum_p h_p K(x_p - x_g)
// the real parts of what NFFT.jl's plans approximate; the two are transposes of each other up to Ny Nx / Npatch.  QU / IQU rotate by psi at the
// HEALPix pixel on the way to the sphere and at the Cartesian pixel on the way to the patch, as the bilinear method does.
//
// How.  K depends on differences only, so both node sets are shifted by 1/2: grid nodes at (i - 1) / N, the standard DFT grid, and no phase is
// needed.  The sums are then a type-2 / type-1 NUFFT through a fine grid 2Ny x 2Nx (kernels_nfft.hpp) whose transforms are those of a second
// context `fc` that the projector owns (same device, stream and precision -- the two-context route of ud_grade):
//   to_healpix   rfft2 (c) -> F2ref -> k_nfft_embed -> ref2F -> C2R (fc) -> k_nfft_interp
//   to_cart      k_nfft_spread -> rfft2 (fc) -> F2ref -> k_nfft_extract -> ref2F -> C2R (c) -> k_nfft_rot_cart (QU only)
// The transposes (pullbacks) are the same two pipelines with the rotation moved to the other end and the scales exchanged:
//   to_healpix^T  k_nfft_spread<ROT> -> ... the to_cart pipeline ... -> C2R (c), scale 1 / (Ny Nx), no k_nfft_rot_cart
//   to_cart^T     k_nfft_rot_cart<ADJ> into a scratch copy -> ... the to_healpix pipeline ... -> k_nfft_interp<no rotation>, scale 1 / Npatch
// Both fine grids are real (field and window are real), so every transform is R2C / C2R.  The scales 1 / (Ny Nx) and Ny Nx / Npatch are folded
// into k_nfft_embed / k_nfft_extract together with the 1 / (4 Ny Nx) resp. 1 / (Ny Nx) of the C2R that follows.
// The nodes are fixed per projector: the constructor sorts them once by tile of the fine grid (nfft_bin_nodes, host, stable) and keeps the
// CSR offsets; both node kernels walk them in that order.
#pragma once
#include <algorithm>
#include "engine_healpix.hpp"
#include "kernels_nfft.hpp"

namespace cmbl {

enum { PROJECT_BILINEAR = 0, PROJECT_NFFT = 1 };
constexpr int NFFT_MAXSIDE = 2048;           // the fine grid must be a size the transforms take (4096)

// Gauss-Legendre nodes and weights on [-1, 1] (Newton on P_n)
inline void nfft_gauss_legendre(int n, std::vector<double>& x, std::vector<double>& w) {
  x.assign(n, 0.0); w.assign(n, 0.0);
  for (int i = 0; i < (n + 1) / 2; ++i) {
    double z = std::cos(M_PI * (i + 0.75) / (n + 0.5)), pp = 1;
    for (int it = 0; it < 100; ++it) {
      double p1 = 1, p2 = 0;
      for (int j = 0; j < n; ++j) { const double p3 = p2; p2 = p1; p1 = ((2.0 * j + 1.0) * z * p2 - j * p3) / (j + 1.0); }
      pp = n * (z * p1 - p2) / (z * z - 1.0);
      const double dz = p1 / pp;
      z -= dz;
      if (std::fabs(dz) < 1e-16) break;
    }
    x[i] = -z; x[n - 1 - i] = z;
    w[i] = w[n - 1 - i] = 2.0 / ((1.0 - z * z) * pp * pp);
  }
}
// 1 / What(k / 2N), k = 0 ... N/2, What(xi) = integral of W(t) cos(2 pi xi t) over |t| <= w/2.  With t = (w/2) sin(th) the integrand is entire
// in th: Gauss-Legendre on [0, pi/2], doubled, converges to rounding.
inline std::vector<double> nfft_deconv_table(int N, int w) {
  std::vector<double> x, wt, out((size_t)N / 2 + 1);
  nfft_gauss_legendre(96, x, wt);
  const double beta = NFFT_BETA_PER_W * w, hw = 0.5 * w;
  for (int k = 0; k <= N / 2; ++k) {
    const double xi = (double)k / (2.0 * N);
    double s = 0;
    for (size_t q = 0; q < x.size(); ++q) {
      const double th = 0.25 * M_PI * (x[q] + 1.0);
      s += wt[q] * std::exp(beta * (std::cos(th) - 1.0)) * std::cos(th) * hw * std::cos(2.0 * M_PI * xi * hw * std::sin(th));
    }
    out[k] = 1.0 / (2.0 * 0.25 * M_PI * s);
  }
  return out;
}

// Counting sort of the nodes by tile of the ny x nx fine grid, tile of a node = tile of the cell floor(t).  order[s] = node at sorted slot s
// (stable, so ascending within a tile); off[b ntY + a] ... off[b ntY + a + 1] the slots of tile (a, b).
struct NfftBins { std::vector<int> order, off; };
inline NfftBins nfft_bin_nodes(const std::vector<double>& ty, const std::vector<double>& tx, int ny, int nx) {
  const int ntY = nfft_ntiles(ny), ntX = nfft_ntiles(nx);
  const size_t n = ty.size();
  NfftBins b;
  b.order.assign(n, 0); b.off.assign((size_t)ntY * ntX + 1, 0);
  std::vector<int> tile(n);
  auto cell = [](double t, int m) { const int k = (int)std::floor(t); return k < 0 ? 0 : k > m - 1 ? m - 1 : k; };
  for (size_t k = 0; k < n; ++k) {
    tile[k] = nfft_tile_of(cell(tx[k], nx), nx, ntX) * ntY + nfft_tile_of(cell(ty[k], ny), ny, ntY);
    ++b.off[(size_t)tile[k] + 1];
  }
  for (size_t t = 0; t + 1 < b.off.size(); ++t) b.off[t + 1] += b.off[t];
  std::vector<int> next(b.off.begin(), b.off.end() - 1);
  for (size_t k = 0; k < n; ++k) b.order[(size_t)next[tile[k]]++] = (int)k;
  return b;
}

template <typename T> Ctx<T>* nfft_check_ctx(Ctx<T>* c) {
  constexpr int w = NfftWidth<T>::w;
  CMBL_REQUIRE(c->Ny % 2 == 0 && c->Nx % 2 == 0, ERR_SHAPE, "projector (nfft): Ny and Nx must be even");
  CMBL_REQUIRE(2 * c->Ny >= w && 2 * c->Nx >= w, ERR_SHAPE, "projector (nfft): the fine grid 2Ny x 2Nx must hold one window");
  CMBL_REQUIRE(c->Ny <= NFFT_MAXSIDE && c->Nx <= NFFT_MAXSIDE, ERR_SHAPE, "projector (nfft): Ny and Nx must be at most 2048 (the fine grid is 2Ny x 2Nx)");
  return c;
}

template <typename T>
struct NfftProjector : Projector<T> {
  using Base = Projector<T>;
  using Base::c; using Base::L; using Base::npix; using Base::ncart; using Base::g;
  static constexpr int W = NfftWidth<T>::w;
  static_assert(W % 2 == 0 && W <= NFFT_MAXW && W / 2 <= 8, "tile edges are at least 8 cells: the reach of a window must not exceed that");
  std::unique_ptr<Ctx<T>> fc;                // the fine grid's context
  DevBuf nty, ntx, npx, nc2, ns2, noff, decy, decx;
  DevBuf cref, cF, fref, fF, fmap;           // coarse / fine half planes in reference and F layout, fine maps
  DevBuf rotm;                               // the rotated copy of a cotangent on the patch (to_cart_adjoint)
  NfftNodes<T> nd{};
  NfftModes<T> md{};
  int ntiles = 0;

  NfftProjector(Ctx<T>* ctx, int nside_, int kind, const double* params) : Base(nfft_check_ctx(ctx), nside_, kind, params) {
    CMBL_REQUIRE(L.n_inpatch > 0, ERR_ARG, "projector (nfft): no HEALPix pixel centre lies in the patch (the reference divides by their number)");
    const size_t ni = (size_t)L.n_inpatch, nt = (size_t)L.n_touched;
    std::vector<int> hin(ni), htouched(nt);
    std::vector<double> hi(nt), hj(nt);
    std::vector<T> hc2(nt), hs2(nt);
    auto down = [&](void* dst, const void* src, size_t bytes) { CMBL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); };
    down(hin.data(), L.inpatch, sizeof(int) * ni); down(htouched.data(), L.touched, sizeof(int) * nt);
    down(hi.data(), L.ti, sizeof(double) * nt); down(hj.data(), L.tj, sizeof(double) * nt);
    down(hc2.data(), L.tc2, sizeof(T) * nt); down(hs2.data(), L.ts2, sizeof(T) * nt);
    CMBL_HIP(hipStreamSynchronize(c->stream));
    // both lists ascend and the patch is a subset of the touched pixels: one walk finds each node's (i, j), psi
    std::vector<double> ty(ni), tx(ni);
    std::vector<size_t> at(ni);
    size_t u = 0;
    for (size_t k = 0; k < ni; ++k) {
      while (u < nt && htouched[u] < hin[k]) ++u;
      CMBL_REQUIRE(u < nt && htouched[u] == hin[k], ERR_STATE, "projector (nfft): a pixel of the patch is missing from the touched list");
      at[k] = u;
      ty[k] = std::min(std::max(2.0 * (hi[u] - 1.0), 0.0), 2.0 * c->Ny - 2.0);     // 1 <= i <= Ny: the clamp moves nothing
      tx[k] = std::min(std::max(2.0 * (hj[u] - 1.0), 0.0), 2.0 * c->Nx - 2.0);
    }
    const NfftBins bins = nfft_bin_nodes(ty, tx, 2 * c->Ny, 2 * c->Nx);
    std::vector<double> sty(ni), stx(ni);
    std::vector<int> spx(ni);
    std::vector<T> sc2(ni), ss2(ni);
    for (size_t s = 0; s < ni; ++s) {
      const size_t k = (size_t)bins.order[s];
      sty[s] = ty[k]; stx[s] = tx[k]; spx[s] = hin[k]; sc2[s] = hc2[at[k]]; ss2[s] = hs2[at[k]];
    }
    c->upload(nty, sty); c->upload(ntx, stx); c->upload(npx, spx); c->upload(nc2, sc2); c->upload(ns2, ss2); c->upload(noff, bins.off);
    auto table = [&](DevBuf& b, int N) {
      const std::vector<double> d = nfft_deconv_table(N, W);
      c->upload(b, std::vector<T>(d.begin(), d.end()));
    };
    table(decy, c->Ny); table(decx, c->Nx);
    nd = NfftNodes<T>{nty.as<double>(), ntx.as<double>(), npx.as<int>(), nc2.as<T>(), ns2.as<T>(), noff.as<int>(), (int)ni, c->Ny, c->Nx};
    md = NfftModes<T>{decy.as<T>(), decx.as<T>()};
    ntiles = nfft_ntiles(2 * c->Ny) * nfft_ntiles(2 * c->Nx);
    fc = std::make_unique<Ctx<T>>(2 * c->Ny, 2 * c->Nx, 0.5 * c->theta, c->device, (void*)c->stream);
  }

  int method() const override { return PROJECT_NFFT; }
  int width() const override { return W; }

  void ensure(long sl) {
    fc->prof_on = false;
    cref.ensure(sizeof(cx<T>) * sl * c->plane()); cF.ensure(sizeof(cx<T>) * sl * c->plane());
    fref.ensure(sizeof(cx<T>) * sl * fc->plane()); fF.ensure(sizeof(cx<T>) * sl * fc->plane());
    fmap.ensure(sizeof(T) * sl * fc->npix());
  }

  void to_healpix(int bi, const void* in, void* hpx_out, int P, int B) override {
    CMBL_REQUIRE(bi == B_MAP || g.kind == HPX_LAMBERT, ERR_ARG, "project_to_healpix: a ProjEquiRect input must be in the MAP basis");
    const long sl = (long)P * B;
    ensure(sl);
    const T* m = c->as_maps(bi, in, c->tmpA, this->inm, P, B);               // Map(cart_field) (:319)
    c->rfft2_F(m, cF.as<cx<T>>(), sl);
    c->F2ref(cF.as<cx<T>>(), cref.as<cx<T>>(), sl);
    CMBL_LAUNCH(c, K_NFFT_MODES, (k_nfft_embed<T>), dim3(nblocks(fc->plane()), (unsigned)sl), 0, c->stream, cref.as<cx<T>>(), fref.as<cx<T>>(), md, c->Ny, c->Nx, (T)4);
    fc->ref2F(fref.as<cx<T>>(), fF.as<cx<T>>(), sl);
    fc->F_to_map(fF.as<cx<T>>(), fmap.as<T>(), sl);
    CMBL_HIP(hipMemsetAsync(hpx_out, 0, sizeof(T) * (size_t)npix * P * B, c->stream));
    CMBL_LAUNCH(c, K_NFFT_INTERP, (k_nfft_interp<T, W>), dim3(nblocks(nd.n)), 0, c->stream, fmap.as<T>(), (T*)hpx_out, nd, npix, P, B);
  }

  void to_cart(const void* hpx, void* map_out, int P, int B) override {
    const long sl = (long)P * B;
    ensure(sl);
    CMBL_LAUNCH(c, K_NFFT_SPREAD, (k_nfft_spread<T, W>), dim3((unsigned)ntiles, (unsigned)B), 0, c->stream, (const T*)hpx, fmap.as<T>(), nd, npix, P);
    fc->rfft2_F(fmap.as<T>(), fF.as<cx<T>>(), sl);
    fc->F2ref(fF.as<cx<T>>(), fref.as<cx<T>>(), sl);
    const T scale = (T)((double)c->Ny * c->Nx / (double)nd.n);              // the C2R below divides by Ny Nx; the definition by Npatch
    CMBL_LAUNCH(c, K_NFFT_MODES, (k_nfft_extract<T>), dim3(nblocks(c->plane()), (unsigned)sl), 0, c->stream, fref.as<cx<T>>(), cref.as<cx<T>>(), md, c->Ny, c->Nx, scale);
    c->ref2F(cref.as<cx<T>>(), cF.as<cx<T>>(), sl);
    c->F_to_map(cF.as<cx<T>>(), (T*)map_out, sl);
    if (P >= 2)
      CMBL_LAUNCH(c, K_NFFT_MODES, (k_nfft_rot_cart<T>), dim3(nblocks(ncart), (unsigned)B), 0, c->stream, (const T*)map_out, (T*)map_out, this->c2.template as<T>(), this->s2.template as<T>(), ncart, P);
  }

  // to_healpix^T: mbar_g = 1 / (Ny Nx) sum_{p in patch} K(x_p - x_g) (Rh(psi_p)^T hbar)_p -- the to_cart pipeline with the rotation on the node
  // values as they are loaded, no k_nfft_rot_cart, and the scale 1 / (Ny Nx) (the C2R's own) in place of 1 / Npatch
  void to_healpix_adjoint(const void* hpx_cot, void* map_out, int P, int B) override {
    const long sl = (long)P * B;
    ensure(sl);
    CMBL_LAUNCH(c, K_NFFT_SPREAD, (k_nfft_spread<T, W, true>), dim3((unsigned)ntiles, (unsigned)B), 0, c->stream, (const T*)hpx_cot, fmap.as<T>(), nd, npix, P);
    fc->rfft2_F(fmap.as<T>(), fF.as<cx<T>>(), sl);
    fc->F2ref(fF.as<cx<T>>(), fref.as<cx<T>>(), sl);
    CMBL_LAUNCH(c, K_NFFT_MODES, (k_nfft_extract<T>), dim3(nblocks(c->plane()), (unsigned)sl), 0, c->stream, fref.as<cx<T>>(), cref.as<cx<T>>(), md, c->Ny, c->Nx, (T)1);
    c->ref2F(cref.as<cx<T>>(), cF.as<cx<T>>(), sl);
    c->F_to_map(cF.as<cx<T>>(), (T*)map_out, sl);
  }

  // to_cart^T: hbar_p = 1 / Npatch sum_g K(x_g - x_p) (Rc(psi_g)^T mbar)_g on the patch, exactly 0 elsewhere -- the to_healpix pipeline on a
  // rotated copy of the input (the caller's array is not modified), no rotation at the nodes, and 1 / Npatch in place of 1 / (Ny Nx)
  void to_cart_adjoint(const void* map_cot, void* hpx_out, int P, int B) override {
    const long sl = (long)P * B;
    ensure(sl);
    const T* m = (const T*)map_cot;
    if (P >= 2) {
      rotm.ensure(sizeof(T) * sl * ncart);
      CMBL_LAUNCH(c, K_NFFT_MODES, (k_nfft_rot_cart<T, true>), dim3(nblocks(ncart), (unsigned)B), 0, c->stream, m, rotm.as<T>(), this->c2.template as<T>(), this->s2.template as<T>(), ncart, P);
      m = rotm.as<T>();
    }
    c->rfft2_F(m, cF.as<cx<T>>(), sl);
    c->F2ref(cF.as<cx<T>>(), cref.as<cx<T>>(), sl);
    const T scale = (T)(4.0 * (double)c->Ny * c->Nx / (double)nd.n);         // the fine C2R divides by 4 Ny Nx; the definition by Npatch
    CMBL_LAUNCH(c, K_NFFT_MODES, (k_nfft_embed<T>), dim3(nblocks(fc->plane()), (unsigned)sl), 0, c->stream, cref.as<cx<T>>(), fref.as<cx<T>>(), md, c->Ny, c->Nx, scale);
    fc->ref2F(fref.as<cx<T>>(), fF.as<cx<T>>(), sl);
    fc->F_to_map(fF.as<cx<T>>(), fmap.as<T>(), sl);
    CMBL_HIP(hipMemsetAsync(hpx_out, 0, sizeof(T) * (size_t)npix * P * B, c->stream));
    CMBL_LAUNCH(c, K_NFFT_INTERP, (k_nfft_interp<T, W, false>), dim3(nblocks(nd.n)), 0, c->stream, fmap.as<T>(), (T*)hpx_out, nd, npix, P, B);
  }
};

}  // namespace cmbl
