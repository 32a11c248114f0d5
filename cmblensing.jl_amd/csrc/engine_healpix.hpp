// Host side of cmbl_projector_* and cmbl_project_* (src/proj_healpix.jl:122-341): the Projector of one (Nside, Cartesian projection) pair.
// Built once, on the device, in double (kernels_healpix.hpp): the table of the Cartesian pixels, and the ascending lists of the HEALPix
// pixels that are touched (0 < i < Ny+1, 0 < j < Nx+1: the support of Images.bilinear_interpolation) and in the patch (1 <= i <= Ny,
// 1 <= j <= Nx: hpx_idxs_in_patch, :270).  The lists come from flags and an exclusive scan of per-workgroup counts (the scan of the few
// thousand counts on the host: the constructor synchronises anyway to learn the list lengths), so their order is fixed.  Every launch goes to the
// context's stream; the two project calls do not synchronise.  The two transposes (cmbl_project_*_adjoint) gather over a CSR of the transposed
// table, built on the first call of each and cached (HpxAdjTable below); after that they do not synchronise either.
#pragma once
#include <algorithm>
#include "engine.hpp"
#include "kernels_healpix.hpp"

namespace cmbl {

enum { PROJ_INFO_COUNTS = 0, PROJ_INFO_THETA, PROJ_INFO_PHI, PROJ_INFO_PSI_CART, PROJ_INFO_IDX_IN_PATCH, PROJ_INFO_IDX_TOUCHED, PROJ_INFO_I, PROJ_INFO_J,
       PROJ_INFO_PSI_HPX };

inline bool hpx_nside_ok(int nside) { return nside >= 1 && nside <= HPX_MAXNSIDE && ispow2(nside); }

// RotZYX(a, b, c) = Rz(a) Ry(b) Rx(c), angles in degrees, row-major
inline void hpx_rotzyx(const double* deg, double* R) {
  const double a = deg[0] * M_PI / 180.0, b = deg[1] * M_PI / 180.0, c = deg[2] * M_PI / 180.0;
  const double ca = std::cos(a), sa = std::sin(a), cb = std::cos(b), sb = std::sin(b), cc = std::cos(c), sc = std::sin(c);
  R[0] = ca * cb; R[1] = ca * sb * sc - sa * cc; R[2] = ca * sb * cc + sa * sc;
  R[3] = sa * cb; R[4] = sa * sb * sc + ca * cc; R[5] = sa * sb * cc - ca * sc;
  R[6] = -sb;     R[7] = cb * sc;                R[8] = cb * cc;
}

struct ProjectorApi {                        // what the C ABI (api.hip) holds of a Projector (see FlowApi in engine.hpp)
  virtual ~ProjectorApi() = default;
  virtual void to_cart(const void* hpx, void* map_out, int P, int B) = 0;
  virtual void to_healpix(int bi, const void* in, void* hpx_out, int P, int B) = 0;
  virtual void to_cart_adjoint(const void* map_cot, void* hpx_out, int P, int B) = 0;      // the transposes (pullbacks), MAP basis
  virtual void to_healpix_adjoint(const void* hpx_cot, void* map_out, int P, int B) = 0;
  virtual void info(int which, double* out, size_t n) = 0;
  virtual int method() const { return 0; }          // CMBL_PROJECT_BILINEAR; engine_nfft.hpp has the other one
  virtual int width() const { return 0; }           // cells per axis a node touches (0: no window)
};

struct HpxAdjTable { DevBuf rowstart, rowout, ent, val; int nrows = 0; bool built = false; };   // the CSR of a transposed table, on the device

template <typename T>
struct Projector : ProjectorApi {
  Ctx<T>* c;
  CartGeom g{};
  int nside;
  long npix, ncart;
  DevBuf theta, phi, psi, c2, s2, pix, w;    // the Cartesian table
  DevBuf touched, ti, tj, tpsi, tc2, ts2, inpatch;
  DevBuf inm;                                // Map(cart_field) of an input in another basis (:311)
  HpxLists<T> L{};

  Projector(Ctx<T>* ctx, int nside_, int kind, const double* params) : c(ctx), nside(nside_) {
    npix = 12L * nside * nside; ncart = c->npix();
    g.kind = kind; g.Ny = c->Ny; g.Nx = c->Nx;
    if (kind == HPX_LAMBERT) {
      g.dx = c->theta / 60.0 * M_PI / 180.0;
      hpx_rotzyx(params, g.R);
      const double hx = g.dx * (g.Nx / 2 + 0.5), hy = g.dx * (g.Ny / 2 + 0.5);
      CMBL_REQUIRE(hx * hx + hy * hy < 4.0, ERR_ARG, "projector: the Lambert patch reaches beyond the sphere (r = 2)");
    } else {
      g.th0 = std::min(params[0], params[1]); g.dth = std::fabs(params[1] - params[0]);
      g.ph0 = std::min(params[2], params[3]); g.dph = std::fabs(params[3] - params[2]);
      CMBL_REQUIRE(g.dth > 0 && g.dph > 0, ERR_ARG, "projector: an empty span");
    }
    const unsigned gc = nblocks(ncart);
    const int nblk = (int)((npix + HPX_CHUNK - 1) / HPX_CHUNK);
    theta.ensure(sizeof(double) * ncart); phi.ensure(sizeof(double) * ncart); psi.ensure(sizeof(double) * ncart);
    c2.ensure(sizeof(T) * ncart); s2.ensure(sizeof(T) * ncart); pix.ensure(sizeof(int4) * ncart); w.ensure(sizeof(T) * 4 * ncart);
    DevBuf flags, counts, bad;
    flags.ensure((size_t)npix); counts.ensure(sizeof(int) * 2 * nblk); bad.ensure(sizeof(int));
    CMBL_HIP(hipMemsetAsync(bad.p, 0, sizeof(int), c->stream));
    const HpxCartTab<T> tab{theta.as<double>(), phi.as<double>(), psi.as<double>(), c2.as<T>(), s2.as<T>(), pix.as<int4>(), w.as<T>(), bad.as<int>()};
    CMBL_LAUNCH(c, K_HPX_BUILD, (k_hpx_cart_table<T>), dim3(gc), 0, c->stream, g, nside, tab);
    CMBL_LAUNCH(c, K_HPX_BUILD, (k_hpx_flags<T>), dim3((unsigned)nblk), 0, c->stream, g, nside, npix, flags.as<unsigned char>(), counts.as<int>());
    std::vector<int> h((size_t)2 * nblk);
    int isbad = 0;
    CMBL_HIP(hipMemcpyAsync(h.data(), counts.p, sizeof(int) * h.size(), hipMemcpyDeviceToHost, c->stream));
    CMBL_HIP(hipMemcpyAsync(&isbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    CMBL_HIP(hipStreamSynchronize(c->stream));
    CMBL_REQUIRE(isbad == 0, ERR_ARG, "projector: a Cartesian pixel has a colatitude outside [0, pi] (healpy.get_interp_val refuses it)");
    long tot[2] = {0, 0};
    for (int k = 0; k < 2; ++k)
      for (int b = 0; b < nblk; ++b) { const int v = h[(size_t)k * nblk + b]; h[(size_t)k * nblk + b] = (int)tot[k]; tot[k] += v; }
    L.n_touched = (int)tot[0]; L.n_inpatch = (int)tot[1];
    const size_t nt = (size_t)std::max(L.n_touched, 1), ni = (size_t)std::max(L.n_inpatch, 1);
    touched.ensure(sizeof(int) * nt); ti.ensure(sizeof(double) * nt); tj.ensure(sizeof(double) * nt); tpsi.ensure(sizeof(double) * nt);
    tc2.ensure(sizeof(T) * nt); ts2.ensure(sizeof(T) * nt); inpatch.ensure(sizeof(int) * ni);
    L.touched = touched.as<int>(); L.ti = ti.as<double>(); L.tj = tj.as<double>(); L.tpsi = tpsi.as<double>(); L.tc2 = tc2.as<T>(); L.ts2 = ts2.as<T>();
    L.inpatch = inpatch.as<int>();
    CMBL_HIP(hipMemcpyAsync(counts.p, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, c->stream));
    CMBL_LAUNCH(c, K_HPX_BUILD, (k_hpx_compact<T>), dim3((unsigned)nblk), 0, c->stream, g, nside, npix, flags.as<unsigned char>(), counts.as<int>(), L);
    CMBL_HIP(hipStreamSynchronize(c->stream));                                // the scratch and `h` go away on return
  }
  Projector(const Projector&) = delete;
  Projector& operator=(const Projector&) = delete;

  void to_cart(const void* hpx, void* map_out, int P, int B) override {
    CMBL_LAUNCH(c, K_HPX_PROJECT, (k_hpx_to_cart<T>), dim3(nblocks(ncart)), 0, c->stream, (const T*)hpx, (T*)map_out, pix.as<int4>(),
                w.as<T>(), c2.as<T>(), s2.as<T>(), ncart, npix, P, B);
  }
  void to_healpix(int bi, const void* in, void* hpx_out, int P, int B) override {
    CMBL_REQUIRE(bi == B_MAP || g.kind == HPX_LAMBERT, ERR_ARG, "project_to_healpix: a ProjEquiRect input must be in the MAP basis");
    const T* m = c->as_maps(bi, in, c->tmpA, inm, P, B);                      // Map(cart_field) (:311)
    CMBL_HIP(hipMemsetAsync(hpx_out, 0, sizeof(T) * (size_t)npix * P * B, c->stream));
    if (L.n_touched > 0)
      CMBL_LAUNCH(c, K_HPX_PROJECT, (k_hpx_to_healpix<T>), dim3(nblocks(L.n_touched)), 0, c->stream, m, (T*)hpx_out, L, c->Ny, c->Nx, npix, P, B);
  }

  // ---- the transposes (kernels_healpix.hpp k_hpx_adjoint) ----
  // The CSR of a transposed table is built on the first adjoint call of its direction and kept: on the host, from a readback of the table the
  // forward kernel reads (nfft_bin_nodes is the precedent), because the order of a row's entries is part of the result and a host sort fixes
  // it without a device sort to write and test; it costs one readback and O(entries log entries) once per projector.
  HpxAdjTable adj_c, adj_h;                                                      // of to_cart, of to_healpix

  // to_cart^T: entries (c, k) keyed by pix[c][k].  The key carries (c, k) in its low bits, so sorting the keys IS the stable sort by pixel of
  // the entries listed by ascending c, then k.  Rows: the distinct pixels, ascending (at most 4 Ny Nx: nothing here is O(npix)).
  void build_adj_cart() {
    if (adj_c.built) return;
    std::vector<int4> hp((size_t)ncart);
    std::vector<T> hw((size_t)4 * ncart);
    CMBL_HIP(hipMemcpyAsync(hp.data(), pix.p, sizeof(int4) * hp.size(), hipMemcpyDeviceToHost, c->stream));
    CMBL_HIP(hipMemcpyAsync(hw.data(), w.p, sizeof(T) * hw.size(), hipMemcpyDeviceToHost, c->stream));
    CMBL_HIP(hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> keys((size_t)4 * ncart);
    for (long cc = 0; cc < ncart; ++cc) {
      const int pk[4] = {hp[cc].x, hp[cc].y, hp[cc].z, hp[cc].w};
      for (int k = 0; k < 4; ++k) {
        CMBL_REQUIRE(pk[k] >= 0 && (long)pk[k] < npix, ERR_STATE, "projector: a pixel of the Cartesian table lies outside the sphere");
        keys[(size_t)4 * cc + k] = ((unsigned long long)pk[k] << 32) | (unsigned long long)(4 * cc + k);
      }
    }
    std::sort(keys.begin(), keys.end());
    std::vector<int> rs, ro, en(keys.size());
    std::vector<T> va(keys.size());
    for (size_t e = 0; e < keys.size(); ++e) {
      const int p = (int)(keys[e] >> 32);
      const unsigned slot = (unsigned)(keys[e] & 0xffffffffull);
      if (ro.empty() || ro.back() != p) { ro.push_back(p); rs.push_back((int)e); }
      en[e] = (int)(slot >> 2); va[e] = hw[slot];
    }
    rs.push_back((int)keys.size());
    c->upload(adj_c.rowstart, rs); c->upload(adj_c.rowout, ro); c->upload(adj_c.ent, en); c->upload(adj_c.val, va);
    adj_c.nrows = (int)ro.size(); adj_c.built = true;
  }
  // to_healpix^T: entries (t, k) keyed by the Cartesian pixel of corner k of touched slot t, corners and weights exactly as k_hpx_to_healpix
  // forms them (a corner outside the map is no entry).  Counting sort over the Ny Nx rows, t ascending, then k: stable.
  void build_adj_hpx() {
    if (adj_h.built) return;
    const size_t nt = (size_t)L.n_touched;
    std::vector<double> hi(nt), hj(nt);
    if (nt) {
      CMBL_HIP(hipMemcpyAsync(hi.data(), L.ti, sizeof(double) * nt, hipMemcpyDeviceToHost, c->stream));
      CMBL_HIP(hipMemcpyAsync(hj.data(), L.tj, sizeof(double) * nt, hipMemcpyDeviceToHost, c->stream));
      CMBL_HIP(hipStreamSynchronize(c->stream));
    }
    const int Ny = c->Ny, Nx = c->Nx;
    auto corners = [&](size_t t, long off[4], T wt[4]) {                      // off < 0: outside
      const double i = hi[t], j = hj[t], fi = std::floor(i), fj = std::floor(j), ci = std::ceil(i), cj = std::ceil(j);
      const double wy[2] = {1.0 - i + fi, i - fi}, wx[2] = {1.0 - j + fj, j - fj};
      const int ys[2] = {(int)fi, (int)ci}, xs[2] = {(int)fj, (int)cj};
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
          const bool in = ys[b] >= 1 && ys[b] <= Ny && xs[a] >= 1 && xs[a] <= Nx;
          wt[2 * a + b] = in ? (T)(wy[b] * wx[a]) : T(0);
          off[2 * a + b] = in ? (long)(xs[a] - 1) * Ny + (ys[b] - 1) : -1;
        }
    };
    std::vector<int> rs((size_t)ncart + 1, 0);
    long off[4]; T wt[4];
    for (size_t t = 0; t < nt; ++t) {
      corners(t, off, wt);
      for (int k = 0; k < 4; ++k) if (off[k] >= 0) ++rs[(size_t)off[k] + 1];
    }
    for (long r = 0; r < ncart; ++r) rs[(size_t)r + 1] += rs[(size_t)r];
    std::vector<int> next(rs.begin(), rs.end() - 1), en((size_t)rs[(size_t)ncart]);
    std::vector<T> va(en.size());
    for (size_t t = 0; t < nt; ++t) {
      corners(t, off, wt);
      for (int k = 0; k < 4; ++k)
        if (off[k] >= 0) { const size_t e = (size_t)next[(size_t)off[k]]++; en[e] = (int)t; va[e] = wt[k]; }
    }
    if (en.empty()) { en.push_back(0); va.push_back(T(0)); }                  // no touched pixel: every row is empty, the arrays are never read
    c->upload(adj_h.rowstart, rs); c->upload(adj_h.ent, en); c->upload(adj_h.val, va);
    adj_h.nrows = (int)ncart; adj_h.built = true;
  }
  template <bool TO_SPHERE>
  void launch_adjoint(const HpxCsr<T>& A, const T* in, T* out, long nin, long nout, int P, int B) {
    const dim3 grid((unsigned)((A.nrows + HPX_ADJ_NT - 1) / HPX_ADJ_NT));
    if (P == 1) CMBL_LAUNCH_NT(c, K_HPX_PROJECT, HPX_ADJ_NT, (k_hpx_adjoint<T, 1, TO_SPHERE>), grid, 0, c->stream, in, out, A, nin, nout, B);
    else if (P == 2) CMBL_LAUNCH_NT(c, K_HPX_PROJECT, HPX_ADJ_NT, (k_hpx_adjoint<T, 2, TO_SPHERE>), grid, 0, c->stream, in, out, A, nin, nout, B);
    else CMBL_LAUNCH_NT(c, K_HPX_PROJECT, HPX_ADJ_NT, (k_hpx_adjoint<T, 3, TO_SPHERE>), grid, 0, c->stream, in, out, A, nin, nout, B);
  }
  // hbar[p] = sum_{(c, k): pix[c][k] = p} w[c][k] (Rc(psi_c)^T mbar[c]); exactly 0 where no Cartesian pixel reads
  void to_cart_adjoint(const void* map_cot, void* hpx_out, int P, int B) override {
    build_adj_cart();
    CMBL_HIP(hipMemsetAsync(hpx_out, 0, sizeof(T) * (size_t)npix * P * B, c->stream));
    const HpxCsr<T> A{adj_c.rowstart.as<int>(), adj_c.rowout.as<int>(), adj_c.ent.as<int>(), adj_c.val.as<T>(), nullptr, c2.as<T>(), s2.as<T>(), adj_c.nrows};
    launch_adjoint<true>(A, (const T*)map_cot, (T*)hpx_out, ncart, npix, P, B);
  }
  // mbar[c] = sum_{(t, k): c_tk = c} v[t][k] (Rh(psi_t)^T hbar[p_t]); every map pixel is written
  void to_healpix_adjoint(const void* hpx_cot, void* map_out, int P, int B) override {
    build_adj_hpx();
    const HpxCsr<T> A{adj_h.rowstart.as<int>(), nullptr, adj_h.ent.as<int>(), adj_h.val.as<T>(), L.touched, L.tc2, L.ts2, adj_h.nrows};
    launch_adjoint<false>(A, (const T*)hpx_cot, (T*)map_out, npix, ncart, P, B);
  }

  void info(int which, double* out, size_t n) override {
    if (which == PROJ_INFO_COUNTS) {
      CMBL_REQUIRE(n == 2, ERR_SHAPE, "projector_info: the counts are two numbers (in patch, touched)");
      out[0] = L.n_inpatch; out[1] = L.n_touched;
      return;
    }
    const bool cart = which >= PROJ_INFO_THETA && which <= PROJ_INFO_PSI_CART;
    const bool isint = which == PROJ_INFO_IDX_IN_PATCH || which == PROJ_INFO_IDX_TOUCHED;
    CMBL_REQUIRE(which >= PROJ_INFO_THETA && which <= PROJ_INFO_PSI_HPX, ERR_ARG, "projector_info: bad selector");
    const size_t want = cart ? (size_t)ncart : which == PROJ_INFO_IDX_IN_PATCH ? (size_t)L.n_inpatch : (size_t)L.n_touched;
    CMBL_REQUIRE(n == want, ERR_SHAPE, "projector_info: output has the wrong length");
    if (n == 0) return;
    const void* src = which == PROJ_INFO_THETA ? theta.p : which == PROJ_INFO_PHI ? phi.p : which == PROJ_INFO_PSI_CART ? psi.p
                    : which == PROJ_INFO_IDX_IN_PATCH ? inpatch.p : which == PROJ_INFO_IDX_TOUCHED ? touched.p : which == PROJ_INFO_I ? ti.p
                    : which == PROJ_INFO_J ? tj.p : tpsi.p;
    if (isint) {
      std::vector<int> v(n);
      CMBL_HIP(hipMemcpyAsync(v.data(), src, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
      CMBL_HIP(hipStreamSynchronize(c->stream));
      for (size_t k = 0; k < n; ++k) out[k] = v[k];
    } else {
      CMBL_HIP(hipMemcpyAsync(out, src, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
      CMBL_HIP(hipStreamSynchronize(c->stream));
    }
  }
};

}  // namespace cmbl
