// Host side of cmbl_clbins_* and cmbl_get_cl: get_Cℓ (src/proj_lambert.jl:470-513) on the device.
// The reference unfolds the half plane to the full plane, masks min(ℓedges) < ℓ < max(ℓedges) (both strict), and histograms five weighted sums into the
// left-closed bins [e_i, e_i+1).  Two facts shape this file:
//   * ℓ and Re(conj(f1) f2) are equal at a mode and at its Hermitian mirror, so every full-plane sum is the half-plane sum weighted by the context's
//     λ (h_lam: 1 on ky = 0 and on the Nyquist row of an even Ny, 2 elsewhere) -- the full plane is never formed;
//   * A = Σ w, Sℓ = Σ w·ℓ and the mode count depend on the grid, the edges and the weight only: ClBins makes them ONCE, on the host, in double, together
//     with each mode's bin, from the very numbers cmbl_ctx_geometry_host(which = 5) returns.  Only S1 = Σ w·CL and S2 = Σ w·CL² need the device.
// ClBins holds no kernel and is made by api.hip; get_cl<T> launches and is instantiated by tu_main_* only (api_decl.hpp has the rule).
#pragma once
#include <algorithm>
#include <cmath>
#include "engine.hpp"
#include "kernels_cl.hpp"

namespace cmbl {

struct ClBins {
  int Ny = 0, Nx = 0, dtype = 0, device = 0, nbins = 0, chunks = 0;
  bool generic = false;
  double theta = 0, alpha = 0;                        // α = Nx·Ny / Δx²  (:473)
  std::vector<double> A, Sl, count;                   // per bin: Σ λw, Σ λw·ℓ, Σ λ (the full-plane number of modes; N of :492 is half of it)
  long listed = 0;                                    // kept half-plane modes
  // two copies of the list, each sorted by (bin, address in ITS layout) so that the gathers of a chunk run along memory: [0] the reference layout
  // [x][ky] of FOURIER / HARMONIC arguments, [1] the context's internal F layout [ky][x slot] that rfft2_F leaves a MAP argument in
  DevBuf idx[2], coef[2], chunk_start, bin_chunk;
  DevBuf part;                                        // chunk partials of the call in flight (calls on one plan are ordered on the context's stream)

  // ledges: nedges finite, strictly increasing doubles; w: the per-mode weight on the half plane [x][ky] or null for (2ℓ+1)/2, i.e. Cℓfid = 1 (:482)
  ClBins(const CtxBase& c, const double* ledges, int nedges, const double* w) {
    Ny = c.Ny; Nx = c.Nx; dtype = c.dtype; device = c.device; generic = c.generic; theta = c.theta;
    const double dx = theta / 60.0 * M_PI / 180.0;
    alpha = (double)Nx * (double)Ny / (dx * dx);
    nbins = nedges - 1;
    A.assign(nbins, 0.0); Sl.assign(nbins, 0.0); count.assign(nbins, 0.0);
    const int Nyh = c.Nyh;
    const long pl = c.plane();
    std::vector<int> bin(pl, -1);                     // reference layout
    std::vector<int> nin(nbins + 1, 0);
    const double lo = ledges[0], hi = ledges[nbins];
    for (int x = 0; x < Nx; ++x)
      for (int ky = 0; ky < Nyh; ++ky) {
        const long i = (long)x * Nyh + ky;
        const double L = c.h_lmag[i];
        if (!(L > lo && L < hi)) continue;            // :476, both strict
        const int b = (int)(std::upper_bound(ledges, ledges + nedges, L) - ledges) - 1;      // e_b <= L < e_b+1
        const double lam = c.h_lam[ky], wi = w ? w[i] : (2.0 * L + 1.0) / 2.0;
        bin[i] = b; ++nin[b + 1];
        A[b] += lam * wi; Sl[b] += lam * wi * L; count[b] += lam;
      }
    for (int b = 0; b < nbins; ++b) nin[b + 1] += nin[b];          // offsets of the bins in the list
    listed = nin[nbins];
    // chunks: each bin's run cut every CL_CHUNK modes
    std::vector<int> cs, bc(nbins + 1, 0);
    for (int b = 0; b < nbins; ++b) {
      for (int s = nin[b]; s < nin[b + 1]; s += CL_CHUNK) cs.push_back(s);
      bc[b + 1] = (int)cs.size();
    }
    chunks = (int)cs.size();
    cs.push_back((int)listed);
    auto xslot = [&](int x) { if (generic) return x; int r = 0; for (int k = 0; k < c.lgNx; ++k) r |= ((x >> k) & 1) << (c.lgNx - 1 - k); return r; };
    CMBL_HIP(hipSetDevice(device));
    for (int lay = 0; lay < 2; ++lay) {               // a counting sort by bin over the modes visited in address order
      std::vector<unsigned> id((size_t)std::max<long>(listed, 1));
      std::vector<double> cf((size_t)std::max<long>(listed, 1));
      std::vector<int> at(nin.begin(), nin.end() - 1);
      auto put = [&](int x, int ky, unsigned addr) {
        const long i = (long)x * Nyh + ky;
        if (bin[i] < 0) return;
        const int k = at[bin[i]]++;
        id[k] = addr; cf[k] = c.h_lam[ky] * (w ? w[i] : (2.0 * c.h_lmag[i] + 1.0) / 2.0);
      };
      if (lay == 0) { for (int x = 0; x < Nx; ++x) for (int ky = 0; ky < Nyh; ++ky) put(x, ky, (unsigned)((long)x * Nyh + ky)); }
      else {
        std::vector<int> xof(Nx);                     // frequency index held by slot s (the bit reversal is its own inverse)
        for (int s = 0; s < Nx; ++s) xof[s] = xslot(s);
        for (int ky = 0; ky < Nyh; ++ky) for (int s = 0; s < Nx; ++s) put(xof[s], ky, (unsigned)((long)ky * Nx + s));
      }
      up(idx[lay], id, c.stream); up(coef[lay], cf, c.stream);
    }
    up(chunk_start, cs, c.stream); up(bin_chunk, bc, c.stream);
  }
  template <typename V> static void up(DevBuf& b, const std::vector<V>& v, hipStream_t st) {
    b.ensure(v.size() * sizeof(V));
    CMBL_HIP(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice, st));
    CMBL_HIP(hipStreamSynchronize(st));
  }
  // a plan belongs to the geometry it was made for: the bins come from that context's ℓmag, the addresses from its layouts
  void check(const CtxBase& c) const {
    CMBL_REQUIRE(c.Ny == Ny && c.Nx == Nx && c.theta == theta && c.generic == generic, ERR_SHAPE, "get_cl: the binning plan was made for a context of another size, pixel size or layout");
    CMBL_REQUIRE(c.dtype == dtype && c.device == device, ERR_ARG, "get_cl: the binning plan was made for a context of another precision or device");
  }
};

// out[slot][pair][moment][bin] (device doubles) on the context's stream.  MAP fields go through rfft2_F into the context's scratch and are read in the
// F layout; complex fields are read where they lie.
template <typename T>
void get_cl(Ctx<T>* c, ClBins& bins, int basis, const void* f1, const void* f2, int P, int B, const ClPairs& pr, int moments, double* out) {
  bins.check(*c);
  const long sl = (long)P * B, pl = c->plane();
  const bool cross = f2 != nullptr && f2 != f1;
  ClArgs<T> a{};
  int lay = 0;
  if (basis == B_MAP) {
    c->tmpA.ensure(sizeof(cx<T>) * (cross ? 2 : 1) * sl * pl);
    cx<T>* F1 = c->tmpA.template as<cx<T>>();
    c->rfft2_F((const T*)f1, F1, sl);
    a.f1 = F1; a.f2 = F1;
    if (cross) { c->rfft2_F((const T*)f2, F1 + sl * pl, sl); a.f2 = F1 + sl * pl; }
    lay = 1;
  } else {
    a.f1 = (const cx<T>*)f1; a.f2 = cross ? (const cx<T>*)f2 : a.f1;
  }
  const long rows = (long)B * pr.n * moments;
  if (bins.chunks > 0) {
    bins.part.ensure(sizeof(double) * rows * bins.chunks);
    a.idx = bins.idx[lay].as<unsigned>(); a.coef = bins.coef[lay].as<double>(); a.chunk_start = bins.chunk_start.as<int>();
    a.part = bins.part.as<double>(); a.plane = pl; a.npol = P; a.chunks = bins.chunks; a.pr = pr;
    const dim3 grid((unsigned)bins.chunks, (unsigned)B);
    if (moments == 1) { if (cross) CMBL_LAUNCH(c, K_CL, (k_cl_chunks<T, 1, true>), grid, 0, c->stream, a); else CMBL_LAUNCH(c, K_CL, (k_cl_chunks<T, 1, false>), grid, 0, c->stream, a); }
    else { if (cross) CMBL_LAUNCH(c, K_CL, (k_cl_chunks<T, 2, true>), grid, 0, c->stream, a); else CMBL_LAUNCH(c, K_CL, (k_cl_chunks<T, 2, false>), grid, 0, c->stream, a); }
  }
  const long total = rows * bins.nbins;
  const dim3 fg((unsigned)((total + NTP - 1) / NTP));
  if (moments == 1) CMBL_LAUNCH(c, K_CL, (k_cl_final<1>), fg, 0, c->stream, bins.part.as<double>(), bins.bin_chunk.as<int>(), out, total, bins.nbins, bins.chunks, 1.0 / bins.alpha);
  else CMBL_LAUNCH(c, K_CL, (k_cl_final<2>), fg, 0, c->stream, bins.part.as<double>(), bins.bin_chunk.as<int>(), out, total, bins.nbins, bins.chunks, 1.0 / bins.alpha);
}

}  // namespace cmbl
