// Host side of cmbl_equirect_cov: Cℓ_to_Cov(:I / :P) on ProjEquiRect (src/proj_equirect.jl:430-503), defined as the covariance of the AzFourier /
// QUAzFourier coefficients of an isotropic Gaussian field, since the reference's own arithmetic lives in CirculantCov.jl.  The ℓ-only
// recurrence coefficients (integers, exact) and weights are made here in double; the correlation table (ngrid >= 4) or nothing (ngrid = 0, the exact mode); then, per
// slab of ring pairs: k_eqcov_rows -> the any-size line transform of length Nx in DOUBLE, on a private Ctx<double> the call owns (like the fine grid
// of the NFFT projector, engine_nfft.hpp) -> k_eqcov_pack_*, which alone rounds to T.  A slab holds as many pairs as fit option "eq_cov_scratch_mb"
// (rows + spectra; at least one pair).  Everything runs on the context's stream; the call returns after synchronising it, because the private
// context and its scratch go away with it.
#pragma once
#include "engine_equirect.hpp"
#include "kernels_equirect_cov.hpp"

namespace cmbl {

// K with span = 2π / K, or 0 when the span is no integer fraction of the circle (|K - round(K)| <= 1e-9 K)
inline int equirect_span_K(const double* pspan) {
  const double K = 2.0 * M_PI / std::fabs(pspan[1] - pspan[0]), Kr = std::round(K);
  return (Kr >= 1.0 && std::fabs(K - Kr) <= 1e-9 * K && Kr <= 4096.0) ? (int)Kr : 0;
}

template <typename T>
void equirect_cov(Ctx<T>* c, const double* tspan, const double* pspan, int pol, int lmax, const double* cl_a, const double* cl_b, int ngrid, void* blocks) {
  const int Ny = c->Ny, Nx = c->Nx, Mh = Nx / 2 + 1, K = equirect_span_K(pspan);
  CMBL_REQUIRE(K >= 1, ERR_SHAPE, "equirect_cov: the azimuthal span must be 2 pi / K for an integer K");
  std::vector<double> th((size_t)Ny), st((size_t)Ny), ct((size_t)Ny);
  equirect_geometry(Ny, Nx, tspan, pspan, th.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
  for (int j = 0; j < Ny; ++j) { st[(size_t)j] = std::sin(th[(size_t)j]); ct[(size_t)j] = std::cos(th[(size_t)j]); }
  // nan2zero.(C(ℓ)) is the caller's (a NaN here is an error); weights (2ℓ+1)/(4π) Cℓ and the ℓ-only recurrence coefficients
  auto wgt = [&](const double* cl, int l) { return (2.0 * l + 1.0) / (4.0 * M_PI) * cl[l]; };
  const int per = pol == 0 ? 4 : 6;
  std::vector<double> cf((size_t)per * (lmax + 1), 0.0);
  EqCov a{};
  if (pol == 0) {
    a.w0 = wgt(cl_a, 0); a.w1 = lmax >= 1 ? wgt(cl_a, 1) : 0.0;
    for (int l = 1; l < lmax; ++l) { double* f = &cf[(size_t)4 * l]; f[0] = 2.0 * l + 1.0; f[1] = (double)l; f[2] = l + 1.0; f[3] = wgt(cl_a, l + 1); }
  } else {
    a.w0 = wgt(cl_a, 2) + wgt(cl_b, 2); a.w1 = wgt(cl_a, 2) - wgt(cl_b, 2);
    for (int l = 2; l < lmax; ++l) {
      double* f = &cf[(size_t)6 * l];
      const double dl = l;
      f[0] = 2.0 * dl + 1.0; f[1] = dl * (dl + 1.0); f[2] = (dl + 1.0) * (dl * dl - 4.0); f[3] = dl * ((dl + 1.0) * (dl + 1.0) - 4.0);
      f[4] = wgt(cl_a, l + 1) + wgt(cl_b, l + 1); f[5] = wgt(cl_a, l + 1) - wgt(cl_b, l + 1);
    }
  }
  Ctx<double> dc(2, Nx, 1.0, c->device, (void*)c->stream);                    // the line transforms of length Nx in double (its genX)
  DevBuf d_th, d_st, d_ct, d_cf, d_tab, d_rows, d_spec;
  dc.upload(d_th, th); dc.upload(d_st, st); dc.upload(d_ct, ct); dc.upload(d_cf, cf);
  a.theta = d_th.as<double>(); a.sin_t = d_st.as<double>(); a.cos_t = d_ct.as<double>(); a.coef = d_cf.as<double>();
  a.dphi = 2.0 * M_PI / ((double)K * Nx); a.Ny = Ny; a.Nx = Nx; a.K = K; a.lmax = lmax; a.ngrid = ngrid;
  if (ngrid > 0) {
    d_tab.ensure(sizeof(double) * (size_t)ngrid * (pol == 0 ? 1 : 2));
    if (pol == 0) CMBL_LAUNCH(c, K_EQ_COV, (k_eqcov_table<0>), dim3(nblocks(ngrid)), 0, c->stream, a, d_tab.as<double>());
    else CMBL_LAUNCH(c, K_EQ_COV, (k_eqcov_table<2>), dim3(nblocks(ngrid)), 0, c->stream, a, d_tab.as<double>());
    a.tab = d_tab.as<double>();
  }
  // slabs of the pair enumeration (kernels_equirect_cov.hpp eqcov_pair): spin 0 the Ny (Ny + 1) / 2 pairs j <= k, spin 2 all Ny² pairs
  const long npairs = pol == 0 ? (long)Ny * (Ny + 1) / 2 : (long)Ny * Ny;
  const size_t row_b = pol == 0 ? sizeof(double) * (size_t)Nx : 2 * sizeof(cx<double>) * (size_t)Nx;
  const size_t spec_b = pol == 0 ? sizeof(cx<double>) * (size_t)Mh : 2 * sizeof(cx<double>) * (size_t)Nx;
  const long cap = (long)std::max(0, c->opts.eq_cov_scratch_mb) << 20;
  const long slab = std::min(npairs, std::max(1L, std::min(cap / (long)(row_b + spec_b), 1L << 24)));
  d_rows.ensure(row_b * (size_t)slab); d_spec.ensure(spec_b * (size_t)slab);
  const GenRun r{c->stream};
  for (long p0 = 0; p0 < npairs; p0 += slab) {
    const int np = (int)std::min(slab, npairs - p0), nseq = pol == 0 ? np : 2 * np;
    GenDft<double> g{};
    g.nseq = nseq; g.nin = Nx; g.nout = pol == 0 ? Mh : Nx; g.scale = g.scale2 = 1.0;
    g.in_seq = 1; g.in_elem = nseq; g.out_seq = 1; g.out_elem = nseq;
    g.in_real = pol == 0 ? 1 : 0; g.in = d_rows.p; g.out = d_spec.p;
    if (pol == 0) {
      CMBL_LAUNCH(c, K_EQ_COV, (k_eqcov_rows<0>), dim3(nblocks((long)np * Nx)), 0, c->stream, a, p0, np, d_rows.p);
      dc.gen_dft(r, dc.genX, g, 1);
      CMBL_LAUNCH(c, K_EQ_COV, (k_eqcov_pack_i<T>), dim3(nblocks((long)np * Mh)), 0, c->stream, d_spec.as<cx<double>>(), (T*)blocks, p0, np, Ny, Mh);
    } else {
      CMBL_LAUNCH(c, K_EQ_COV, (k_eqcov_rows<2>), dim3(nblocks((long)np * Nx)), 0, c->stream, a, p0, np, d_rows.p);
      dc.gen_dft(r, dc.genX, g, 1);
      CMBL_LAUNCH(c, K_EQ_COV, (k_eqcov_pack_p<T>), dim3(nblocks((long)np * Mh)), 0, c->stream, d_spec.as<cx<double>>(), (cx<T>*)blocks, p0, np, Ny, Nx);
    }
  }
  CMBL_HIP(hipStreamSynchronize(c->stream));
}

}  // namespace cmbl
