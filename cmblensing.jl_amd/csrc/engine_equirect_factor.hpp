// Host side of cmbl_equirect_block_svd / _logabsdet / _solve: sqrt, pinv, singular values, log|det| and the solves of BlockDiagEquiRect
// (src/proj_equirect.jl:274-282, 313-347) on the device (kernels_equirect_factor.hpp).  The double working copies (two n x n arrays per block for
// the SVD, one plus the right-hand sides for LU) are the call's own; the blocks go through them in slabs of as many blocks as fit option
// "eq_factor_scratch_mb" (at least one), and since a block never sees another one the results do not depend on the slab.  Every call first
// refuses input that is not finite, and returns after synchronising the context's stream (its scratch goes away with it).
#pragma once
#include <algorithm>
#include <cmath>
#include "engine_equirect.hpp"
#include "kernels_equirect_factor.hpp"

namespace cmbl {

enum { EQ_SIDE_LEFT = 0, EQ_SIDE_RIGHT = 1, EQ_RHS_BLOCKS = 0, EQ_RHS_FIELD = 1 };

// CMBL_ERR_NAN when one of the nreal scalars at `a` is NaN or infinite
template <typename T> void eqf_require_finite(Ctx<T>* c, const void* a, long nreal, const char* what) {
  const unsigned g = std::min(1024u, std::max(1u, nblocks(nreal)));
  DevBuf flags;
  flags.ensure(sizeof(int) * g);
  CMBL_LAUNCH(c, K_EQ_FACTOR, (k_eqf_nonfinite<T>), dim3(g), 0, c->stream, (const T*)a, nreal, flags.as<int>());
  std::vector<int> h(g);
  CMBL_HIP(hipMemcpyAsync(h.data(), flags.p, sizeof(int) * g, hipMemcpyDeviceToHost, c->stream));
  CMBL_HIP(hipStreamSynchronize(c->stream));
  for (int f : h) if (f) fail(ERR_NAN, std::string(what) + ": an input element is not finite");
}
template <typename T> int eqf_slab(const Ctx<T>* c, size_t per_block, int Mh) {
  const size_t cap = (size_t)std::max(0, c->opts.eq_factor_scratch_mb) << 20;
  return (int)std::min<size_t>((size_t)Mh, std::max<size_t>(1, cap / per_block));
}

template <typename T, bool CPLX>
void equirect_svd_c(Ctx<T>* c, const void* blocks, int n, double rtol, void* out_sqrt, void* out_pinv, double* sv_host, int* sweeps_host) {
  using E = typename EqElem<T, CPLX>::type;
  using D = typename EqfD<CPLX>::type;
  const int Mh = c->Nx / 2 + 1;
  const size_t nn = (size_t)n * n;
  eqf_require_finite(c, blocks, (long)(nn * Mh) * (CPLX ? 2 : 1), "equirect_block_svd");
  const int slab = eqf_slab(c, 2 * nn * sizeof(D), Mh);
  DevBuf dG, dV, dsig, dw, dst;
  dG.ensure(nn * sizeof(D) * slab); dV.ensure(nn * sizeof(D) * slab);
  dsig.ensure(sizeof(double) * Mh * n); dw.ensure(sizeof(double) * 2 * Mh * n); dst.ensure(sizeof(int) * 2 * Mh);
  const unsigned g = (unsigned)((n + 31) / 32);
  for (int m0 = 0; m0 < Mh; m0 += slab) {
    const int ns = std::min(slab, Mh - m0);
    CMBL_LAUNCH_NT(c, K_EQ_FACTOR, EQF_JT, (k_eqf_jacobi<T, CPLX>), dim3(ns), 0, c->stream, (const E*)blocks, n, m0, dG.as<D>(), dV.as<D>(), dsig.as<double>(),
                   dw.as<double>(), dst.as<int>(), rtol);
    if (out_sqrt) CMBL_LAUNCH(c, K_EQ_FACTOR, (k_eqf_assemble<T, CPLX>), dim3(g, g, ns), 0, c->stream, (const D*)dG.as<D>(), (const D*)dV.as<D>(), (const double*)dw.as<double>(), 0, (E*)out_sqrt, n, m0);
    if (out_pinv) CMBL_LAUNCH(c, K_EQ_FACTOR, (k_eqf_assemble<T, CPLX>), dim3(g, g, ns), 0, c->stream, (const D*)dV.as<D>(), (const D*)dG.as<D>(), (const double*)dw.as<double>(), 1, (E*)out_pinv, n, m0);
  }
  std::vector<int> st((size_t)2 * Mh);
  std::vector<double> sv(sv_host ? (size_t)Mh * n : 0);
  CMBL_HIP(hipMemcpyAsync(st.data(), dst.p, sizeof(int) * st.size(), hipMemcpyDeviceToHost, c->stream));
  if (sv_host) CMBL_HIP(hipMemcpyAsync(sv.data(), dsig.p, sizeof(double) * sv.size(), hipMemcpyDeviceToHost, c->stream));
  CMBL_HIP(hipStreamSynchronize(c->stream));
  for (int m = 0; m < Mh; ++m) {
    if (sweeps_host) sweeps_host[m] = st[(size_t)2 * m];
    if (!st[(size_t)2 * m + 1]) fail(ERR_STATE, "equirect_block_svd: block " + std::to_string(m) + " has not converged after " + std::to_string(EQF_SWEEPS) + " Jacobi sweeps");
  }
  if (sv_host)
    for (int m = 0; m < Mh; ++m) {
      std::sort(sv.begin() + (size_t)m * n, sv.begin() + (size_t)(m + 1) * n, [](double a, double b) { return a > b; });
      std::copy(sv.begin() + (size_t)m * n, sv.begin() + (size_t)(m + 1) * n, sv_host + (size_t)m * n);
    }
}
template <typename T>
void equirect_block_svd(Ctx<T>* c, const void* blocks, bool cplx, int n, double rtol, void* out_sqrt, void* out_pinv, double* sv_host, int* sweeps_host) {
  if (cplx) equirect_svd_c<T, true>(c, blocks, n, rtol, out_sqrt, out_pinv, sv_host, sweeps_host);
  else equirect_svd_c<T, false>(c, blocks, n, rtol, out_sqrt, out_pinv, sv_host, sweeps_host);
}

// (Σ log|u_kk|, Π u_kk / |u_kk| times the parities) over all blocks, summed on the host in double in the order (m, k); a zero pivot: (-inf, 0)
template <typename T, bool CPLX> void equirect_logabsdet_c(Ctx<T>* c, const void* blocks, int n, double* out) {
  using E = typename EqElem<T, CPLX>::type;
  using D = typename EqfD<CPLX>::type;
  const int Mh = c->Nx / 2 + 1;
  const size_t nn = (size_t)n * n;
  eqf_require_finite(c, blocks, (long)(nn * Mh) * (CPLX ? 2 : 1), "equirect_block_logabsdet");
  const int slab = eqf_slab(c, nn * sizeof(D), Mh);
  DevBuf dW, dperm, ddg, dinfo, dpar;
  dW.ensure(nn * sizeof(D) * slab); dperm.ensure(sizeof(int) * (size_t)slab * n);
  ddg.ensure(sizeof(D) * (size_t)Mh * n); dinfo.ensure(sizeof(int) * Mh); dpar.ensure(sizeof(int) * Mh);
  for (int m0 = 0; m0 < Mh; m0 += slab)
    CMBL_LAUNCH(c, K_EQ_FACTOR, (k_eqf_lu<T, CPLX>), dim3(std::min(slab, Mh - m0)), 0, c->stream, (const E*)blocks, n, m0, 0, dW.as<D>(), dperm.as<int>(), ddg.as<D>(),
                dinfo.as<int>(), dpar.as<int>());
  std::vector<double> dg((size_t)Mh * n * (CPLX ? 2 : 1));
  std::vector<int> info((size_t)Mh), par((size_t)Mh);
  CMBL_HIP(hipMemcpyAsync(dg.data(), ddg.p, sizeof(double) * dg.size(), hipMemcpyDeviceToHost, c->stream));
  CMBL_HIP(hipMemcpyAsync(info.data(), dinfo.p, sizeof(int) * Mh, hipMemcpyDeviceToHost, c->stream));
  CMBL_HIP(hipMemcpyAsync(par.data(), dpar.p, sizeof(int) * Mh, hipMemcpyDeviceToHost, c->stream));
  CMBL_HIP(hipStreamSynchronize(c->stream));
  double l = 0, sr = 1, si = 0;
  for (int m = 0; m < Mh; ++m) {
    if (info[(size_t)m]) { out[0] = -INFINITY; out[1] = out[2] = 0; return; }
    for (int k = 0; k < n; ++k) {
      const size_t i = (size_t)m * n + k;
      const double re = CPLX ? dg[2 * i] : dg[i], im = CPLX ? dg[2 * i + 1] : 0.0, a = std::hypot(re, im);
      l += std::log(a);
      const double pr = re / a, pi = im / a, nr = sr * pr - si * pi, ni = sr * pi + si * pr;
      sr = nr; si = ni;
    }
    if (par[(size_t)m]) { sr = -sr; si = -si; }
  }
  out[0] = l; out[1] = sr; out[2] = si;
}
template <typename T> void equirect_block_logabsdet(Ctx<T>* c, const void* blocks, bool cplx, int n, double* out) {
  if (cplx) equirect_logabsdet_c<T, true>(c, blocks, n, out); else equirect_logabsdet_c<T, false>(c, blocks, n, out);
}

// A \ rhs (side LEFT) or rhs / A (side RIGHT: the left solve with A^H on conjugate-transposed right-hand sides, stored back conjugate-transposed);
// rhs: a block array (kind BLOCKS, n right-hand sides per block) or an AzFourier field (B, Mh, n) (kind FIELD, B per block, LEFT only)
template <typename T, bool ACPLX, bool RCPLX>
void equirect_solve_c(Ctx<T>* c, const void* A, int n, int side, const void* rhs, int kind, void* out, int B) {
  constexpr bool OC = ACPLX || RCPLX;
  using AE = typename EqElem<T, ACPLX>::type;
  using AD = typename EqfD<ACPLX>::type;
  using XD = typename EqfD<OC>::type;
  const int Mh = c->Nx / 2 + 1, nrhs = kind == EQ_RHS_BLOCKS ? n : B;
  const size_t nn = (size_t)n * n;
  eqf_require_finite(c, A, (long)(nn * Mh) * (ACPLX ? 2 : 1), "equirect_block_solve");
  eqf_require_finite(c, rhs, (long)Mh * n * nrhs * (RCPLX ? 2 : 1), "equirect_block_solve");
  const int slab = eqf_slab(c, nn * sizeof(AD) + (size_t)nrhs * n * sizeof(XD), Mh);
  DevBuf dW, dX, dperm, ddg, dinfo, dpar;
  dW.ensure(nn * sizeof(AD) * slab); dX.ensure((size_t)nrhs * n * sizeof(XD) * slab); dperm.ensure(sizeof(int) * (size_t)slab * n);
  ddg.ensure(sizeof(AD) * (size_t)Mh * n); dinfo.ensure(sizeof(int) * Mh); dpar.ensure(sizeof(int) * Mh);
  const bool right = side == EQ_SIDE_RIGHT;
  const long sm = kind == EQ_RHS_BLOCKS ? (long)nn : (long)n, sc = kind == EQ_RHS_BLOCKS ? (right ? 1L : (long)n) : (long)Mh * n, se = right ? (long)n : 1L;
  std::vector<int> info((size_t)Mh);
  for (int m0 = 0; m0 < Mh; m0 += slab) {
    const int ns = std::min(slab, Mh - m0);
    CMBL_LAUNCH(c, K_EQ_FACTOR, (k_eqf_lu<T, ACPLX>), dim3(ns), 0, c->stream, (const AE*)A, n, m0, right ? 1 : 0, dW.as<AD>(), dperm.as<int>(), ddg.as<AD>(),
                dinfo.as<int>(), dpar.as<int>());
    CMBL_HIP(hipMemcpyAsync(info.data() + m0, dinfo.as<int>() + m0, sizeof(int) * ns, hipMemcpyDeviceToHost, c->stream));
    CMBL_HIP(hipStreamSynchronize(c->stream));
    for (int m = m0; m < m0 + ns; ++m)
      if (info[(size_t)m]) fail(ERR_NAN, "equirect_block_solve: block " + std::to_string(m) + " is singular (a pivot is exactly zero)");
    CMBL_LAUNCH(c, K_EQ_FACTOR, (k_eqf_solve<T, ACPLX, RCPLX>), dim3((unsigned)((nrhs + EQF_RT - 1) / EQF_RT), (unsigned)ns), 0, c->stream, (const AD*)dW.as<AD>(),
                (const int*)dperm.as<int>(), n, m0, (const typename EqElem<T, RCPLX>::type*)rhs, sm, sc, se, right ? 1 : 0, nrhs, dX.as<XD>(),
                (typename EqElem<T, OC>::type*)out);
  }
  CMBL_HIP(hipStreamSynchronize(c->stream));
}
template <typename T> void equirect_block_solve(Ctx<T>* c, const void* A, bool acplx, int n, int side, const void* rhs, bool rcplx, int kind, void* out, int B) {
  if (acplx) { if (rcplx) equirect_solve_c<T, true, true>(c, A, n, side, rhs, kind, out, B); else equirect_solve_c<T, true, false>(c, A, n, side, rhs, kind, out, B); }
  else { if (rcplx) equirect_solve_c<T, false, true>(c, A, n, side, rhs, kind, out, B); else equirect_solve_c<T, false, false>(c, A, n, side, rhs, kind, out, B); }
}

}  // namespace cmbl
