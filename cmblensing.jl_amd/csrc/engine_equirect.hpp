// Host side of cmbl_equirect_* (src/proj_equirect.jl): the geometry of ProjEquiRect (:71-127, host, double), the AzFourier / QUAzFourier transforms
// (:149-178) and the BlockDiagEquiRect products (:224-269, 358-360, 505-533).  Every launch goes to the context's stream and no call synchronises
// it except block_dot, which returns a number to the host.  The azimuthal line transforms are the context's any-size launches (Ctx::gen_dft) along
// the SLOW map axis (element stride Ny, the Ny lines of a plane are the sequences); the QU pack / unpack are one pointwise kernel per direction
// (kernels_equirect.hpp).  Scratch (the pair of half spectra, or the full QU spectrum) is the context's, grown on demand.
#pragma once
#include "engine.hpp"
#include "kernels_equirect.hpp"

namespace cmbl {

enum { B_AZFOURIER = 3 };

inline double eq_rem2pi(double x) {                                          // rem2pi(x, RoundDown): in [0, 2 pi)
  const double tp = 2.0 * M_PI;
  double r = x - tp * std::floor(x / tp);
  if (r < 0) r += tp;
  if (r >= tp) r -= tp;
  return r;
}
// ProjEquiRect(; Ny, Nx, θspan, φspan) (:71-81, 112-120).  theta, omega: Ny; phi: Nx; the edges one more; lx: Ny x Nx, Ny contiguous
inline void equirect_geometry(int Ny, int Nx, const double* tspan, const double* pspan, double* theta, double* phi, double* theta_edges, double* phi_edges, double* omega, double* lx) {
  const double t0 = std::min(tspan[0], tspan[1]), t1 = std::max(tspan[0], tspan[1]), f0 = std::min(pspan[0], pspan[1]), f1 = std::max(pspan[0], pspan[1]);
  auto lin = [](double a, double b, int i, int nm1) { return i == nm1 ? b : a + (b - a) * ((double)i / (double)nm1); };   // range(a, b, length = nm1 + 1)[i + 1]
  std::vector<double> te((size_t)Ny + 1), pe((size_t)Nx + 1), th((size_t)Ny);
  for (int j = 0; j <= Ny; ++j) te[j] = lin(t0, t1, j, Ny);
  for (int j = 0; j < Ny; ++j) th[j] = lin(t0, t1, 2 * j + 1, 2 * Ny);
  for (int i = 0; i <= Nx; ++i) pe[i] = eq_rem2pi(lin(f0, f1, i, Nx));
  const double dphi = eq_rem2pi(pe[1] - pe[0]);
  for (int j = 0; j < Ny; ++j) {
    if (theta) theta[j] = th[j];
    if (omega) omega[j] = dphi * (std::cos(te[j]) - std::cos(te[j + 1]));
    if (lx) {
      const double dx = std::sin(th[j]) * std::fabs(f0 - f1) / Nx, dl = 2.0 * M_PI / (Nx * dx);
      for (int i = 0; i < Nx; ++i) lx[(size_t)i * Ny + j] = (double)(i < (Nx + 1) / 2 ? i : i - Nx) * dl;     // ifftshift(-Nx÷2:(Nx-1)÷2)
    }
  }
  if (phi) for (int i = 0; i < Nx; ++i) phi[i] = eq_rem2pi(lin(f0, f1, 2 * i + 1, 2 * Nx));
  if (theta_edges) std::copy(te.begin(), te.end(), theta_edges);
  if (phi_edges) std::copy(pe.begin(), pe.end(), phi_edges);
}

inline unsigned eq_grid(long n) { return (unsigned)((n + NTP - 1) / NTP); }

// the launch block of a length-Nx transform along x of `lines` = Ny lines per slice; strides in elements of the respective side
template <typename T> GenDft<T> eq_xpass(const Ctx<T>* c, long in_slice, long out_slice, int nin, int nout) {
  GenDft<T> a{};
  a.nseq = c->Ny; a.nin = nin; a.nout = nout; a.scale = a.scale2 = (T)(1.0 / std::sqrt((double)c->Nx));
  a.in_seq = 1; a.in_elem = c->Ny; a.in_slice = in_slice; a.out_seq = 1; a.out_elem = c->Ny; a.out_slice = out_slice;
  return a;
}

// Map <-> AzFourier (npol 1), QUMap <-> QUAzFourier (npol 2); same-basis calls copy
template <typename T> void equirect_convert(Ctx<T>* c, int bi, const void* in, int bo, void* out, int npol, int B) {
  const int Ny = c->Ny, Nx = c->Nx, Mh = Nx / 2 + 1;
  const long npix = c->npix(), half = (long)Ny * Mh;
  if (bi == bo) {
    const size_t bytes = bi == B_MAP ? sizeof(T) * npix * npol * B : sizeof(cx<T>) * half * npol * B;
    CMBL_HIP(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, c->stream));
    return;
  }
  if (c->eqX.N != Nx) c->build_axis(c->eqX, Nx);
  const GenRun r{c->stream};
  if (npol == 1) {
    if (bi == B_MAP) {                                                       // m_rfft(arr, 2) / sqrt(Nx) (:149-152)
      GenDft<T> a = eq_xpass(c, npix, half, Nx, Mh);
      a.in_real = 1; a.in = in; a.out = out;
      c->gen_dft(r, c->eqX, a, B);
    } else {                                                                 // m_irfft(arr, Nx, 2) * sqrt(Nx) (:154-157): 1 / Nx of the c2r folded in
      GenDft<T> a = eq_xpass(c, half, npix, Mh, Nx);
      a.herm = 1; a.out_real = 1; a.inverse = 1; a.in = in; a.out = out;
      c->gen_dft(r, c->eqX, a, B);
    }
    return;
  }
  if (bi == B_MAP) {                                                         // :160-168.  One pair transform gives fft(Q) and fft(U), the pack kernel F and conj(F[mirror])
    c->eq_scratch.ensure(sizeof(cx<T>) * 2 * half * B);
    cx<T>* FQ = c->eq_scratch.template as<cx<T>>(); cx<T>* FU = FQ + half * B;
    GenDft<T> a = eq_xpass(c, 2 * npix, half, Nx, Mh);
    a.in_real = 1; a.in = in; a.in2 = (const T*)in + npix; a.out = FQ; a.out2 = FU;
    c->gen_dft(r, c->eqX, a, B);
    CMBL_LAUNCH(c, K_EQ_POINT, (k_eq_qu_pack<T>), dim3(eq_grid(half * B)), 0, c->stream, FQ, FU, (cx<T>*)out, Ny, half * B);
  } else {                                                                   // :170-178.  The unpack kernel builds the full spectrum, one complex transform gives Q = Re, U = Im
    c->eq_scratch.ensure(sizeof(cx<T>) * npix * B);
    cx<T>* F = c->eq_scratch.template as<cx<T>>();
    CMBL_LAUNCH(c, K_EQ_POINT, (k_eq_qu_unpack<T>), dim3(eq_grid(npix * B)), 0, c->stream, (const cx<T>*)in, F, Ny, Nx, npix * B);
    GenDft<T> a = eq_xpass(c, npix, 2 * npix, Nx, Nx);
    a.inverse = 1; a.out_real = 1; a.in = F; a.out = out; a.out2 = (T*)out + npix;
    c->gen_dft(r, c->eqX, a, B);
  }
}

// out[p, m, b] = sum_q M[p, q, m] f[q, m, b], or with conj(M[q, p, m]) (:230-240)
template <typename T, bool CPLX, bool ADJ> void equirect_apply_bc(Ctx<T>* c, const void* blocks, int n, const cx<T>* f, cx<T>* out, int B) {
  using E = typename EqElem<T, CPLX>::type;
  const int Mh = c->Nx / 2 + 1;
  const dim3 grid((unsigned)((n + EQ_TP - 1) / EQ_TP), (unsigned)Mh);
  if (B == 1) CMBL_LAUNCH(c, K_EQ_APPLY, (k_eq_apply<T, CPLX, ADJ, 1>), grid, 0, c->stream, (const E*)blocks, f, out, n, Mh, B);
  else if (B <= 4) CMBL_LAUNCH(c, K_EQ_APPLY, (k_eq_apply<T, CPLX, ADJ, 4>), grid, 0, c->stream, (const E*)blocks, f, out, n, Mh, B);
  else CMBL_LAUNCH(c, K_EQ_APPLY, (k_eq_apply<T, CPLX, ADJ, 8>), grid, 0, c->stream, (const E*)blocks, f, out, n, Mh, B);
}
template <typename T> void equirect_block_apply(Ctx<T>* c, const void* blocks, bool cplx, int n, bool adjoint, const void* in, void* out, int B) {
  const cx<T>* f = (const cx<T>*)in; cx<T>* o = (cx<T>*)out;
  if (cplx) { if (adjoint) equirect_apply_bc<T, true, true>(c, blocks, n, f, o, B); else equirect_apply_bc<T, true, false>(c, blocks, n, f, o, B); }
  else { if (adjoint) equirect_apply_bc<T, false, true>(c, blocks, n, f, o, B); else equirect_apply_bc<T, false, false>(c, blocks, n, f, o, B); }
}

// A * B, A' * B, A * B' (:254-269)
template <typename T, bool CPLX> void equirect_matmul_c(Ctx<T>* c, const void* A, bool adjA, const void* Bm, bool adjB, int n, void* out) {
  using E = typename EqElem<T, CPLX>::type;
  const unsigned g = (unsigned)((n + EQ_MT - 1) / EQ_MT);
  const dim3 grid(g, g, (unsigned)(c->Nx / 2 + 1));
  if (adjA) CMBL_LAUNCH(c, K_EQ_MATMUL, (k_eq_matmul<T, CPLX, EQ_HN>), grid, 0, c->stream, (const E*)A, (const E*)Bm, (E*)out, n);
  else if (adjB) CMBL_LAUNCH(c, K_EQ_MATMUL, (k_eq_matmul<T, CPLX, EQ_NH>), grid, 0, c->stream, (const E*)A, (const E*)Bm, (E*)out, n);
  else CMBL_LAUNCH(c, K_EQ_MATMUL, (k_eq_matmul<T, CPLX, EQ_NN>), grid, 0, c->stream, (const E*)A, (const E*)Bm, (E*)out, n);
}
template <typename T> void equirect_block_matmul(Ctx<T>* c, const void* A, bool adjA, const void* Bm, bool adjB, bool cplx, int n, void* out) {
  if (cplx) equirect_matmul_c<T, true>(c, A, adjA, Bm, adjB, n, out); else equirect_matmul_c<T, false>(c, A, adjA, Bm, adjB, n, out);
}

// dot(A', B) (:358-360): out = (re, im) on the host; synchronises the stream
template <typename T> void equirect_block_dot(Ctx<T>* c, const void* A, const void* Bm, bool cplx, int n, double* out) {
  const unsigned g = (unsigned)((n + 31) / 32);
  const dim3 grid(g, g, (unsigned)(c->Nx / 2 + 1));
  const long nparts = (long)g * g * grid.z;
  c->eq_scratch.ensure(sizeof(double) * 2 * (nparts + 1));
  double* part = c->eq_scratch.template as<double>(); double* res = part + 2 * nparts;
  if (cplx) CMBL_LAUNCH(c, K_REDUCE, (k_eq_dot_part<T, true>), grid, 0, c->stream, (const cx<T>*)A, (const cx<T>*)Bm, part, n);
  else CMBL_LAUNCH(c, K_REDUCE, (k_eq_dot_part<T, false>), grid, 0, c->stream, (const T*)A, (const T*)Bm, part, n);
  CMBL_LAUNCH(c, K_REDUCE, (k_eq_dot_sum<NTP>), dim3(1), 0, c->stream, (const double*)part, nparts, res);
  CMBL_HIP(hipMemcpyAsync(out, res, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  CMBL_HIP(hipStreamSynchronize(c->stream));
}

// the weights of a beam, rounded to T like the reference's T.(Ω) (:509, 521), on the device (the upload is a blocking copy: `w` may go away)
template <typename T> const T* equirect_weights(Ctx<T>* c, const double* w_host, int nw) {
  std::vector<T> w((size_t)nw);
  for (int i = 0; i < nw; ++i) w[(size_t)i] = (T)w_host[i];
  c->eq_w.ensure(sizeof(T) * (size_t)nw);
  CMBL_HIP(hipMemcpyAsync(c->eq_w.p, w.data(), sizeof(T) * (size_t)nw, hipMemcpyHostToDevice, c->stream));
  CMBL_HIP(hipStreamSynchronize(c->stream));
  return c->eq_w.template as<T>();
}
template <typename T> void equirect_scale_columns(Ctx<T>* c, void* blocks, bool cplx, int n, const double* w_host) {
  const T* w = equirect_weights(c, w_host, n);
  const long total = (long)n * n * (c->Nx / 2 + 1);
  if (cplx) CMBL_LAUNCH(c, K_EQ_POINT, (k_eq_scale_cols<T, true>), dim3(eq_grid(total)), 0, c->stream, (cx<T>*)blocks, w, n, total);
  else CMBL_LAUNCH(c, K_EQ_POINT, (k_eq_scale_cols<T, false>), dim3(eq_grid(total)), 0, c->stream, (T*)blocks, w, n, total);
}
template <typename T> void equirect_beam_pol(Ctx<T>* c, const void* blocksI, const double* omega_host, void* out) {
  const T* w = equirect_weights(c, omega_host, c->Ny);
  const long total = 4L * c->Ny * c->Ny * (c->Nx / 2 + 1);
  CMBL_LAUNCH(c, K_EQ_POINT, (k_eq_beam_pol<T>), dim3(eq_grid(total)), 0, c->stream, (const T*)blocksI, w, (cx<T>*)out, c->Ny, total);
}

}  // namespace cmbl
