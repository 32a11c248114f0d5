// The θ-dependent operators of a data set, evaluated on the device (cmbl_dataset_theta_model / cmbl_logpdf_mixed_theta):
//   Cf(θ) = Cfs(bandpower amplitudes) + (r/r0) Cten,  Cϕ(Aϕ) = Cϕ0 Aϕ / Aϕ0,  D(r) = sqrt((C + 2 Cn^ + σ²len) C⁻¹) with C = Cfs + (r/r0) Cten,
//   G(Aϕ) = g0⁻¹ sqrt(1 + 2 Nϕ Cϕ(Aϕ)⁻¹)                                              (src/dataset.jl:272-274, 316-328)
// One pointwise pass over the half plane (F layout, [ky][x slot]) writes pinv(Cf), pinv(D), pinv(Cϕ), pinv(G) in the context's precision and
// leaves per workgroup the partial sums of  logdet Cf + logdet Cϕ,  logdet(D0⁻¹ D)  and  logdet G;  k_theta_sum adds them in a fixed order.
// The DEFINITION of every formula is the host algebra of theta._ops / sim.HarmOp (the 2 x 2 TE block reads the ET plane for both
// off-diagonals, `+ scalar` touches TT, EE, BB, pinv is 1/x with every non-finite result replaced by 0, logdet skips non-finite terms).
// All arithmetic is double in either precision, only the store rounds, and NO product is contracted into a following sum or difference:
// pinv is discontinuous at 0, and a determinant TT EE - ET² that is exactly 0 in separately rounded arithmetic (ℓ = 0, modes outside the
// spectra, fully correlated modes) is a tiny non-zero number when the compiler fuses the subtraction -- hence the pragma in every function.
#pragma once
#include "common.hpp"

namespace cmbl {

constexpr int TH_MAXBANDS = 3;             // TT, TE, EE: BB is never rescaled (src/proj_lambert.jl:385-393)
constexpr int TH_MAXBLK = 1024;            // workgroups of the pass = partial sums per logdet

// the arguments of cmbl_dataset_theta_model (host pointers, reference layout)
struct ThetaModelArgs {
  const double* cfs; int nplanes; const double* c0; int nbands; const int* band_planes; const int32_t* band_idx; const int* band_nbins;
  const double *cten, *cn; double s2len, r0; const double* cphi0; double aphi0; const double *nphi, *g; double logdet_cn;
};

struct ThBlk { double a, b, c, d, e; };    // BlockDiagIEB planes (TT, TE, ET, EE, BB) of one mode

__host__ __device__ inline double th_pinv(double x) {
#pragma clang fp contract(off)
  const double r = 1.0 / x;
  return __builtin_isfinite(r) ? r : 0.0;
}
// one term of Σ λ log|x|, non-finite terms skipped (src/proj_lambert.jl:331-336)
__host__ __device__ inline double th_logterm(double x, double lam) {
#pragma clang fp contract(off)
  const double v = log(fabs(x)) * lam;
  return __builtin_isfinite(v) ? v : 0.0;
}
__host__ __device__ inline ThBlk th_add(const ThBlk& x, const ThBlk& y) {
#pragma clang fp contract(off)
  return {x.a + y.a, x.b + y.b, x.c + y.c, x.d + y.d, x.e + y.e};
}
__host__ __device__ inline ThBlk th_scale(const ThBlk& x, double s) {
#pragma clang fp contract(off)
  return {x.a * s, x.b * s, x.c * s, x.d * s, x.e * s};
}
__host__ __device__ inline ThBlk th_mm(const ThBlk& x, const ThBlk& y) {
#pragma clang fp contract(off)
  const double p1 = x.a * y.a, p2 = x.b * y.c, p3 = x.a * y.b, p4 = x.b * y.d, p5 = x.c * y.a, p6 = x.d * y.c, p7 = x.c * y.b, p8 = x.d * y.d;
  return {p1 + p2, p3 + p4, p5 + p6, p7 + p8, x.e * y.e};
}
__host__ __device__ inline double th_det(const ThBlk& x) {
#pragma clang fp contract(off)
  const double p = x.a * x.d, q = x.c * x.c;
  return p - q;
}
__host__ __device__ inline ThBlk th_pinv(const ThBlk& x) {                 // src/field_vectors.jl:80-84
#pragma clang fp contract(off)
  const double idet = th_pinv(th_det(x));
  const double o = -(x.c * idet);
  return {x.d * idet, o, o, x.a * idet, th_pinv(x.e)};
}
__host__ __device__ inline ThBlk th_sqrt(const ThBlk& x) {                 // src/field_vectors.jl:68-73
#pragma clang fp contract(off)
  const double s = sqrt(th_det(x));
  const double s2 = 2 * s;
  const double t = th_pinv(sqrt(x.a + (x.d + s2)));
  const double o = t * x.c;
  return {t * (x.a + s), o, o, t * (x.d + s), sqrt(x.e)};
}
// D = sqrt((C + N2) C⁻¹), N2 = 2 Cn^ + σ²len already formed (src/dataset.jl:322-328)
__host__ __device__ inline ThBlk th_mix(const ThBlk& C, const ThBlk& N2) { return th_sqrt(th_mm(th_add(C, N2), th_pinv(C))); }
__host__ __device__ inline ThBlk th_noise2(const ThBlk& cn, double s2len) {
#pragma clang fp contract(off)
  const ThBlk n = th_scale(cn, 2.0);
  return {n.a + s2len, n.b, n.c, n.d + s2len, n.e + s2len};
}
// the same for one plane of a diagonal operator
__host__ __device__ inline double th_mix(double C, double cn, double s2len) {
#pragma clang fp contract(off)
  const double n2 = cn * 2.0 + s2len;
  const double m = (C + n2) * th_pinv(C);
  return sqrt(m);
}
__host__ __device__ inline double th_g(double nphi, double cphi) {          // sqrt(1 + 2 Nϕ Cϕ⁻¹)
#pragma clang fp contract(off)
  const double t = 2 * nphi * th_pinv(cphi);
  return sqrt(1 + t);
}

// What the pass reads (all double, F layout, resident) and where it writes
struct ThetaDev {
  const double *cfs, *c0, *cten, *cn, *d0inv;   // np planes each; c0 (bandpower base) may be nullptr: then cfs
  const double *cphi0, *nphi, *g0inv, *guser;   // one plane each; guser may be nullptr
  const int* bidx[TH_MAXBANDS];                 // bin index of every mode, per band; value nb[k] = the constant amplitude 1
  int bmask[TH_MAXBANDS], bnb[TH_MAXBANDS], boff[TH_MAXBANDS], nbands;
  int np, Nx, Ny, Nyh;
  long pl;
  double s2len, aphi0;
};
struct ThetaPoint {
  double s, aphi;                // r / r0 (1 when r is not named), Aϕ (Aϕ0 when not named)
  int r_named, g_theta;          // r named: logdet(D0⁻¹ D) is formed; g_theta: Aϕ named and no fixed G: G(Aϕ) and logdet G are formed
  const double* amps;            // the amplitude vectors of this θ, bands concatenated; nullptr: ones
};

__device__ __forceinline__ double th_amp(const ThetaDev& m, const ThetaPoint& t, int k, long j) {
  if (!(m.bmask[k])) return 1.0;
  const int i = m.bidx[k][j];
  return (t.amps == nullptr || i >= m.bnb[k]) ? 1.0 : t.amps[m.boff[k] + i];
}

// grid: nblk workgroups (<= TH_MAXBLK) of NTP threads, grid-stride over the half plane; part[3][nblk]
template <typename T, bool BLOCK>
__global__ __launch_bounds__(NTP) void k_theta_ops(ThetaDev m, ThetaPoint t, T* __restrict__ cf_inv, T* __restrict__ d_inv, T* __restrict__ cphi_inv,
                                                    T* __restrict__ g_inv, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[3][NTP / 64];
  double acc[3] = {0.0, 0.0, 0.0};
  const long pl = m.pl;
  for (long j = (long)blockIdx.x * NTP + threadIdx.x; j < pl; j += (long)gridDim.x * NTP) {
    const int ky = (int)(j / m.Nx);
    const double lam = (ky == 0 || (m.Ny % 2 == 0 && ky == m.Nyh - 1)) ? 1.0 : 2.0;
    const double* base = m.c0 ? m.c0 : m.cfs;
    if constexpr (BLOCK) {
      ThBlk cb{base[j], base[pl + j], base[2 * pl + j], base[3 * pl + j], base[4 * pl + j]};
      for (int k = 0; k < m.nbands; ++k) {
        const double a = th_amp(m, t, k, j);
        if (m.bmask[k] & 1) cb.a = a * cb.a;
        if (m.bmask[k] & 2) cb.b = a * cb.b;
        if (m.bmask[k] & 4) cb.c = a * cb.c;
        if (m.bmask[k] & 8) cb.d = a * cb.d;
      }
      const ThBlk ten = th_scale(ThBlk{m.cten[j], m.cten[pl + j], m.cten[2 * pl + j], m.cten[3 * pl + j], m.cten[4 * pl + j]}, t.s);
      const ThBlk cf = th_add(cb, ten);
      const ThBlk cfi = th_pinv(cf);
      acc[0] += th_logterm(th_det(cf), lam);
      acc[0] += th_logterm(cf.e, lam);
      const ThBlk cs{m.cfs[j], m.cfs[pl + j], m.cfs[2 * pl + j], m.cfs[3 * pl + j], m.cfs[4 * pl + j]};
      const ThBlk n2 = th_noise2(ThBlk{m.cn[j], m.cn[pl + j], m.cn[2 * pl + j], m.cn[3 * pl + j], m.cn[4 * pl + j]}, m.s2len);
      const ThBlk D = th_mix(th_add(cs, ten), n2);
      const ThBlk Di = th_pinv(D);
      if (t.r_named) {
        const ThBlk q = th_mm(ThBlk{m.d0inv[j], m.d0inv[pl + j], m.d0inv[2 * pl + j], m.d0inv[3 * pl + j], m.d0inv[4 * pl + j]}, D);
        acc[1] += th_logterm(th_det(q), lam);
        acc[1] += th_logterm(q.e, lam);
      }
      cf_inv[j] = (T)cfi.a; cf_inv[pl + j] = (T)cfi.b; cf_inv[2 * pl + j] = (T)cfi.c; cf_inv[3 * pl + j] = (T)cfi.d; cf_inv[4 * pl + j] = (T)cfi.e;
      d_inv[j] = (T)Di.a; d_inv[pl + j] = (T)Di.b; d_inv[2 * pl + j] = (T)Di.c; d_inv[3 * pl + j] = (T)Di.d; d_inv[4 * pl + j] = (T)Di.e;
    } else {
      for (int p = 0; p < m.np; ++p) {
        const long o = p * pl + j;
        double cb = base[o];
        for (int k = 0; k < m.nbands; ++k) if (m.bmask[k] & (1 << p)) cb = th_amp(m, t, k, j) * cb;
        const double ten = m.cten[o] * t.s;
        const double cf = cb + ten;
        acc[0] += th_logterm(cf, lam);
        const double D = th_mix(m.cfs[o] + ten, m.cn[o], m.s2len);
        if (t.r_named) acc[1] += th_logterm(m.d0inv[o] * D, lam);
        cf_inv[o] = (T)th_pinv(cf);
        d_inv[o] = (T)th_pinv(D);
      }
    }
    const double cphi = m.cphi0[j] * t.aphi / m.aphi0;
    acc[0] += th_logterm(cphi, lam);
    cphi_inv[j] = (T)th_pinv(cphi);
    double G = m.guser ? m.guser[j] : 1.0;
    if (t.g_theta) {
      G = m.g0inv[j] * th_g(m.nphi[j], cphi);
      acc[2] += th_logterm(G, lam);
    }
    g_inv[j] = (T)th_pinv(G);
  }
  // fixed-order sum of the workgroup: lanes by shuffle, wavefronts in index order
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double r = 0;
    for (int w = 0; w < NTP / 64; ++w) r += red[threadIdx.x][w];
    part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = r;
  }
}

// out[k] = Σ_g part[k][g], one workgroup, the same order in every run
static __global__ __launch_bounds__(NTP) void k_theta_sum(const double* __restrict__ part, int nblk, double* __restrict__ out) {
  __shared__ double red[3][NTP / 64];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double v = 0;
    for (int i = threadIdx.x; i < nblk; i += NTP) v += part[(size_t)k * nblk + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double r = 0;
    for (int w = 0; w < NTP / 64; ++w) r += red[threadIdx.x][w];
    out[threadIdx.x] = r;
  }
}

}  // namespace cmbl
