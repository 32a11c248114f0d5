// Cℓ_to_Cov on ProjEquiRect (src/proj_equirect.jl:430-503): the kernels behind cmbl_equirect_cov.  The blocks are the covariance of the AzFourier /
// QUAzFourier coefficients of an isotropic Gaussian field.  ALL arithmetic is in double whatever the context's precision; only the
// final store of k_eqcov_pack_* rounds to T.  No atomics, one writer per element and one fixed order of operations: bit-identical between runs
// and between slab sizes.
//   k_eqcov_table     the correlation sums on the uniform grid β_i = i π / (ngrid - 1): one thread per node, upward three-term recurrences in ℓ
//   k_eqcov_rows      per ring pair (j, k) and azimuth n < Nx: the K-fold periodised sequence Σ_r c_jk[n + r Nx], c_jk[d] the correlation at
//                     separation d Δφ (haversine form), from the table (4-point Lagrange) or by the recurrence at the point itself (ngrid = 0);
//                     spin 2: times the bearing phases.  Written [n][sequence], neighbouring pairs contiguous, for the strided line transforms
//   k_eqcov_pack_i    Re of the half spectrum -> blocks[m][k][j] and its mirror blocks[m][j][k]
//   k_eqcov_pack_p    the four quadrants γ_m, ξ_m, conj ξ_J(m), conj γ_J(m), J(m) = (Nx - m) mod Nx
// The ℓ-only coefficients come from the host in double (engine_equirect_cov.hpp) and are read with a wave-uniform index.  They are the INTEGERS of
// the recurrences (exact in double) and each step ends in a true division: with pre-divided, i.e. rounded, coefficients every point would run the
// same slightly wrong recurrence, an error that grows with ℓ and does not average out (measured: 7e-14 / 3e-13 of the block maximum at ℓmax = 2000
// against 3e-15 / 1e-15 for this form).
//   spin 0, 4 per ℓ:  P_{ℓ+1} = ((2ℓ+1) x P_ℓ - ℓ P_{ℓ-1}) / (ℓ+1);  w_{ℓ+1} = (2ℓ+3)/(4π) C_{ℓ+1}
//   spin 2, 6 per ℓ:  d^{ℓ+1}_{2,±2} = ((2ℓ+1) (ℓ(ℓ+1) x ∓ 4) d^ℓ - (ℓ+1)(ℓ²-4) d^{ℓ-1}) / (ℓ ((ℓ+1)²-4));
//                     w±_{ℓ+1} = (2ℓ+3)/(4π) (C^EE ± C^BB)_{ℓ+1};  start d²_{2,±2} = ((1 ± x)/2)²
#pragma once
#include "common.hpp"

namespace cmbl {

struct EqCov {
  const double* theta; const double* sin_t; const double* cos_t;             // Ny each
  const double* coef;                                                        // 4 (spin 0) or 6 (spin 2) doubles per ℓ ≤ lmax
  const double* tab;                                                         // ngrid (spin 0) or 2 ngrid (F+ then F-) doubles; unused when ngrid = 0
  double w0, w1;                                                             // spin 0: w_0, w_1; spin 2: w+_2, w-_2
  double dphi;                                                               // 2π / (K Nx)
  int Ny, Nx, K, lmax, ngrid;
};

__device__ __forceinline__ double eqcov_sum_i(const EqCov& a, double x) {
  double pm = 1.0, p = x, acc = a.w0 + a.w1 * x;
  for (int l = 1; l < a.lmax; ++l) {
    const double* cf = a.coef + 4 * l;
    const double pn = (cf[0] * x * p - cf[1] * pm) / cf[2];
    pm = p; p = pn;
    acc += cf[3] * pn;
  }
  return acc;
}
__device__ __forceinline__ void eqcov_sum_p(const EqCov& a, double x, double& fp, double& fm) {
  const double hp = (1.0 + x) / 2.0, hm = (1.0 - x) / 2.0;
  double pm = 0.0, p = hp * hp, mm = 0.0, m = hm * hm;
  double ap = a.w0 * p, am = a.w1 * m;
  for (int l = 2; l < a.lmax; ++l) {
    const double* cf = a.coef + 6 * l;
    const double lx = cf[1] * x;
    const double pn = (cf[0] * (lx - 4.0) * p - cf[2] * pm) / cf[3], mn = (cf[0] * (lx + 4.0) * m - cf[2] * mm) / cf[3];
    pm = p; p = pn; mm = m; m = mn;
    ap += cf[4] * pn; am += cf[5] * mn;
  }
  fp = ap; fm = am;
}

// grid ceil(ngrid / NTP)
template <int POL>
__global__ __launch_bounds__(NTP) void k_eqcov_table(EqCov a, double* __restrict__ tab) {
  const int i = blockIdx.x * NTP + threadIdx.x;
  if (i >= a.ngrid) return;
  const double s = sin(0.5 * ((double)i * (M_PI / (double)(a.ngrid - 1))));
  const double x = 1.0 - 2.0 * s * s;
  if (POL == 0) tab[i] = eqcov_sum_i(a, x);
  else { double fp, fm; eqcov_sum_p(a, x, fp, fm); tab[i] = fp; tab[a.ngrid + i] = fm; }
}

// cubic Lagrange through the 4 nodes around β; the stencil is shifted inwards at the two ends.  i0 + 3 <= ngrid - 1 (ngrid >= 4)
__device__ __forceinline__ void eqcov_lagrange(const EqCov& a, double h, int& i0, double (&w)[4]) {
  const double beta = 2.0 * asin(sqrt(fmin(h, 1.0)));
  const double u = beta * ((double)(a.ngrid - 1) / M_PI);
  i0 = min(max((int)floor(u) - 1, 0), a.ngrid - 4);
  const double s = u - (double)i0;
  w[0] = -(s - 1.0) * (s - 2.0) * (s - 3.0) / 6.0;
  w[1] = s * (s - 2.0) * (s - 3.0) / 2.0;
  w[2] = -s * (s - 1.0) * (s - 3.0) / 2.0;
  w[3] = s * (s - 1.0) * (s - 2.0) / 6.0;
}

// (re + i im)² / |re + i im|²; 1 where the number vanishes (coincident or antipodal points: the limit)
__device__ __forceinline__ cx<double> eqcov_unit2(double re, double im) {
  const double n = re * re + im * im;
  if (!(n > 1e-24)) return mk<double>(1.0, 0.0);
  return mk<double>((re * re - im * im) / n, 2.0 * re * im / n);
}

// pair g of the slab's enumeration: spin 0 the upper triangle g = k (k + 1) / 2 + j, j <= k; spin 2 all pairs g = k Ny + j
template <int POL> __device__ __forceinline__ void eqcov_pair(long g, int Ny, int& j, int& k) {
  if (POL == 0) {
    long kk = (long)((sqrt(8.0 * (double)g + 1.0) - 1.0) * 0.5);
    while (kk * (kk + 1) / 2 > g) --kk;
    while ((kk + 1) * (kk + 2) / 2 <= g) ++kk;
    k = (int)kk; j = (int)(g - kk * (kk + 1) / 2);
  } else { k = (int)(g / Ny); j = (int)(g - (long)k * Ny); }
}

// pairs [p0, p0 + np) of the enumeration; one thread per (n, pair), the pair fastest.  rows: spin 0 real [n][np]; spin 2 complex [n][2 np], the
// sequence of E[P1 conj P2] at column pl, of E[P1 P2] at column np + pl.  grid ceil(np * Nx / NTP)
template <int POL>
__global__ __launch_bounds__(NTP) void k_eqcov_rows(EqCov a, long p0, int np, void* __restrict__ rows) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= (long)np * a.Nx) return;
  const int n = (int)(i / np), pl = (int)(i - (long)n * np);
  int j, k;
  eqcov_pair<POL>(p0 + pl, a.Ny, j, k);
  const double tj = a.theta[j], tk = a.theta[k], sj = a.sin_t[j], sk = a.sin_t[k], cj = a.cos_t[j], ck = a.cos_t[k];
  const double sdt = sin(0.5 * (tj - tk)), h0 = sdt * sdt, ss = sj * sk;
  const double sjk = sin(tk - tj);
  double acc = 0.0;
  cx<double> ag = mk<double>(0.0, 0.0), ax = ag;
  for (int r = 0; r < a.K; ++r) {
    const double D = (double)(n + r * a.Nx) * a.dphi;
    const double sh1 = sin(0.5 * D), sh = sh1 * sh1;
    const double h = h0 + ss * sh;
    double f0 = 0.0, f1 = 0.0;
    if (a.ngrid > 0) {
      int i0; double w[4];
      eqcov_lagrange(a, h, i0, w);
      const double* t = a.tab + i0;
      f0 = w[0] * t[0] + w[1] * t[1] + w[2] * t[2] + w[3] * t[3];
      if (POL != 0) { t += a.ngrid; f1 = w[0] * t[0] + w[1] * t[1] + w[2] * t[2] + w[3] * t[3]; }
    } else {
      const double x = 1.0 - 2.0 * h;
      if (POL == 0) f0 = eqcov_sum_i(a, x); else eqcov_sum_p(a, x, f0, f1);
    }
    if (POL == 0) acc += f0;
    else {
      // sin β (cos ψ, sin ψ) = (A, B): ψ1 the bearing at ring j's point of ring k's point, from e_θ towards e_φ; ψ2 the bearing back.
      // E[P1 conj P2] = F+ e^{2i(ψ1 - ψ2)}, E[P1 P2] = F- e^{2i(ψ1 + ψ2)} (the signs are the harmonic-space oracle's, tests/_equirect_cov_ref.py)
      const double sD = sin(D);
      const double A1 = sjk - 2.0 * cj * sk * sh, B1 = sk * sD, A2 = -sjk - 2.0 * ck * sj * sh, B2 = -sj * sD;
      const cx<double> eg = eqcov_unit2(A1 * A2 + B1 * B2, B1 * A2 - A1 * B2), ex = eqcov_unit2(A1 * A2 - B1 * B2, B1 * A2 + A1 * B2);
      ag.x += f0 * eg.x; ag.y += f0 * eg.y; ax.x += f1 * ex.x; ax.y += f1 * ex.y;
    }
  }
  if (POL == 0) ((double*)rows)[i] = acc;
  else {
    cx<double>* o = (cx<double>*)rows + (long)n * 2 * np;
    o[pl] = ag; o[np + pl] = ax;
  }
}

// spec: [m][np] complex, m <= Nx/2, the forward transforms of the rows.  One thread per (m, pair).  grid ceil(np * Mh / NTP)
template <typename T>
__global__ __launch_bounds__(NTP) void k_eqcov_pack_i(const cx<double>* __restrict__ spec, T* __restrict__ blocks, long p0, int np, int Ny, int Mh) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= (long)np * Mh) return;
  const int m = (int)(i / np), pl = (int)(i - (long)m * np);
  int j, k;
  eqcov_pair<0>(p0 + pl, Ny, j, k);
  const T v = (T)spec[i].x;
  T* b = blocks + (long)m * Ny * Ny;
  b[(long)k * Ny + j] = v;
  if (j != k) b[(long)j * Ny + k] = v;
}
// spec: [q][2 np] complex, q < Nx: G = spec[q][pl], X = spec[q][np + pl], the FORWARD transforms Σ_n . e^{-2πi q n / Nx} of the two sequences, so that
// γ_m = Σ_d E[P1 conj P2](d) e^{+2πi m d / Nx} = G[J(m)] and ξ_m = X[J(m)].  blocks[m][q][p], n = 2 Ny (the reference's blocks[p, q, m], :488-494)
template <typename T>
__global__ __launch_bounds__(NTP) void k_eqcov_pack_p(const cx<double>* __restrict__ spec, cx<T>* __restrict__ blocks, long p0, int np, int Ny, int Nx) {
  const int Mh = Nx / 2 + 1;
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= (long)np * Mh) return;
  const int m = (int)(i / np), pl = (int)(i - (long)m * np), J = (Nx - m) % Nx;
  int j, k;
  eqcov_pair<2>(p0 + pl, Ny, j, k);
  const cx<double>* sm = spec + (long)m * 2 * np;
  const cx<double>* sJ = spec + (long)J * 2 * np;
  const cx<double> Gm = sm[pl], Xm = sm[np + pl], GJ = sJ[pl], XJ = sJ[np + pl];
  const long n2 = 2L * Ny;
  cx<T>* b = blocks + (long)m * n2 * n2;
  b[(long)k * n2 + j] = mk<T>((T)GJ.x, (T)GJ.y);                             // [j, k] = γ_m
  b[(long)(k + Ny) * n2 + j] = mk<T>((T)XJ.x, (T)XJ.y);                      // [j, k + Ny] = ξ_m
  b[(long)k * n2 + Ny + j] = mk<T>((T)Xm.x, (T)-Xm.y);                       // [j + Ny, k] = conj ξ_J(m)
  b[(long)(k + Ny) * n2 + Ny + j] = mk<T>((T)Gm.x, (T)-Gm.y);                // [j + Ny, k + Ny] = conj γ_J(m)
}

}  // namespace cmbl
