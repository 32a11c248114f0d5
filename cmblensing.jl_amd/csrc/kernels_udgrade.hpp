// ud_grade (src/proj_lambert.jl:533-592): the kernels that change a field's resolution between TWO contexts of different size.  All three are
// HBM-bound pointwise / gather kernels: no LDS, no atomics, one thread per output element, `slices` = npol * nbatch planes handled alike.
//   k_ud_mean     map [slice][x][y] of the fine grid   -> mean over fac x fac pixel blocks on the coarse grid         (:561)
//   k_ud_repl     map of the coarse grid               -> every pixel replicated fac x fac on the fine grid          (:575-580)
//   k_ud_fourier  half plane in the internal F layout of the fine context ([slice][ky][x slot]) -> F layout of the coarse context: gather of
//                 the coarse grid's frequencies (:566), optional zeroing at and above the coarse Nyquist (:557), optional 1 / PWF (:552,571)
//                 and optional separable complex weight (the block mean as a Fourier-space multiply, engine_ud.hpp)
#pragma once
#include "common.hpp"

namespace cmbl {

template <typename T, int N> struct alignas(N * sizeof(T) <= 16 ? N * sizeof(T) : 16) UdVec { T v[N]; };

// One coarse pixel (X, Y) per thread, consecutive lanes on consecutive Y: a lane reads `fac` contiguous reals of each of `fac` fine columns
// (FAC = 2, 4: one vector load per column -- the host checks the alignment; FAC = 3 and FAC = 0, the run-time factor: scalar loads).  The sum runs
// in the working precision in the fixed order y inner, x outer.  grid (ceil(Nyd * Nxd / NTP), slices)
template <typename T, int FAC>
__global__ __launch_bounds__(NTP) void k_ud_mean(const T* __restrict__ in, T* __restrict__ out, int Nyd, int Nxd, int fac_rt) {
  const int fac = FAC ? FAC : fac_rt;
  const long npd = (long)Nyd * Nxd, i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= npd) return;
  const int X = (int)(i / Nyd), Y = (int)(i - (long)X * Nyd);
  const long Nys = (long)Nyd * fac;
  const T* p = in + ((long)blockIdx.y * Nxd * fac + (long)X * fac) * Nys + (long)Y * fac;
  T acc = 0;
  if constexpr (FAC == 2 || FAC == 4) {
#pragma unroll
    for (int b = 0; b < FAC; ++b) {
      const UdVec<T, FAC> v = *reinterpret_cast<const UdVec<T, FAC>*>(p + b * Nys);
#pragma unroll
      for (int a = 0; a < FAC; ++a) acc += v.v[a];
    }
  } else {
    for (int b = 0; b < fac; ++b)
      for (int a = 0; a < fac; ++a) acc += p[b * Nys + a];
  }
  out[(long)blockIdx.y * npd + i] = acc / (T)(fac * fac);
}

// One fine pixel per thread (stores coalesced along y).  grid (ceil(Nyu * Nxu / NTP), slices); (Nyu, Nxu) = fac * the coarse sides
template <typename T>
__global__ __launch_bounds__(NTP) void k_ud_repl(const T* __restrict__ in, T* __restrict__ out, int Nyu, int Nxu, int fac) {
  const long npu = (long)Nyu * Nxu, i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= npu) return;
  const int x = (int)(i / Nyu), y = (int)(i - (long)x * Nyu);
  const int Nyc = Nyu / fac, Nxc = Nxu / fac;
  out[(long)blockIdx.y * npu + i] = in[((long)blockIdx.y * Nxc + x / fac) * Nyc + y / fac];
}

// lgNx >= 0: x slot s of an F layout holds frequency index brev(s) (fused power-of-two path); < 0: natural order (any-size path)
__device__ __forceinline__ int ud_slot(int i, int lgNx) { return lgNx >= 0 ? brev(i, lgNx) : i; }
__device__ __forceinline__ double ud_sinc(int k, int N) {                   // sinc(k / N) = pixwin at the k-th frequency of an N-pixel side (:200)
  if (k == 0) return 1.0;
  const double t = (double)k / (double)N;
  return sinpi(t) / (M_PI * t);
}

template <typename T> struct UdFourier {
  const cx<T>* in; cx<T>* out;            // F layouts of the fine (Nys x Nxs) and the coarse (Nyd x Nxd) grid; in == out allowed when the grids are equal
  const cx<double>* wy; const cx<double>* wx;   // separable complex weight wy[ky] * wx[kx index] on the coarse grid, or null
  int Nys, Nxs, lgNxs, Nyd, Nxd, lgNxd;
  int pwNy, pwNx;                          // sides of the grid whose pixel window is the denominator of PWF
  int zero, deconv;                        // anti-aliasing by the integer Nyquist rule; multiply by 1 / PWF and nan2zero
  int slices;
};

// One coefficient (ky, x slot) of the coarse half plane per thread, all slices in a loop: the factor is formed once per thread, in double, and
// rounded once.  grid ceil((Nyd / 2 + 1) * Nxd / NTP)
template <typename T>
__global__ __launch_bounds__(NTP) void k_ud_fourier(const UdFourier<T> a) {
  const int Nyhd = a.Nyd / 2 + 1, Nyhs = a.Nys / 2 + 1;
  const long pld = (long)Nyhd * a.Nxd, pls = (long)Nyhs * a.Nxs, i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= pld) return;
  const int ky = (int)(i / a.Nxd), slot = (int)(i - (long)ky * a.Nxd);
  const int ix = ud_slot(slot, a.lgNxd);                                   // column index of the coarse grid, frequency kx = ix or ix - Nxd (:566)
  const int kx = ix < (a.Nxd + 1) / 2 ? ix : ix - a.Nxd;
  const long src = (long)ky * a.Nxs + ud_slot(kx >= 0 ? kx : kx + a.Nxs, a.lgNxs);
  const bool dead = a.zero && (2 * ky >= a.Nyd || 2 * (kx < 0 ? -kx : kx) >= a.Nxd);
  double wr = 1, wi = 0;
  if (a.wy) { const cx<double> u = a.wy[ky], v = a.wx[ix]; wr = u.x * v.x - u.y * v.y; wi = u.x * v.y + u.y * v.x; }
  if (a.deconv) {
    const double inv = (ud_sinc(ky, a.pwNy) * ud_sinc(kx, a.pwNx)) / (ud_sinc(ky, a.Nyd) * ud_sinc(kx, a.Nxd));
    wr *= inv; wi *= inv;
  }
  const cx<T> w = mk<T>((T)wr, (T)wi);
#pragma unroll 4
  for (int s = 0; s < a.slices; ++s) {
    cx<T> v = mk<T>((T)0, (T)0);
    if (!dead) {
      v = a.in[s * pls + src];
      if (a.wy) v = v * w;
      else if (a.deconv) v = w.x * v;
      if (a.deconv && !(isfinite(v.x) && isfinite(v.y))) v = mk<T>((T)0, (T)0);
    }
    a.out[s * pld + i] = v;
  }
}

}  // namespace cmbl
