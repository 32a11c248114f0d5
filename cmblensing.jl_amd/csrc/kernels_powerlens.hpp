// Kernels of PowerLens (src/powerlens.jl) and Taylens (src/taylens.jl): lensing by a Taylor series in the deflection.
//
//   PowerLens(order) f  = f + Σ_{n=1..order} Σ_{a+b=n} dx^a dy^b / (a! b!) · irfft((iℓx)^a (iℓy)^b rfft f)                     (:40-48)
//   PowerLens(order)' g = rfft g + Σ_n (-1)^n Σ_{a+b=n} (iℓx)^a (iℓy)^b rfft(dx^a dy^b g) / (a! b!)                            (:50-58)
//   Taylens(order) f    = the same sum with the residual d - round(d / Δx) Δx in place of d, f and every derivative map read at the pixel
//                         round(d / Δx) away (src/taylens.jl:25-66)
//
// As written the factors leave the range of single precision at moderate order: ℓmax^10 = 6.7e38 > FLT_MAX at 2' pixels, while (∇ϕ)^10 ~ 1e-37.
// Here every factor is in pixel units, k = ℓ Δx in [-π√2, π√2] and u = d / Δx: term for term the same number, and no power leaves the range.
//
// Maps are [x][y] with y fastest (I = i + Ny j) as in kernels_bilinear.hpp; Fourier planes are in the internal F layout [ky][x slot], the x slot
// bit-reversed or natural: the kernels only index lx_r and ly with it.  The sums over a run in a fixed order in one thread: no atomics.
#pragma once
#include "common.hpp"
#include "kernels_bilinear.hpp"

namespace cmbl {

constexpr int PL_MAXORDER = 12;
template <typename T> struct PlCoef { T c[PL_MAXORDER + 1]; };            // 1 / (a! (n-a)!), a = 0..n, of one total order n (made in double on the host)
template <typename T, int V> struct alignas(V * sizeof(T)) PlVec { T v[V]; };   // V consecutive reals: one 16-byte load where V sizeof(T) = 16

// i^q z: a quarter-turn, not a complex multiply
template <int Q, typename T> __device__ __forceinline__ cx<T> pl_rot(cx<T> z) {
  constexpr int q = Q & 3;
  if (q == 0) return z;
  if (q == 1) return mk<T>(-z.y, z.x);
  if (q == 2) return mk<T>(-z.x, -z.y);
  return mk<T>(z.y, -z.x);
}
// w[a] = x^a y^(N-a) c[a], a = 0..N: the powers built up one multiply at a time
template <int N, typename T> __device__ __forceinline__ void pl_monomials(T x, T y, const T* __restrict__ c, T (&w)[N + 1]) {
  T py[N + 1];
  py[0] = (T)1;
#pragma unroll
  for (int b = 1; b <= N; ++b) py[b] = py[b - 1] * y;
  T px = (T)1;
#pragma unroll
  for (int a = 0; a <= N; ++a) { w[a] = px * py[N - a] * c[a]; px *= x; }
}
template <int N, typename T> __device__ __forceinline__ void pl_monomials(T x, T y, T (&w)[N + 1]) {
  T one[N + 1];
#pragma unroll
  for (int a = 0; a <= N; ++a) one[a] = (T)1;
  pl_monomials<N, T>(x, y, one, w);
}

// The table of one operator from deflection maps in radians: u = d / Δx in pixels, (ux, uy) per pixel.  Taylens: the wrapped linear index of the
// pixel (i + rint(uy), j + rint(ux)) -- rint is Julia's round, half to even; the index arithmetic is in integers after rint, as k_bl_rows does
// it after floor -- and the residual u - rint(u) in [-1/2, 1/2].
template <typename T>
__global__ __launch_bounds__(NTP) void k_pl_table(const T* __restrict__ dy, const T* __restrict__ dx, T div, int taylens, cx<T>* __restrict__ u,
                                                 unsigned* __restrict__ src, int Ny, int Nx) {
  const long I = (long)blockIdx.x * NTP + threadIdx.x;
  if (I >= (long)Ny * Nx) return;
  T a = dy[I] / div, b = dx[I] / div;
  if (taylens) {
    const int j = (int)(I / Ny), i = (int)(I - (long)j * Ny);
    const T ra = rint(a), rb = rint(b);
    src[I] = (unsigned)bl_wrap<T>(j, rb, Nx) * (unsigned)Ny + (unsigned)bl_wrap<T>(i, ra, Ny);
    a -= ra; b -= rb;                                              // NaN for a non-finite deflection (the pixel then reads NaN)
  }
  u[I] = mk<T>(b, a);
}

// out[a][s] = i^N kx^a ky^(N-a) F[s], a = 0..N: the N + 1 derivative planes of total order N of all S slices from one read of F
template <typename T, int N>
__global__ __launch_bounds__(NTP) void k_pl_mult(const cx<T>* __restrict__ F, cx<T>* __restrict__ out, const T* __restrict__ lx_r, const T* __restrict__ ly,
                                                T dx, int Nx, long plane, int S) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= plane) return;
  T c[N + 1];
  pl_monomials<N, T>(lx_r[(unsigned)i % (unsigned)Nx] * dx, ly[(unsigned)i / (unsigned)Nx] * dx, c);
  for (int s = 0; s < S; ++s) {
    const cx<T> v = pl_rot<N, T>(F[(long)s * plane + i]);
#pragma unroll
    for (int a = 0; a <= N; ++a) out[((long)a * S + s) * plane + i] = c[a] * v;
  }
}

// out[s] = base[s] + Σ_a ux^a uy^(N-a) / (a! (N-a)!) D[a][s], a ascending, for V consecutive pixels per thread (npix % V == 0).  TAY: base (when
// `gather_base`: the first order, whose base is f itself) and every D are read at the source pixel.  N = 0: the base alone (Taylens(0): the permutation).
template <typename T, int N, bool TAY, int V>
__global__ __launch_bounds__(NTP) void k_pl_accum(const cx<T>* __restrict__ u, const unsigned* __restrict__ src, const T* __restrict__ D, const T* base,
                                                 T* out, PlCoef<T> cf, int gather_base, long npix, int S) {
  static_assert(!TAY || V == 1, "the gather is scalar");
  const long I = ((long)blockIdx.x * NTP + threadIdx.x) * V;
  if (I >= npix) return;
  T w[V][N + 1];
  const PlVec<T, 2 * V> uu = *reinterpret_cast<const PlVec<T, 2 * V>*>(u + I);
#pragma unroll
  for (int v = 0; v < V; ++v) pl_monomials<N, T>(uu.v[2 * v], uu.v[2 * v + 1], cf.c, w[v]);
  const long J = TAY ? (long)src[I] : I;
  for (int s = 0; s < S; ++s) {
    PlVec<T, V> acc = *reinterpret_cast<const PlVec<T, V>*>(base + (long)s * npix + (TAY && gather_base ? J : I));
    if (N > 0) {
#pragma unroll
      for (int a = 0; a <= N; ++a) {
        const PlVec<T, V> d = *reinterpret_cast<const PlVec<T, V>*>(D + ((long)a * S + s) * npix + J);
#pragma unroll
        for (int v = 0; v < V; ++v) acc.v[v] += w[v][a] * d.v[v];
      }
    }
    *reinterpret_cast<PlVec<T, V>*>(out + (long)s * npix + I) = acc;
  }
}

// W[a][s] = ux^a uy^(N-a) / (a! (N-a)!) g[s], a = 0..N: the N + 1 weighted maps of every slice from one read of g
template <typename T, int N, int V>
__global__ __launch_bounds__(NTP) void k_pl_premul(const cx<T>* __restrict__ u, const T* __restrict__ g, T* __restrict__ W, PlCoef<T> cf, long npix, int S) {
  const long I = ((long)blockIdx.x * NTP + threadIdx.x) * V;
  if (I >= npix) return;
  T w[V][N + 1];
  const PlVec<T, 2 * V> uu = *reinterpret_cast<const PlVec<T, 2 * V>*>(u + I);
#pragma unroll
  for (int v = 0; v < V; ++v) pl_monomials<N, T>(uu.v[2 * v], uu.v[2 * v + 1], cf.c, w[v]);
  for (int s = 0; s < S; ++s) {
    const PlVec<T, V> gv = *reinterpret_cast<const PlVec<T, V>*>(g + (long)s * npix + I);
#pragma unroll
    for (int a = 0; a <= N; ++a) {
      PlVec<T, V> o;
#pragma unroll
      for (int v = 0; v < V; ++v) o.v[v] = w[v][a] * gv.v[v];
      *reinterpret_cast<PlVec<T, V>*>(W + ((long)a * S + s) * npix + I) = o;
    }
  }
}

// r[s] += (-i)^N Σ_a kx^a ky^(N-a) G[a][s], a ascending
template <typename T, int N>
__global__ __launch_bounds__(NTP) void k_pl_combine(const cx<T>* __restrict__ G, cx<T>* __restrict__ r, const T* __restrict__ lx_r, const T* __restrict__ ly,
                                                   T dx, int Nx, long plane, int S) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= plane) return;
  T c[N + 1];
  pl_monomials<N, T>(lx_r[(unsigned)i % (unsigned)Nx] * dx, ly[(unsigned)i / (unsigned)Nx] * dx, c);
  for (int s = 0; s < S; ++s) {
    cx<T> acc = mk<T>((T)0, (T)0);
#pragma unroll
    for (int a = 0; a <= N; ++a) acc = acc + c[a] * G[((long)a * S + s) * plane + i];
    r[(long)s * plane + i] = r[(long)s * plane + i] + pl_rot<3 * N, T>(acc);
  }
}

}  // namespace cmbl
