// make_mask (src/masking.jl:1-67): the kernels behind cmbl_edt_sq and cmbl_make_mask.  Planes are map planes [x][y] (y contiguous) or their
// transposes [y][x]; all arithmetic is int32 or double whatever the context's precision; no atomics, every output element has one writer and
// one fixed order of operations, so results are bit-identical between runs.
//   k_mask_border    feature bytes of !boundarymask(pad) (:31-38): 1 on the outer `pad` rows and columns
//   k_mask_scatter   feature bytes of sim_ptsrcs (:60-67) from given (y, x) positions (duplicates store the same byte)
//   k_mask_below     feature bytes of bleed(img, w) (:40-44): d2 < w^2, exact on integers
//   k_edt_cols       exact Euclidean distance transform, pass along the contiguous axis: g = distance to the nearest feature of the line
//   k_edt_rows       ... pass along the other axis, on the transposed plane: d2[i] = min_j (i - j)^2 + g[j]^2
//   k_mask_gauss     one axis of imfilter(d, Kernel.gaussian(sigma)) (:51): correlation along the contiguous axis, "replicate" border
//   k_mask_point     sqrt, the cosine profiles of cos_apod (:53), their product or the boolean `&` (:16-21), Float32.(...) (:23), store in T
#pragma once
#include "common.hpp"

namespace cmbl {

constexpr int EDT_MAXN = 4096;              // longest side of a context (Ctx::Ctx)
constexpr int EDT_INF = 1 << 14;            // "no feature in this line": > any distance on the grid, and EDT_INF^2 + 4095^2 < 2^31
constexpr int MASK_TILE = NTP;              // outputs per workgroup of k_mask_gauss
constexpr int MASK_MAXSIGMA = 1024;         // 4 * sigma + 1 taps: at 1024 the kernel is wider than the widest map

// grid ceil(Ny * Nx / NT)
template <int NT>
__global__ __launch_bounds__(NT) void k_mask_border(unsigned char* __restrict__ feat, int Ny, int Nx, int pad) {
  const long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i >= (long)Ny * Nx) return;
  const int x = (int)(i / Ny), y = (int)(i - (long)x * Ny);
  feat[i] = (y < pad || y >= Ny - pad || x < pad || x >= Nx - pad) ? 1 : 0;
}
// grid ceil(nsrc / NT); the host has checked every position against the map
template <int NT>
__global__ __launch_bounds__(NT) void k_mask_scatter(unsigned char* __restrict__ feat, const int* __restrict__ yx, int nsrc, int Ny) {
  const int s = blockIdx.x * NT + threadIdx.x;
  if (s < nsrc) feat[(long)yx[2 * s + 1] * Ny + yx[2 * s]] = 1;
}
// grid ceil(n / NT)
template <int NT>
__global__ __launch_bounds__(NT) void k_mask_below(const int* __restrict__ d2, unsigned char* __restrict__ feat, long n, int w2) {
  const long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i < n) feat[i] = d2[i] < w2 ? 1 : 0;
}

// One workgroup per line of `n` contiguous bytes (a column of a map plane).  The line is fetched whole and coalesced into LDS; thread t then
// owns the run [t * run, (t + 1) * run): it notes the last and the first feature of its run, the threads exchange them with one max-scan and one
// min-scan over the NT runs, and two walks over the run (up, then down) give g = min(y - last feature at or below y, first feature at or above
// y - y), EDT_INF where the line has no feature.  A line with a feature raises *found, if given (every writer stores the same 1).  grid (lines)
template <int NT>
__global__ __launch_bounds__(NT) void k_edt_cols(const unsigned char* __restrict__ feat, int* __restrict__ g, int n, int* __restrict__ found) {
  __shared__ unsigned char f[EDT_MAXN];
  __shared__ int d[EDT_MAXN];
  __shared__ int lo[2][NT], hi[2][NT];
  const int t = threadIdx.x;
  const long base = (long)blockIdx.x * n;
  for (int y = t; y < n; y += NT) f[y] = feat[base + y];
  __syncthreads();
  const int run = (n + NT - 1) / NT, y0 = min(t * run, n), y1 = min(y0 + run, n);
  int last = -EDT_INF, first = 2 * EDT_INF;                                  // y - last and first - y stay >= EDT_INF for every y of the grid
  for (int y = y0; y < y1; ++y)
    if (f[y]) { last = y; if (first == 2 * EDT_INF) first = y; }
  lo[0][t] = last; hi[0][t] = first;
  __syncthreads();
  int cur = 0;
  for (int s = 1; s < NT; s <<= 1, cur ^= 1) {                              // inclusive scans: lo towards higher t (max), hi towards lower t (min)
    lo[cur ^ 1][t] = t >= s ? max(lo[cur][t], lo[cur][t - s]) : lo[cur][t];
    hi[cur ^ 1][t] = t + s < NT ? min(hi[cur][t], hi[cur][t + s]) : hi[cur][t];
    __syncthreads();
  }
  last = t > 0 ? lo[cur][t - 1] : -EDT_INF;
  first = t + 1 < NT ? hi[cur][t + 1] : 2 * EDT_INF;
  if (found && t == 0 && lo[cur][NT - 1] >= 0) *found = 1;
  for (int y = y0; y < y1; ++y) { if (f[y]) last = y; d[y] = min(y - last, EDT_INF); }
  for (int y = y1 - 1; y >= y0; --y) { if (f[y]) first = y; d[y] = min(d[y], first - y); }
  __syncthreads();
  for (int y = t; y < n; y += NT) g[base + y] = d[y];
}

// One workgroup per line of `n` contiguous g (a row of the map, on the transposed plane), in place.  The line of g^2 sits in LDS; the thread of
// element i starts from best = g[i]^2 and walks outward, r = 1, 2, ..., taking r^2 + g[i -+ r]^2, until r^2 >= best (no farther element can
// win) or both sides have left the line: exact in integers, at worst n candidates.  grid (lines)
template <int NT>
__global__ __launch_bounds__(NT) void k_edt_rows(int* __restrict__ g, int n) {
  __shared__ int q[EDT_MAXN];
  const int t = threadIdx.x;
  int* line = g + (long)blockIdx.x * n;
  for (int i = t; i < n; i += NT) { const int v = line[i]; q[i] = v * v; }
  __syncthreads();
  for (int i = t; i < n; i += NT) {
    int best = q[i];
    const int rmax = max(i, n - 1 - i);
    for (int r = 1; r <= rmax; ++r) {
      const int r2 = r * r;
      if (r2 >= best) break;
      if (i - r >= 0) best = min(best, r2 + q[i - r]);
      if (i + r < n) best = min(best, r2 + q[i + r]);
    }
    line[i] = best;
  }
}

__device__ __forceinline__ double mask_dist(int d2) { return sqrt((double)d2); }
__device__ __forceinline__ double mask_dist(double d) { return d; }

// Correlation of every line of `n` contiguous values with `ntaps` = 2 R + 1 taps, index clamped at both ends (imfilter's "replicate"; the taps
// may be wider than the line).  IN = int: the input is d2 and the filtered quantity its square root (the unclamped distance, :49-51).  A
// workgroup makes MASK_TILE consecutive outputs of one line from MASK_TILE + 2 R inputs held in LDS; the sum runs over the taps in ascending
// order.  grid (ceil(n / MASK_TILE), lines), dynamic LDS (MASK_TILE + 2 R) doubles
template <typename IN>
__global__ __launch_bounds__(NTP) void k_mask_gauss(const IN* __restrict__ in, double* __restrict__ out, const double* __restrict__ taps, int ntaps, int n) {
  extern __shared__ double s_gauss[];
  const int R = ntaps / 2, i0 = blockIdx.x * MASK_TILE;
  const long base = (long)blockIdx.y * n;
  for (int j = threadIdx.x; j < MASK_TILE + 2 * R; j += NTP) s_gauss[j] = mask_dist(in[base + min(max(i0 - R + j, 0), n - 1)]);
  __syncthreads();
  const int i = i0 + threadIdx.x;
  if (i >= n) return;
  double acc = 0;
  for (int k = 0; k < ntaps; ++k) acc += taps[k] * s_gauss[threadIdx.x + k];
  out[base + i] = acc;
}

template <typename T> struct MaskPoint {
  const int* d2b; const double* distb;      // boundary: d2 to the nearest padded pixel, or (edge rounding) the filtered distance itself
  const int* d2p;                           // apodised point sources: d2 to the nearest bled pixel; null: no sources
  const int* d2s;                           // boolean path: d2 to the nearest source; null: no sources
  T* out;
  int Ny, Nx, pad, apod_w, src_w;
};
__device__ __forceinline__ double mask_cos(double d, int w) { return (1.0 - cos(fmin(d, (double)w) / (double)w * M_PI)) / 2.0; }

// grid ceil(Ny * Nx / NTP)
template <typename T>
__global__ __launch_bounds__(NTP) void k_mask_point(const MaskPoint<T> a) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= (long)a.Ny * a.Nx) return;
  double v;
  if (a.apod_w == 0) {                                                       // boundary .& ptsrc (:17)
    const int x = (int)(i / a.Ny), y = (int)(i - (long)x * a.Ny);
    const bool inside = y >= a.pad && y < a.Ny - a.pad && x >= a.pad && x < a.Nx - a.pad;
    v = inside && (!a.d2s || a.d2s[i] >= a.src_w * a.src_w) ? 1.0 : 0.0;
  } else {                                                                   // cos_apod(boundary, ...) .* cos_apod(ptsrc, ...) (:19-20)
    v = mask_cos(a.distb ? a.distb[i] : mask_dist(a.d2b[i]), a.apod_w);
    if (a.d2p) v *= mask_cos(mask_dist(a.d2p[i]), a.src_w);
  }
  a.out[i] = (T)(float)v;                                                    // Float32.(mask_array) whatever T (:23; T.(...) in src/dataset.jl:280)
}

}  // namespace cmbl
