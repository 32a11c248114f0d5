// Kernels of BilinearLens (src/bilinearlens.jl): lensing by bilinear interpolation at the deflected pixel centres.
//
// Maps are [x][y] with y (length Ny) fastest, the reference's column-major (Ny, Nx): pixel (i, j) has linear index I = i + Ny j and is deflected to
// (i + dy, j + dx) in pixel units.  Per pixel the TABLE holds the wrapped linear index of the neighbour (floor(i + dy), floor(j + dx)) and the two
// fractions (fy, fx) -- 12 bytes in single precision instead of four index / weight pairs; the other three neighbours and the closed-form weights
// (1-fy)(1-fx), fy(1-fx), (1-fy)fx, fy fx (= inv(A)[1, :] of :67-73) are formed in registers.  floor and the fraction come from the deflection
// alone and the pixel index is added afterwards in integers: the position never loses the eps * N pixels that `ĩs .+ (1:Ny)` in the working
// precision costs (:44-45).
//
// The transposed operator is a gather as well, over a CSR of L' made once per table: an integer count per source pixel, an exclusive scan, an
// integer-atomic fill, and then every (short) row is put in order of its target index, so that the summation order -- every bit of L'g -- does
// not depend on the order in which the atomics landed.  No floating-point atomics anywhere.
#pragma once
#include "common.hpp"
#include "kernels_pointwise.hpp"

namespace cmbl {

constexpr int BL_SCAN = 4 * NTP;                 // elements per workgroup of the scan
constexpr int BL_MAXIT = 16;                     // most GMRES iterations (the least-squares thread keeps the Hessenberg matrix in private memory)

// i + fl (fl integral-valued) wrapped into [0, N): mod(i - 1, N) + 1 of :48 for any sign and length of the deflection.  fmod is exact.
template <typename T> __device__ __forceinline__ int bl_wrap(int i, T fl, int N) {
  const int r = isfinite(fl) ? (int)fmod(fl, (T)N) : 0;         // in (-N, N)
  int t = i + r;
  if (t < 0) t += N;
  if (t >= N) t -= N;
  return t;
}
// the four neighbours in the reference's order (:62): (i0, j0), (i0+1, j0), (i0, j0+1), (i0+1, j0+1)
__device__ __forceinline__ void bl_neigh(unsigned b, int Ny, int Nx, unsigned a[4]) {
  const unsigned j0 = b / (unsigned)Ny, i0 = b - j0 * (unsigned)Ny;
  const unsigned i1 = i0 + 1 == (unsigned)Ny ? 0u : i0 + 1, j1 = j0 + 1 == (unsigned)Nx ? 0u : j0 + 1;
  a[0] = b; a[1] = j0 * Ny + i1; a[2] = j1 * Ny + i0; a[3] = j1 * Ny + i1;
}
template <typename T> __device__ __forceinline__ T bl_weight(cx<T> f, int k) {
  const T wy = (k & 1) ? f.x : (T)1 - f.x, wx = (k & 2) ? f.y : (T)1 - f.y;
  return wy * wx;
}

// flag |= any(v != 0): norm(ϕ) == 0 makes the operator the identity (:34)
template <typename T> __global__ __launch_bounds__(NTP) void k_bl_anynz(const T* __restrict__ v, long n, int* __restrict__ flag) {
  bool nz = false;
  for (long i = (long)blockIdx.x * NTP + threadIdx.x; i < n; i += (long)gridDim.x * NTP) nz |= v[i] != (T)0;
  if (nz) atomicOr(flag, 1);
}
// (i lx, i ly) F -> out[2][slices][plane], F layout
template <typename T>
__global__ __launch_bounds__(NTP) void k_bl_gradmult(const cx<T>* __restrict__ F, cx<T>* __restrict__ out, const T* __restrict__ lx_r, const T* __restrict__ ly,
                                                    int Nx, long plane, int S) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= plane) return;
  const T lx = lx_r[(unsigned)i % (unsigned)Nx], l_y = ly[(unsigned)i / (unsigned)Nx];
  for (int s = 0; s < S; ++s) {
    const cx<T> v = F[(long)s * plane + i];
    out[(long)s * plane + i] = mk<T>(-lx * v.y, lx * v.x);
    out[((long)S + s) * plane + i] = mk<T>(-l_y * v.y, l_y * v.x);
  }
}
// the table of one operator from the deflection maps: (sign * d) / div pixels (div = Δx for maps of ∇ϕ, :43; sign = -1: BilinearLens(-ϕ), :94)
template <typename T>
__global__ __launch_bounds__(NTP) void k_bl_rows(const T* __restrict__ dy, const T* __restrict__ dx, T div, T sign, unsigned* __restrict__ base,
                                                cx<T>* __restrict__ fr, int Ny, int Nx) {
  const long I = (long)blockIdx.x * NTP + threadIdx.x;
  if (I >= (long)Ny * Nx) return;
  const int j = (int)(I / Ny), i = (int)(I - (long)j * Ny);
  const T a = sign * dy[I] / div, b = sign * dx[I] / div;
  const T fa = floor(a), fb = floor(b);
  base[I] = (unsigned)bl_wrap<T>(j, fb, Nx) * (unsigned)Ny + (unsigned)bl_wrap<T>(i, fa, Ny);
  fr[I] = mk<T>(a - fa, b - fb);                             // in [0, 1]; NaN for a non-finite deflection (the pixel then reads NaN)
}
// f̃[I] = Σ₄ w f[idx] for every slice (:107-115): one thread per pixel reads its table entry once
template <typename T>
__global__ __launch_bounds__(NTP) void k_bl_gather(const unsigned* __restrict__ base, const cx<T>* __restrict__ fr, const T* __restrict__ in,
                                                  T* __restrict__ out, int Ny, int Nx, int S) {
  const long npix = (long)Ny * Nx;
  const long I = (long)blockIdx.x * NTP + threadIdx.x;
  if (I >= npix) return;
  unsigned a[4];
  bl_neigh(base[I], Ny, Nx, a);
  const cx<T> f = fr[I];
  const T w0 = bl_weight<T>(f, 0), w1 = bl_weight<T>(f, 1), w2 = bl_weight<T>(f, 2), w3 = bl_weight<T>(f, 3);
  for (int s = 0; s < S; ++s) {
    const T* p = in + (long)s * npix;
    out[(long)s * npix + I] = w0 * p[a[0]] + w1 * p[a[1]] + w2 * p[a[2]] + w3 * p[a[3]];
  }
}

// ---- CSR of the transposed operator --------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(NTP) void k_bl_count(const unsigned* __restrict__ base, unsigned* __restrict__ cnt, int Ny, int Nx) {
  const long I = (long)blockIdx.x * NTP + threadIdx.x;
  if (I >= (long)Ny * Nx) return;
  unsigned a[4];
  bl_neigh(base[I], Ny, Nx, a);
  for (int k = 0; k < 4; ++k) atomicAdd(&cnt[a[k]], 1u);
}
// exclusive scan, three launches: per workgroup of BL_SCAN elements, over the workgroup totals (one workgroup), and the offsets added back
__device__ __forceinline__ unsigned bl_block_excl(unsigned t, unsigned* sh, unsigned* total) {
  const int tid = threadIdx.x;
  sh[tid] = t;
  __syncthreads();
  for (int o = 1; o < NTP; o <<= 1) {
    const unsigned x = tid >= o ? sh[tid - o] : 0u;
    __syncthreads();
    sh[tid] += x;
    __syncthreads();
  }
  const unsigned incl = sh[tid];
  *total = sh[NTP - 1];
  __syncthreads();
  return incl - t;
}
static __global__ __launch_bounds__(NTP) void k_bl_scan1(const unsigned* __restrict__ cnt, unsigned* __restrict__ excl, unsigned* __restrict__ blksum, long n) {
  __shared__ unsigned sh[NTP];
  const long b0 = (long)blockIdx.x * BL_SCAN + 4L * threadIdx.x;
  unsigned loc[4], t = 0;
  for (int k = 0; k < 4; ++k) { loc[k] = t; t += b0 + k < n ? cnt[b0 + k] : 0u; }
  unsigned total;
  const unsigned off = bl_block_excl(t, sh, &total);
  for (int k = 0; k < 4; ++k) if (b0 + k < n) excl[b0 + k] = off + loc[k];
  if (threadIdx.x == 0) blksum[blockIdx.x] = total;
}
static __global__ __launch_bounds__(NTP) void k_bl_scan2(unsigned* __restrict__ blksum, int nblk) {
  __shared__ unsigned sh[NTP];
  const int per = (nblk + NTP - 1) / NTP, b0 = threadIdx.x * per;
  unsigned t = 0;
  for (int k = 0; k < per; ++k) if (b0 + k < nblk) t += blksum[b0 + k];
  unsigned total;
  unsigned off = bl_block_excl(t, sh, &total);
  for (int k = 0; k < per; ++k) if (b0 + k < nblk) { const unsigned v = blksum[b0 + k]; blksum[b0 + k] = off; off += v; }
}
static __global__ __launch_bounds__(NTP) void k_bl_scan3(unsigned* __restrict__ excl, const unsigned* __restrict__ blksum, long n, unsigned total) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i < n) excl[i] += blksum[i / BL_SCAN];
  if (i == 0) excl[n] = total;
}
// keys[pos] = 4 I + k in the row of source pixel a[k]; the order within a row is whatever the atomics gave -- k_bl_sort settles it
static __global__ __launch_bounds__(NTP) void k_bl_fill(const unsigned* __restrict__ base, const unsigned* __restrict__ rowstart, unsigned* __restrict__ cur,
                                                       unsigned* __restrict__ keys, int Ny, int Nx) {
  const long I = (long)blockIdx.x * NTP + threadIdx.x;
  if (I >= (long)Ny * Nx) return;
  unsigned a[4];
  bl_neigh(base[I], Ny, Nx, a);
  for (int k = 0; k < 4; ++k) keys[rowstart[a[k]] + atomicAdd(&cur[a[k]], 1u)] = ((unsigned)I << 2) | (unsigned)k;
}
// one thread per source pixel: its row sorted by key (rows hold 4 entries on average: insertion sort; heap sort beyond 32 so that a deflection
// that piles many pixels onto one stays O(L log L)), then decoded in place to the target index, with the weight next to it
template <typename T>
__global__ __launch_bounds__(NTP) void k_bl_sort(const unsigned* __restrict__ rowstart, unsigned* __restrict__ col, T* __restrict__ val,
                                                const cx<T>* __restrict__ fr, long npix) {
  const long J = (long)blockIdx.x * NTP + threadIdx.x;
  if (J >= npix) return;
  const unsigned s = rowstart[J], e = rowstart[J + 1];
  unsigned* r = col + s;
  const int L = (int)(e - s);
  if (L <= 32) {
    for (int p = 1; p < L; ++p) {
      const unsigned v = r[p];
      int q = p - 1;
      while (q >= 0 && r[q] > v) { r[q + 1] = r[q]; --q; }
      r[q + 1] = v;
    }
  } else {
    auto sift = [&](int root, int end) {
      for (;;) {
        int ch = 2 * root + 1;
        if (ch >= end) break;
        if (ch + 1 < end && r[ch] < r[ch + 1]) ++ch;
        if (r[root] >= r[ch]) break;
        const unsigned t = r[root]; r[root] = r[ch]; r[ch] = t;
        root = ch;
      }
    };
    for (int st = L / 2 - 1; st >= 0; --st) sift(st, L);
    for (int end = L - 1; end > 0; --end) { const unsigned t = r[0]; r[0] = r[end]; r[end] = t; sift(0, end); }
  }
  for (int p = 0; p < L; ++p) {
    const unsigned key = r[p], I = key >> 2;
    val[s + p] = bl_weight<T>(fr[I], (int)(key & 3u));
    r[p] = I;
  }
}
// g̃[J] = Σ_row val g[col] for every slice (:117-125), four slices per pass over the row
template <typename T>
__global__ __launch_bounds__(NTP) void k_bl_csr(const unsigned* __restrict__ rowstart, const unsigned* __restrict__ col, const T* __restrict__ val,
                                               const T* __restrict__ in, T* __restrict__ out, long npix, int S) {
  const long J = (long)blockIdx.x * NTP + threadIdx.x;
  if (J >= npix) return;
  const unsigned s = rowstart[J], e = rowstart[J + 1];
  for (int s0 = 0; s0 < S; s0 += 4) {
    T acc[4] = {0, 0, 0, 0};
    const int ns = S - s0 < 4 ? S - s0 : 4;
    for (unsigned p = s; p < e; ++p) {
      const unsigned c = col[p];
      const T v = val[p];
#pragma unroll
      for (int q = 0; q < 4; ++q) if (q < ns) acc[q] += v * in[(long)(s0 + q) * npix + c];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) if (q < ns) out[(long)(s0 + q) * npix + J] = acc[q];
  }
}

// ---- GMRES (src/numerical_algorithms.jl:193-214) as Arnoldi with modified Gram-Schmidt, per slice ----------------------------------------
// One pass of modified Gram-Schmidt: w -= h q (h = the dot of the previous pass, read from the device) and the partial sums of the NEXT dot
// <w, qdot> (qdot null: <w, w>), in double.  grid (blocks, slices); the partials are finished by k_reduce_final<T, SUM_FLOAT64>.
template <typename T>
__global__ __launch_bounds__(NTP) void k_bl_mgs(T* __restrict__ w, const T* __restrict__ qprev, const double* __restrict__ hprev, const T* __restrict__ qdot,
                                               double* __restrict__ part, long n) {
  const int s = blockIdx.y;
  const long off = (long)s * n;
  const double h = qprev ? hprev[s] : 0.0;
  double acc = 0;
  for (long i = (long)blockIdx.x * NTP + threadIdx.x; i < n; i += (long)gridDim.x * NTP) {
    T x = w[off + i];
    if (qprev) { x = (T)((double)x - h * (double)qprev[off + i]); w[off + i] = x; }
    const T y = qdot ? qdot[off + i] : x;
    acc += (double)x * (double)y;
  }
  const double r = block_sum<double>(acc);
  if (threadIdx.x == 0) part[(long)s * gridDim.x + blockIdx.x] = r;
}
// breakdown test of column k: the new direction is rounding noise when its squared norm is below thr2 x that of the column before orthogonalisation
// (= the sum of squares of the column's entries, Pythagoras).  col: h(0, k) with stride `cs` doubles between rows.
__device__ __forceinline__ bool bl_alive(double nrm2, const double* col, long cs, int rows, double thr2) {
  double tot = nrm2;
  for (int j = 0; j < rows; ++j) { const double h = col[(long)j * cs]; tot += h * h; }
  return nrm2 > 0 && nrm2 > thr2 * tot;
}
// q = w / |w| (in place), or 0 on breakdown: every later column of that slice is then 0 as well, and k_bl_lsq stops at this one
template <typename T>
__global__ __launch_bounds__(NTP) void k_bl_scale(T* __restrict__ w, const double* __restrict__ nrm2, const double* __restrict__ col, long cs, int rows,
                                                 double thr2, long n) {
  const int s = blockIdx.y;
  const double v = nrm2[s];
  const double sc = bl_alive(v, col + s, cs, rows, thr2) ? 1.0 / sqrt(v) : 0.0;
  for (long i = (long)blockIdx.x * NTP + threadIdx.x; i < n; i += (long)gridDim.x * NTP) w[(long)s * n + i] = (T)((double)w[(long)s * n + i] * sc);
}
// min |beta e1 - H y| per slice by Givens rotations, one thread per slice.  H[(j m + k) S + s] = h(j, k), the sub-diagonal entries SQUARED (they are
// the norms' squares as reduced); beta^2 at row (m + 1), column 0.
static __global__ __launch_bounds__(64) void k_bl_lsq(const double* __restrict__ H, double* __restrict__ y, int m, int S, double thr2) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  double R[BL_MAXIT + 1][BL_MAXIT], g[BL_MAXIT + 1], cs_[BL_MAXIT], sn_[BL_MAXIT];
  auto h = [&](int j, int k) { return H[((long)j * m + k) * S + s]; };
  int meff = 0;
  g[0] = sqrt(h(m + 1, 0));
  for (int k = 0; k < m; ++k) {
    for (int j = 0; j <= k; ++j) R[j][k] = h(j, k);
    const double sub2 = h(k + 1, k);
    const bool alive = bl_alive(sub2, H + ((long)k) * S + s, (long)m * S, k + 1, thr2);
    double sub = alive ? sqrt(sub2) : 0.0;
    for (int j = 0; j < k; ++j) {                                           // the rotations of the earlier columns
      const double a = R[j][k], b = R[j + 1][k];
      R[j][k] = cs_[j] * a + sn_[j] * b; R[j + 1][k] = -sn_[j] * a + cs_[j] * b;
    }
    const double d = hypot(R[k][k], sub);
    cs_[k] = d > 0 ? R[k][k] / d : 1.0; sn_[k] = d > 0 ? sub / d : 0.0;
    R[k][k] = d;
    g[k + 1] = -sn_[k] * g[k]; g[k] = cs_[k] * g[k];
    meff = k + 1;
    if (!alive) break;
  }
  for (int k = m - 1; k >= 0; --k) {
    double v = 0;
    if (k < meff && R[k][k] != 0) {
      v = g[k];
      for (int j = k + 1; j < meff; ++j) v -= R[k][j] * y[(long)j * S + s];
      v /= R[k][k];
    }
    y[(long)k * S + s] = v;
  }
}
// x = Σ_k y_k q_k  (`view(K, :, 1:n) * α`, :212, in the orthonormal basis)
template <typename T>
__global__ __launch_bounds__(NTP) void k_bl_combine(const T* __restrict__ Q, const double* __restrict__ y, T* __restrict__ out, int m, int S, long n) {
  const int s = blockIdx.y;
  for (long i = (long)blockIdx.x * NTP + threadIdx.x; i < n; i += (long)gridDim.x * NTP) {
    double acc = 0;
    for (int k = 0; k < m; ++k) acc += y[(long)k * S + s] * (double)Q[((long)k * S + s) * n + i];
    out[(long)s * n + i] = (T)acc;
  }
}

// ---- pullback (:165-171) -----------------------------------------------------------------------------------------------------------------
// v[k][b] = Σ_pol Δ[b][pol] ∇_k f̃[b][pol]; g = [2][B P][npix]
template <typename T>
__global__ __launch_bounds__(NTP) void k_bl_polsum(const T* __restrict__ delta, const T* __restrict__ g, T* __restrict__ v, long npix, int P, int B) {
  const int b = blockIdx.y;
  const long S = (long)P * B;
  for (long i = (long)blockIdx.x * NTP + threadIdx.x; i < npix; i += (long)gridDim.x * NTP) {
    T a0 = 0, a1 = 0;
    for (int p = 0; p < P; ++p) {
      const long o = ((long)b * P + p) * npix + i;
      const T d = delta[o];
      a0 += d * g[o]; a1 += d * g[S * npix + o];
    }
    v[(long)b * npix + i] = a0; v[((long)B + b) * npix + i] = a1;
  }
}
// δϕ = ∇' · v = -(i lx V1 + i ly V2), V = [2][B][plane] in F layout
template <typename T>
__global__ __launch_bounds__(NTP) void k_bl_div(const cx<T>* __restrict__ V, cx<T>* __restrict__ out, const T* __restrict__ lx_r, const T* __restrict__ ly,
                                               int Nx, long plane, int B) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= plane) return;
  const T lx = lx_r[(unsigned)i % (unsigned)Nx], l_y = ly[(unsigned)i / (unsigned)Nx];
  for (int b = 0; b < B; ++b) {
    const cx<T> a = V[(long)b * plane + i], c = V[((long)B + b) * plane + i];
    out[(long)b * plane + i] = mk<T>(lx * a.y + l_y * c.y, -(lx * a.x + l_y * c.x));
  }
}

}  // namespace cmbl
