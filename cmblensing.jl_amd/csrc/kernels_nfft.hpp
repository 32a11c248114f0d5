// The non-uniform half of project(...; method = :fft) (src/proj_healpix.jl:229-236, 314-325): the kernels behind a Projector of method
// CMBL_PROJECT_NFFT (engine_nfft.hpp has the host side and the definition).  Oversampled-grid NUFFT, sigma = 2: the fine grid is 2Ny x 2Nx,
// stored like a map (y fastest), and a node at the fractional pixel (i, j) (1-based) sits at the fine coordinates t = (2 (i - 1), 2 (j - 1)).
// Window: exp of semicircle, W(t) = exp(beta (sqrt(1 - (2t/w)^2) - 1)) on |t| <= w/2, beta = 2.3 w, separable; a node touches the w cells
// k0 ... k0 + w - 1 of each axis, k0 = ceil(t - w/2), wrapped periodically (2N >= w: the w cells are distinct).  Node positions and window
// arguments are double and each window value is rounded once to T; grids, sums and transforms are T.
// No atomics: every fine cell, every HEALPix pixel and every mode has one writer and one fixed order of summation.
//   k_nfft_embed     coarse half plane -> fine half plane: deconvolve, Hermitian weights of the Nyquist modes, scale   (Cartesian -> HEALPix)
//   k_nfft_interp    fine grid -> HEALPix pixels of the patch, QU rotation and scatter fused
//   k_nfft_spread    HEALPix pixels of the patch -> fine grid, one workgroup per tile of the fine grid                    (HEALPix -> Cartesian)
//   k_nfft_extract   fine half plane -> coarse half plane: the transpose of k_nfft_embed
//   k_nfft_rot_cart  QU rotation at the Cartesian pixels, in place
// The transposes of the two directions reuse the same kernels: k_nfft_spread<ROT> rotates the node values as it loads them,
// k_nfft_interp<ROT = false> does not rotate, k_nfft_rot_cart<ADJ> applies the transposed rotation into a scratch array.
// Half planes are in the reference layout [kx slot][ky] (ky fastest, natural order), which both contexts convert to and from.
#pragma once
#include <cmath>
#include "common.hpp"

namespace cmbl {

constexpr int NFFT_TILE = 16;                // largest tile edge of k_nfft_spread: NFFT_TILE^2 == NTP threads, one cell each
constexpr int NFFT_CHUNK = 64;               // nodes staged through LDS at a time
constexpr int NFFT_MAXW = 16;
constexpr double NFFT_BETA_PER_W = 2.3;
static_assert(NFFT_TILE * NFFT_TILE == NTP, "one thread per cell of a full tile");
template <typename T> struct NfftWidth { static constexpr int w = sizeof(T) == 4 ? 8 : 14; };   // from tests/golden/nfft_budget.json

// Tiles of one axis of n cells: nt = ceil(n / NFFT_TILE) tiles, tile a = [a n / nt, (a + 1) n / nt) (integer division).  Every edge is at most
// NFFT_TILE, and at least 8 unless the axis is one tile: never shorter than the reach w/2 <= 8 of a window, so the nodes that touch a tile
// lie in that tile or in one of its two (periodic) neighbours.
__host__ __device__ __forceinline__ int nfft_ntiles(int n) { return (n + NFFT_TILE - 1) / NFFT_TILE; }
__host__ __device__ __forceinline__ int nfft_tile_start(int a, int n, int nt) { return (int)(((long)a * n) / nt); }
__host__ __device__ __forceinline__ int nfft_tile_of(int k, int n, int nt) { return (int)((((long)k + 1) * nt - 1) / n); }

__host__ __device__ __forceinline__ double nfft_window(double t, int w) {
  const double z = 2.0 * t / (double)w, s = 1.0 - z * z;
  return s >= 0.0 ? exp(NFFT_BETA_PER_W * (double)w * (sqrt(s) - 1.0)) : 0.0;
}
// first cell of the window of a node at fine coordinate t (may be negative: the caller wraps)
__host__ __device__ __forceinline__ int nfft_first(double t, int w) { return (int)ceil(t - 0.5 * (double)w); }
__host__ __device__ __forceinline__ int nfft_wrap(int k, int n) { return k < 0 ? k + n : k >= n ? k - n : k; }   // k in [-n, 2n)

template <typename T> struct NfftNodes {     // the pixels of the patch, sorted by tile of the fine grid (stable: ascending pixel within a tile)
  const double* ty; const double* tx;        // fine coordinates, in [0, 2N - 2]
  const int* pix;                            // HEALPix pixel
  const T* c2; const T* s2;                  // cos 2 psi, sin 2 psi at the pixel
  const int* off;                            // CSR offsets: tile (a, b) = nodes off[b ntY + a] ... off[b ntY + a + 1]
  int n, Ny, Nx;                             // nodes; the COARSE sides
};
template <typename T> struct NfftModes {     // 1 / What(k / 2N) per axis, k = 0 ... N/2
  const T* dy; const T* dx;
};

// is (ky, lx) in I_Ny x I_Nx
__device__ __forceinline__ bool nfft_in_I(int ky, int lx, int Ny, int Nx) { return ky >= -(Ny / 2) && ky < Ny / 2 && lx >= -(Nx / 2) && lx < Nx / 2; }

// F: coarse half planes [Nx][Ny/2 + 1] (unnormalised rfft of the maps); G: fine half planes [2 Nx][Ny + 1].  Mode (ky, lx) of G, ky >= 0, is
//   scale * wgt * F[lx mod Nx][ky] / (What_y(ky) What_x(lx)),   wgt = ([l in I] + [-l in I]) / 2,
// the Hermitian form of sum_{l in I} c_l exp(2 pi i l x): each Nyquist mode of the coarse grid is split between +N/2 and -N/2, which is what
// makes the fine C2R return the real part (the cosine of the unpaired mode).  Everything else of G is zero.
// grid (ceil(2 Nx (Ny + 1) / NTP), slices)
template <typename T>
__global__ __launch_bounds__(NTP) void k_nfft_embed(const cx<T>* __restrict__ F, cx<T>* __restrict__ G, const NfftModes<T> md, int Ny, int Nx, T scale) {
  const int nyh = Ny / 2 + 1, fyh = Ny + 1;
  const long e = (long)blockIdx.x * NTP + threadIdx.x, fplane = (long)2 * Nx * fyh;
  if (e >= fplane) return;
  const int sx = (int)(e / fyh), ky = (int)(e - (long)sx * fyh);
  const int lx = sx < Nx ? sx : sx - 2 * Nx;
  cx<T> v = mk<T>(0, 0);
  if (ky <= Ny / 2 && lx >= -(Nx / 2) && lx <= Nx / 2) {
    const T wgt = (T)0.5 * (T)((nfft_in_I(ky, lx, Ny, Nx) ? 1 : 0) + (nfft_in_I(-ky, -lx, Ny, Nx) ? 1 : 0));
    const int xs = lx < 0 ? lx + Nx : lx;                                   // lx = +Nx/2 and -Nx/2 read the one Nyquist slot
    const cx<T> f = F[(long)blockIdx.y * Nx * nyh + (long)xs * nyh + ky];
    v = (scale * wgt * md.dy[ky] * md.dx[lx < 0 ? -lx : lx]) * f;
  }
  G[(long)blockIdx.y * fplane + e] = v;
}

// fine maps (2Ny, 2Nx, npol, nbatch) -> HEALPix (npix, npol, nbatch), which the host has zeroed: one thread per node, the 2 w window values in
// registers, reused over all slices.  Each value is sum_dx wx[dx] (sum_dy wy[dy] g[x][y]) in that order.  QU as in :332-333:
// Q' = Q cos 2 psi + U sin 2 psi, U' = U cos 2 psi - Q sin 2 psi.  ROT = false (the transpose of to_cart, whose rotation sits at the Cartesian
// pixels): no rotation.  grid ceil(n / NTP)
template <typename T, int W, bool ROT = true>
__global__ __launch_bounds__(NTP) void k_nfft_interp(const T* __restrict__ fine, T* __restrict__ hpx, const NfftNodes<T> nd, long npix, int npol, int nbatch) {
  const int s = blockIdx.x * NTP + threadIdx.x;
  if (s >= nd.n) return;
  const int ny = 2 * nd.Ny, nx = 2 * nd.Nx;
  const double ty = nd.ty[s], tx = nd.tx[s];
  const int k0y = nfft_first(ty, W), k0x = nfft_first(tx, W);
  T wy[W], wx[W];
  int iy[W];
#pragma unroll
  for (int d = 0; d < W; ++d) {
    wy[d] = (T)nfft_window((double)(k0y + d) - ty, W);
    wx[d] = (T)nfft_window((double)(k0x + d) - tx, W);
    iy[d] = nfft_wrap(k0y + d, ny);
  }
  const long p = nd.pix[s], nfine = (long)ny * nx;
  const T cc = nd.c2[s], ss = nd.s2[s];
  auto val = [&](const T* g) {
    T acc = 0;
#pragma unroll
    for (int dx = 0; dx < W; ++dx) {
      const T* col = g + (long)nfft_wrap(k0x + dx, nx) * ny;
      T in = 0;
#pragma unroll
      for (int dy = 0; dy < W; ++dy) in = fma(wy[dy], col[iy[dy]], in);
      acc = fma(wx[dx], in, acc);
    }
    return acc;
  };
  for (int b = 0; b < nbatch; ++b) {
    const T* gb = fine + (long)b * npol * nfine;
    T* hb = hpx + (long)b * npol * npix + p;
    int q = 0;
    if (npol != 2) { hb[0] = val(gb); q = 1; }
    if (npol >= 2) {
      const T Q = val(gb + (long)q * nfine), U = val(gb + (long)(q + 1) * nfine);
      hb[(long)q * npix] = ROT ? fma(U, ss, Q * cc) : Q;
      hb[(long)(q + 1) * npix] = ROT ? fma(-Q, ss, U * cc) : U;
    }
  }
}

// HEALPix (npix, npol, nbatch) -> fine maps (2Ny, 2Nx, npol, nbatch): fine[c] = sum_p h_p Wy(cy - ty_p) Wx(cx - tx_p), periodic.  Workgroup
// (tile, batch): thread (ly, lx) owns cell (y0 + ly, x0 + lx) of the tile and up to three accumulators (the npol planes of the batch entry).
// It walks the nodes of the distinct tiles among the tile's 3 x 3 periodic neighbourhood in a fixed order (x offset outer, y offset inner,
// nodes ascending) as ONE list -- the up to nine CSR ranges end to end -- NFFT_CHUNK at a time: the workgroup stages first cell, the 2 W window
// values and the npol values of each node of the chunk in LDS, then every cell adds the nodes whose window covers it.  A cell's distance from a node's first cell is taken modulo the grid,
// so a window that wraps, and a grid of fewer than three tiles, need no special case.  Every cell of the grid is written once (zeros included).
// ROT (the transpose of to_healpix): QU are rotated as they are staged, by the transpose of :332-333 at the node,
// Q' = Q cos 2 psi - U sin 2 psi, U' = U cos 2 psi + Q sin 2 psi.
// grid (ntY ntX, nbatch)
template <typename T, int W, bool ROT = false>
__global__ __launch_bounds__(NTP) void k_nfft_spread(const T* __restrict__ hpx, T* __restrict__ fine, const NfftNodes<T> nd, long npix, int npol) {
  __shared__ T swy[NFFT_CHUNK][W], swx[NFFT_CHUNK][W], sval[3][NFFT_CHUNK];
  __shared__ int sk0y[NFFT_CHUNK], sk0x[NFFT_CHUNK];
  __shared__ int rbeg[9], rpre[10];                                        // the ranges: first slot, and the exclusive prefix of their lengths
  const int ny = 2 * nd.Ny, nx = 2 * nd.Nx, ntY = nfft_ntiles(ny), ntX = nfft_ntiles(nx);
  const int a = blockIdx.x % ntY, bt = blockIdx.x / ntY, t = threadIdx.x;
  const int y0 = nfft_tile_start(a, ny, ntY), hy = nfft_tile_start(a + 1, ny, ntY) - y0;
  const int x0 = nfft_tile_start(bt, nx, ntX), hx = nfft_tile_start(bt + 1, nx, ntX) - x0;
  const int ly = t % NFFT_TILE, lx = t / NFFT_TILE, cy = y0 + ly, cx = x0 + lx;
  const bool active = ly < hy && lx < hx;
  const T* hb = hpx + (long)blockIdx.y * npol * npix;
  T acc[3] = {0, 0, 0};
  const int nay = ntY < 3 ? ntY : 3, nax = ntX < 3 ? ntX : 3;             // distinct neighbours per axis
  const int nr = nay * nax;
  if (t == 0) {
    rpre[0] = 0;
    for (int ox = 0; ox < nax; ++ox)
      for (int oy = 0; oy < nay; ++oy) {
        const int sa = (a + (nay == 3 ? oy - 1 : oy) + ntY) % ntY, sb = (bt + (nax == 3 ? ox - 1 : ox) + ntX) % ntX, r = ox * nay + oy;
        rbeg[r] = nd.off[sb * ntY + sa];
        rpre[r + 1] = rpre[r] + (nd.off[sb * ntY + sa + 1] - rbeg[r]);
      }
  }
  __syncthreads();
  const int total = rpre[nr];
  auto slot_of = [&](int e) { int r = 0; while (e >= rpre[r + 1]) ++r; return rbeg[r] + (e - rpre[r]); };   // e < total: ends within the nr ranges
  for (int c0 = 0; c0 < total; c0 += NFFT_CHUNK) {
    const int cn = total - c0 < NFFT_CHUNK ? total - c0 : NFFT_CHUNK;
    __syncthreads();                                                        // the previous chunk has been consumed
    for (int e = t; e < cn * 2 * W; e += NTP) {
      const int q = e / (2 * W), r = e - q * 2 * W, ax = r / W, d = r - ax * W, s = slot_of(c0 + q);
      const double tt = ax ? nd.tx[s] : nd.ty[s];
      const int k0 = nfft_first(tt, W);
      const T v = (T)nfft_window((double)(k0 + d) - tt, W);
      if (ax) swx[q][d] = v; else swy[q][d] = v;
      if (d == 0) { if (ax) sk0x[q] = k0; else sk0y[q] = k0; }
    }
    if (ROT && npol >= 2) {
      for (int q = t; q < cn; q += NTP) {
        const int s = slot_of(c0 + q);
        const long p = nd.pix[s];
        if (npol == 3) sval[0][q] = hb[p];
        const T Q = hb[(long)(npol - 2) * npix + p], U = hb[(long)(npol - 1) * npix + p], cc = nd.c2[s], ss = nd.s2[s];
        sval[npol - 2][q] = fma(-U, ss, Q * cc);
        sval[npol - 1][q] = fma(Q, ss, U * cc);
      }
    } else
      for (int e = t; e < cn * npol; e += NTP) {
        const int k = e / cn, q = e - k * cn;
        sval[k][q] = hb[(long)k * npix + nd.pix[slot_of(c0 + q)]];
      }
    __syncthreads();
    if (active)
      for (int q = 0; q < cn; ++q) {
        const int dy = nfft_wrap(cy - sk0y[q], ny), dx = nfft_wrap(cx - sk0x[q], nx);
        if (dy < W && dx < W) {
          const T wgt = swy[q][dy] * swx[q][dx];
          for (int k = 0; k < npol; ++k) acc[k] = fma(wgt, sval[k][q], acc[k]);
        }
      }
  }
  if (active)
    for (int k = 0; k < npol; ++k) fine[((long)blockIdx.y * npol + k) * ny * nx + (long)cx * ny + cy] = acc[k];
}

// G: fine half planes [2 Nx][Ny + 1] (unnormalised rfft of the spread grid); A: coarse half planes [Nx][Ny/2 + 1].  With
// Hhat(ky, lx) = G[lx mod 2Nx][ky] / (What_y(ky) What_x(lx)) for ky >= 0 and Hhat(-ky, lx) = conj Hhat(ky, -lx), slot (ky, sx) of A is
//   scale * (Hhat(ky-, lx-) + Hhat(ky+, lx+)) / 2,
// (ky-, lx-) the slot's signed mode with Nyquist taken as -N/2 and (ky+, lx+) with Nyquist taken as +N/2: the Hermitian part of
// sum_{l in I} Hhat_l exp(2 pi i l g / N), so that the coarse C2R returns the real part.  The transpose of k_nfft_embed.
// grid (ceil(Nx (Ny/2 + 1) / NTP), slices)
template <typename T>
__global__ __launch_bounds__(NTP) void k_nfft_extract(const cx<T>* __restrict__ G, cx<T>* __restrict__ A, const NfftModes<T> md, int Ny, int Nx, T scale) {
  const int nyh = Ny / 2 + 1, fyh = Ny + 1;
  const long e = (long)blockIdx.x * NTP + threadIdx.x, plane = (long)Nx * nyh;
  if (e >= plane) return;
  const int sx = (int)(e / nyh), ky = (int)(e - (long)sx * nyh);
  const cx<T>* g = G + (long)blockIdx.y * 2 * Nx * fyh;
  auto Hhat = [&](int k, int l) {
    const bool neg = k < 0;
    const int kk = neg ? -k : k, ll = neg ? -l : l;
    const cx<T> v = g[(long)(ll < 0 ? ll + 2 * Nx : ll) * fyh + kk];
    return (md.dy[kk] * md.dx[l < 0 ? -l : l]) * (neg ? conj(v) : v);
  };
  const int lxm = sx < Nx / 2 ? sx : sx - Nx, lxp = sx <= Nx / 2 ? sx : sx - Nx, kym = ky < Ny / 2 ? ky : -(Ny / 2);
  const cx<T> hm = Hhat(kym, lxm), hp = Hhat(ky, lxp);
  A[(long)blockIdx.y * plane + e] = (scale * (T)0.5) * (hm + hp);
}

// maps (Ny Nx, npol, nbatch), src -> dst (the same array: in place): Q' = Q cos 2 psi - U sin 2 psi, U' = U cos 2 psi + Q sin 2 psi (:243-244).
// ADJ: the transpose, Q' = Q cos 2 psi + U sin 2 psi, U' = U cos 2 psi - Q sin 2 psi, into another array, the I plane of npol = 3 copied.
// grid (ceil(Ny Nx / NTP), nbatch)
template <typename T, bool ADJ = false>
__global__ __launch_bounds__(NTP) void k_nfft_rot_cart(const T* src, T* dst, const T* __restrict__ c2, const T* __restrict__ s2, long ncart, int npol) {
  const long c = (long)blockIdx.x * NTP + threadIdx.x;
  if (c >= ncart) return;
  const long o = ((long)blockIdx.y * npol + (npol - 2)) * ncart + c;
  const T Q = src[o], U = src[o + ncart], cc = c2[c], ss = s2[c];
  dst[o] = ADJ ? fma(U, ss, Q * cc) : fma(-U, ss, Q * cc);
  dst[o + ncart] = ADJ ? fma(-Q, ss, U * cc) : fma(Q, ss, U * cc);
  if (ADJ && npol == 3) dst[o - ncart] = src[o - ncart];
}

}  // namespace cmbl
