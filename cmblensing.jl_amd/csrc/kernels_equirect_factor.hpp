// BlockDiagEquiRect factorisations (src/proj_equirect.jl:274-282, 313-347): the kernels behind cmbl_equirect_block_svd / _logabsdet / _solve.
// Blocks are `blocks` (n, n, Nx/2+1) with the row index p contiguous, so a matrix COLUMN is contiguous.  ALL arithmetic is double (real or complex
// double, EqfD) whatever the storage type; the storage type T / cx<T> appears in loads and in the final stores only (the double-precision rule of
// Cl_to_Cov).  One workgroup owns one block for a whole factorisation; it synchronises with the workgroup barrier alone -- no flag,
// no grid barrier, no spin wait, no atomic -- and every loop bound is known at launch (n, or EQF_SWEEPS), so no input can make a launch hang.
// One writer per element and a fixed order of operations: results are bit-identical between runs and for every slab size.
//   k_eqf_nonfinite   does an array hold a value that is not finite?  one flag per workgroup, the host reads them
//   k_eqf_jacobi      one-sided (Hestenes) Jacobi SVD: G = A, V = I, column pairs rotated until orthogonal; sigma and the two weight rows
//   k_eqf_assemble    out = X diag(w) Y^H: sqrt = G diag(sigma^-1/2) V^H and pinv = V diag(sigma^-2, cut) G^H
//   k_eqf_lu          right-looking LU with partial pivoting, panels of EQF_NB columns, the trailing update a rank-EQF_NB product staged in LDS
//   k_eqf_solve       forward and back substitution, one wavefront per right-hand side
#pragma once
#include "kernels_equirect.hpp"

namespace cmbl {

constexpr int EQF_NMAX = 2048;     // largest block size the device path takes
constexpr int EQF_SWEEPS = 60;     // sweep cap of the Jacobi iteration (a condition of termination, not a tuning result)
constexpr int EQF_JT = 1024;       // threads of k_eqf_jacobi: 16 wavefronts share the n/2 disjoint pairs of a round
constexpr int EQF_NB = 16;         // panel width of k_eqf_lu
constexpr int EQF_TL = 64;         // tile side of its trailing update
constexpr int EQF_RT = NTP / 64;   // right-hand sides per workgroup of k_eqf_solve (one per wavefront)

template <bool CPLX> struct EqfD { using type = double; };
template <> struct EqfD<true> { using type = cx<double>; };

__device__ __forceinline__ double eqf_abs2(double a) { return a * a; }
__device__ __forceinline__ double eqf_abs2(cx<double> a) { return a.x * a.x + a.y * a.y; }
__device__ __forceinline__ double eqf_conj(double a) { return a; }
__device__ __forceinline__ cx<double> eqf_conj(cx<double> a) { return conj(a); }
// a / b; the complex quotient by Smith's rule (no overflow of |b|^2)
__device__ __forceinline__ double eqf_div(double a, double b) { return a / b; }
__device__ __forceinline__ cx<double> eqf_div(cx<double> a, double b) { return mk<double>(a.x / b, a.y / b); }
__device__ __forceinline__ cx<double> eqf_div(cx<double> a, cx<double> b) {
  if (fabs(b.x) >= fabs(b.y)) { const double r = b.y / b.x, d = b.x + b.y * r; return mk<double>((a.x + a.y * r) / d, (a.y - a.x * r) / d); }
  const double r = b.x / b.y, d = b.x * r + b.y;
  return mk<double>((a.x * r + a.y) / d, (a.y * r - a.x) / d);
}
// storage -> double on the way in, double -> storage at the final store (the only rounding)
template <bool CPLX, typename S> __device__ __forceinline__ typename EqfD<CPLX>::type eqf_ld(S v) {
  if constexpr (CPLX) return mk<double>((double)eq_re(v), (double)eq_im(v)); else return (double)eq_re(v);
}
template <typename T, bool CPLX, typename D> __device__ __forceinline__ typename EqElem<T, CPLX>::type eqf_round(D v) {
  if constexpr (CPLX) return mk<T>((T)eq_re(v), (T)eq_im(v)); else return (T)eq_re(v);
}
// butterfly sum over the 64 lanes: every lane ends with the same bits (a + b == b + a at every stage)
__device__ __forceinline__ double eqf_wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- finite check ----------------------------------------------------------------------------------------------------------------------------
// a: nreal scalars (a complex array counts twice).  flags[blockIdx.x] = 1 when the workgroup met a NaN or an infinity.  grid: any, grid-stride
template <typename T>
__global__ __launch_bounds__(NTP) void k_eqf_nonfinite(const T* __restrict__ a, long nreal, int* __restrict__ flags) {
  int bad = 0;
  for (long i = (long)blockIdx.x * NTP + threadIdx.x; i < nreal; i += (long)gridDim.x * NTP) bad |= !isfinite((double)a[i]);
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) flags[blockIdx.x] = bad;
}

// ---- one-sided Jacobi SVD --------------------------------------------------------------------------------------------------------------------
// Round-robin schedule over np = n + (n & 1) columns (an odd n gets a dummy column np - 1): R = np - 1 rounds of np / 2 disjoint pairs; in round r
// pair 0 is (np - 1, r) and pair k >= 1 is ((r + k) mod R, (r - k) mod R): every pair once per sweep.
__device__ __forceinline__ void eqf_pair(int np, int r, int k, int& i, int& j) {
  const int R = np - 1;
  const int a = k == 0 ? np - 1 : (r + k) % R, b = k == 0 ? r : (r + R - k) % R;
  i = min(a, b); j = max(a, b);
}
// One workgroup per block m0 + blockIdx.x, working copies G, V (n x n doubles / complex doubles each) at slab slot blockIdx.x.  A pair (i, j), i < j,
// belongs to one wavefront: alpha = |g_i|^2, beta = |g_j|^2, gamma = g_i^H g_j by wave reductions along the contiguous columns; it is SKIPPED when
// alpha, beta or gamma is exactly zero, when alpha and beta both lie at or below the noise floor (n 2^-53)^2 |A|_F^2 of the block (null-space columns
// hold rounding noise of that size; rotating them among themselves would never settle), when alpha or beta lies at or below the dead level
// (2^-53)^4 |A|_F^2 (a column of norm 2^-106 |A|_F adds at most 2^-53 |A|_F^1/2 to sqrt whatever its direction and is cut from pinv; in a block with
// exactly proportional rows a noise column can never leave the span of the others, shrinks by 2^-53 per sweep and would otherwise be rotated until
// it underflows), or when |gamma| <= n 2^-53 sqrt(alpha beta); otherwise
// columns i, j of G and V are multiplied by the unitary [c, s ph; -s conj(ph), c], ph = gamma / |gamma|.  Sweeps repeat until one rotates nothing
// or EQF_SWEEPS.  Then sigma[k] = |g_k|, wts[0][k] = sigma^-1/2 (0 where sigma == 0) and wts[1][k] = sigma^-2 (0 where sigma <= rtol max sigma);
// status = (sweeps run, converged).
template <typename T, bool CPLX>
__global__ __launch_bounds__(EQF_JT) void k_eqf_jacobi(const typename EqElem<T, CPLX>::type* __restrict__ A, int n, int m0, typename EqfD<CPLX>::type* Gs,
                                                      typename EqfD<CPLX>::type* Vs, double* sigma, double* wts, int* status, double rtol) {
  using D = typename EqfD<CPLX>::type;
  constexpr int NW = EQF_JT / 64;
  __shared__ double s_red[NW];
  __shared__ int s_rot;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, m = m0 + (int)blockIdx.x;
  const size_t nn = (size_t)n * n;
  const typename EqElem<T, CPLX>::type* Am = A + (size_t)m * nn;
  D* G = Gs + (size_t)blockIdx.x * nn; D* V = Vs + (size_t)blockIdx.x * nn;
  double fro = 0;
  for (size_t i = t; i < nn; i += EQF_JT) {
    const D v = eqf_ld<CPLX>(Am[i]);
    G[i] = v;
    D e = eq_zero<D>();
    if (i / n == i % n) e = eqf_ld<CPLX>(1.0);
    V[i] = e;
    fro += eqf_abs2(v);
  }
  fro = eqf_wsum(fro);
  if (lane == 0) s_red[w] = fro;
  __syncthreads();
  fro = 0;
  for (int k = 0; k < NW; ++k) fro += s_red[k];
  const double tol = (double)n * 0x1p-53, floor2 = tol * tol * fro, dead2 = 0x1p-212 * fro;
  const int np = n + (n & 1);
  int sweeps = 0, converged = 0;
  for (int sweep = 0; sweep < EQF_SWEEPS; ++sweep) {
    __syncthreads();
    if (t == 0) s_rot = 0;
    __syncthreads();
    for (int r = 0; r < np - 1; ++r) {
      for (int k = w; k < np / 2; k += NW) {
        int i, j;
        eqf_pair(np, r, k, i, j);
        if (j >= n) continue;                                                // the dummy column of an odd n
        D* gi = G + (size_t)i * n; D* gj = G + (size_t)j * n;
        double al = 0, be = 0, gr = 0, gim = 0;
        for (int q = lane; q < n; q += 64) {
          const D x = gi[q], y = gj[q];
          al += eqf_abs2(x); be += eqf_abs2(y);
          const D p = eqf_conj(x) * y;
          gr += eq_re(p); gim += eq_im(p);
        }
        al = eqf_wsum(al); be = eqf_wsum(be); gr = eqf_wsum(gr);
        if constexpr (CPLX) gim = eqf_wsum(gim);
        const double ag = CPLX ? sqrt(gr * gr + gim * gim) : fabs(gr);
        if (al == 0.0 || be == 0.0 || ag == 0.0) continue;
        if ((al <= floor2 && be <= floor2) || al <= dead2 || be <= dead2) continue;
        if (!(ag > tol * sqrt(al * be))) continue;
        const double zeta = (be - al) / (2.0 * ag);
        const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
        D ph;
        if constexpr (CPLX) ph = mk<double>(gr / ag, gim / ag); else ph = gr / ag;
        const D sp = sn * ph, spc = sn * eqf_conj(ph);
        for (int q = lane; q < n; q += 64) {
          const D x = gi[q], y = gj[q];
          gi[q] = cs * x - spc * y;
          gj[q] = sp * x + cs * y;
        }
        D* vi = V + (size_t)i * n; D* vj = V + (size_t)j * n;
        for (int q = lane; q < n; q += 64) {
          const D x = vi[q], y = vj[q];
          vi[q] = cs * x - spc * y;
          vj[q] = sp * x + cs * y;
        }
        if (lane == 0) s_rot = 1;                                            // (every writer stores the same value)
      }
      __syncthreads();                                                       // the next round pairs columns other wavefronts wrote
    }
    ++sweeps;
    if (s_rot == 0) { converged = 1; break; }                                // uniform: read after the barrier that ended the last round
  }
  __syncthreads();
  double* sg = sigma + (size_t)m * n;
  double smax = 0;
  for (int k = w; k < n; k += NW) {
    const D* gk = G + (size_t)k * n;
    double a = 0;
    for (int q = lane; q < n; q += 64) a += eqf_abs2(gk[q]);
    a = sqrt(eqf_wsum(a));
    if (lane == 0) sg[k] = a;
    smax = fmax(smax, a);
  }
  if (lane == 0) s_red[w] = smax;
  __syncthreads();
  smax = 0;
  for (int k = 0; k < NW; ++k) smax = fmax(smax, s_red[k]);
  double* ws = wts + (size_t)m * 2 * n;
  for (int k = t; k < n; k += EQF_JT) {
    const double s = sg[k];
    ws[k] = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
    ws[n + k] = s > rtol * smax ? 1.0 / (s * s) : 0.0;
  }
  if (t == 0) { status[2 * m] = sweeps; status[2 * m + 1] = converged; }
}

// out[m0 + z][q][p] = sum_k X[p, k] w[k] conj(Y[q, k]), k ascending, rounded to the storage type at the store.  X, Y: slab slot z; w: row
// `wrow` (0 sqrt, 1 pinv) of the block's weights.  A workgroup makes a 32 x 32 tile; both operand tiles go through LDS.  grid (ceil(n / 32),
// ceil(n / 32), blocks of the slab)
template <typename T, bool CPLX>
__global__ __launch_bounds__(NTP) void k_eqf_assemble(const typename EqfD<CPLX>::type* __restrict__ Xs, const typename EqfD<CPLX>::type* __restrict__ Ys,
                                                     const double* __restrict__ wts, int wrow, typename EqElem<T, CPLX>::type* __restrict__ out, int n, int m0) {
  using D = typename EqfD<CPLX>::type;
  __shared__ D sx[32][33], sy[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, p0 = blockIdx.x * 32, q0 = blockIdx.y * 32, m = m0 + (int)blockIdx.z;
  const size_t nn = (size_t)n * n;
  const D* X = Xs + (size_t)blockIdx.z * nn; const D* Y = Ys + (size_t)blockIdx.z * nn;
  const double* wv = wts + ((size_t)m * 2 + wrow) * n;
  D acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = eq_zero<D>();
  for (int k0 = 0; k0 < n; k0 += 32) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kk = ty + 8 * i, k = k0 + kk, p = p0 + tx, q = q0 + tx;
      sx[kk][tx] = (k < n && p < n) ? wv[k] * X[(size_t)k * n + p] : eq_zero<D>();
      sy[kk][tx] = (k < n && q < n) ? eqf_conj(Y[(size_t)k * n + q]) : eq_zero<D>();
    }
    __syncthreads();
    for (int kk = 0; kk < 32; ++kk) {
      const D x = sx[kk][tx];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = acc[i] + x * sy[kk][ty + 8 * i];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = p0 + tx, q = q0 + ty + 8 * i;
    if (p < n && q < n) out[(size_t)m * nn + (size_t)q * n + p] = eqf_round<T, CPLX>(acc[i]);
  }
}

// ---- LU with partial pivoting ----------------------------------------------------------------------------------------------------------------
// One workgroup per block.  W (slab slot blockIdx.x) starts as A, or as A^H (conjT: element [p, q] = conj(A[q, p]), for the right-hand solve), and
// ends as L (unit lower, below the diagonal) and U.  Per panel of EQF_NB columns: column by column the pivot (largest modulus at or below the
// diagonal, a tie to the lowest row), the swap of the two whole rows, the scaling of the column and the rank-1 update of the rest of the PANEL;
// then the rows of U right of the panel (a triangular solve with the panel's unit L, one thread per column), then the trailing matrix minus
// L21 U12 as EQF_TL x EQF_TL tiles, both EQF_NB-deep operand tiles staged in LDS (2 x 16 x 64 elements: 16 KiB real, 32 KiB complex, of the
// 160 KiB of a CU), the sum over the panel index ascending in plain double FMAs.  The trailing matrix is so read and written n / EQF_NB times.
// A zero pivot (the whole column at and below the diagonal is exactly 0) leaves the column as it is and records info = column + 1 (the first one).
// perm[i]: the row of A that ended up in row i; parity: of the swaps; dg: the diagonal of U.
template <typename T, bool CPLX>
__global__ __launch_bounds__(NTP) void k_eqf_lu(const typename EqElem<T, CPLX>::type* __restrict__ A, int n, int m0, int conjT, typename EqfD<CPLX>::type* Ws,
                                               int* perms, typename EqfD<CPLX>::type* dg, int* info, int* parity) {
  using D = typename EqfD<CPLX>::type;
  __shared__ D sL[EQF_NB][EQF_TL], sU[EQF_NB][EQF_TL], sT[EQF_NB][EQF_NB];
  __shared__ double s_val[NTP / 64];
  __shared__ int s_idx[NTP / 64], s_info, s_par;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, m = m0 + (int)blockIdx.x;
  const size_t nn = (size_t)n * n;
  const typename EqElem<T, CPLX>::type* Am = A + (size_t)m * nn;
  D* W = Ws + (size_t)blockIdx.x * nn;
  int* perm = perms + (size_t)blockIdx.x * n;
  for (size_t i = t; i < nn; i += NTP) {
    if (conjT) { const size_t q = i / n, p = i % n; W[i] = eqf_conj(eqf_ld<CPLX>(Am[p * n + q])); }
    else W[i] = eqf_ld<CPLX>(Am[i]);
  }
  for (int i = t; i < n; i += NTP) perm[i] = i;
  if (t == 0) { s_info = 0; s_par = 0; }
  __syncthreads();
  for (int k0 = 0; k0 < n; k0 += EQF_NB) {
    const int kb = min(EQF_NB, n - k0), k1 = k0 + kb;
    for (int j = k0; j < k1; ++j) {
      D* cj = W + (size_t)j * n;
      double best = -1.0; int bi = n;
      for (int r = j + t; r < n; r += NTP) { const double v = eqf_abs2(cj[r]); if (v > best) { best = v; bi = r; } }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
      }
      if (lane == 0) { s_val[w] = best; s_idx[w] = bi; }
      __syncthreads();
      best = s_val[0]; bi = s_idx[0];
      for (int k = 1; k < NTP / 64; ++k) if (s_val[k] > best || (s_val[k] == best && s_idx[k] < bi)) { best = s_val[k]; bi = s_idx[k]; }
      const int piv = bi < n ? bi : j;                                       // uniform; j <= piv < n (row j always competes; an overflowed column of NaNs keeps row j)
      const D pv = cj[piv];
      const bool zero = !(best > 0.0);
      __syncthreads();                                                       // pv has been read before the swap moves it
      if (piv != j) {
        for (int c = t; c < n; c += NTP) { D* col = W + (size_t)c * n; const D a = col[j]; col[j] = col[piv]; col[piv] = a; }
        if (t == 0) { const int a = perm[j]; perm[j] = perm[piv]; perm[piv] = a; s_par ^= 1; }
      }
      if (zero && t == 0 && s_info == 0) s_info = j + 1;
      __syncthreads();
      if (!zero) {
        for (int r = j + 1 + t; r < n; r += NTP) cj[r] = eqf_div(cj[r], pv);
        __syncthreads();
        const int rows = n - j - 1, cols = k1 - 1 - j;
        for (long idx = t; idx < (long)rows * cols; idx += NTP) {
          const int c = j + 1 + (int)(idx / rows), r = j + 1 + (int)(idx % rows);
          D* col = W + (size_t)c * n;
          col[r] = col[r] - cj[r] * col[j];
        }
        __syncthreads();
      }
    }
    if (k1 >= n) break;
    // U12 = L11^-1 A12: the unit lower triangle of the panel through LDS, one thread per column right of the panel
    for (int i = t; i < EQF_NB * EQF_NB; i += NTP) {
      const int a = i % EQF_NB, b = i / EQF_NB;                              // sT[b][a] = L[k0 + a, k0 + b]
      sT[b][a] = (a < kb && b < a) ? W[(size_t)(k0 + b) * n + k0 + a] : eq_zero<D>();
    }
    __syncthreads();
    for (int c = k1 + t; c < n; c += NTP) {
      D* col = W + (size_t)c * n + k0;
      D x[EQF_NB];
#pragma unroll
      for (int a = 0; a < EQF_NB; ++a) x[a] = a < kb ? col[a] : eq_zero<D>();
#pragma unroll
      for (int a = 1; a < EQF_NB; ++a) {
#pragma unroll
        for (int b = 0; b < a; ++b) x[a] = x[a] - sT[b][a] * x[b];
      }
#pragma unroll
      for (int a = 1; a < EQF_NB; ++a) if (a < kb) col[a] = x[a];
    }
    __syncthreads();
    // A22 -= L21 U12
    const int tr = t & 15, tc = t >> 4;
    for (int r0 = k1; r0 < n; r0 += EQF_TL) {
      __syncthreads();
      for (int i = t; i < EQF_NB * EQF_TL; i += NTP) {
        const int rr = i % EQF_TL, kk = i / EQF_TL;
        sL[kk][rr] = (kk < kb && r0 + rr < n) ? W[(size_t)(k0 + kk) * n + r0 + rr] : eq_zero<D>();
      }
      for (int c0 = k1; c0 < n; c0 += EQF_TL) {
        __syncthreads();
        for (int i = t; i < EQF_NB * EQF_TL; i += NTP) {
          const int kk = i % EQF_NB, cc = i / EQF_NB;
          sU[kk][cc] = (kk < kb && c0 + cc < n) ? W[(size_t)(c0 + cc) * n + k0 + kk] : eq_zero<D>();
        }
        __syncthreads();
        D acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = eq_zero<D>();
#pragma unroll 4
        for (int kk = 0; kk < EQF_NB; ++kk) {
          D l[4], u[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) { l[a] = sL[kk][tr + 16 * a]; u[a] = sU[kk][tc + 16 * a]; }
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = acc[a][b] + l[a] * u[b];
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int c = c0 + tc + 16 * b;
          if (c >= n) continue;
          D* col = W + (size_t)c * n;
#pragma unroll
          for (int a = 0; a < 4; ++a) { const int r = r0 + tr + 16 * a; if (r < n) col[r] = col[r] - acc[a][b]; }
        }
      }
    }
    __syncthreads();
  }
  __syncthreads();
  for (int k = t; k < n; k += NTP) dg[(size_t)m * n + k] = W[(size_t)k * n + k];
  if (t == 0) { info[m] = s_info; parity[m] = s_par; }
}

// ---- triangular solves -----------------------------------------------------------------------------------------------------------------------
// One wavefront per right-hand side, EQF_RT of them per workgroup: x = P b, then L x = x (unit L) and U x = x, column-oriented, the lanes along the
// rows; x lives in the double scratch Xs (slab slot, right-hand side) until the final store rounds it.  Element i of right-hand side c of block m is
// rhs[m * sm + c * sc + i * se], conjugated when cj (the right-hand solve reads and writes conjugate-transposed); `out` has the same strides.
// grid (ceil(nrhs / EQF_RT), blocks of the slab)
template <typename T, bool ACPLX, bool RCPLX>
__global__ __launch_bounds__(NTP) void k_eqf_solve(const typename EqfD<ACPLX>::type* __restrict__ Ws, const int* __restrict__ perms, int n, int m0,
                                                  const typename EqElem<T, RCPLX>::type* __restrict__ rhs, long sm, long sc, long se, int cj, int nrhs,
                                                  typename EqfD<ACPLX || RCPLX>::type* Xs, typename EqElem<T, ACPLX || RCPLX>::type* __restrict__ out) {
  constexpr bool OC = ACPLX || RCPLX;
  using AD = typename EqfD<ACPLX>::type;
  using XD = typename EqfD<OC>::type;
  const int lane = threadIdx.x & 63, col = (int)blockIdx.x * EQF_RT + ((int)threadIdx.x >> 6), m = m0 + (int)blockIdx.y;
  const bool valid = col < nrhs;
  const AD* W = Ws + (size_t)blockIdx.y * n * n;
  const int* perm = perms + (size_t)blockIdx.y * n;
  XD* x = Xs + ((size_t)blockIdx.y * nrhs + (valid ? col : 0)) * n;
  const long base = (long)m * sm + (long)col * sc;
  if (valid)
    for (int i = lane; i < n; i += 64) {
      XD v;
      if constexpr (OC) v = mk<double>((double)eq_re(rhs[base + perm[i] * se]), (double)eq_im(rhs[base + perm[i] * se]));
      else v = (double)eq_re(rhs[base + perm[i] * se]);
      x[i] = cj ? eqf_conj(v) : v;
    }
  __syncthreads();
  for (int k = 0; k < n; ++k) {
    if (valid) {
      const XD xk = x[k];
      const AD* ck = W + (size_t)k * n;
      for (int i = k + 1 + lane; i < n; i += 64) x[i] = x[i] - ck[i] * xk;
    }
    __syncthreads();
  }
  for (int k = n - 1; k >= 0; --k) {
    if (valid) {
      const AD* ck = W + (size_t)k * n;
      const XD xk = eqf_div(x[k], ck[k]);                                     // every lane reads x[k] before lane 0 overwrites it (one instruction stream)
      if (lane == 0) x[k] = xk;
      for (int i = lane; i < k; i += 64) x[i] = x[i] - ck[i] * xk;
    }
    __syncthreads();
  }
  if (valid)
    for (int i = lane; i < n; i += 64) out[base + i * se] = eqf_round<T, OC>(cj ? eqf_conj(x[i]) : x[i]);
}

}  // namespace cmbl
