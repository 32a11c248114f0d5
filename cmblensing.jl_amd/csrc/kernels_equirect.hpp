// ProjEquiRect (src/proj_equirect.jl): the kernels behind cmbl_equirect_*.  Arrays are the reference's, column-major: maps (Ny, Nx, [2,] B) with
// theta contiguous, AzFourier fields (n, Nx/2+1, B) complex with n = Ny (I) or 2 Ny (QU), operators `blocks` (n, n, Nx/2+1) with the row index p
// contiguous, real T or cx<T>.  No atomics; every output element has one writer and one fixed order of operations, so results are bit-identical
// between runs.
//   k_eq_qu_pack      QUAzFourier (:160-168) after the transforms of Q and U: top rows F = FQ + i FU, bottom rows conj(F[(Nx - m) mod Nx]) = FQ - i FU
//   k_eq_qu_unpack    QUMap (:170-178) before the inverse transform: the full spectrum F (Ny, Nx), "second assignment wins" at columns 0 and Nx/2
//   k_eq_apply        M * f and M' * f (:230-240)
//   k_eq_matmul       M1 * M2, M1' * M2, M1 * M2' (:254-269) on the matrix cores (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64)
//   k_eq_dot_part, k_eq_dot_sum   dot(M1', M2) (:358-360), two stages in double
//   k_eq_scale_cols   blocks[j, k, m] *= w[k] (Cl_to_Beam(:I), :505-515)
//   k_eq_beam_pol     [B 0; 0 B] * diag(w, w) (Cl_to_Beam(:P), :517-533)
#pragma once
#include "common.hpp"

namespace cmbl {

template <typename T, bool CPLX> struct EqElem { using type = T; };
template <typename T> struct EqElem<T, true> { using type = cx<T>; };
template <typename T> __device__ __forceinline__ T eq_re(T v) { return v; }
template <typename T> __device__ __forceinline__ T eq_im(T) { return T(0); }
template <typename T> __device__ __forceinline__ T eq_re(cx<T> v) { return v.x; }
template <typename T> __device__ __forceinline__ T eq_im(cx<T> v) { return v.y; }
template <typename E> __device__ __forceinline__ E eq_zero() { E z{}; return z; }

// ---- QU pack / unpack: one pointwise kernel per direction ----------------------------------------------------------------------------------
// FQ, FU: (Ny, Mh, B) each, the scaled half spectra of Q and U (one pair transform).  out: (2 Ny, Mh, B).  grid ceil(Ny * Mh * B / NTP)
template <typename T>
__global__ __launch_bounds__(NTP) void k_eq_qu_pack(const cx<T>* __restrict__ FQ, const cx<T>* __restrict__ FU, cx<T>* __restrict__ out, int Ny, long total) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= total) return;
  const long col = i / Ny;                                                   // (m, b) flattened
  const int y = (int)(i - col * Ny);
  const cx<T> q = FQ[i], u = FU[i];
  out[col * 2 * Ny + y] = mk<T>(q.x - u.y, q.y + u.x);                       // F[:, m] = FQ + i FU
  out[col * 2 * Ny + Ny + y] = mk<T>(q.x + u.y, q.y - u.x);                  // conj(F[:, (Nx - m) mod Nx]) = FQ - i FU (Q, U real)
}
// in: (2 Ny, Mh, B), F: (Ny, Nx, B); Nx even.  Column c <= Nx/2 takes the top rows of column c, THEN column (Nx - m) mod Nx takes conj(bottom rows
// of column m) for m = 0 ... Nx/2: columns 0 and Nx/2 end up as conj(bottom).  grid ceil(Ny * Nx * B / NTP)
template <typename T>
__global__ __launch_bounds__(NTP) void k_eq_qu_unpack(const cx<T>* __restrict__ in, cx<T>* __restrict__ F, int Ny, int Nx, long total) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= total) return;
  const long col = i / Ny;
  const int y = (int)(i - col * Ny), Mh = Nx / 2 + 1;
  const long b = col / Nx;
  const int c = (int)(col - b * Nx);
  const bool top = c > 0 && c < Nx / 2;
  const int m = top ? c : (Nx - c) % Nx;
  const cx<T> v = in[(b * Mh + m) * 2 * Ny + (top ? 0 : Ny) + y];
  F[i] = top ? v : conj(v);
}

// ---- M * f and M' * f ----------------------------------------------------------------------------------------------------------------------
// One workgroup makes EQ_TP rows p of one block m for every batch slot: lane = row, the four wavefronts split the summation index q (wave w takes
// q = w, w + 4, ... of every tile, ascending), their partial sums are added in wave order.  The batch runs in registers, BC slots at a time, so a
// block element is fetched once per BC slots.  Plain form: M[p, q] is contiguous along p, the lanes' loads are coalesced as they are.  Adjoint
// form: conj(M[q, p]) is contiguous along the summation index, so the tile is fetched with the lanes along q and turned in LDS.
constexpr int EQ_TP = 64, EQ_TQ = 32;
template <typename T, bool CPLX, bool ADJ, int BC>
__global__ __launch_bounds__(NTP) void k_eq_apply(const typename EqElem<T, CPLX>::type* __restrict__ M, const cx<T>* __restrict__ f, cx<T>* __restrict__ out, int n, int Mh, int nbatch) {
  using E = typename EqElem<T, CPLX>::type;
  __shared__ cx<T> sf[EQ_TQ][BC];
  __shared__ E tile[ADJ ? EQ_TQ : 1][EQ_TP + 1];
  __shared__ cx<T> red[3][EQ_TP][BC];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int m = blockIdx.y, p0 = blockIdx.x * EQ_TP, p = p0 + lane, pc = min(p, n - 1);
  const E* Mm = M + (size_t)m * n * n;
  for (int b0 = 0; b0 < nbatch; b0 += BC) {
    cx<T> acc[BC];
#pragma unroll
    for (int b = 0; b < BC; ++b) acc[b] = mk<T>(T(0), T(0));
    for (int q0 = 0; q0 < n; q0 += EQ_TQ) {
      __syncthreads();                                                       // the previous tile has been consumed
      for (int i = t; i < EQ_TQ * BC; i += NTP) {
        const int qq = i % EQ_TQ, b = i / EQ_TQ, q = q0 + qq;
        sf[qq][b] = (q < n && b0 + b < nbatch) ? f[((size_t)(b0 + b) * Mh + m) * n + q] : mk<T>(T(0), T(0));
      }
      if constexpr (ADJ) {
        for (int i = t; i < EQ_TQ * EQ_TP; i += NTP) {
          const int qq = i % EQ_TQ, j = i / EQ_TQ, q = q0 + qq, pj = p0 + j;
          tile[qq][j] = (q < n && pj < n) ? Mm[(size_t)pj * n + q] : eq_zero<E>();
        }
      }
      __syncthreads();
#pragma unroll 4
      for (int qq = w; qq < EQ_TQ; qq += 4) {
        const int q = q0 + qq;
        if (q >= n) break;                                                   // (uniform over the wavefront)
        E v;
        if constexpr (ADJ) v = tile[qq][lane]; else v = Mm[(size_t)q * n + pc];
        const T vr = eq_re(v), vi = ADJ ? -eq_im(v) : eq_im(v);
#pragma unroll
        for (int b = 0; b < BC; ++b) {
          const cx<T> x = sf[qq][b];
          acc[b].x += vr * x.x; acc[b].y += vr * x.y;
          if constexpr (CPLX) { acc[b].x -= vi * x.y; acc[b].y += vi * x.x; }
        }
      }
    }
    __syncthreads();
    if (w > 0) {
#pragma unroll
      for (int b = 0; b < BC; ++b) red[w - 1][lane][b] = acc[b];
    }
    __syncthreads();
    if (w == 0 && p < n) {
#pragma unroll
      for (int b = 0; b < BC; ++b) {
        if (b0 + b >= nbatch) break;
        cx<T> s = acc[b];
        for (int k = 0; k < 3; ++k) s = s + red[k][lane][b];
        out[((size_t)(b0 + b) * Mh + m) * n + p] = s;
      }
    }
  }
}

// ---- operator products on the matrix cores -------------------------------------------------------------------------------------------------
// C[p, q, m] = sum_j X[p, j] Y[j, q] with X = A or A' and Y = B or B'.  A workgroup of four wavefronts makes a 64 x 64 tile of C; the summation
// index runs in tiles of 16.  Both operand tiles are staged through LDS as planar real / imaginary planes [j][p] and [j][q], zero beyond n; an
// adjoint operand is fetched along ITS contiguous index and conjugated on the way in, so neither form needs a transposed copy in memory.  Each
// wavefront owns a 32 x 32 quarter as 2 x 2 MFMA tiles; a complex product is four real accumulations (re: Xr Yr and (-Xi) Yi, im: Xr Yi and Xi Yr).
// The MFMA is fed with Y as its row operand and X as its column operand (it computes C transposed), so that the 16 lanes of a result register lie
// along p, the contiguous index of C.  A and B operand maps of v_mfma_*_16x16x4: lane l holds row (column) l & 15 at k = l >> 4; result register
// r of lane l is row 4 (l >> 4) + r in single precision and row (l >> 4) + 4 r in double, column l & 15.
constexpr int EQ_MT = 64, EQ_KT = 16, EQ_LD = 80;
enum { EQ_NN = 0, EQ_HN = 1, EQ_NH = 2 };
template <typename T> struct EqMfma;
template <> struct EqMfma<float> {
  using acc_t = __attribute__((ext_vector_type(4))) float;
  static __device__ __forceinline__ acc_t run(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int r) { return 4 * (lane >> 4) + r; }
};
template <> struct EqMfma<double> {
  using acc_t = __attribute__((ext_vector_type(4))) double;
  static __device__ __forceinline__ acc_t run(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};

// grid (ceil(n / 64), ceil(n / 64), Mh)
template <typename T, bool CPLX, int MODE>
__global__ __launch_bounds__(NTP) void k_eq_matmul(const typename EqElem<T, CPLX>::type* __restrict__ A, const typename EqElem<T, CPLX>::type* __restrict__ B,
                                                  typename EqElem<T, CPLX>::type* __restrict__ Cout, int n) {
  using E = typename EqElem<T, CPLX>::type;
  using acc_t = typename EqMfma<T>::acc_t;
  constexpr int NPL = CPLX ? 2 : 1;
  __shared__ T sX[NPL][EQ_KT][EQ_LD], sY[NPL][EQ_KT][EQ_LD];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wp = (w & 1) * 32, wq = (w >> 1) * 32;
  const int p0 = blockIdx.x * EQ_MT, q0 = blockIdx.y * EQ_MT;
  const size_t mo = (size_t)blockIdx.z * n * n;
  const E* Am = A + mo; const E* Bm = B + mo;
  acc_t cre[2][2], cim[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) { cre[a][b] = acc_t{0, 0, 0, 0}; cim[a][b] = acc_t{0, 0, 0, 0}; }

  for (int j0 = 0; j0 < n; j0 += EQ_KT) {
    __syncthreads();
#pragma unroll
    for (int i = t; i < EQ_MT * EQ_KT; i += NTP) {
      // X[p, j]: A[p + n j] (contiguous along p) or conj(A[j + n p]) (contiguous along j)
      int pp, kk;
      if (MODE == EQ_HN) { kk = i % EQ_KT; pp = i / EQ_KT; } else { pp = i % EQ_MT; kk = i / EQ_MT; }
      const int p = p0 + pp, j = j0 + kk;
      E v = eq_zero<E>();
      if (p < n && j < n) v = MODE == EQ_HN ? Am[(size_t)p * n + j] : Am[(size_t)j * n + p];
      sX[0][kk][pp] = eq_re(v);
      if constexpr (CPLX) sX[1][kk][pp] = MODE == EQ_HN ? -eq_im(v) : eq_im(v);
      // Y[j, q]: B[j + n q] (contiguous along j) or conj(B[q + n j]) (contiguous along q)
      int qq;
      if (MODE == EQ_NH) { qq = i % EQ_MT; kk = i / EQ_MT; } else { kk = i % EQ_KT; qq = i / EQ_KT; }
      const int q = q0 + qq, jy = j0 + kk;
      E u = eq_zero<E>();
      if (q < n && jy < n) u = MODE == EQ_NH ? Bm[(size_t)jy * n + q] : Bm[(size_t)q * n + jy];
      sY[0][kk][qq] = eq_re(u);
      if constexpr (CPLX) sY[1][kk][qq] = MODE == EQ_NH ? -eq_im(u) : eq_im(u);
    }
    __syncthreads();
#pragma unroll
    for (int k0 = 0; k0 < EQ_KT; k0 += 4) {
      const int k = k0 + (lane >> 4), l = lane & 15;
      T xr[2], xi[2], yr[2], yi[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        xr[a] = sX[0][k][wp + 16 * a + l]; yr[a] = sY[0][k][wq + 16 * a + l];
        if constexpr (CPLX) { xi[a] = sX[1][k][wp + 16 * a + l]; yi[a] = sY[1][k][wq + 16 * a + l]; }
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)                                             // a: 16 columns q (MFMA rows), b: 16 rows p (MFMA columns)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          cre[a][b] = EqMfma<T>::run(yr[a], xr[b], cre[a][b]);
          if constexpr (CPLX) {
            cre[a][b] = EqMfma<T>::run(-yi[a], xi[b], cre[a][b]);
            cim[a][b] = EqMfma<T>::run(yi[a], xr[b], cim[a][b]);
            cim[a][b] = EqMfma<T>::run(yr[a], xi[b], cim[a][b]);
          }
        }
    }
  }
  E* Cm = Cout + mo;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = q0 + wq + 16 * a + EqMfma<T>::row(lane, r), p = p0 + wp + 16 * b + (lane & 15);
        if (p < n && q < n) {
          if constexpr (CPLX) Cm[(size_t)q * n + p] = mk<T>(cre[a][b][r], cim[a][b][r]);
          else Cm[(size_t)q * n + p] = cre[a][b][r];
        }
      }
}

// ---- dot(M1', M2) = sum conj(A[q, p, m]) B[p, q, m] ------------------------------------------------------------------------------------------
// (as written in the reference: the element of A is the TRANSPOSED one.)  Stage 1: a workgroup takes a 32 x 32 tile (p, q) of one block, reads the
// tile of B along p and the mirrored tile of A along q (both coalesced), turns the latter in LDS and leaves ONE partial sum in double, formed in a
// fixed order (per thread over its four elements, then a tree over the 256 threads); stage 2: one workgroup adds the partial sums, again in a
// fixed order.  grid (ceil(n / 32), ceil(n / 32), Mh); part: 2 doubles per workgroup
template <typename T, bool CPLX>
__global__ __launch_bounds__(NTP) void k_eq_dot_part(const typename EqElem<T, CPLX>::type* __restrict__ A, const typename EqElem<T, CPLX>::type* __restrict__ B, double* __restrict__ part, int n) {
  using E = typename EqElem<T, CPLX>::type;
  __shared__ E ta[32][33];
  __shared__ double sr[NTP], si[NTP];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int p0 = blockIdx.x * 32, q0 = blockIdx.y * 32;
  const size_t mo = (size_t)blockIdx.z * n * n;
#pragma unroll
  for (int i = 0; i < 4; ++i) {                                               // A[q, p]: q contiguous
    const int q = q0 + tx, p = p0 + ty + 8 * i;
    ta[ty + 8 * i][tx] = (q < n && p < n) ? A[mo + (size_t)p * n + q] : eq_zero<E>();
  }
  __syncthreads();
  double re = 0, im = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {                                               // B[p, q]: p contiguous
    const int p = p0 + tx, q = q0 + ty + 8 * i;
    if (p < n && q < n) {
      const E a = ta[tx][ty + 8 * i], b = B[mo + (size_t)q * n + p];
      const double ar = eq_re(a), ai = eq_im(a), br = eq_re(b), bi = eq_im(b);
      re += ar * br + ai * bi; im += ar * bi - ai * br;
    }
  }
  sr[threadIdx.x] = re; si[threadIdx.x] = im;
  __syncthreads();
  for (int s = NTP / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { sr[threadIdx.x] += sr[threadIdx.x + s]; si[threadIdx.x] += si[threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const size_t o = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    part[2 * o] = sr[0]; part[2 * o + 1] = si[0];
  }
}
// one workgroup (a template so that only the units that launch it compile it)
template <int NT>
__global__ __launch_bounds__(NT) void k_eq_dot_sum(const double* __restrict__ part, long nparts, double* __restrict__ out) {
  __shared__ double sr[NT], si[NT];
  double re = 0, im = 0;
  for (long i = threadIdx.x; i < nparts; i += NT) { re += part[2 * i]; im += part[2 * i + 1]; }
  sr[threadIdx.x] = re; si[threadIdx.x] = im;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { sr[threadIdx.x] += sr[threadIdx.x + s]; si[threadIdx.x] += si[threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = sr[0]; out[1] = si[0]; }
}

// ---- beams ---------------------------------------------------------------------------------------------------------------------------------
// blocks[j, k, m] *= w[k], in place.  grid ceil(n * n * Mh / NTP)
template <typename T, bool CPLX>
__global__ __launch_bounds__(NTP) void k_eq_scale_cols(typename EqElem<T, CPLX>::type* __restrict__ blocks, const T* __restrict__ wgt, int n, long total) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= total) return;
  const T s = wgt[(i / n) % n];
  if constexpr (CPLX) { cx<T> v = blocks[i]; blocks[i] = mk<T>(v.x * s, v.y * s); }
  else blocks[i] *= s;
}
// out (2 Ny, 2 Ny, Mh) complex = [B 0; 0 B] * diag(w, w) from the real blocks B (Ny, Ny, Mh).  grid ceil(4 Ny * Ny * Mh / NTP)
template <typename T>
__global__ __launch_bounds__(NTP) void k_eq_beam_pol(const T* __restrict__ Bi, const T* __restrict__ wgt, cx<T>* __restrict__ out, int Ny, long total) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= total) return;
  const int n = 2 * Ny;
  const long m = i / ((long)n * n);
  const int k = (int)((i / n) % n), j = (int)(i % n);
  const bool diag = (j < Ny) == (k < Ny);
  const int jj = j % Ny, kk = k % Ny;
  out[i] = mk<T>(diag ? Bi[(m * Ny + kk) * Ny + jj] * wgt[kk] : T(0), T(0));
}

}  // namespace cmbl
