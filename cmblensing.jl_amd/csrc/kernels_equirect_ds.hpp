// NoLensingDataSet on ProjEquiRect (src/dataset.jl:37-47, 68-80, src/maximization.jl:17-42, src/numerical_algorithms.jl:73-134): the kernels behind
// cmbl_eqds_* and cmbl_equirect_field_dot.  Layouts are those of kernels_equirect.hpp.  No atomics; every output element has one writer and one
// fixed order of operations, so results are bit-identical between runs.
//   k_eqds_apply2     out = sa A x + sc C y, each operand plain or adjoint, real or complex (compile-time), with the tiling of k_eq_apply (a block element is fetched once
//                     per BC batch slots); optionally leaves the partial sums of dot(v, out) for a third vector v
//   k_eqds_dot_part, k_eqds_dot_fin   per-slot dot products in double, two stages: of Az arrays with the weights that make them the map dot (:355), of
//                     map arrays plain or with a diagonal weight in between
//   k_eqds_pix        the data-space pointwise step: out = sgn wb (d - wa in), every factor optional
//   k_eqds_wcomb      W = M Cn^-1 M and M Cn^-1 of map-diagonal operators, once per operator change
// The dot of two maps, formed in the Az basis: spin 0  sum_m w_m Re(conj(a) b) over the half spectrum with w = 1 at m = 0 and m = Nx/2 (even Nx), 2
// elsewhere; spin 2  the same over all 2 Ny packed rows with w = 1/2 at columns 0 and Nx/2, 1 elsewhere.  This is the map dot for images of maps only.
#pragma once
#include "kernels_pointwise.hpp"
#include "kernels_equirect.hpp"

namespace cmbl {

__device__ __forceinline__ double eqds_w(int m, int Nx, int spin2) {
  const bool edge = m == 0 || 2 * m == Nx;
  return spin2 ? (edge ? 0.5 : 1.0) : (edge ? 1.0 : 2.0);
}

template <typename T> struct EqdsArgs {
  const void* A; const cx<T>* x; T sa;
  const void* C; const cx<T>* y; T sc;                             // C == nullptr and y != nullptr: + sc y (the identity in C's place)
  cx<T>* out;
  const cx<T>* dotv; double* part;                                           // part != nullptr: part[(b Mh + m) gridDim.x + blockIdx.x] = partial of dot(dotv, out)
  int n, Mh, Nx, spin2, nbatch;
};

// acc[b] += sum_q M[p, q] s f[q, m, b0 + b] (or with conj(M[q, p])) for the workgroup's rows p: the loop of k_eq_apply.  Every thread of the
// workgroup calls it (it synchronises).  tile_raw: EQ_TQ * (EQ_TP + 1) elements of cx<T>, used by the adjoint form.
template <typename T, bool CPLX, bool ADJ, int BC>
__device__ __forceinline__ void eqds_pass(const void* Mv, const cx<T>* __restrict__ f, T s, cx<T>* acc, cx<T> (*sf)[BC], cx<T>* tile_raw, int n, int Mh, int m,
                                          int p0, int b0, int nbatch) {
  using E = typename EqElem<T, CPLX>::type;
  constexpr int LD = EQ_TP + 1;
  E* tile = reinterpret_cast<E*>(tile_raw);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, pc = min(p0 + lane, n - 1);
  const E* __restrict__ Mm = (const E*)Mv + (size_t)m * n * n;
  for (int q0 = 0; q0 < n; q0 += EQ_TQ) {
    __syncthreads();                                                         // the previous tile has been consumed
    for (int i = t; i < EQ_TQ * BC; i += NTP) {
      const int qq = i % EQ_TQ, b = i / EQ_TQ, q = q0 + qq;
      cx<T> v = mk<T>(T(0), T(0));
      if (q < n && b0 + b < nbatch) { v = f[((size_t)(b0 + b) * Mh + m) * n + q]; v = mk<T>(s * v.x, s * v.y); }
      sf[qq][b] = v;
    }
    if constexpr (ADJ) {
      for (int i = t; i < EQ_TQ * EQ_TP; i += NTP) {
        const int qq = i % EQ_TQ, j = i / EQ_TQ, q = q0 + qq, pj = p0 + j;
        tile[qq * LD + j] = (q < n && pj < n) ? Mm[(size_t)pj * n + q] : eq_zero<E>();
      }
    }
    __syncthreads();
#pragma unroll(CPLX ? 8 : 4)
    for (int qq = w; qq < EQ_TQ; qq += 4) {                                  // (complex blocks: all 8 loads of a wavefront's share of the tile in flight; measured)
      const int q = q0 + qq;
      if (q >= n) break;                                                     // (uniform over the wavefront)
      E v;
      if constexpr (ADJ) v = tile[qq * LD + lane]; else v = Mm[(size_t)q * n + pc];
      const T vr = eq_re(v), vi = ADJ ? -eq_im(v) : eq_im(v);
#pragma unroll
      for (int b = 0; b < BC; ++b) {
        const cx<T> x = sf[qq][b];
        acc[b].x += vr * x.x; acc[b].y += vr * x.y;
        if constexpr (CPLX) { acc[b].x -= vi * x.y; acc[b].y += vi * x.x; }
      }
    }
  }
}

// grid (ceil(n / EQ_TP), Mh).  The wavefronts split the summation index as in k_eq_apply; wavefront 0 adds their sums in wave order, stores its
// rows and, when asked, reduces w_m Re(conj(dotv) out) over its 64 rows in double (shuffle tree, fixed order).
template <typename T, bool CA, bool ADJA, bool CC, bool ADJC, bool TWO, int BC>
__global__ __launch_bounds__(NTP) void k_eqds_apply2(EqdsArgs<T> a) {
  constexpr int NTILE = (ADJA || (TWO && ADJC)) ? EQ_TQ * (EQ_TP + 1) : 1, NRED = 3 * EQ_TP * BC;     // a plain form carries no turned tile
  __shared__ cx<T> sf[EQ_TQ][BC];
  __shared__ cx<T> buf[NTILE > NRED ? NTILE : NRED];                         // the turned tile of an adjoint pass, then the wavefronts' partial sums: never live together
  cx<T>* tile = buf;
  cx<T> (*red)[EQ_TP][BC] = reinterpret_cast<cx<T> (*)[EQ_TP][BC]>(buf);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int n = a.n, Mh = a.Mh, m = blockIdx.y, p0 = blockIdx.x * EQ_TP, p = p0 + lane, pc = min(p, n - 1);
  const double wm = eqds_w(m, a.Nx, a.spin2);
  for (int b0 = 0; b0 < a.nbatch; b0 += BC) {
    cx<T> acc[BC];
#pragma unroll
    for (int b = 0; b < BC; ++b) acc[b] = mk<T>(T(0), T(0));
    eqds_pass<T, CA, ADJA, BC>(a.A, a.x, a.sa, acc, sf, tile, n, Mh, m, p0, b0, a.nbatch);
    if constexpr (TWO) eqds_pass<T, CC, ADJC, BC>(a.C, a.y, a.sc, acc, sf, tile, n, Mh, m, p0, b0, a.nbatch);
    __syncthreads();
    if (w > 0) {
#pragma unroll
      for (int b = 0; b < BC; ++b) red[w - 1][lane][b] = acc[b];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int b = 0; b < BC; ++b) {
        if (b0 + b >= a.nbatch) break;
        cx<T> s = acc[b];
        for (int k = 0; k < 3; ++k) s = s + red[k][lane][b];
        const size_t idx = ((size_t)(b0 + b) * Mh + m) * n + pc;             // (a row beyond n reads row n - 1 and stores nothing)
        if constexpr (!TWO) {
          if (a.y) { const cx<T> yv = a.y[idx]; s = mk<T>(s.x + a.sc * yv.x, s.y + a.sc * yv.y); }
        }
        if (p < n) a.out[idx] = s;
        if (a.part) {
          const cx<T> v = a.dotv[idx];
          double d = p < n ? wm * ((double)v.x * (double)s.x + (double)v.y * (double)s.y) : 0.0;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) d += __shfl_down(d, o, 64);
          if (lane == 0) a.part[((size_t)(b0 + b) * Mh + m) * gridDim.x + blockIdx.x] = d;
        }
      }
    }
  }
}

// ---- per-slot dots --------------------------------------------------------------------------------------------------------------------------
// stage 1, grid (nblk, B): workgroup k of slot b adds its strided share of the terms in double (per thread ascending, then the tree of block_sum).
//   AZ: a, b are (n, Mh) complex per slot, len = n Mh; term = w_m Re(conj(a) b)
//   map: a, b are (npix, P) real per slot, len = npix P; term = a wgt b, wgt (wplanes = 1 or P planes) or nullptr for 1
template <typename T, bool AZ>
__global__ __launch_bounds__(NTP) void k_eqds_dot_part(const void* __restrict__ av, const void* __restrict__ bv, const T* __restrict__ wgt, int wplanes, double* __restrict__ part,
                                                      long len, int n, int Nx, int spin2, long npix) {
  const int bt = blockIdx.y;
  double acc = 0;
  for (long i = (long)blockIdx.x * NTP + threadIdx.x; i < len; i += (long)gridDim.x * NTP) {
    if constexpr (AZ) {
      const cx<T> x = ((const cx<T>*)av)[(size_t)bt * len + i], y = ((const cx<T>*)bv)[(size_t)bt * len + i];
      acc += eqds_w((int)(i / n), Nx, spin2) * ((double)x.x * (double)y.x + (double)x.y * (double)y.y);
    } else {
      const T x = ((const T*)av)[(size_t)bt * len + i], y = ((const T*)bv)[(size_t)bt * len + i];
      const T wv = wgt ? wgt[(wplanes == 1 ? 0 : i / npix) * npix + i % npix] : T(1);
      acc += (double)x * (double)wv * (double)y;
    }
  }
  const double r = block_sum<double>(acc);
  if (threadIdx.x == 0) part[(size_t)bt * gridDim.x + blockIdx.x] = r;
}
// stage 2, grid (B): out[b] = sum of the nper partial sums of slot b, in a fixed order
static __global__ __launch_bounds__(NTP) void k_eqds_dot_fin(const double* __restrict__ part, long nper, double* __restrict__ out) {
  const int bt = blockIdx.x;
  double acc = 0;
  for (long i = threadIdx.x; i < nper; i += NTP) acc += part[(size_t)bt * nper + i];
  const double r = block_sum<double>(acc);
  if (threadIdx.x == 0) out[bt] = r;
}

// ---- pointwise, maps (npix, P, B) -----------------------------------------------------------------------------------------------------------
// out = sgn * wb * (d - wa * in);  in == nullptr: 0;  d == nullptr: the bracket is wa * in;  wa, wb == nullptr: 1.  wa, wb: npa, npb = 1 or P planes.
// out may be in or d (same index).  grid ceil(total / NTP)
template <typename T>
__global__ __launch_bounds__(NTP) void k_eqds_pix(T* out, const T* in, const T* d, const T* __restrict__ wa, int npa, const T* __restrict__ wb, int npb, T sgn, int P, long npix, long total) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= total) return;
  const long pix = i % npix;
  const int pol = (int)((i / npix) % P);
  T v = in ? in[i] : T(0);
  if (wa) v *= wa[(npa == 1 ? 0 : pol) * npix + pix];
  if (d) v = d[i] - v;
  if (wb) v *= wb[(npb == 1 ? 0 : pol) * npix + pix];
  out[i] = sgn * v;
}
// MC = M * Ci and W = MC * M for np = max(npm, npc) planes; M == nullptr: 1.  grid ceil(np * npix / NTP)
template <typename T>
__global__ __launch_bounds__(NTP) void k_eqds_wcomb(T* __restrict__ W, T* __restrict__ MC, const T* __restrict__ M, int npm, const T* __restrict__ Ci, int npc, long npix, long total) {
  const long i = (long)blockIdx.x * NTP + threadIdx.x;
  if (i >= total) return;
  const long pix = i % npix, pl = i / npix;
  const T mv = M ? M[(npm == 1 ? 0 : pl) * npix + pix] : T(1);
  const T mc = mv * Ci[(npc == 1 ? 0 : pl) * npix + pix];
  MC[i] = mc; W[i] = mc * mv;
}

}  // namespace cmbl
