// get_Cℓ (src/proj_lambert.jl:470-513): the binned sums S1 = Σ w·CL and S2 = Σ w·CL² of auto- and cross-spectra, CL = Re(conj(f1)·f2) / α, over the
// λ-weighted half plane.  Which mode belongs to which bin, and with which coefficient λ·w, is decided on the host in double when the binning plan is made
// (engine_cl.hpp ClBins): the plan's list holds the kept modes sorted by (bin, address) and is cut into CHUNKS of at most CL_CHUNK modes that never
// straddle a bin.  Both kernels are deterministic -- no atomics, every sum in a fixed order -- and accumulate in double whatever the field's precision;
// a batch slot's numbers depend on that slot's data and the plan alone.
//   k_cl_chunks  grid (chunks, slots): one workgroup strides its chunk, gathers the npol planes of a mode ONCE and forms every requested product from
//                registers; fixed tree over the workgroup; part[slot][pair][moment][chunk]
//   k_cl_final   one thread per (slot, pair, moment, bin): its bin's chunk partials in ascending order, times 1/α (S1) or 1/α² (S2)
// Bandwidth- and latency-bound gathers: no LDS beyond the tree, 8 modes in flight per thread at a full chunk.
#pragma once
#include "common.hpp"
#include "kernels_pointwise.hpp"

namespace cmbl {

constexpr int CL_MAXPAIRS = 9;            // every ordered pair of three planes
constexpr int CL_CHUNK = 2048;            // modes per workgroup: 8 per thread

struct ClPairs { int n; signed char a[CL_MAXPAIRS], b[CL_MAXPAIRS]; };

template <typename T> struct ClArgs {
  const cx<T>* f1; const cx<T>* f2;       // [slot][npol][plane] complex planes, both in the layout `idx` addresses (f2 == f1 for auto-spectra)
  const unsigned* idx;                    // address of every listed mode within a plane
  const double* coef;                     // λ·w of every listed mode
  const int* chunk_start;                 // [chunks + 1] offsets into the list
  double* part;                           // [slot][pair][moment][chunk]
  long plane; int npol, chunks;
  ClPairs pr;
};

template <typename T> __device__ __forceinline__ cx<T> cl_sel(const cx<T> (&v)[3], int k) { return k == 0 ? v[0] : k == 1 ? v[1] : v[2]; }

template <typename T, int MOM, bool CROSS>
__global__ __launch_bounds__(NTP) void k_cl_chunks(const ClArgs<T> a) {
  const int c = blockIdx.x, s = blockIdx.y;
  const int i0 = a.chunk_start[c], i1 = a.chunk_start[c + 1];
  const cx<T>* p1 = a.f1 + (long)s * a.npol * a.plane;
  const cx<T>* p2 = a.f2 + (long)s * a.npol * a.plane;
  double s1[CL_MAXPAIRS], s2[CL_MAXPAIRS];
#pragma unroll
  for (int k = 0; k < CL_MAXPAIRS; ++k) { s1[k] = 0; s2[k] = 0; }
  for (int i = i0 + (int)threadIdx.x; i < i1; i += NTP) {
    const unsigned j = a.idx[i];
    const double w = a.coef[i];
    cx<T> u[3], v[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      u[p] = mk<T>((T)0, (T)0); v[p] = u[p];
      if (p < a.npol) { u[p] = p1[p * a.plane + j]; v[p] = CROSS ? p2[p * a.plane + j] : u[p]; }
    }
#pragma unroll
    for (int k = 0; k < CL_MAXPAIRS; ++k)
      if (k < a.pr.n) {
        const cx<T> x = cl_sel(u, a.pr.a[k]), y = cl_sel(v, a.pr.b[k]);
        const double cl = (double)x.x * (double)y.x + (double)x.y * (double)y.y;
        s1[k] += w * cl;
        if (MOM == 2) s2[k] += w * cl * cl;
      }
  }
#pragma unroll
  for (int k = 0; k < CL_MAXPAIRS; ++k)
    if (k < a.pr.n) {                                                       // uniform over the workgroup: every thread takes part in the tree
      const double r1 = block_sum<double>(s1[k]);
      double r2 = 0;
      if (MOM == 2) r2 = block_sum<double>(s2[k]);
      if (threadIdx.x == 0) {
        double* o = a.part + (((long)s * a.pr.n + k) * MOM) * a.chunks + c;
        o[0] = r1;
        if (MOM == 2) o[a.chunks] = r2;
      }
    }
}

// out[slot][pair][moment][bin]; bin_chunk[nbins + 1]: the chunks of a bin (none for an empty bin, which gets 0)
template <int MOM>
__global__ __launch_bounds__(NTP) void k_cl_final(const double* __restrict__ part, const int* __restrict__ bin_chunk, double* __restrict__ out,
                                                  long total, int nbins, int chunks, double inv_alpha) {
  const long t = (long)blockIdx.x * NTP + threadIdx.x;
  if (t >= total) return;
  const int b = (int)(t % nbins);
  const long row = t / nbins;                                               // (slot, pair, moment)
  const double* p = part + row * chunks;
  double r = 0;
  for (int c = bin_chunk[b]; c < bin_chunk[b + 1]; ++c) r += p[c];
  out[t] = r * ((row % MOM) == 0 ? inv_alpha : inv_alpha * inv_alpha);
}

}  // namespace cmbl
