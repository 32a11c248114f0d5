// Column pass of a BilinearLens in the L slot of a data set (src/dataset.jl:223, src/bilinearlens.jl:107-125), power-of-two maps:
//   rfft_y(L f)  or  rfft_y(L' g)  of a map, straight into the mixed layout.
// k_y_r2c (kernels_fft.hpp) with another loader: where that kernel reads its R packed pairs of a column tile from the map, this one forms them --
// SRC 0 by the bilinear gather from the operator's table (k_bl_gather: base, fr, the weights of bl_weight), SRC 1 by the row sum over the sorted
// CSR of the transpose (k_bl_csr) -- and hands them to the same mpt_write_forward / half_store.  The lensed map never goes to memory, and the
// launch replaces three (gather, y_r2c and the map between them).
//
// The arithmetic of the two gathers is kept expression for expression, with the summation order of a CSR row: L'g is bit-identical between runs,
// and the result differs from the composition only by how the compiler contracts the same expressions.  No floating-point atomics.
//
// Latency: a thread holds R pairs = 2R pixels of one slice.  The table entries of all of them are loaded first, then the 8R neighbour values
// (SRC 0) or, in lock step over the row position, one entry of each of the 2R rows (SRC 1): 2R independent gathers in flight per thread where
// k_bl_gather / k_bl_csr walk their slices one dependent gather at a time.  One workgroup serves one slice (grid.y = slices, as k_y_r2c), so the
// table entry of a pixel is fetched once per slice, the repeats coming from the L2 (DESIGN.md has why it is not kept across the pol slices).
#pragma once
#include "kernels_fft.hpp"
#include "kernels_bilinear.hpp"

namespace cmbl {

template <typename T> struct LensTab;                      // engine.hpp

template <typename T, int R, int NT, int LGM, int SRC>
__global__ __launch_bounds__(NT) void k_y_lens(LensTab<T> tab, const T* __restrict__ in, cx<T>* __restrict__ out, const cx<T>* __restrict__ twY, int Nx) {
  using G = ColTile<R, NT, LGM>;
  constexpr int M = G::M, LD = G::LDM, C = G::C, Ny = 2 * M;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cx<T>* tw = reinterpret_cast<cx<T>*>(smem);
  cx<T>* s = tw + M;                            // half of the twiddle circle (see row_tw)
  const int x0 = xcd_tile(blockIdx.x, gridDim.x) * C;
  const size_t sl = blockIdx.y;
  TwStage<T, NT, M> twr;
  twr.issue(twY);
  using PM = PairMap<R, NT, LGM>;
  const unsigned pix0 = (unsigned)x0 * (unsigned)Ny;                       // first pixel of the tile; pair e of the tile = pixels pix0 + 2e, + 1
  const T* __restrict__ p = in + sl * (size_t)Nx * Ny;
  cx<T> v[R];
  if constexpr (SRC == 0) {
    unsigned b[2 * R];
    cx<T> f[2 * R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const unsigned I = pix0 + 2u * (unsigned)PM::e(i);
      b[2 * i] = tab.base[I]; b[2 * i + 1] = tab.base[I + 1];
      f[2 * i] = tab.fr[I]; f[2 * i + 1] = tab.fr[I + 1];
    }
    T g[2 * R][4];
#pragma unroll
    for (int j = 0; j < 2 * R; ++j) {
      unsigned a[4];
      bl_neigh(b[j], Ny, Nx, a);
#pragma unroll
      for (int k = 0; k < 4; ++k) g[j][k] = p[a[k]];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      T r[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = 2 * i + h;
        const T w0 = bl_weight<T>(f[j], 0), w1 = bl_weight<T>(f[j], 1), w2 = bl_weight<T>(f[j], 2), w3 = bl_weight<T>(f[j], 3);
        r[h] = w0 * g[j][0] + w1 * g[j][1] + w2 * g[j][2] + w3 * g[j][3];
      }
      v[i] = mk<T>(r[0], r[1]);
    }
  } else {
    unsigned rs[2 * R], re[2 * R], len = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const unsigned J = pix0 + 2u * (unsigned)PM::e(i);
      const unsigned r0 = tab.rowstart[J], r1 = tab.rowstart[J + 1], r2 = tab.rowstart[J + 2];
      rs[2 * i] = r0; re[2 * i] = r1; rs[2 * i + 1] = r1; re[2 * i + 1] = r2;
      len = max(len, max(r1 - r0, r2 - r1));
    }
    T acc[2 * R];
#pragma unroll
    for (int j = 0; j < 2 * R; ++j) acc[j] = 0;
    for (unsigned q = 0; q < len; ++q) {
#pragma unroll
      for (int j = 0; j < 2 * R; ++j) {
        const unsigned at = rs[j] + q;
        if (at < re[j]) acc[j] += tab.val[at] * p[tab.col[at]];
      }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) v[i] = mk<T>(acc[2 * i], acc[2 * i + 1]);
  }
  twr.commit(tw);
  __syncthreads();
  mpt_write_forward<T, R, NT, LGM, LD>(s, tw, [&](int i) { return v[i]; });
  half_store<T, NT, LD, LGM, G::LGC>(s, out + sl * (size_t)mixed_rows(G::Nyh) * Nx, tw, x0);
}

}  // namespace cmbl
