// Host side of cmbl_edt_sq and cmbl_make_mask (src/masking.jl:1-67).  Every launch goes to the context's stream; the scratch planes belong to
// the call (one allocation, released when the call returns, after the stream has drained).  The kernels are those of kernels_mask.hpp; the
// transposes between the two passes of the distance transform, and between the two axes of the filter, are the context's tiled k_transpose, so
// that every pass reads and writes whole lines.
#pragma once
#include "engine.hpp"
#include "kernels_mask.hpp"

namespace cmbl {

struct MaskArgs { const int32_t* src_yx; int nsrc, pad, apod_w, round_w, src_w; };

// Kernel.gaussian(sigma) of ImageFiltering.jl, one factor: exp(-x^2 / 2 sigma^2) for x = -2 ceil(sigma) ... 2 ceil(sigma), normalised to sum 1
inline std::vector<double> mask_gauss_taps(int sigma) {
  const int R = 2 * sigma;
  std::vector<double> w((size_t)2 * R + 1);
  double sum = 0;
  for (int x = -R; x <= R; ++x) sum += w[(size_t)(x + R)] = std::exp(-(double)x * x / (2.0 * sigma * sigma));
  for (double& v : w) v /= sum;
  return w;
}

// Squared distance to the nearest feature byte of the map plane `feat` [x][y] (ImageMorphology.feature_transform + norm, :42-43, 48-49).
// `gT` and `out` are planes of npix ints; the result is left in gT TRANSPOSED ([y][x]) and, with `untranspose`, in out as a map plane [x][y]
// (`out` serves as scratch either way).  *found (may be null) is raised when the plane has a feature.
template <typename T> void edt_sq(Ctx<T>* c, const unsigned char* feat, int* out, int* gT, int* found, bool untranspose) {
  CMBL_LAUNCH(c, K_EDT, (k_edt_cols<NTP>), dim3((unsigned)c->Nx), 0, c->stream, feat, out, c->Ny, found);
  c->transpose(out, gT, c->Nx, c->Ny, 1);
  CMBL_LAUNCH(c, K_EDT, (k_edt_rows<NTP>), dim3((unsigned)c->Ny), 0, c->stream, gT, c->Nx);
  if (untranspose) c->transpose(gT, out, c->Ny, c->Nx, 1);
}

template <typename T> void edt_sq_checked(Ctx<T>* c, const unsigned char* feat, int* d2) {
  DevBuf scratch;
  scratch.ensure(sizeof(int) * (c->npix() + 1));
  int* gT = scratch.as<int>(); int* found = gT + c->npix();
  CMBL_HIP(hipMemsetAsync(found, 0, sizeof(int), c->stream));
  edt_sq(c, feat, d2, gT, found, true);
  int has = 0;
  CMBL_HIP(hipMemcpyAsync(&has, found, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  CMBL_HIP(hipStreamSynchronize(c->stream));
  CMBL_REQUIRE(has != 0, ERR_ARG, "edt_sq: the plane has no feature (no non-zero byte), the distance is undefined");
}

template <typename IN> void mask_gauss(CtxBase* c, const IN* in, double* out, const double* taps, int ntaps, int n, int lines) {
  const size_t lds = sizeof(double) * (size_t)(MASK_TILE + ntaps - 1);
  CMBL_LAUNCH(c, K_MASK_GAUSS, (k_mask_gauss<IN>), dim3((unsigned)((n + MASK_TILE - 1) / MASK_TILE), (unsigned)lines), lds, c->stream, in, out, taps, ntaps, n);
}

// make_mask (:2-24) in pixel units; the entry point has checked the arguments (include/cmblens.h)
template <typename T> void make_mask(Ctx<T>* c, const MaskArgs& m, T* out) {
  const long np = c->npix();
  const int Ny = c->Ny, Nx = c->Nx;
  const unsigned gp = (unsigned)((np + NTP - 1) / NTP);
  const bool apod = m.apod_w > 0, srcs = m.nsrc > 0, smooth = apod && m.round_w > 0;
  MaskPoint<T> a{};
  a.out = out; a.Ny = Ny; a.Nx = Nx; a.pad = m.pad; a.apod_w = m.apod_w; a.src_w = m.src_w;

  // one allocation: [two double planes and the taps] [int planes: I1 the transposed side of every transform, I2 the boundary's d2, I0 the sources']
  // [source positions] [feature bytes].  After the argument checks each feature plane has a feature (pad > 0 with apod_w > 0; a source; its own
  // pixel bled as src_w > 0), so no transform here needs the `found` flag.
  const std::vector<double> taps = smooth ? mask_gauss_taps(m.round_w) : std::vector<double>();
  const int nplanes = (apod || srcs ? 1 : 0) + (apod ? 1 : 0) + (srcs ? 1 : 0);
  const size_t nd = smooth ? 2 * (size_t)np + taps.size() : 0, ni = (size_t)nplanes * np + 2 * (size_t)m.nsrc;
  DevBuf scratch;
  scratch.ensure(sizeof(double) * nd + sizeof(int) * ni + (size_t)np);
  double* D0 = scratch.as<double>(); double* D1 = D0 + np; double* tapd = D1 + np;
  int* I1 = reinterpret_cast<int*>(scratch.as<double>() + nd); int* I2 = I1 + np; int* I0 = apod ? I2 + np : I2;
  int* yx = I1 + (size_t)nplanes * np; int* const found = nullptr;
  unsigned char* feat = reinterpret_cast<unsigned char*>(yx + 2 * m.nsrc);

  if (apod) {                                                                // cos_apod(boundary, apod_w, round_w) (:46-54): the distance to the padding, in I2 or D1
    CMBL_LAUNCH(c, K_MASK_POINT, (k_mask_border<NTP>), dim3(gp), 0, c->stream, feat, Ny, Nx, m.pad);
    edt_sq(c, feat, I2, I1, found, !smooth);
    if (smooth) {                                                            // imfilter(distance, Kernel.gaussian(round_w)): along x on [y][x], then along y on [x][y]
      CMBL_HIP(hipMemcpyAsync(tapd, taps.data(), sizeof(double) * taps.size(), hipMemcpyHostToDevice, c->stream));
      mask_gauss(c, I1, D1, tapd, (int)taps.size(), Nx, Ny);
      c->transpose(D1, D0, Ny, Nx, 1);
      mask_gauss(c, D0, D1, tapd, (int)taps.size(), Ny, Nx);
      a.distb = D1;
    } else a.d2b = I2;
  }
  if (srcs) {
    CMBL_HIP(hipMemcpyAsync(yx, m.src_yx, sizeof(int) * 2 * (size_t)m.nsrc, hipMemcpyHostToDevice, c->stream));
    CMBL_HIP(hipMemsetAsync(feat, 0, (size_t)np, c->stream));
    CMBL_LAUNCH(c, K_MASK_POINT, (k_mask_scatter<NTP>), dim3((unsigned)((m.nsrc + NTP - 1) / NTP)), 0, c->stream, feat, yx, m.nsrc, Ny);
    edt_sq(c, feat, I0, I1, found, true);                                    // bleed(sources, src_w) = d2 < src_w^2 (:40-44)
    a.d2s = I0;
    if (apod) {                                                              // cos_apod(.!bleed, src_w): the distance to the nearest bled pixel
      CMBL_LAUNCH(c, K_MASK_POINT, (k_mask_below<NTP>), dim3(gp), 0, c->stream, I0, feat, np, m.src_w * m.src_w);
      edt_sq(c, feat, I0, I1, found, true);
      a.d2p = I0;
    }
  }
  CMBL_LAUNCH(c, K_MASK_POINT, (k_mask_point<T>), dim3(gp), 0, c->stream, a);
  CMBL_HIP(hipStreamSynchronize(c->stream));                                 // the scratch (and `taps`, the source of a host copy) go away on return
}

}  // namespace cmbl
