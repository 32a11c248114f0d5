// HEALPix <-> Cartesian projection (src/proj_healpix.jl): the geometry and the kernels behind cmbl_projector_* and cmbl_project_*.
// All geometry is double whatever the context's precision (a deliberate departure from the reference's T): the ring lookup is
// discontinuous in its index outputs, and a Float32 angle at Nside 2048 is good to 1e-3 of a pixel only.  Field values, the stored weights
// and cos 2ψ / sin 2ψ are T.  RING ordering, pixel indices 0-based.  No atomics: every output element has one writer and one fixed order
// of operations, so results are bit-identical between runs.
//   hpx_pix2ang       pix2angRing (Healpix.jl), the standard RING formulas
//   hpx_ring_info     start pixel, pixel count, colatitude and shift of ring r = 1 ... 4 Nside - 1
//   hpx_interp        the four pixels and weights of healpy.get_interp_val (T_Healpix_Base::get_interpol)
//   CartGeom          θϕ_to_ij / ij_to_θϕ / get_ψpol of ProjLambert (:89-119) and ProjEquiRect (:59-77); ψ from hand-carried tangents
//   k_hpx_cart_table  per Cartesian pixel: θ, ϕ, ψ, cos 2ψ, sin 2ψ, four pixels, four weights
//   k_hpx_flags       per HEALPix pixel: touched (0 < i < Ny+1, 0 < j < Nx+1) and in-patch (1 <= i <= Ny, 1 <= j <= Nx) flags, counts per block
//   k_hpx_compact     the two ascending lists from the flags and the scanned block counts; (i, j), ψ, cos 2ψ, sin 2ψ of the touched pixels
//   k_hpx_to_cart     HEALPix -> Cartesian gather, QU rotation of :243-244 fused
//   k_hpx_to_healpix  Cartesian -> HEALPix gather (Images.bilinear_interpolation, outside = 0), QU rotation of :332-333 fused
//   k_hpx_adjoint     the transpose of either gather: a gather over the CSR of the transposed table, the transposed rotation on the input
#pragma once
#include <cmath>
#include "common.hpp"

namespace cmbl {

constexpr int HPX_MAXNSIDE = 8192;          // npix = 12 Nside^2 < 2^31: pixel indices fit int32
constexpr int HPX_ITEMS = 8;                // consecutive pixels per thread of k_hpx_flags / k_hpx_compact
constexpr int HPX_CHUNK = NTP * HPX_ITEMS;  // ... per workgroup
constexpr double HPX_PI = 3.14159265358979323846, HPX_TWOPI = 6.28318530717958647692, HPX_TWOTHIRD = 2.0 / 3.0;
enum { HPX_LAMBERT = 0, HPX_EQUIRECT = 1 };
enum { HPX_TOUCHED = 1, HPX_INPATCH = 2 };

__host__ __device__ __forceinline__ long hpx_isqrt(long v) {
  long r = (long)sqrt((double)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}
// colatitude of a cap ring from t = ring^2 / (3 Nside^2) = 1 - |z|, without the cancellation of acos near the pole
__host__ __device__ __forceinline__ double hpx_cap_theta(double t) { return atan2(sqrt(t * (2.0 - t)), 1.0 - t); }

__host__ __device__ inline void hpx_pix2ang(long nside, long p, double* theta, double* phi) {
  const long npix = 12 * nside * nside, ncap = 2 * nside * (nside - 1);
  const double n2 = 3.0 * (double)nside * (double)nside;
  if (p < ncap) {
    const long ring = (1 + hpx_isqrt(1 + 2 * p)) >> 1, iphi = p + 1 - 2 * ring * (ring - 1);
    *theta = hpx_cap_theta((double)(ring * ring) / n2);
    *phi = ((double)iphi - 0.5) * HPX_PI / (2.0 * (double)ring);
  } else if (p < npix - ncap) {
    const long ip = p - ncap, ring = ip / (4 * nside) + nside, iphi = ip % (4 * nside) + 1;
    const double fodd = ((ring + nside) & 1) ? 1.0 : 0.5;
    *theta = acos((double)(2 * nside - ring) * 2.0 / (3.0 * (double)nside));
    *phi = ((double)iphi - fodd) * HPX_PI / (2.0 * (double)nside);
  } else {
    const long ip = npix - p, ring = (1 + hpx_isqrt(2 * ip - 1)) >> 1, iphi = 4 * ring + 1 - (ip - 2 * ring * (ring - 1));
    *theta = HPX_PI - hpx_cap_theta((double)(ring * ring) / n2);
    *phi = ((double)iphi - 0.5) * HPX_PI / (2.0 * (double)ring);
  }
}

// ring r = 1 ... 4 Nside - 1, counted from the north pole
__host__ __device__ inline void hpx_ring_info(long nside, long r, long* sp, long* nr, double* theta, bool* shift) {
  const long npix = 12 * nside * nside, ncap = 2 * nside * (nside - 1);
  const double n2 = 3.0 * (double)nside * (double)nside;
  if (r < nside) {
    *nr = 4 * r; *sp = 2 * r * (r - 1); *theta = hpx_cap_theta((double)(r * r) / n2); *shift = true;
  } else if (r <= 3 * nside) {
    *nr = 4 * nside; *sp = ncap + (r - nside) * 4 * nside; *theta = acos((double)(2 * nside - r) * 2.0 / (3.0 * (double)nside));
    *shift = ((r - nside) & 1) == 0;
  } else {
    const long s = 4 * nside - r;
    *nr = 4 * s; *sp = npix - 2 * s * (s + 1); *theta = HPX_PI - hpx_cap_theta((double)(s * s) / n2); *shift = true;
  }
}

// the two pixels of ring r on either side of ϕ (any real ϕ: it comes from an atan, or from a span) and the weight of the second
__host__ __device__ inline double hpx_ring_pair(long nside, long r, double phi, long* p1, long* p2, double* theta) {
  long sp, nr; bool shift;
  hpx_ring_info(nside, r, &sp, &nr, theta, &shift);
  const double t = phi / (HPX_TWOPI / (double)nr) - (shift ? 0.5 : 0.0), fl = floor(t);
  long i1 = (long)fl % nr;
  if (i1 < 0) i1 += nr;
  const long i2 = i1 + 1 < nr ? i1 + 1 : 0;
  *p1 = sp + i1; *p2 = sp + i2;
  return t - fl;
}

// T_Healpix_Base::get_interpol; θ in [0, π] (the caller has checked).  wθ is clamped to [0, 1]: where ring_above and the ring's own colatitude
// disagree by an ulp the interpolant is continuous, so the clamp moves the value by an ulp and keeps every weight >= 0.
__host__ __device__ inline void hpx_interp(long nside, double theta, double phi, long pix[4], double w[4]) {
  const long npix = 12 * nside * nside;
  const double z = cos(theta), az = fabs(z);
  long ir1;
  if (az <= HPX_TWOTHIRD) ir1 = (long)((double)nside * (2.0 - 1.5 * z));
  else {
    const double sh = sin(0.5 * (z > 0 ? theta : HPX_PI - theta));                 // 1 - |z| = 2 sin^2(half the distance to the pole)
    const long ir = (long)((double)nside * sqrt(6.0 * sh * sh));
    ir1 = z > 0 ? ir : 4 * nside - ir - 1;
  }
  ir1 = ir1 < 0 ? 0 : ir1 > 4 * nside - 1 ? 4 * nside - 1 : ir1;
  const long ir2 = ir1 + 1;
  double th1 = 0, th2 = 0;
  if (ir1 > 0) { const double ww = hpx_ring_pair(nside, ir1, phi, &pix[0], &pix[1], &th1); w[0] = 1.0 - ww; w[1] = ww; }
  if (ir2 < 4 * nside) { const double ww = hpx_ring_pair(nside, ir2, phi, &pix[2], &pix[3], &th2); w[2] = 1.0 - ww; w[3] = ww; }
  if (ir1 == 0) {
    const double wt = fmin(fmax(theta / th2, 0.0), 1.0), fac = (1.0 - wt) * 0.25;
    w[2] = w[2] * wt + fac; w[3] = w[3] * wt + fac; w[0] = fac; w[1] = fac;
    pix[0] = (pix[2] + 2) & 3; pix[1] = (pix[3] + 2) & 3;
  } else if (ir2 == 4 * nside) {
    const double wt = fmin(fmax((theta - th1) / (HPX_PI - th1), 0.0), 1.0), fac = wt * 0.25;
    w[0] = w[0] * (1.0 - wt) + fac; w[1] = w[1] * (1.0 - wt) + fac; w[2] = fac; w[3] = fac;
    pix[2] = ((pix[0] + 2) & 3) + npix - 4; pix[3] = ((pix[1] + 2) & 3) + npix - 4;
  } else {
    const double wt = fmin(fmax((theta - th1) / (th2 - th1), 0.0), 1.0);
    w[0] *= 1.0 - wt; w[1] *= 1.0 - wt; w[2] *= wt; w[3] *= wt;
  }
}

// The Cartesian projection as the geometry needs it.  LAMBERT: R = RotZYX(rotator) = Rz Ry Rx (row-major), dx the pixel size in radians.
// With w = R n(θ, ϕ), n = (cos ϕ sin θ, sin ϕ sin θ, cos θ), and (θ', ϕ') the angles of w, the reference's r = 2 cos(θ'/2), x = -r sin ϕ',
// y = -r cos ϕ' are x = -w_y s, y = -w_x s with s = sqrt(2 / (1 - w_z)): the same map without the cancellation of cos(θ'/2) at the patch's
// centre (w_z = -1).  Backwards, with r^2 = x^2 + y^2: w = (-y q, -x q, r^2/2 - 1), q = sqrt(1 - r^2/4).  EQUIRECT: th0 / ph0 the start of the
// spans, dth / dph their lengths (:59-71).
struct CartGeom {
  int kind, Ny, Nx;
  double dx, R[9];
  double th0, dth, ph0, dph;

  __host__ __device__ void ij_to_ang(double i, double j, double* theta, double* phi) const {
    if (kind == HPX_EQUIRECT) { *theta = dth / Ny * i + th0; *phi = dph / Nx * j + ph0; return; }
    const double x = dx * (j - (double)(Nx / 2) - 0.5), y = dx * (i - (double)(Ny / 2) - 0.5);
    const double r2 = x * x + y * y, q = sqrt(1.0 - 0.25 * r2);                     // NaN beyond r = 2: the caller checks θ
    const double w0 = -y * q, w1 = -x * q, w2 = 0.5 * r2 - 1.0;
    const double n0 = R[0] * w0 + R[3] * w1 + R[6] * w2, n1 = R[1] * w0 + R[4] * w1 + R[7] * w2, n2 = R[2] * w0 + R[5] * w1 + R[8] * w2;   // R \ w
    *theta = atan2(sqrt(n0 * n0 + n1 * n1), n2);
    *phi = atan2(n1, n0);
  }
  // (i, j) and, if J is given, J = ∂(i, j)/∂(θ, ϕ) as {J11, J12, J21, J22}
  __host__ __device__ void ang_to_ij(double theta, double phi, double* i, double* j, double* J) const {
    if (kind == HPX_EQUIRECT) {
      double d = fmod(phi - ph0, HPX_TWOPI);                                        // rem2pi(ϕ - φ0, RoundDown)
      if (d < 0) d += HPX_TWOPI;
      *i = (theta - th0) / dth * Ny; *j = d / dph * Nx;
      if (J) { J[0] = Ny / dth; J[1] = 0; J[2] = 0; J[3] = Nx / dph; }
      return;
    }
    const double st = sin(theta), ct = cos(theta), sp = sin(phi), cp = cos(phi);
    const double n[3] = {cp * st, sp * st, ct};
    const double w0 = R[0] * n[0] + R[1] * n[1] + R[2] * n[2], w1 = R[3] * n[0] + R[4] * n[1] + R[5] * n[2], w2 = R[6] * n[0] + R[7] * n[1] + R[8] * n[2];
    const double s = sqrt(2.0 / (1.0 - w2)), ci = (double)(Ny / 2) + 0.5, cj = (double)(Nx / 2) + 0.5;
    *i = -w0 * s / dx + ci; *j = -w1 * s / dx + cj;
    if (!J) return;
    const double dn[2][3] = {{cp * ct, sp * ct, -st}, {-sp * st, cp * st, 0.0}};    // ∂n/∂θ, ∂n/∂ϕ
    for (int k = 0; k < 2; ++k) {
      const double d0 = R[0] * dn[k][0] + R[1] * dn[k][1] + R[2] * dn[k][2], d1 = R[3] * dn[k][0] + R[4] * dn[k][1] + R[5] * dn[k][2],
                   d2 = R[6] * dn[k][0] + R[7] * dn[k][1] + R[8] * dn[k][2];
      const double ds = 0.5 * s / (1.0 - w2) * d2;
      J[k] = -(d0 * s + w0 * ds) / dx; J[2 + k] = -(d1 * s + w1 * ds) / dx;
    }
  }
  // get_ψpol: 0 for EQUIRECT (:75-77); (atan(J11, J21) + atan(-J22, J12) - π) / 2 for LAMBERT (:114-119)
  __host__ __device__ double psi(const double* J) const { return kind == HPX_EQUIRECT ? 0.0 : 0.5 * (atan2(J[0], J[2]) + atan2(-J[3], J[1]) - HPX_PI); }
};

template <typename T> struct HpxCartTab {            // per Cartesian pixel c = (j - 1) Ny + (i - 1), the order of a map plane
  double* theta; double* phi; double* psi;
  T* c2; T* s2;
  int4* pix;
  T* w;                                              // [c][4]
  int* bad;                                          // raised where θ is outside [0, π] or not a number
};

// grid ceil(Ny Nx / NTP)
template <typename T>
__global__ __launch_bounds__(NTP) void k_hpx_cart_table(const CartGeom g, int nside, const HpxCartTab<T> t) {
  const long c = (long)blockIdx.x * NTP + threadIdx.x;
  if (c >= (long)g.Ny * g.Nx) return;
  const int jx = (int)(c / g.Ny), iy = (int)(c - (long)jx * g.Ny);
  double th, ph, i, j, J[4];
  g.ij_to_ang((double)(iy + 1), (double)(jx + 1), &th, &ph);
  t.theta[c] = th; t.phi[c] = ph;
  if (!(th >= 0.0 && th <= HPX_PI)) {
    *t.bad = 1;
    t.psi[c] = 0; t.c2[c] = 1; t.s2[c] = 0; t.pix[c] = make_int4(0, 0, 0, 0);
    for (int k = 0; k < 4; ++k) t.w[4 * c + k] = 0;
    return;
  }
  g.ang_to_ij(th, ph, &i, &j, J);
  const double psi = g.psi(J);
  t.psi[c] = psi; t.c2[c] = (T)cos(2.0 * psi); t.s2[c] = (T)sin(2.0 * psi);
  long pix[4]; double w[4];
  hpx_interp(nside, th, ph, pix, w);
  t.pix[c] = make_int4((int)pix[0], (int)pix[1], (int)pix[2], (int)pix[3]);
  for (int k = 0; k < 4; ++k) t.w[4 * c + k] = (T)w[k];
}

__host__ __device__ __forceinline__ int hpx_flag_of(const CartGeom& g, double i, double j) {
  int f = 0;
  if (i > 0.0 && i < (double)(g.Ny + 1) && j > 0.0 && j < (double)(g.Nx + 1)) f |= HPX_TOUCHED;
  if (i >= 1.0 && i <= (double)g.Ny && j >= 1.0 && j <= (double)g.Nx) f |= HPX_INPATCH;
  return f;
}

// sums of (a, b) over the workgroup's threads, exclusive prefix of the calling thread returned in *ea / *eb.  Hillis-Steele over NTP slots.
template <int NT>
__device__ __forceinline__ void hpx_block_scan2(int a, int b, int* ea, int* eb, int* ta, int* tb) {
  __shared__ int sa[2][NT], sb[2][NT];
  const int t = threadIdx.x;
  sa[0][t] = a; sb[0][t] = b;
  __syncthreads();
  int cur = 0;
  for (int s = 1; s < NT; s <<= 1, cur ^= 1) {
    sa[cur ^ 1][t] = t >= s ? sa[cur][t] + sa[cur][t - s] : sa[cur][t];
    sb[cur ^ 1][t] = t >= s ? sb[cur][t] + sb[cur][t - s] : sb[cur][t];
    __syncthreads();
  }
  *ea = sa[cur][t] - a; *eb = sb[cur][t] - b;
  *ta = sa[cur][NT - 1]; *tb = sb[cur][NT - 1];
  __syncthreads();
}

// Thread t of workgroup g owns the pixels [g HPX_CHUNK + t HPX_ITEMS, ... + HPX_ITEMS).  flags[npix]; counts[2][nblocks]: touched, in-patch.
// grid ceil(npix / HPX_CHUNK)
template <typename T>
__global__ __launch_bounds__(NTP) void k_hpx_flags(const CartGeom g, int nside, long npix, unsigned char* __restrict__ flags, int* __restrict__ counts) {
  const long p0 = (long)blockIdx.x * HPX_CHUNK + (long)threadIdx.x * HPX_ITEMS;
  int na = 0, nb = 0;
  for (int k = 0; k < HPX_ITEMS; ++k) {
    const long p = p0 + k;
    if (p >= npix) break;
    double th, ph, i, j;
    hpx_pix2ang(nside, p, &th, &ph);
    g.ang_to_ij(th, ph, &i, &j, nullptr);
    const int f = hpx_flag_of(g, i, j);
    flags[p] = (unsigned char)f;
    na += f & 1; nb += (f >> 1) & 1;
  }
  int ea, eb, ta, tb;
  hpx_block_scan2<NTP>(na, nb, &ea, &eb, &ta, &tb);
  if (threadIdx.x == 0) { counts[blockIdx.x] = ta; counts[gridDim.x + blockIdx.x] = tb; }
}

template <typename T> struct HpxLists {
  int* touched; double* ti; double* tj; double* tpsi; T* tc2; T* ts2;   // n_touched each, ascending pixel index
  int* inpatch;                                                        // n_inpatch, ascending
  int n_touched, n_inpatch;
};

// offsets[2][nblocks]: the exclusive scan of k_hpx_flags' counts.  Same ownership of pixels as k_hpx_flags; a slot beyond the list lengths
// the host allocated from the same counts cannot occur, and is refused all the same.
template <typename T>
__global__ __launch_bounds__(NTP) void k_hpx_compact(const CartGeom g, int nside, long npix, const unsigned char* __restrict__ flags,
                                                     const int* __restrict__ offsets, const HpxLists<T> L) {
  const long p0 = (long)blockIdx.x * HPX_CHUNK + (long)threadIdx.x * HPX_ITEMS;
  int na = 0, nb = 0;
  for (int k = 0; k < HPX_ITEMS; ++k) {
    const long p = p0 + k;
    if (p >= npix) break;
    const int f = flags[p];
    na += f & 1; nb += (f >> 1) & 1;
  }
  int ea, eb, ta, tb;
  hpx_block_scan2<NTP>(na, nb, &ea, &eb, &ta, &tb);
  int sa = offsets[blockIdx.x] + ea, sb = offsets[gridDim.x + blockIdx.x] + eb;
  for (int k = 0; k < HPX_ITEMS; ++k) {
    const long p = p0 + k;
    if (p >= npix) break;
    const int f = flags[p];
    if (f & HPX_INPATCH) { if (sb < L.n_inpatch) L.inpatch[sb] = (int)p; ++sb; }
    if (f & HPX_TOUCHED) {
      if (sa < L.n_touched) {
        double th, ph, i, j, J[4];
        hpx_pix2ang(nside, p, &th, &ph);
        g.ang_to_ij(th, ph, &i, &j, J);
        const double psi = g.psi(J);
        L.touched[sa] = (int)p; L.ti[sa] = i; L.tj[sa] = j; L.tpsi[sa] = psi;
        L.tc2[sa] = (T)cos(2.0 * psi); L.ts2[sa] = (T)sin(2.0 * psi);
      }
      ++sa;
    }
  }
}

// HEALPix (npix, npol, nbatch) -> maps (Ny, Nx, npol, nbatch): one thread per Cartesian pixel; the four pixels and weights are read once and
// reused over all slices.  Each value is four multiply-adds in T in a fixed order.  QU (the last two of npol = 2, 3) are rotated as in
// :243-244: Q' = Q cos 2ψ - U sin 2ψ, U' = U cos 2ψ + Q sin 2ψ.  grid ceil(Ny Nx / NTP)
template <typename T>
__global__ __launch_bounds__(NTP) void k_hpx_to_cart(const T* __restrict__ hpx, T* __restrict__ out, const int4* __restrict__ pix, const T* __restrict__ w,
                                                     const T* __restrict__ c2, const T* __restrict__ s2, long ncart, long npix, int npol, int nbatch) {
  const long c = (long)blockIdx.x * NTP + threadIdx.x;
  if (c >= ncart) return;
  const int4 p = pix[c];
  const T w0 = w[4 * c], w1 = w[4 * c + 1], w2 = w[4 * c + 2], w3 = w[4 * c + 3];
  const T cc = c2[c], ss = s2[c];
  auto val = [&](const T* h) { return fma(w3, h[p.w], fma(w2, h[p.z], fma(w1, h[p.y], w0 * h[p.x]))); };
  for (int b = 0; b < nbatch; ++b) {
    const T* hb = hpx + (long)b * npol * npix;
    T* ob = out + (long)b * npol * ncart + c;
    int q = 0;
    if (npol != 2) { ob[0] = val(hb); q = 1; }
    if (npol >= 2) {
      const T Q = val(hb + (long)q * npix), U = val(hb + (long)(q + 1) * npix);
      ob[(long)q * ncart] = fma(-U, ss, Q * cc);
      ob[(long)(q + 1) * ncart] = fma(Q, ss, U * cc);
    }
  }
}

// maps (Ny, Nx, npol, nbatch) -> HEALPix (npix, npol, nbatch), which the host has zeroed: one thread per touched pixel.
// Images.bilinear_interpolation(img, i, j): corners (⌊i⌋, ⌊j⌋), (⌈i⌉, ⌊j⌋), (⌊i⌋, ⌈j⌉), (⌈i⌉, ⌈j⌉), 1-based, weights the products of
// (1 - i + ⌊i⌋), (i - ⌊i⌋) and likewise in j, a corner outside the array counts as zero.  The weights are formed in double and rounded
// once.  QU as in :332-333: Q' = Q cos 2ψ + U sin 2ψ, U' = U cos 2ψ - Q sin 2ψ.  grid ceil(n_touched / NTP)
template <typename T>
__global__ __launch_bounds__(NTP) void k_hpx_to_healpix(const T* __restrict__ map, T* __restrict__ hpx, const HpxLists<T> L, int Ny, int Nx, long npix,
                                                        int npol, int nbatch) {
  const int t = blockIdx.x * NTP + threadIdx.x;
  if (t >= L.n_touched) return;
  const long p = L.touched[t];
  const double i = L.ti[t], j = L.tj[t], fi = floor(i), fj = floor(j), ci = ceil(i), cj = ceil(j);
  const double wy[2] = {1.0 - i + fi, i - fi}, wx[2] = {1.0 - j + fj, j - fj};
  const int ys[2] = {(int)fi, (int)ci}, xs[2] = {(int)fj, (int)cj};
  T wt[4]; long off[4];
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      const bool in = ys[b] >= 1 && ys[b] <= Ny && xs[a] >= 1 && xs[a] <= Nx;
      wt[2 * a + b] = in ? (T)(wy[b] * wx[a]) : T(0);
      off[2 * a + b] = in ? (long)(xs[a] - 1) * Ny + (ys[b] - 1) : 0;
    }
  const T cc = L.tc2[t], ss = L.ts2[t];
  const long ncart = (long)Ny * Nx;
  auto val = [&](const T* m) { return fma(wt[3], m[off[3]], fma(wt[2], m[off[2]], fma(wt[1], m[off[1]], wt[0] * m[off[0]]))); };
  for (int b = 0; b < nbatch; ++b) {
    const T* mb = map + (long)b * npol * ncart;
    T* hb = hpx + (long)b * npol * npix + p;
    int q = 0;
    if (npol != 2) { hb[0] = val(mb); q = 1; }
    if (npol >= 2) {
      const T Q = val(mb + (long)q * ncart), U = val(mb + (long)(q + 1) * ncart);
      hb[(long)q * npix] = fma(U, ss, Q * cc);
      hb[(long)(q + 1) * npix] = fma(-Q, ss, U * cc);
    }
  }
}

// ---- the transposes (pullbacks) of the two gathers ---------------------------------------------------------------------------------------
// Both are gathers over a CSR of the transposed table (engine_healpix.hpp builds it): a row is an OUTPUT element, its entries the (input
// element, corner) pairs that read it in the forward direction, ordered by ascending input element, then by corner.
//   to_cart^T     row = a HEALPix pixel some Cartesian pixel reads (rowout), entry = Cartesian pixel c (its value, cos 2ψ_c, sin 2ψ_c), weight w[c][k]
//   to_healpix^T  row = a Cartesian pixel (all of them, rowout null), entry = slot t of the touched list (value at src[t] = the pixel, ψ_t), weight v[t][k]
template <typename T> struct HpxCsr {
  const int* rowstart;                               // nrows + 1
  const int* rowout;                                 // output element of row r; null: r itself
  const int* ent;                                    // per entry: slot of the forward table
  const T* val;                                      // per entry: the forward weight, as the forward kernel rounds it
  const int* src;                                    // input element of a slot; null: the slot itself
  const T* c2; const T* s2;                          // per slot
  int nrows;
};
constexpr int HPX_ADJ_NT = 64;                       // one wave per workgroup: a long row holds back its own wave and nothing else
constexpr int HPX_ADJ_NB = 4;                        // batch entries per pass over a row (NP * HPX_ADJ_NB accumulators in registers)
constexpr int HPX_ADJ_AHEAD = 4;                     // entries whose loads are issued together

// out[o_r] = Σ_entries val * (R^T in[src])  for every slice: one thread per row, the row summed in its stored order in T, one fma per entry
// (bit-identical between runs, the contract of k_bl_csr); an entry is read once per HPX_ADJ_NB batch entries and reused over their planes.
// The rotation acts on the INPUT, at the entry's ψ: TO_SPHERE (to_cart^T) Q' = Q cos 2ψ + U sin 2ψ, U' = U cos 2ψ - Q sin 2ψ (the transpose of
// :243-244); otherwise (to_healpix^T) Q' = Q cos 2ψ - U sin 2ψ, U' = U cos 2ψ + Q sin 2ψ (the transpose of :332-333).  Rows have any length:
// there is no bound and no barrier, and the waves of a launch retire independently.  A row without entries writes 0.
// in (nin, NP, nbatch), out (nout, NP, nbatch).  grid ceil(nrows / HPX_ADJ_NT), HPX_ADJ_NT threads
template <typename T, int NP, bool TO_SPHERE>
__global__ __launch_bounds__(HPX_ADJ_NT) void k_hpx_adjoint(const T* __restrict__ in, T* __restrict__ out, const HpxCsr<T> A, long nin, long nout, int nbatch) {
  const int r = blockIdx.x * HPX_ADJ_NT + threadIdx.x;
  if (r >= A.nrows) return;
  const int s = A.rowstart[r], e = A.rowstart[r + 1];
  const long o = A.rowout ? A.rowout[r] : r;
  for (int b0 = 0; b0 < nbatch; b0 += HPX_ADJ_NB) {
    const int nb = nbatch - b0 < HPX_ADJ_NB ? nbatch - b0 : HPX_ADJ_NB;
    T acc[HPX_ADJ_NB][NP];
#pragma unroll
    for (int q = 0; q < HPX_ADJ_NB; ++q)
#pragma unroll
      for (int k = 0; k < NP; ++k) acc[q][k] = 0;
    // one entry: the dependent loads slot -> (pixel, cos, sin) -> values, then the row's next fma
    auto add = [&](int k, T v) {
      const long i = A.src ? A.src[k] : k;
      T cc = 1, ss = 0;
      if constexpr (NP >= 2) { cc = A.c2[k]; ss = A.s2[k]; }
#pragma unroll
      for (int q = 0; q < HPX_ADJ_NB; ++q)
        if (q < nb) {
          const T* ib = in + (long)(b0 + q) * NP * nin + i;
          if constexpr (NP != 2) acc[q][0] = fma(v, ib[0], acc[q][0]);
          if constexpr (NP >= 2) {
            const T Q = ib[(long)(NP - 2) * nin], U = ib[(long)(NP - 1) * nin];
            const T rq = TO_SPHERE ? fma(U, ss, Q * cc) : fma(-U, ss, Q * cc);
            const T ru = TO_SPHERE ? fma(-Q, ss, U * cc) : fma(Q, ss, U * cc);
            acc[q][NP - 2] = fma(v, rq, acc[q][NP - 2]);
            acc[q][NP - 1] = fma(v, ru, acc[q][NP - 1]);
          }
        }
    };
    // HPX_ADJ_AHEAD entries at a time, so that their chains of dependent loads overlap; the fma chain keeps the stored order
    int p = s;
    for (; p + HPX_ADJ_AHEAD <= e; p += HPX_ADJ_AHEAD) {
      int k[HPX_ADJ_AHEAD]; T v[HPX_ADJ_AHEAD];
#pragma unroll
      for (int u = 0; u < HPX_ADJ_AHEAD; ++u) { k[u] = A.ent[p + u]; v[u] = A.val[p + u]; }
#pragma unroll
      for (int u = 0; u < HPX_ADJ_AHEAD; ++u) add(k[u], v[u]);
    }
    for (; p < e; ++p) add(A.ent[p], A.val[p]);
#pragma unroll
    for (int q = 0; q < HPX_ADJ_NB; ++q)
      if (q < nb)
#pragma unroll
        for (int k = 0; k < NP; ++k) out[((long)(b0 + q) * NP + k) * nout + o] = acc[q][k];
  }
}

}  // namespace cmbl
