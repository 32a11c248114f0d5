// The θ-dependent operators of a data set, evaluated on the device (cmbl_dataset_theta_model / cmbl_logpdf_mixed_theta):
//   Cf(θ) = Cfs(bandpower amplitudes) + (r/r0) Cten,  Cϕ(Aϕ) = Cϕ0 Aϕ / Aϕ0,  D(r) = sqrt((C + 2 Cn^ + σ²len) C⁻¹) with C = Cfs + (r/r0) Cten,
//   G(Aϕ) = g0⁻¹ sqrt(1 + 2 Nϕ Cϕ(Aϕ)⁻¹)                                              (src/dataset.jl:272-274, 316-328)
// One pointwise pass over the half plane (F layout, [ky][x slot]) writes pinv(Cf), pinv(D), pinv(Cϕ), pinv(G) in the context's precision and
// leaves per workgroup the partial sums of  logdet Cf + logdet Cϕ,  logdet(D0⁻¹ D)  and  logdet G;  k_theta_sum adds them in a fixed order.
// The DEFINITION of every formula is the host algebra of theta._ops / sim.HarmOp (the 2 x 2 TE block reads the ET plane for both
// off-diagonals, `+ scalar` touches TT, EE, BB, pinv is 1/x with every non-finite result replaced by 0, logdet skips non-finite terms).
// All arithmetic is double in either precision, only the store rounds, and NO product is contracted into a following sum or difference:
// pinv is discontinuous at 0, and a determinant TT EE - ET² that is exactly 0 in separately rounded arithmetic (ℓ = 0, modes outside the
// spectra, fully correlated modes) is a tiny non-zero number when the compiler fuses the subtraction -- hence the pragma in every function.
#pragma once
#include <type_traits>
#include "common.hpp"

namespace cmbl {

constexpr int TH_MAXBANDS = 3;             // TT, TE, EE: BB is never rescaled (src/proj_lambert.jl:385-393)
constexpr int TH_MAXBLK = 1024;            // workgroups of the pass = partial sums per logdet

// the arguments of cmbl_dataset_theta_model (host pointers, reference layout)
struct ThetaModelArgs {
  const double* cfs; int nplanes; const double* c0; int nbands; const int* band_planes; const int32_t* band_idx; const int* band_nbins;
  const double *cten, *cn; double s2len, r0; const double* cphi0; double aphi0; const double *nphi, *g; double logdet_cn;
};

// The helpers below are templates on the scalar type S: double for the operators themselves, ThDual<N> (a value with N tangents, forward
// mode) for their θ-derivatives in k_theta_grad -- the derivative is the derivative of exactly the formulas that define the operators.
// pinv keeps its discontinuity (tangent 0 where the value is replaced by 0), a skipped log term has tangent 0, and sqrt(0) has tangent 0.
template <int N> struct ThDual { double v; double d[N]; };

__host__ __device__ inline double th_val(double x) { return x; }
template <int N> __host__ __device__ inline double th_val(const ThDual<N>& x) { return x.v; }
template <typename S> __host__ __device__ inline S th_const(double x) {
  if constexpr (std::is_same<S, double>::value) return x;
  else { S r{}; r.v = x; return r; }
}
template <int N> __host__ __device__ inline ThDual<N> operator+(const ThDual<N>& x, const ThDual<N>& y) {
#pragma clang fp contract(off)
  ThDual<N> r; r.v = x.v + y.v;
  for (int i = 0; i < N; ++i) r.d[i] = x.d[i] + y.d[i];
  return r;
}
template <int N> __host__ __device__ inline ThDual<N> operator+(const ThDual<N>& x, double y) { ThDual<N> r = x; r.v = x.v + y; return r; }
template <int N> __host__ __device__ inline ThDual<N> operator+(double y, const ThDual<N>& x) { ThDual<N> r = x; r.v = y + x.v; return r; }
template <int N> __host__ __device__ inline ThDual<N> operator-(const ThDual<N>& x, const ThDual<N>& y) {
#pragma clang fp contract(off)
  ThDual<N> r; r.v = x.v - y.v;
  for (int i = 0; i < N; ++i) r.d[i] = x.d[i] - y.d[i];
  return r;
}
template <int N> __host__ __device__ inline ThDual<N> operator-(const ThDual<N>& x) {
  ThDual<N> r; r.v = -x.v;
  for (int i = 0; i < N; ++i) r.d[i] = -x.d[i];
  return r;
}
template <int N> __host__ __device__ inline ThDual<N> operator*(const ThDual<N>& x, const ThDual<N>& y) {
#pragma clang fp contract(off)
  ThDual<N> r; r.v = x.v * y.v;
  for (int i = 0; i < N; ++i) { const double p = x.d[i] * y.v, q = x.v * y.d[i]; r.d[i] = p + q; }
  return r;
}
template <int N> __host__ __device__ inline ThDual<N> operator*(const ThDual<N>& x, double y) {
#pragma clang fp contract(off)
  ThDual<N> r; r.v = x.v * y;
  for (int i = 0; i < N; ++i) r.d[i] = x.d[i] * y;
  return r;
}
template <int N> __host__ __device__ inline ThDual<N> operator*(double y, const ThDual<N>& x) {
#pragma clang fp contract(off)
  ThDual<N> r; r.v = y * x.v;
  for (int i = 0; i < N; ++i) r.d[i] = y * x.d[i];
  return r;
}
template <int N> __host__ __device__ inline ThDual<N> operator/(const ThDual<N>& x, double y) {
#pragma clang fp contract(off)
  ThDual<N> r; r.v = x.v / y;
  for (int i = 0; i < N; ++i) r.d[i] = x.d[i] / y;
  return r;
}
// 1 / x: the tangent is formed as -(x' v) v, so that a tangent that is exactly 0 stays 0 however large v is
template <int N> __host__ __device__ inline ThDual<N> operator/(double y, const ThDual<N>& x) {
#pragma clang fp contract(off)
  ThDual<N> r; const double v = 1.0 / x.v; r.v = y / x.v;
  for (int i = 0; i < N; ++i) r.d[i] = -((x.d[i] * v) * r.v);
  return r;
}
__host__ __device__ inline double th_sqrt1(double x) { return sqrt(x); }
template <int N> __host__ __device__ inline ThDual<N> th_sqrt1(const ThDual<N>& x) {
#pragma clang fp contract(off)
  ThDual<N> r; r.v = sqrt(x.v);
  const double k = r.v > 0 ? 0.5 / r.v : 0.0;
  for (int i = 0; i < N; ++i) r.d[i] = r.v > 0 ? x.d[i] * k : 0.0;
  return r;
}
__host__ __device__ inline double th_logabs(double x) { return log(fabs(x)); }
template <int N> __host__ __device__ inline ThDual<N> th_logabs(const ThDual<N>& x) {
#pragma clang fp contract(off)
  ThDual<N> r; r.v = log(fabs(x.v));
  for (int i = 0; i < N; ++i) r.d[i] = x.d[i] / x.v;
  return r;
}

template <typename S> struct ThBlkT { S a, b, c, d, e; };    // BlockDiagIEB planes (TT, TE, ET, EE, BB) of one mode
using ThBlk = ThBlkT<double>;

template <typename S> __host__ __device__ inline S th_pinv(const S& x) {
#pragma clang fp contract(off)
  const S r = 1.0 / x;
  return __builtin_isfinite(th_val(r)) ? r : th_const<S>(0.0);
}
// one term of Σ λ log|x|, non-finite terms skipped (src/proj_lambert.jl:331-336)
template <typename S> __host__ __device__ inline S th_logterm(const S& x, double lam) {
#pragma clang fp contract(off)
  const S v = th_logabs(x) * lam;
  return __builtin_isfinite(th_val(v)) ? v : th_const<S>(0.0);
}
template <typename S, typename S2> __host__ __device__ inline ThBlkT<S> th_add(const ThBlkT<S>& x, const ThBlkT<S2>& y) {
#pragma clang fp contract(off)
  return {x.a + y.a, x.b + y.b, x.c + y.c, x.d + y.d, x.e + y.e};
}
template <typename S> __host__ __device__ inline ThBlkT<S> th_scale(const ThBlk& x, const S& s) {
#pragma clang fp contract(off)
  return {x.a * s, x.b * s, x.c * s, x.d * s, x.e * s};
}
template <typename S, typename S2> __host__ __device__ inline ThBlkT<S2> th_mm(const ThBlkT<S>& x, const ThBlkT<S2>& y) {
#pragma clang fp contract(off)
  const S2 p1 = x.a * y.a, p2 = x.b * y.c, p3 = x.a * y.b, p4 = x.b * y.d, p5 = x.c * y.a, p6 = x.d * y.c, p7 = x.c * y.b, p8 = x.d * y.d;
  return {p1 + p2, p3 + p4, p5 + p6, p7 + p8, x.e * y.e};
}
template <typename S> __host__ __device__ inline S th_det(const ThBlkT<S>& x) {
#pragma clang fp contract(off)
  const S p = x.a * x.d, q = x.c * x.c;
  return p - q;
}
template <typename S> __host__ __device__ inline ThBlkT<S> th_pinv(const ThBlkT<S>& x) {                 // src/field_vectors.jl:80-84
#pragma clang fp contract(off)
  const S idet = th_pinv(th_det(x));
  const S o = -(x.c * idet);
  return {x.d * idet, o, o, x.a * idet, th_pinv(x.e)};
}
template <typename S> __host__ __device__ inline ThBlkT<S> th_sqrt(const ThBlkT<S>& x) {                 // src/field_vectors.jl:68-73
#pragma clang fp contract(off)
  const S s = th_sqrt1(th_det(x));
  const S s2 = 2.0 * s;
  const S t = th_pinv(th_sqrt1(x.a + (x.d + s2)));
  const S o = t * x.c;
  return {t * (x.a + s), o, o, t * (x.d + s), th_sqrt1(x.e)};
}
// D = sqrt((C + N2) C⁻¹), N2 = 2 Cn^ + σ²len already formed (src/dataset.jl:322-328)
template <typename S> __host__ __device__ inline ThBlkT<S> th_mix(const ThBlkT<S>& C, const ThBlk& N2) { return th_sqrt(th_mm(th_add(C, N2), th_pinv(C))); }
__host__ __device__ inline ThBlk th_noise2(const ThBlk& cn, double s2len) {
#pragma clang fp contract(off)
  const ThBlk n = th_scale(cn, 2.0);
  return {n.a + s2len, n.b, n.c, n.d + s2len, n.e + s2len};
}
// the same for one plane of a diagonal operator
template <typename S> __host__ __device__ inline S th_mix(const S& C, double cn, double s2len) {
#pragma clang fp contract(off)
  const double n2 = cn * 2.0 + s2len;
  const S m = (C + n2) * th_pinv(C);
  return th_sqrt1(m);
}
template <typename S> __host__ __device__ inline S th_g(double nphi, const S& cphi) {          // sqrt(1 + 2 Nϕ Cϕ⁻¹)
#pragma clang fp contract(off)
  const S t = (2 * nphi) * th_pinv(cphi);
  return th_sqrt1(1.0 + t);
}

// What the pass reads (all double, F layout, resident) and where it writes
struct ThetaDev {
  const double *cfs, *c0, *cten, *cn, *d0inv;   // np planes each; c0 (bandpower base) may be nullptr: then cfs
  const double *cphi0, *nphi, *g0inv, *guser;   // one plane each; guser may be nullptr
  const int* bidx[TH_MAXBANDS];                 // bin index of every mode, per band; value nb[k] = the constant amplitude 1
  int bmask[TH_MAXBANDS], bnb[TH_MAXBANDS], boff[TH_MAXBANDS], nbands;
  int np, Nx, Ny, Nyh;
  long pl;
  double s2len, aphi0;
};
struct ThetaPoint {
  double s, aphi;                // r / r0 (1 when r is not named), Aϕ (Aϕ0 when not named)
  int r_named, g_theta;          // r named: logdet(D0⁻¹ D) is formed; g_theta: Aϕ named and no fixed G: G(Aϕ) and logdet G are formed
  const double* amps;            // the amplitude vectors of this θ, bands concatenated; nullptr: ones
};

__device__ __forceinline__ double th_amp(const ThetaDev& m, const ThetaPoint& t, int k, long j) {
  if (!(m.bmask[k])) return 1.0;
  const int i = m.bidx[k][j];
  return (t.amps == nullptr || i >= m.bnb[k]) ? 1.0 : t.amps[m.boff[k] + i];
}

// grid: nblk workgroups (<= TH_MAXBLK) of NTP threads, grid-stride over the half plane; part[3][nblk]
template <typename T, bool BLOCK>
__global__ __launch_bounds__(NTP) void k_theta_ops(ThetaDev m, ThetaPoint t, T* __restrict__ cf_inv, T* __restrict__ d_inv, T* __restrict__ cphi_inv,
                                                    T* __restrict__ g_inv, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[3][NTP / 64];
  double acc[3] = {0.0, 0.0, 0.0};
  const long pl = m.pl;
  for (long j = (long)blockIdx.x * NTP + threadIdx.x; j < pl; j += (long)gridDim.x * NTP) {
    const int ky = (int)(j / m.Nx);
    const double lam = (ky == 0 || (m.Ny % 2 == 0 && ky == m.Nyh - 1)) ? 1.0 : 2.0;
    const double* base = m.c0 ? m.c0 : m.cfs;
    if constexpr (BLOCK) {
      ThBlk cb{base[j], base[pl + j], base[2 * pl + j], base[3 * pl + j], base[4 * pl + j]};
      for (int k = 0; k < m.nbands; ++k) {
        const double a = th_amp(m, t, k, j);
        if (m.bmask[k] & 1) cb.a = a * cb.a;
        if (m.bmask[k] & 2) cb.b = a * cb.b;
        if (m.bmask[k] & 4) cb.c = a * cb.c;
        if (m.bmask[k] & 8) cb.d = a * cb.d;
      }
      const ThBlk ten = th_scale(ThBlk{m.cten[j], m.cten[pl + j], m.cten[2 * pl + j], m.cten[3 * pl + j], m.cten[4 * pl + j]}, t.s);
      const ThBlk cf = th_add(cb, ten);
      const ThBlk cfi = th_pinv(cf);
      acc[0] += th_logterm(th_det(cf), lam);
      acc[0] += th_logterm(cf.e, lam);
      const ThBlk cs{m.cfs[j], m.cfs[pl + j], m.cfs[2 * pl + j], m.cfs[3 * pl + j], m.cfs[4 * pl + j]};
      const ThBlk n2 = th_noise2(ThBlk{m.cn[j], m.cn[pl + j], m.cn[2 * pl + j], m.cn[3 * pl + j], m.cn[4 * pl + j]}, m.s2len);
      const ThBlk D = th_mix(th_add(cs, ten), n2);
      const ThBlk Di = th_pinv(D);
      if (t.r_named) {
        const ThBlk q = th_mm(ThBlk{m.d0inv[j], m.d0inv[pl + j], m.d0inv[2 * pl + j], m.d0inv[3 * pl + j], m.d0inv[4 * pl + j]}, D);
        acc[1] += th_logterm(th_det(q), lam);
        acc[1] += th_logterm(q.e, lam);
      }
      cf_inv[j] = (T)cfi.a; cf_inv[pl + j] = (T)cfi.b; cf_inv[2 * pl + j] = (T)cfi.c; cf_inv[3 * pl + j] = (T)cfi.d; cf_inv[4 * pl + j] = (T)cfi.e;
      d_inv[j] = (T)Di.a; d_inv[pl + j] = (T)Di.b; d_inv[2 * pl + j] = (T)Di.c; d_inv[3 * pl + j] = (T)Di.d; d_inv[4 * pl + j] = (T)Di.e;
    } else {
      for (int p = 0; p < m.np; ++p) {
        const long o = p * pl + j;
        double cb = base[o];
        for (int k = 0; k < m.nbands; ++k) if (m.bmask[k] & (1 << p)) cb = th_amp(m, t, k, j) * cb;
        const double ten = m.cten[o] * t.s;
        const double cf = cb + ten;
        acc[0] += th_logterm(cf, lam);
        const double D = th_mix(m.cfs[o] + ten, m.cn[o], m.s2len);
        if (t.r_named) acc[1] += th_logterm(m.d0inv[o] * D, lam);
        cf_inv[o] = (T)th_pinv(cf);
        d_inv[o] = (T)th_pinv(D);
      }
    }
    const double cphi = m.cphi0[j] * t.aphi / m.aphi0;
    acc[0] += th_logterm(cphi, lam);
    cphi_inv[j] = (T)th_pinv(cphi);
    double G = m.guser ? m.guser[j] : 1.0;
    if (t.g_theta) {
      G = m.g0inv[j] * th_g(m.nphi[j], cphi);
      acc[2] += th_logterm(G, lam);
    }
    g_inv[j] = (T)th_pinv(G);
  }
  // fixed-order sum of the workgroup: lanes by shuffle, wavefronts in index order
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double r = 0;
    for (int w = 0; w < NTP / 64; ++w) r += red[threadIdx.x][w];
    part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = r;
  }
}

// out[k] = Σ_g part[k][g], one workgroup, the same order in every run
static __global__ __launch_bounds__(NTP) void k_theta_sum(const double* __restrict__ part, int nblk, double* __restrict__ out) {
  __shared__ double red[3][NTP / 64];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double v = 0;
    for (int i = threadIdx.x; i < nblk; i += NTP) v += part[(size_t)k * nblk + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double r = 0;
    for (int w = 0; w < NTP / 64; ++w) r += red[threadIdx.x][w];
    out[threadIdx.x] = r;
  }
}

// ---- θ-gradient of logpdf(ds; f, ϕ, θ) and of logpdf(Mixed(ds); f°, ϕ°, θ) (cmbl_grad_theta_logpdf / cmbl_grad_theta_logpdf_mixed) ----
// With lp(f, ϕ, θ) = −½ [⟨f, pinv(Cf) f⟩ + logdet Cf + ⟨ϕ, pinv(Cϕ) ϕ⟩ + logdet Cϕ] + (terms without θ), ⟨a, b⟩ = Σ λ Re(conj a · b) / (Ny Nx):
//   unmixed  ∂lp/∂θ_k at fixed (f, ϕ): the tangent of the expression above, mode by mode;
//   mixed    ϕ = G⁻¹ ϕ°, f = D⁻¹ f^, f^ = L(ϕ)⁻¹ f°, ĝ = ∂lp/∂f^, gϕ° = ∂lp/∂ϕ°:
//            d/dr  += −⟨ĝ, (∂D/∂r) f⟩ − ∂/∂r logdet(D0⁻¹ D),      d/dAϕ += −⟨gϕ°, (∂lnG/∂Aϕ) ϕ°⟩ − ∂/∂Aϕ logdet G      (G(Aϕ) only without a fixed G)
// The operators are evaluated with ThDual: Cf carries the tangents of r and of the band amplitudes (one mode lies in one bin per band, so one
// tangent per band), D that of r, Cϕ and G that of Aϕ.  want: bit 0 r, bit 1 Aϕ, bit 2 the amplitudes; what is not wanted is not formed.
enum { TH_WANT_R = 1, TH_WANT_APHI = 2, TH_WANT_AMPS = 4 };
constexpr int TH_CHUNK = 1024;             // entries of a sorted per-band mode list that one workgroup of k_theta_bins adds

template <typename T> struct ThetaFields {   // F layout; harmonic fields [slot][pol][mode], ϕ-like fields [slot][mode]
  const cx<T>* f; const cx<T>* phi;          // f (harmonic), ϕ
  const cx<T>* ghat; const cx<T>* phio; const cx<T>* gphio;   // mixed form only: ĝ (harmonic), ϕ°, gϕ°
};
struct ThChunk { int start, count, band, amp; };   // a run of one band's sorted mode list inside one bin; amp = boff[band] + bin

template <typename T> __device__ __forceinline__ double th_re(cx<T> a, cx<T> b) {                     // Re(conj a · b)
#pragma clang fp contract(off)
  const double p = (double)a.x * (double)b.x, q = (double)a.y * (double)b.y;
  return p + q;
}

// grid: (nblk <= TH_MAXBLK, nbatch) workgroups of NTP threads, grid-stride over the half plane.  part[slot][2][nblk]: the r and Aϕ sums of the
// workgroup; contrib[slot][band][mode]: what the mode adds to the derivative of its bin's amplitude (0 where it lies in no bin)
template <typename T, bool BLOCK, bool MIXED>
__global__ __launch_bounds__(NTP) void k_theta_grad(ThetaDev m, ThetaPoint t, ThetaFields<T> fl, int want, double r0, double* __restrict__ part,
                                                    double* __restrict__ contrib) {
#pragma clang fp contract(off)
  using DF = ThDual<1 + TH_MAXBANDS>;        // tangents: 0 r, 1 + k band k
  using D1 = ThDual<1>;
  __shared__ double red[2][NTP / 64];
  double acc[2] = {0.0, 0.0};
  const long pl = m.pl;
  const int b = blockIdx.y, P = BLOCK ? 3 : m.np;
  const double sc = 1.0 / ((double)m.Ny * (double)m.Nx);
  const bool wr = want & TH_WANT_R, wa = want & TH_WANT_APHI, wb = want & TH_WANT_AMPS;
  DF sF = th_const<DF>(t.s);
  D1 s1 = th_const<D1>(t.s);
  if (wr) { sF.d[0] = 1.0 / r0; s1.d[0] = 1.0 / r0; }
  const double* base = m.c0 ? m.c0 : m.cfs;
  for (long j = (long)blockIdx.x * NTP + threadIdx.x; j < pl; j += (long)gridDim.x * NTP) {
    const int ky = (int)(j / m.Nx);
    const double lam = (ky == 0 || (m.Ny % 2 == 0 && ky == m.Nyh - 1)) ? 1.0 : 2.0;
    const double w = lam * sc;
    DF amp[TH_MAXBANDS];
#pragma unroll
    for (int k = 0; k < TH_MAXBANDS; ++k) {
      amp[k] = th_const<DF>(1.0);
      if (k < m.nbands && m.bmask[k]) {
        amp[k].v = th_amp(m, t, k, j);
        if (wb && m.bidx[k][j] < m.bnb[k]) amp[k].d[1 + k] = 1.0;
      }
    }
    double dband[TH_MAXBANDS] = {0.0, 0.0, 0.0};
    if (wr || wb) {
      if constexpr (BLOCK) {
        const cx<T> fI = fl.f[((long)b * 3 + 0) * pl + j], fE = fl.f[((long)b * 3 + 1) * pl + j], fB = fl.f[((long)b * 3 + 2) * pl + j];
        ThBlkT<DF> cb{th_const<DF>(base[j]), th_const<DF>(base[pl + j]), th_const<DF>(base[2 * pl + j]), th_const<DF>(base[3 * pl + j]), th_const<DF>(base[4 * pl + j])};
#pragma unroll
        for (int k = 0; k < TH_MAXBANDS; ++k) {                                   // bmask is 0 past the last band
          if (m.bmask[k] & 1) cb.a = amp[k] * cb.a;
          if (m.bmask[k] & 2) cb.b = amp[k] * cb.b;
          if (m.bmask[k] & 4) cb.c = amp[k] * cb.c;
          if (m.bmask[k] & 8) cb.d = amp[k] * cb.d;
        }
        const ThBlk tenb{m.cten[j], m.cten[pl + j], m.cten[2 * pl + j], m.cten[3 * pl + j], m.cten[4 * pl + j]};
        const ThBlkT<DF> cf = th_add(cb, th_scale(tenb, sF));
        const ThBlkT<DF> cfi = th_pinv(cf);
        const DF lt = th_logterm(th_det(cf), lam) + th_logterm(cf.e, lam);
        const DF q = cfi.a * th_re(fI, fI) + (cfi.b + cfi.c) * th_re(fI, fE) + cfi.d * th_re(fE, fE) + cfi.e * th_re(fB, fB);
        if (wr) acc[0] += -0.5 * (q.d[0] * w + lt.d[0]);
#pragma unroll
        for (int k = 0; k < TH_MAXBANDS; ++k) dband[k] = -0.5 * (q.d[1 + k] * w + lt.d[1 + k]);
        if (MIXED && wr) {
          const cx<T> gI = fl.ghat[((long)b * 3 + 0) * pl + j], gE = fl.ghat[((long)b * 3 + 1) * pl + j], gB = fl.ghat[((long)b * 3 + 2) * pl + j];
          const ThBlk cs{m.cfs[j], m.cfs[pl + j], m.cfs[2 * pl + j], m.cfs[3 * pl + j], m.cfs[4 * pl + j]};
          const ThBlk n2 = th_noise2(ThBlk{m.cn[j], m.cn[pl + j], m.cn[2 * pl + j], m.cn[3 * pl + j], m.cn[4 * pl + j]}, m.s2len);
          const ThBlkT<D1> D = th_mix(th_add(th_scale(tenb, s1), cs), n2);
          const ThBlkT<D1> qd = th_mm(ThBlk{m.d0inv[j], m.d0inv[pl + j], m.d0inv[2 * pl + j], m.d0inv[3 * pl + j], m.d0inv[4 * pl + j]}, D);
          const D1 ld = th_logterm(th_det(qd), lam) + th_logterm(qd.e, lam);
          // Re(conj ĝ · (∂D/∂r) f), the block applied as the operator is: (a I + b E, c I + d E, e B)
          const double cross = D.a.d[0] * th_re(gI, fI) + D.b.d[0] * th_re(gI, fE) + D.c.d[0] * th_re(gE, fI) + D.d.d[0] * th_re(gE, fE) + D.e.d[0] * th_re(gB, fB);
          acc[0] += -(cross * w) - ld.d[0];
        }
      } else {
        for (int p = 0; p < P; ++p) {
          const long o = p * pl + j;
          const cx<T> fp = fl.f[((long)b * P + p) * pl + j];
          DF cb = th_const<DF>(base[o]);
#pragma unroll
          for (int k = 0; k < TH_MAXBANDS; ++k) if (m.bmask[k] & (1 << p)) cb = amp[k] * cb;
          const DF cf = cb + m.cten[o] * sF;
          const DF lt = th_logterm(cf, lam);
          const DF q = th_pinv(cf) * th_re(fp, fp);
          if (wr) acc[0] += -0.5 * (q.d[0] * w + lt.d[0]);
#pragma unroll
          for (int k = 0; k < TH_MAXBANDS; ++k) dband[k] += -0.5 * (q.d[1 + k] * w + lt.d[1 + k]);
          if (MIXED && wr) {
            const D1 D = th_mix(m.cten[o] * s1 + m.cfs[o], m.cn[o], m.s2len);
            const D1 ld = th_logterm(m.d0inv[o] * D, lam);
            acc[0] += -((D.d[0] * th_re(fl.ghat[((long)b * P + p) * pl + j], fp)) * w) - ld.d[0];
          }
        }
      }
    }
    if (wb) {
#pragma unroll
      for (int k = 0; k < TH_MAXBANDS; ++k) if (k < m.nbands) contrib[((long)b * m.nbands + k) * pl + j] = dband[k];
    }
    if (wa) {
      D1 A = th_const<D1>(t.aphi);
      A.d[0] = 1.0;
      const D1 cphi = m.cphi0[j] * A / m.aphi0;
      const cx<T> ph = fl.phi[(long)b * pl + j];
      const D1 q = th_pinv(cphi) * th_re(ph, ph);
      const D1 lt = th_logterm(cphi, lam);
      acc[1] += -0.5 * (q.d[0] * w + lt.d[0]);
      if (MIXED && t.g_theta) {
        const D1 G = m.g0inv[j] * th_g(m.nphi[j], cphi);
        const D1 lg = th_logterm(G, lam);
        const double dlng = G.d[0] * th_pinv(G.v);
        acc[1] += -((dlng * th_re(fl.gphio[(long)b * pl + j], fl.phio[(long)b * pl + j])) * w) - lg.d[0];
      }
    }
  }
  // fixed-order sum of the workgroup: lanes by shuffle, wavefronts in index order
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double r = 0;
    for (int w = 0; w < NTP / 64; ++w) r += red[threadIdx.x][w];
    part[((size_t)b * 2 + threadIdx.x) * gridDim.x + blockIdx.x] = r;
  }
}

// The per-bin sums without atomics: each band's modes are listed once, sorted by bin (theta_install), and cut into chunks that never straddle
// a bin.  grid: (nchunks, nbatch); cpart[slot][chunk] = Σ contrib over the chunk's modes, in a fixed order
static __global__ __launch_bounds__(NTP) void k_theta_bins(const ThChunk* __restrict__ chunks, const int* __restrict__ list, const double* __restrict__ contrib,
                                                           int nbands, long pl, double* __restrict__ cpart) {
  __shared__ double red[NTP / 64];
  const ThChunk c = chunks[blockIdx.x];
  const double* src = contrib + ((size_t)blockIdx.y * nbands + c.band) * pl;
  double v = 0;
  for (int i = threadIdx.x; i < c.count; i += NTP) v += src[list[c.start + i]];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0;
    for (int w = 0; w < NTP / 64; ++w) r += red[w];
    cpart[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = r;
  }
}

// out[slot][2 + namps]: entries 0, 1 from part[slot][2][nblk], entry 2 + a from the chunk sums ampchunk[a] ... ampchunk[a + 1] - 1 of cpart.
// grid: (2 + namps, nbatch) workgroups of NTP threads, launched like k_theta_sum; the same order in every run
static __global__ __launch_bounds__(NTP) void k_theta_grad_sum(const double* __restrict__ part, int nblk, const double* __restrict__ cpart, int nchunks,
                                                               const int* __restrict__ ampchunk, int want, double* __restrict__ out) {
  __shared__ double red[NTP / 64];
  const int e = blockIdx.x, b = blockIdx.y, nout = gridDim.x;
  double v = 0;
  if (e < 2) {
    if (want & (e == 0 ? TH_WANT_R : TH_WANT_APHI))
      for (int i = threadIdx.x; i < nblk; i += NTP) v += part[((size_t)b * 2 + e) * nblk + i];
  } else if (want & TH_WANT_AMPS) {
    for (int i = ampchunk[e - 2] + threadIdx.x; i < ampchunk[e - 1]; i += NTP) v += cpart[(size_t)b * nchunks + i];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0;
    for (int w = 0; w < NTP / 64; ++w) r += red[w];
    out[(size_t)b * nout + e] = r;
  }
}

}  // namespace cmbl
