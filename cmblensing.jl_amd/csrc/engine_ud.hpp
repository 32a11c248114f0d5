// Host side of cmbl_ud_grade (src/proj_lambert.jl:533-592): the one operation that spans TWO contexts, `s` (the field's grid) and `d` (the new
// grid).  Both share precision, device and stream (checked by the entry point); every launch below goes to that stream.  Transforms, operand
// staging and scratch are the contexts' own (rfft2_F / F_to_map / ref2F / F2ref, tmpA = a half plane in F layout, tmpB = a map); the kernels
// are those of kernels_udgrade.hpp.  Each step acts on every (pol, batch) plane alike, so pol components are never mixed and HARMONIC planes
// pass through like FOURIER planes.
#pragma once
#include "engine.hpp"
#include "kernels_udgrade.hpp"

namespace cmbl {

enum UdMode { UD_MAP = 0, UD_FOURIER = 1 };
struct UdGeom { int dir, fac; };           // dir: -1 downgrade (s finer than d), 0 equal geometry, +1 upgrade; sides and pixel size differ by `fac`

// "Can only ud_grade in integer steps" (:545-548): an integer fac >= 2 on both axes and in the pixel size (relative 1e-6), or equal geometry
inline UdGeom ud_geometry(const CtxBase& s, const CtxBase& d) {
  auto same = [](double a, double b) { return std::fabs(a - b) <= 1e-6 * std::fabs(b); };
  auto steps = [&](const CtxBase& fine, const CtxBase& coarse) {
    if (fine.Ny % coarse.Ny != 0) return 0;
    const int fac = fine.Ny / coarse.Ny;
    return fac >= 2 && (long)fac * coarse.Nx == fine.Nx && same(fac * fine.theta, coarse.theta) ? fac : 0;
  };
  if (s.Ny == d.Ny && s.Nx == d.Nx && same(s.theta, d.theta)) return {0, 1};
  if (const int f = steps(s, d)) return {-1, f};
  if (const int f = steps(d, s)) return {+1, f};
  fail(ERR_SHAPE, "ud_grade: the two grids must differ by one integer factor >= 2 in Ny, Nx and theta_pix (integer steps only)");
}

// The block mean as a Fourier-space multiply.  After anti-aliasing no two surviving frequencies of the fine grid alias onto one of the coarse
// grid, so the rfft of the block mean is  F_new[k] = F[k] D_y(ky) D_x(kx) / fac^4,  D(k) = sum_{a < fac} exp(2 pi i k a / N),  N the fine side.
// Per axis a table of D / fac^2 over the coarse grid's frequency indices, built once per pair of grids in double: wy[Ny_d / 2 + 1], wx[Nx_d].
template <typename T> const cx<double>* ud_weights(Ctx<T>* s, Ctx<T>* d, int fac) {
  std::unique_ptr<DevBuf>& b = d->ud_w[((long)s->Ny << 16) | s->Nx];
  if (!b) {
    std::vector<cx<double>> w((size_t)d->Nyh + d->Nx);
    auto fill = [&](cx<double>* t, int n, int Nd, int N) {
      for (int i = 0; i < n; ++i) {
        const long k = i < (Nd + 1) / 2 ? i : i - Nd;
        double re = 0, im = 0;
        for (int a = 0; a < fac; ++a) {                                     // the phase reduced exactly
          const double ph = 2.0 * M_PI * (double)(((k * a) % N + N) % N) / (double)N;
          re += std::cos(ph); im += std::sin(ph);
        }
        t[i] = mk<double>(re / ((double)fac * fac), im / ((double)fac * fac));
      }
    };
    fill(w.data(), d->Nyh, d->Ny, s->Ny);
    fill(w.data() + d->Nyh, d->Nx, d->Nx, s->Nx);
    auto nb = std::make_unique<DevBuf>();
    d->upload(*nb, w);
    b = std::move(nb);
  }
  return b->template as<cx<double>>();
}

template <typename T> void ud_mean(Ctx<T>* d, const T* in, T* out, int fac, long slices) {
  const dim3 grid((unsigned)((d->npix() + NTP - 1) / NTP), (unsigned)slices);
  // every run of `fac` reals starts a multiple of `fac` reals behind `in`: the vector loads are aligned when `in` is
  const bool aligned = reinterpret_cast<uintptr_t>(in) % std::min<size_t>(fac * sizeof(T), 16) == 0;
  if (fac == 2 && aligned) CMBL_LAUNCH(d, K_UD, (k_ud_mean<T, 2>), grid, 0, d->stream, in, out, d->Ny, d->Nx, fac);
  else if (fac == 4 && aligned) CMBL_LAUNCH(d, K_UD, (k_ud_mean<T, 4>), grid, 0, d->stream, in, out, d->Ny, d->Nx, fac);
  else if (fac == 3) CMBL_LAUNCH(d, K_UD, (k_ud_mean<T, 3>), grid, 0, d->stream, in, out, d->Ny, d->Nx, fac);
  else CMBL_LAUNCH(d, K_UD, (k_ud_mean<T, 0>), grid, 0, d->stream, in, out, d->Ny, d->Nx, fac);
}
template <typename T> void ud_repl(Ctx<T>* d, const T* in, T* out, int fac, long slices) {
  CMBL_LAUNCH(d, K_UD, (k_ud_repl<T>), dim3((unsigned)((d->npix() + NTP - 1) / NTP), (unsigned)slices), 0, d->stream, in, out, d->Ny, d->Nx, fac);
}
// F layout of `s` -> F layout of `d` (s == d: in place, the 1 / PWF of the grid with sides pwNy x pwNx alone)
template <typename T>
void ud_fourier(Ctx<T>* s, Ctx<T>* d, const cx<T>* in, cx<T>* out, const cx<double>* w, bool zero, bool deconv, int pwNy, int pwNx, long slices) {
  UdFourier<T> a{};
  a.in = in; a.out = out; a.wy = w; a.wx = w ? w + d->Nyh : nullptr;
  a.Nys = s->Ny; a.Nxs = s->Nx; a.lgNxs = s->generic ? -1 : s->lgNx;
  a.Nyd = d->Ny; a.Nxd = d->Nx; a.lgNxd = d->generic ? -1 : d->lgNx;
  a.pwNy = pwNy; a.pwNx = pwNx; a.zero = zero; a.deconv = deconv; a.slices = (int)slices;
  CMBL_LAUNCH(d, K_UD, (k_ud_fourier<T>), dim3((unsigned)((d->plane() + NTP - 1) / NTP)), 0, d->stream, a);
}

template <typename T>
void ud_grade(Ctx<T>* s, Ctx<T>* d, int mode, bool deconv, bool aa, int bi, const void* in, int bo, void* out, int P, int B) {
  const UdGeom g = ud_geometry(*s, *d);
  const long sl = (long)P * B;
  const int fac = g.fac;
  auto F_of = [&](Ctx<T>* c) { c->tmpA.ensure(sizeof(cx<T>) * sl * c->plane()); return c->tmpA.template as<cx<T>>(); };
  auto map_of = [&](Ctx<T>* c) { c->tmpB.ensure(sizeof(T) * sl * c->npix()); return c->tmpB.template as<T>(); };
  // the field as a half plane in the F layout of its grid / as a map (a complex input is taken as the transform of real maps)
  auto src_F = [&]() { cx<T>* F = F_of(s); if (bi == B_MAP) s->rfft2_F((const T*)in, F, sl); else s->ref2F((const cx<T>*)in, F, sl); return F; };
  auto src_map = [&]() -> const T* {
    if (bi == B_MAP) return (const T*)in;
    cx<T>* F = F_of(s); T* m = map_of(s);
    s->ref2F((const cx<T>*)in, F, sl); s->F_to_map(F, m, sl);
    return m;
  };
  auto emit_F = [&](cx<T>* F) { if (bo == B_MAP) d->F_to_map(F, (T*)out, sl); else d->F2ref(F, (cx<T>*)out, sl); };

  if (g.dir == 0) {                                                         // θnew == θ && return f (:542): a copy, or the basis conversion asked for
    if (bi == bo) { CMBL_HIP(hipMemcpyAsync(out, in, (bi == B_MAP ? sizeof(T) * s->npix() : sizeof(cx<T>) * s->plane()) * sl, hipMemcpyDeviceToDevice, s->stream)); return; }
    cx<T>* F = src_F();
    if (bo == B_MAP) s->F_to_map(F, (T*)out, sl); else s->F2ref(F, (cx<T>*)out, sl);
    return;
  }
  if (g.dir > 0) {                                                          // upgrade (:575-589)
    CMBL_REQUIRE(mode == UD_MAP, ERR_ARG, "ud_grade: upgrading in Fourier mode is not implemented (src/proj_lambert.jl:585)");
    CMBL_REQUIRE(!deconv, ERR_ARG, "ud_grade: upgrading with deconv_pixwin is not implemented (src/proj_lambert.jl:582)");
    const T* m = src_map();
    if (bo == B_MAP) return ud_repl(d, m, (T*)out, fac, sl);
    T* md = map_of(d); cx<T>* F = F_of(d);
    ud_repl(d, m, md, fac, sl);
    d->rfft2_F(md, F, sl);
    return d->F2ref(F, (cx<T>*)out, sl);
  }
  // downgrade (:555-572)
  if (mode == UD_FOURIER || aa) {
    // Fourier mode: the coarse grid's frequencies of the (anti-aliased) half plane, not rescaled (:566).  Map mode with anti-aliasing: the same
    // gather carries the block mean as the weight of ud_weights -- one transform at the fine size instead of the reference's two.
    cx<T>* Fs = src_F(); cx<T>* Fd = F_of(d);
    ud_fourier(s, d, Fs, Fd, mode == UD_MAP ? ud_weights(s, d, fac) : nullptr, aa, deconv, s->Ny, s->Nx, sl);
    return emit_F(Fd);
  }
  // map mode without anti-aliasing, where aliasing is part of the answer: the literal sequence (:561, 571)
  const T* m = src_map();
  if (!deconv && bo == B_MAP) return ud_mean(d, m, (T*)out, fac, sl);
  T* md = map_of(d); cx<T>* Fd = F_of(d);
  ud_mean(d, m, md, fac, sl);
  d->rfft2_F(md, Fd, sl);
  if (deconv) ud_fourier(d, d, Fd, Fd, (const cx<double>*)nullptr, false, true, s->Ny, s->Nx, sl);
  emit_F(Fd);
}

// pixwin(θpix, ℓ) (src/proj_lambert.jl:200) on the half plane of the context, reference layout [x][ky]: the ℓ of the grid are k * 2π / (N Δx), so
// the window is sinc(ky / Ny) * sinc(kx / Nx) whatever the pixel size
inline void pixwin_plane(const CtxBase& c, double* out) {
  auto sinc = [](double t) { return t == 0 ? 1.0 : std::sin(M_PI * t) / (M_PI * t); };
  for (int x = 0; x < c.Nx; ++x) {
    const int kx = x < (c.Nx + 1) / 2 ? x : x - c.Nx;
    for (int ky = 0; ky < c.Nyh; ++ky) out[(size_t)x * c.Nyh + ky] = sinc((double)ky / c.Ny) * sinc((double)kx / c.Nx);
  }
}

}  // namespace cmbl
