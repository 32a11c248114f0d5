"""NumPy restatement of the reference's `PowerLens` (src/powerlens.jl) and `Taylens` (src/taylens.jl), for the tests of cmbl_powerlens_*.
Independent of the engine: nothing here imports the package.  Neither operator is covered by the reference's test/runtests.jl, so this file
restates the formulas of the source, and tests/test_powerlens_ref.py pins it by answers that use neither.

    PowerLens(order) * f  (:40-48):  f̃ = Ł(f) + Σ_{n=1..order} Σ_{(a,b)=zip(0:n,n:-1:0)} ∇1ϕ^a ∇2ϕ^b Ł(∇[1]^a ∇[2]^b Ð(f)) / a! / b!
    PowerLens(order)' * g (:50-58):  r = Ð(g) + Σ_n (-1)^n Σ_{(a,b)} ∇[1]^a ∇[2]^b Ð(∇1ϕ^a ∇2ϕ^b Ł(g)) / a! / b!       (a Fourier field)
    Taylens(order) * f (src/taylens.jl:25-66):  di = round(dy/Δx), dj = round(dx/Δx) (half to even), the residual r = d - (dj, di) Δx, and the
        PowerLens sum of r with f and every derivative map read at pixel (wrap(y + di), wrap(x + dj))

with ∇[1] = iℓx, ∇[2] = iℓy, ∇1ϕ = dx, ∇2ϕ = dy the deflection in radians, in the precision `T` asked for: float64 is the oracle of the GPU tests,
float32 the reference's own single-precision arithmetic, whose distance from float64 is the budget of the single-precision comparisons
(tests/golden/powerlens_budget.json).  As written, ℓ^n leaves the range of float32 from n = 10 on at 2' pixels (ℓmax^10 = 6.7e38); `pixel_units=True`
forms the same terms from ℓΔx and d/Δx, which is how the engine forms them and the only way the float32 sum of those orders is finite.

Layouts, cases and inputs are those of tests/_bilinear_ref.py: map (..., Nx, Ny) with Ny fastest, Fourier (..., Nx, Ny//2+1)."""
from math import factorial

import numpy as np

import _bilinear_ref as _B
from _bilinear_ref import CASES, THETA, P, B, Geom, ctype, rfft2, irfft2, make_phi, rel      # noqa: F401

# further shapes of the GPU tests (Ny, Nx, rms deflection in pixels), with inputs made by the recipe of tests/_bilinear_ref.py; they have no entry
# in the budget file: the GPU tests measure the float32 error of this restatement for them
GPU_CASES = {"64x64": (64, 64, 0.7), "128x64": (128, 64, 0.7), "96x160": (96, 160, 0.7)}
ALL_CASES = {**CASES, **GPU_CASES}
_inputs = {}


def inputs(case, T):
    """(ϕ (Nx, Ny), f, g (B, P, Nx, Ny)) of a case, rounded to T: made once, never modified"""
    if case in CASES:
        return _B.inputs(case, T)
    key = (case, np.dtype(T).name)
    if key not in _inputs:
        Ny, Nx, rms = GPU_CASES[case]
        rng = np.random.default_rng(Ny * 10007 + Nx)
        phi = make_phi(Ny, Nx, THETA, rms, Ny + Nx)
        _inputs[key] = tuple(a.astype(T) for a in (phi, rng.standard_normal((B, P, Nx, Ny)), rng.standard_normal((B, P, Nx, Ny))))
    return _inputs[key]


def const_defl(Ny, Nx, uy, ux, T=np.float64):
    """constant deflection maps (dy, dx) in radians whose quotient by Δx IN T is exactly (uy, ux) pixels"""
    dx = Geom(Ny, Nx, THETA, T).dx
    T = np.dtype(T).type

    def exact(u):
        d = T(u) * dx
        for c in (d, np.nextafter(d, T(np.inf)), np.nextafter(d, T(-np.inf))):
            if c / dx == T(u):
                return c
        raise AssertionError(u)
    return np.full((Nx, Ny), exact(uy), dtype=T), np.full((Nx, Ny), exact(ux), dtype=T)

QUANTITIES = ("PowerLens*f", "PowerLens'g", "Taylens*f")
BUDGET_ORDERS = (2, 4)


def grad_phi(g, phi):
    """(dy, dx) in radians, maps (Nx, Ny): Ł(∇*ϕ) (:23, 26)"""
    gx, gy = g.grad(rfft2(np.asarray(phi, dtype=g.T)))
    return irfft2(gy, g.Ny).astype(g.T), irfft2(gx, g.Ny).astype(g.T)


def ipow(n, C):
    """i^n, exactly"""
    return np.array((1, 1j, -1, -1j)[n % 4], dtype=C)


class PowerLens:
    """PowerLens(ϕ, order) or PowerLens(d, order) on a grid in precision T; `phi` a map (Nx, Ny), or `defl=(dy, dx)` maps in radians"""

    def __init__(self, Ny, Nx, theta_pix, T, order, phi=None, defl=None, pixel_units=False):
        self.g = g = Geom(Ny, Nx, theta_pix, T)
        self.T, self.C, self.order = g.T, ctype(g.T), int(order)
        dy, dx = (np.asarray(d, dtype=g.T) for d in defl) if defl is not None else grad_phi(g, phi)
        self.lx, self.ly = g.lx, g.ly
        if pixel_units:
            dy, dx, self.lx, self.ly = dy / g.dx, dx / g.dx, g.lx * g.dx, g.ly * g.dx
        self.d1, self.d2 = self.residual(dx, dy, g.T(1) if pixel_units else g.dx)

    def residual(self, dx, dy, pix):
        return dx, dy

    def remap(self, m):
        return m

    def deriv(self, F, a, b):
        """∇[1]^a ∇[2]^b on Fourier planes: i^(a+b) ℓx^a ℓy^b F, the powers in T"""
        return (ipow(a + b, self.C) * (self.lx[:, None] ** a * self.ly[None, :] ** b).astype(self.T)).astype(self.C) * F

    def mul(self, f):
        f = np.asarray(f, dtype=self.T)
        F = rfft2(f)
        out = self.remap(f.copy())
        for n in range(1, self.order + 1):
            for a, b in zip(range(0, n + 1), range(n, -1, -1)):
                D = self.remap(irfft2(self.deriv(F, a, b), self.g.Ny).astype(self.T))
                out = out + self.d1 ** a * self.d2 ** b * D / self.T(factorial(a)) / self.T(factorial(b))
        return out.astype(self.T)

    def adj(self, g):
        g = np.asarray(g, dtype=self.T)
        r = rfft2(g).astype(self.C)
        for n in range(1, self.order + 1):
            for a, b in zip(range(0, n + 1), range(n, -1, -1)):
                r = r + self.T((-1) ** n) * self.deriv(rfft2((self.d1 ** a * self.d2 ** b * g).astype(self.T)), a, b) / self.T(factorial(a)) / self.T(factorial(b))
        return r.astype(self.C)


class Taylens(PowerLens):
    """Taylens(ϕ, order) / Taylens(d, order); the reference defines `*` alone"""

    def residual(self, dx, dy, pix):
        Ny, Nx = self.g.Ny, self.g.Nx
        di, dj = np.rint(dy / pix), np.rint(dx / pix)                                # round.(Int, dy/Δx): half to even (src/taylens.jl:35-36)
        self.i = np.mod(di.astype(np.int64) + np.arange(Ny)[None, :], Ny)             # indexwrap.(di .+ (1:Ny), Ny), 0-based
        self.j = np.mod(dj.astype(np.int64) + np.arange(Nx)[:, None], Nx)
        return (dx - dj.astype(self.T) * pix).astype(self.T), (dy - di.astype(self.T) * pix).astype(self.T)      # :41-44

    def remap(self, m):
        return m[..., self.j, self.i]                                                 # getindex.(Ref(arr), i, j) (:54)

    def adj(self, g):
        raise NotImplementedError("src/taylens.jl defines no adjoint")


KINDS = {"PowerLens": PowerLens, "Taylens": Taylens}


def action(q, L, f, g):
    return L.adj(g) if q == "PowerLens'g" else L.mul(f)


_results = {}


def result(case, q, order, T_in, T, sign=1.0, pixel_units=False):
    """quantity q of a case at one order, computed in precision T from the case's inputs rounded to T_in, with ϕ scaled by `sign`"""
    key = (case, q, order, np.dtype(T_in).name, np.dtype(T).name, sign, pixel_units)
    if key not in _results:
        Ny, Nx, _ = ALL_CASES[case]
        phi, f, g = (a.astype(T) for a in inputs(case, T_in))
        L = KINDS[q.split("*")[0].split("'")[0]](Ny, Nx, THETA, T, order, phi=T(sign) * phi, pixel_units=pixel_units)
        _results[key] = action(q, L, f, g)
    return _results[key]


def f32_error(case, q, order, sign=1.0):
    """the relative L2 error of the restatement in float32 against float64 on inputs rounded to float32.  As written up to order 9; from order
    10 on ℓmax^n > FLT_MAX, the float32 sum as written is not finite, and the same terms are formed in pixel units"""
    r32 = result(case, q, order, np.float32, np.float32, sign, pixel_units=order >= 10)
    r64 = result(case, q, order, np.float32, np.float64, sign)
    return rel(r32.astype(r64.dtype), r64)
