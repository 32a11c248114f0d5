"""NumPy / SciPy-sparse restatement of the reference's `BilinearLens` (src/bilinearlens.jl) and `gmres` (src/numerical_algorithms.jl:193-214), for
the tests of cmbl_bilinear_*.  Independent of the engine: nothing here imports the package.

Everything is written as the reference writes it -- the pixel index added to the deflection in the working precision (:44-45), the weights as
inv(A)[1, :] (:67-73), the sparse matrix with its duplicates summed (:85), gmres by the QR factorisation of the Krylov matrix -- in the precision
`T` asked for: float64 is the oracle of the GPU tests, float32 "the reference's own Float32 arithmetic" whose distance from the float64 result is
the error budget of the single-precision comparisons (tests/golden/bilinear_budget.json, made by tests/test_bilinear_ref.py).

Array layouts are the engine's host layouts: map (..., Nx, Ny) real == Julia (Ny, Nx, ...), so that the C-order ravel of a plane is Julia's
column-major `[:]` (I = i + Ny j); Fourier (..., Nx, Ny//2+1) complex, the unnormalised rfft over both axes (src/util_fft.jl:20-25)."""
import numpy as np
import scipy.fft as sfft
import scipy.sparse as sp

CASES = {"64x128": (64, 128, 0.7), "30x45": (30, 45, 0.7), "12x8": (12, 8, 6.0)}       # (Ny, Nx, rms deflection in pixels per component)
THETA = 2.0
P, B = 2, 2
QUANTITIES = ("L*f", "L'g", "L\\f", "L'\\g", "dphi")


def ctype(T):
    return np.complex64 if np.dtype(T) == np.float32 else np.complex128


def rfft2(m):                                            # m_rfft (src/util_fft.jl:20), in the precision of m
    return sfft.rfft2(m, axes=(-2, -1))


def irfft2(F, Ny):                                       # m_irfft (src/util_fft.jl:25)
    return sfft.irfft2(F, s=(F.shape[-2], Ny), axes=(-2, -1))


def kfreq(N):
    i = np.arange(N)
    return np.where(i < (N + 1) // 2, i, i - N)


class Geom:
    """Δx, ℓx, ℓy in T (src/proj_lambert.jl:58-64): ℓy on the half plane, its Nyquist entry negative"""

    def __init__(self, Ny, Nx, theta_pix, T):
        T = np.dtype(T).type
        self.Ny, self.Nx, self.T = Ny, Nx, T
        self.dx = T(np.deg2rad(theta_pix / 60))
        self.lx = kfreq(Nx).astype(T) * T(2 * np.pi / float(T(Nx) * self.dx))
        self.ly = (kfreq(Ny).astype(T) * T(2 * np.pi / float(T(Ny) * self.dx)))[:Ny // 2 + 1]

    def grad(self, F):
        """∇ * f on Fourier planes: (iℓx F, iℓy F)"""
        C = ctype(self.T)
        return (1j * self.lx[:, None]).astype(C) * F, (1j * self.ly[None, :]).astype(C) * F


def deflection(g, phi):
    """(dy, dx) in pixels, maps (Nx, Ny): `(∇*ϕ)./Δx` (:43); ϕ a map (Nx, Ny) in T"""
    gx, gy = g.grad(rfft2(phi.astype(g.T)))
    return (irfft2(gy, g.Ny) / g.dx).astype(g.T), (irfft2(gx, g.Ny) / g.dx).astype(g.T)


def sparse_repr(dy, dx, T):
    """:42-86 from the pixel-unit deflection maps (Nx, Ny): the npix x npix matrix, float T"""
    T = np.dtype(T).type
    Nx, Ny = dy.shape
    it = (dy.astype(T) + np.arange(1, Ny + 1, dtype=T)[None, :]).ravel()          # ĩs .= ĩs .+ (1:Ny), in T
    jt = (dx.astype(T) + np.arange(1, Nx + 1, dtype=T)[:, None]).ravel()
    left, top = np.floor(it).astype(np.int64), np.floor(jt).astype(np.int64)
    right, bottom = left + 1, top + 1
    wrap = lambda i, N: np.mod(i - 1, N)                                          # indexwrap, 0-based
    sub = lambda i, j: wrap(i, Ny) + Ny * wrap(j, Nx)
    M = np.stack([sub(left, top), sub(right, top), sub(left, bottom), sub(right, bottom)], axis=1)
    xm, xp = left.astype(T) - it, right.astype(T) - it
    ym, yp = top.astype(T) - jt, bottom.astype(T) - jt
    one = np.ones_like(xm)
    A = np.stack([np.stack([one, xm, ym, xm * ym], 1), np.stack([one, xp, ym, xp * ym], 1),
                  np.stack([one, xm, yp, xm * yp], 1), np.stack([one, xp, yp, xp * yp], 1)], axis=1)
    V = np.linalg.inv(A)[:, 0, :].astype(T)                                       # inv(A)[1, :]
    n = Nx * Ny
    K = np.repeat(np.arange(n), 4)
    return sp.csr_matrix((V.ravel(), (K, M.ravel())), shape=(n, n), dtype=T)


def gmres(A, b, Pl, maxiter=5):
    """src/numerical_algorithms.jl:193-214 as written; A, Pl sparse, b a vector"""
    n = maxiter
    K = np.empty((b.size, n + 1), dtype=b.dtype)
    K[:, 0] = Pl @ b
    for i in range(1, n + 1):
        K[:, i] = Pl @ (A @ K[:, i - 1])
    Q, R = np.linalg.qr(K[:, 1:])
    alpha = np.linalg.solve(R, Q.T @ K[:, 0])
    return K[:, :n] @ alpha


class BilinearLens:
    """BilinearLens(ϕ) on a grid, precision T; `phi` a map (Nx, Ny), or `defl=(dy, dx)` pixel-unit maps"""

    def __init__(self, Ny, Nx, theta_pix, T, phi=None, defl=None):
        self.g = Geom(Ny, Nx, theta_pix, T)
        self.T = self.g.T
        self.identity = phi is not None and not np.any(phi)                       # norm(ϕ) == 0 (:34)
        self._anti = None
        if self.identity:
            return
        self.defl = tuple(np.asarray(d, dtype=self.T) for d in defl) if defl is not None else deflection(self.g, np.asarray(phi))
        self.L = sparse_repr(self.defl[0], self.defl[1], self.T)

    @property
    def anti(self):                                                               # :92-97
        if self._anti is None:
            self._anti = sparse_repr(-self.defl[0], -self.defl[1], self.T)
        return self._anti

    def _each(self, f, fn):
        f = np.asarray(f, dtype=self.T)
        if self.identity:
            return f.copy()
        out = np.empty_like(f)
        flat_in, flat_out = f.reshape(-1, f.shape[-2] * f.shape[-1]), out.reshape(-1, f.shape[-2] * f.shape[-1])
        for s in range(flat_in.shape[0]):
            flat_out[s] = fn(flat_in[s])
        return out

    def mul(self, f):                                                             # L * f (:107-115)
        return self._each(f, lambda v: self.L @ v)

    def adj(self, g):                                                             # L' * g (:117-125)
        return self._each(g, lambda v: self.L.T @ v)

    def ldiv(self, f, maxiter=5):                                                 # L \ f (:127-138)
        return self._each(f, lambda v: gmres(self.L, v, self.anti, maxiter))

    def adj_ldiv(self, g, maxiter=5):                                             # L' \ g (:140-151)
        return self._each(g, lambda v: gmres(self.L.T.tocsr(), v, self.anti.T.tocsr(), maxiter))

    def pullback(self, f_lensed, delta):
        """:165-171  maps (B, P, Nx, Ny) -> (δϕ Fourier (B, 1, Nx, Nyh), δf = L'Δ maps)"""
        g = self.g
        gx, gy = g.grad(rfft2(np.asarray(f_lensed, dtype=self.T)))
        delta = np.asarray(delta, dtype=self.T)
        v1 = np.sum(delta * irfft2(gx, g.Ny).astype(self.T), axis=1, keepdims=True)
        v2 = np.sum(delta * irfft2(gy, g.Ny).astype(self.T), axis=1, keepdims=True)
        a, _ = g.grad(rfft2(v1))
        _, b = g.grad(rfft2(v2))
        return -(a + b), self.adj(delta)                                          # ∇' = -∇ on the Fourier planes


def make_phi(Ny, Nx, theta_pix, rms_px, seed):
    """a seeded red-spectrum ϕ map (Nx, Ny), float64, scaled so that each component of ∇ϕ/Δx has the stated rms in pixels"""
    rng = np.random.default_rng(seed)
    F = rfft2(rng.standard_normal((Nx, Ny)))
    k = np.hypot(kfreq(Nx)[:, None] / Nx, kfreq(Ny)[None, :Ny // 2 + 1] / Ny)
    F = F * np.where(k > 0, 1.0 / np.maximum(k, 1e-30) ** 3, 0.0)
    phi = irfft2(F, Ny)
    dy, dx = deflection(Geom(Ny, Nx, theta_pix, np.float64), phi)
    return phi * (rms_px / np.sqrt(0.5 * (np.mean(dy ** 2) + np.mean(dx ** 2))))


_inputs = {}


def inputs(case, T):
    """(ϕ (Nx, Ny), f, g (B, P, Nx, Ny)) of a case, rounded to T and returned in T: made once, never modified"""
    key = (case, np.dtype(T).name)
    if key not in _inputs:
        Ny, Nx, rms = CASES[case]
        rng = np.random.default_rng(Ny * 10007 + Nx)
        phi = make_phi(Ny, Nx, THETA, rms, Ny + Nx)
        _inputs[key] = tuple(a.astype(T) for a in (phi, rng.standard_normal((B, P, Nx, Ny)), rng.standard_normal((B, P, Nx, Ny))))
    return _inputs[key]


_results = {}


def results(case, T_in, T):
    """the five quantities of a case computed in precision T from the inputs rounded to T_in; L\\f̃ is taken of f̃ = L*f rounded to T_in"""
    key = (case, np.dtype(T_in).name, np.dtype(T).name)
    if key not in _results:
        Ny, Nx, _ = CASES[case]
        phi, f, g = (a.astype(T) for a in inputs(case, T_in))
        ft_in = lensed_input(case, T_in).astype(T)
        L = BilinearLens(Ny, Nx, THETA, T, phi=phi)
        dphi, _ = L.pullback(ft_in, g)
        _results[key] = {"L*f": L.mul(f), "L'g": L.adj(g), "L\\f": L.ldiv(ft_in), "L'\\g": L.adj_ldiv(g), "dphi": dphi}
    return _results[key]


def lensed_input(case, T_in):
    """f̃ = L*f in float64, rounded to T_in: the argument of L\\f̃ and the primal output of the pullback in every comparison"""
    Ny, Nx, _ = CASES[case]
    phi, f, _ = (a.astype(np.float64) for a in inputs(case, T_in))
    return BilinearLens(Ny, Nx, THETA, np.float64, phi=phi).mul(f).astype(T_in)


def rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))
