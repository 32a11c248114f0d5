"""Two independent restatements of `Cℓ_to_Cov` on ProjEquiRect, written from the DEFINITION of the blocks (the covariance of the AzFourier /
QUAzFourier coefficients of an isotropic Gaussian field), not from the kernels and not from CirculantCov.jl (which is not available).

(a) `cov_I` / `cov_P`: real space.  The correlation functions Σ (2ℓ+1)/(4π) Cℓ · {Pℓ, d^ℓ_{22}, d^ℓ_{2,-2}}(β) by upward three-term recurrences,
    vectorised over the points of all ring pairs; β through the haversine form; the bearing phases of spin 2; the K-fold periodisation;
    `np.fft`; the block layout.  `dt` is np.float64 or np.longdouble (the yardstick of the float64 budget).
(b) `harmonic_I` / `harmonic_P`: harmonic space, for conventions only (ℓmax ≤ 16).  Yℓm and ₂Yℓm from Wigner-d by its defining sum, the dense
    map-space covariances E[P Pᴴ], E[P Pᵀ] of the field model P = Q + iU = -Σ (Eℓm + i Bℓm) ₂Yℓm on the patch, pushed through
    `_equirect_ref.az_fwd` / `qu_fwd` as matrices.  On a patch that spans 2π/K the model keeps the orders m ≡ 0 (mod K) with K times their
    power: the field that has the period of the patch and, on the full ring, the modes K·m of the isotropic one -- which is what the
    periodised sequences of (a) describe.  (b) fixes every sign: where (a) and (b) disagree, (a) is wrong.

Blocks are returned as the device holds them: (Nx//2+1, n, n) indexed [m, q, p] == the reference's blocks[p, q, m] = E[v_p conj(v_q)]."""
import math

import numpy as np

from _equirect_ref import geometry, az_fwd, qu_fwd

TWO_PI = 2.0 * np.pi


def span_K(phi_span):
    """(K, ok): the azimuthal span is 2π/K"""
    f0, f1 = sorted(float(v) for v in phi_span)
    K = TWO_PI / (f1 - f0)
    return int(round(K)), abs(K - round(K)) <= 1e-9 * K and round(K) >= 1


def _pi(dt):
    return dt(4) * np.arctan(dt(1))


def weights(cl, dt=np.float64):
    """(2ℓ+1)/(4π) Cℓ, NaN -> 0"""
    cl = np.nan_to_num(np.asarray(cl, dtype=np.float64), nan=0.0).astype(dt)
    l = np.arange(cl.size).astype(dt)
    return (2 * l + 1) / (4 * _pi(dt)) * cl


# ---- the three sums over ℓ ----------------------------------------------------------------------------------------------------------------
def sum_legendre(x, w):
    """Σ_ℓ w[ℓ] Pℓ(x): (ℓ+1) P_{ℓ+1} = (2ℓ+1) x Pℓ - ℓ P_{ℓ-1}"""
    dt = x.dtype.type
    pm, p = np.ones_like(x), x.copy()
    acc = w[0] * pm
    if w.size > 1:
        acc = acc + w[1] * p
    for l in range(1, w.size - 1):
        pm, p = p, (dt(2 * l + 1) * x * p - dt(l) * pm) / dt(l + 1)
        acc += w[l + 1] * p
    return acc


def sum_d2(x, w, sign):
    """Σ_{ℓ≥2} w[ℓ] d^ℓ_{2,±2}(β), x = cos β, sign = +1: d_{22}, -1: d_{2,-2}.
    ℓ ((ℓ+1)² - 4) d^{ℓ+1} = (2ℓ+1) (ℓ(ℓ+1) x ∓ 4) d^ℓ - (ℓ+1)(ℓ² - 4) d^{ℓ-1}, from d² = ((1 ± x)/2)²"""
    dt = x.dtype.type
    dm, d = np.zeros_like(x), ((1 + sign * x) / 2) ** 2
    acc = w[2] * d
    for l in range(2, w.size - 1):
        den = dt(l) * dt((l + 1) ** 2 - 4)
        dm, d = d, (dt(2 * l + 1) * (dt(l * (l + 1)) * x - dt(4 * sign)) * d - dt((l + 1) * (l * l - 4)) * dm) / den
        acc += w[l + 1] * d
    return acc


# ---- (a) real space -----------------------------------------------------------------------------------------------------------------------
def _pairs(Ny):
    j, k = np.triu_indices(Ny)
    return j, k


def _separations(theta, K, Nx, j, k, dt):
    """per pair and d < K Nx: (sin²(β/2), A1, B1, A2, B2) with sin β (cos ψ, sin ψ) = (A, B): ψ1 the bearing at ring j's point (azimuth 0) of
    ring k's point (azimuth d Δφ), from e_θ towards e_φ; ψ2 the bearing of the first point at the second"""
    th = np.asarray(theta, dtype=np.float64).astype(dt)
    dphi = 2 * _pi(dt) / dt(K * Nx)
    D = (np.arange(K * Nx).astype(dt) * dphi)[None, :]
    t1, t2 = th[j][:, None], th[k][:, None]
    s1, c1, s2, c2 = np.sin(t1), np.cos(t1), np.sin(t2), np.cos(t2)
    sh = np.sin(D / 2) ** 2
    h = np.sin((t1 - t2) / 2) ** 2 + s1 * s2 * sh
    sD = np.sin(D)
    A1 = np.sin(t2 - t1) - 2 * c1 * s2 * sh
    B1 = s2 * sD
    A2 = np.sin(t1 - t2) - 2 * c2 * s1 * sh
    B2 = -s1 * sD
    return h, A1, B1, A2, B2


def _unit2(re, im):
    """(re + i im)² / |re + i im|², 1 where the number vanishes (coincident or antipodal points: the limit)"""
    n = re * re + im * im
    ok = n > 1e-24
    n = np.where(ok, n, 1)
    return np.where(ok, (re * re - im * im) / n, 1) + 1j * np.where(ok, 2 * re * im / n, 0)


def _periodise(c, K, Nx):
    return c.reshape(c.shape[0], K, Nx).sum(axis=1)


def _cdt(dt):
    return np.clongdouble if dt is np.longdouble else np.complex128


def _fft_rows(c, dt):
    """Σ_n c[:, n] e^{-2πi m n / Nx}, all m"""
    if dt is np.longdouble:                                                  # np.fft computes in double: a plain DFT matrix instead
        Nx = c.shape[1]
        mn = (np.arange(Nx)[:, None] * np.arange(Nx)[None, :]) % Nx
        ang = -2 * _pi(dt) * mn.astype(dt) / dt(Nx)
        return c.astype(np.clongdouble) @ (np.cos(ang) + 1j * np.sin(ang))
    return np.fft.fft(c, axis=1)


def correlation(h, cl_a, cl_b=None, dt=np.float64, table=None):
    """the sums at sin²(β/2) = h: w(β) (cl_b None) or (F+, F-); `table` = (ngrid, tables...) switches to the 4-point Lagrange lookup"""
    if table is not None:
        beta = 2 * np.arcsin(np.sqrt(np.minimum(h, 1)))
        return tuple(lagrange4(t, beta) for t in table[1:]) if cl_b is not None else lagrange4(table[1], beta)
    x = 1 - 2 * h
    if cl_b is None:
        return sum_legendre(x, weights(cl_a, dt))
    wa, wb = weights(cl_a, dt), weights(cl_b, dt)
    return sum_d2(x, wa + wb, +1), sum_d2(x, wa - wb, -1)


def make_table(ngrid, cl_a, cl_b=None, dt=np.float64):
    """the sums on the uniform grid β_i = i π / (ngrid - 1)"""
    beta = np.arange(ngrid).astype(dt) * (_pi(dt) / dt(ngrid - 1))
    h = np.sin(beta / 2) ** 2
    r = correlation(h, cl_a, cl_b, dt)
    return (ngrid,) + (tuple(r) if cl_b is not None else (r,))


def lagrange4(t, beta):
    """cubic Lagrange through the 4 nodes around β (the stencil is shifted inwards at the two ends)"""
    n = t.size
    u = beta * ((n - 1) / np.pi)
    i0 = np.clip(np.floor(u).astype(np.int64) - 1, 0, n - 4)
    s = u - i0
    w0 = -(s - 1) * (s - 2) * (s - 3) / 6
    w1 = s * (s - 2) * (s - 3) / 2
    w2 = -s * (s - 1) * (s - 3) / 2
    w3 = s * (s - 1) * (s - 2) / 6
    return w0 * t[i0] + w1 * t[i0 + 1] + w2 * t[i0 + 2] + w3 * t[i0 + 3]


def cov_I(theta, phi_span, Nx, cl, dt=np.float64, table=None):
    """blocks[j, k, m] = Re Σ_{d < K Nx} w(β_jk(d)) e^{-2πi m d / Nx}, m ≤ Nx÷2, as [m, q, p]"""
    K, ok = span_K(phi_span)
    assert ok
    Ny = len(theta)
    j, k = _pairs(Ny)
    h = _separations(theta, K, Nx, j, k, dt)[0]
    c = _periodise(correlation(h, cl, None, dt, table), K, Nx)
    F = _fft_rows(c, dt)[:, :Nx // 2 + 1].real
    out = np.zeros((Nx // 2 + 1, Ny, Ny), dtype=dt)
    out[:, k, j] = F.T
    out[:, j, k] = F.T
    return out


def cov_P(theta, phi_span, Nx, cl_ee, cl_bb, dt=np.float64, table=None):
    """the 2Ny x 2Ny complex blocks E[v vᴴ], v = (P̂[:, m]; conj P̂[:, (Nx-m) mod Nx]), as [m, q, p]"""
    K, ok = span_K(phi_span)
    assert ok and Nx % 2 == 0
    Ny = len(theta)
    j, k = (a.ravel() for a in np.meshgrid(np.arange(Ny), np.arange(Ny), indexing="ij"))
    h, A1, B1, A2, B2 = _separations(theta, K, Nx, j, k, dt)
    Fp, Fm = correlation(h, cl_ee, cl_bb, dt, table)
    # P = e^{2iψ} P' with P' in the frame of the great circle: E[P1 conj P2] = F+ e^{2i(ψ1 - ψ2)}, E[P1 P2] = F- e^{2i(ψ1 + ψ2)}
    # (the sign of ψ is the one harmonic_P confirms; the other fails test_equirect_cov_ref.py)
    g = Fp * _unit2(A1 * A2 + B1 * B2, B1 * A2 - A1 * B2)
    x = Fm * _unit2(A1 * A2 - B1 * B2, B1 * A2 + A1 * B2)
    # E[P̂_m(j) conj P̂_m(k)] = Σ_d E[P(j, 0) conj P(k, d)] e^{+2πi m d / Nx}: the forward transform read at (Nx - m) mod Nx
    G, X = _fft_rows(_periodise(g, K, Nx), dt), _fft_rows(_periodise(x, K, Nx), dt)
    Mh = Nx // 2 + 1
    m = np.arange(Mh)
    J = (Nx - m) % Nx
    gam = lambda mm: G[:, (Nx - mm) % Nx].reshape(Ny, Ny, Mh)              # [j, k, m]
    xi = lambda mm: X[:, (Nx - mm) % Nx].reshape(Ny, Ny, Mh)
    ref = np.zeros((2 * Ny, 2 * Ny, Mh), dtype=_cdt(dt))                    # the reference's [p, q, m]
    ref[:Ny, :Ny] = gam(m)
    ref[:Ny, Ny:] = xi(m)
    ref[Ny:, :Ny] = np.conj(xi(J))
    ref[Ny:, Ny:] = np.conj(gam(J))
    return np.ascontiguousarray(np.transpose(ref, (2, 1, 0)))


# ---- (b) harmonic space -------------------------------------------------------------------------------------------------------------------
def wigner_d(l, mp, m, beta):
    """d^l_{m' m}(β) by its defining sum"""
    f = math.factorial
    pre = math.sqrt(f(l + mp) * f(l - mp) * f(l + m) * f(l - m))
    c, s = np.cos(beta / 2), np.sin(beta / 2)
    out = np.zeros_like(beta)
    for t in range(max(0, m - mp), min(l + m, l - mp) + 1):
        den = f(l + m - t) * f(t) * f(mp - m + t) * f(l - mp - t)
        out = out + (-1) ** (mp - m + t) * pre / den * c ** (2 * l + m - mp - 2 * t) * s ** (mp - m + 2 * t)
    return out


def sYlm(s, l, m, theta, phi):
    """ₛYℓm(θ, φ) = (-1)^s sqrt((2ℓ+1)/(4π)) d^ℓ_{m,-s}(θ) e^{imφ}; theta (Ny), phi (Nx) -> (Nx, Ny)"""
    return (-1) ** s * math.sqrt((2 * l + 1) / (4 * np.pi)) * np.exp(1j * m * phi)[:, None] * wigner_d(l, m, -s, theta)[None, :]


def _map_cov(s, theta, phi, K, ca, cb):
    """(E[P Pᴴ], E[P Pᵀ]) over the pixels (n, j) flattened, of P = -Σ (E + iB)ℓm ₛYℓm with E_{ℓ,-m} = (-1)^m conj E_ℓm (B alike), orders m ≡ 0
    (mod K) with K times their power; s = 0: ca the spectrum, cb = 0"""
    npx = theta.size * phi.size
    H, S = np.zeros((npx, npx), dtype=np.complex128), np.zeros((npx, npx), dtype=np.complex128)
    for l in range(abs(s), len(ca)):
        for m in range(-l, l + 1):
            if m % K:
                continue
            y, ym = sYlm(s, l, m, theta, phi).ravel(), sYlm(s, l, -m, theta, phi).ravel()
            H += K * (ca[l] + cb[l]) * np.outer(y, np.conj(y))
            S += K * (ca[l] - cb[l]) * (-1) ** m * np.outer(y, ym)
    return H, S


def _patch(Ny, Nx, theta_span, phi_span):
    g = geometry(Ny, Nx, theta_span, phi_span)
    K, ok = span_K(phi_span)
    assert ok
    return g["theta"], g["phi"][0] + np.arange(Nx) * (TWO_PI / (K * Nx)), K


def harmonic_I(Ny, Nx, theta_span, phi_span, cl):
    """-> (blocks [m, q, p] complex, the largest |entry| of the covariance between DIFFERENT m)"""
    theta, phi, K = _patch(Ny, Nx, theta_span, phi_span)
    H, _ = _map_cov(0, theta, phi, K, np.asarray(cl, float), np.zeros(len(cl)))
    Mh = Nx // 2 + 1
    eye = np.eye(Nx * Ny).reshape(Nx * Ny, 1, Nx, Ny)
    A = az_fwd(eye, np.float64).reshape(Nx * Ny, Mh * Ny).T                  # f̂ = A f
    C = (A @ H @ np.conj(A.T)).reshape(Mh, Ny, Mh, Ny)                      # [m, p, m', q]
    return _diag_blocks(C, Mh)


def harmonic_P(Ny, Nx, theta_span, phi_span, cl_ee, cl_bb):
    theta, phi, K = _patch(Ny, Nx, theta_span, phi_span)
    H, S = _map_cov(2, theta, phi, K, np.asarray(cl_ee, float), np.asarray(cl_bb, float))
    Mh, npx = Nx // 2 + 1, Nx * Ny
    eye = np.eye(npx).reshape(npx, Nx, Ny)
    zero = np.zeros_like(eye)
    vq = qu_fwd(np.stack([eye, zero], axis=1), np.float64).reshape(npx, Mh * 2 * Ny).T      # v of P = e_p
    vu = qu_fwd(np.stack([zero, eye], axis=1), np.float64).reshape(npx, Mh * 2 * Ny).T      # v of P = i e_p
    A, B = (vq - 1j * vu) / 2, (vq + 1j * vu) / 2                                           # v = A P + B conj(P)
    AH, BH = np.conj(A.T), np.conj(B.T)
    C = A @ H @ AH + A @ S @ BH + B @ np.conj(S) @ AH + B @ np.conj(H) @ BH
    return _diag_blocks(C.reshape(Mh, 2 * Ny, Mh, 2 * Ny), Mh)


def _diag_blocks(C, Mh):
    off = max((float(np.abs(C[m, :, mm, :]).max()) for m in range(Mh) for mm in range(Mh) if m != mm), default=0.0)
    blocks = np.stack([C[m, :, m, :].T for m in range(Mh)])                 # [m, q, p]
    return blocks, off


# ---- comparison and the shared cases ------------------------------------------------------------------------------------------------------
def err_per_m(got, ref):
    """max_{jk} |Δ| / max_{jk} |ref| per m"""
    got, ref = np.asarray(got), np.asarray(ref)
    d = np.abs(got.astype(ref.dtype) - ref).reshape(ref.shape[0], -1).max(axis=1)
    return np.asarray(d / np.abs(ref).reshape(ref.shape[0], -1).max(axis=1), dtype=np.float64)


REF_THETA_SPAN = (np.pi / 2 + np.deg2rad(40.0), np.pi / 2 + np.deg2rad(70.0))  # test/runtests.jl:629-630
REF_PHI_SPAN = (np.deg2rad(-60.0), np.deg2rad(60.0))
LMAX_TEST = 2000                                                               # see test_equirect_cov_ref.py::test_reference_properties

# (Ny, Nx, theta_span, phi_span) of the GPU cases
GPU_CASES = [(2, 4, (0.6, 2.2), (0.0, TWO_PI)), (5, 12, (0.4, 1.3), (0.3, 0.3 + TWO_PI / 3)), (7, 14, (1.0, 2.9), (-np.pi / 2, np.pi / 2)),
             (32, 64, REF_THETA_SPAN, REF_PHI_SPAN)]


def case_id(c):
    return f"{c[0]}x{c[1]}"


def camb_total(lmax):
    """the total TT, EE, BB of tests/golden/camb_cls.npz as arrays over ℓ = 0 ... lmax (0 below ℓ = 2)"""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camb_cls.npz"))
    out = []
    for k in ("total_TT", "total_EE", "total_BB"):
        a = np.zeros(lmax + 1)
        ell = d["ell"]
        sel = ell <= lmax
        a[ell[sel]] = d[k][sel]
        out.append(a)
    return out


# ---- the reference's own properties (test/runtests.jl:691-720) on blocks, NumPy float64 ---------------------------------------------------
def reference_properties(C, spin, Nx, seed=0):
    """{name: norm(lhs - rhs) / max(norm(lhs), norm(rhs))} of sqrt·sqrt ≈ C, pinv(C)·C·f ≈ f, (C\\C)·f ≈ f, (C/C)·f ≈ f and fᴴ(C g) ≈ (fᴴ C) g with a
    white map f and g = sqrt(C)·white, on the blocks C [m, q, p] (any precision; the algebra runs in float64 like the product's host side)"""
    import _equirect_ref as E
    C = np.asarray(C)
    C = C.astype(np.complex128 if np.iscomplexobj(C) else np.float64)
    Ny = C.shape[1] // (1 if spin == 0 else 2)
    rng = np.random.default_rng([seed, spin, Ny, Nx])
    P = 1 if spin == 0 else 2
    fwd = (lambda m: E.az_fwd(m, np.float64)) if spin == 0 else (lambda m: E.qu_fwd(m, np.float64))
    inv = (lambda f: E.az_inv(f, Nx, np.float64)) if spin == 0 else (lambda f: E.qu_inv(f, Nx, np.float64))
    f, white = fwd(rng.standard_normal((1, P, Nx, Ny))), fwd(rng.standard_normal((1, P, Nx, Ny)))
    rel = lambda a, b: float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(a.ravel()), np.linalg.norm(b.ravel())))
    S, Pi = E.op_sqrt(C), E.op_pinv(C)
    out = {"sqrt": rel(E.apply(S, E.apply(S, f)), E.apply(C, f)),
           "pinv": rel(E.apply(Pi, E.apply(C, f)), f),
           "solve": rel(E.apply(E.op_solve(C, C), f), f),
           "rdiv": rel(E.apply(E.op_rdiv(C, C), f), f)}
    g = E.apply(S, white)
    a, b = E.field_dot(inv(f), inv(E.apply(C, g))), E.field_dot(inv(E.apply(C, f, adjoint=True)), inv(g))
    out["adjoint"] = abs(a - b) / max(abs(a), abs(b))
    return out
