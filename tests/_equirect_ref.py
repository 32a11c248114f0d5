"""NumPy restatement of the reference's ProjEquiRect (src/proj_equirect.jl), written from its formulas: geometry (:71-127), the four basis
transforms (:149-178), the block products (:224-269, 358-360), the beams (:505-533) and the host-side sqrt / pinv / logabsdet (:313-347).

Arrays are the reference's read row-major, as the device holds them: maps (B, P, Nx, Ny); AzFourier fields (B, Nx//2+1, n), n = Ny or 2 Ny;
blocks (Nx//2+1, n, n) indexed [m, q, p] == the reference's blocks[p, q, m].  `dt` is np.float32 or np.float64: every function computes in
that precision (SciPy's pocketfft transforms in the precision of its input), so the float32 run is the yardstick of the float32 budgets."""
import numpy as np
import scipy.fft as sfft

TWO_PI = 2.0 * np.pi


def cdt(dt):
    return np.complex64 if np.dtype(dt) == np.float32 else np.complex128


def rem2pi(x):
    """rem2pi(x, RoundDown): in [0, 2π)"""
    r = np.asarray(x, dtype=np.float64) - TWO_PI * np.floor(np.asarray(x, dtype=np.float64) / TWO_PI)
    r = np.where(r < 0, r + TWO_PI, r)
    return np.where(r >= TWO_PI, r - TWO_PI, r)


def _range(a, b, n):
    i = np.arange(n, dtype=np.float64)
    v = a + (b - a) * (i / (n - 1))
    v[-1] = b
    return v


def geometry(Ny, Nx, theta_span, phi_span):
    t0, t1 = sorted(float(v) for v in theta_span)
    f0, f1 = sorted(float(v) for v in phi_span)
    g = {}
    g["phi_edges"] = rem2pi(_range(f0, f1, Nx + 1))
    g["phi"] = rem2pi(_range(f0, f1, 2 * Nx + 1)[1::2])
    g["theta_edges"] = _range(t0, t1, Ny + 1)
    g["theta"] = _range(t0, t1, 2 * Ny + 1)[1::2]
    g["omega"] = rem2pi(g["phi_edges"][1] - g["phi_edges"][0]) * (np.cos(g["theta_edges"][:-1]) - np.cos(g["theta_edges"][1:]))
    dx = np.sin(g["theta"]) * abs(f0 - f1) / Nx
    k = np.array([i if i < (Nx + 1) // 2 else i - Nx for i in range(Nx)], dtype=np.float64)          # ifftshift(-Nx÷2:(Nx-1)÷2)
    g["lx"] = k[None, :] * (TWO_PI / (Nx * dx))[:, None]                                              # (Ny, Nx)
    return g


# ---- bases (:149-178) -----------------------------------------------------------------------------------------------------------------------
def az_fwd(m, dt):
    """AzFourier(f): (B, 1, Nx, Ny) -> (B, Mh, Ny)"""
    m = np.asarray(m, dtype=dt)
    Nx = m.shape[2]
    return (sfft.rfft(m[:, 0], axis=1) / dt(np.sqrt(Nx))).astype(cdt(dt))


def az_inv(f, Nx, dt):
    """Map(f): (B, Mh, Ny) -> (B, 1, Nx, Ny); c2r: the imaginary parts of m = 0 and (even Nx) m = Nx/2 are never read"""
    f = np.array(f, dtype=cdt(dt))
    f[:, 0] = f[:, 0].real
    if Nx % 2 == 0:
        f[:, -1] = f[:, -1].real
    return (sfft.irfft(f, n=Nx, axis=1) * dt(np.sqrt(Nx))).astype(dt)[:, None]


def _mirror(Nx):
    return (Nx - np.arange(Nx // 2 + 1)) % Nx


def qu_fwd(m, dt):
    """QUAzFourier(f): (B, 2, Nx, Ny) -> (B, Mh, 2 Ny)"""
    m = np.asarray(m, dtype=dt)
    Nx = m.shape[2]
    assert Nx % 2 == 0, "the reference throws a dimension mismatch for odd Nx (:166)"
    F = (sfft.fft((m[:, 0] + 1j * m[:, 1]).astype(cdt(dt)), axis=1) / dt(np.sqrt(Nx))).astype(cdt(dt))
    return np.concatenate([F[:, :Nx // 2 + 1], np.conj(F[:, _mirror(Nx)])], axis=2)


def qu_inv(f, Nx, dt):
    """QUMap(f): (B, Mh, 2 Ny) -> (B, 2, Nx, Ny); the second assignment wins at columns 0 and Nx/2 (:174-175)"""
    f = np.asarray(f, dtype=cdt(dt))
    Ny = f.shape[2] // 2
    F = np.zeros((f.shape[0], Nx, Ny), dtype=cdt(dt))
    F[:, :Nx // 2 + 1] = f[:, :, :Ny]
    F[:, _mirror(Nx)] = np.conj(f[:, :, Ny:])
    P = (sfft.ifft(F, axis=1) * dt(np.sqrt(Nx))).astype(cdt(dt))
    return np.stack([P.real, P.imag], axis=1).astype(dt)


def field_dot(a, b):
    """dot(a, b) of two map arrays (:355)"""
    return float(np.dot(np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()))


# ---- operators (:224-269, 358-360, 505-533) -------------------------------------------------------------------------------------------------
def apply(M, f, adjoint=False):
    """M * f: out[p, m, b] = Σ_q M[p, q, m] f[q, m, b]; M' * f: with conj(M[q, p, m])"""
    Mr = np.conj(M) if adjoint else _ref(M)                                  # [m, p, q] of the matrix that acts
    return (Mr[None] @ np.asarray(f)[..., None])[..., 0]


def matmul(A, B, adjA=False, adjB=False):
    """A * B, A' * B, A * B' as [m, q, p] arrays"""
    assert not (adjA and adjB)
    X = np.conj(A) if adjA else _ref(A)                                      # [m, p, j]
    Y = np.conj(B) if adjB else _ref(B)                                      # [m, j, q]
    return _ref(X @ Y)


def block_dot(A, B):
    """dot(A', B) = Σ conj(A[q, p, m]) B[p, q, m]"""
    return complex(np.sum(np.conj(np.transpose(A, (0, 2, 1))).astype(np.complex128) * np.asarray(B, dtype=np.complex128)))


def scale_columns(M, w):
    """blocks[j, k, m] *= w[k]"""
    return M * np.asarray(w, dtype=M.real.dtype)[None, :, None]


def beam_pol(Bi, w):
    """[B 0; 0 B] * diag(w, w) with the real blocks B: complex (Mh, 2Ny, 2Ny)"""
    Mh, Ny, _ = Bi.shape
    s = scale_columns(Bi, w)
    out = np.zeros((Mh, 2 * Ny, 2 * Ny), dtype=cdt(Bi.dtype))
    out[:, :Ny, :Ny] = s
    out[:, Ny:, Ny:] = s
    return out


def _ref(M):
    return np.transpose(M, (0, 2, 1))                                        # [m, p, q]: the matrices as the reference sees them


def op_sqrt(M):
    u, s, vh = np.linalg.svd(_ref(M).astype(np.complex128 if np.iscomplexobj(M) else np.float64))
    return _ref((u * np.sqrt(s)[:, None, :]) @ vh).astype(M.dtype)


def op_pinv(M):
    return _ref(np.linalg.pinv(_ref(M).astype(np.complex128 if np.iscomplexobj(M) else np.float64))).astype(M.dtype)


def op_solve(A, B):
    """A \\ B"""
    return _ref(np.linalg.solve(_ref(A).astype(np.complex128), _ref(B).astype(np.complex128)))


def op_rdiv(A, B):
    """A / B"""
    return _ref(_ref(A).astype(np.complex128) @ np.linalg.inv(_ref(B).astype(np.complex128)))


def op_logabsdet(M):
    sign, lad = np.linalg.slogdet(_ref(M).astype(np.complex128 if np.iscomplexobj(M) else np.float64))
    return float(lad.sum()), complex(np.prod(sign))


def op_logdet(M):
    l, s = op_logabsdet(M)
    return l + np.log(s)


# ---- the inputs of the GPU cases (float32-representable, so that both precisions and the budgets see the same numbers) ----------------------
# (Ny, Nx, nbatch, spins, operators?)
CASES = [(32, 64, 1, (0, 2), True), (64, 32, 3, (0, 2), True), (17, 30, 3, (0, 2), True), (33, 45, 1, (0,), True), (65, 16, 1, (0, 2), True),
         (96, 64, 3, (0, 2), True), (8, 4096, 1, (0, 2), True), (4096, 2, 1, (0, 2), False)]


def case_id(c):
    return f"{c[0]}x{c[1]}_B{c[2]}"


def _r32(a):
    return a.astype(np.float32).astype(np.float64)


def case_fields(Ny, Nx, B, spin, seed=0):
    """(map, az): a random map and an independent random, NON-symmetric array in the azimuthal basis"""
    rng = np.random.default_rng([seed, Ny, Nx, B, spin])
    P = 1 if spin == 0 else 2
    m = _r32(rng.standard_normal((B, P, Nx, Ny)))
    az = _r32(rng.standard_normal((B, Nx // 2 + 1, P * Ny))) + 1j * _r32(rng.standard_normal((B, Nx // 2 + 1, P * Ny)))
    return m, az


def case_blocks(n, Mh, cplx, seed=0, spd=False):
    """random blocks [m, q, p]; spd: A A' + I per m (Hermitian positive definite)"""
    rng = np.random.default_rng([seed, n, Mh, int(cplx), int(spd)])
    A = rng.standard_normal((Mh, n, n)) / np.sqrt(n)
    if cplx:
        A = A + 1j * rng.standard_normal((Mh, n, n)) / np.sqrt(n)
    if spd:
        A = A @ np.conj(np.transpose(A, (0, 2, 1))) + np.eye(n)[None]
    if cplx:
        return _r32(A.real) + 1j * _r32(A.imag)
    return _r32(A)


def gamma_bound(n, absM, absf, adjoint=False):
    """2 (2n + 4) 2^-24 (|M| |f|)[p]: the componentwise bound on a float32 evaluation, in any order, of the length-n complex inner products"""
    return 2.0 * (2 * n + 4) * 2.0 ** -24 * apply(absM, absf, adjoint)


def gamma_bound_mm(n, absA, absB, adjA=False, adjB=False):
    return 2.0 * (2 * n + 4) * 2.0 ** -24 * matmul(absA, absB, adjA, adjB)
