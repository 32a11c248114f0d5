"""NumPy restatement of the one-sided Jacobi SVD of csrc/kernels_equirect_factor.hpp (k_eqf_jacobi) -- the same pair schedule, rotation
threshold, skip rules and noise floor, in float64 -- and the inputs that tests/test_gpu_equirect_factor.py and tests/test_equirect_factor_ref.py
share.  Matrices here are mathematical, [m, p, q] (row, column); `_equirect_ref._ref` turns the device layout [m, q, p] into it.

What differs from the device: the order in which the three inner products of a pair are summed (NumPy's pairwise sums, the device's wave
butterfly).  That moves the last bits of a rotation, not the scheme."""
import numpy as np

import _equirect_ref as R

SWEEP_CAP = 60                                             # EQF_SWEEPS
# (Ny, Nx) of the GPU file: real n = Ny and complex n = 2 Ny blocks give n in {2, 3, 4, 6, 17, 33, 34, 64, 65, 66, 128, 130}
SHAPES = [(2, 4), (3, 6), (17, 30), (33, 8), (64, 8), (65, 4)]


def kinds(Ny):
    """(n, complex) of the two operator families on a projection with Ny rings"""
    return [(Ny, False), (2 * Ny, True)]


def schedule(n):
    """rounds of disjoint pairs (i < j): np = n + (n & 1) columns, R = np - 1 rounds; pair 0 of round r is (np - 1, r), pair k >= 1 is
    ((r + k) mod R, (r - k) mod R); a pair with the dummy column np - 1 of an odd n is dropped"""
    npad = n + (n & 1)
    Rr = npad - 1
    rounds = []
    for r in range(Rr):
        pr = []
        for k in range(npad // 2):
            a, b = (npad - 1, r) if k == 0 else ((r + k) % Rr, (r + Rr - k) % Rr)
            i, j = min(a, b), max(a, b)
            if j < n:
                pr.append((i, j))
        rounds.append(pr)
    return rounds


def jacobi_svd(A, cap=SWEEP_CAP):
    """A: (Mh, n, n) [m, p, q].  Returns G, V (A = G V^H, the columns of G orthogonal), sigma (Mh, n) unsorted, sweeps (Mh,) ints and
    converged (Mh,) bools.  All blocks advance together; a block that has converged rotates nothing in later sweeps (its state is a fixed
    point), so its count stays what a lone run would give."""
    A = np.asarray(A)
    cplx = np.iscomplexobj(A)
    G = A.astype(np.complex128 if cplx else np.float64).copy()
    Mh, n, _ = G.shape
    V = np.broadcast_to(np.eye(n, dtype=G.dtype), G.shape).copy()
    tol = n * 2.0 ** -53
    fro = np.sum(np.abs(G) ** 2, axis=(1, 2))
    floor2, dead2 = (tol * tol * fro)[:, None], (2.0 ** -212 * fro)[:, None]
    rounds = [(np.array([p[0] for p in pr], dtype=int), np.array([p[1] for p in pr], dtype=int)) for pr in schedule(n)]
    sweeps = np.zeros(Mh, dtype=int)
    done = np.zeros(Mh, dtype=bool)
    for _ in range(cap):
        rotated = np.zeros(Mh, dtype=bool)
        for I, J in rounds:
            if I.size == 0:
                continue
            gi, gj = G[:, :, I], G[:, :, J]
            al, be = np.sum(np.abs(gi) ** 2, axis=1), np.sum(np.abs(gj) ** 2, axis=1)
            ga = np.sum(np.conj(gi) * gj, axis=1)
            ag = np.abs(ga)
            with np.errstate(all="ignore"):
                rot = (al != 0) & (be != 0) & (ag != 0) & ~((al <= floor2) & (be <= floor2)) & (al > dead2) & (be > dead2) & \
                    (ag > tol * np.sqrt(al * be))
                zeta = np.where(rot, (be - al) / (2.0 * np.where(rot, ag, 1.0)), 0.0)
                t = np.where(zeta >= 0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
                ph = np.where(rot, ga / np.where(rot, ag, 1.0), 1.0)
            c = np.where(rot, c, 1.0)[:, None, :]
            sp = np.where(rot, s * ph, 0.0)[:, None, :]
            spc = np.conj(sp)
            for X in (G, V):
                xi, xj = X[:, :, I], X[:, :, J]
                X[:, :, I], X[:, :, J] = c * xi - spc * xj, sp * xi + c * xj
            rotated |= rot.any(axis=1)
        sweeps[~done] += 1
        done |= ~rotated
        if done.all():
            break
    return G, V, np.sqrt(np.sum(np.abs(G) ** 2, axis=1)), sweeps, done


def assemble(G, V, sig, rtol=1e-15):
    """(sqrt, pinv) = (G diag(sigma^-1/2) V^H with the term dropped where sigma == 0, V diag(sigma^-2, 0 where sigma <= rtol max sigma) G^H), like
    k_eqf_assemble"""
    with np.errstate(divide="ignore", over="ignore"):
        ws = np.where(sig > 0, 1.0 / np.sqrt(sig), 0.0)
        wp = np.where(sig > rtol * sig.max(axis=1, keepdims=True), 1.0 / (sig * sig), 0.0)
    VH, GH = np.conj(np.transpose(V, (0, 2, 1))), np.conj(np.transpose(G, (0, 2, 1)))
    return (G * ws[:, None, :]) @ VH, (V * wp[:, None, :]) @ GH


# ---- inputs (all float32-representable) ------------------------------------------------------------------------------------------------------
def _haar(rng, Mh, n, cplx):
    Z = rng.standard_normal((Mh, n, n))
    if cplx:
        Z = Z + 1j * rng.standard_normal((Mh, n, n))
    Q, Rm = np.linalg.qr(Z)
    d = np.diagonal(Rm, axis1=1, axis2=2)
    return Q * (d / np.abs(d))[:, None, :]


def _r32c(A):
    return R._r32(A.real) + 1j * R._r32(A.imag) if np.iscomplexobj(A) else R._r32(A)


def general_blocks(n, Mh, cplx, seed=0):
    """well-conditioned general blocks [m, q, p]: U diag(s) V^H, s uniform in [0.5, 2], Haar U, V from a seeded QR"""
    rng = np.random.default_rng([seed, n, Mh, int(cplx), 77])
    s = rng.uniform(0.5, 2.0, (Mh, n))
    A = (_haar(rng, Mh, n, cplx) * s[:, None, :]) @ np.conj(np.transpose(_haar(rng, Mh, n, cplx), (0, 2, 1)))
    return R._ref(_r32c(A))


# seeds of R.case_blocks(n, Mh, cplx, seed) whose blocks all have condition number <= 1e3 (chosen on the CPU; the tests assert the bound)
GAUSS_SEED = {(128, 5, True): 2}


def gauss_blocks(n, Mh, cplx):
    return R.case_blocks(n, Mh, cplx, seed=GAUSS_SEED.get((n, Mh, cplx), 0))


def _quant(a, bits):
    return np.round(a * 2.0 ** bits) / 2.0 ** bits


def half_rank_blocks(n, Mh, cplx, seed=0):
    """general blocks of rank r = n - n // 2 EXACTLY, float32-representable: L B with B (r x n) = U diag(s) V^H, s in [0.6, 2], rounded to
    multiples of 2^-10, and L (n x r) = [I; Q], every row of Q one entry +-1/2.  Every entry of L B is a multiple of 2^-11
    below 4 in modulus: exact in float32 and in the float64 product that forms it.  L^H L >= I, so the r non-zero singular values stay >= those of
    B (>= 0.5 after the rounding); the other n // 2 are zero up to the rounding of whoever factorises.  (A plain U diag(s, 0) V^H rounded to
    float32 would have its zero singular values at 1e-8: neither rank deficient nor cut by rtol = 1e-10.)"""
    rng = np.random.default_rng([seed, n, Mh, int(cplx), 78])
    r = n - n // 2
    s = rng.uniform(0.6, 2.0, (Mh, r))
    U, V = _haar(rng, Mh, r, cplx), _haar(rng, Mh, n, cplx)
    B = (U * s[:, None, :]) @ np.conj(np.transpose(V, (0, 2, 1)))[:, :r, :]
    B = _quant(B.real, 10) + 1j * _quant(B.imag, 10) if cplx else _quant(B, 10)
    L = np.zeros((Mh, n, r))
    L[:, np.arange(r), np.arange(r)] = 1.0
    for m in range(Mh):
        L[m, r + np.arange(n - r), rng.integers(0, r, n - r)] = rng.choice([-0.5, 0.5], n - r)
    A = L @ B
    assert np.array_equal(_r32c(A), A)
    return R._ref(A)


def psd_half_rank_blocks(n, Mh, cplx, seed=0):
    """Hermitian positive semi-definite blocks of rank r = n - n // 2 exactly: C C^H with the entries of C (n x r) multiples of 2^-5 in [-2, 2]
    (every product a multiple of 2^-10, the sums below 2^11: exact in float32)"""
    rng = np.random.default_rng([seed, n, Mh, int(cplx), 79])
    r = n - n // 2
    q = lambda: np.clip(_quant(rng.standard_normal((Mh, n, r)) / np.sqrt(2.0), 5), -2.0, 2.0)
    C = q() + 1j * q() if cplx else q()
    A = C @ np.conj(np.transpose(C, (0, 2, 1)))
    assert np.array_equal(_r32c(A), A)
    return R._ref(A)


def with_zero_block(blocks, m=1):
    """the same blocks with block m all zeros"""
    b = blocks.copy()
    b[m] = 0
    return b


KINDS = ("general", "spd", "gauss", "halfrank", "psdhalf", "zeroblock")


def svd_inputs(n, Mh, cplx):
    """{kind: blocks [m, q, p]} of every input the GPU file hands to the device SVD for one block size"""
    return {"general": general_blocks(n, Mh, cplx), "spd": R.case_blocks(n, Mh, cplx, spd=True), "gauss": gauss_blocks(n, Mh, cplx),
            "halfrank": half_rank_blocks(n, Mh, cplx), "psdhalf": psd_half_rank_blocks(n, Mh, cplx),
            "zeroblock": with_zero_block(general_blocks(n, Mh, cplx))}
