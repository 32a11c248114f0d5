"""Pins tests/_equirect_ref.py, the NumPy restatement of the reference's ProjEquiRect that tests/test_gpu_equirect.py compares the device with:
the reference's own property tests that need no CirculantCov (test/runtests.jl:641-732) at its size (32, 64) in both precisions, the
"second assignment wins" rule of QUMap, the library's host geometry (`cmbl_equirect_geometry_host`, needs no device) against the restatement,
the float32 budgets of the transforms (tests/golden/equirect_budget.json) and the derived γ-bound of the float32 products on every GPU case."""
import json
import os

import numpy as np
import pytest

import _equirect_ref as R

BUDGET_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "equirect_budget.json")
NY, NX = 32, 64
THETA_SPAN = (np.pi / 2 - np.deg2rad(10), np.pi / 2 + np.deg2rad(10))
RTOL = 1e-4                                                                  # the reference's (test/runtests.jl:636)


def rel(a, b):
    return float(np.linalg.norm((np.asarray(a) - np.asarray(b)).ravel()) / np.linalg.norm(np.asarray(b).ravel()))


def test_geometry_properties():
    """edges and centres interleave strictly increasing; the φ-span identity of the non-periodic case (test/runtests.jl:641-653)"""
    span = (np.deg2rad(-50.0), np.deg2rad(50.0))
    g = R.geometry(NY, NX, THETA_SPAN, span)
    assert g["theta"].shape == (NY,) and g["phi"].shape == (NX,) and g["lx"].shape == (NY, NX)
    inter = np.empty(2 * NY + 1)
    inter[0::2], inter[1::2] = g["theta_edges"], g["theta"]
    assert np.all(np.diff(inter) > 0)
    dpix = R.rem2pi(g["phi"][1] - g["phi"][0])
    got = R.rem2pi(g["phi"][-1] - g["phi"][0]) + dpix
    assert np.isclose(got, R.rem2pi(span[1] - span[0]), rtol=1e-12)
    assert np.all((g["phi"] >= 0) & (g["phi"] < 2 * np.pi)) and np.all((g["phi_edges"] >= 0) & (g["phi_edges"] < 2 * np.pi))
    assert np.isclose(g["omega"].sum() * NX, (span[1] - span[0]) * (np.cos(THETA_SPAN[0]) - np.cos(THETA_SPAN[1])), rtol=1e-12)   # the patch's solid angle


@pytest.mark.parametrize("spans", [(THETA_SPAN, (0.0, 2 * np.pi)), (THETA_SPAN, (np.deg2rad(-50.0), np.deg2rad(50.0))), ((2.0, 1.0), (5.0, 0.5))])
@pytest.mark.parametrize("shape", [(32, 64), (17, 30), (33, 45), (2, 2)])
def test_library_geometry_matches_the_restatement(spans, shape):
    import cmblensing_jl_amd as C
    g, w = C.equirect_geometry(shape[0], shape[1], *spans), R.geometry(shape[0], shape[1], *spans)
    for k in w:
        assert g[k].shape == w[k].shape, k
        assert np.all(np.abs(g[k] - w[k]) <= 1e-15 * np.abs(w[k]) + 1e-300), (k, np.max(np.abs(g[k] - w[k])))


def test_library_geometry_rejects_bad_sizes():
    import cmblensing_jl_amd as C
    with pytest.raises(C.CmblError) as e:
        C.equirect_geometry(1, 64, THETA_SPAN, (0.0, 1.0))
    assert e.value.code == 2
    with pytest.raises(C.CmblError) as e:
        C.equirect_geometry(8, 4097, THETA_SPAN, (0.0, 1.0))
    assert e.value.code == 2


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_transform_properties(dt):
    """round trips, basis-independent dot, v ≈ conj(w) at the monopole and Nyquist columns (test/runtests.jl:664-678, 722-732)"""
    tol = 1e-5 if dt == np.float32 else 1e-13
    f0, _ = R.case_fields(NY, NX, 1, 0)
    f2, _ = R.case_fields(NY, NX, 1, 2)
    a0, a2 = R.az_fwd(f0, dt), R.qu_fwd(f2, dt)
    assert a0.shape == (1, NX // 2 + 1, NY) and a2.shape == (1, NX // 2 + 1, 2 * NY)
    assert a0.dtype == R.cdt(dt) and a2.dtype == R.cdt(dt)
    m0, m2 = R.az_inv(a0, NX, dt), R.qu_inv(a2, NX, dt)
    assert m0.dtype == dt and m2.dtype == dt
    assert rel(m0, f0) < tol and rel(m2, f2) < tol
    assert np.isclose(R.field_dot(m0, m0), R.field_dot(f0, f0), rtol=10 * tol) and np.isclose(R.field_dot(m2, m2), R.field_dot(f2, f2), rtol=10 * tol)
    # the transforms are unitary up to the Hermitian double counting: |f|² = Σ λ_m |a|², λ = 1 at m = 0 and Nx/2, else 2 (spin 0); Σ |a|² / 2 ... (spin 2: both halves)
    lam = np.full(NX // 2 + 1, 2.0); lam[0] = lam[-1] = 1.0
    assert np.isclose(np.sum(lam[None, :, None] * np.abs(a0.astype(np.complex128)) ** 2), R.field_dot(f0, f0), rtol=10 * tol)
    for col in (0, NX // 2):
        v, w = a2[0, col, :NY], a2[0, col, NY:]
        assert rel(v, np.conj(w)) < tol
    # odd Nx: spin 0 round trip
    f, _ = R.case_fields(33, 45, 1, 0)
    assert rel(R.az_inv(R.az_fwd(f, dt), 45, dt), f) < tol


def test_qumap_second_assignment_wins():
    """a NON-symmetric QUAzFourier array through QUMap: columns 0 and Nx/2 of the spectrum are conj(bottom rows), not the top rows (:174-175)"""
    _, a = R.case_fields(NY, NX, 1, 2)
    m = R.qu_inv(a, NX, np.float64)
    F = np.fft.fft(m[:, 0] + 1j * m[:, 1], axis=1) / np.sqrt(NX)             # (1, Nx, Ny)
    for col in (0, NX // 2):
        assert rel(F[0, col], np.conj(a[0, col, NY:])) < 1e-13
        assert rel(F[0, col], a[0, col, :NY]) > 0.5
    assert rel(F[0, 1], a[0, 1, :NY]) < 1e-13 and rel(F[0, NX - 1], np.conj(a[0, 1, NY:])) < 1e-13
    # ... so QUAzFourier(QUMap(a)) is a projection, not the identity, on such an array
    assert rel(R.qu_fwd(m, np.float64), a) > 0.1


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("spin", [0, 2])
def test_operator_properties(dt, spin):
    """test/runtests.jl:690-720 with synthetic blocks A A' + I per m in place of Cℓ_to_Cov"""
    n, Mh = (NY if spin == 0 else 2 * NY), NX // 2 + 1
    cd = R.cdt(dt)
    M = R.case_blocks(n, Mh, spin == 2, spd=True).astype(cd if spin == 2 else dt)
    fm, _ = R.case_fields(NY, NX, 1, spin)
    f = (R.az_fwd(fm, dt) if spin == 0 else R.qu_fwd(fm, dt))
    Mf = R.apply(M, f)
    assert Mf.dtype == cd
    S, Pi = R.op_sqrt(M), R.op_pinv(M)
    assert S.dtype == M.dtype and Pi.dtype == M.dtype
    assert rel(R.apply(S, R.apply(S, f)), Mf) < RTOL
    assert rel(R.apply(R.matmul(S, S), f), Mf) < RTOL
    assert rel(R.apply(Pi, Mf), f) < RTOL
    assert rel(R.apply(R.op_solve(M, M).astype(cd), f), f) < RTOL
    assert rel(R.apply(R.op_rdiv(M, M).astype(cd), f), f) < RTOL
    tol = 1e-5 if dt == np.float32 else 1e-13
    assert rel(R.apply(M + M, f), R.apply(M, 2 * f)) < tol and rel(R.apply(2 * M, f), R.apply(M, 2 * f)) < tol
    l, s = R.op_logabsdet(M)
    assert np.isclose(R.op_logdet(M), l, rtol=1e-12)
    # adjoint: <f, M g> = <M' f, g>, and the three product forms against plain matrix algebra
    g = R.apply(S, f)
    lhs, rhs = np.vdot(f.astype(np.complex128), R.apply(M, g).astype(np.complex128)), np.vdot(R.apply(M, f, adjoint=True).astype(np.complex128), g.astype(np.complex128))
    assert abs(lhs - rhs) < RTOL * abs(lhs)
    A, B = R.case_blocks(n, Mh, spin == 2, seed=1), R.case_blocks(n, Mh, spin == 2, seed=2)
    Ar, Br = np.transpose(A, (0, 2, 1)), np.transpose(B, (0, 2, 1))          # [m, p, q]
    H = lambda X: np.conj(np.transpose(X, (0, 2, 1)))
    for adjA, adjB, want in ((False, False, Ar @ Br), (True, False, H(Ar) @ Br), (False, True, Ar @ H(Br))):
        assert rel(np.transpose(R.matmul(A, B, adjA, adjB), (0, 2, 1)), want) < 1e-13
    assert np.isclose(R.block_dot(A, B), np.einsum("mqp,mpq->", np.conj(Ar), Br), rtol=1e-12)
    fq = R.apply(A, f.astype(np.complex128))
    assert rel(fq[0, 3], Ar[3] @ f[0, 3].astype(np.complex128)) < 1e-13 and rel(R.apply(A, f.astype(np.complex128), True)[0, 3], H(Ar)[3] @ f[0, 3].astype(np.complex128)) < 1e-13


def test_beams():
    Mh = NX // 2 + 1
    Bi = R.case_blocks(NY, Mh, False)
    w = R.geometry(NY, NX, THETA_SPAN, (0.0, 2 * np.pi))["omega"]
    Br = np.transpose(Bi, (0, 2, 1))
    assert rel(np.transpose(R.scale_columns(Bi, w), (0, 2, 1)), Br @ np.diag(w)) < 1e-14
    Z = np.zeros((NY, NY))
    want = np.stack([np.block([[Br[m], Z], [Z, Br[m]]]) @ np.diag(np.concatenate([w, w])) for m in range(Mh)])
    got = R.beam_pol(Bi, w)
    assert got.dtype == np.complex128 and rel(np.transpose(got, (0, 2, 1)), want) < 1e-14


# ---- float32: the budgets of the transforms and the derived bound of the products, on the very inputs of the GPU cases -----------------------
def transform_budgets():
    """per case and quantity: relative L2 distance of the float32 restatement from its own float64 result on the same inputs"""
    out = {}
    for c in R.CASES:
        Ny, Nx, B, spins, _ = c
        e = {}
        for spin in spins:
            m, a = R.case_fields(Ny, Nx, B, spin)
            fwd, inv = (R.az_fwd, R.az_inv) if spin == 0 else (R.qu_fwd, R.qu_inv)
            e["az_fwd" if spin == 0 else "qu_fwd"] = rel(fwd(m, np.float32), fwd(m, np.float64))
            e["az_inv" if spin == 0 else "qu_inv"] = rel(inv(a, Nx, np.float32), inv(a, Nx, np.float64))
        out[R.case_id(c)] = e
    return out


def test_transform_budget_file():
    """tests/golden/equirect_budget.json holds the float32 restatement's own error per case and quantity (the GPU test allows 3 x that).  With
    CMBL_WRITE_EQUIRECT_BUDGET=1 the file is written; otherwise the committed figures must be what this machine's pocketfft gives, within a
    factor 2 (its float32 kernels differ a little between vector widths)."""
    now = transform_budgets()
    if os.environ.get("CMBL_WRITE_EQUIRECT_BUDGET"):
        with open(BUDGET_PATH, "w") as f:
            json.dump({"what": "relative L2 error of the float32 run of tests/_equirect_ref.py against its float64 run, same inputs", "cases": now}, f, indent=1, sort_keys=True)
            f.write("\n")
    have = json.load(open(BUDGET_PATH))["cases"]
    assert sorted(have) == sorted(now)
    for k, e in now.items():
        assert sorted(have[k]) == sorted(e), k
        for q, v in e.items():
            assert 0 < have[k][q] < 1e-5 and 0.5 * v <= have[k][q] <= 2 * v, (k, q, have[k][q], v)


@pytest.mark.parametrize("case", [c for c in R.CASES if c[4]], ids=R.case_id)
def test_float32_products_stay_inside_the_derived_bound(case):
    """|got − want| ≤ 2 (2n + 4) 2⁻²⁴ (|M| |f|)[p] holds for the float32 restatement itself on every GPU case: the bound is not too tight for
    correct code (it is the bound tests/test_gpu_equirect.py asserts of the device)"""
    Ny, Nx, B, spins, _ = case
    Mh = Nx // 2 + 1
    for spin in spins:
        n = Ny if spin == 0 else 2 * Ny
        _, f = R.case_fields(Ny, Nx, B, spin)
        for cplx in ((False, True) if spin == 0 else (True,)):
            M = R.case_blocks(n, Mh, cplx)
            M32, f32 = M.astype(np.complex64 if cplx else np.float32), f.astype(np.complex64)
            for adj in (False, True):
                got, want = R.apply(M32, f32, adj), R.apply(M, f, adj)
                assert got.dtype == np.complex64
                bound = R.gamma_bound(n, np.abs(M), np.abs(f), adj)
                assert np.all(np.abs(got - want) <= bound), (spin, cplx, adj, float(np.max(np.abs(got - want) / bound)))
            if n <= 192:
                A, Bm = R.case_blocks(n, Mh, cplx, seed=1), R.case_blocks(n, Mh, cplx, seed=2)
                got, want = R.matmul(A.astype(M32.dtype), Bm.astype(M32.dtype)), R.matmul(A, Bm)
                assert np.all(np.abs(got - want) <= R.gamma_bound_mm(n, np.abs(A), np.abs(Bm)))
