"""ProjEquiRect on the device against the float64 run of tests/_equirect_ref.py (pinned by tests/test_equirect_ref.py), in both context
precisions: the four transforms, M * f and M' * f with real and complex blocks, the three operator products (matrix cores), dot(M1', M2), the
beams, simulate, the error codes and bit-identical repeats.

Tolerances.  float64: 1e-12 relative L2 (the project's class bound).  float32 products, derived: every output of a length-n complex inner product
evaluated in float32 in ANY order (the MFMA equals an fmaf chain bit for bit) obeys |got − want| ≤ 2 (2n + 4) 2⁻²⁴ (|M| |f|)[p]; asserted
componentwise with |M| |f| formed in float64 from the inputs, and its L2 form is the literal tolerance handed to `_tol.close`.  float32
transforms: 3 x the float32 restatement's own error on the same inputs (tests/golden/equirect_budget.json).  Errors seen on the MI355X:
profiles/equirect_parity.txt."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _equirect_ref as R
import _tol

pytestmark = pytest.mark.gpu

BUDGET = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "equirect_budget.json")))["cases"]
THETA_SPAN = (np.pi / 2 - np.deg2rad(10), np.pi / 2 + np.deg2rad(10))
PHI_SPAN = (0.0, 2 * np.pi)
DTYPES = [torch.float32, torch.float64]
OPCASES = [c for c in R.CASES if c[4]]


@pytest.fixture(scope="module")
def C():
    import cmblensing_jl_amd as C
    return C


_projs = {}


def proj_of(C, Ny, Nx, T):
    k = (Ny, Nx, T)
    if k not in _projs:
        _projs[k] = C.ProjEquiRect(Ny, Nx, THETA_SPAN, PHI_SPAN, T=T)
    return _projs[k]


def host(t):
    return t.detach().cpu().numpy()


_wants = {}


def once(key, fn):
    """the float64 reference of a comparison, computed once and shared between the precisions (never modified)"""
    if key not in _wants:
        _wants[key] = fn()
    return _wants[key]


def l2_of(bound, want):
    return float(np.linalg.norm(bound.ravel()) / np.linalg.norm(np.asarray(want).ravel()))


def check_product(what, got, want, bound, T):
    """float64: 1e-12 relative L2; float32: the derived componentwise bound and its L2 form"""
    got = host(got) if torch.is_tensor(got) else got
    if T == torch.float64:
        return _tol.close(what, got, want, 1e-12)
    worst = float(np.max(np.abs(got - want) / bound))
    print(f"{what}: max |got - want| / bound = {worst:.3f}")
    assert np.all(np.abs(got - want) <= bound), (what, worst)
    return _tol.close(what, got, want, l2_of(bound, want))


@pytest.mark.parametrize("T", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_transforms(C, case, T):
    Ny, Nx, B, spins, _ = case
    p = proj_of(C, Ny, Nx, T)
    for spin in spins:
        m, a = R.case_fields(Ny, Nx, B, spin)
        fwd, inv = (R.az_fwd, R.az_inv) if spin == 0 else (R.qu_fwd, R.qu_inv)
        names = ("az_fwd", "az_inv") if spin == 0 else ("qu_fwd", "qu_inv")
        tol = lambda q: 1e-12 if T == torch.float64 else 3.0 * BUDGET[R.case_id(case)][q]
        fm, fa = C.EquiRectField(p, m, C.MAP), C.EquiRectField(p, a, C.AZFOURIER)
        got_f, got_i = fm.to(C.AZFOURIER), fa.to(C.MAP)
        assert got_f.arr.dtype == p.CT and got_i.arr.dtype == p.T and got_f.basis == C.AZFOURIER and got_i.basis == C.MAP
        e1 = _tol.close(f"{names[0]} {R.case_id(case)}", host(got_f.arr), fwd(m, np.float64), tol(names[0]))
        e2 = _tol.close(f"{names[1]} {R.case_id(case)}", host(got_i.arr), inv(a, Nx, np.float64), tol(names[1]))
        print(f"{R.case_id(case)} spin {spin}: {names[0]} {e1:.2e} (tol {tol(names[0]):.2e}), {names[1]} {e2:.2e} (tol {tol(names[1]):.2e})")
        # a second identical call gives bit-identical output
        assert torch.equal(fm.to(C.AZFOURIER).arr, got_f.arr) and torch.equal(fa.to(C.MAP).arr, got_i.arr)
        if spin == 2:                                                        # the views
            assert torch.equal(fm["Pl"], got_f.arr) and torch.equal(fa["Qx"], got_i.arr[:, 0]) and torch.equal(fa["Px"].imag, got_i.arr[:, 1])
        else:
            assert torch.equal(fm["Il"], got_f.arr) and torch.equal(fa["Ix"], got_i.arr[:, 0])


@pytest.mark.parametrize("T", DTYPES, ids=["f32", "f64"])
def test_qumap_second_assignment_wins_on_the_device(C, T):
    """QUAzFourier(QUMap(a)) of a non-symmetric array: columns 0 and Nx/2 come back as conj(bottom rows) in BOTH halves"""
    Ny, Nx = 32, 64
    p = proj_of(C, Ny, Nx, T)
    _, a = R.case_fields(Ny, Nx, 1, 2)
    back = host(C.EquiRectField(p, a, C.AZFOURIER).to(C.MAP).to(C.AZFOURIER).arr)
    tol = 1e-12 if T == torch.float64 else 3.0 * (BUDGET["32x64_B1"]["qu_fwd"] + BUDGET["32x64_B1"]["qu_inv"])
    for col in (0, Nx // 2):
        _tol.close(f"top of column {col}", back[0, col, :Ny], np.conj(a[0, col, Ny:]), tol)
        _tol.close(f"bottom of column {col}", back[0, col, Ny:], a[0, col, Ny:], tol)
    _tol.close("an inner column", back[0, 1], a[0, 1], tol)


@pytest.mark.parametrize("T", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", OPCASES, ids=R.case_id)
def test_block_apply(C, case, T):
    Ny, Nx, B, spins, _ = case
    p = proj_of(C, Ny, Nx, T)
    Mh = Nx // 2 + 1
    for spin in spins:
        n = Ny if spin == 0 else 2 * Ny
        for nb in sorted({1, B}):
            _, f = R.case_fields(Ny, Nx, nb, spin)
            F = C.EquiRectField(p, f, C.AZFOURIER)
            for cplx in ((False, True) if spin == 0 else (True,)):
                Mn = R.case_blocks(n, Mh, cplx)
                M = C.BlockDiagEquiRect(Mn, p)
                assert M.complex == cplx and M.blocks.dtype == (p.CT if cplx else p.T)
                for adj in (False, True):
                    got = (M.H * F) if adj else (M * F)
                    assert got.basis == C.AZFOURIER and got.arr.dtype == p.CT
                    what = f"M{'h' if adj else ''}*f {R.case_id(case)} n={n} B={nb} {'complex' if cplx else 'real'}"
                    want, bound = once(what, lambda: (R.apply(Mn, f, adj), R.gamma_bound(n, np.abs(Mn), np.abs(f), adj)))
                    check_product(what, got.arr, want, bound, T)
                    again = (M.H * F) if adj else (M * F)
                    assert torch.equal(again.arr, got.arr)


@pytest.mark.parametrize("T", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", OPCASES, ids=R.case_id)
def test_block_products_dot_and_beams(C, case, T):
    Ny, Nx, B, spins, _ = case
    p = proj_of(C, Ny, Nx, T)
    Mh = Nx // 2 + 1
    for spin in spins:
        n = Ny if spin == 0 else 2 * Ny
        for cplx in ((False, True) if spin == 0 else (True,)):
            An, Bn = R.case_blocks(n, Mh, cplx, seed=1), R.case_blocks(n, Mh, cplx, seed=2)
            A, Bm = C.BlockDiagEquiRect(An, p), C.BlockDiagEquiRect(Bn, p)
            for name, adjA, adjB, got in (("A*B", False, False, A * Bm), ("Ah*B", True, False, A.H * Bm), ("A*Bh", False, True, A * Bm.H)):
                assert got.blocks.dtype == A.blocks.dtype and got.n == n
                what = f"{name} {R.case_id(case)} n={n} {'complex' if cplx else 'real'}"
                want, bound = once(what, lambda: (R.matmul(An, Bn, adjA, adjB), R.gamma_bound_mm(n, np.abs(An), np.abs(Bn), adjA, adjB)))
                check_product(what, got.blocks, want, bound, T)
            assert torch.equal((A * Bm).blocks, (A * Bm).blocks)
            # dot(A', B): accumulated in double from the stored (T) elements
            d, w = A.H.dot(Bm), R.block_dot(An, Bn)
            scale = float(np.sum(np.abs(An.transpose(0, 2, 1)) * np.abs(Bn)))
            assert abs(d - w) <= 1e-12 * scale, (d, w)
            assert A.H.dot(Bm) == d
    # beams from real Ny blocks
    Bi = R.case_blocks(Ny, Mh, False)
    om = np.asarray(p.omega, dtype=np.float64)                               # T.(Ω), as the reference's Ω′
    tol = 1e-12 if T == torch.float64 else 2.0 ** -23                        # one rounding of the product (and of Ω, in T already)
    bI = C.Cl_to_Beam("I", Bi, p)
    _tol.close(f"beam I {R.case_id(case)}", host(bI.blocks), R.scale_columns(Bi, om), tol)
    if 0 in spins and 2 in spins:
        bP = C.Cl_to_Beam("P", Bi, p)
        assert bP.complex and bP.n == 2 * Ny
        _tol.close(f"beam P {R.case_id(case)}", host(bP.blocks), R.beam_pol(Bi, om), tol)
        assert np.count_nonzero(host(bP.blocks)[:, :Ny, Ny:]) == 0 and np.count_nonzero(host(bP.blocks)[:, Ny:, :Ny]) == 0


@pytest.mark.parametrize("T", DTYPES, ids=["f32", "f64"])
def test_host_algebra_and_operator_identities(C, T):
    """the reference's operator tests (test/runtests.jl:690-720) through the device products, rtol 1e-4"""
    Ny, Nx = 32, 64
    p = proj_of(C, Ny, Nx, T)
    Mh = Nx // 2 + 1
    rel = _tol.rel
    for spin in (0, 2):
        n = Ny if spin == 0 else 2 * Ny
        Mn = R.case_blocks(n, Mh, spin == 2, spd=True)
        M = C.BlockDiagEquiRect(Mn, p)
        m, _ = R.case_fields(Ny, Nx, 1, spin)
        f = C.EquiRectField(p, m, C.MAP)
        Mf = host((M * f).arr)
        S = M.sqrt()
        assert S is M.sqrt() and S.blocks.dtype == M.blocks.dtype            # cached, in the block type
        assert rel(host((S * (S * f)).arr), Mf) < 1e-4 and rel(host(((S * S) * f).arr), Mf) < 1e-4
        fa = host(f.to(C.AZFOURIER).arr)
        assert rel(host((M.pinv() * (M * f)).arr), fa) < 1e-4
        assert rel(host((M.solve(M) * f).arr), fa) < 1e-4 and rel(host(((M / M) * f).arr), fa) < 1e-4
        assert rel(host(((M + M) * f).arr), host((M * (2 * f)).arr)) < 1e-6 and rel(host(((2 * M) * f).arr), host((M * (2 * f)).arr)) < 1e-6
        l, s = M.logabsdet()
        assert np.isclose(M.logdet(), l, rtol=1e-12) and np.isclose(l, R.op_logabsdet(Mn)[0], rtol=1e-6)
        g = S * f
        lhs = np.vdot(fa, host((M * g).arr)); rhs = np.vdot(host((M.H * f).arr), host(g.arr))
        assert abs(lhs - rhs) < 1e-4 * abs(lhs)
        assert np.isclose(f.dot(f), R.field_dot(m, m), rtol=1e-5) and np.isclose(f.to(C.AZFOURIER).dot(f.to(C.AZFOURIER)), R.field_dot(m, m), rtol=1e-5)


@pytest.mark.parametrize("T", DTYPES, ids=["f32", "f64"])
def test_simulate(C, T):
    """output type, and the second moment of 64 draws against diag(M): E|f[p, m]|² = M[p, p, m] for f = sqrt(M) AzFourier(white).  Inner columns
    (complex, independent between m): the mean over draws and columns of |f|² / M[p, p, m] per row p has standard error 1 / sqrt(64 (Mh − 2));
    columns 0 and Nx/2 (real): per element, standard error sqrt(2 / 64).  Within 5 standard errors."""
    Ny, Nx, nd = 32, 64, 64
    p = proj_of(C, Ny, Nx, T)
    Mh = Nx // 2 + 1
    Mn = R.case_blocks(Ny, Mh, False, spd=True)
    M = C.BlockDiagEquiRect(Mn, p)
    s = C.simulate(M, seed=7, nbatch=nd)
    assert isinstance(s, C.EquiRectField) and s.basis == C.AZFOURIER and s.arr.dtype == p.CT and tuple(s.arr.shape) == (nd, Mh, Ny)
    M2 = C.BlockDiagEquiRect(R.case_blocks(2 * Ny, Mh, True, spd=True), p)
    s2 = C.simulate(M2, seed=7)
    assert s2.arr.dtype == p.CT and tuple(s2.arr.shape) == (1, Mh, 2 * Ny) and s2.to(C.MAP).arr.dtype == p.T
    diag = np.stack([np.diag(Mn[m]) for m in range(Mh)])                     # (Mh, Ny)
    r = np.abs(host(s.arr).astype(np.complex128)) ** 2 / diag[None]
    inner = r[:, 1:-1].mean(axis=(0, 1))
    assert np.all(np.abs(inner - 1) < 5 / np.sqrt(nd * (Mh - 2))), float(np.max(np.abs(inner - 1)) * np.sqrt(nd * (Mh - 2)))
    edge = r[:, [0, -1]].mean(axis=0)
    assert np.all(np.abs(edge - 1) < 5 * np.sqrt(2.0 / nd)), float(np.max(np.abs(edge - 1)) / np.sqrt(2.0 / nd))
    assert torch.equal(C.simulate(M, seed=7, nbatch=nd).arr, s.arr)


def test_error_codes(C):
    T = torch.float32
    p = proj_of(C, 33, 45, T)
    lib, vp = p.lib, lambda t: ctypes.c_void_p(t.data_ptr())
    m2 = torch.zeros((1, 2, 45, 33), dtype=T, device=p.device)
    a2 = torch.zeros((1, 23, 66), dtype=p.CT, device=p.device)
    assert lib.cmbl_equirect_convert(p._h, C.MAP, vp(m2), C.AZFOURIER, vp(a2), 2, 1) == 2          # QU with odd Nx: CMBL_ERR_SHAPE
    assert lib.cmbl_equirect_convert(p._h, C.AZFOURIER, vp(a2), C.MAP, vp(m2), 2, 1) == 2
    with pytest.raises(ValueError):
        C.EquiRectField(p, m2, C.MAP)
    assert lib.cmbl_equirect_convert(p._h, C.MAP, vp(m2), C.AZFOURIER, vp(a2), 3, 1) == 1          # npol 3: CMBL_ERR_ARG
    assert lib.cmbl_equirect_convert(p._h, C.MAP, vp(m2), C.AZFOURIER, vp(m2), 1, 1) == 1          # in == out
    assert lib.cmbl_equirect_convert(p._h, C.MAP, vp(m2), C.FOURIER, vp(a2), 1, 1) == 1            # not a basis of this projection
    n = 33
    A = torch.zeros((23, n, n), dtype=T, device=p.device); Bm = torch.zeros_like(A); O = torch.zeros_like(A)
    f = torch.zeros((1, 23, n), dtype=p.CT, device=p.device); o = torch.zeros_like(f)
    assert lib.cmbl_equirect_block_apply(p._h, vp(A), 0, 34, 0, vp(f), vp(o), 1) == 2              # n neither Ny nor 2 Ny
    assert lib.cmbl_equirect_block_apply(p._h, vp(A), 0, n, 0, vp(f), vp(f), 1) == 1
    assert lib.cmbl_equirect_block_matmul(p._h, vp(A), 1, vp(Bm), 1, 0, n, vp(O)) == 1              # both adjoint
    assert lib.cmbl_equirect_block_matmul(p._h, vp(A), 0, vp(Bm), 0, 0, n, vp(A)) == 1              # out aliases an input
    assert lib.cmbl_equirect_block_matmul(p._h, vp(A), 0, vp(Bm), 0, 0, 30, vp(O)) == 2
    w = (ctypes.c_double * n)()
    assert lib.cmbl_equirect_block_scale_columns(p._h, vp(A), 0, n, w, n - 1) == 2
    assert lib.cmbl_equirect_block_apply(p._h, vp(A), 0, n, 0, vp(f), vp(o), 1) == 0
    M = C.BlockDiagEquiRect(A, p)
    with pytest.raises(TypeError):
        M.H * M.H
