"""cmbl_bilinear_* on the device against tests/_bilinear_ref.py, the float64 restatement of the reference's BilinearLens (src/bilinearlens.jl,
gmres of src/numerical_algorithms.jl:193-214; pinned on its own by tests/test_bilinear_ref.py), on identical inputs: ϕ from a seeded red spectrum
scaled to a stated rms deflection, f and g white noise, P = 2, B = 2 with distinct slices.

Shapes (tests/_bilinear_ref.py CASES), the smallest at which each path can go wrong:
  64 x 128, 0.7 px   the reference's own test size; rectangular, so an x / y swap shows; power-of-two transforms
  30 x 45,  0.7 px   any-size transforms, odd Nx, no Nyquist column
  12 x 8,   6 px     positions wrap more than once; negative floor / mod

Tolerances (relative L2 of output fields, tests/_tol.py).  Double precision: 1e-12, the transform class bound (the two GMRES formulations differ
by <= 3e-14 on the CPU).  Single precision: 3 x the figure of that case and quantity in tests/golden/bilinear_budget.json -- the distance of the
reference's own Float32 arithmetic from float64 on these inputs, never the code under test; the 3 covers another FFT and another GMRES
formulation.  Known answers through set_deflection are exact (rolls) or bounded as stated at the assertion.  Measured: profiles/bilinear_parity.txt."""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _bilinear_ref as R
from _tol import close

DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
MAP, FOURIER = 0, 1
FWD, INV, ADJ, INVADJ = 0, 1, 2, 3
MODES = {"L*f": FWD, "L'g": ADJ, "L\\f": INV, "L'\\g": INVADJ}
P, B = R.P, R.B
BUDGET = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bilinear_budget.json")))["cases"]


def tol(case, q, prec):
    return 1e-12 if prec == "f64" else 3.0 * BUDGET[case]["err"][q]


def _pkg():
    import cmblensing_jl_amd as C
    return C


_projs = {}


def proj(Ny, Nx, prec):
    k = (Ny, Nx, prec)
    if k not in _projs:
        _projs[k] = _pkg().ProjLambert(Ny, Nx, R.THETA, DT[prec][0])
    return _projs[k]


def lens(case, prec, phi=None):
    """(context, a fresh operator with the case's ϕ set)"""
    C = _pkg()
    Ny, Nx, _ = R.CASES[case]
    p = proj(Ny, Nx, prec)
    phi = R.inputs(case, DT[prec][1])[0] if phi is None else phi
    return p, C.BilinearLens(p)(C.Field(p, p.tensor(phi[None, None]), C.MAP))


def field(p, a, basis=MAP):
    C = _pkg()
    f = C.Field(p, p.tensor(a), MAP)
    return f if basis == MAP else f.to(basis)


def host(f):
    return f.arr.cpu().numpy()


def as_map(p, f):
    return host(f.to(MAP))


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", list(R.CASES))
def test_parity_of_the_four_actions(case, prec):
    T = DT[prec][1]
    p, L = lens(case, prec)
    _, f, g = R.inputs(case, T)
    want = R.results(case, T, np.float64)
    arg = {"L*f": f, "L'g": g, "L\\f": R.lensed_input(case, T), "L'\\g": g}
    for q, mode in MODES.items():
        for bi in (MAP, FOURIER):
            x = field(p, arg[q], bi)
            for bo in (MAP, FOURIER):
                out = L._apply(mode, x, basis_out=bo)
                assert out.basis == bo
                close((q, "in", bi, "out", bo), as_map(p, out), want[q], tol(case, q, prec))


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", list(R.CASES))
def test_parity_of_the_pullback(case, prec):
    T = DT[prec][1]
    p, L = lens(case, prec)
    _, f, g = R.inputs(case, T)
    want = R.results(case, T, np.float64)
    ft = field(p, R.lensed_input(case, T))
    for bd in (MAP, FOURIER):
        for bdf in (MAP, FOURIER):
            dphi, df = L.gradient(ft, field(p, g, bd), basis_df=bdf)
            assert dphi.basis == FOURIER and df.basis == bdf and dphi.arr.shape == (B, 1, p.Nx, p.Nyh)
            close(("dphi", "delta", bd), host(dphi), want["dphi"], tol(case, "dphi", prec))
            close(("df", "delta", bd, "out", bdf), as_map(p, df), want["L'g"], tol(case, "L'g", prec))


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx", [(64, 128), (30, 45), (12, 8)])
def test_known_answers_through_set_deflection(Ny, Nx, prec):
    C = _pkg()
    T = DT[prec][1]
    p = proj(Ny, Nx, prec)
    f = np.random.default_rng(Ny + Nx).standard_normal((B, P, Nx, Ny)).astype(T)
    F = field(p, f)
    sy, sx = 3, -(Nx + 2)
    L = C.BilinearLens(p).set_deflection(np.full((Nx, Ny), sy), np.full((Nx, Ny), sx))
    np.testing.assert_array_equal(host(L * F), np.roll(f, (-sx, -sy), axis=(-2, -1)))          # bit for bit
    np.testing.assert_array_equal(host(L.adjoint * F), np.roll(f, (sx, sy), axis=(-2, -1)))
    # Pl A = I: the Krylov space has one direction -- the breakdown path; L \ (L * f) = f
    e = np.linalg.norm(host(L.ldiv(L * F)) - f) / np.linalg.norm(f)
    assert e < (1e-6 if prec == "f32" else 1e-13), e
    e = np.linalg.norm(host(L.adjoint.ldiv(L.adjoint * F)) - f) / np.linalg.norm(f)
    assert e < (1e-6 if prec == "f32" else 1e-13), e
    L.set_deflection(np.full((Nx, Ny), 0.5), np.zeros((Nx, Ny)))
    np.testing.assert_allclose(host(L * F), 0.5 * (f + np.roll(f, -1, axis=-1)), rtol=0, atol=4 * np.finfo(T).eps * np.abs(f).max())
    L.set_deflection(np.zeros((Nx, Ny)), np.full((Nx, Ny), -1.5))
    np.testing.assert_allclose(host(L * F), 0.5 * (np.roll(f, 1, axis=-2) + np.roll(f, 2, axis=-2)), rtol=0, atol=4 * np.finfo(T).eps * np.abs(f).max())


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", list(R.CASES))
def test_adjoint_identity_on_the_device(case, prec):
    T = DT[prec][1]
    p, L = lens(case, prec)
    _, f, g = R.inputs(case, T)
    F, G = field(p, f), field(p, g)
    lhs, rhs = F.dot(L * G), (L.adjoint * F).dot(G)                   # per batch slot
    scale = np.sqrt(F.dot(F) * G.dot(G))
    assert np.all(np.abs(lhs - rhs) <= (1e-5 if prec == "f32" else 1e-13) * scale), (lhs, rhs)


@pytest.mark.parametrize("case", list(R.CASES))
def test_the_transpose_is_deterministic(case):
    p, L = lens(case, "f32")
    g = field(p, R.inputs(case, np.float32)[2])
    a, b = host(L.adjoint * g), host(L.adjoint * g)
    _, L2 = lens(case, "f32")
    c = host(L2.adjoint * g)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(host(L.adjoint.ldiv(g)), host(L2.adjoint.ldiv(g)))


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", ["64x128", "30x45"])
def test_the_inverse_beats_the_preconditioner_alone(case, prec):
    C = _pkg()
    T = DT[prec][1]
    p, L = lens(case, prec)
    phi, f, _ = R.inputs(case, T)
    ft = L * field(p, f)
    _, Lm = lens(case, prec, phi=-phi)                                 # Pl = BilinearLens(-ϕ)
    res = lambda x: np.linalg.norm(host(L * x) - host(ft)) / np.linalg.norm(host(ft))
    assert res(L.ldiv(ft)) < res(Lm * ft)
    assert res(L.ldiv(ft, maxiter=8)) < res(Lm * ft)


def test_zero_phi_copies():
    C = _pkg()
    p = proj(30, 45, "f32")
    L = C.BilinearLens(p)(C.Field(p, p.tensor(np.zeros((1, 1, 45, 30))), MAP))
    f = np.random.default_rng(1).standard_normal((B, P, 45, 30)).astype(np.float32)
    F = field(p, f)
    for out in (L * F, L.adjoint * F, L.ldiv(F), L.adjoint.ldiv(F)):
        np.testing.assert_array_equal(host(out), f)
    np.testing.assert_array_equal(host(L._apply(FWD, F.to(FOURIER), basis_out=FOURIER)), host(F.to(FOURIER)))
    dphi, df = L.gradient(F, F)
    np.testing.assert_array_equal(host(df), f)


def test_error_codes():
    C = _pkg()
    ARG, SHAPE, STATE = 1, 2, 5
    p = proj(30, 45, "f32")
    L = C.BilinearLens(p)
    f = p.tensor(np.ones((B, P, 45, 30)))
    out = p.empty(MAP, P, B)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    assert p.lib.cmbl_bilinear_apply(L._h, FWD, MAP, ptr(f), MAP, ptr(out), P, B, 5) == STATE          # as cmbl_lenseflow_apply before any ϕ
    Lf = C.LenseFlow(p, 3)
    assert p.lib.cmbl_lenseflow_apply(Lf._h, FWD, MAP, ptr(f), MAP, ptr(out), P, B) == STATE
    phi2 = p.tensor(np.ones((2, 1, 45, 30)))
    assert p.lib.cmbl_bilinear_set_phi(L._h, MAP, ptr(phi2), 2) == SHAPE                                # a batched ϕ
    assert b"batched" in p.lib.cmbl_last_error()
    with pytest.raises(C.CmblError):
        L(C.Field(p, phi2, MAP))
    assert p.lib.cmbl_bilinear_set_phi(L._h, MAP, ptr(phi2), 1) == 0
    assert p.lib.cmbl_bilinear_apply(L._h, 4, MAP, ptr(f), MAP, ptr(out), P, B, 5) == ARG
    assert p.lib.cmbl_bilinear_apply(L._h, INV, MAP, ptr(f), MAP, ptr(out), P, B, 0) == ARG
    assert p.lib.cmbl_bilinear_apply(L._h, INV, MAP, ptr(f), MAP, ptr(out), P, B, 17) == ARG
    assert p.lib.cmbl_bilinear_apply(L._h, FWD, MAP, ptr(f), MAP, ptr(out), 4, B, 5) == SHAPE
    assert p.lib.cmbl_bilinear_apply(L._h, FWD, MAP, ptr(f), MAP, ptr(out), P, B, 5) == 0 and torch.isfinite(out).all()


@pytest.mark.parametrize("case", ["64x128", "30x45"])
def test_slices_are_independent(case):
    p, L = lens(case, "f32")
    f = R.inputs(case, np.float32)[1].copy()
    base = {q: host(L._apply(m, field(p, f))) for q, m in MODES.items()}
    f2 = f.copy()
    f2[1, 0] = np.random.default_rng(9).standard_normal(f2[1, 0].shape)
    for q, m in MODES.items():
        got = host(L._apply(m, field(p, f2)))
        for b in range(B):
            for pol in range(P):
                if (b, pol) != (1, 0):
                    assert np.array_equal(got[b, pol], base[q][b, pol]), (q, b, pol)
        assert not np.array_equal(got[1, 0], base[q][1, 0])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_new_phi_rebuilds_the_anti_lensing_tables(prec):
    C = _pkg()
    T = DT[prec][1]
    case = "30x45"
    Ny, Nx, rms = R.CASES[case]
    p, L = lens(case, prec)
    f = field(p, R.inputs(case, T)[1])
    L.ldiv(f), L.adjoint.ldiv(f)                                       # the tables of -ϕ₁ and both transposes now exist
    phi2 = C.Field(p, p.tensor(R.make_phi(Ny, Nx, R.THETA, rms, 99)[None, None]), MAP)
    L(phi2)
    fresh = C.BilinearLens(p)(phi2)
    for fn in ("ldiv",):
        assert np.array_equal(host(getattr(L, fn)(f)), host(getattr(fresh, fn)(f)))
    assert np.array_equal(host(L.adjoint.ldiv(f)), host(fresh.adjoint.ldiv(f)))
    assert np.array_equal(host(L.adjoint * f), host(fresh.adjoint * f))
