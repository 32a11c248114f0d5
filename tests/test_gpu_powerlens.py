"""cmbl_powerlens_* on the device against tests/_powerlens_ref.py, the float64 restatement of the reference's PowerLens (src/powerlens.jl) and Taylens
(src/taylens.jl; pinned on its own by tests/test_powerlens_ref.py), on identical inputs: ϕ from a seeded red spectrum scaled to a stated rms
deflection, f and g white noise, P = 2, B = 2 with distinct slices.

Shapes, the smallest at which each path can go wrong:
  64 x 128, 0.7 px   rectangular, so an x / y swap shows; power-of-two transforms; vector accesses
  30 x 45,  0.7 px   any-size transforms, odd Nx, no Nyquist column, npix % 4 = 2: the scalar pointwise kernels in single precision
  12 x 8,   6 px     Taylens' permutation is not the identity and wraps
  64 x 64            the one-launch small path of the flows' size class
  128 x 64           a power of two with Ny > Nx
  96 x 160           the compile-time-plan transforms at the two smallest lengths of their list

Tolerances (relative L2 of output fields, tests/_tol.py).  Double precision: 1e-12, the transform class bound.  Single precision: 3 x the figure of
that case, quantity and order in tests/golden/powerlens_budget.json -- the distance of the restatement's own float32 arithmetic from float64 on
these inputs, never the code under test; the 3 is that of tests/test_gpu_bilinear.py: the engine rounds in another order (another FFT, terms in
pixel units).  Where the file has no entry (orders other than 2 and 4, the three further shapes) the same figure is measured here from the
restatement, run in float32 through the same chain of transforms as the comparison (own32).  Where that figure is zero (order 0, MAP -> MAP: a
copy or a permutation) the result must be equal bit for bit."""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _powerlens_ref as R
from _tol import close

DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
MAP, FOURIER = 0, 1
FWD, INV, ADJ, INVADJ = 0, 1, 2, 3
POWERLENS, TAYLENS = 0, 1
ORDERS = (0, 1, 2, 4, 7)
P, B = R.P, R.B
BUDGET = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "powerlens_budget.json")))["cases"]


def _pkg():
    import cmblensing_jl_amd as C
    return C


_own = {}


def own32(case, q, order, sign, bi, bo):
    """The figure of a comparison that has no budget entry: the restatement in float32 run through the very chain of transforms the comparison
    contains -- the one that makes a Fourier argument from the case's map and the one back to maps (both operators act on maps, src/powerlens.jl:43,
    53), the action (as written up to order 9, in pixel units from order 10 on, where ℓ^n leaves the range of float32), the one that turns L*f into a
    Fourier result or L'g into a map -- and its relative L2 distance from the float64 answer in the basis compared"""
    key = (case, q, order, sign, bi, bo)
    if key not in _own:
        Ny, Nx, _ = R.ALL_CASES[case]
        T = np.float32
        phi, f, g = R.inputs(case, T)
        x = g if q == "PowerLens'g" else f
        if bi != MAP:
            x = R.irfft2(R.rfft2(x), Ny).astype(T)
        L = R.KINDS[q.split("*")[0].split("'")[0]](Ny, Nx, R.THETA, T, order, phi=T(sign) * phi, pixel_units=order >= 10)
        y = R.action(q, L, x, x)
        if q == "PowerLens'g":
            y = y if bo != MAP else R.irfft2(y, Ny).astype(T)
        else:
            y = y if bo == MAP else R.rfft2(y)
        want = wanted(q, R.result(case, q, order, T, np.float64, sign), Ny, bo)
        _own[key] = R.rel(y.astype(want.dtype), want)
    return _own[key]


def tol(case, q, order, prec, sign=1.0, bi=MAP, bo=MAP):
    """(tolerance, whether the result must be equal bit for bit: a copy or a permutation of maps)"""
    if prec == "f64":
        return 1e-12, False
    if sign == 1.0 and case in BUDGET and str(order) in BUDGET[case]["err"][q]:
        return 3.0 * BUDGET[case]["err"][q][str(order)], False
    e = own32(case, q, order, sign, bi, bo)
    return 3.0 * e, e == 0


_projs = {}


def proj(Ny, Nx, prec):
    k = (Ny, Nx, prec)
    if k not in _projs:
        _projs[k] = _pkg().ProjLambert(Ny, Nx, R.THETA, DT[prec][0])
    return _projs[k]


def make(q, p, order):
    C = _pkg()
    return (C.Taylens if q.startswith("Taylens") else C.PowerLens)(p, order)


def lens(case, q, order, prec, phi=None):
    """(context, a fresh operator of the quantity's kind with the case's ϕ set)"""
    C = _pkg()
    Ny, Nx, _ = R.ALL_CASES[case]
    p = proj(Ny, Nx, prec)
    phi = R.inputs(case, DT[prec][1])[0] if phi is None else phi
    return p, make(q, p, order)(C.Field(p, p.tensor(phi[None, None]), C.MAP))


def field(p, a, basis=MAP):
    C = _pkg()
    f = C.Field(p, p.tensor(a), MAP)
    return f if basis == MAP else f.to(basis)


def host(f):
    return f.arr.cpu().numpy()


def act(L, q, x, bo):
    return L._apply(ADJ if q == "PowerLens'g" else FWD, x, basis_out=bo)


def wanted(q, want, Ny, bo):
    """the float64 answer in the basis asked for: L'g is a Fourier field, L*f a map"""
    if q == "PowerLens'g":
        return want if bo == FOURIER else R.irfft2(want, Ny)
    return want if bo == MAP else R.rfft2(want)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", list(R.ALL_CASES))
def test_parity(case, prec):
    T = DT[prec][1]
    Ny = R.ALL_CASES[case][0]
    _, f, g = R.inputs(case, T)
    for q in R.QUANTITIES:
        arg = g if q == "PowerLens'g" else f
        for order in ORDERS:
            p, L = lens(case, q, order, prec)
            want = R.result(case, q, order, T, np.float64)
            for bi in (MAP, FOURIER):
                x = field(p, arg, bi)
                for bo in (MAP, FOURIER):
                    t, exact = tol(case, q, order, prec, bi=bi, bo=bo)
                    out = act(L, q, x, bo)
                    assert out.basis == bo
                    if exact:
                        np.testing.assert_array_equal(host(out), want.astype(T))
                    else:
                        close((q, order, "in", bi, "out", bo), host(out), wanted(q, want, Ny, bo), t)
            t, exact = tol(case, q, order, prec)
            # in place, MAP -> MAP
            x = field(p, arg.copy())
            ptr = ctypes.c_void_p(x.arr.data_ptr())
            assert p.lib.cmbl_powerlens_apply(L._h, ADJ if q == "PowerLens'g" else FWD, MAP, ptr, MAP, ptr, P, B) == 0
            if exact:
                np.testing.assert_array_equal(host(x), want.astype(T))
            else:
                close((q, order, "in place"), host(x), wanted(q, want, Ny, MAP), t)


def test_order_twelve_stays_in_the_range_of_single_precision():
    """as written ℓmax^12 = 4e46 overflows float32; the engine's pixel-unit terms do not.  A plane wave, the case's ϕ (0.7 px rms), fixed seed"""
    C = _pkg()
    case, order = "64x128", 12
    Ny, Nx, _ = R.CASES[case]
    phi = R.inputs(case, np.float32)[0]
    rng = np.random.default_rng(12)
    x, y = np.arange(Nx)[:, None], np.arange(Ny)[None, :]
    f = np.stack([np.cos(2 * np.pi * (mx * x / Nx + my * y / Ny) + ph) for mx, my, ph in zip(rng.integers(1, 6, P * B), rng.integers(1, 6, P * B), rng.uniform(0, 6, P * B))])
    f = f.reshape(B, P, Nx, Ny).astype(np.float32)
    p = proj(Ny, Nx, "f32")
    for q in R.QUANTITIES:
        K = R.KINDS[q.split("*")[0].split("'")[0]]
        want = R.action(q, K(Ny, Nx, R.THETA, np.float64, order, phi=phi.astype(np.float64)), f.astype(np.float64), f.astype(np.float64))
        own = R.action(q, K(Ny, Nx, R.THETA, np.float32, order, phi=phi, pixel_units=True), f, f)
        e32 = R.rel(own.astype(want.dtype), want)
        assert np.isfinite(e32) and e32 > 0
        L = make(q, p, order)(C.Field(p, p.tensor(phi[None, None]), C.MAP))
        got = host(act(L, q, field(p, f), FOURIER if q == "PowerLens'g" else MAP))
        assert np.all(np.isfinite(got)), q
        print(q, "restatement f32", e32, "engine", R.rel(got, want))
        close((q, order), got, want, 3.0 * e32)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx", [(64, 128), (30, 45), (12, 8)])
def test_known_answers_through_set_deflection(Ny, Nx, prec):
    C = _pkg()
    T = DT[prec][1]
    p = proj(Ny, Nx, prec)
    f = np.random.default_rng(Ny + Nx).standard_normal((B, P, Nx, Ny)).astype(T)
    F = field(p, f)
    sy, sx = 3, -(Nx + 2)
    for order in (0, 4):                                             # an integer deflection: a roll at any order, bit for bit
        L = C.Taylens(p, order).set_deflection(*R.const_defl(Ny, Nx, sy, sx, T))
        np.testing.assert_array_equal(host(L * F), np.roll(f, (-sx, -sy), axis=(-2, -1)))
    for u, n in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (-2.5, -2)):          # ties go to the even pixel
        np.testing.assert_array_equal(host(C.Taylens(p, 0).set_deflection(*R.const_defl(Ny, Nx, u, 0.0, T)) * F), np.roll(f, -n, axis=-1))
        np.testing.assert_array_equal(host(C.Taylens(p, 0).set_deflection(*R.const_defl(Ny, Nx, 0.0, u, T)) * F), np.roll(f, -n, axis=-2))
    # a zero deflection and order 0 are copies
    z = np.zeros((Nx, Ny), T)
    np.testing.assert_array_equal(host(C.PowerLens(p, 5).set_deflection(z, z) * F), f)
    np.testing.assert_array_equal(host(C.PowerLens(p, 0).set_deflection(z + T(1e-4), z) * F), f)
    # a plane wave under a constant shift is the truncated series (tests/test_powerlens_ref.py), double precision: transform class bound
    if prec == "f64":
        from math import factorial
        x, y = np.arange(Nx)[:, None], np.arange(Ny)[None, :]
        phase = 2 * np.pi * (2 * x / Nx + 1 * y / Ny)
        uy, ux = 0.3, -0.45
        theta = 2 * np.pi * (2 * ux / Nx + 1 * uy / Ny)
        dx = np.deg2rad(R.THETA / 60)
        w = np.broadcast_to(np.cos(phase), (B, P, Nx, Ny)).copy()
        for order in (2, 7, 12):
            L = C.PowerLens(p, order).set_deflection(np.full((Nx, Ny), uy * dx), np.full((Nx, Ny), ux * dx))
            want = sum(theta ** n / factorial(n) * np.cos(phase + n * np.pi / 2) for n in range(order + 1))
            close(("plane wave", order), host(L * field(p, w)), np.broadcast_to(want, w.shape), 1e-12)


@pytest.mark.parametrize("case", ["64x128", "30x45"])
def test_repeats_are_bit_identical(case):
    f, g = R.inputs(case, np.float32)[1:]
    for q in R.QUANTITIES:
        p, L = lens(case, q, 4, "f32")
        x = field(p, g if q == "PowerLens'g" else f)
        a, b = host(act(L, q, x, MAP)), host(act(L, q, x, MAP))
        _, L2 = lens(case, q, 4, "f32")
        assert np.array_equal(a, b) and np.array_equal(a, host(act(L2, q, x, MAP))), q


@pytest.mark.parametrize("case", ["64x128", "30x45"])
def test_slices_are_independent(case):
    C = _pkg()
    Ny, Nx, _ = R.CASES[case]
    p = proj(Ny, Nx, "f32")
    phi = C.Field(p, p.tensor(R.inputs(case, np.float32)[0][None, None]), C.MAP)
    f = np.random.default_rng(6).standard_normal((2, 3, Nx, Ny)).astype(np.float32)          # P B = 6
    f2 = f.copy()
    f2[1, 0] = np.random.default_rng(9).standard_normal(f2[1, 0].shape)
    for q in R.QUANTITIES:
        L = make(q, p, 3)(phi)
        base, got = host(act(L, q, field(p, f), MAP)), host(act(L, q, field(p, f2), MAP))
        for b in range(2):
            for pol in range(3):
                if (b, pol) != (1, 0):
                    assert np.array_equal(got[b, pol], base[b, pol]), (q, b, pol)
        assert not np.array_equal(got[1, 0], base[1, 0])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_new_phi_replaces_the_table_and_antilensing_negates_it(prec):
    C = _pkg()
    T = DT[prec][1]
    case, order = "30x45", 4
    Ny, Nx, rms = R.CASES[case]
    _, f, g = R.inputs(case, T)
    phi2 = R.make_phi(Ny, Nx, R.THETA, rms, 99)
    for q in R.QUANTITIES:
        p, L = lens(case, q, order, prec)
        x = field(p, g if q == "PowerLens'g" else f)
        first = host(act(L, q, x, MAP))
        F2 = C.Field(p, p.tensor(phi2[None, None]), MAP)
        L(F2)
        fresh = make(q, p, order)(F2)
        again = host(act(L, q, x, MAP))
        assert np.array_equal(again, host(act(fresh, q, x, MAP))) and not np.array_equal(again, first), q
        _, L1 = lens(case, q, order, prec)
        A = C.antilensing(L1)
        assert type(A) is type(L1) and A.order == order
        want = R.result(case, q, order, T, np.float64, sign=-1.0)
        close((q, "antilensing"), host(act(A, q, x, FOURIER if q == "PowerLens'g" else MAP)), want, tol(case, q, order, prec, sign=-1.0)[0])
    # after set_deflection, antilensing negates the deflection
    p = proj(Ny, Nx, prec)
    dy, dx = R.const_defl(Ny, Nx, 2, -1, T)
    A = C.antilensing(C.Taylens(p, 2).set_deflection(dy, dx))
    np.testing.assert_array_equal(host(A * field(p, f)), np.roll(f, (-1, 2), axis=(-2, -1)))


def test_error_codes():
    C = _pkg()
    ARG, SHAPE, STATE = 1, 2, 5
    p = proj(30, 45, "f32")
    lib = p.lib
    f = p.tensor(np.ones((B, P, 45, 30)))
    out = p.empty(MAP, P, B)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    h = ctypes.c_void_p()
    for order, kind in ((-1, POWERLENS), (13, POWERLENS), (13, TAYLENS), (2, 2), (2, -1)):
        assert lib.cmbl_powerlens_create(p._h, order, kind, ctypes.byref(h)) == ARG and not h
        assert b"src/" in lib.cmbl_last_error()
    with pytest.raises(C.CmblError):
        C.PowerLens(p, 13)
    LP, LT = C.PowerLens(p, 2), C.Taylens(p, 2)
    for L in (LP, LT):
        assert lib.cmbl_powerlens_apply(L._h, FWD, MAP, ptr(f), MAP, ptr(out), P, B) == STATE          # as cmbl_lenseflow_apply before any ϕ
        assert b"set_phi" in lib.cmbl_last_error()
    phi2 = p.tensor(np.ones((2, 1, 45, 30)))
    for L in (LP, LT):
        assert lib.cmbl_powerlens_set_phi(L._h, MAP, ptr(phi2), 2) == SHAPE                              # a batched ϕ
        assert b"batched" in lib.cmbl_last_error() and b"src/powerlens.jl:25" in lib.cmbl_last_error()
        assert lib.cmbl_powerlens_set_phi(L._h, MAP, ptr(phi2), 1) == 0
        for mode in (INV, INVADJ, 4, -1):
            assert lib.cmbl_powerlens_apply(L._h, mode, MAP, ptr(f), MAP, ptr(out), P, B) == ARG
        assert lib.cmbl_powerlens_apply(L._h, INV, MAP, ptr(f), MAP, ptr(out), P, B) == ARG and b"no inverse (src/powerlens.jl" in lib.cmbl_last_error()
        assert lib.cmbl_powerlens_apply(L._h, FWD, MAP, ptr(f), MAP, ptr(out), 4, B) == SHAPE
        assert lib.cmbl_powerlens_apply(L._h, FWD, MAP, ptr(f), MAP, ptr(out), P, B) == 0 and torch.isfinite(out).all()
    assert lib.cmbl_powerlens_apply(LT._h, ADJ, MAP, ptr(f), MAP, ptr(out), P, B) == ARG and b"no adjoint (src/taylens.jl" in lib.cmbl_last_error()
    assert lib.cmbl_powerlens_apply(LP._h, ADJ, MAP, ptr(f), MAP, ptr(out), P, B) == 0
    with pytest.raises(NotImplementedError):
        LT.adjoint
    with pytest.raises(C.CmblError):
        LP(C.Field(p, phi2, MAP))
