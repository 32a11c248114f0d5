"""tests/_powerlens_ref.py -- the restatement of the reference's PowerLens and Taylens that the GPU tests of cmbl_powerlens_* compare with -- pinned
WITHOUT the engine, by answers that use neither: the truncated series of a plane wave under a constant shift, the adjoint identity, rolls, the
tie rule of the nearest pixel, the order-0 and zero-ϕ copies.

It also makes tests/golden/powerlens_budget.json: per case of the GPU tests, per quantity and per order in {2, 4}, the relative L2 error of the
restatement run in float32 (the reference's own single-precision arithmetic) against the float64 run on the same inputs rounded to float32.  The
file is written when it is missing or CMBL_WRITE_BUDGET=1; otherwise the committed figures must be reproduced within a factor 2."""
import json
import os
from math import factorial

import numpy as np
import pytest

import _powerlens_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "tests", "golden", "powerlens_budget.json")
SHAPES = [(64, 128), (30, 45), (12, 8), (9, 7)]                     # (Ny, Nx)
DX = np.deg2rad(R.THETA / 60)


const_defl = R.const_defl


@pytest.mark.parametrize("Ny,Nx", SHAPES)
def test_plane_wave_under_a_constant_shift_is_the_truncated_series(Ny, Nx):
    """f = cos(k.x) and d constant: every derivative is a phase, so PowerLens(order) f = Σ_{n <= order} θ^n / n! cos(k.x + n π/2), θ = k.d"""
    mx, my = 2, 1
    x, y = np.arange(Nx)[:, None], np.arange(Ny)[None, :]
    phase = 2 * np.pi * (mx * x / Nx + my * y / Ny)
    uy, ux = 0.3, -0.45                                              # pixels
    theta = 2 * np.pi * (mx * ux / Nx + my * uy / Ny)
    f = np.cos(phase)
    exact = np.cos(phase + theta)
    last = np.inf
    for order in range(2, 13):
        L = R.PowerLens(Ny, Nx, R.THETA, np.float64, order, defl=(np.full((Nx, Ny), uy * DX), np.full((Nx, Ny), ux * DX)))
        want = sum(theta ** n / factorial(n) * np.cos(phase + n * np.pi / 2) for n in range(order + 1))
        got = L.mul(f)
        e = np.max(np.abs(got - want))
        assert e < 1e-13, (order, e)
        np.testing.assert_allclose(R.PowerLens(Ny, Nx, R.THETA, np.float64, order, defl=(np.full((Nx, Ny), uy * DX), np.full((Nx, Ny), ux * DX)),
                                               pixel_units=True).mul(f), want, rtol=0, atol=1e-13)
        dist = np.max(np.abs(got - exact))
        assert dist < last or dist < 1e-13, (order, dist, last)     # the distance from the exact shift falls with the order
        last = dist
    assert last < 1e-9                                               # |θ| < 0.2 here: θ^13 / 13!


@pytest.mark.parametrize("order", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("Ny,Nx", SHAPES)
def test_adjoint_identity(Ny, Nx, order):
    """<f, L g> = <L'f, g>, white f and g, even and odd sides"""
    rng = np.random.default_rng(Ny * 31 + Nx + order)
    f, g = rng.standard_normal((2, Nx, Ny))
    dy, dx = (0.7 * DX * rng.standard_normal((Nx, Ny)) for _ in range(2))
    L = R.PowerLens(Ny, Nx, R.THETA, np.float64, order, defl=(dy, dx))
    lhs = np.sum(f * L.mul(g))
    # L'f is a Fourier field whose Nyquist entries need not be those of a real map: the identity holds with its real part folded as irfft does
    rhs = np.sum(R.irfft2(L.adj(f), Ny) * g)
    assert abs(lhs - rhs) <= 1e-13 * abs(lhs), (lhs, rhs)


@pytest.mark.parametrize("T", [np.float64, np.float32])
@pytest.mark.parametrize("Ny,Nx", SHAPES)
def test_taylens_of_an_integer_deflection_is_a_roll_at_any_order(Ny, Nx, T):
    f = np.random.default_rng(0).standard_normal((2, Nx, Ny)).astype(T)
    sy, sx = 3, -(Nx + 2)                                            # longer than a side, negative
    for order in (0, 1, 4, 7):
        L = R.Taylens(Ny, Nx, R.THETA, T, order, defl=const_defl(Ny, Nx, sy, sx, T))
        np.testing.assert_array_equal(L.mul(f), np.roll(f, (-sx, -sy), axis=(-2, -1)))          # f̃[i, j] = f[i + 3, j - (Nx + 2)]


@pytest.mark.parametrize("Ny,Nx", SHAPES)
def test_taylens_below_half_a_pixel_is_powerlens(Ny, Nx):
    rng = np.random.default_rng(5)
    f = rng.standard_normal((2, Nx, Ny))
    dy, dx = (DX * rng.uniform(-0.49, 0.49, (Nx, Ny)) for _ in range(2))
    for order in (1, 3, 4):
        a, b = R.Taylens(Ny, Nx, R.THETA, np.float64, order, defl=(dy, dx)), R.PowerLens(Ny, Nx, R.THETA, np.float64, order, defl=(dy, dx))
        np.testing.assert_array_equal(a.mul(f), b.mul(f))


@pytest.mark.parametrize("T", [np.float64, np.float32])
def test_taylens_half_pixel_ties_go_to_the_even_pixel(T):
    Ny, Nx = 12, 8
    f = np.random.default_rng(2).standard_normal((1, Nx, Ny)).astype(T)
    for u, n in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (-2.5, -2)):
        L = R.Taylens(Ny, Nx, R.THETA, T, 0, defl=const_defl(Ny, Nx, u, 0.0, T))
        np.testing.assert_array_equal(L.mul(f), np.roll(f, -n, axis=-1))
        L = R.Taylens(Ny, Nx, R.THETA, T, 0, defl=const_defl(Ny, Nx, 0.0, u, T))
        np.testing.assert_array_equal(L.mul(f), np.roll(f, -n, axis=-2))


def test_order_zero_and_zero_phi_are_copies():
    f = np.random.default_rng(4).standard_normal((2, 2, 8, 12))
    phi = R.make_phi(12, 8, R.THETA, 0.7, 1)
    for K in (R.PowerLens, R.Taylens):
        np.testing.assert_array_equal(K(12, 8, R.THETA, np.float64, 5, phi=np.zeros((8, 12))).mul(f), f)
    np.testing.assert_array_equal(R.PowerLens(12, 8, R.THETA, np.float64, 0, phi=phi).mul(f), f)
    np.testing.assert_array_equal(R.PowerLens(12, 8, R.THETA, np.float64, 0, phi=phi).adj(f), R.rfft2(f))
    np.testing.assert_array_equal(R.PowerLens(12, 8, R.THETA, np.float64, 5, phi=np.zeros((8, 12))).adj(f), R.rfft2(f))


def test_pixel_units_are_the_same_sum():
    """the engine's form of the terms (ℓΔx, d/Δx) against the form as written, float64"""
    for case in R.CASES:
        for q in R.QUANTITIES:
            a, b = R.result(case, q, 4, np.float64, np.float64), R.result(case, q, 4, np.float64, np.float64, pixel_units=True)
            assert R.rel(a, b) < 1e-13, (case, q)


def budget():
    return {c: {q: {str(o): R.f32_error(c, q, o) for o in R.BUDGET_ORDERS} for q in R.QUANTITIES} for c in R.CASES}


def test_single_precision_budget():
    got = budget()
    if not os.path.exists(BUDGET) or os.environ.get("CMBL_WRITE_BUDGET"):
        with open(BUDGET, "w") as f:
            json.dump({"what": "relative L2 error of tests/_powerlens_ref.py in float32 against float64, inputs rounded to float32, per quantity and order",
                       "theta_pix": R.THETA,
                       "cases": {c: {"Ny": R.CASES[c][0], "Nx": R.CASES[c][1], "rms_px": R.CASES[c][2], "err": got[c]} for c in got}}, f, indent=1)
            f.write("\n")
    table = json.load(open(BUDGET))["cases"]
    assert set(table) == set(R.CASES)
    for c in got:
        for q in R.QUANTITIES:
            for o in map(str, R.BUDGET_ORDERS):
                assert 1e-8 < table[c]["err"][q][o] < 1e-3, (c, q, o)  # single-precision rounding, nothing else
                assert 0.5 < got[c][q][o] / table[c]["err"][q][o] < 2.0, (c, q, o, got[c][q][o], table[c]["err"][q][o])
