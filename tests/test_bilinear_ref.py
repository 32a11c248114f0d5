"""tests/_bilinear_ref.py -- the restatement of the reference's BilinearLens that the GPU tests of cmbl_bilinear_* compare with -- pinned WITHOUT the
engine, by answers that use neither: row sums, rolls, two-point means, the adjoint identity, the residual of the gmres solve, the zero-ϕ identity.

It also makes tests/golden/bilinear_budget.json: per case of the GPU tests and per quantity, the relative L2 error of the restatement run in Float32
(the reference's own single-precision arithmetic, index added in Float32, Krylov basis in Float32) against the float64 run on the same inputs rounded
to float32.  The file is written when it is missing or CMBL_WRITE_BUDGET=1; otherwise the committed figures must be reproduced within a factor 2
(they are norms of rounding errors over thousands of pixels: stable, but not to the bit across BLAS builds)."""
import json
import os

import numpy as np
import pytest

import _bilinear_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "tests", "golden", "bilinear_budget.json")
SHAPES = [(64, 128), (24, 20), (12, 8), (9, 7)]                     # (Ny, Nx)


def smooth_defl(Ny, Nx, amp, seed=3):
    rng = np.random.default_rng(seed)
    return amp * rng.standard_normal((Nx, Ny)), amp * rng.standard_normal((Nx, Ny))


@pytest.mark.parametrize("Ny,Nx", SHAPES)
def test_rows_sum_to_one_and_a_constant_is_invariant(Ny, Nx):
    dy, dx = smooth_defl(Ny, Nx, 2.5)
    L = R.BilinearLens(Ny, Nx, 2.0, np.float64, defl=(dy, dx))
    np.testing.assert_allclose(np.asarray(L.L.sum(axis=1)).ravel(), 1.0, atol=1e-13)
    assert L.L.nnz <= 4 * Ny * Nx and np.all(np.diff(L.L.indptr) <= 4)
    np.testing.assert_allclose(L.mul(np.full((1, Nx, Ny), 3.25)), 3.25, atol=1e-12)


@pytest.mark.parametrize("T", [np.float64, np.float32])
@pytest.mark.parametrize("Ny,Nx", SHAPES)
def test_integer_deflections_roll(Ny, Nx, T):
    f = np.random.default_rng(0).standard_normal((2, Nx, Ny)).astype(T)
    sy, sx = 3, -(Nx + 2)                                            # longer than a side, negative
    L = R.BilinearLens(Ny, Nx, 2.0, T, defl=(np.full((Nx, Ny), sy), np.full((Nx, Ny), sx)))
    np.testing.assert_array_equal(L.mul(f), np.roll(f, (-sx, -sy), axis=(-2, -1)))          # f̃[i, j] = f[i + 3, j - (Nx + 2)]
    np.testing.assert_array_equal(L.adj(f), np.roll(f, (sx, sy), axis=(-2, -1)))


@pytest.mark.parametrize("Ny,Nx", SHAPES)
def test_half_pixel_deflections_average_two_points(Ny, Nx):
    f = np.random.default_rng(1).standard_normal((1, Nx, Ny))
    L = R.BilinearLens(Ny, Nx, 2.0, np.float64, defl=(np.full((Nx, Ny), 0.5), np.zeros((Nx, Ny))))
    np.testing.assert_allclose(L.mul(f), 0.5 * (f + np.roll(f, -1, axis=-1)), atol=1e-14)
    L = R.BilinearLens(Ny, Nx, 2.0, np.float64, defl=(np.zeros((Nx, Ny)), np.full((Nx, Ny), -1.5)))
    np.testing.assert_allclose(L.mul(f), 0.5 * (np.roll(f, 1, axis=-2) + np.roll(f, 2, axis=-2)), atol=1e-14)


@pytest.mark.parametrize("case", list(R.CASES))
def test_adjoint_identity(case):
    Ny, Nx, _ = R.CASES[case]
    phi, f, g = R.inputs(case, np.float64)
    L = R.BilinearLens(Ny, Nx, R.THETA, np.float64, phi=phi)
    lhs, rhs = np.sum(f * L.mul(g)), np.sum(L.adj(f) * g)
    assert abs(lhs - rhs) <= 1e-13 * np.sqrt(np.sum(f * f) * np.sum(g * g))


@pytest.mark.parametrize("case", ["64x128", "30x45"])
def test_gmres_reduces_the_residual(case):
    Ny, Nx, _ = R.CASES[case]
    phi, f, g = R.inputs(case, np.float64)
    L = R.BilinearLens(Ny, Nx, R.THETA, np.float64, phi=phi)
    b = L.mul(f)
    res = lambda x: np.linalg.norm(L.mul(x) - b) / np.linalg.norm(b)
    x0 = np.stack([[(L.anti @ v.ravel()).reshape(Nx, Ny) for v in bb] for bb in b])          # x = Pl b
    assert res(L.ldiv(b)) < res(x0)
    rest = lambda x: np.linalg.norm(L.adj(x) - g) / np.linalg.norm(g)
    x0t = np.stack([[(L.anti.T @ v.ravel()).reshape(Nx, Ny) for v in bb] for bb in g])
    assert rest(L.adj_ldiv(g)) < rest(x0t)


def test_zero_phi_is_the_identity():
    f = np.random.default_rng(4).standard_normal((2, 2, 8, 12))
    L = R.BilinearLens(12, 8, 2.0, np.float64, phi=np.zeros((8, 12)))
    for fn in (L.mul, L.adj, L.ldiv, L.adj_ldiv):
        np.testing.assert_array_equal(fn(f), f)


def budget():
    out = {}
    for case in R.CASES:
        r64, r32 = R.results(case, np.float32, np.float64), R.results(case, np.float32, np.float32)
        out[case] = {q: R.rel(r32[q].astype(r64[q].dtype), r64[q]) for q in R.QUANTITIES}
    return out


def test_single_precision_budget():
    got = budget()
    if not os.path.exists(BUDGET) or os.environ.get("CMBL_WRITE_BUDGET"):
        with open(BUDGET, "w") as f:
            json.dump({"what": "relative L2 error of tests/_bilinear_ref.py in float32 against float64, inputs rounded to float32", "theta_pix": R.THETA,
                       "cases": {c: {"Ny": R.CASES[c][0], "Nx": R.CASES[c][1], "rms_px": R.CASES[c][2], "err": got[c]} for c in got}}, f, indent=1)
            f.write("\n")
    table = json.load(open(BUDGET))["cases"]
    assert set(table) == set(R.CASES)
    for c in got:
        for q in R.QUANTITIES:
            assert 1e-8 < table[c]["err"][q] < 1e-3, (c, q)           # single-precision rounding, nothing else
            assert 0.5 < got[c][q] / table[c]["err"][q] < 2.0, (c, q, got[c][q], table[c]["err"][q])
