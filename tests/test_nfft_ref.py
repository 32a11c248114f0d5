"""Pins tests/_nfft_ref.py, the restatement of the non-uniform-FFT method of the HEALPix projection, by properties: no reference output
exists (NFFT.jl is not available), so the definition is held to what characterises it and the window algorithm to the definition.  Also the
Python layer's method names, which need no device.

Bounds.  The direct sums are float64 sums of Ny Nx (or Npatch) terms of size <= Ny Nx each: the identities below hold to a few 1e-15 of the
natural scale (measured 3e-15 for the transposition, 2e-14 for the trigonometric polynomials); 1e-12 leaves room without letting a wrong
term through, which would show at 1e-3 or more.  The window algorithm in float64 is held to its entry of tests/golden/nfft_budget.json
(tools/make_nfft_budget.py: the largest of 16 draws) times the project's factor 3, here on draws of its own."""
import json
import os

import numpy as np
import pytest

import _healpix_ref as R
import _nfft_ref as N

BUDGET = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nfft_budget.json")))
CASES = list(N.CASES)


def _fields(P, seed, B=2, npol=3):
    g = np.random.default_rng(seed)
    return g.standard_normal((B, npol, P.cart.Nx, P.cart.Ny)), g.standard_normal((B, npol, P.npix))


@pytest.mark.parametrize("case", CASES)
def test_cases_are_what_the_budget_was_made_for(case):
    P = N.projector(case)
    assert P.npatch == BUDGET["cases"][case]["npatch"] > 0
    assert P.cut_margin() > 1e-9
    assert {k: BUDGET["cases"][case][k]["width"] for k in ("f32", "f64")} == N.WIDTH


def test_npatch_of_the_lambert_cases():
    assert [N.projector(c).npatch for c in ("n16_base", "n32_mixed", "n8_wrap")] == [218, 373, 26]


@pytest.mark.parametrize("case", CASES)
def test_transposition_identity(case):
    """Ny Nx dot(to_healpix(m), h) = Npatch dot(m, to_cart(h)) for I fields, by the definition"""
    P = N.projector(case)
    m, h = _fields(P, 11, npol=1)
    lhs = P.cart.Ny * P.cart.Nx * np.sum(P.direct_to_healpix(m) * h)
    rhs = P.npatch * np.sum(m * P.direct_to_cart(h))
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def _trig_poly(Ny, Nx, seed):
    """coefficients of a real trigonometric polynomial with |l| < N/2 on each axis; returns a function of the 1-based (i, j)"""
    g = np.random.default_rng(seed)
    ly, lx = np.meshgrid(np.arange(-(Ny // 2) + 1, Ny // 2), np.arange(-(Nx // 2) + 1, Nx // 2), indexing="ij")
    a, b = g.standard_normal(ly.shape), g.standard_normal(ly.shape)

    def f(i, j):
        y, x = (np.asarray(i, dtype=np.float64) - Ny // 2 - 1) / Ny, (np.asarray(j, dtype=np.float64) - Nx // 2 - 1) / Nx
        ph = 2 * np.pi * (ly[..., None] * y.ravel() + lx[..., None] * x.ravel())
        return (a[..., None] * np.cos(ph) + b[..., None] * np.sin(ph)).sum((0, 1)).reshape(y.shape)
    return f


@pytest.mark.parametrize("case", CASES)
def test_trigonometric_polynomials_are_reproduced(case):
    P = N.projector(case)
    Ny, Nx = P.cart.Ny, P.cart.Nx
    f = _trig_poly(Ny, Nx, 3)
    jj, ii = np.meshgrid(np.arange(1, Nx + 1), np.arange(1, Ny + 1), indexing="ij")
    m = f(ii, jj)[None, None]                                                # (1, 1, Nx, Ny)
    got = P.direct_to_healpix(m)[0, 0, P.hpx_idxs_in_patch]
    want = f(P.i_in, P.j_in)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    got = P.window_to_healpix(m)[0, 0, P.hpx_idxs_in_patch]
    assert np.linalg.norm(got - want) <= 3 * BUDGET["cases"][case]["f64"]["to_healpix"] * np.linalg.norm(want)


def test_a_node_on_a_grid_point_returns_that_pixel():
    Ny, Nx = 12, 16
    g = np.random.default_rng(5)
    m = g.standard_normal((Nx, Ny))
    i, j = np.array([1.0, 5.0, 12.0, 7.0]), np.array([1.0, 16.0, 9.0, 3.0])
    K = N.kernel_matrix(Ny, Nx, i, j)
    got = np.einsum("pxy,xy->p", K, m) / (Ny * Nx)
    want = m[j.astype(int) - 1, i.astype(int) - 1]
    assert np.max(np.abs(got - want)) <= 1e-12
    plan = N.Plan(Ny, Nx, i, j, np.float64)
    assert np.max(np.abs(plan.to_nodes(m) - want)) <= 3e-12                   # truncation 2e-13 relative, |m| up to 3


@pytest.mark.parametrize("case", CASES)
def test_exact_zeros_outside_the_patch(case):
    P = N.projector(case)
    m, _ = _fields(P, 2)
    outside = np.ones(P.npix, dtype=bool)
    outside[P.hpx_idxs_in_patch] = False
    for out in (P.direct_to_healpix(m), P.window_to_healpix(m), P.window_to_healpix(m, np.float32)):
        assert np.all(out[..., outside] == 0) and np.all(out[..., P.hpx_idxs_in_patch] != 0)


@pytest.mark.parametrize("case", CASES)
def test_qu_rotation_there_and_back(case):
    """the two rotations undo each other on the pixels of the patch, and I is not touched by either"""
    P = N.projector(case)
    g = np.random.default_rng(8)
    f = g.standard_normal((2, 3, P.npatch))
    back = R._rotate(R._rotate(f, P.psi_in, R.rot_to_healpix), P.psi_in, R.rot_to_cart)
    assert np.max(np.abs(back - f)) <= 1e-14 * np.max(np.abs(f)) * 4
    assert np.array_equal(R._rotate(f, P.psi_in, R.rot_to_healpix)[:, 0], f[:, 0])
    # ... and the projected QU planes are the rotated projections of Q and U taken as spin-0 fields (:327-335)
    m, _ = _fields(P, 9)
    full = P.direct_to_healpix(m)[..., P.hpx_idxs_in_patch]
    Q, U = (P.direct_to_healpix(m[:, k:k + 1])[:, 0][..., P.hpx_idxs_in_patch] for k in (1, 2))
    wantQ, wantU = R.rot_to_healpix(Q, U, P.psi_in)
    assert np.array_equal(full[:, 1], wantQ) and np.array_equal(full[:, 2], wantU)


@pytest.mark.parametrize("case", CASES)
def test_window_restatement_meets_its_budget(case):
    P = N.projector(case)
    m, h = _fields(P, 21, B=3)
    b = BUDGET["cases"][case]["f64"]
    eh = N.rel_planes(P.window_to_healpix(m), P.direct_to_healpix(m))
    ec = N.rel_planes(P.window_to_cart(h), P.direct_to_cart(h))
    print(case, "to_healpix", eh, "budget", b["to_healpix"], "to_cart", ec, "budget", b["to_cart"])
    assert np.all(eh <= max(3 * b["to_healpix"], 1e-12)) and np.all(ec <= max(3 * b["to_cart"], 1e-12))
    assert b["to_healpix"] < 1e-12 and b["to_cart"] < 1e-12                  # float64 width: truncation under 1e-12


def test_width_scan_of_the_budget_falls_as_designed():
    """the widths are chosen from this scan: truncation under the rounding floor of the precision (6e-8 / 1e-16 times the transforms' growth)"""
    w = {int(k): max(v.values()) for k, v in BUDGET["widths"].items()}
    assert all(w[a] > 10 * w[b] for a, b in ((6, 8), (8, 10), (10, 12), (12, 14)))
    assert w[N.WIDTH["f32"]] < 3e-7 and w[N.WIDTH["f64"]] < 3e-13


def test_plan_refuses_what_the_device_refuses():
    i = j = np.array([2.5])
    for Ny, Nx in ((7, 8), (8, 9), (2, 8)):
        with pytest.raises(ValueError):
            N.Plan(Ny, Nx, i, j)


def test_method_names_of_the_python_layer():
    """needs no device: "nfft" is accepted, "fft" is refused as before, anything else is a ValueError"""
    pytest.importorskip("torch")
    from cmblensing_jl_amd import healpix as H
    assert H._method("bilinear") == 0 and H._method("nfft") == 1
    with pytest.raises(NotImplementedError):
        H._method("fft")
    for bad in ("NFFT", "nearest", "", None):
        with pytest.raises(ValueError):
            H._method(bad)
