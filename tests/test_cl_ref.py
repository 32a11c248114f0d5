"""tests/_cl_ref.py -- the float64 restatement of the reference's get_Cℓ / get_ρℓ / cov_to_Cℓ that the GPU tests of cmbl_get_cl compare with -- pinned
WITHOUT the engine, by answers that use neither: the identity between the literal full-plane route and the λ-weighted half-plane route the library
runs, the closed form of a delta map, the edge rules against a brute-force loop, ρℓ(f, f) = 1, and what cov_to_Cℓ does to Cℓ_to_Cov."""
import numpy as np
import pytest

import _cl_ref as R

THETA = 2.0
SHAPES = [(16, 16), (15, 16), (16, 12)]                                   # (Ny, Nx): even and odd Ny, square / rectangular, Nx even


def planes(Ny, Nx, seed=0, n=2):
    """rffts of real maps, (n, Nx, Ny//2+1)"""
    return np.fft.rfft2(np.random.default_rng(seed).standard_normal((n, Nx, Ny)), axes=(-2, -1))


def tie_edges(L):
    """three edges that ARE ℓmag values of modes of the grid: lmag[ky=3, kx=0] < lmag[5, 0] < lmag[9, 0] (half planes are [x, ky])"""
    e = np.array([L[0, 3], L[0, 5], L[0, 9]]) if L.shape[1] > 9 else np.array([L[0, 3], L[0, 5], L[0, L.shape[1] - 1]])
    assert e[0] < e[1] < e[2]
    return e


@pytest.mark.parametrize("Ny,Nx", SHAPES)
@pytest.mark.parametrize("edges", ["default", "coarse", "tie"])
def test_literal_route_equals_the_half_plane_route(Ny, Nx, edges):
    """unfold -> strict mask -> left-closed histogram (the reference as written) against the λ-weighted half-plane sums, bin for bin.  Nx is even
    here: for an odd Nx the reference's unfold reads one past the row (n2 = n+3 under @inbounds), so only the Hermitian mirror it intends is
    defined there -- and the half-plane route IS that mirror."""
    F = planes(Ny, Nx)
    L = R.lmag(Ny, Nx, THETA)
    e = {"default": None, "coarse": np.array([10.0, 700.0, 1500.0, 1501.0, 4000.0, 9000.0]), "tie": tie_edges(L)}[edges]
    for F1, F2, fid in ((F[0], None, None), (F[0], F[1], None), (F[0], F[1], lambda l: 1 / l ** 2)):
        a = R.get_cl(F1, F2, L, Ny, THETA, ledges=e, Clfid=fid, route=R.sums_full)
        b = R.get_cl(F1, F2, L, Ny, THETA, ledges=e, Clfid=fid, route=R.sums_half)
        assert np.array_equal(a["count"], b["count"]) and a["count"].sum() > 0
        for k in ("A", "Sl", "S1", "S2"):
            scale = np.abs(a[k]).max()
            np.testing.assert_allclose(b[k], a[k], rtol=1e-13, atol=1e-13 * scale, err_msg=k)
        assert np.array_equal(np.isnan(a["cl"]), np.isnan(b["cl"]))


def test_hermitian_mirror_for_odd_nx():
    """odd Nx: the unfolded plane this file defines is the full FFT of the real map -- the mirror the reference intends"""
    for Ny, Nx in ((16, 15), (15, 9)):
        m = np.random.default_rng(3).standard_normal((Nx, Ny))
        np.testing.assert_allclose(R.unfold(np.fft.rfft2(m), Ny), np.fft.fft2(m), atol=1e-12)
    m = np.random.default_rng(4).standard_normal((16, 16))
    np.testing.assert_allclose(R.unfold(np.fft.rfft2(m), 16), np.fft.fft2(m), atol=1e-12)


@pytest.mark.parametrize("Ny,Nx", SHAPES + [(45, 75)])
def test_delta_map(Ny, Nx):
    """f = 1 at one pixel: |f_ℓ|² = 1 everywhere, so every populated bin has Cℓ = 1/α, ℓ = Sℓ/A and σℓ = 0 to rounding"""
    m = np.zeros((Nx, Ny))
    m[3, 5] = 1.0
    F = np.fft.rfft2(m)
    L = R.lmag(Ny, Nx, THETA)
    for fid in (None, lambda l: 1 / l ** 2):
        r = R.get_cl(F, None, L, Ny, THETA, Clfid=fid)
        ok = r["A"] > 0
        assert ok.any() and np.array_equal(ok, r["count"] > 0)
        np.testing.assert_allclose(r["cl"][ok], 1 / R.alpha(Ny, Nx, THETA), rtol=1e-13)
        np.testing.assert_array_equal(r["ell"][ok], r["Sl"][ok] / r["A"][ok])
        assert np.all(r["sigma"][ok] <= 1e-7 / R.alpha(Ny, Nx, THETA))            # sqrt of a difference of two numbers equal to 1e-16 relative
        assert np.all(np.isnan(r["cl"][~ok]))


def test_edge_rules():
    """edges that coincide with ℓmag values: the mode AT the first edge is out (strict >), the mode at the middle edge belongs to the UPPER bin
    (left-closed), the mode at the last edge is out (strict <); the counts equal a brute-force loop over the full plane"""
    Ny, Nx = 24, 20
    L = R.lmag(Ny, Nx, THETA)
    e = tie_edges(L)
    w = R.weight(L)
    one = lambda x, ky: (np.arange(Nx)[:, None] == x) & (np.arange(Ny // 2 + 1)[None, :] == ky)
    sums = lambda sel: R.sums_half(sel.astype(complex), sel.astype(complex), L, w, Ny, 1.0, e)
    # (S1 of an indicator field is λ·w of that mode in the bin it falls in; α = 1 here)
    assert sums(one(0, 3))[1].tolist() == [0, 0] and sums(one(0, 9))[1].tolist() == [0, 0]
    assert sums(one(0, 5))[1].tolist() == [0, 2 * w[0, 5]]                  # ky = 5 and its mirror -5: the UPPER bin
    assert sums(one(0, 4))[1].tolist() == [2 * w[0, 4], 0] and sums(one(0, 8))[1].tolist() == [0, 2 * w[0, 8]]
    # brute force over the full plane, mode by mode
    Lf = R.unfold(L, Ny)
    cnt = [0, 0]
    for x in range(Nx):
        for y in range(Ny):
            l = Lf[x, y]
            if not (l > e[0] and l < e[2]):
                continue
            cnt[0 if l < e[1] else 1] += 1
    got = R.get_cl(planes(Ny, Nx)[0], None, L, Ny, THETA, ledges=e)
    assert got["count"].tolist() == cnt
    assert R.get_cl(planes(Ny, Nx)[0], None, L, Ny, THETA, ledges=e, route=R.sums_full)["count"].tolist() == cnt
    # the default edges 0:50:16000 leave ℓ = 0 out
    r = R.get_cl(np.ones((Nx, Ny // 2 + 1)), None, L, Ny, THETA)
    assert r["count"].sum() == Nx * Ny - 1


@pytest.mark.parametrize("Ny,Nx", SHAPES)
def test_rho_of_a_field_with_itself_is_one(Ny, Nx):
    F = planes(Ny, Nx)
    L = R.lmag(Ny, Nx, THETA)
    ell, rho = R.get_rhol(F[0], F[0], L, Ny, THETA)
    ok = ~np.isnan(rho)
    assert ok.any()
    np.testing.assert_allclose(rho[ok], 1.0, rtol=1e-13)
    _, rho01 = R.get_rhol(F[0], F[1], L, Ny, THETA)
    assert np.all(np.abs(rho01[ok]) <= 1 + 1e-12) and np.abs(rho01[ok]).min() < 0.5       # Cauchy-Schwarz (1 is reached where a bin holds one real mode); independent maps decorrelate


def test_sigma_is_the_weighted_scatter():
    """σℓ = sqrt((S2/A − (S1/A)²)/N) with N = count/2; the reference's line 498 as written, S2/A − S1², is negative wherever A > 1"""
    Ny, Nx = 16, 16
    F = planes(Ny, Nx)[0]
    L = R.lmag(Ny, Nx, THETA)
    r = R.get_cl(F, None, L, Ny, THETA)
    ok = r["count"] > 2
    assert ok.any() and np.all(r["sigma"][ok] > 0) and np.all(r["sigma"][ok] < r["cl"][ok] * 3)
    assert np.all(r["S2"][ok] / r["A"][ok] - r["S1"][ok] ** 2 < 0)               # the quirk: sqrt of this throws
    b = int(np.flatnonzero(ok)[0])                                          # one bin by hand
    e = R.default_edges()
    sel = (L >= e[b]) & (L < e[b + 1]) & (L > 0)
    lw = (np.broadcast_to(R.lam(Ny)[None, :], L.shape) * R.weight(L))[sel]
    cl = (np.abs(F) ** 2)[sel] / R.alpha(Ny, Nx, THETA)
    mean = (lw * cl).sum() / lw.sum()
    var = (lw * cl ** 2).sum() / lw.sum() - mean ** 2
    np.testing.assert_allclose(r["sigma"][b], np.sqrt(var / (r["count"][b] / 2)), rtol=1e-12)


def test_cov_to_cl_is_not_the_inverse_of_cl_to_cov(capsys):
    """Cℓ_to_Cov divides Cℓ(ℓmag) by Ωpix = Δx² (src/proj_lambert.jl:362-364); cov_to_Cℓ is literally get_Cℓ(sqrt.(diag C))·sqrt(α) (:415-419), which
    gives Cℓ/(Ωpix·α)·sqrt(α) = Cℓ / (Δx·sqrt(Nx·Ny)): NOT the table back (that would need the factor Ωpix·α = Nx·Ny).  The ratio is recorded and
    pinned to that closed form; it is asserted to be 1 nowhere, because it is not."""
    for Ny, Nx in SHAPES:
        L = R.lmag(Ny, Nx, THETA)
        cl0 = 3.7e-5                                                        # a flat table: binning changes nothing
        diag = np.full(L.shape, cl0) / np.deg2rad(THETA / 60) ** 2
        ell, back = R.cov_to_cl(diag, L, Ny, THETA)
        ok = ~np.isnan(back)
        ratio = back[ok] / cl0
        want = 1 / (np.deg2rad(THETA / 60) * np.sqrt(Nx * Ny))
        print(f"cov_to_Cl(Cl_to_Cov(Cl)) / Cl at {Ny}x{Nx}, theta = {THETA}': {ratio[0]:.6g} (1 / (dx sqrt(Nx Ny)) = {want:.6g})")
        np.testing.assert_allclose(ratio, want, rtol=1e-12)
        assert abs(want - 1) > 0.5
