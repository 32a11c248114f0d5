"""tests/_udgrade_ref.py -- the float64 restatement of the reference's ud_grade that the GPU tests of cmbl_ud_grade compare with -- pinned
WITHOUT the engine, by answers that use neither: constants, reshape-means, the closed form of a band-limited field, the identity between
the literal three-transform sequence and the fused Fourier-space form the library runs, the Fourier mode's fac^2, the error cases."""
import os
import re

import numpy as np
import pytest

import _udgrade_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(24, 36, 2), (45, 30, 3), (32, 32, 4), (70, 70, 5)]           # (Ny, Nx, fac): even / odd targets, square / rectangular
THETA = 1.5


def field(Ny, Nx, seed=0, lead=(2,)):
    return np.random.default_rng(seed).standard_normal(lead + (Nx, Ny))


def band_limited(Ny, Nx, fac, seed=1, lead=(2,)):
    """a real field with power strictly below the Nyquist frequency of the grid coarser by `fac`"""
    F = R.rfft2(field(Ny, Nx, seed, lead)) * R.antialias_mask(Ny, Nx, Ny // fac, Nx // fac)
    return R.irfft2(F, Ny)


def as_map(res):
    arr, basis, Ny, Nx = res
    return arr if basis == "map" else R.irfft2(arr, Ny)


def as_fourier(res):
    arr, basis, Ny, Nx = res
    return arr if basis == "fourier" else R.rfft2(arr)


@pytest.mark.parametrize("Ny,Nx,fac", SHAPES)
def test_a_constant_map_stays_constant(Ny, Nx, fac):
    m = np.full((1, Nx, Ny), 2.5)
    for mode in ("map", "fourier"):
        for dc in (False, True):
            for aa in (False, True):
                got = as_map(R.ud_grade(m, "map", Ny, Nx, THETA, fac * THETA, mode, dc, aa))
                scale = fac ** 2 if mode == "fourier" else 1            # the Fourier mode's missing 1/fac^2
                assert got.shape == (1, Nx // fac, Ny // fac)
                np.testing.assert_allclose(got, 2.5 * scale, rtol=1e-12)
    up = R.ud_grade(m[..., :Nx // fac, :Ny // fac], "map", Ny // fac, Nx // fac, fac * THETA, THETA, "map", False, False)
    assert up[1:] == ("map", Ny, Nx)
    np.testing.assert_array_equal(up[0], m)


@pytest.mark.parametrize("Ny,Nx,fac", SHAPES)
def test_downgrade_of_upgrade_is_the_identity_and_the_mean_is_a_reshape_mean(Ny, Nx, fac):
    m = field(Ny // fac, Nx // fac, 3)
    up = R.ud_grade(m, "map", Ny // fac, Nx // fac, fac * THETA, THETA, "map", False, False)
    assert up[0][0, 1, 2] == m[0, 1 // fac, 2 // fac] and up[0][1, fac, 2 * fac] == m[1, 1, 2]
    back = R.ud_grade(up[0], "map", Ny, Nx, THETA, fac * THETA, "map", False, False)
    assert back[1:] == ("map", Ny // fac, Nx // fac)
    np.testing.assert_allclose(back[0], m, rtol=0, atol=1e-14)
    f = field(Ny, Nx, 4)
    want = np.array([[f[s, X * fac:(X + 1) * fac, Y * fac:(Y + 1) * fac].mean() for Y in range(Ny // fac)] for s in range(2) for X in range(Nx // fac)])
    got = R.ud_grade(f, "map", Ny, Nx, THETA, fac * THETA, "map", False, False)[0]
    np.testing.assert_allclose(got.reshape(want.shape), want, rtol=0, atol=1e-14)
    # a Fourier input goes through its map
    got_f = R.ud_grade(R.rfft2(f), "fourier", Ny, Nx, THETA, fac * THETA, "map", False, False)[0]
    np.testing.assert_allclose(got_f, got, rtol=0, atol=1e-13)


@pytest.mark.parametrize("Ny,Nx,fac", SHAPES)
def test_band_limited_closed_form(Ny, Nx, fac):
    """|D(k)| / fac is the pixel-window ratio identically, so the default downgrade (mean, then the deconvolution) of a field band-limited
    below the new Nyquist leaves only the half-pixel shift of the pixel centres: F_new[k] = F[k] / fac^2 * exp(iπ (fac-1) (ky/Ny + kx/Nx))"""
    m = band_limited(Ny, Nx, fac)
    Nyn, Nxn = Ny // fac, Nx // fac
    k = np.arange(-(max(Ny, Nx) // 2), max(Ny, Nx) // 2 + 1)
    for N in (Ny, Nx):                                                   # the identity itself, at every frequency below the new Nyquist
        kk = k[2 * np.abs(k) < N // fac]
        D = np.exp(2j * np.pi * np.outer(kk, np.arange(fac)) / N).sum(axis=1)
        np.testing.assert_allclose(np.abs(D) / fac, R.pixwin(fac * THETA, kk * 2 * np.pi / (N * np.deg2rad(THETA / 60))) / R.pixwin(THETA, kk * 2 * np.pi / (N * np.deg2rad(THETA / 60))), rtol=1e-13)
    ky, kx = R.kfreq(Nyn)[:Nyn // 2 + 1], R.kfreq(Nxn)
    want = R.truncate(R.rfft2(m), Nyn, Nxn) / fac ** 2 * np.exp(1j * np.pi * (fac - 1) * (ky[None, :] / Ny + kx[:, None] / Nx))
    for aa in (True, False):                                             # (nothing to alias: the filter changes nothing)
        got, basis, a, b = R.ud_grade(m, "map", Ny, Nx, THETA, fac * THETA, "map", True, aa)
        assert (basis, a, b) == ("fourier", Nyn, Nxn)
        assert np.linalg.norm(got - want) < 1e-12 * np.linalg.norm(want)


@pytest.mark.parametrize("Ny,Nx,fac", [(24, 36, 2), (45, 30, 3)] + SHAPES[2:])
@pytest.mark.parametrize("deconv", [True, False])
def test_fused_form_equals_the_literal_sequence(Ny, Nx, fac, deconv):
    f = field(Ny, Nx, 5)                                                 # full-band: the anti-aliasing filter does remove power
    want = as_fourier(R.ud_grade(f, "map", Ny, Nx, THETA, fac * THETA, "map", deconv, True))
    got = R.ud_grade_fused(R.rfft2(f), Ny, Nx, THETA, fac * THETA, deconv)
    assert got.shape == want.shape == (2, Nx // fac, Ny // fac // 2 + 1)
    assert np.linalg.norm(got - want) < 1e-12 * np.linalg.norm(want)
    # ... and the filter matters: without it the two differ
    alias = as_fourier(R.ud_grade(f, "map", Ny, Nx, THETA, fac * THETA, "map", deconv, False))
    assert np.linalg.norm(alias - want) > 1e-2 * np.linalg.norm(want)


@pytest.mark.parametrize("Ny,Nx,fac", SHAPES)
def test_fourier_mode_is_fac2_times_the_band_limited_map_mode(Ny, Nx, fac):
    """the reference's Fourier mode truncates the unnormalised half plane and does not rescale it: its map is fac^2 times too large, and it
    samples the field at the old pixel centres where the block mean samples it half a new pixel away"""
    m = band_limited(Ny, Nx, fac)
    Nyn, Nxn = Ny // fac, Nx // fac
    four = R.ud_grade(m, "map", Ny, Nx, THETA, fac * THETA, "fourier")
    assert four[1:] == ("fourier", Nyn, Nxn)
    mapm = as_fourier(R.ud_grade(m, "map", Ny, Nx, THETA, fac * THETA, "map"))
    ky, kx = R.kfreq(Nyn)[:Nyn // 2 + 1], R.kfreq(Nxn)
    shift = np.exp(1j * np.pi * (fac - 1) * (ky[None, :] / Ny + kx[:, None] / Nx))
    assert np.linalg.norm(four[0] * shift - fac ** 2 * mapm) < 1e-12 * np.linalg.norm(four[0])
    np.testing.assert_allclose(as_map(four)[:, 0, 0], fac ** 2 * m[:, 0, 0], rtol=1e-11)     # pixel (0, 0) keeps its centre


def test_truncation_keeps_the_new_grid_s_frequencies():
    for Ny, Nx, Nyn, Nxn in [(24, 36, 12, 18), (45, 30, 15, 10), (70, 70, 14, 14)]:
        ky, kx = R.kfreq(Ny)[:Ny // 2 + 1], R.kfreq(Nx)
        tag = (1000 * kx[:, None] + ky[None, :]).astype(complex)
        got = R.truncate(tag, Nyn, Nxn).real
        np.testing.assert_array_equal(got, 1000 * R.kfreq(Nxn)[:, None] + np.arange(Nyn // 2 + 1)[None, :])
        keep = R.antialias_mask(Ny, Nx, Nyn, Nxn)
        assert keep.sum() == (2 * ((Nxn - 1) // 2) + 1) * ((Nyn - 1) // 2 + 1)      # |k| < N_new / 2, strictly


def test_pixwin():
    ell = np.array([0.0, 100.0, 5400.0, 10800.0])
    np.testing.assert_allclose(R.pixwin(2.0, ell), [1.0, np.sin(100 * np.deg2rad(2 / 60) / 2) / (100 * np.deg2rad(2 / 60) / 2), 2 / np.pi, 0.0], atol=1e-15)
    pw = R.pixwin_plane(8, 6, 3.0)
    assert pw.shape == (6, 5) and pw[0, 0] == 1.0
    np.testing.assert_allclose(pw[3, 4], (2 / np.pi) ** 2, rtol=1e-14)   # both axes at Nyquist, whatever the pixel size


def test_error_cases_raise():
    m = field(24, 36)
    with pytest.raises(ValueError):
        R.ud_grade(m, "map", 24, 36, 1.0, 2.5)                           # not an integer step
    with pytest.raises(ValueError):
        R.ud_grade(m, "map", 24, 36, 1.0, 5.0)                           # integer, but 5 does not divide the sides
    with pytest.raises(ValueError):
        R.ud_grade(m, "map", 24, 36, 1.0, 2.0, mode="nearest")
    with pytest.raises(ValueError):
        R.ud_grade(m, "map", 24, 36, 2.0, 1.0)                           # upgrade with the default deconvolution
    with pytest.raises(ValueError):
        R.ud_grade(m, "map", 24, 36, 2.0, 1.0, mode="fourier")
    assert R.ud_grade(m, "map", 24, 36, 2.0, 2.0, mode="nearest")[0] is not None       # equal pixel size returns before the mode is looked at


def test_the_boundary_declares_ud_grade():
    """the C ABI, the ctypes binding, the Python host and the Julia glue all carry the new entry points (no GPU needed to see that)"""
    hdr = open(os.path.join(ROOT, "include", "cmblens.h"), encoding="utf-8").read()
    assert re.search(r"int cmbl_ud_grade\(cmbl_ctx\* src, cmbl_ctx\* dst, int mode, int deconv_pixwin, int anti_aliasing,\s*int basis_in, const void\* in, "
                     r"int basis_out, void\* out, int npol, int nbatch\);", hdr)
    assert "int cmbl_pixwin_host(cmbl_ctx* ctx, double* out_host, size_t n);" in hdr and "enum { CMBL_UD_MAP = 0, CMBL_UD_FOURIER = 1 };" in hdr
    from cmblensing_jl_amd.lib import SYMBOLS
    assert {"cmbl_ud_grade", "cmbl_pixwin_host"} <= set(SYMBOLS)
    import cmblensing_jl_amd as C
    assert callable(C.ud_grade) and (C.UD_MAP, C.UD_FOURIER) == (0, 1)
    np.testing.assert_allclose(C.pixwin(2.0, [0.0, 5400.0]), R.pixwin(2.0, [0.0, 5400.0]), rtol=1e-15)
    jl = open(os.path.join(ROOT, "julia", "CMBLensingHIPExt.jl"), encoding="utf-8").read()
    assert "ccall((:cmbl_ud_grade, lib)" in jl
