"""tests/_mask_ref.py -- the SciPy restatement of the reference's make_mask (src/masking.jl) that the GPU tests of cmbl_edt_sq and cmbl_make_mask
compare with -- pinned WITHOUT the engine: the distance transform against brute force, the closed form of the border profile, the flip
symmetries, the range, the taps of Kernel.gaussian and the unit conversion.  The last test is the one CPU-side statement about the product: the
two entry points are bound and declared."""
import os
import re

import numpy as np

import _mask_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_edt_against_brute_force():
    feat = np.zeros((31, 20), dtype=bool)                              # Ny = 20, Nx = 31
    for x, y in ((0, 0), (30, 19), (7, 3), (7, 4), (22, 11)):
        feat[x, y] = True
    d2 = R.edt_sq(feat)
    assert d2.dtype == np.int64 and np.array_equal(d2, R.edt_sq_brute(feat))
    assert d2[30, 0] == min(30 ** 2, 19 ** 2, 23 ** 2 + 3 ** 2, 8 ** 2 + 11 ** 2)
    assert np.array_equal(R.bleed(feat, 3), R.edt_sq_brute(feat) < 9)


def test_closed_form_without_rounding_and_sources():
    """on the centre row, away from the corners, pixel i >= pad is d = i - pad + 1 from the padding: mask = (1 - cos(min(d, w) / w pi)) / 2"""
    Ny, Nx, pad, w = 48, 64, 5, 9
    m = R.make_mask(Ny, Nx, np.zeros((0, 2), int), pad, w, 0, 0)
    assert m.dtype == np.float32 and m.shape == (Nx, Ny)
    i = np.arange(pad, Nx // 2)
    want = ((1 - np.cos(np.minimum(i - pad + 1, w) / w * np.pi)) / 2).astype(np.float32)
    assert np.array_equal(m[pad:Nx // 2, Ny // 2], want)
    j = np.arange(pad, Ny // 2)
    want = ((1 - np.cos(np.minimum(j - pad + 1, w) / w * np.pi)) / 2).astype(np.float32)
    assert np.array_equal(m[Nx // 2, pad:Ny // 2], want)
    assert not m[:pad].any() and not m[:, :pad].any() and not m[Nx - pad:].any() and not m[:, Ny - pad:].any()
    assert m[Nx // 2, Ny // 2] == 1


def test_flip_invariance_and_range():
    for Ny, Nx, pad, apod_w, round_w, src_w, nsrc in R.MASK_CASES:
        m = R.make_mask(Ny, Nx, np.zeros((0, 2), int), pad, apod_w, round_w, src_w)
        assert np.abs(m - m[::-1]).max() <= 2 ** -23 and np.abs(m - m[:, ::-1]).max() <= 2 ** -23     # the filter's sums are not mirrored: one float32 step
        if round_w == 0:
            assert np.array_equal(m, m[::-1]) and np.array_equal(m, m[:, ::-1])
        ms = R.make_mask(Ny, Nx, R.case_sources(Ny, Nx, nsrc), pad, apod_w, round_w, src_w)
        assert ms.min() >= 0 and ms.max() <= 1 and (ms <= m).all()
        frac = np.mean((ms > 0) & (ms < 1))
        assert frac > 0.2, frac                                           # a non-trivial mask at every shape of the GPU tests


def test_boolean_path_and_degenerate_padding():
    src = np.array([[3, 4], [3, 4], [0, 0], [19, 30]])                    # duplicates and corners, (y, x)
    m = R.make_mask(20, 31, src, 2, 0, 5, 3)
    assert set(np.unique(m)) <= {0.0, 1.0} and m[4, 3] == 0 and m[15, 10] == 1 and m[1, 10] == 0
    assert not R.make_mask(20, 31, src, 10, 4, 2, 3).any()                # 2 pad >= Ny: all zero
    assert not R.make_mask(20, 31, src, 10, 0, 0, 3).any()


def test_gaussian_taps():
    for s in (1, 3, 10, 20, 2.5):
        t = R.gaussian_taps(s)
        assert len(t) == 4 * int(np.ceil(s)) + 1 and abs(t.sum() - 1) < 1e-15
        assert np.array_equal(t, t[::-1]) and t.argmax() == len(t) // 2
        assert np.isclose(t[0] / t[len(t) // 2], np.exp(-(2 * np.ceil(s)) ** 2 / (2 * s * s)), rtol=1e-14)


def test_wide_filter_clamps_the_border():
    """41 taps on a 32-wide line: scipy's mode="nearest" is the index clamp of imfilter's "replicate" border"""
    rng = np.random.default_rng(0)
    d = rng.random((32, 5))
    taps = R.gaussian_taps(10)
    from scipy import ndimage
    got = ndimage.correlate1d(d, taps, axis=0, mode="nearest")
    idx = np.clip(np.arange(32)[:, None] + np.arange(-20, 21)[None, :], 0, 31)
    np.testing.assert_allclose(got, np.einsum("ikc,k->ic", d[idx], taps), rtol=1e-13)


def test_unit_conversion_rounds_half_to_even():
    assert R.deg2npix(1, 2.0) == 30 and R.deg2npix(1, 3.0) == 20 and R.deg2npix(2, 3.0) == 40 and R.arcmin2npix(7, 3.0) == 2
    assert R.arcmin2npix(7, 2.0) == 4 and R.arcmin2npix(5, 2.0) == 2 and R.arcmin2npix(3, 2.0) == 2       # 3.5 -> 4, 2.5 -> 2, 1.5 -> 2
    assert R.deg2npix(0.125, 3.0) == 2 and R.deg2npix(0.375, 3.0) == 8                                      # 2.5 -> 2, 7.5 -> 8
    assert R.default_num_ptsrcs(128, 128, 3.0) == 49 and R.default_num_ptsrcs(1024, 1024, 2.0) == 1398


def test_the_entry_points_are_bound_and_declared():
    from cmblensing_jl_amd import lib
    hdr = open(os.path.join(ROOT, "include", "cmblens.h")).read()
    for name, nargs in (("cmbl_edt_sq", 3), ("cmbl_make_mask", 8)):
        assert name in lib.SYMBOLS and len(lib.SIGNATURES[name]) == nargs
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and m.group(1).count(",") + 1 == nargs
