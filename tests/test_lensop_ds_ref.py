"""Pins tests/_lensop_ds_ref.py (the oracle's data set with BilinearLens / PowerLens / Taylens in its L slot) by properties, on the CPU: the normal
operator of the Wiener filter is symmetric, ∇f vanishes at the converged filter, δϕ of gradientphi_logpdf is _bilinear_ref's pullback fed by hand,
and the conjugate gradient takes the iteration counts recorded for this construction.  (The ϕ-gradient is NOT tested against finite differences:
the bilinear pullback uses the spectral gradient of f~ and is not the derivative of a piecewise-bilinear map; the reference's own test gives it
atol = 300.)"""
import numpy as np
import pytest

import oracle as O
import _bilinear_ref as BR
import _lensop_ds_ref as R


def _plain(Nside, pol, mask, kind="BilinearLens", order=None):
    """the construction the iteration counts were recorded with: oracle.load_sim as it is (θ = 3', beam 3', border mask 0.4° / 0.4°, one slot),
    float64, the operator swapped in, the data as simulated"""
    so = O.load_sim(3.0, Nside, pol, np.float64, beam_fwhm=3.0, pixel_mask=R.PM if mask else None, Nbatch=1)
    return R.LensOpDataSet.of(so["ds"], kind, order=order), so


@pytest.mark.parametrize("kind,order", [("BilinearLens", None), ("PowerLens", 4)])
def test_normal_operator_is_symmetric(kind, order):
    ds, so = _plain((64, 128), "P", True, kind, order)
    L = ds.L(so["phi"])
    zero = np.zeros_like(so["d"])
    A = lambda f: -ds.gradientf_logpdf(f, L, zero)
    rng = np.random.default_rng(3)
    a, b = (ds.Cf.sqrt()(O.rfft2(rng.standard_normal((1, 2, 128, 64)))) for _ in range(2))
    lhs, rhs = ds.dot(a, A(b)), ds.dot(A(a), b)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
    assert ds.dot(a, A(a)) > 0


def test_gradientf_vanishes_at_the_converged_wiener_filter():
    ds, so = _plain((32, 32), "P", False)
    fw, hist = ds.argmaxf_logpdf(so["phi"], tol=1e-12, nsteps=200)
    g = ds.gradientf_logpdf(fw, ds.L(so["phi"]), ds.d)
    b = ds.gradientf_logpdf(np.zeros_like(fw), ds.L(so["phi"]), ds.d)
    assert np.sqrt(ds.dot(g, g) / ds.dot(b, b)) < 1e-5, len(hist)


def test_gradientphi_is_the_pullback_fed_by_hand():
    ds, so = _plain((64, 128), "P", True)
    proj, f, phi, d = ds.proj, so["f"], so["phi"], so["d"]
    got = ds.gradientphi_logpdf(f, phi, d)
    Lb = BR.BilinearLens(64, 128, 3.0, np.float64, phi=O.irfft2(phi[0, 0], 64))
    ftil = Lb.mul(O.from_harm(proj, f))
    z = ds.M(ds.B(O.to_harm(proj, ftil))) - d
    delta = O.irfft2(O.harm_to_qu(proj, -ds.B.T_()(ds.Mt(ds.Cn.pinv()(z)))), 64)
    dphi, _ = Lb.pullback(ftil, delta)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = dphi - O.nan2zero(phi / ds.Cphi)
    assert BR.rel(got, want) < 1e-13


# (Nside, pol, mask) -> iterations to tol = 1e-1 of this construction on the CPU, float64 (LenseFlow takes 29 on the first).  The two long solves
# were recorded for "36 x 60 I, mask" and "32 x 64 IP, mask" without the mask's parameters: a border mask of 0.3 deg / 0.35 deg gives them (163, 173);
# the 0.4 deg / 0.4 deg mask of the first row gives 186 and 157 there.
PM2 = dict(pad_deg=0.3, apod_deg=0.35)
ITERS = [((64, 128), "P", R.PM, 27), ((32, 32), "P", None, 5), ((4096, 32), "P", None, 7), ((36, 60), "I", PM2, 164), ((32, 64), "IP", PM2, 172)]


@pytest.mark.parametrize("Nside,pol,mask,want", ITERS)
def test_wiener_filter_iteration_counts(Nside, pol, mask, want):
    so = O.load_sim(3.0, Nside, pol, np.float64, beam_fwhm=3.0, pixel_mask=mask, Nbatch=1)
    ds = R.LensOpDataSet.of(so["ds"], "BilinearLens")
    _, hist = ds.argmaxf_logpdf(so["phi"], tol=1e-1, nsteps=500)
    assert abs(len(hist) - want) <= 1, len(hist)


def test_taylens_has_a_mean_and_nothing_else():
    ds, so = _plain((32, 32), "P", False, "Taylens", 3)
    L = ds.L(so["phi"])
    assert np.all(np.isfinite(ds.mean(L, so["f"])))
    with pytest.raises(NotImplementedError):
        ds.gradientf_logpdf(so["f"], L, so["d"])
    with pytest.raises(NotImplementedError):
        ds.gradientphi_logpdf(so["f"], so["phi"], so["d"])
