"""Pins tests/_healpix_ref.py, the NumPy restatement of the HEALPix projection (src/proj_healpix.jl), by properties: the reference has no
tests for that file, and neither Healpix.jl nor healpy is at hand.  CPU only.  The import of cmblensing_jl_amd.healpix below ties the file to
the feature (the Python layer's own argument checks are exercised here too, without a device)."""
import numpy as np
import pytest

import _healpix_ref as R

NSIDES = [1, 2, 4, 8, 16, 32, 64]
ROTATORS = [(0, 90, 0), (0, 30, 0), (40, -20, 10), (0, 0, 0), (0, 180, 0)]
PI = np.pi


def rng(seed):
    return np.random.default_rng(seed)


def sphere_points(n, seed):
    g = rng(seed)
    return np.arccos(g.uniform(-1, 1, n)), g.uniform(-PI, PI, n)


# ---- the Python layer's host-side checks (no device needed) ---------------------------------------------------------------------------
def test_python_layer_argument_checks():
    from cmblensing_jl_amd import healpix as H
    assert H.ProjHealpix(16).npix == 3072 and H.ProjHealpix(16) == H.ProjHealpix(16)
    for bad in (0, 3, 12, 16384, 2.5):
        with pytest.raises(ValueError):
            H.ProjHealpix(bad)
    f = H.HealpixMap(np.zeros(12 * 8 * 8))
    assert f.Nside == 8 and f.basis == "I" and tuple(f.arr.shape) == (1, 1, 768)
    with pytest.raises(ValueError):
        H.HealpixMap(np.zeros(100))
    with pytest.raises(ValueError):
        H.HealpixField(H.ProjHealpix(2), np.zeros((3, 48)), "QU")
    a = rng(0).standard_normal((2, 3, 48))
    f = H.HealpixField(H.ProjHealpix(2), a, "IQU")
    assert np.isclose(f.dot(f), (a * a).sum())
    assert np.array_equal(f.I.arr.numpy(), a[:, :1]) and np.array_equal(f.Q.arr.numpy(), a[:, 1:2]) and np.array_equal(f.U.arr.numpy(), a[:, 2:])
    assert f.P.basis == "QU" and np.array_equal(f["P"].arr.numpy(), a[:, 1:])
    with pytest.raises(ValueError):
        f.dot(H.HealpixField(H.ProjHealpix(1), np.zeros((2, 3, 12)), "IQU"))
    with pytest.raises(NotImplementedError, match="out"):
        H.project(f, None, method="fft")
    with pytest.raises(NotImplementedError):
        H.Projector(H.ProjHealpix(2), None, method="fft")


def test_pix2ang_host_entry_point_matches_the_restatement():
    from cmblensing_jl_amd import healpix as H
    for nside in (1, 2, 8, 64):
        th, ph = H.pix2ang_ring(nside)
        rt, rp = R.pix2ang(nside)
        assert np.max(np.abs(th - rt)) < 1e-14 and np.max(np.abs(ph - rp)) < 1e-14
    th, ph = H.pix2ang_ring(4, [0, 5, 191])
    assert np.allclose(th, R.pix2ang(4, [0, 5, 191])[0], atol=1e-14)


# ---- pix2ang ------------------------------------------------------------------------------------------------------------------------------
def test_pix2ang_nside1_exact():
    th, ph = R.pix2ang(1)
    want_th = np.repeat([np.arccos(2 / 3), PI / 2, PI - np.arccos(2 / 3)], 4)
    want_ph = np.concatenate([PI / 4 + np.arange(4) * PI / 2, np.arange(4) * PI / 2, PI / 4 + np.arange(4) * PI / 2])
    ulp = np.spacing(PI)                                                                # one ulp at the largest angle: acos(-2/3) against π - acos(2/3)
    assert np.max(np.abs(th - want_th)) <= ulp and np.max(np.abs(ph - want_ph)) <= ulp


@pytest.mark.parametrize("nside", NSIDES)
def test_pix2ang_properties(nside):
    th, ph = R.pix2ang(nside)
    npix = 12 * nside * nside
    v = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    assert np.max(np.abs(v.sum(axis=1))) < 1e-12 * npix
    r = np.arange(1, 4 * nside)
    sp, nr, rth, _ = R.ring_info(nside, r)
    assert sp[0] == 0 and np.array_equal(sp[1:], np.cumsum(nr)[:-1]) and sp[-1] + nr[-1] == npix
    for k in range(r.size):
        sl = slice(sp[k], sp[k] + nr[k])
        assert np.max(np.abs(np.cos(th[sl]) - R.ring_z(nside, r[k]))) < 1e-15          # ring z against the closed forms
        assert np.all(th[sl] == rth[k])                                                 # pix2ang and the interpolation agree on the ring
        assert np.all(np.diff(ph[sl]) > 0) and ph[sl][0] >= 0 and ph[sl][-1] < 2 * PI   # ϕ ascends inside a ring
    assert np.all(np.diff(rth) > 0)


# ---- ring interpolation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nside", NSIDES)
def test_interp_weights_and_exactness(nside):
    npix = 12 * nside * nside
    th, ph = sphere_points(4000, nside)
    th[:4] = [0.0, PI, 1e-12, PI - 1e-12]
    pix, w = R.interp_weights(nside, th, ph)
    assert np.all(w >= 0) and np.max(np.abs(w.sum(axis=0) - 1)) < 1e-14
    assert pix.min() >= 0 and pix.max() < npix
    m = rng(100 + nside).standard_normal(npix)
    cth, cph = R.pix2ang(nside)
    assert np.max(np.abs(R.interp_val(m, cth, cph) - m)) < 1e-12                      # at every pixel centre: that pixel's value
    assert np.max(np.abs(R.interp_val(m, cth, cph - 2 * PI) - m)) < 1e-12             # ... also with ϕ from an atan
    assert np.max(np.abs(R.interp_val(np.full(npix, 2.5), th, ph) - 2.5)) < 1e-14
    _, _, rth, _ = R.ring_info(nside, np.array([1, 4 * nside - 1]))
    mid = (th >= rth[0]) & (th <= rth[1])
    assert mid.sum() > 100
    assert np.max(np.abs(R.interp_val(cth, th[mid], ph[mid]) - th[mid])) < 1e-12      # map_k = θ_k is reproduced between the first and last ring
    with pytest.raises(ValueError):
        R.interp_weights(nside, [-1e-3], [0.0])
    with pytest.raises(ValueError):
        R.interp_weights(nside, [PI + 1e-3], [0.0])


@pytest.mark.parametrize("nside", NSIDES)
def test_interp_is_continuous_across_every_case_boundary(nside):
    npix = 12 * nside * nside
    m = rng(200 + nside).standard_normal(npix)
    eps, g = 1e-9, rng(300 + nside)
    bound = 1e-6 * np.max(np.abs(m))

    def jump(th, ph, dth, dph):
        return np.max(np.abs(R.interp_val(m, np.clip(th + dth, 0, PI), ph + dph) - R.interp_val(m, np.clip(th - dth, 0, PI), ph - dph)))

    _, _, rth, _ = R.ring_info(nside, np.arange(1, 4 * nside))
    nper = 8
    ths = np.repeat(rth, nper)                                                          # ring colatitudes (the first and the last ring included)
    assert jump(ths, g.uniform(-PI, PI, ths.size), eps, 0) < bound
    zb = np.repeat([np.arccos(2 / 3), np.arccos(-2 / 3)], 64)                           # |z| = 2/3
    assert jump(zb, g.uniform(-PI, PI, zb.size), eps, 0) < bound
    th = np.arccos(g.uniform(-1, 1, 512))
    assert jump(th, np.zeros(512), 0, eps) < bound                                      # ϕ = 0
    assert jump(th, np.full(512, 2 * PI), 0, eps) < bound
    cth, cph = R.pix2ang(nside)                                                         # a pixel centre's ϕ, on its own ring and between rings
    k = g.integers(0, npix, 512)
    assert jump(cth[k], cph[k], 0, eps) < bound
    assert jump(np.clip(cth[k] + g.uniform(-0.3, 0.3, 512) / nside, 0, PI), cph[k], 0, eps) < bound
    pole = np.repeat([0.0, PI], 32)                                                     # across the poles themselves
    ph = g.uniform(-PI, PI, 64)
    assert np.max(np.abs(R.interp_val(m, np.abs(pole - eps), ph) - R.interp_val(m, np.abs(pole - eps), ph + PI))) < bound


# ---- ij <-> θϕ ------------------------------------------------------------------------------------------------------------------------------------
def carts():
    out = [R.Lambert(48, 64, 30.0, rot) for rot in ROTATORS]
    out.append(R.Lambert(33, 20, 120.0, (40, -20, 10)))
    out.append(R.EquiRect(24, 32, (0.9, 1.7), (-0.5, 0.6)))                             # a φ-span crossing 0
    return out


@pytest.mark.parametrize("k", range(7))
def test_ij_angle_maps_are_inverse(k):
    c = carts()[k]
    g = rng(400 + k)
    i, j = g.uniform(0, c.Ny + 1, 2000), g.uniform(0, c.Nx + 1, 2000)
    th, ph = c.ij_to_ang(i, j)
    assert np.all((th >= 0) & (th <= PI))
    i2, j2 = c.ang_to_ij(th, ph)
    assert np.max(np.abs(i2 - i)) < 1e-9 and np.max(np.abs(j2 - j)) < 1e-9
    th2, ph2 = c.ij_to_ang(i2, j2)
    assert np.max(np.abs(th2 - th)) < 1e-12
    assert np.max(np.abs(np.angle(np.exp(1j * (ph2 - ph))))) < 1e-9


def test_centre_of_the_default_patch():
    for Ny, Nx in ((48, 64), (33, 20)):
        th, ph = R.Lambert(Ny, Nx, 30.0).ij_to_ang(Ny // 2 + 0.5, Nx // 2 + 0.5)
        assert abs(th - PI / 2) < 1e-15 and abs(ph) < 1e-15


def test_lambert_orientation_matches_the_reference_formulas():
    """θϕ_to_ij as the reference writes it (:101-112): rotate, r = 2 cos(θ'/2), x = -r sin ϕ', y = -r cos ϕ', i <-> y, j <-> x"""
    for rot in ROTATORS:
        c = R.Lambert(48, 64, 30.0, rot)
        th, ph = c.ij_to_ang(*np.meshgrid(np.arange(1.0, 49), np.arange(1.0, 65)))
        n = np.stack([np.cos(ph) * np.sin(th), np.sin(ph) * np.sin(th), np.cos(th)])
        w = np.einsum("ab,b...->a...", R.rotzyx(rot), n)
        el, az = np.arctan2(w[2], np.hypot(w[0], w[1])), np.arctan2(w[1], w[0])
        r = 2 * np.cos((PI / 2 - el) / 2)
        i, j = c.ang_to_ij(th, ph)
        assert np.max(np.abs(-r * np.cos(az) / c.dx + 48 // 2 + 0.5 - i)) < 1e-9
        assert np.max(np.abs(-r * np.sin(az) / c.dx + 64 // 2 + 0.5 - j)) < 1e-9


@pytest.mark.parametrize("k", range(6))
def test_psi_against_central_differences(k):
    c = carts()[k]
    g = rng(500 + k)
    th, ph = c.ij_to_ang(g.uniform(1, c.Ny, 500), g.uniform(1, c.Nx, 500))
    h = 1e-6
    J11, J21 = ((a - b) / (2 * h) for a, b in zip(c.ang_to_ij(th + h, ph), c.ang_to_ij(th - h, ph)))
    J12, J22 = ((a - b) / (2 * h) for a, b in zip(c.ang_to_ij(th, ph + h), c.ang_to_ij(th, ph - h)))
    fd = 0.5 * (np.arctan2(J11, J21) + np.arctan2(-J22, J12) - PI)
    d = c.psi(th, ph) - fd
    assert np.max(np.abs(np.angle(np.exp(2j * d)) / 2)) < 1e-6                          # ψ is an angle of a spin-2 rotation: compared modulo π


# ---- flat bilinear ----------------------------------------------------------------------------------------------------------------------------------
def test_flat_bilinear():
    img = rng(6).standard_normal((5, 7))                                                # (Nx, Ny)
    jj, ii = np.meshgrid(np.arange(1.0, 6), np.arange(1.0, 8), indexing="ij")
    assert np.array_equal(R.flat_bilinear(img, ii, jj), img)
    assert np.allclose(R.flat_bilinear(img, np.full(5, 0.5), np.arange(1.0, 6)), 0.5 * img[:, 0], atol=1e-15)
    assert np.all(R.flat_bilinear(img, np.array([0.0, -0.3, 8.0, 3.0, 3.0]), np.array([2.0, 2.0, 2.0, 0.0, 6.0])) == 0)
    assert np.isclose(R.flat_bilinear(img, np.array([2.25]), np.array([3.5]))[0],
                      0.75 * 0.5 * img[2, 1] + 0.25 * 0.5 * img[2, 2] + 0.75 * 0.5 * img[3, 1] + 0.25 * 0.5 * img[3, 2])


# ---- round trip ----------------------------------------------------------------------------------------------------------------------------------------
def test_dipole_round_trip():
    """f = a·n̂ on Nside 64 -> a 48 x 64 patch of 30' pixels -> back.  Linear interpolation of f between samples h apart errs by at most
    h^2/8 max|f''| per axis; along any great-circle direction |f''| <= |a|.  Sphere -> patch: the four pixels lie within one ring spacing in θ
    (<= hθ) and one pixel spacing in ϕ along the ring (arc <= hϕ); both are below 1.2 sqrt(4π / npix) ... taken as 2 sqrt(4π / npix) to cover the
    polar-cap rings, plus the cross term of the same size: bound 3 * (2 sqrt(4π/npix))^2 / 8 |a|.  Patch -> sphere: bilinear on a grid of
    spacing Δx (the Lambert map stretches lengths by at most 1/cos(r/2) ~ 1.02 here): 2 (1.05 Δx)^2 / 8 |a| for the interpolation of the exact
    patch values, plus the first leg's error carried through (the weights sum to 1).  The bounds are recorded in the assertion messages."""
    nside, a = 64, np.array([0.3, -0.5, 0.8])
    th, ph = R.pix2ang(nside)
    f = a @ np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    c = R.Lambert(48, 64, 30.0)
    P = R.Projector(nside, c)
    exact = a @ np.stack([np.sin(P.thetas) * np.cos(P.phis), np.sin(P.thetas) * np.sin(P.phis), np.cos(P.thetas)])
    hs = 2 * np.sqrt(4 * PI / (12 * nside * nside))
    b1 = 3 * hs ** 2 / 8 * np.linalg.norm(a)
    m = P.to_cart(f[None, None])
    e1 = np.max(np.abs(m.ravel() - exact))
    assert e1 < b1, (e1, b1)
    b2 = b1 + 2 * (1.05 * c.dx) ** 2 / 8 * np.linalg.norm(a)
    back = P.to_healpix(m)[0, 0]
    e2 = np.max(np.abs(back[P.hpx_idxs_in_patch] - f[P.hpx_idxs_in_patch]))
    assert e2 < b2, (e2, b2)
    assert e1 > 1e-3 * b1 and e2 > 1e-3 * b2                                           # the bounds are of the right order, not vacuous
    outside = np.setdiff1d(np.arange(f.size), P.touched)
    assert np.all(back[outside] == 0) and P.hpx_idxs_in_patch.size > 0 and np.all(np.isin(P.hpx_idxs_in_patch, P.touched))


# ---- QU ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_qu_rotations():
    g = rng(7)
    Q, U, psi = g.standard_normal(50), g.standard_normal(50), g.uniform(-PI, PI, 50)
    Q2, U2 = R.rot_to_healpix(*R.rot_to_cart(Q, U, psi), psi)
    assert np.max(np.abs(Q2 - Q)) < 1e-15 and np.max(np.abs(U2 - U)) < 1e-15
    # one pixel by hand, ψ = 15°: cos 2ψ = √3/2, sin 2ψ = 1/2; (Q, U) = (2, 4)
    c, s = np.sqrt(3) / 2, 0.5
    assert np.allclose(R.rot_to_cart(2.0, 4.0, np.deg2rad(15)), (2 * c - 4 * s, 4 * c + 2 * s), atol=1e-15)       # :243-244
    assert np.allclose(R.rot_to_healpix(2.0, 4.0, np.deg2rad(15)), (2 * c + 4 * s, 4 * c - 2 * s), atol=1e-15)    # :332-333
    # the projections apply them to the last two planes only
    P = R.Projector(4, R.Lambert(33, 20, 120.0, (40, -20, 10)))
    h = g.standard_normal((2, 3, 192))
    m = P.to_cart(h)
    raw = R.interp_val(h, P.thetas, P.phis)
    assert np.array_equal(m[:, 0].reshape(2, -1), raw[:, 0])
    assert np.allclose(m[:, 1].reshape(2, -1), raw[:, 1] * np.cos(2 * P.psi_cart) - raw[:, 2] * np.sin(2 * P.psi_cart), atol=1e-15)
