"""The HEALPix projection on the device (cmbl_projector_*, cmbl_project_*) against tests/_healpix_ref.py, the float64 NumPy restatement of
src/proj_healpix.jl (pinned on its own by tests/test_healpix_ref.py), on identical inputs, in both context precisions.

Cases (every one with npol 1, 2, 3 and nbatch 1, 3): Nside 1 and 2 on a 16 x 24 patch of 400' pixels, rotator (0, 90, 0) [*]; Nside 4 on
33 x 20 (odd Ny), 120', (40, -20, 10); Nside 16 on 64 x 48, 30', with (0, 90, 0) (crosses ϕ = 0), (0, 0, 0) (south-cap branch) and
(0, 180, 0) (north-cap branch); Nside 64 on 48 x 64, 10', (0, 30, 0); Nside 16 on a ProjEquiRect 24 x 32 whose φ-span crosses 0.
[*] the issue that introduced the feature asked for 600' pixels there; a 16 x 24 Lambert patch of 600' pixels reaches r = |x| > 2, where
θ = 2 acos(r/2) does not exist (the reference throws): 400' is the largest round size that fits, and the 600' patch is tested as an error.

Tolerances, DERIVED (max|f| = the largest input magnitude).  Projected VALUES are compared, not index tables: the interpolant is continuous
across every case boundary of the ring lookup, so a one-ulp disagreement about a floor changes which four pixels are read but not the value.
  float64: 1e-12 max|f| -- a few ulp of angle error times the 4 Nside / 2π gain of a weight stays below 1e-13 at Nside <= 64.
  float32: the geometry is shared and double, so the errors are the rounding of four weights and four multiply-adds: 8 * 2^-24 max|f|; the QU
  planes add the rotation's two more roundings of each of two terms: 12 * 2^-24 max|f|.
  θ, ϕ, ψ, is, js: 1e-12 in both precisions (ϕ compared modulo 2π and ψ modulo π: they are an azimuth and the angle of a spin-2 rotation, each
  taken from an atan whose branch cut an ulp can cross).
  hpx_idxs_in_patch and the touched list: exactly equal and ascending; the test asserts the condition for that, that no HEALPix centre of the
  restatement lies within 1e-9 pixel of a line the sets are cut on.
Measured on MI355X: profiles/healpix_parity.txt (CMBL_PARITY_LOG)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _healpix_ref as R
import _tol

DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
U32 = 2.0 ** -24
ERR_ARG, ERR_SHAPE = 1, 2
EQ_SPANS = ((0.9, 1.7), (-0.5, 0.6))

# name: (Nside, Ny, Nx, theta_pix or None for ProjEquiRect, rotator)
CASES = {
    "n1": (1, 16, 24, 400.0, (0, 90, 0)),
    "n2": (2, 16, 24, 400.0, (0, 90, 0)),
    "n4_odd": (4, 33, 20, 120.0, (40, -20, 10)),
    "n16_phi0": (16, 64, 48, 30.0, (0, 90, 0)),
    "n16_south": (16, 64, 48, 30.0, (0, 0, 0)),
    "n16_north": (16, 64, 48, 30.0, (0, 180, 0)),
    "n64": (64, 48, 64, 10.0, (0, 30, 0)),
    "n16_equirect": (16, 24, 32, None, None),
}


def _pkg():
    import cmblensing_jl_amd as C
    return C


_ref, _dev = {}, {}


def ref(case):
    """the restatement's Projector of a case: computed once, shared, never modified"""
    if case not in _ref:
        nside, Ny, Nx, theta, rot = CASES[case]
        with np.errstate(all="ignore"):                                      # a HEALPix centre at the patch's antipode maps to infinity
            _ref[case] = R.Projector(nside, R.EquiRect(Ny, Nx, *EQ_SPANS) if theta is None else R.Lambert(Ny, Nx, theta, rot))
    return _ref[case]


def dev(case, prec):
    """(cart_proj, Projector) on the device"""
    k = (case, prec)
    if k not in _dev:
        C = _pkg()
        nside, Ny, Nx, theta, rot = CASES[case]
        p = C.ProjEquiRect(Ny, Nx, *EQ_SPANS, T=DT[prec][0]) if theta is None else C.ProjLambert(Ny, Nx, theta, DT[prec][0], rotator=rot)
        _dev[k] = (p, C.Projector(C.ProjHealpix(nside), p))
    return _dev[k]


def cart_field(p, arr):
    C = _pkg()
    eq = isinstance(p, C.ProjEquiRect) and arr.shape[1] < 3               # EquiRectField is spin 0 or 2; IQU on a ProjEquiRect is a plain MAP Field
    return C.EquiRectField(p, arr, C.MAP) if eq else C.Field(p, p.tensor(arr), C.MAP)


def basis_of(npol):
    return {1: "I", 2: "QU", 3: "IQU"}[npol]


def check_values(what, got, want, fmax, prec, npol):
    """max |got - want| per plane against the derived bound; logged"""
    for k in range(npol):
        pol = npol >= 2 and k >= npol - 2
        tol = 1e-12 * fmax if prec == "f64" else (12 if pol else 8) * U32 * fmax
        err = float(np.max(np.abs(got[:, k].astype(np.float64) - want[:, k])))
        _tol._record(_tol._key(f"{what} plane {k}"), err, tol)
        print(f"{what} plane {k}: max error {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (what, k, err, tol)


@pytest.mark.parametrize("case", list(CASES))
def test_cut_lines_are_clear_in_the_restatement(case):
    """the condition under which the two pixel lists can be compared exactly"""
    assert ref(case).cut_margin() > 1e-9
    assert ref(case).touched.size > 0


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_geometry_and_lists(case, prec):
    r = ref(case)
    _, P = dev(case, prec)
    assert r.cut_margin() > 1e-9
    assert np.array_equal(P.hpx_idxs_in_patch, r.hpx_idxs_in_patch) and np.all(np.diff(P.hpx_idxs_in_patch) > 0)
    assert np.array_equal(P.touched, r.touched) and np.all(np.diff(P.touched) > 0)
    assert (P.n_in_patch, P.n_touched) == (r.hpx_idxs_in_patch.size, r.touched.size)
    wrap = lambda d, period: np.abs((d + period / 2) % period - period / 2)
    for name, got, want, period in (("theta", P.thetas, r.thetas, None), ("phi", P.phis, r.phis, 2 * np.pi), ("psi_cart", P.psi_cart, r.psi_cart, np.pi),
                                    ("is", P.is_, r.is_, None), ("js", P.js, r.js, None), ("psi_hpx", P.psi_hpx, r.psi_hpx, np.pi)):
        d = got - want
        err = float(np.max(np.abs(d) if period is None else wrap(d, period)))
        _tol._record(_tol._key(f"{case} {prec} {name}"), err, 1e-12)
        print(f"{case} {prec} {name}: max error {err:.3e}")
        assert err <= 1e-12, (name, err)


@pytest.mark.parametrize("nbatch", [1, 3])
@pytest.mark.parametrize("npol", [1, 2, 3])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_project_both_directions(case, prec, npol, nbatch):
    C = _pkg()
    r = ref(case)
    p, P = dev(case, prec)
    g = np.random.default_rng(1000 * npol + nbatch)
    # sphere -> patch
    h = g.standard_normal((nbatch, npol, r.npix)).astype(DT[prec][1])
    f = C.project(C.HealpixField(P.hpx_proj, h, basis_of(npol)), p, projector=P)
    got = f.arr.cpu().numpy()
    assert got.shape == (nbatch, npol, p.Nx, p.Ny) and got.dtype == DT[prec][1]
    check_values(f"{case} {prec} to_cart", got, r.to_cart(h), float(np.max(np.abs(h))), prec, npol)
    again = C.project(C.HealpixField(P.hpx_proj, h, basis_of(npol)), p, projector=P).arr.cpu().numpy()
    assert np.array_equal(got, again)                                        # bit-identical between runs
    # patch -> sphere
    m = g.standard_normal((nbatch, npol, p.Nx, p.Ny)).astype(DT[prec][1])
    s = C.project(cart_field(p, m), P.hpx_proj, projector=P)
    got = s.arr.cpu().numpy()
    assert s.basis == basis_of(npol) and got.shape == (nbatch, npol, r.npix) and got.dtype == DT[prec][1]
    check_values(f"{case} {prec} to_healpix", got, r.to_healpix(m), float(np.max(np.abs(m))), prec, npol)
    outside = np.ones(r.npix, dtype=bool)
    outside[r.touched] = False
    assert np.all(got[..., outside] == 0)                                    # exactly 0 outside the touched set
    assert np.array_equal(got, C.project(cart_field(p, m), P.hpx_proj, projector=P).arr.cpu().numpy())


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_one_shot_project_equals_cached_projector(prec):
    C = _pkg()
    p, P = dev("n4_odd", prec)
    g = np.random.default_rng(5)
    h = C.HealpixField(P.hpx_proj, g.standard_normal((2, 2, 192)).astype(DT[prec][1]), "QU")
    assert torch.equal(C.project(h, p).arr, C.project(h, p, projector=P).arr)
    m = C.Field(p, p.tensor(g.standard_normal((2, 2, p.Nx, p.Ny))), C.MAP)
    assert torch.equal(C.project(m, C.ProjHealpix(4)).arr, C.project(m, P.hpx_proj, projector=P).arr)
    # Map(cart_field) (:311): an input in another basis is converted first, with the library's own transform
    mF = m.to(C.FOURIER)
    assert torch.equal(C.project(mF, P.hpx_proj, projector=P).arr, C.project(mF.to(C.MAP), P.hpx_proj, projector=P).arr)
    with pytest.raises(ValueError):
        C.project(h, p, projector=dev("n16_phi0", prec)[1])


def test_errors():
    C = _pkg()
    p = C.ProjLambert(16, 24, 400.0, torch.float32)
    lib, hnd = p.lib, ctypes.c_void_p()
    rot = (ctypes.c_double * 3)(0, 90, 0)
    for bad in (0, 3, 12, 16384, -4):
        assert lib.cmbl_projector_create(p._h, bad, 0, rot, ctypes.byref(hnd)) == ERR_SHAPE
        with pytest.raises(ValueError):
            C.ProjHealpix(bad)
    th, ph = ctypes.c_double(), ctypes.c_double()
    assert lib.cmbl_healpix_pix2ang_host(3, 0, 1, ctypes.byref(th), ctypes.byref(ph)) == ERR_SHAPE
    assert lib.cmbl_projector_create(p._h, 4, 7, rot, ctypes.byref(hnd)) == ERR_ARG
    P = C.Projector(C.ProjHealpix(2), p)
    a = torch.zeros((1, 4, 48), dtype=torch.float32, device=p.device)
    o = torch.zeros((1, 4, 24, 16), dtype=torch.float32, device=p.device)
    for npol in (0, 4):
        assert lib.cmbl_project_to_cart(P._h, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(o.data_ptr()), npol, 1) == ERR_SHAPE
        assert lib.cmbl_project_to_healpix(P._h, 0, ctypes.c_void_p(o.data_ptr()), ctypes.c_void_p(a.data_ptr()), npol, 1) == ERR_SHAPE
    with pytest.raises(NotImplementedError):
        C.project(C.HealpixMap(np.zeros(48)), p, method="fft")
    with pytest.raises(NotImplementedError):
        C.Projector(C.ProjHealpix(2), p, method="fft")
    with pytest.raises(C.CmblError):                                         # θ = 2 acos(r/2) does not exist beyond r = 2
        C.Projector(C.ProjHealpix(2), C.ProjLambert(16, 24, 600.0, torch.float32))
    with pytest.raises(C.CmblError):                                         # a colatitude outside [0, π], as healpy refuses it
        C.Projector(C.ProjHealpix(2), C.ProjEquiRect(8, 8, (2.0, 3.5), (0.0, 1.0)))
