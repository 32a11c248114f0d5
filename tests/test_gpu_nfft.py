"""The non-uniform-FFT method of the HEALPix projection on the device (cmbl_projector_create_method(..., CMBL_PROJECT_NFFT), method="nfft")
against the exact sums it approximates (tests/_nfft_ref.py `direct_*`, float64, pinned by tests/test_nfft_ref.py), in both precisions.

Cases (every one with npol 1, 2, 3 and nbatch 1, 3, both directions): Nside 16 on 24 x 32 at 120', rotator (0, 90, 0); Nside 32 on 30 x 44 at
60', (40, -20, 10) -- sides that are no powers of two, fine grid 60 x 88; Nside 8 on 8 x 12 at 240', (0, 30, 0) -- the smallest side float64
accepts, where the window wraps round the periodic fine grid; Nside 16 on a ProjEquiRect 24 x 32 with the spans of tests/test_gpu_healpix.py;
and, since all of those run the any-size transforms, Nside 32 on 32 x 64 at 60', (0, 90, 0): powers of two, where the patch's and the fine
grid's contexts both take the fused transforms and their bit-reversed half-plane layout.

Tolerances.  Relative L2 error per plane <= 3 x the case's entry of tests/golden/nfft_budget.json (floor 1e-12): the project's factor
(tests/_tol.py) over the error the window RESTATEMENT shows in that dtype against the same sums (tools/make_nfft_budget.py), not over
anything measured on the code under test.  The transposition identity is held to 3 x the mismatch the restatement shows, in the same
normalisation.  The trigonometric-polynomial check needs no oracle: the polynomial's values at the projector's own (i, j) readbacks; its
bound is the case's to_healpix bound.  Every comparison is logged through _tol._record (CMBL_PARITY_LOG)."""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _nfft_ref as N
import _tol

DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
ERR_ARG, ERR_SHAPE = 1, 2
BUDGET = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nfft_budget.json")))
CASES = list(N.CASES)
_dev = {}


def _pkg():
    import cmblensing_jl_amd as C
    return C


def cart_proj(case, prec):
    C = _pkg()
    nside, Ny, Nx, theta, rot = N.CASES[case]
    return C.ProjEquiRect(Ny, Nx, *N.EQ_SPANS, T=DT[prec][0]) if theta is None else C.ProjLambert(Ny, Nx, theta, DT[prec][0], rotator=rot)


def dev(case, prec):
    """(cart_proj, nfft Projector) on the device, made once"""
    k = (case, prec)
    if k not in _dev:
        C = _pkg()
        p = cart_proj(case, prec)
        _dev[k] = (p, C.Projector(C.ProjHealpix(N.CASES[case][0]), p, method="nfft"))
    return _dev[k]


def cart_field(p, arr):
    C = _pkg()
    eq = isinstance(p, C.ProjEquiRect) and arr.shape[1] < 3               # EquiRectField is spin 0 or 2; IQU on a ProjEquiRect is a plain MAP Field
    return C.EquiRectField(p, arr, C.MAP) if eq else C.Field(p, p.tensor(arr), C.MAP)


def basis_of(npol):
    return {1: "I", 2: "QU", 3: "IQU"}[npol]


def tol_of(case, prec, what):
    return max(_tol.FACTOR * BUDGET["cases"][case][prec][what], _tol.FLOOR)


def check_planes(what, got, want, tol):
    for k, err in enumerate(N.rel_planes(got, want)):
        _tol._record(_tol._key(f"{what} plane {k}"), float(err), tol)
        print(f"{what} plane {k}: relative L2 error {err:.3e}, bound {tol:.3e}")
    assert np.all(N.rel_planes(got, want) <= tol), (what, N.rel_planes(got, want), tol)


def check_lists(case, P):
    r = N.projector(case)
    assert r.cut_margin() > 1e-9
    assert np.array_equal(P.hpx_idxs_in_patch, r.hpx_idxs_in_patch) and P.n_in_patch == r.npatch


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES)
def test_lists_method_and_width(case, prec):
    p, P = dev(case, prec)
    check_lists(case, P)
    assert P.method == "nfft" and P.window_width == N.WIDTH[prec] == BUDGET["cases"][case][prec]["width"]
    m, w = ctypes.c_int(-1), ctypes.c_int(-1)
    assert p.lib.cmbl_projector_method(P._h, ctypes.byref(m), ctypes.byref(w)) == 0 and (m.value, w.value) == (1, N.WIDTH[prec])
    B = _pkg().Projector(P.hpx_proj, p)
    assert B.method == "bilinear" and B.window_width == 0


@pytest.mark.parametrize("nbatch", [1, 3])
@pytest.mark.parametrize("npol", [1, 2, 3])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES)
def test_project_both_directions(case, prec, npol, nbatch):
    C = _pkg()
    r = N.projector(case)
    p, P = dev(case, prec)
    check_lists(case, P)
    g = np.random.default_rng(1000 * npol + nbatch)
    # sphere -> patch
    h = g.standard_normal((nbatch, npol, r.npix)).astype(DT[prec][1])
    f = C.project(C.HealpixField(P.hpx_proj, h, basis_of(npol)), p, method="nfft", projector=P)
    got = f.arr.cpu().numpy()
    assert got.shape == (nbatch, npol, p.Nx, p.Ny) and got.dtype == DT[prec][1]
    check_planes(f"{case} {prec} to_cart", got, r.direct_to_cart(h), tol_of(case, prec, "to_cart"))
    # patch -> sphere
    m = g.standard_normal((nbatch, npol, p.Nx, p.Ny)).astype(DT[prec][1])
    s = C.project(cart_field(p, m), P.hpx_proj, method="nfft", projector=P)
    got = s.arr.cpu().numpy()
    assert s.basis == basis_of(npol) and got.shape == (nbatch, npol, r.npix) and got.dtype == DT[prec][1]
    check_planes(f"{case} {prec} to_healpix", got, r.direct_to_healpix(m), tol_of(case, prec, "to_healpix"))
    outside = np.ones(r.npix, dtype=bool)
    outside[r.hpx_idxs_in_patch] = False
    assert np.all(got[..., outside] == 0)                                    # exactly 0 outside hpx_idxs_in_patch


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES)
def test_transposition_on_the_device(case, prec):
    """Ny Nx dot(to_healpix(m), h) = Npatch dot(m, to_cart(h)) for random I fields, as a fraction of Ny Nx |to_healpix(m)| |h on the patch|"""
    C = _pkg()
    r = N.projector(case)
    p, P = dev(case, prec)
    g = np.random.default_rng(77)
    tol = max(_tol.FACTOR * BUDGET["cases"][case][prec]["transpose"], _tol.FLOOR)
    for trial in range(4):
        m = g.standard_normal((1, 1, p.Nx, p.Ny)).astype(DT[prec][1])
        h = g.standard_normal((1, 1, r.npix)).astype(DT[prec][1])
        th = P.to_healpix(cart_field(p, m)).arr.cpu().numpy().astype(np.float64)
        tc = P.to_cart(C.HealpixField(P.hpx_proj, h, "I")).arr.cpu().numpy().astype(np.float64)
        lhs, rhs = p.Ny * p.Nx * np.sum(th * h), P.n_in_patch * np.sum(m.astype(np.float64) * tc)
        err = abs(lhs - rhs) / (p.Ny * p.Nx * np.linalg.norm(th) * np.linalg.norm(h[..., r.hpx_idxs_in_patch].astype(np.float64)))
        _tol._record(_tol._key(f"{case} {prec} transposition"), float(err), tol)
        print(f"{case} {prec} transposition {trial}: {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (err, tol)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES)
def test_trigonometric_polynomial_lands_on_the_centres(case, prec):
    """a polynomial with |l| < N/2 sampled on the patch is reproduced at the HEALPix centres: no oracle, the projector's own (i, j)"""
    p, P = dev(case, prec)
    Ny, Nx = p.Ny, p.Nx
    g = np.random.default_rng(3)
    ly, lx = np.meshgrid(np.arange(-(Ny // 2) + 1, Ny // 2), np.arange(-(Nx // 2) + 1, Nx // 2), indexing="ij")
    a, b = g.standard_normal(ly.shape), g.standard_normal(ly.shape)

    def poly(i, j):
        y, x = (np.asarray(i, dtype=np.float64) - Ny // 2 - 1) / Ny, (np.asarray(j, dtype=np.float64) - Nx // 2 - 1) / Nx
        ph = 2 * np.pi * (ly[..., None] * y.ravel() + lx[..., None] * x.ravel())
        return (a[..., None] * np.cos(ph) + b[..., None] * np.sin(ph)).sum((0, 1)).reshape(y.shape)

    jj, ii = np.meshgrid(np.arange(1, Nx + 1), np.arange(1, Ny + 1), indexing="ij")
    m = poly(ii, jj)[None, None].astype(DT[prec][1])                         # (1, 1, Nx, Ny)
    got = P.to_healpix(cart_field(p, m)).arr.cpu().numpy()[0, 0]
    pos = np.searchsorted(P.touched, P.hpx_idxs_in_patch)
    want = poly(P.is_[pos], P.js[pos])
    # the sampled polynomial is rounded to the dtype before it goes in: 2^-24 or 2^-53 relative per sample, an order below the bound
    err = float(np.linalg.norm(got[P.hpx_idxs_in_patch] - want) / np.linalg.norm(want))
    tol = tol_of(case, prec, "to_healpix")
    _tol._record(_tol._key(f"{case} {prec} trig poly"), err, tol)
    print(f"{case} {prec} trig poly: relative L2 error {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES)
def test_runs_are_bit_identical(case, prec):
    C = _pkg()
    r = N.projector(case)
    p, P = dev(case, prec)
    g = np.random.default_rng(4)
    h = C.HealpixField(P.hpx_proj, g.standard_normal((3, 3, r.npix)).astype(DT[prec][1]), "IQU")
    m = cart_field(p, g.standard_normal((3, 3, p.Nx, p.Ny)).astype(DT[prec][1]))
    a, b = P.to_cart(h).arr.clone(), P.to_healpix(m).arr.clone()
    assert torch.equal(a, P.to_cart(h).arr) and torch.equal(b, P.to_healpix(m).arr)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_one_shot_project_equals_cached_projector(prec):
    C = _pkg()
    p, P = dev("n32_mixed", prec)
    g = np.random.default_rng(5)
    h = C.HealpixField(P.hpx_proj, g.standard_normal((2, 2, P.hpx_proj.npix)).astype(DT[prec][1]), "QU")
    assert torch.equal(C.project(h, p, method="nfft").arr, C.project(h, p, method="nfft", projector=P).arr)
    m = C.Field(p, p.tensor(g.standard_normal((2, 2, p.Nx, p.Ny))), C.MAP)
    assert torch.equal(C.project(m, P.hpx_proj, method="nfft").arr, C.project(m, P.hpx_proj, method="nfft", projector=P).arr)
    # Map(cart_field) (:319): an input in another basis is converted first, with the library's own transform
    mF = m.to(C.FOURIER)
    assert torch.equal(C.project(mF, P.hpx_proj, method="nfft", projector=P).arr, C.project(mF.to(C.MAP), P.hpx_proj, method="nfft", projector=P).arr)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bilinear_is_unchanged_through_the_new_entry_point(prec):
    C = _pkg()
    p = cart_proj("n16_base", prec)
    old, new = C.Projector(C.ProjHealpix(16), p), ctypes.c_void_p()
    rot = (ctypes.c_double * 3)(0, 90, 0)
    assert p.lib.cmbl_projector_create_method(p._h, 16, 0, rot, 0, ctypes.byref(new)) == 0
    try:
        g = np.random.default_rng(6)
        h = p.tensor(g.standard_normal((2, 3, 3072)))
        m = p.tensor(g.standard_normal((2, 3, p.Nx, p.Ny)))
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())

        def run(handle):
            oc, oh = torch.empty_like(m), torch.empty_like(h)
            assert p.lib.cmbl_project_to_cart(handle, ptr(h), ptr(oc), 3, 2) == 0
            assert p.lib.cmbl_project_to_healpix(handle, 0, ptr(m), ptr(oh), 3, 2) == 0
            return oc, oh

        (ac, ah), (bc, bh) = run(old._h), run(new)
        assert torch.equal(ac, bc) and torch.equal(ah, bh) and float(ac.abs().sum()) > 0 and float(ah.abs().sum()) > 0
        mm, w = ctypes.c_int(-1), ctypes.c_int(-1)
        assert p.lib.cmbl_projector_method(new, ctypes.byref(mm), ctypes.byref(w)) == 0 and (mm.value, w.value) == (0, 0)
    finally:
        assert p.lib.cmbl_projector_destroy(new) == 0


def test_errors():
    C = _pkg()
    hnd = ctypes.c_void_p()
    rot = (ctypes.c_double * 3)(0, 90, 0)

    def create(p, nside, method, params=rot, kind=0):
        return p.lib.cmbl_projector_create_method(p._h, nside, kind, params, method, ctypes.byref(hnd))

    for Ny, Nx in ((25, 32), (24, 31)):                                      # an odd side
        assert create(C.ProjLambert(Ny, Nx, 120.0, torch.float64), 16, 1) == ERR_SHAPE
    for T in (torch.float32, torch.float64):                                 # below the minimum: the fine grid 4 cells wide holds no window
        assert create(C.ProjLambert(2, 32, 120.0, T), 16, 1) == ERR_SHAPE
        assert create(C.ProjLambert(32, 2, 120.0, T), 16, 1) == ERR_SHAPE
    assert create(C.ProjLambert(6, 32, 120.0, torch.float64), 16, 1) == ERR_SHAPE      # 2 N = 12 < 14
    assert create(C.ProjLambert(16, 2050, 1.0, torch.float32), 16, 1) == ERR_SHAPE
    assert create(C.ProjLambert(2050, 16, 1.0, torch.float32), 16, 1) == ERR_SHAPE
    p = C.ProjLambert(24, 32, 120.0, torch.float32)
    for bad in (2, -1, 7):
        assert create(p, 16, bad) == ERR_ARG
    # no HEALPix centre in the patch: Nside 1 on 8 x 8 pixels of 10' around (θ, ϕ) = (120°, 0), 30° from the nearest of the 12 centres
    empty = (ctypes.c_double * 3)(0, 60, 0)
    small = N.Projector(1, N.R.Lambert(8, 8, 10.0, (0, 60, 0)))
    assert small.npatch == 0
    for T in (torch.float32, torch.float64):
        assert create(C.ProjLambert(8, 8, 10.0, T), 1, 1, empty) == ERR_ARG
        assert create(C.ProjLambert(8, 8, 10.0, T), 1, 0, empty) == 0        # ... which the bilinear method accepts
        assert p.lib.cmbl_projector_destroy(hnd) == 0
    with pytest.raises(C.CmblError):
        C.Projector(C.ProjHealpix(1), C.ProjLambert(8, 8, 10.0, torch.float32, rotator=(0, 60, 0)), method="nfft")
    # a ProjEquiRect field that is not MAP
    pe, Pe = dev("n16_equirect", "f32")
    a = torch.zeros((1, 1, 32, 13, 2), dtype=torch.float32, device=pe.device)
    o = torch.zeros((1, 1, 3072), dtype=torch.float32, device=pe.device)
    assert pe.lib.cmbl_project_to_healpix(Pe._h, 1, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(o.data_ptr()), 1, 1) == ERR_ARG
    # a projector of the other method handed to project, either way round
    pl, Pn = dev("n16_base", "f32")
    Pb = C.Projector(Pn.hpx_proj, pl)
    h = C.HealpixMap(np.zeros(3072, dtype=np.float32))
    with pytest.raises(ValueError):
        C.project(h, pl, method="nfft", projector=Pb)
    with pytest.raises(ValueError):
        C.project(h, pl, projector=Pn)
    with pytest.raises(ValueError):
        C.project(h, pl, method="spline")
    with pytest.raises(NotImplementedError):                                 # the reference's own spelling stays refused, message and all
        C.project(h, pl, method="fft")
