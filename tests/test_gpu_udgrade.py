"""cmbl_ud_grade / cmbl_pixwin_host on the device against tests/_udgrade_ref.py, the float64 restatement of the reference's ud_grade
(src/proj_lambert.jl:533-592; pinned on its own by tests/test_udgrade_ref.py), on identical inputs: P = 2, B = 2 with distinct data per slice;
complex inputs are the rfft of real maps.

Shapes: the smallest at which each branch can go wrong --
  128^2 -> 64^2, 64x128 -> 32x64 (fac 2)   both sides on the fused power-of-two path (bit-reversed kx), rectangular
  96^2 -> 32^2 (3)                         any-size source (compile-time plan, natural kx) -> power-of-two target
  128^2 -> 32^2 (4)                        the fac = 4 vector loads
  120x90 -> 40x30 (3)                      both sides any-size, run-time plans
  90x50 -> 45x25 (2), 70^2 -> 14^2 (5)     odd target sides (no Nyquist row / column); the generic-fac loop
  32^2 -> 128^2 (4), 15x25 -> 45x75 (3)    upgrade
Every downgrade shape runs both modes x the four flag settings x basis_in, basis_out in {MAP, FOURIER}, in both precisions: a call is a
few launches on at most 128^2 pixels, the whole file takes seconds.

Tolerances (relative L2 against the float64 helper on the rounded inputs, tests/_tol.py): the transform class bounds of DESIGN.md §3, 1.5e-6 in
single and 1e-12 in double precision, for every path; measured on MI355X: profiles/ud_grade_parity.txt."""
import ctypes
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _udgrade_ref as R
from _tol import close

DT = {"f32": (torch.float32, np.float32, np.complex64), "f64": (torch.float64, np.float64, np.complex128)}
TOL = {"f32": 1.5e-6, "f64": 1e-12}
THETA = 2.0
P, B = 2, 2
DOWN = [(128, 128, 2), (64, 128, 2), (96, 96, 3), (128, 128, 4), (120, 90, 3), (90, 50, 2), (70, 70, 5)]      # (Ny, Nx, fac) of the source
UP = [(32, 32, 4), (15, 25, 3)]
MAP, FOURIER, HARMONIC = 0, 1, 2
UD_MAP, UD_FOURIER = 0, 1


def _pkg():
    import cmblensing_jl_amd as C
    return C


_projs = {}


def proj(Ny, Nx, theta, prec):
    k = (Ny, Nx, theta, prec)
    if k not in _projs:
        _projs[k] = _pkg().ProjLambert(Ny, Nx, theta, DT[prec][0])
    return _projs[k]


_inputs = {}


def inputs(Ny, Nx, prec, nb=B):
    """(map, its rfft) rounded to the working precision, as float64 / complex128 host arrays: computed once per shape, never modified"""
    k = (Ny, Nx, prec, nb)
    if k not in _inputs:
        m = np.random.default_rng(Ny * 10007 + Nx).standard_normal((B, P, Nx, Ny))[:nb].astype(DT[prec][1])
        F = R.rfft2(m.astype(np.float64)).astype(DT[prec][2])
        _inputs[k] = (m, F)
    return _inputs[k]


def raw(ps, pd, mode, dc, aa, bi, t, bo, out=None):
    """the entry point itself: (return code, output tensor)"""
    nb = t.shape[0]
    out = pd.empty(bo, P, nb) if out is None else out
    rc = ps.lib.cmbl_ud_grade(ps._h, pd._h, mode, int(dc), int(aa), bi, ctypes.c_void_p(t.data_ptr()), bo, ctypes.c_void_p(out.data_ptr()), P, nb)
    return rc, out


def want(res, bo):
    arr, basis, Ny, Nx = res
    if bo == MAP:
        return arr if basis == "map" else R.irfft2(arr, Ny)
    return arr if basis == "fourier" else R.rfft2(arr)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx,fac", DOWN)
def test_downgrade(Ny, Nx, fac, prec):
    ps, pd = proj(Ny, Nx, THETA, prec), proj(Ny // fac, Nx // fac, fac * THETA, prec)
    host = dict(zip((MAP, FOURIER), inputs(Ny, Nx, prec)))
    dev = {b: ps.tensor(a) for b, a in host.items()}
    for mode, dc, aa, bi in itertools.product((UD_MAP, UD_FOURIER), (1, 0), (1, 0), (MAP, FOURIER)):
        ref = R.ud_grade(host[bi], "map" if bi == MAP else "fourier", Ny, Nx, THETA, fac * THETA, "map" if mode == UD_MAP else "fourier", bool(dc), bool(aa))
        assert ref[2:] == (pd.Ny, pd.Nx)
        for bo in (MAP, FOURIER):
            rc, out = raw(ps, pd, mode, dc, aa, bi, dev[bi], bo)
            assert rc == 0, ps.lib.cmbl_last_error()
            close(("ud_grade", "map" if mode == UD_MAP else "fourier", "deconv", dc, "aa", aa, "in", bi, "out", bo), out.cpu().numpy(), want(ref, bo), TOL[prec])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx,fac", UP)
def test_upgrade(Ny, Nx, fac, prec):
    ps, pd = proj(Ny, Nx, fac * THETA, prec), proj(Ny * fac, Nx * fac, THETA, prec)
    host = dict(zip((MAP, FOURIER), inputs(Ny, Nx, prec)))
    for bi, bo, aa in itertools.product((MAP, FOURIER), (MAP, FOURIER), (0, 1)):             # anti_aliasing is ignored
        ref = R.ud_grade(host[bi], "map" if bi == MAP else "fourier", Ny, Nx, fac * THETA, THETA, "map", False, bool(aa))
        rc, out = raw(ps, pd, UD_MAP, 0, aa, bi, ps.tensor(host[bi]), bo)
        assert rc == 0, ps.lib.cmbl_last_error()
        got = out.cpu().numpy()
        if bi == MAP and bo == MAP:
            np.testing.assert_array_equal(got, np.repeat(np.repeat(host[MAP], fac, axis=-1), fac, axis=-2))      # a pure copy
        close(("ud_grade up", "aa", aa, "in", bi, "out", bo), got, want(ref, bo), TOL[prec])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_harmonic_planes_in_fourier_mode(prec):
    ps, pd = proj(128, 128, THETA, prec), proj(64, 64, 2 * THETA, prec)
    F = inputs(128, 128, prec)[1]
    for dc, aa in itertools.product((0, 1), (0, 1)):
        rc, out = raw(ps, pd, UD_FOURIER, dc, aa, HARMONIC, ps.tensor(F), HARMONIC)
        assert rc == 0, ps.lib.cmbl_last_error()
        ref = R.ud_grade(F, "fourier", 128, 128, THETA, 2 * THETA, "fourier", bool(dc), bool(aa))
        close(("ud_grade harmonic", dc, aa), out.cpu().numpy(), ref[0], TOL[prec])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_equal_geometry(prec):
    ps, pd = proj(96, 64, THETA, prec), _pkg().ProjLambert(96, 64, THETA, DT[prec][0])          # two contexts of one geometry
    m, F = inputs(96, 64, prec)
    for mode in (UD_MAP, UD_FOURIER):
        rc, out = raw(ps, pd, mode, 1, 1, MAP, ps.tensor(m), MAP)
        assert rc == 0 and np.array_equal(out.cpu().numpy(), m)
        rc, out = raw(ps, pd, mode, 1, 1, FOURIER, ps.tensor(F), FOURIER)
        assert rc == 0 and np.array_equal(out.cpu().numpy(), F)
        rc, out = raw(ps, pd, mode, 0, 0, MAP, ps.tensor(m), FOURIER)
        assert rc == 0
        close(("ud_grade equal geometry rfft", mode), out.cpu().numpy(), R.rfft2(m.astype(np.float64)), TOL[prec])
        rc, out = raw(ps, pd, mode, 0, 0, FOURIER, ps.tensor(F), MAP)
        assert rc == 0
        close(("ud_grade equal geometry irfft", mode), out.cpu().numpy(), R.irfft2(F.astype(np.complex128), 96), TOL[prec])
    rc, out = raw(ps, ps, UD_FOURIER, 0, 0, HARMONIC, ps.tensor(F), HARMONIC)                    # ... and one context on both sides
    assert rc == 0 and np.array_equal(out.cpu().numpy(), F)


def test_error_codes():
    C = _pkg()
    ARG, SHAPE = 1, 2
    ps, pd = proj(128, 128, THETA, "f32"), proj(64, 64, 2 * THETA, "f32")
    m, F = (ps.tensor(a) for a in inputs(128, 128, "f32"))
    small = pd.tensor(inputs(64, 64, "f32")[0])
    assert raw(ps, proj(64, 64, 2 * THETA, "f64"), UD_MAP, 1, 1, MAP, m, MAP)[0] == ARG          # dtype
    with torch.cuda.stream(torch.cuda.Stream()):
        other = C.ProjLambert(64, 64, 2 * THETA, torch.float32)
    assert raw(ps, other, UD_MAP, 1, 1, MAP, m, MAP)[0] == ARG                                   # stream
    assert b"stream" in ps.lib.cmbl_last_error()
    assert raw(ps, proj(96, 96, 2 * THETA, "f32"), UD_MAP, 1, 1, MAP, m, MAP)[0] == SHAPE        # 128 / 96
    assert raw(ps, proj(64, 32, 2 * THETA, "f32"), UD_MAP, 1, 1, MAP, m, MAP)[0] == SHAPE        # different steps on the two axes
    assert raw(ps, proj(64, 64, 3 * THETA, "f32"), UD_MAP, 1, 1, MAP, m, MAP)[0] == SHAPE        # pixel size does not follow the sides
    assert raw(ps, proj(64, 64, 2 * THETA * (1 + 1e-4), "f32"), UD_MAP, 1, 1, MAP, m, MAP)[0] == SHAPE
    assert raw(ps, proj(64, 64, 2 * THETA * (1 + 1e-8), "f32"), UD_MAP, 1, 1, MAP, m, MAP)[0] == 0            # within the relative 1e-6
    assert raw(ps, pd, UD_MAP, 0, 0, MAP, m, MAP, out=m)[0] == ARG                               # in == out
    assert raw(ps, pd, UD_FOURIER, 0, 0, FOURIER, F, FOURIER, out=F.view(-1)[64:])[0] == ARG     # overlapping
    assert raw(pd, ps, UD_MAP, 1, 0, MAP, small, MAP)[0] == ARG                                  # upgrade with deconvolution
    assert raw(pd, ps, UD_FOURIER, 0, 0, MAP, small, MAP)[0] == ARG                              # Fourier upgrade
    assert raw(pd, ps, UD_MAP, 0, 0, MAP, small, MAP)[0] == 0
    assert raw(ps, pd, 2, 0, 0, MAP, m, MAP)[0] == ARG                                           # mode
    for bi, bo in ((HARMONIC, FOURIER), (FOURIER, HARMONIC), (HARMONIC, MAP), (MAP, HARMONIC)):
        assert raw(ps, pd, UD_FOURIER, 0, 0, bi, m if bi == MAP else F, bo)[0] == ARG
    assert raw(ps, pd, UD_MAP, 0, 0, HARMONIC, F, HARMONIC)[0] == ARG                            # EB planes have no maps of their own
    n = ctypes.c_size_t(5)
    assert ps.lib.cmbl_pixwin_host(ps._h, np.empty(5).ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n) == SHAPE
    # the calls above left the library usable
    rc, out = raw(ps, pd, UD_MAP, 0, 0, MAP, m, MAP)
    assert rc == 0 and torch.isfinite(out).all()


@pytest.mark.parametrize("Ny,Nx,fac", [(128, 128, 2), (120, 90, 3)])
def test_batch_slots_are_independent(Ny, Nx, fac):
    ps, pd = proj(Ny, Nx, THETA, "f32"), proj(Ny // fac, Nx // fac, fac * THETA, "f32")
    both = dict(zip((MAP, FOURIER), inputs(Ny, Nx, "f32")))
    for mode, dc, aa, bi, bo in [(UD_MAP, 1, 1, MAP, FOURIER), (UD_MAP, 1, 1, FOURIER, MAP), (UD_MAP, 1, 0, MAP, MAP), (UD_MAP, 0, 0, FOURIER, MAP),
                                 (UD_FOURIER, 0, 0, MAP, FOURIER), (UD_FOURIER, 1, 1, FOURIER, MAP)]:
        rc, two = raw(ps, pd, mode, dc, aa, bi, ps.tensor(both[bi]), bo)
        assert rc == 0
        for b in range(B):
            rc, one = raw(ps, pd, mode, dc, aa, bi, ps.tensor(both[bi][b:b + 1]), bo)
            assert rc == 0 and torch.equal(one[0], two[b]), (mode, dc, aa, bi, bo, b)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx,fac", [(128, 128, 2), (96, 96, 3), (70, 70, 5)])
def test_band_limited_closed_form(Ny, Nx, fac, prec):
    """a field band-limited below the new Nyquist: the default downgrade leaves F[k] / fac^2 and the half-pixel shift of the pixel centres"""
    C = _pkg()
    Nyn, Nxn = Ny // fac, Nx // fac
    m = inputs(Ny, Nx, prec)[0].astype(np.float64)
    m = R.irfft2(R.rfft2(m) * R.antialias_mask(Ny, Nx, Nyn, Nxn), Ny).astype(DT[prec][1])
    ky, kx = R.kfreq(Nyn)[:Nyn // 2 + 1], R.kfreq(Nxn)
    expect = R.truncate(R.rfft2(m.astype(np.float64)) * R.antialias_mask(Ny, Nx, Nyn, Nxn), Nyn, Nxn) / fac ** 2 \
        * np.exp(1j * np.pi * (fac - 1) * (ky[None, :] / Ny + kx[:, None] / Nx))
    ps = proj(Ny, Nx, THETA, prec)
    got = C.ud_grade(C.Field(ps, ps.tensor(m), C.MAP), fac * THETA)
    assert got.basis == C.FOURIER and (got.proj.Ny, got.proj.Nx, got.proj.theta_pix) == (Nyn, Nxn, fac * THETA)
    close("ud_grade band-limited closed form", got.arr.cpu().numpy(), expect, TOL[prec])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_python_host(prec):
    C = _pkg()
    ps = proj(120, 90, THETA, prec)
    m, F = inputs(120, 90, prec)
    f = C.Field(ps, ps.tensor(m), C.MAP)
    assert C.ud_grade(f, THETA) is f
    g = C.ud_grade(f, 3 * THETA, deconv_pixwin=False)                                            # map mode without deconvolution: a MAP field
    assert g.basis == C.MAP and g.proj is C.ud_grade(f, 3 * THETA).proj                          # the new context is made once
    close("python map", g.arr.cpu().numpy(), R.ud_grade(m, "map", 120, 90, THETA, 3 * THETA, "map", False, True)[0], TOL[prec])
    h = C.ud_grade(C.Field(ps, ps.tensor(F), C.HARMONIC), 3 * THETA, mode="fourier")
    assert h.basis == C.HARMONIC
    close("python harmonic", h.arr.cpu().numpy(), R.ud_grade(F, "fourier", 120, 90, THETA, 3 * THETA, "fourier")[0], TOL[prec])
    up = C.ud_grade(g, THETA, deconv_pixwin=False, proj_new=ps)
    assert up.proj is ps and up.basis == C.MAP
    np.testing.assert_array_equal(up.arr.cpu().numpy(), np.repeat(np.repeat(g.arr.cpu().numpy(), 3, axis=-1), 3, axis=-2))
    for bad in (lambda: C.ud_grade(f, 2.5 * THETA), lambda: C.ud_grade(f, 7 * THETA), lambda: C.ud_grade(f, 3 * THETA, mode="nearest"),
                lambda: C.ud_grade(g, THETA), lambda: C.ud_grade(g, THETA, mode="fourier"),
                lambda: C.ud_grade(C.Field(ps, ps.tensor(F), C.HARMONIC), 3 * THETA)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("Ny,Nx", [(64, 128), (45, 25), (70, 14)])
def test_pixwin(Ny, Nx):
    C = _pkg()
    p = proj(Ny, Nx, 3.0, "f32")
    ly, lx = R.ells(Ny, Nx, 3.0)
    expect = np.sinc(lx * np.deg2rad(3.0 / 60) / (2 * np.pi))[:, None] * np.sinc(ly * np.deg2rad(3.0 / 60) / (2 * np.pi))[None, :]
    assert p.pixwin.shape == (Nx, Ny // 2 + 1)
    np.testing.assert_allclose(p.pixwin, expect, rtol=1e-13)
    np.testing.assert_allclose(C.pixwin(3.0, p.lx), expect[:, 0], rtol=1e-6)                    # the context's own (working-precision) multipoles
