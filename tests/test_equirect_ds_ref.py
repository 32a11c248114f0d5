"""The float64 oracle of the ProjEquiRect data set (tests/_equirect_ds_ref.py) checked against itself on the CPU: its gradient against a finite
difference of its logpdf, the symmetry of its Hessian, its CG against a dense solve, the precondition under which a CG held in the Az basis is the
reference's (map-held) one, and that no comparison of the GPU tests sits in rounding noise.  Plus the boundary: the header declares and the library
exports every cmbl_eqds_* entry point."""
import ctypes
import os
import re

import numpy as np
import pytest

import _equirect_ds_ref as D
import _equirect_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64
SMALL = [(12, 16, 2, 0, "pix"), (12, 16, 2, 2, "pix"), (12, 16, 2, 2, "blk"), (12, 16, 2, 0, "bare"), (9, 15, 2, 0, "pix")]
_cache = {}


def case(c, **kw):
    k = (c, tuple(sorted(kw.items())))
    if k not in _cache:
        o = D.build_case(c, **kw)
        _cache[k] = (o, D.derive(o, F64))
    return _cache[k]


@pytest.mark.parametrize("c", SMALL, ids=D.case_id)
def test_gradient_is_the_derivative_of_logpdf(c):
    o, g = case(c)
    h = o["fstart"] * 10
    grad = D.gradientf(o, g, o["f"], o["d"], F64)
    want = D.map_dot(D.to_map(h, o["P"], o["Nx"], F64), D.to_map(grad, o["P"], o["Nx"], F64))
    eps = 1e-3                                                               # logpdf is quadratic in f: the central difference is exact up to rounding
    got = (D.logpdf(o, g, o["f"] + eps * h, o["d"], F64) - D.logpdf(o, g, o["f"] - eps * h, o["d"], F64)) / (2 * eps)
    np.testing.assert_allclose(got, want, rtol=1e-8)
    np.testing.assert_allclose(D.az_dot(h, grad, o["Nx"], o["P"] == 2), want, rtol=1e-12)       # the weighted Az dot is the map dot
    # the three forms of the entry point
    z = np.zeros_like(o["f"])
    np.testing.assert_allclose(D.gradientf(o, g, None, o["d"], F64), D.gradientf(o, g, z, o["d"], F64), atol=1e-13)
    np.testing.assert_allclose(D.gradientf(o, g, o["f"], None, F64), D.gradientf(o, g, o["f"], 0 * o["d"], F64), atol=1e-13)


@pytest.mark.parametrize("c", SMALL, ids=D.case_id)
def test_hessian_is_symmetric_in_the_field_dot(c):
    o, g = case(c)
    mp = lambda f: D.to_map(f, o["P"], o["Nx"], F64)
    u, v = o["f"], o["fstart"]
    a, b = D.map_dot(mp(u), mp(D.hessian(o, g, v, F64))), D.map_dot(mp(D.hessian(o, g, u, F64)), mp(v))
    np.testing.assert_allclose(a, b, rtol=1e-11)
    a, b = D.map_dot(mp(u), mp(D.preconditioner(o, g, v, F64))), D.map_dot(mp(D.preconditioner(o, g, u, F64)), mp(v))
    np.testing.assert_allclose(a, b, rtol=1e-11)
    assert np.all(D.map_dot(mp(u), mp(D.hessian(o, g, u, F64))) > 0)


@pytest.mark.parametrize("c", SMALL[:3], ids=D.case_id)
def test_tight_cg_is_the_dense_solve(c):
    o, g = case(c)
    P, Nx, Ny = o["P"], o["Nx"], o["Ny"]
    N = P * Nx * Ny
    eye = np.eye(N).reshape(N, P, Nx, Ny)
    A = D.to_map(D.hessian(o, g, D.to_az(eye, P, F64), F64), P, Nx, F64).reshape(N, N).T
    assert np.abs(A - A.T).max() < 1e-11 * np.abs(A).max()
    b = D.to_map(D.rhs(o, g, o["d"], F64), P, Nx, F64).reshape(o["B"], N)
    want = np.linalg.solve(A, b.T).T.reshape(o["B"], P, Nx, Ny)
    _, h1 = D.wiener(o, g, o["d"], F64, nsteps=1)
    f, hist = D.wiener(o, g, o["d"], F64, nsteps=400, tol=1e-22 * h1[0].max())
    assert len(hist) < 400
    assert R.field_dot(D.to_map(f, P, Nx, F64) - want, D.to_map(f, P, Nx, F64) - want) ** 0.5 < 1e-9 * R.field_dot(want, want) ** 0.5
    # the maximum: the gradient vanishes there
    gr = D.gradientf(o, g, f, o["d"], F64)
    assert np.abs(gr).max() < 1e-8 * np.abs(D.rhs(o, g, o["d"], F64)).max()


@pytest.mark.parametrize("c", SMALL[:3], ids=D.case_id)
def test_az_held_cg_is_the_map_held_one_for_symmetrised_blocks_only(c):
    """The precondition of cmbl_eqds_*: block operators that map images of maps to images of maps.  With it the CG held in the Az basis reproduces
    the map-held one to rounding; with unsymmetrised random blocks it is another iteration altogether."""
    o, g = case(c)
    fm, hm = D.wiener(o, g, o["d"], F64, fstart=o["fstart"])
    fa, ha = D.wiener_az(o, g, o["d"], F64, fstart=o["fstart"])
    np.testing.assert_allclose(ha, hm, rtol=1e-11)
    assert np.abs(fa - fm).max() < 1e-12 * np.abs(fm).max()
    if o["P"] == 1:
        return                                                               # real spin-0 blocks are symmetrised as they are
    o, g = case(c, symmetric=False)
    fm, hm = D.wiener(o, g, o["d"], F64, fstart=o["fstart"])
    fa, ha = D.wiener_az(o, g, o["d"], F64, fstart=o["fstart"])
    assert np.abs(ha[-1] - hm[-1]).max() > 1e-3 * np.abs(hm[-1]).max() or np.abs(fa - fm).max() > 1e-3 * np.abs(fm).max()


@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_gpu_cases_are_compared_above_rounding_noise(c):
    """res after the last compared step >= 1e-6 res_1 in every slot, from zero and from fstart: a case that converges further within the 8
    compared steps needs other operators, not another bound"""
    o, g = case(c)
    for fs in (None, o["fstart"]):
        _, h = D.wiener(o, g, o["d"], F64, fstart=fs)
        assert h.shape == (D.NSTEPS, o["B"])
        print(D.case_id(c), "from zero" if fs is None else "from fstart", "res_8 / res_1 =", (h[-1] / h[0]).min())
        assert np.all(h[-1] >= 1e-6 * h[0])
        assert np.all(h[-1] < h[0])


def test_header_declares_and_library_exports_the_entry_points():
    import __graft_entry__ as g
    lib = ctypes.CDLL(g.build())
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cmblens.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(cmbl_eqds_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(["cmbl_eqds_create", "cmbl_eqds_destroy", "cmbl_eqds_set_block_op", "cmbl_eqds_set_pixel_op", "cmbl_eqds_set_logdet", "cmbl_eqds_mean",
                            "cmbl_eqds_gradientf_logpdf", "cmbl_eqds_logpdf", "cmbl_eqds_wiener_cg"])
    for s in names + ["cmbl_equirect_field_dot"]:
        assert hasattr(lib, s), s
    assert "#define CMBL_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "cmblens.h")).read()       # additive only
    import cmblensing_jl_amd as C
    assert C.EquiRectDataSet.argmaxf_logpdf and C.EquiRectField.dot_batch
