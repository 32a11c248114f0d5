"""CPU checks of the pullbacks of `project`: the float64 restatement of the four transposes (tests/_project_adjoint_ref.py) against the
forward restatements it transposes, the Python layer as far as it goes without a device, and the two new entry points of the C ABI.

  * for every case and npol, random x, y:  |<A x, y> - <x, Aᵀ y>| <= 1e-13 |A x| |y|, A = `_healpix_ref.Projector.to_cart` / `to_healpix`
    and `_nfft_ref.Projector.direct_to_cart` / `direct_to_healpix`, Aᵀ the new restatement;
  * at Nside 1 and 2 on 16 x 24 the dense matrix of A, built column by column, equals the transpose of the dense matrix of Aᵀ to 1e-14;
  * the envelope helper bounds the transposes and counts the rows;
  * `project_adjoint` and the two `Projector` methods exist and refuse what `project` refuses, with the same messages;
  * include/cmblens.h declares, lib.SYMBOLS lists and the built library exports cmbl_project_to_cart_adjoint / _to_healpix_adjoint."""
import os
import re
import subprocess

import numpy as np
import pytest

import _healpix_ref as R
import _nfft_ref as N
import _project_adjoint_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cmbl_project_to_cart_adjoint", "cmbl_project_to_healpix_adjoint")


def _identity(Ax, y, x, ATy):
    Ax, y, x, ATy = (np.asarray(a, dtype=np.float64).ravel() for a in (Ax, y, x, ATy))
    return abs(np.dot(Ax, y) - np.dot(x, ATy)), np.linalg.norm(Ax) * np.linalg.norm(y)


@pytest.mark.parametrize("npol", [1, 2, 3])
@pytest.mark.parametrize("case", list(A.BILINEAR_CASES))
def test_bilinear_restatement_is_the_transpose(case, npol):
    r = A.ref(case)
    assert r.cut_margin() > 1e-9
    g = np.random.default_rng(100 + npol)
    Nx, Ny = r.cart.Nx, r.cart.Ny
    h, m = g.standard_normal((2, npol, r.npix)), g.standard_normal((2, npol, Nx, Ny))
    for name, (Ax, y, x, ATy) in (("to_cart", (r.to_cart(h), m, h, A.to_cart_T(r, m))), ("to_healpix", (r.to_healpix(m), h, m, A.to_healpix_T(r, h)))):
        err, scale = _identity(Ax, y, x, ATy)
        assert err <= 1e-13 * scale, (case, name, err / scale)
    # (1) is exactly 0 wherever no Cartesian pixel reads, (2) ignores the cotangent outside the touched set
    read = np.zeros(r.npix, dtype=bool)
    read[A.cart_table(r)[0].ravel()] = True
    assert np.all(A.to_cart_T(r, m)[..., ~read] == 0)
    h2 = h.copy()
    outside = np.ones(r.npix, dtype=bool)
    outside[r.touched] = False
    h2[..., outside] = 1e30
    assert np.array_equal(A.to_healpix_T(r, h2), A.to_healpix_T(r, h))


@pytest.mark.parametrize("npol", [1, 2, 3])
@pytest.mark.parametrize("case", list(N.CASES))
def test_nfft_restatement_is_the_transpose(case, npol):
    r = N.projector(case)
    g = np.random.default_rng(200 + npol)
    Nx, Ny = r.cart.Nx, r.cart.Ny
    h, m = g.standard_normal((2, npol, r.npix)), g.standard_normal((2, npol, Nx, Ny))
    for name, (Ax, y, x, ATy) in (("to_cart", (r.direct_to_cart(h), m, h, A.nfft_to_cart_T(r, m))),
                                  ("to_healpix", (r.direct_to_healpix(m), h, m, A.nfft_to_healpix_T(r, h)))):
        err, scale = _identity(Ax, y, x, ATy)
        assert err <= 1e-13 * scale, (case, name, err / scale)
    outside = np.ones(r.npix, dtype=bool)
    outside[r.hpx_idxs_in_patch] = False
    assert np.all(A.nfft_to_cart_T(r, m)[..., outside] == 0)


def _dense(op, nin_shape, npol):
    """the matrix of `op` on (npol,) + nin_shape inputs, column by column (the unit vectors travel as the batch)"""
    n = npol * int(np.prod(nin_shape))
    cols = op(np.eye(n).reshape((n, npol) + tuple(nin_shape)))
    return cols.reshape(n, -1).T                                              # (nout, nin)


@pytest.mark.parametrize("npol", [1, 2, 3])
@pytest.mark.parametrize("case", ["n1", "n2"])
def test_dense_matrices_are_transposes(case, npol):
    r = A.ref(case)
    Nx, Ny = r.cart.Nx, r.cart.Ny
    Mc, McT = _dense(r.to_cart, (r.npix,), npol), _dense(lambda g: A.to_cart_T(r, g), (Nx, Ny), npol)
    assert Mc.shape == McT.T.shape and np.max(np.abs(Mc - McT.T)) <= 1e-14
    Mh, MhT = _dense(r.to_healpix, (Nx, Ny), npol), _dense(lambda h: A.to_healpix_T(r, h), (r.npix,), npol)
    assert Mh.shape == MhT.T.shape and np.max(np.abs(Mh - MhT.T)) <= 1e-14
    assert np.any(Mc != 0) and np.any(Mh != 0)


@pytest.mark.parametrize("which", ["to_cart", "to_healpix"])
@pytest.mark.parametrize("case", ["n4_odd", "n16_north", "n64_coarse"])
def test_envelope_bounds_the_transpose_and_counts_the_rows(case, which):
    r = A.ref(case)
    g = np.random.default_rng(7)
    Nx, Ny = r.cart.Nx, r.cart.Ny
    x = g.standard_normal((2, 3, Nx, Ny)) if which == "to_cart" else g.standard_normal((2, 3, r.npix))
    out = A.to_cart_T(r, x) if which == "to_cart" else A.to_healpix_T(r, x)
    E, L, S = A.envelope(r, x, which)
    assert E.shape == out.shape and np.all(np.abs(out) <= E * (1 + 1e-12) + 1e-300)
    entries = 4 * Nx * Ny if which == "to_cart" else int(A.flat_corners(r)[2].sum())
    assert L.sum() == entries and L.size == out[0, 0].size and np.all(S >= 0)
    assert np.all(E.reshape(2, 3, -1)[:, :, L == 0] == 0)
    if case == "n64_coarse" and which == "to_healpix":
        assert L.max() >= 200                                                # the long rows of (2) the device test is after


def test_long_rows_of_the_first_transpose():
    _, L, _ = A.envelope(A.ref("n64"), np.zeros((1, 1, 64, 48)), "to_cart")
    assert L.max() >= 50                                                      # Nside 64 read on 10' pixels


def test_python_layer_without_a_device():
    import cmblensing_jl_amd as C
    from cmblensing_jl_amd import healpix as H
    assert callable(C.project_adjoint) and C.project_adjoint is H.project_adjoint
    assert callable(C.Projector.to_cart_adjoint) and callable(C.Projector.to_healpix_adjoint)
    h = C.HealpixMap(np.zeros(48))

    def outcome(fn, *a, **k):
        with pytest.raises(Exception) as e:
            fn(*a, **k)
        return type(e.value), str(e.value)

    class NotAProjection:
        pass

    for args, kw in (((h, C.ProjHealpix(2)), {}),                             # sphere => sphere
                     ((NotAProjection(), NotAProjection()), {}),              # patch => patch
                     ((h, NotAProjection()), {"method": "spline"}),
                     ((h, NotAProjection()), {"method": "fft"})):
        want, got = outcome(C.project, *args, **kw), outcome(C.project_adjoint, *args, **kw)
        assert got == want, (got, want)
    assert outcome(C.project_adjoint, h, C.ProjHealpix(2))[0] is TypeError
    assert outcome(C.project_adjoint, h, NotAProjection(), method="spline")[0] is ValueError
    assert outcome(C.project_adjoint, h, NotAProjection(), method="fft")[0] is NotImplementedError


def test_header_declares_and_binding_lists_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "cmblens.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, args in zip(NEW, ("const void* map_cot, void* hpx_out", "const void* hpx_cot, void* map_out")):
        assert re.search(r"\bint %s\(cmbl_projector\* P, %s, int npol, int nbatch\);" % (name, re.escape(args)), code), name
    assert "NOT here: NEST ordering." in hdr and "the AD rules.\n" not in hdr[hdr.index("HEALPix <-> Cartesian projection"):]
    assert "#define CMBL_ABI_VERSION 3" in hdr
    from cmblensing_jl_amd import lib
    for name in NEW:
        assert name in lib.SYMBOLS and len(lib.SIGNATURES[name]) == 5


def test_built_library_exports_the_entry_points():
    import __graft_entry__ as g
    path = g.build()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    for name in NEW:
        assert name in exported, name
