"""The pullbacks of `project` on the device (cmbl_project_to_cart_adjoint / cmbl_project_to_healpix_adjoint, `project_adjoint`, autograd)
against tests/_project_adjoint_ref.py, the float64 NumPy restatement of the four transposes (pinned on its own by
tests/test_project_adjoint_ref.py), on identical inputs, in both precisions, npol 1, 2, 3 and nbatch 1, 3.

Bilinear cases (`_project_adjoint_ref.BILINEAR_CASES`): the shapes of tests/test_gpu_healpix.py -- among them Nside 16 on 64 x 48 at 30' with
three rotators (duplicate pixels at the poles) and Nside 64 on 48 x 64 at 10' (a HEALPix pixel is read by ~a hundred Cartesian pixels: long
rows of to_cartᵀ) -- plus n64_coarse, Nside 64 on 16 x 24 at 400', where a Cartesian pixel collects a few hundred corners (long rows of
to_healpixᵀ).  Every case first asserts cut_margin() > 1e-9 on the restatement.

Bilinear tolerances, DERIVED, elementwise: |got - want| <= tol E(g), E the envelope (the I-plane transpose applied to |g|, |Q̄| + |Ū| in the
pol planes; the weights are non-negative, so E bounds every partial sum of the row).
  float32: tol = (L + 8) 2^-24, L the length of that element's row: one rounding per fma of the row, the rounding of each weight to the
  dtype, and the rotation's roundings.
  float64: |got - want| <= 1e-12 max|g| max(1, row weight sum): the geometry-error allowance of tests/test_gpu_healpix.py scaled by the row's
  weight.
to_cartᵀ is exactly 0 wherever the restatement is; two runs are bit-identical.

NFFT cases: `_nfft_ref.CASES`.  Relative L2 error per plane against the sums through K <= 3 x the case's entry of
tests/golden/project_adjoint_budget.json (tools/make_project_adjoint_budget.py: the error of the window RESTATEMENT in that dtype, never a
device figure), floor 1e-12.  to_cartᵀ is exactly 0 outside hpx_idxs_in_patch.

The adjoint identity |<A x, y> - <x, Aᵀ y>| / (|A x| |y|) on the device needs no oracle (dots on the host in double).  float64: <= 1e-12
(bilinear) or 3 x the restatement's own mismatch in the budget file, floor 1e-12 (nfft).  float32: the value bounds carried through the dot,
|<A x, y> - <x, Aᵀ y>| <= Σ |y| ε_A + Σ |x| ε_Aᵀ with ε the elementwise value bounds (bilinear; the forward's are those of
tests/test_gpu_healpix.py), or tol_A |A x| |y| + tol_Aᵀ |x| |Aᵀ y| with the relative L2 bounds (nfft; each norm of a device result divided by
1 - tol to bound the exact one).  Every comparison is logged through _tol._record (CMBL_PARITY_LOG).
Measured on MI355X: profiles/project_adjoint_parity.txt (CMBL_PARITY_LOG)."""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _nfft_ref as N
import _project_adjoint_ref as A
import _tol

DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
U32 = 2.0 ** -24
ERR_ARG, ERR_SHAPE = 1, 2
HERE = os.path.dirname(os.path.abspath(__file__))
BUDGET = json.load(open(os.path.join(HERE, "golden", "project_adjoint_budget.json")))
FWD_BUDGET = json.load(open(os.path.join(HERE, "golden", "nfft_budget.json")))
_dev = {}


def _pkg():
    import cmblensing_jl_amd as C
    return C


def dev(method, case, prec):
    """(cart_proj, Projector) on the device, made once"""
    k = (method, case, prec)
    if k not in _dev:
        C = _pkg()
        nside, Ny, Nx, theta, rot = (A.BILINEAR_CASES if method == "bilinear" else N.CASES)[case]
        p = C.ProjEquiRect(Ny, Nx, *A.EQ_SPANS, T=DT[prec][0]) if theta is None else C.ProjLambert(Ny, Nx, theta, DT[prec][0], rotator=rot)
        _dev[k] = (p, C.Projector(C.ProjHealpix(nside), p, method=method))
    return _dev[k]


def cart_field(p, arr):
    C = _pkg()
    eq = isinstance(p, C.ProjEquiRect) and arr.shape[1] < 3               # EquiRectField is spin 0 or 2; IQU on a ProjEquiRect is a plain MAP Field
    return C.EquiRectField(p, arr, C.MAP) if eq else C.Field(p, p.tensor(arr), C.MAP)


def basis_of(npol):
    return {1: "I", 2: "QU", 3: "IQU"}[npol]


def draws(r, prec, npol, nbatch, seed):
    g = np.random.default_rng(seed + 1000 * npol + nbatch)
    m = g.standard_normal((nbatch, npol, r.cart.Nx, r.cart.Ny)).astype(DT[prec][1])
    h = g.standard_normal((nbatch, npol, r.npix)).astype(DT[prec][1])
    return m, h


def run_adjoints(P, p, m, h, method):
    """(to_cartᵀ m, to_healpixᵀ h) through `project_adjoint`, as NumPy"""
    C = _pkg()
    hc = C.project_adjoint(cart_field(p, m), P.hpx_proj, method=method, projector=P)
    mc = C.project_adjoint(C.HealpixField(P.hpx_proj, h, basis_of(h.shape[1])), p, method=method, projector=P)
    assert hc.basis == basis_of(m.shape[1]) and hc.arr.shape == h.shape and mc.arr.shape == m.shape
    assert isinstance(mc, C.EquiRectField) == (isinstance(p, C.ProjEquiRect) and m.shape[1] < 3)
    return hc.arr, mc.arr


def bilinear_bound(r, g, which, prec):
    """the elementwise bound on |got - want| of a bilinear transpose, shaped like its output"""
    E, L, S = A.envelope(r, g, which)
    rows = (lambda a: a) if which == "to_cart" else (lambda a: a.reshape(r.cart.Nx, r.cart.Ny))
    if prec == "f64":
        return 1e-12 * float(np.max(np.abs(g))) * np.maximum(1.0, rows(S)) * np.ones_like(E)
    return (rows(L) + 8) * U32 * E


def check_elementwise(what, got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))    # bound 0: the row is empty, the value exactly 0
    k = int(np.argmax(ratio))
    _tol._record(_tol._key(what), float(err.ravel()[k]), float(bound.ravel()[k]))
    print(f"{what}: worst element error {err.ravel()[k]:.3e}, its bound {bound.ravel()[k]:.3e}; max error {err.max():.3e}")
    assert np.all(err <= bound), (what, float(err.ravel()[k]), float(bound.ravel()[k]))


@pytest.mark.parametrize("nbatch", [1, 3])
@pytest.mark.parametrize("npol", [1, 2, 3])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", list(A.BILINEAR_CASES))
def test_bilinear_values(case, prec, npol, nbatch):
    r = A.ref(case)
    assert r.cut_margin() > 1e-9
    p, P = dev("bilinear", case, prec)
    m, h = draws(r, prec, npol, nbatch, 11)
    hc, mc = run_adjoints(P, p, m, h, "bilinear")
    got_h, got_m = hc.cpu().numpy(), mc.cpu().numpy()
    assert got_h.dtype == DT[prec][1] and got_m.dtype == DT[prec][1]
    want_h, want_m = A.to_cart_T(r, m), A.to_healpix_T(r, h)
    check_elementwise(f"{case} {prec} to_cart^T", got_h, want_h, bilinear_bound(r, m, "to_cart", prec))
    check_elementwise(f"{case} {prec} to_healpix^T", got_m, want_m, bilinear_bound(r, h, "to_healpix", prec))
    assert np.all(got_h[want_h == 0] == 0)                                   # exactly 0 wherever the restatement is
    again_h, again_m = run_adjoints(P, p, m, h, "bilinear")
    assert torch.equal(hc, again_h) and torch.equal(mc, again_m)             # bit-identical between runs


def nfft_tol(budget, case, prec, what):
    return max(_tol.FACTOR * budget["cases"][case][prec][what], _tol.FLOOR)


def check_planes(what, got, want, tol):
    errs = N.rel_planes(got, want)
    for k, err in enumerate(errs):
        _tol._record(_tol._key(f"{what} plane {k}"), float(err), tol)
        print(f"{what} plane {k}: relative L2 error {err:.3e}, bound {tol:.3e}")
    assert np.all(errs <= tol), (what, errs, tol)


@pytest.mark.parametrize("nbatch", [1, 3])
@pytest.mark.parametrize("npol", [1, 2, 3])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", list(N.CASES))
def test_nfft_values(case, prec, npol, nbatch):
    r = N.projector(case)
    assert r.cut_margin() > 1e-9
    p, P = dev("nfft", case, prec)
    assert np.array_equal(P.hpx_idxs_in_patch, r.hpx_idxs_in_patch)
    m, h = draws(r, prec, npol, nbatch, 23)
    m_dev = p.tensor(m)
    keep = m_dev.clone()
    hc = P.to_cart_adjoint(_pkg().Field(p, m_dev, _pkg().MAP)).arr
    assert torch.equal(m_dev, keep)                                          # the caller's array is never modified
    _, mc = run_adjoints(P, p, m, h, "nfft")
    got_h, got_m = hc.cpu().numpy(), mc.cpu().numpy()
    check_planes(f"{case} {prec} to_cart^T", got_h[..., r.hpx_idxs_in_patch], A.nfft_to_cart_T(r, m)[..., r.hpx_idxs_in_patch],
                 nfft_tol(BUDGET, case, prec, "to_cart_adjoint"))
    check_planes(f"{case} {prec} to_healpix^T", got_m, A.nfft_to_healpix_T(r, h), nfft_tol(BUDGET, case, prec, "to_healpix_adjoint"))
    outside = np.ones(r.npix, dtype=bool)
    outside[r.hpx_idxs_in_patch] = False
    assert np.all(got_h[..., outside] == 0)                                  # exactly 0 outside hpx_idxs_in_patch
    again_h, again_m = run_adjoints(P, p, m, h, "nfft")
    assert torch.equal(hc, again_h) and torch.equal(mc, again_m)


def _dot(a, b):
    return float(np.dot(np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()))


def _norm(a):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64).ravel()))


@pytest.mark.parametrize("nbatch", [1, 3])
@pytest.mark.parametrize("npol", [1, 2, 3])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("method,case", [("bilinear", c) for c in A.BILINEAR_CASES] + [("nfft", c) for c in N.CASES])
def test_adjoint_identity_on_the_device(method, case, prec, npol, nbatch):
    C = _pkg()
    r = A.ref(case) if method == "bilinear" else N.projector(case)
    p, P = dev(method, case, prec)
    m, h = draws(r, prec, npol, nbatch, 37)
    Ah = C.project(C.HealpixField(P.hpx_proj, h, basis_of(npol)), p, method=method, projector=P).arr.cpu().numpy()      # to_cart h
    Am = C.project(cart_field(p, m), P.hpx_proj, method=method, projector=P).arr.cpu().numpy()                           # to_healpix m
    hc, mc = run_adjoints(P, p, m, h, method)
    ATm, ATh = hc.cpu().numpy(), mc.cpu().numpy()                              # to_cartᵀ m, to_healpixᵀ h
    pol = np.array([npol >= 2 and k >= npol - 2 for k in range(npol)])
    for name, Ax, y, x, ATy in (("to_cart", Ah, m, h, ATm), ("to_healpix", Am, h, m, ATh)):
        scale = _norm(Ax) * _norm(y)
        err = abs(_dot(Ax, y) - _dot(x, ATy)) / scale
        if prec == "f64":
            tol = 1e-12 if method == "bilinear" else nfft_tol(BUDGET, case, prec, f"identity_{name}")
        elif method == "bilinear":
            eps_fwd = np.where(pol, 12.0, 8.0)[None, :, None] * U32 * float(np.max(np.abs(x)))          # per element of A x (tests/test_gpu_healpix.py)
            eps_adj = bilinear_bound(r, y, name, prec)                                                    # per element of Aᵀ y
            ya, xa = np.abs(y.astype(np.float64)).reshape(nbatch, npol, -1), np.abs(x.astype(np.float64))
            tol = (float(np.sum(ya * eps_fwd)) + float(np.sum(xa * eps_adj.reshape(xa.shape)))) / scale
        else:
            ta, tt = nfft_tol(FWD_BUDGET, case, prec, name), nfft_tol(BUDGET, case, prec, f"{name}_adjoint")
            tol = (ta * scale / (1 - ta) + tt * _norm(x) * _norm(ATy) / (1 - tt)) / scale
        _tol._record(_tol._key(f"{method} {case} {prec} identity {name}"), err, tol)
        print(f"{method} {case} {prec} identity {name}: {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("method,case", [("bilinear", "n64"), ("bilinear", "n64_coarse"), ("nfft", "n8_wrap")])
def test_batches_beyond_one_pass_equal_single_batches(method, case, prec):
    """nbatch 6: the bilinear gather takes its batch entries four at a time; every slice sums in the same order whatever the grouping"""
    r = A.ref(case) if method == "bilinear" else N.projector(case)
    p, P = dev(method, case, prec)
    m, h = draws(r, prec, 3, 6, 41)
    hc, mc = run_adjoints(P, p, m, h, method)
    for b in (0, 3, 4, 5):
        h1, m1 = run_adjoints(P, p, m[b:b + 1], h[b:b + 1], method)
        assert torch.equal(hc[b:b + 1], h1) and torch.equal(mc[b:b + 1], m1)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("method,case", [("bilinear", "n4_odd"), ("bilinear", "n16_equirect"), ("nfft", "n16_base")])
def test_autograd_runs_the_adjoint(method, case, prec):
    C = _pkg()
    r = A.ref(case) if method == "bilinear" else N.projector(case)
    p, P = dev(method, case, prec)
    m, h = draws(r, prec, 2, 2, 53)
    gm, gh = draws(r, prec, 2, 2, 59)
    # sphere -> patch
    x = p.tensor(h).requires_grad_(True)
    out = C.project(C.HealpixField(P.hpx_proj, x, "QU"), p, method=method, projector=P)
    assert out.arr.grad_fn is not None
    (out.arr * p.tensor(gm)).sum().backward()
    want = C.project_adjoint(cart_field(p, gm), P.hpx_proj, method=method, projector=P).arr
    assert x.grad is not None and torch.equal(x.grad, want) and float(want.abs().sum()) > 0
    plain = C.project(C.HealpixField(P.hpx_proj, p.tensor(h), "QU"), p, method=method, projector=P)
    assert plain.arr.grad_fn is None and not plain.arr.requires_grad and torch.equal(plain.arr, out.arr.detach())
    raw = torch.empty_like(plain.arr)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    assert p.lib.cmbl_project_to_cart(P._h, ptr(p.tensor(h)), ptr(raw), 2, 2) == 0 and torch.equal(raw, plain.arr)
    # patch -> sphere
    x = p.tensor(m).requires_grad_(True)
    out = C.project(cart_field(p, x), P.hpx_proj, method=method, projector=P)
    assert out.arr.grad_fn is not None and out.basis == "QU"
    (out.arr * p.tensor(gh)).sum().backward()
    want = C.project_adjoint(C.HealpixField(P.hpx_proj, gh, "QU"), p, method=method, projector=P).arr
    assert x.grad is not None and torch.equal(x.grad, want) and float(want.abs().sum()) > 0
    plain = C.project(cart_field(p, m), P.hpx_proj, method=method, projector=P)
    assert plain.arr.grad_fn is None and not plain.arr.requires_grad and torch.equal(plain.arr, out.arr.detach())
    raw = torch.empty_like(plain.arr)
    assert p.lib.cmbl_project_to_healpix(P._h, 0, ptr(p.tensor(m)), ptr(raw), 2, 2) == 0 and torch.equal(raw, plain.arr)


def test_autograd_takes_map_input_only():
    C = _pkg()
    p, P = dev("bilinear", "n4_odd", "f32")
    g = np.random.default_rng(5)
    F = C.Field(p, p.tensor(g.standard_normal((1, 1, p.Nx, p.Ny))), C.MAP).to(C.FOURIER)
    F.arr.requires_grad_(True)
    with pytest.raises(ValueError):
        C.project(F, P.hpx_proj, projector=P)


def test_errors():
    C = _pkg()
    p, P = dev("bilinear", "n2", "f32")
    lib = p.lib
    a = torch.zeros((1, 4, 48), dtype=torch.float32, device=p.device)
    o = torch.zeros((1, 4, 24, 16), dtype=torch.float32, device=p.device)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for npol, nbatch in ((4, 1), (0, 1), (1, 0), (3, -1)):
        assert lib.cmbl_project_to_cart_adjoint(P._h, ptr(o), ptr(a), npol, nbatch) == ERR_SHAPE
        assert lib.cmbl_project_to_healpix_adjoint(P._h, ptr(a), ptr(o), npol, nbatch) == ERR_SHAPE
    assert lib.cmbl_project_to_cart_adjoint(P._h, ptr(o), ptr(o), 1, 1) == ERR_ARG                # out aliases the input
    # a cotangent of another Nside
    other = C.HealpixMap(np.zeros(12 * 16, dtype=np.float32))
    with pytest.raises(ValueError):
        P.to_healpix_adjoint(other)
    with pytest.raises(ValueError):
        C.project_adjoint(other, p, projector=P)
    # a cotangent on another patch
    q = C.ProjLambert(16, 20, 400.0, torch.float32)
    with pytest.raises(ValueError):
        P.to_cart_adjoint(C.Field(q, q.tensor(np.zeros((1, 1, 20, 16))), C.MAP))
    # a projector of the other method, either way round
    pn, Pn = dev("nfft", "n16_base", "f32")
    Pb = C.Projector(Pn.hpx_proj, pn)
    h = C.HealpixMap(np.zeros(Pn.hpx_proj.npix, dtype=np.float32))
    with pytest.raises(ValueError):
        C.project_adjoint(h, pn, method="nfft", projector=Pb)
    with pytest.raises(ValueError):
        C.project_adjoint(h, pn, projector=Pn)
    with pytest.raises(ValueError):
        C.project_adjoint(h, pn, method="spline")
    with pytest.raises(NotImplementedError):
        C.project_adjoint(h, pn, method="fft")
    with pytest.raises(TypeError):
        C.project_adjoint(h, Pn.hpx_proj)
