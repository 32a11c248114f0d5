"""Cℓ_to_Cov on ProjEquiRect on the device (cmbl_equirect_cov, Cl_to_Cov) against oracle (a) of tests/_equirect_cov_ref.py (pinned to the
harmonic-space oracle by tests/test_equirect_cov_ref.py), in both context precisions.

Tolerances, per azimuthal mode m, of e[m] = max_jk |got - want| / max_jk |want| (tests/golden/equirect_cov_budget.json holds the budgets):
  exact mode (ngrid = 0) against the float64 oracle: 3 x the oracle's own float64-vs-longdouble error at that m; float32 contexts add 2^-24, the
  rounding of the final store (the arithmetic is double in either precision);
  table mode against the SAME exact oracle: 3 x the error of the float64 restatement of the 4-point Lagrange lookup at that m (+ 2^-24).
Each figure is printed before it is asserted; `_tol.sample_close` records worst e[m] / tolerance[m], which must stay below 1."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _equirect_cov_ref as R
import _tol

pytestmark = pytest.mark.gpu

BUDGET = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "equirect_cov_budget.json")))
DTYPES = [torch.float32, torch.float64]
TABLE_CASES = [R.GPU_CASES[1], R.GPU_CASES[3]]
REF_CASE = R.GPU_CASES[3]
_PD = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def C():
    import cmblensing_jl_amd as C
    return C


_projs, _wants = {}, {}


def proj_of(C, case, T):
    k = (R.case_id(case), T)
    if k not in _projs:
        _projs[k] = C.ProjEquiRect(case[0], case[1], case[2], case[3], T=T)
    return _projs[k]


def spectra():
    return _once("cl", lambda: R.camb_total(R.LMAX_TEST))


def _once(key, fn):
    if key not in _wants:
        _wants[key] = fn()
    return _wants[key]


def want(case, pol):
    """the float64 exact-mode oracle, computed once and shared (never modified)"""
    def make():
        tt, ee, bb = spectra()
        theta = R.geometry(case[0], case[1], case[2], case[3])["theta"]
        return R.cov_I(theta, case[3], case[1], tt) if pol == "I" else R.cov_P(theta, case[3], case[1], ee, bb)
    return _once((R.case_id(case), pol), make)


def device_cov(C, case, pol, T, ngrid):
    tt, ee, bb = spectra()
    p = proj_of(C, case, T)
    M = C.Cl_to_Cov("I", p, tt, lmax=R.LMAX_TEST, ngrid=ngrid) if pol == "I" else C.Cl_to_Cov("P", p, ee, bb, lmax=R.LMAX_TEST, ngrid=ngrid)
    p.synchronize()
    assert M.blocks.dtype == (p.T if pol == "I" else p.CT) and M.n == (case[0] if pol == "I" else 2 * case[0])
    return M


def check_per_m(what, got, ref, budget, T):
    e = R.err_per_m(got.astype(np.float64 if not np.iscomplexobj(got) else np.complex128), ref)
    tol = 3.0 * np.asarray(budget) + (2.0 ** -24 if T == torch.float32 else 0.0)
    worst = float(np.max(e / tol))
    print(f"{what}: worst e[m] / tol[m] = {worst:.3f}; max e = {e.max():.3e}, at the worst m: e = {e[np.argmax(e / tol)]:.3e}, tol = {tol[np.argmax(e / tol)]:.3e}")
    _tol.sample_close(what, worst, 1.0)


@pytest.mark.parametrize("T", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("pol", ["I", "P"])
@pytest.mark.parametrize("case", R.GPU_CASES, ids=R.case_id)
def test_exact_mode(C, case, pol, T):
    got = device_cov(C, case, pol, T, 0).blocks.cpu().numpy()
    check_per_m(f"exact {pol}", got, want(case, pol), BUDGET["oracle"][f"{R.case_id(case)}_{pol}"], T)


@pytest.mark.parametrize("T", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("ngrid", [50_000, 2001])
@pytest.mark.parametrize("pol", ["I", "P"])
@pytest.mark.parametrize("case", TABLE_CASES, ids=R.case_id)
def test_table_mode(C, case, pol, ngrid, T):
    got = device_cov(C, case, pol, T, ngrid).blocks.cpu().numpy()
    check_per_m(f"table {pol} {ngrid}", got, want(case, pol), BUDGET["interp"][f"{R.case_id(case)}_{pol}_{ngrid}"], T)


@pytest.mark.parametrize("T", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("pol", ["I", "P"])
def test_repeats_and_slabs_are_bit_identical(C, pol, T):
    """the call twice, then with the scratch cap forced to one ring pair per slab (every slab boundary inside the ring loop)"""
    p = proj_of(C, REF_CASE, T)
    a = device_cov(C, REF_CASE, pol, T, 2001).blocks
    b = device_cov(C, REF_CASE, pol, T, 2001).blocks
    assert torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b)
    old = p._ctx.set_option("eq_cov_scratch_mb", 0)
    try:
        s = device_cov(C, REF_CASE, pol, T, 2001).blocks
    finally:
        p._ctx.set_option("eq_cov_scratch_mb", old)
    assert torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(s) if s.is_complex() else s)
    # a cap that splits an exact-mode run of a small case mid-ring as well
    case = R.GPU_CASES[2]
    q = proj_of(C, case, T)
    e0 = device_cov(C, case, pol, T, 0).blocks
    old = q._ctx.set_option("eq_cov_scratch_mb", 0)
    try:
        e1 = device_cov(C, case, pol, T, 0).blocks
    finally:
        q._ctx.set_option("eq_cov_scratch_mb", old)
    assert torch.equal(torch.view_as_real(e0) if e0.is_complex() else e0, torch.view_as_real(e1) if e1.is_complex() else e1)


def _rel(a, b):
    a, b = (x.arr.cpu().numpy().astype(np.complex128).ravel() for x in (a, b))
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(a), np.linalg.norm(b)))


@pytest.mark.parametrize("T", DTYPES, ids=["f32", "f64"])
def test_reference_properties_end_to_end(C, T):
    """test/runtests.jl:681-720 through the device operators at the reference's rtol = 1e-4, with the default table (ngrid = 50 000)"""
    p = proj_of(C, REF_CASE, T)
    Ny, Nx = REF_CASE[:2]
    tt, ee, bb = spectra()
    ell = np.arange(R.LMAX_TEST + 1)
    Cf0 = C.Cl_to_Cov("I", p, C.Cls(ell, tt))                               # Cls objects and the default ℓmax, clamped to what the spectrum holds
    Cf2 = C.Cl_to_Cov("P", p, C.Cls(ell, ee), C.Cls(ell, bb))
    assert torch.equal(Cf0.blocks, device_cov(C, REF_CASE, "I", T, 50_000).blocks)      # == arrays with the explicit ℓmax
    rng = np.random.default_rng(5)
    rtol = 1e-4
    for Cf, P in ((Cf0, 1), (Cf2, 2)):
        f = C.EquiRectField(p, p.tensor(rng.standard_normal((1, P, Nx, Ny))), C.MAP).to(C.AZFOURIER)
        errs = {"sqrt": _rel(Cf.sqrt() * (Cf.sqrt() * f), Cf * f), "pinv": _rel(Cf.pinv() * (Cf * f), f),
                "solve": _rel(Cf.solve(Cf) * f, f), "rdiv": _rel(Cf.rdiv(Cf) * f, f), "sum": _rel((Cf + Cf) * f, Cf * (2 * f))}
        g = C.simulate(Cf, seed=3)
        assert g.arr.dtype == p.CT and g.to(C.MAP).arr.dtype == p.T
        a, b = f.dot(Cf * g), (Cf.H * f).dot(g)                             # f' (C g) = (f' C) g
        errs["adjoint"] = abs(a - b) / max(abs(a), abs(b))
        print(f"spin {0 if P == 1 else 2}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= rtol, (P, k, v)
        assert abs(Cf.logdet() - Cf.logabsdet()[0]) <= 1e-8 * abs(Cf.logabsdet()[0])
    # Cℓ_to_Beam from the spectrum == the old form fed with the same blocks
    for pol in "IP":
        new, old = C.Cl_to_Beam(pol, C.Cls(ell, tt), p), C.Cl_to_Beam(pol, Cf0, p)
        assert torch.equal(torch.view_as_real(new.blocks) if new.complex else new.blocks, torch.view_as_real(old.blocks) if old.complex else old.blocks)


def test_error_codes(C):
    from cmblensing_jl_amd.lib import CmblError
    tt, ee, bb = (np.ascontiguousarray(a[:51]) for a in spectra())
    code = lambda fn: pytest.raises(CmblError, fn).value.code
    odd = C.ProjEquiRect(4, 9, (1.0, 2.0), (0.0, 2 * np.pi))
    frac = C.ProjEquiRect(4, 8, (1.0, 2.0), np.deg2rad((-50.0, 50.0)))       # 100 degrees: K = 3.6
    ok = C.ProjEquiRect(4, 8, (1.0, 2.0), (0.0, np.pi))
    assert code(lambda: C.Cl_to_Cov("I", frac, tt, ngrid=0)) == 2           # CMBL_ERR_SHAPE
    assert code(lambda: C.Cl_to_Cov("P", odd, ee, bb, ngrid=0)) == 2
    assert code(lambda: C.Cl_to_Cov("I", ok, tt, ngrid=3)) == 2
    assert code(lambda: C.Cl_to_Cov("P", ok, ee[:2], bb[:2], ngrid=0)) == 2  # ℓmax = 1
    C.Cl_to_Cov("I", odd, tt, ngrid=0)                                       # odd Nx is fine for spin 0
    bad = tt.copy()
    bad[7] = np.nan                                                          # the Python layer maps NaN to 0 like the reference; the C ABI refuses it
    out = torch.empty((ok.Mh, ok.Ny, ok.Ny), dtype=ok.T, device=ok.device)
    ts, ps = np.array(ok.theta_span), np.array(ok.phi_span)
    rc = ok.lib.cmbl_equirect_cov(ok._h, ts.ctypes.data_as(_PD), ps.ctypes.data_as(_PD), 0, 50, bad.ctypes.data_as(_PD), None, 0, ctypes.c_void_p(out.data_ptr()))
    assert rc == 4                                                           # CMBL_ERR_NAN
    got = C.Cl_to_Cov("I", ok, bad, ngrid=0)
    bad[7] = 0.0
    assert torch.equal(got.blocks, C.Cl_to_Cov("I", ok, bad, ngrid=0).blocks)
