"""`EquiRectDataSet` (cmbl_eqds_*: the reference's NoLensingDataSet on ProjEquiRect and its Wiener filter on the device) and `EquiRectField.dot_batch`
(cmbl_equirect_field_dot) against the float64 NumPy oracle tests/_equirect_ds_ref.py, in both context precisions.

Bounds: tests/golden/equirect_dataset_budget.json holds, per case and quantity, the distance of the oracle run in float32 from the oracle run in
float64 on the same inputs (tools/make_equirect_dataset_budget.py; never a device figure).  A float32 context is allowed 3 x that, a float64 context
3 x that x 2^-29 (the ratio of the unit roundoffs) with the floor 1e-12; every comparison goes through tests/_tol.py and is logged.  The CG is
compared step by step over 8 steps with tol = 0; tests/test_equirect_ds_ref.py checks that the 8th residual is still >= 1e-6 of the first.

Cases (tests/_equirect_ds_ref.py::CASES): (17, 30) B = 3, spin 0 and 2: n below one row tile, ragged in p and q, the 4-slot batch form, also with Cn
block-diagonal and with neither beam nor mask; (33, 45) B = 1: odd Nx (no Nyquist column in the dot), batch form 1; (96, 64) B = 3: n = 96 / 192,
several row and summation tiles; (32, 64) B = 9: the 8-slot form with a remainder.

The best-iterate rule (the iterate of the lowest residual is returned) has no case here: a CPU search over seeds 0-5 of every case, from zero and
from fstart, found no residual that rises within the 8 compared steps, so every run returns its last iterate; the rule itself is the shared solver's
(CgSolver::solve with k_cg_beta / k_cg_keep_best), tested on the flat-sky path by
tests/test_gpu_anysize.py::test_wiener_returns_the_iterate_of_the_lowest_residual."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _equirect_ds_ref as D
import _equirect_ref as R
import _tol

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
TID = ["f32", "f64"]
BUDGET = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "equirect_dataset_budget.json")))["cases"]
F64 = np.float64


@pytest.fixture(scope="module")
def C():
    import cmblensing_jl_amd as C
    return C


_projs, _once_cache = {}, {}


def proj_of(C, Ny, Nx, T):
    if (Ny, Nx, T) not in _projs:
        _projs[(Ny, Nx, T)] = C.ProjEquiRect(Ny, Nx, (1.0, 2.0), (0.0, 2 * np.pi), T=T)
    return _projs[(Ny, Nx, T)]


def once(key, fn):
    """references are computed once, shared and never modified"""
    if key not in _once_cache:
        _once_cache[key] = fn()
    return _once_cache[key]


def inputs(c):
    return once(("in", c), lambda: D.build_case(c))


def reference(c):
    return once(("ref", c), lambda: D.reference(c, F64))


def bound(c, q, T):
    b = BUDGET[D.case_id(c)][q]
    return 3.0 * b if T == torch.float32 else max(3.0 * b * 2.0 ** -29, 1e-12)


def compare(c, q, got, T, what=None):
    want, tol = reference(c)[q], bound(c, q, T)
    got = got.arr.cpu().numpy() if hasattr(got, "arr") else np.asarray(got)
    e = _tol.scalars_close(what or q, got, want, tol) if q in D.SCALARS else _tol.close(what or q, got, want, tol)
    print(f"{D.case_id(c)} {what or q}: error {e:.3e}, bound {tol:.3e}")


def dev(p, a, T):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return p.tensor(a.astype(np.complex64 if T == torch.float32 else np.complex128))
    return p.tensor(a.astype(np.float32 if T == torch.float32 else np.float64))


def dataset(C, c, T, **kw):
    o = inputs(c)
    p = proj_of(C, o["Ny"], o["Nx"], T)
    op = lambda a: None if a is None else C.BlockDiagEquiRect(dev(p, a, T), p)
    Cn = op(o["Cn"]) if o["Cn"] is not None else dev(p, o["var"], T)
    args = dict(M=None if o["M"] is None else dev(p, o["M"], T), B=op(o["beam"]), Mhat=o["Mhat"], Cnhat=o["Cnhat"])
    args.update(kw)
    return C.EquiRectDataSet(p, op(o["Cf"]), Cn, **args), p, o


def az(C, p, a, T):
    return C.EquiRectField(p, dev(p, a, T), C.AZFOURIER)


def mp(C, p, a, T):
    from cmblensing_jl_amd.engine import MAP
    return C.EquiRectField(p, dev(p, a, T), MAP)


@pytest.mark.parametrize("T", DTYPES, ids=TID)
@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_model_gradient_logpdf(C, c, T):
    ds, p, o = dataset(C, c, T)
    f, d = az(C, p, o["f"], T), mp(C, p, o["d"], T)
    compare(c, "mean", ds.mean(f), T)
    compare(c, "grad", ds.gradientf_logpdf(f, d), T)
    compare(c, "grad_f0", ds.gradientf_logpdf(None, d), T)
    compare(c, "grad_d0", ds.gradientf_logpdf(f, 0), T)
    compare(c, "logpdf", ds.logpdf(f, d), T)
    assert abs(ds.logdet_sum - D.derive(o, F64)["logdet"]) <= 1e-9 * abs(ds.logdet_sum)


@pytest.mark.parametrize("T", DTYPES, ids=TID)
@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_wiener_filter_step_by_step(C, c, T):
    ds, p, o = dataset(C, c, T)
    d = mp(C, p, o["d"], T)
    f, hist = ds.argmaxf_logpdf(d, tol=0.0, nsteps=D.NSTEPS)
    assert hist.shape == (D.NSTEPS, o["B"])
    compare(c, "hist", hist, T)
    compare(c, "f_cg", f, T)
    f2, hist2 = ds.argmaxf_logpdf(d, tol=0.0, nsteps=D.NSTEPS)
    assert torch.equal(f.arr, f2.arr) and np.array_equal(hist, hist2)        # one writer, one order: bit-identical runs
    f, hist = ds.argmaxf_logpdf(d, fstart=az(C, p, o["fstart"], T), tol=0.0, nsteps=D.NSTEPS)
    compare(c, "hist_fs", hist, T)
    compare(c, "f_cg_fs", f, T)


@pytest.mark.parametrize("T", DTYPES, ids=TID)
@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_stop_rule(C, c, T):
    """tol at the oracle's 5th residual maximum, raised by 1e-3 of itself so that neither side sits on the strict `res < tol`: the solver stops
    where the oracle does, and returns that iterate"""
    ds, p, o = dataset(C, c, T)
    ref = reference(c)
    f, hist = ds.argmaxf_logpdf(mp(C, p, o["d"], T), tol=ref["tol_stop"], nsteps=50)
    assert ref["n_stop"] == BUDGET[D.case_id(c)]["n_stop"] < 50 and len(hist) == ref["n_stop"]
    assert np.all(hist[-1] < ref["tol_stop"]) and not np.all(hist[-2] < ref["tol_stop"])
    compare(c, "f_stop", f, T)


@pytest.mark.parametrize("T", DTYPES, ids=TID)
@pytest.mark.parametrize("c", [D.CASES[0], D.CASES[1], D.CASES[7]], ids=D.case_id)
def test_sample_f_with_injected_white_draws(C, c, T):
    ds, p, o = dataset(C, c, T)
    f, hist = ds.sample_f(0, mp(C, p, o["d"], T), white=(mp(C, p, o["wf"], T), mp(C, p, o["wn"], T)), offset=True, tol=0.0, nsteps=D.NSTEPS)
    assert hist.shape == (D.NSTEPS, o["B"])
    compare(c, "sample_f", f, T)
    # the device generator: same seed, same sample; a (f, d) pair of the right shapes
    sf, sd = ds.simulate(3, o["B"])
    sf2, sd2 = ds.simulate(3, o["B"])
    assert torch.equal(sf.arr, sf2.arr) and torch.equal(sd.arr, sd2.arr) and sd.arr.shape == (o["B"], o["P"], o["Nx"], o["Ny"])
    assert bool(torch.isfinite(sd.arr).all())


@pytest.mark.parametrize("T", DTYPES, ids=TID)
@pytest.mark.parametrize("c", [D.CASES[1], D.CASES[2], D.CASES[5]], ids=D.case_id)
def test_dot_batch_in_both_bases(C, c, T):
    """per-slot map dots in double.  The operands are float32-exact in either context (Az arrays that are images of maps; maps rounded to float32),
    the products of two float32 numbers are exact in double and the sum of N terms is in double, so the error is at most N 2^-53 Σ|a||b|: the
    bound is 1e-12 Σ|a||b| in both precisions and both bases (N <= 8192 here); a sum in float would miss it by five orders"""
    _, p, o = dataset(C, c, T)
    P, Nx = o["P"], o["Nx"]
    a, b = o["f"], o["fstart"]
    am, bm = D.to_map(a, P, Nx, F64), D.to_map(b, P, Nx, F64)
    want_az = D.map_dot(am, bm)                                                # of the float32-exact Az arrays: the map dot of their maps
    scale_az = np.array([np.sum(np.abs(x) * np.abs(y)) for x, y in zip(am, bm)])
    got_az = az(C, p, a, T).dot_batch(az(C, p, b, T))
    assert got_az.shape == (o["B"],)
    np.testing.assert_allclose(D.az_dot(a, b, Nx, P == 2), want_az, rtol=0, atol=1e-13 * scale_az.max())       # the oracle's two forms agree
    _tol.sample_close("dot_batch az", float(np.max(np.abs(got_az - want_az) / scale_az)), 1e-12)
    am32, bm32 = am.astype(np.float32).astype(F64), bm.astype(np.float32).astype(F64)
    scale = np.array([np.sum(np.abs(x) * np.abs(y)) for x, y in zip(am32, bm32)])
    got_map = mp(C, p, am32, T).dot_batch(mp(C, p, bm32, T))
    _tol.sample_close("dot_batch map", float(np.max(np.abs(got_map - D.map_dot(am32, bm32)) / scale)), 1e-12)
    print(D.case_id(c), "az", np.abs(got_az - want_az) / scale_az, "map", np.abs(got_map - D.map_dot(am32, bm32)) / scale)


@pytest.mark.parametrize("T", DTYPES, ids=TID)
@pytest.mark.parametrize("spin", [0, 2])
def test_wiener_filter_with_cl_to_cov(C, spin, T):
    """the reference's own test size (32 x 64, test/runtests.jl:629-630) with Cf = Cl_to_Cov built on the device and downloaded for the oracle (the
    covariance build has its own tests); the budget is the oracle's on the NumPy restatement of the same blocks"""
    import _equirect_cov_ref as V
    p = once(("clproj", T), lambda: C.ProjEquiRect(D.CL_NY, D.CL_NX, V.REF_THETA_SPAN, V.REF_PHI_SPAN, T=T))
    tt, ee, bb = V.camb_total(V.LMAX_TEST)
    Cf = C.Cl_to_Cov("I", p, tt, lmax=V.LMAX_TEST) if spin == 0 else C.Cl_to_Cov("P", p, ee, bb, lmax=V.LMAX_TEST)
    blocks = Cf.blocks.cpu().numpy()
    o = D.cl_case(spin, blocks.astype(np.complex128 if spin == 2 else np.float64))
    ref = once(("clref", spin, T), lambda: D.cl_reference(o, F64))
    op = lambda a: C.BlockDiagEquiRect(dev(p, a, T), p)
    ds = C.EquiRectDataSet(p, Cf, dev(p, o["var"], T), M=dev(p, o["M"], T), B=op(o["beam"]), Mhat=o["Mhat"], Cnhat=o["Cnhat"])
    f, hist = ds.argmaxf_logpdf(mp(C, p, o["d"], T), tol=0.0, nsteps=D.NSTEPS)
    for q, got in (("hist", hist), ("f_cg", f.arr.cpu().numpy())):
        b = BUDGET[f"cl_{D.CL_NY}x{D.CL_NX}_s{spin}"][q]
        tol = 3.0 * b if T == torch.float32 else max(3.0 * b * 2.0 ** -29, 1e-12)
        e = (_tol.scalars_close if q in D.SCALARS else _tol.close)(q, got, ref[q], tol)
        print(f"Cl_to_Cov 32x64 spin {spin} {q}: error {e:.3e}, bound {tol:.3e}")


def test_errors(C):
    from cmblensing_jl_amd.lib import CmblError, check
    c = D.CASES[1]
    ds, p, o = dataset(C, c, torch.float32)
    f = az(C, p, o["f"], torch.float32)
    h = ctypes.c_void_p()
    check(p.lib.cmbl_eqds_create(p._h, 2, ctypes.byref(h)))
    out = torch.empty((o["B"], 2, o["Nx"], o["Ny"]), dtype=torch.float32, device=p.device)
    with pytest.raises(CmblError) as e:                                      # no Cf^-1
        check(p.lib.cmbl_eqds_mean(h, f.arr.data_ptr(), out.data_ptr(), o["B"]))
    assert e.value.code == 5 and "CF_INV" in str(e.value)
    real = C.BlockDiagEquiRect(dev(p, R.case_blocks(o["Ny"], p.Mh, False, spd=True), torch.float32), p)
    with pytest.raises(CmblError) as e:                                      # QU with n = Ny
        check(p.lib.cmbl_eqds_set_block_op(h, 0, real.blocks.data_ptr(), 0, o["Ny"]))
    assert e.value.code == 2
    check(p.lib.cmbl_eqds_set_block_op(h, 0, ds.CfI.blocks.data_ptr(), 1, 2 * o["Ny"]))
    with pytest.raises(CmblError) as e:                                      # no form of Cn^-1
        check(p.lib.cmbl_eqds_gradientf_logpdf(h, f.arr.data_ptr(), None, torch.empty_like(f.arr).data_ptr(), o["B"]))
    assert e.value.code == 5
    with pytest.raises(CmblError) as e:                                      # nbatch > 256
        check(p.lib.cmbl_eqds_mean(h, f.arr.data_ptr(), out.data_ptr(), 257))
    assert e.value.code == 2
    check(p.lib.cmbl_eqds_destroy(h))
    podd = proj_of(C, 33, 45, torch.float32)
    with pytest.raises(CmblError) as e:                                      # QU on an odd Nx
        check(podd.lib.cmbl_eqds_create(podd._h, 2, ctypes.byref(h)))
    assert e.value.code == 2
    # the constructor: unsymmetrised blocks are refused, a missing hat is named
    raw = C.BlockDiagEquiRect(dev(p, R.case_blocks(2 * o["Ny"], p.Mh, True, spd=True), torch.float32), p)
    with pytest.raises(ValueError, match="images of maps"):
        C.EquiRectDataSet(p, raw, dev(p, o["var"], torch.float32), Cnhat=1.0)
    with pytest.raises(ValueError, match="Mhat"):
        dataset(C, c, torch.float32, Mhat=None)
    with pytest.raises(ValueError, match="Cnhat"):
        dataset(C, c, torch.float32, Cnhat=None)
