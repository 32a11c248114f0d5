"""The θ-gradient on the device: `grad_theta_logpdf` / `grad_theta_logpdf_mixed` (cmbl_grad_theta_logpdf[_mixed], k_theta_grad of
csrc/kernels_theta.hpp) against tests/_theta_grad_ref.py, the float64 restatement that tests/test_theta_grad_ref.py pins to the oracle.

Error figure and bounds.  For r and Aϕ the mixed gradient is explicit − cross − logdet with the last two 10³–10⁴ times the result, so the
figure is max |got − want| / S per parameter group, S = |explicit| + |cross| + |logdet| of that parameter (the reference returns the parts).
The class bounds are the project's own for θ-dependent scalars, 1e-10 (fp64) and 3e-5 (fp32), relative to S.  Shapes: the three of
tests/test_gpu_theta_device.py, the smallest that reach the fused path (with mask and beam), a non-square map and the any-size path."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from _tol import sample_close
from _theta_grad_ref import ThetaGradRef
from test_gpu_theta_device import SHAPES, LE, BANDS, _pair, _state

# Measured on MI355X: fp64 at most 2.7e-14; fp32 at most 7e-8 where a cross term enlarges S, but up to 2.8e-5 for the amplitudes
# of the mixed form (T+QU 64x64), where S is the size of the result itself, a near-cancellation of a quadratic-form part and a trace part
# formed from fp32 fields.  That is 7 % inside the class bound and depends on the fields of the fixture: should another seed or shape exceed
# it, the issue's rule applies -- record the measured figure in DESIGN §5 and set the fp32 bound to 3 x that, with the reason.
RT = {"f32": 3e-5, "f64": 1e-10}
AMPS = {"ATT": np.array([1.3, 1.0, 0.8]), "ATE": np.array([0.9, 1.1, 1.0]), "AEE": np.array([1.2, 0.85, 1.05])}
THETAS = {"r+Aphi": dict(r=0.25, Aphi=1.1), "r": dict(r=0.3), "Aphi": dict(Aphi=0.9)}


def _bands(pol):
    return {n: AMPS[n] for n in BANDS[pol][1]}


def _band_thetas(pol):
    names = list(BANDS[pol][1])
    return {"all": dict(r=0.3, Aphi=1.1, **_bands(pol)), "one band": {names[-1]: AMPS[names[-1]]}}


def _split(theta):
    return theta.get("r"), theta.get("Aphi"), {k: v for k, v in theta.items() if k not in ("r", "Aphi")}


@functools.lru_cache(maxsize=None)
def _ref(pol, shape, B, banded, key):
    """the reference is float64 whatever the device precision: once per case, shared by both precisions and by every test that needs it"""
    _, so, _, (fo_o, po_o), _ = _pair("f64", pol, shape, B)
    theta = (_band_thetas(pol) if banded else THETAS)[key]
    r, A, amps = _split(theta)
    ref = ThetaGradRef(so["ds"], so["Cfs"], so["Cten"], bands=BANDS[pol][1] if banded else None)
    lp, mixed, _ = ref.mixed(fo_o, po_o, r, A, amps)
    return lp, mixed, ref.unmixed(so["f"], so["phi"], r, A, amps)


def _compare(label, prec, got, want):
    assert set(got) == set(want), (label, set(got), set(want))
    for name in want:
        g, w = np.asarray(got[name]), want[name]
        assert g.shape == w["total"].shape, (label, name, g.shape)
        err = float(np.max(np.abs(g - w["total"]) / w["S"]))
        print(f"[{label}] {name}: max |got - want| / S = {err:.3e}   (want {np.ravel(w['total'])[:3]}, S {np.ravel(w['S'])[:3]})")
        sample_close(f"{label} {name}", err, RT[prec])


def _fields(C, so, sd):
    p = sd["proj"]
    return C.Field(p, p.tensor(so["f"]), C.HARMONIC), C.Field(p, p.tensor(so["phi"]), C.FOURIER)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("pol", ["I", "P", "IP"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_reference(prec, pol, shape):
    """both forms at θ = (r, Aϕ) and at θ naming one parameter only; the value is the grid's bit for bit, a second call is bit-identical, the
    data set is untouched"""
    C, so, sd, _, (fo, po) = _pair(prec, pol, shape)
    ds = sd["ds"]
    f, phi = _fields(C, so, sd)
    before, lp0 = _state(ds), ds.logpdf_mixed(fo, po)
    print()
    for key in (THETAS if shape == "64x64" else ("r+Aphi", "r")):
        theta = THETAS[key]
        lp_w, mixed_w, unmixed_w = _ref(pol, shape, 1, False, key)
        lp, g = C.grad_theta_logpdf_mixed(ds, fo, po, theta)
        lp2, g2 = C.grad_theta_logpdf_mixed(ds, fo, po, theta)
        assert np.array_equal(lp, lp2) and all(np.array_equal(g[k], g2[k]) for k in g)
        assert np.array_equal(lp, C.logpdf_mixed_theta_grid(ds, fo, po, [theta])[0])
        np.testing.assert_allclose(lp, lp_w, rtol=RT[prec])
        _compare(f"{prec} {pol} {shape} mixed {key}", prec, g, mixed_w)
        u = C.grad_theta_logpdf(ds, f, phi, theta)
        u2 = C.grad_theta_logpdf(ds, f, phi, theta)
        assert all(np.array_equal(u[k], u2[k]) for k in u)
        _compare(f"{prec} {pol} {shape} unmixed {key}", prec, u, unmixed_w)
    after = _state(ds)
    assert np.array_equal(ds.logpdf_mixed(fo, po), lp0)
    assert before[1:] == after[1:] and all(torch.equal(before[0][k], after[0][k]) for k in before[0]) and before[0].keys() == after[0].keys()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("pol", ["P", "IP"])
def test_bandpower_amplitudes(prec, pol):
    """bands (P: EE; IP: TT, TE, EE) together with r and Aϕ, and one amplitude vector alone"""
    C, so, sd, _, (fo, po) = _pair(prec, pol, "64x64")
    ds = sd["ds"]
    f, phi = _fields(C, so, sd)
    cls = {k: C.Cls(v.ell, v.cl) for k, v in so["cls"]["unlensed_scalar"].items()}
    C.use_bandpowers(ds, BANDS[pol][0], cls)
    print()
    try:
        for key, theta in _band_thetas(pol).items():
            lp_w, mixed_w, unmixed_w = _ref(pol, "64x64", 1, True, key)
            lp, g = C.grad_theta_logpdf_mixed(ds, fo, po, theta)
            assert np.array_equal(lp, C.logpdf_mixed_theta_grid(ds, fo, po, [theta])[0])
            np.testing.assert_allclose(lp, lp_w, rtol=RT[prec])
            assert all(g[n].shape == (1, len(LE) - 1) for n in theta if n not in ("r", "Aphi"))
            _compare(f"{prec} {pol} bands mixed {key}", prec, g, mixed_w)
            lp2, g2 = C.grad_theta_logpdf_mixed(ds, fo, po, theta)
            assert np.array_equal(lp, lp2) and all(np.array_equal(g[k], g2[k]) for k in g)
            _compare(f"{prec} {pol} bands unmixed {key}", prec, C.grad_theta_logpdf(ds, f, phi, theta), unmixed_w)
    finally:
        ds.host.pop("Cfs_bands")
        C.set_theta(ds)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_batch_slots(prec):
    """B = 2 with different slots: both against the reference; slot 0 of the B = 2 call is the B = 1 call bit for bit, in both forms (a slot's
    numbers do not depend on the other slots: the θ pass sums per slot in an order that does not know B, and the fields it reads from the
    ∇logpdf(Mixed) pipeline are made slot by slot)"""
    C, so, sd, _, (fo, po) = _pair(prec, "P", "64x64", B=2)
    ds, p = sd["ds"], sd["proj"]
    f, phi = _fields(C, so, sd)
    theta = THETAS["r+Aphi"]
    lp_w, mixed_w, unmixed_w = _ref("P", "64x64", 2, False, "r+Aphi")
    lp, g = C.grad_theta_logpdf_mixed(ds, fo, po, theta)
    u = C.grad_theta_logpdf(ds, f, phi, theta)
    assert lp.shape == (2,) and g["r"].shape == (2,)
    print()
    np.testing.assert_allclose(lp, lp_w, rtol=RT[prec])
    _compare(f"{prec} B=2 mixed", prec, g, mixed_w)
    _compare(f"{prec} B=2 unmixed", prec, u, unmixed_w)
    assert abs(g["Aphi"][0] - g["Aphi"][1]) > 1e-3 * abs(g["Aphi"][0])          # the slots really differ
    one = lambda x, b: C.Field(p, x.arr[b:b + 1].contiguous(), x.basis)
    u0 = C.grad_theta_logpdf(ds, one(f, 0), one(phi, 0), theta)
    assert all(np.array_equal(u[k][:1], u0[k]) for k in u)
    d = ds.d
    try:
        ds.set_data(one(d, 0))
        lp0, g0 = C.grad_theta_logpdf_mixed(ds, one(fo, 0), one(po, 0), theta)
    finally:
        ds.set_data(d)
    for k in g:
        print(f"[{prec}] slot 0 of B = 2 vs B = 1, mixed {k}: {g[k][0]!r} vs {g0[k][0]!r}")
        assert np.array_equal(g[k][:1], g0[k]), k


def _guarded(ds, fn, B, ncols, *args):
    """a direct call of the C ABI with an output array of exactly B * ncols doubles followed by a guard: (rows, the guard is untouched)"""
    pd = ctypes.POINTER(ctypes.c_double)
    buf = np.full(B * ncols + 64, 1.2345e300)
    from cmblensing_jl_amd.lib import check
    check(fn(*args, buf.ctypes.data_as(pd)))
    return buf[:B * ncols].reshape(B, ncols).copy(), bool(np.all(buf[B * ncols:] == 1.2345e300))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bands_installed_but_not_named(prec):
    """a model WITH bands, B = 2 and a θ that names r and Aϕ only: the result has rows of 2 doubles (the caller's namps = 0), not of 2 + Σ nbins --
    through grad_theta_logpdf, grad_theta_logpdf_mixed, the MUSE adapter and the C ABI with an exactly sized array.  Amplitudes that are not
    named are ones, so the reference is the one without bands"""
    C, so, sd, _, (fo, po) = _pair(prec, "P", "64x64", B=2)
    ds = sd["ds"]
    f, phi = _fields(C, so, sd)
    theta = THETAS["r+Aphi"]
    lp_w, mixed_w, unmixed_w = _ref("P", "64x64", 2, False, "r+Aphi")
    cls = {k: C.Cls(v.ell, v.cl) for k, v in so["cls"]["unlensed_scalar"].items()}
    C.use_bandpowers(ds, BANDS["P"][0], cls)
    print()
    try:
        lp, g = C.grad_theta_logpdf_mixed(ds, fo, po, theta)
        np.testing.assert_allclose(lp, lp_w, rtol=RT[prec])
        _compare(f"{prec} bands installed, mixed", prec, g, mixed_w)
        u = C.grad_theta_logpdf(ds, f, phi, theta)
        _compare(f"{prec} bands installed, unmixed", prec, u, unmixed_w)
        got = C.CMBLensingMuseProblem(ds, grad="device").grad_theta_logLike(ds.d, dict(f=f, phi=phi), theta)
        for k in theta:
            err = float(abs(got[k] - unmixed_w[k]["total"].sum()) / unmixed_w[k]["S"].sum())
            print(f"[{prec}] bands installed, MUSE grad=device {k}: |got - ref| / S = {err:.3e}")
            sample_close(f"{prec} bands installed muse {k}", err, RT[prec])
        # the C ABI itself: 2 doubles per slot are written and nothing behind them; with the amplitudes given (ones) the rows are 2 + 3 long
        vp = lambda x: ctypes.c_void_p(x.arr.data_ptr())
        fa, pa = f.arr.contiguous(), phi.arr.contiguous()
        pv = lambda a: ctypes.c_void_p(a.data_ptr())
        rows, clean = _guarded(ds, ds.lib.cmbl_grad_theta_logpdf, 2, 2, ds._h, pv(fa), pv(pa), 2, theta["r"], theta["Aphi"], None, 0, 3)
        assert clean and np.array_equal(rows[:, 0], u["r"]) and np.array_equal(rows[:, 1], u["Aphi"])
        ones = np.ones(3)
        rows5, clean = _guarded(ds, ds.lib.cmbl_grad_theta_logpdf, 2, 5, ds._h, pv(fa), pv(pa), 2, theta["r"], theta["Aphi"],
                                ones.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 3, 7)
        assert clean and np.all(rows5[:, 2:] != 0)
        np.testing.assert_allclose(rows5[:, :2], rows, rtol=1e-12)           # amplitudes of one are the fiducial covariance
        lpb = np.empty(2)
        ds.L.invalidate()
        rows, clean = _guarded(ds, ds.lib.cmbl_grad_theta_logpdf_mixed, 2, 2, ds._h, ds.L._h, vp(fo), vp(po), 2, theta["r"], theta["Aphi"], None, 0, 3,
                               lpb.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        assert clean and np.array_equal(lpb, lp) and np.array_equal(rows[:, 0], g["r"]) and np.array_equal(rows[:, 1], g["Aphi"])
    finally:
        ds.host.pop("Cfs_bands")
        C.set_theta(ds)


def test_error_returns():
    """CMBL_ERR_STATE before any model install; CMBL_ERR_ARG for the derivative of a parameter θ does not name (NaN r, NaN Aϕ, NULL amps);
    CMBL_ERR_SHAPE for a wrong namps"""
    import cmblensing_jl_amd as C
    from cmblensing_jl_amd.lib import check
    from cmblensing_jl_amd.theta import _install_theta_model
    from bench import synthetic_cls
    s = C.load_sim(3.0, (32, 32), "P", synthetic_cls(), T=torch.float32, beam_fwhm=1.0, Nphi="flat")
    ds = s["ds"]
    fo, po = ds.mix(s["f"], s["phi"])
    fo, po, f, phi = fo.to(C.MAP), po.to(C.FOURIER), s["f"].to(C.HARMONIC), s["phi"].to(C.FOURIER)
    pd = ctypes.POINTER(ctypes.c_double)
    vp = lambda x: ctypes.c_void_p(x.arr.data_ptr())
    dp = lambda a: None if a is None else a.ctypes.data_as(pd)
    nan = float("nan")
    lp, grad = np.empty(1), np.empty(8)

    def unmixed(r, A, amps, namps, want):
        check(ds.lib.cmbl_grad_theta_logpdf(ds._h, vp(f), vp(phi), 1, r, A, dp(amps), namps, want, dp(grad)))

    def mixed(r, A, amps, namps, want):
        check(ds.lib.cmbl_grad_theta_logpdf_mixed(ds._h, ds.L._h, vp(fo), vp(po), 1, r, A, dp(amps), namps, want, dp(lp), dp(grad)))

    def code(fn, *a):
        with pytest.raises(C.CmblError) as e:
            fn(*a)
        return e.value.code

    for fn in (unmixed, mixed):
        assert code(fn, 0.2, 1.0, None, 0, 3) == 5                   # CMBL_ERR_STATE
    C.use_bandpowers(ds, {"EE": (LE, "AEE")}, synthetic_cls()["unlensed_scalar"])
    _install_theta_model(ds)
    amps = np.ones(3)
    for fn in (unmixed, mixed):
        assert code(fn, nan, 1.0, amps, 3, 1) == 1                   # CMBL_ERR_ARG: d/dr with r not named
        assert code(fn, 0.2, nan, amps, 3, 2) == 1                   # d/dAϕ with Aϕ not named
        assert code(fn, 0.2, 1.0, None, 0, 4) == 1                   # d/d amplitudes without amplitudes
        assert code(fn, 0.2, 1.0, np.ones(2), 2, 7) == 2             # CMBL_ERR_SHAPE: the model has 3 bins
        fn(0.2, 1.0, amps, 3, 7)                                     # ... and the data set still works after the refusals
        assert np.all(np.isfinite(grad[:5]))
        fn(0.2, nan, None, 0, 1)                                     # what is not asked for may stay unnamed, and is written as 0
        assert grad[0] != 0 and grad[1] == 0


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_muse_problem_on_device(prec):
    """CMBLensingMuseProblem(grad="device"): in fp64 it agrees with the central differences of grad="fd" to their accuracy (the 1e-5 of
    tests/test_gpu_drivers.py, relative to S); in fp32, where the differences are unusable, it agrees with the reference to the class bound"""
    C, so, sd, _, _ = _pair(prec, "P", "64x64")
    ds = sd["ds"]
    f, phi = _fields(C, so, sd)
    z, d = dict(f=f, phi=phi), ds.d
    theta = dict(Aphi=1.0, r=0.2)
    ref = ThetaGradRef(so["ds"], so["Cfs"], so["Cten"])
    want = ref.unmixed(so["f"], so["phi"], r=0.2, Aphi=1.0)
    got = C.CMBLensingMuseProblem(ds, grad="device").grad_theta_logLike(d, z, theta)
    print()
    try:
        for k in theta:
            assert np.shape(got[k]) == ()
            err = float(abs(got[k] - want[k]["total"].sum()) / want[k]["S"].sum())
            print(f"[{prec}] MUSE grad=device {k}: {float(got[k]):+.9e}, |got - ref| / S = {err:.3e}")
            sample_close(f"{prec} muse device {k}", err, RT[prec])
        if prec == "f64":
            # the differences' own accuracy: at Aϕ = 1 the quadratic-form and the trace part of the derivative nearly cancel, and with the default
            # step of 1e-3 the truncation error of the central difference is 1.7e-4 of S (measured against the reference, which the device matches
            # to 4e-16); it falls as the step squared, so at 1e-4 it is 2e-6, below the 1e-5, with a rounding error of eps |lp| / h = 1e-8 of S
            fd = C.CMBLensingMuseProblem(ds, fd_step=1e-4).grad_theta_logLike(d, z, theta)
            for k in theta:
                err = float(abs(got[k] - fd[k]) / want[k]["S"].sum())
                print(f"[{prec}] MUSE device vs fd {k}: {err:.3e} of S")
                sample_close(f"{prec} muse device vs fd {k}", err, 1e-5)
    finally:
        C.set_theta(ds)
