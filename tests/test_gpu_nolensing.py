"""The flat-sky NoLensingDataSet on the device (d = M B f + n; src/dataset.jl:37-47, 68-73, 341-352; src/maximization.jl:17-42, 56-62, 235) against
the float64 oracle of tests/_nolensing_ref.py, in both forms of the engine:
  fused    : Dataset::nolens_adjoint, in the Wiener filter inside CgSolver::solve_fused, with PwNlAp (pixel mask) or PwNlDiag (none) -- power-of-two maps, the default
  composed : the identity NoLens<T> in the L slot of the composed paths (here: option fused_harm off, CMBL_NO_FUSED_HARM=1; any-size maps always)
Shapes (Ny, Nx): 32 x 32, 32 x 64, 64 x 32 (the smallest the fused kernels take, non-square both ways, Nyh = 17 / 33 leave a tail row group) in both
forms, 24 x 40 composed; I / P / IP; f32 and f64; B = 2, and B = 17 at 32 x 32 P (the B > 16 branch of PwCgP).  tests/test_nolensing_ref.py pins
every fixture used here on the CPU (history lengths with their margins, the closed form without a mask).
Bounds (tests/_nolensing_ref.bound): double precision the class bounds of test_gpu_parity.test_dataset_gradientf_and_wiener (scalars 1e-8, fields
1e-9); single precision max(class bound 1e-3 / 4e-6, 3 x the float32 oracle's own distance from the float64 oracle, which
tests/golden/nolensing_budget.json records per case and quantity).  Every comparison prints its figure; measured: profiles/nolensing_parity.txt."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as O
import _nolensing_ref as N
from test_gpu_cg_rules import _form_env, ERR_NAN
from test_gpu_parity import DT, _pkg

PRECS, FORMS = ["f32", "f64"], ["fused", "composed"]
SHAPE_FORMS = [(s, f) for s in N.POW2 for f in FORMS] + [(N.ANYSIZE, "composed")]
FLOW_CLASSES = {"x_grad", "flow_y_fwd", "adj_y", "adj_x", "delta_cols", "delta_rows", "gradhess_mult", "dphi_reduce", "dphi_combine"}
ERR_ARG = 1                                                  # CMBL_ERR_ARG (include/cmblens.h)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nolensing_budget.json")) as _f:
    BUDGET = json.load(_f)


def _cls(ref):
    C = _pkg()
    return {g: {k: C.Cls(v.ell, v.cl) for k, v in ref["so"]["cls"][g].items()} for g in ("unlensed_scalar", "tensor", "total")}


def check(what, err, bnd):
    """one line per comparison (collected into profiles/nolensing_parity.txt), then the assertion"""
    print(f"nolensing_parity {what} err {err:.3e} bound {bnd:.3e}")
    assert err <= bnd, (what, err, bnd)


class Device:
    """the device data set of one (precision, pol, shape, form, batch size, mask), made once by load_nolensing_sim; d is the oracle's"""

    def __init__(self, prec, pol, shape, form, B=2, mask=True):
        self.C = C = _pkg()
        self.prec, self.pol, self.shape, self.form, self.B, self.mask = prec, pol, shape, form, B, mask
        self.case = N.case_key(pol, shape, B, mask)
        self.ref = ref = N.sim(pol, shape, np.float64, B, mask)
        with _form_env(form):
            self.sd = C.load_nolensing_sim(N.THETA, shape, pol, _cls(ref), T=DT[prec][0], beam_fwhm=N.BEAM, pixel_mask=N.PM if mask else None, Nbatch=B)
        self.ds, self.p = self.sd["ds"], self.sd["proj"]
        self.fused = form == "fused" and shape != N.ANYSIZE
        assert bool(self.p.get_option("fused_harm")) == (form == "fused")
        self.d, self.f = self.field(ref["d"]), self.field(ref["f"])

    def field(self, a):
        return self.C.Field(self.p, self.p.tensor(np.array(a)), self.C.HARMONIC)

    def bound(self, run, q):
        return N.bound(BUDGET, self.prec, self.case, run, q)

    def solve(self, nsteps, tol=0.0, d=None):
        """(iterate tensor (B, P, Nx, Nyh), history (length, B))"""
        fw, hist = self.ds.argmaxf_logpdf(d=self.d if d is None else d, tol=tol, nsteps=nsteps)
        return fw.arr, np.array([r for _, r in hist]).reshape(len(hist), -1)

    def launches(self, nsteps):
        """{kernel class: launches} of one solve of `nsteps` steps at tol = 0"""
        self.p.prof_enable()
        self.p.prof_reset()
        self.solve(nsteps)
        table = self.p.prof_table()
        self.p.prof_enable(False)
        return {k: n for k, (_, n) in table.items()}


_devices = {}


def device(prec, pol, shape, form, B=2, mask=True):
    key = (prec, pol, tuple(shape), form, B, mask)
    if key not in _devices:
        _devices[key] = Device(prec, pol, tuple(shape), form, B, mask)
    return _devices[key]


def against_oracle(dev, run, x, hist, xo, ho):
    assert hist.shape == ho.shape, (hist.shape, ho.shape)
    check(f"{dev.case} {dev.prec} {dev.form} {run} hist", N.distance("hist", hist, ho), dev.bound(run, "hist"))
    check(f"{dev.case} {dev.prec} {dev.form} {run} x", N.distance("x", x.cpu().numpy(), xo), dev.bound(run, "x"))


@pytest.mark.parametrize("shape,form", SHAPE_FORMS)
@pytest.mark.parametrize("pol", N.POLS)
@pytest.mark.parametrize("prec", PRECS)
def test_model_against_the_reference(prec, pol, shape, form):
    """gradientf_logpdf(f, d), mean(f), logpdf(f) and the one-pass logpdf with its gradient; d = None reads the data of the data set"""
    dev = device(prec, pol, shape, form)
    ds, ods, ref = dev.ds, dev.ref["ds"], dev.ref
    tag = f"{dev.case} {prec} {form}"
    want_g = ods.gradientf_logpdf(ref["f"], N.IDENTITY, ref["d"])
    g = ds.gradientf_logpdf(dev.f, dev.d)
    check(f"{tag} gradientf_logpdf", N.distance("x", g.arr.cpu().numpy(), want_g), dev.bound("model", "grad"))
    ds.set_data(dev.d)
    assert torch.equal(ds.gradientf_logpdf(dev.f).arr, g.arr)
    check(f"{tag} gradientf_logpdf(zero_d)", N.distance("x", ds.gradientf_logpdf(dev.f, zero_d=True).arr.cpu().numpy(),
                                                        ods.gradientf_logpdf(ref["f"], N.IDENTITY, np.zeros_like(ref["d"]))), dev.bound("model", "grad"))
    check(f"{tag} mean", N.distance("x", ds.mean(dev.f).arr.cpu().numpy(), ods.mean(N.IDENTITY, ref["f"])), dev.bound("model", "mean"))
    want_lp = ods.logpdf(ref["f"])
    lp = ds.logpdf(dev.f)
    check(f"{tag} logpdf", N.distance("hist", lp, want_lp), dev.bound("model", "logpdf"))
    lp2, g2 = ds.logpdf_and_gradient(dev.f, dev.d)
    assert np.array_equal(lp, lp2)
    check(f"{tag} logpdf_and_gradient", N.distance("x", g2.arr.cpu().numpy(), want_g), dev.bound("model", "grad"))
    # logdet_sum enters as it is set
    ds.set_logdet(ds.logdet_sum + 2.0)
    assert np.allclose(ds.logpdf(dev.f), lp - 1.0, rtol=1e-12, atol=0)
    ds.set_logdet(ds.logdet_sum - 2.0)


@pytest.mark.parametrize("shape", N.POW2)
@pytest.mark.parametrize("pol", N.POLS)
@pytest.mark.parametrize("prec", PRECS)
def test_imaginary_parts_in_self_conjugate_modes_fused_against_composed(prec, pol, shape):
    """a spectrum no real map has: the fused form projects the Hermitian rows on its way to the pixel mask, as the composed form's c2r does"""
    fu, co = device(prec, pol, shape, "fused"), device(prec, pol, shape, "composed")
    f = fu.field(N.with_imag_selfconj(fu.ref["f"]))
    a, b = fu.ds.gradientf_logpdf(f, fu.d).arr.cpu().numpy(), co.ds.gradientf_logpdf(co.field(N.with_imag_selfconj(co.ref["f"])), co.d).arr.cpu().numpy()
    check(f"{fu.case} {prec} imag-selfconj fused-vs-composed gradientf", N.distance("x", a, b), fu.bound("model", "grad"))
    clean = fu.ds.gradientf_logpdf(fu.f, fu.d).arr.cpu().numpy()
    assert N.distance("x", a, clean) > 1e-3                  # the input really differs


@pytest.mark.parametrize("shape,form", SHAPE_FORMS)
@pytest.mark.parametrize("pol", N.POLS)
@pytest.mark.parametrize("prec", PRECS)
def test_eight_steps_against_the_reference(prec, pol, shape, form):
    dev = device(prec, pol, shape, form)
    x, h = dev.solve(N.NSHORT)
    against_oracle(dev, f"n{N.NSHORT}", x, h, *N.solve(pol, shape, np.float64, 2, True, N.NSHORT, 0.0))
    x2, h2 = dev.solve(N.NSHORT)                             # a repeated solve is bit-identical
    assert torch.equal(x, x2) and np.array_equal(h, h2)
    if dev.fused:                                            # the two forms agree within the bound
        xc, hc = device(prec, pol, shape, "composed").solve(N.NSHORT)
        check(f"{dev.case} {prec} fused-vs-composed hist", N.distance("hist", h, hc), dev.bound(f"n{N.NSHORT}", "hist"))
        check(f"{dev.case} {prec} fused-vs-composed x", N.distance("x", x.cpu().numpy(), xc.cpu().numpy()), dev.bound(f"n{N.NSHORT}", "x"))
    # MAP_joint of a NoLensingDataSet is its Wiener filter (src/maximization.jl:235)
    dev.ds.set_data(dev.d)
    f, phi = dev.C.MAP_joint(dev.ds, cg_tol=0.0, cg_nsteps=N.NSHORT)
    assert phi is None and torch.equal(f.arr, x)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape,B", sorted(N.STOPS))
@pytest.mark.parametrize("prec", PRECS)
def test_pol_P_stops_at_the_length_of_the_table(prec, shape, B, form):
    if shape == N.ANYSIZE and form == "fused":
        return                                               # an any-size map runs the composed form whatever the option: one case, not two
    dev = device(prec, "P", shape, form, B=B)
    x, h = dev.solve(500, tol=N.TOL)
    print("stopped", dev.case, prec, form, len(h), h[-2:].max(axis=1))
    assert len(h) == N.STOPS[(shape, B)][0], (len(h), N.STOPS[(shape, B)])
    against_oracle(dev, "tol", x, h, *N.solve("P", shape, np.float64, B, True, 500, N.TOL))
    xn, hn = dev.solve(len(h))                               # what was enqueued past the stop changed nothing
    assert torch.equal(x, xn) and np.array_equal(h, hn)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pol", N.POLS)
@pytest.mark.parametrize("prec", PRECS)
def test_without_a_mask_one_step_reaches_the_closed_form(prec, pol, form):
    """the preconditioner is the inverse of the operator: default tol, a history of length 2.  (Not run past its stop at tol = 0: the residual is
    exactly 0 there in float32.)"""
    dev = device(prec, pol, (32, 32), form, mask=False)
    fw, hist = dev.ds.argmaxf_logpdf(d=dev.d)
    h = np.array([r for _, r in hist])
    xo, ho = N.solve(pol, (32, 32), np.float64, 2, False, 500, N.TOL)
    assert len(h) == len(ho) == 2 and np.all(h[1] < N.TOL)
    check(f"{dev.case} {prec} {form} first residual", N.distance("hist", h[:1], ho[:1]), dev.bound("tol", "hist"))
    check(f"{dev.case} {prec} {form} x", N.distance("x", fw.arr.cpu().numpy(), xo), dev.bound("tol", "x"))
    check(f"{dev.case} {prec} {form} closed form", N.distance("x", fw.arr.cpu().numpy(), N.closed_form(dev.ref["ds"], dev.ref["d"])), dev.bound("tol", "x"))
    fw2, hist2 = dev.ds.argmaxf_logpdf(d=dev.d)
    assert torch.equal(fw.arr, fw2.arr) and np.array_equal(h, np.array([r for _, r in hist2]))


@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("pol", N.POLS)
@pytest.mark.parametrize("prec", PRECS)
def test_the_form_really_runs(prec, pol, mask):
    """fused: row-carrier (with a mask) or flat-carrier launches and no flow kernel, at most 7 launches per iteration with a pixel mask and 3
    without (the difference of two solves of different nsteps); composed: no row-carrier launch and no flow kernel either"""
    n0, n1 = (3, 7) if mask else (2, 2)
    fu, co = device(prec, pol, (32, 32), "fused", mask=mask), device(prec, pol, (32, 32), "composed", mask=mask)
    a = fu.launches(n1)
    assert not FLOW_CLASSES & set(a), sorted(a)
    assert ("x_harm" in a) == mask and "harm_dot" in a and "cg_update" in a, sorted(a)
    c = co.launches(n1)
    assert "x_harm" not in c and not FLOW_CLASSES & set(c) and "cg_update" in c, sorted(c)
    if mask:
        b = fu.launches(n0)
        per_it = (sum(a.values()) - sum(b.values())) / (n1 - n0)
        cper = (sum(c.values()) - sum(co.launches(n0).values())) / (n1 - n0)
        print("launches per iteration", fu.case, prec, "fused", per_it, "composed", cper)
        assert per_it <= 7 and per_it == int(per_it), (per_it, a, b)
        assert cper > per_it
    else:
        # a no-mask solve is not run past its stop: the one iteration it has is what remains when the launches of the start are taken off, and those
        # are the launches of a solve of a single step (nsteps = 1: no iteration)
        b = fu.launches(1)
        per_it = sum(a.values()) - sum(b.values())
        print("launches per iteration", fu.case, prec, "fused", per_it)
        assert per_it <= 3, (per_it, a, b)


@pytest.mark.parametrize("pol", N.POLS)
@pytest.mark.parametrize("prec", PRECS)
def test_equals_a_lensing_data_set_with_a_flow_at_zero_phi(prec, pol):
    """what one had to run before: a BaseDataSet with a LenseFlow at ϕ = 0 on the same operators"""
    dev = device(prec, pol, (32, 32), "fused")
    C = dev.C
    sd = C.load_sim(N.THETA, (32, 32), pol, _cls(dev.ref), T=DT[prec][0], beam_fwhm=N.BEAM, pixel_mask=N.PM, Nbatch=2, Nphi="flat")
    phi0 = C.Field(sd["proj"], torch.zeros_like(sd["phi"].arr), C.FOURIER)
    d = C.Field(sd["proj"], sd["proj"].tensor(np.array(dev.ref["d"])), C.HARMONIC)
    fw, hist = sd["ds"].argmaxf_logpdf(phi0, d=d, tol=0.0, nsteps=N.NSHORT)
    x, h = dev.solve(N.NSHORT)
    check(f"{dev.case} {prec} flow(0) hist", N.distance("hist", h, np.array([r for _, r in hist])), dev.bound(f"n{N.NSHORT}", "hist"))
    check(f"{dev.case} {prec} flow(0) x", N.distance("x", x.cpu().numpy(), fw.arr.cpu().numpy()), dev.bound(f"n{N.NSHORT}", "x"))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pol", N.POLS)
@pytest.mark.parametrize("prec", PRECS)
def test_sample_f_from_injected_white_draws(prec, pol, form):
    dev = device(prec, pol, (32, 32), form)
    wf, wn = N.whites(pol, (32, 32))
    want, ho = dev.ref["ds"].sample_f(wf, wn, tol=0.0, nsteps=N.NSHORT)
    dev.ds.set_data(dev.d)
    got, hist = dev.C.sample_f(dev.ds, None, wf, wn, tol=0.0, nsteps=N.NSHORT)
    assert len(hist) == len(ho) == N.NSHORT
    check(f"{dev.case} {prec} {form} sample_f", N.distance("x", got.arr.cpu().numpy(), want), dev.bound("sample_f", "x"))
    # ... and simulate_data from the same draws is the reference's d = M B f + n
    ods = dev.ref["ds"]
    ct = np.complex128
    dsim = ods.mean(N.IDENTITY, ods.Cf.sqrt()(O.flatsky.rfft2(wf).astype(ct))) + ods.Cn.sqrt()(O.flatsky.rfft2(wn).astype(ct))
    check(f"{dev.case} {prec} {form} simulate_data", N.distance("x", dev.ds.simulate_data(wf, wn).arr.cpu().numpy(), dsim), dev.bound("model", "mean"))


@pytest.mark.parametrize("prec", PRECS)
def test_load_nolensing_sim_makes_the_data_and_covariance_it_says(prec):
    dev = device(prec, "P", (32, 32), "fused")
    C, ref = dev.C, dev.ref
    simtol = 2.5e-6 if prec == "f32" else 1e-10                # the class bound of a simulated d (test_gpu_parity.test_dataset_gradientf_and_wiener)
    # default: d = M B f + n, Cf unlensed, logdet Cf + logdet Cn
    check(f"{prec} simulated d", N.distance("x", dev.sd["d"].arr.cpu().numpy(), ref["d"]), simtol)
    assert dev.sd["ftilde"].basis == C.MAP and torch.equal(dev.sd["ftilde"].arr, dev.sd["f"].to(C.MAP).arr)       # L = I: f~ is f, as a map
    ods = ref["ds"]
    # (a float32 context hands out its multipoles rounded to float32, 6e-8: a spectrum falling like l^-10 moves by 6e-7, against |log C| ~ 10 per mode)
    want_logdet = float(np.squeeze(ods.Cf.logdet(ods.proj) + ods.Cn.logdet(ods.proj)))
    assert dev.ds.logdet_sum == pytest.approx(want_logdet, rel=2e-7 if prec == "f32" else 1e-9)
    assert np.allclose(dev.ds.ops["Cf_inv"].cpu().numpy(), ods.Cf.pinv().d, rtol=2e-6 if prec == "f32" else 1e-12, atol=0)
    assert "Cphi_inv" not in dev.ds.ops and "D" not in dev.ds.ops and "G_inv" not in dev.ds.ops
    # lensed_data: the data of the lensing model on the same draws; lensed_covariance: Cf = Cf~ in the prior and in the preconditioner
    sl = C.load_nolensing_sim(N.THETA, (32, 32), "P", _cls(ref), lensed_covariance=True, lensed_data=True, T=DT[prec][0], beam_fwhm=N.BEAM, pixel_mask=N.PM, Nbatch=2)
    check(f"{prec} simulated lensed d", N.distance("x", sl["d"].arr.cpu().numpy(), ref["so"]["d"]), simtol)
    assert N.distance("x", sl["d"].arr.cpu().numpy(), ref["d"]) > 1e-2
    lens = ref["so"]["ds"]
    assert np.allclose(sl["ds"].ops["Cf_inv"].cpu().numpy(), lens.Cftilde.pinv().d, rtol=2e-6 if prec == "f32" else 1e-12, atol=0)
    want_pre = (lens.Cftilde.pinv() + (lens.Bhat.T_() @ lens.Mfhat.T_() @ lens.Cnhat.pinv() @ lens.Mfhat @ lens.Bhat)).pinv().d
    assert np.allclose(sl["ds"].ops["precond_inv"].cpu().numpy(), want_pre, rtol=2e-6 if prec == "f32" else 1e-12, atol=0)
    assert isinstance(sl["ds"].L, C.IdentityLens) and isinstance(sl["ds"], C.NoLensingDataSet)
    with pytest.raises(TypeError):
        C.load_nolensing_sim(N.THETA, (32, 32), "P", _cls(ref), L=C.BilinearLens)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("prec", PRECS)
def test_a_slot_of_zero_data_is_a_nan_error_and_leaves_nothing_behind(prec, form):
    """d[1] = 0: res = r'z = 0 in slot 1, alpha = 0 / 0 at step 2 and the residual is NaN from there.  The solve returns CMBL_ERR_NAN and the next
    valid solve on the same data set is the one before it, bit for bit (as in tests/test_gpu_cg_rules.py)."""
    dev = device(prec, "I", (32, 32), form)
    before = dev.solve(N.NSHORT)
    d0 = dev.field(dev.ref["d"])
    d0.arr[1] = 0
    with pytest.raises(dev.C.CmblError) as e:
        dev.solve(20, d=d0)
    assert e.value.code == ERR_NAN and "NaN residual" in str(e.value), str(e.value)
    after = dev.solve(N.NSHORT)
    assert torch.equal(before[0], after[0]) and np.array_equal(before[1], after[1])


@pytest.mark.parametrize("prec", PRECS)
def test_identity_in_a_lensing_data_set_has_no_pullback(prec):
    """cmbl_grad_logpdf_op with the identity and a gphi_out is CMBL_ERR_ARG; the value and the gradient with respect to f are the no-lensing ones
    (logpdf up to the ϕ terms, which at ϕ = 0 are logdet Cϕ / 2)"""
    dev = device(prec, "P", (32, 32), "fused")
    C = dev.C
    sd = C.load_sim(N.THETA, (32, 32), "P", _cls(dev.ref), T=DT[prec][0], beam_fwhm=N.BEAM, pixel_mask=N.PM, Nbatch=2, Nphi="flat", L=C.IdentityLens)
    ds, p = sd["ds"], sd["proj"]
    assert isinstance(ds.L, C.IdentityLens)
    F = lambda a, b: C.Field(p, p.tensor(np.array(a)), b)
    f, d = F(dev.ref["f"], C.HARMONIC), F(dev.ref["d"], C.HARMONIC)
    phi0 = C.Field(p, torch.zeros_like(sd["phi"].arr[:1]), C.FOURIER)
    with pytest.raises(C.CmblError) as e:
        ds.grad_logpdf(f, phi0, d)
    assert e.value.code == ERR_ARG and "Identity" in str(e.value) and "pullback" in str(e.value), str(e.value)
    lp, gf, gp = ds.grad_logpdf(f, phi0, d, want_phi=False)
    assert gp is None
    check(f"{prec} grad_logpdf_op(identity) gf", N.distance("x", gf.arr.cpu().numpy(), dev.ref["ds"].gradientf_logpdf(dev.ref["f"], N.IDENTITY, dev.ref["d"])),
          dev.bound("model", "grad"))
    nl = dev.ds.logpdf(dev.f, dev.d)
    assert np.allclose(lp - nl, (dev.ds.logdet_sum - ds.logdet_sum) / 2, rtol=0, atol=(1e-3 if prec == "f32" else 1e-8) * np.abs(nl).max())
    for what, call in (("MAP_joint", lambda: C.MAP_joint(ds)), ("gradient_logpdf_mixed", lambda: ds.gradient_logpdf_mixed(f, phi0))):
        with pytest.raises(NotImplementedError, match=r"pullback of `L \\ f`"):
            call()
