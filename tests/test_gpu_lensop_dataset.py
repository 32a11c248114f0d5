r"""GPU parity of a data set with another operator than LenseFlow in its `L` slot (`load_sim(L = BilinearLens)`, src/dataset.jl:223, 306, 333;
src/bilinearlens.jl:10-17): Wiener filter, ∇f, logpdf, ∇ϕ, logpdf_mixed and MAP_marg through `cmbl_gradientf_logpdf_op`, `cmbl_wiener_cg_op`,
`cmbl_grad_logpdf_op`, against tests/_lensop_ds_ref.py (the oracle's data set over tests/_bilinear_ref.py / tests/_powerlens_ref.py) on identical
inputs.

Tolerances.  float64: the literal class bounds of the LenseFlow data-set tests (tests/test_gpu_parity.py, tests/test_gpu_drivers.py).  float32:
3 x the figure of that case and quantity in tests/golden/lensop_dataset_budget.json -- the distance of the CPU restatement in float32 from the same
in float64 (tools/make_lensop_dataset_budget.py), never a figure of the device.  Every comparison goes through tests/_tol.py.

Cases (tests/_lensop_ds_ref.py CASES): A 64 x 128 QU, beam, border mask, two data slots against one ϕ of 0.7 px rms (the power-of-two path, fused
and composed); B 36 x 60 I with mask (any-size composition); C 32 x 64 IP with mask (P = 3, the TE block next to the lens); D 32 x 64 QU with
`set_deflection` of 6 px rms (positions wrap more than once across both edges inside the fused loader)."""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _lensop_ds_ref as R
from _tol import close, rel, scalars_close

DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
# float64 class bounds: gradientf 4e-10, 8-step residuals 1e-8, 8-step iterate 1e-9, logpdf 1e-10 (tests/test_gpu_parity.py:312-330, LPTOL),
# ∂logpdf/∂ϕ 1e-9, MAP_marg 1e-7 (tests/test_gpu_drivers.py:242, 263-265), converged solve 1e-4 (tests/test_gpu_parity.py:322)
F64 = dict(gradf=4e-10, hist=1e-8, hist2=1e-8, wf=1e-9, wf2=1e-9, logpdf=1e-10, logpdf_mixed=1e-10, gradphi=1e-9, wf_conv=1e-4, phi1=1e-7, phi2=1e-7, g_norm=1e-7)
BUDGET = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lensop_dataset_budget.json")))["cases"]


def tol(prec, case, q):
    return F64[q] if prec == "f64" else 3 * BUDGET[case][q]


def check(prec, case, q, got, ref=None):
    want = (ref if ref is not None else R.reference()[case])[q]
    got = got.arr.cpu().numpy() if hasattr(got, "arr") else np.asarray(got)
    e = (scalars_close((case, q), got, want, rtol=tol(prec, case, q)) if q in R.SCALARS else close((case, q), got, want, tol(prec, case, q)))
    print(f"{prec} {case} {q}: {e:.3e} (tolerance {tol(prec, case, q):.2e})")


def _pkg():
    import cmblensing_jl_amd as C
    return C


_dev = {}


def device(prec, case, L=None):
    """(C, load_sim dict) of a case on the device in precision `prec` with `L` in the slot (default BilinearLens) and the reference's data set;
    one per (prec, case, operator), shared by the tests"""
    C = _pkg()
    key = (prec, case, L)
    if key not in _dev:
        Nside, pol, mask, B = R.CASES[case]
        so = R.sim(case)
        cls = {g: {k: C.Cls(v.ell, v.cl) for k, v in so["cls"][g].items()} for g in ("unlensed_scalar", "tensor", "total")}
        make = {None: C.BilinearLens, "PowerLens4": lambda p: C.PowerLens(p, 4), "Taylens3": lambda p: C.Taylens(p, 3), "LenseFlow": None}[L]
        # (one slot: load_sim draws a ϕ per slot, and BilinearLens / PowerLens refuse a batched ϕ as the reference's do; the tests pass B slots of f and d)
        sd = C.load_sim(3.0, Nside, pol, cls, T=DT[prec][0], beam_fwhm=3.0, pixel_mask=R.PM if mask else None, Nbatch=1, Nphi=so["ds"].Nphi * 2, L=make)
        _dev[key] = sd
    return C, _dev[key]


def fields(C, sd, case, ref_case=None):
    """the reference's f, ϕ and data of a case as device Fields (rounded to the device's precision); the data set takes the data"""
    p, so = sd["proj"], R.sim(case)
    F = lambda a, b: C.Field(p, p.tensor(a), b)
    d = F(R.reference()[ref_case or case]["d"], C.HARMONIC)
    sd["ds"].set_data(d)
    return F, F(so["f"], C.HARMONIC), F(so["phi"], C.FOURIER), d


def hist_array(h):
    return np.array([np.atleast_1d(r) for _, r in h])


def run_case(prec, case, fused):
    C, sd = device(prec, case)
    ds, p = sd["ds"], sd["proj"]
    assert isinstance(ds.L, C.BilinearLens)
    p.set_option("lens_fused", fused)
    try:
        F, f, phi, d = fields(C, sd, case)
        check(prec, case, "gradf", ds.gradientf_logpdf(f, phi))
        fw, h = ds.argmaxf_logpdf(phi, tol=0.0, nsteps=8)
        assert len(h) == 8
        check(prec, case, "wf", fw)
        check(prec, case, "hist", hist_array(h))
        # the restart and ∇ϕ from the reference's 8-iteration iterate: identical inputs on both sides
        fw_ref = F(R.reference()[case]["wf"], C.HARMONIC)
        fw2, h2 = ds.argmaxf_logpdf(phi, fstart=fw_ref, tol=0.0, nsteps=8)
        check(prec, case, "wf2", fw2)
        check(prec, case, "hist2", hist_array(h2))
        check(prec, case, "logpdf", ds.logpdf(f, phi))
        check(prec, case, "gradphi", ds.gradientphi_logpdf(fw_ref, phi))
        lp, gf, gp = ds.grad_logpdf(f, phi)
        check(prec, case, "logpdf", lp)
        check(prec, case, "gradf", gf)
        assert gp.arr.shape[0] == f.arr.shape[0]
    finally:
        p.set_option("lens_fused", 0)
    return C, sd


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_case_A_power_of_two_with_mask_two_slots(prec, fused):
    C, sd = run_case(prec, "A", fused)
    ds, p = sd["ds"], sd["proj"]
    p.set_option("lens_fused", fused)
    try:
        F, f, phi, d = fields(C, sd, "A")
        ref = R.reference()["A"]
        fw, h = ds.argmaxf_logpdf(phi, tol=1e-1, nsteps=500)
        n = ref["n_conv"]
        assert abs(len(h) - n) <= (1 if prec == "f64" else max(2, n // 20)), (len(h), n)
        check(prec, "A", "wf_conv", fw)
        # logpdf_mixed (value): unmix through the operator's own gmres
        check(prec, "A", "logpdf_mixed", ds.logpdf_mixed(F(ref["mix_f"], C.MAP), F(ref["mix_phi"], C.FOURIER)))
    finally:
        p.set_option("lens_fused", 0)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", ["B", "C"])
def test_cases_B_C_any_size_and_three_components(prec, case):
    run_case(prec, case, 1)                                              # B: the switch must not matter on the any-size path


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_case_D_large_deflection_wraps_both_edges(prec, fused):
    C, sd = device(prec, "D")
    ds, p = sd["ds"], sd["proj"]
    Ny, Nx = R.CASES["D"][0]
    dy, dx = R.big_deflection(Ny, Nx)
    for dd, N, ax in ((dy, Ny, 1), (dx, Nx, 0)):                       # positions leave the map across both edges of both axes
        pos = dd + np.arange(N).reshape((1, N) if ax == 1 else (N, 1))
        assert (pos < -1).any() and (pos > N).any()
    p.set_option("lens_fused", fused)
    try:
        F, f, phi, d = fields(C, sd, "D")
        ds.L.set_deflection(dy, dx)
        check(prec, "D", "gradf", ds.gradientf_logpdf(f, None))
        fw, h = ds.argmaxf_logpdf(None, tol=0.0, nsteps=8)
        check(prec, "D", "wf", fw)
        check(prec, "D", "hist", hist_array(h))
    finally:
        p.set_option("lens_fused", 0)


@pytest.mark.parametrize("spb", [1, 4])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_map_marg_two_steps(prec, spb):
    """two MAP_marg steps (src/maximization.jl:245-343) with injected white noise against the same loop over the reference helper"""
    C, sd = device(prec, "A")
    ds, p = sd["ds"], sd["proj"]
    F, f, phi, d = fields(C, sd, "A")
    ods = R.sim("A")["ds"]
    ds.set_data(C.Field(p, d.arr[:1].contiguous(), C.HARMONIC))
    ds.host["Nphi"] = ods.Nphi
    (Ny, Nx), P = R.CASES["A"][0], ds.P
    wf, wn = R.whites(P, Nx, Ny)
    try:
        phi_g, tr = C.MAP_marg(ds, Nsims=R.NSIMS, sims_per_batch=spb, whites={C.rng.STREAM_F: wf, C.rng.STREAM_N: wn}, **R.MARG_KW)
    finally:
        ds.set_data(d)
    case = f"A/MAP_marg{spb}"
    assert [len(t["ncg"]) for t in tr] == [1 + R.NSIMS // spb, 1]
    check(prec, case, "phi1", tr[0]["phi"], R.reference()[case])
    check(prec, case, "phi2", phi_g, R.reference()[case])
    check(prec, case, "g_norm", [t["g_norm"] for t in tr], R.reference()[case])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_powerlens_in_the_slot(prec):
    case = "A/PowerLens4"
    C, sd = device(prec, "A", "PowerLens4")
    ds = sd["ds"]
    assert isinstance(ds.L, C.PowerLens) and ds.L.order == 4
    F, f, phi, d = fields(C, sd, "A", case)
    ref = R.reference()[case]
    check(prec, case, "gradf", ds.gradientf_logpdf(f, phi), ref)
    fw, h = ds.argmaxf_logpdf(phi, tol=0.0, nsteps=8)
    check(prec, case, "wf", fw, ref)
    check(prec, case, "hist", hist_array(h), ref)
    # the reference has no pullback of PowerLens with respect to ϕ: refused, not approximated
    with pytest.raises(C.CmblError) as e:
        ds.gradientphi_logpdf(fw, phi)
    assert e.value.code == 1 and "pullback" in str(e.value)
    lp, gf, gp = ds.grad_logpdf(f, phi, want_phi=False)                  # value and ∇f are defined
    assert gp is None and np.all(np.isfinite(lp))
    close((case, "gradf from grad_logpdf"), gf.arr.cpu().numpy(), ref["gradf"], tol(prec, case, "gradf"))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_taylens_in_the_slot_has_mean_and_logpdf_only(prec):
    C, sd = device(prec, "A", "Taylens3")
    ds = sd["ds"]
    F, f, phi, d = fields(C, sd, "A")
    import oracle as O
    ods = R.LensOpDataSet.of(R.sim("A")["ds"], "Taylens", order=3)
    so = R.sim("A")
    want_mu = ods.mean(ods.L(so["phi"]), so["f"])
    want_lp = np.atleast_1d(ods.logpdf(so["f"], so["phi"], R.reference()["A"]["d"]))
    # bounds: the class bounds of the LenseFlow data-set tests for simulated data (2.5e-6 / 1e-10) and logpdf (5e-8 / 1e-10), tests/test_gpu_parity.py:29, 304
    close("Taylens mean", ds.mean(f, phi).arr.cpu().numpy(), want_mu, 2.5e-6 if prec == "f32" else 1e-10)
    scalars_close("Taylens logpdf", ds.logpdf(f, phi), want_lp, rtol=5e-8 if prec == "f32" else 1e-10)
    for call in (lambda: ds.gradientf_logpdf(f, phi), lambda: ds.argmaxf_logpdf(phi, tol=0.0, nsteps=2), lambda: ds.grad_logpdf(f, phi, want_phi=False),
                 lambda: ds.grad_logpdf(f, phi, want_f=False)):
        with pytest.raises(C.CmblError) as e:
            call()
        assert e.value.code == 1, str(e.value)                          # CMBL_ERR_ARG


# one shape per compiled column class of the fused pass (Ny = 32 ... 4096), and both orientations of the smallest
FUSED_SHAPES = [(32, 64), (64, 32), (128, 32), (256, 32), (512, 32), (1024, 32), (2048, 32), (4096, 32)]
_fs = {}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx", FUSED_SHAPES)
def test_fused_column_pass_against_the_composition(Ny, Nx, prec, B):
    """one gradientf_logpdf with lens_fused = 1 and with 0: the two differ by how ~7 roundings of one four-term sum are contracted, the transform
    behind them is the same code -- relative L2 below 16 eps; and two fused runs are bit-identical (the sorted CSR of L', no float atomics)"""
    C = _pkg()
    from bench import synthetic_cls
    if (Ny, Nx, prec) not in _fs:
        _fs.clear()                                                      # one resident data set at a time
        _fs[(Ny, Nx, prec)] = C.load_sim(3.0, (Ny, Nx), "P", synthetic_cls(), T=DT[prec][0], beam_fwhm=3.0, Nbatch=1, Nphi="flat", L=C.BilinearLens)
    s = _fs[(Ny, Nx, prec)]
    ds, p = s["ds"], s["proj"]
    # B distinct slots against the one ϕ: the simulated field and data, and copies shifted along x and rescaled
    slots = lambda a: torch.cat([torch.roll(a, 3 * b, dims=2) * (1.0 + 0.25 * b) for b in range(B)]).contiguous()
    f, d, phi = C.Field(p, slots(s["f"].arr), C.HARMONIC), C.Field(p, slots(s["d"].arr), C.HARMONIC), s["phi"]
    out, launches = {}, {}
    try:
        for fused in (0, 1, 1):
            p.set_option("lens_fused", fused)
            p.prof_reset()
            p.prof_enable(True)
            out.setdefault(fused, []).append(ds.gradientf_logpdf(f, phi, d=d).arr.clone())
            p.prof_enable(False)
            launches[fused] = p.prof_table().get("lens_y", (0.0, 0))[1]
    finally:
        p.prof_enable(False)
        p.set_option("lens_fused", 0)
    assert launches == {0: 0, 1: 2}, launches                            # the fused pass ran: once for L, once for L' -- and only under the option
    eps = float(np.finfo(DT[prec][1]).eps)
    e = rel(out[1][0].cpu().numpy(), out[0][0].cpu().numpy())
    print(f"{Ny} x {Nx} {prec} B = {B}: fused against composition {e:.3e} ({e / eps:.2f} eps)")
    assert 0 <= e < 16 * eps, (e, e / eps)
    assert torch.equal(out[1][0], out[1][1])
    assert torch.isfinite(out[1][0]).all()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_lenseflow_view_runs_the_old_entry_points(prec, case):
    """cmbl_gradientf_logpdf_op / cmbl_wiener_cg_op through cmbl_lensop_from_lenseflow equal the flow-typed entry points bit for bit (64 x 128, 36 x 60)"""
    C, sd = device(prec, case, "LenseFlow")
    from cmblensing_jl_amd.lib import check as ok
    ds, p = sd["ds"], sd["proj"]
    assert isinstance(ds.L, C.LenseFlow)
    F, f, phi, d = fields(C, sd, case)
    B = f.arr.shape[0]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    want = ds.gradientf_logpdf(f, phi).arr                                     # cmbl_gradientf_logpdf_op through the view ...
    got = p.empty(C.HARMONIC, ds.P, B)
    ok(ds.lib.cmbl_gradientf_logpdf(ds._h, ds.L._h, ptr(f.arr), None, 0, ptr(got), B))      # ... and the flow-typed symbol
    assert torch.equal(got, want)
    fw, h = ds.argmaxf_logpdf(phi, tol=0.0, nsteps=6)                          # cmbl_wiener_cg_op
    got = p.empty(C.HARMONIC, ds.P, B)
    hist, nit = (ctypes.c_double * (6 * B))(), ctypes.c_int(0)
    ok(ds.lib.cmbl_wiener_cg(ds._h, ds.L._h, ptr(d.arr), None, 0.0, 6, ptr(got), hist, ctypes.byref(nit), B))
    assert torch.equal(got, fw.arr) and nit.value == 6
    assert np.array_equal(np.array(hist[:6 * B]).reshape(6, B), hist_array(h))
    # ... and the one call for value and both gradients agrees with the composition LenseFlow keeps in Python
    lp, gf, gp = ds.grad_logpdf(f, phi)
    scalars_close((case, "LenseFlow view: logpdf"), lp, ds.logpdf(f, phi), rtol=5e-8 if prec == "f32" else 1e-10)
    close((case, "LenseFlow view: grad f"), gf.arr.cpu().numpy(), want.cpu().numpy(), 1e-4 if prec == "f32" else 4e-10)
    close((case, "LenseFlow view: grad phi"), gp.arr.cpu().numpy(), ds.gradientphi_logpdf(f, phi).arr.cpu().numpy(), 3e-4 if prec == "f32" else 1e-9)


def test_refusals():
    C, sd = device("f32", "D")
    ds, p = sd["ds"], sd["proj"]
    F, f, phi, d = fields(C, sd, "D")
    from cmblensing_jl_amd.lib import CmblError
    # an operator that was never given a ϕ or a deflection: CMBL_ERR_STATE
    old = ds.L
    try:
        ds.L = C.BilinearLens(p)
        with pytest.raises(CmblError) as e:
            ds.gradientf_logpdf(f, None)
        assert e.value.code == 5
        with pytest.raises(CmblError) as e:
            ds.argmaxf_logpdf(None, tol=0.0, nsteps=2)
        assert e.value.code == 5
        # a batched ϕ is refused by BilinearLens as it is today (src/bilinearlens.jl:40): CMBL_ERR_SHAPE
        phi2 = C.Field(p, torch.cat([phi.arr, phi.arr]).contiguous(), C.FOURIER)
        with pytest.raises(CmblError) as e:
            ds.L(phi2)
        assert e.value.code == 2
        # the drivers that need the pullback of L \ f
        with pytest.raises(NotImplementedError):
            C.MAP_joint(ds)
        with pytest.raises(NotImplementedError):
            C.sample_joint(ds, 1)
        # operator and data set on different contexts: Python refuses the assignment, the library the call (CMBL_ERR_ARG)
        p2 = C.ProjLambert(p.Ny, p.Nx, 3.0, torch.float32)
        other = C.BilinearLens(p2)
        with pytest.raises(ValueError):
            ds.L = other
        out = p.empty(C.HARMONIC, ds.P, 1)
        rc = ds.lib.cmbl_gradientf_logpdf_op(ds._h, other._view(), ctypes.c_void_p(f.arr.data_ptr()), None, 0, ctypes.c_void_p(out.data_ptr()), 1)
        assert rc == 1 and b"different contexts" in ds.lib.cmbl_last_error()
    finally:
        ds.L = old
