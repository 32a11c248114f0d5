r"""GPU parity of a flat-sky data set whose noise covariance is diagonal in the I/QU map basis, Cn = Diagonal(V) (`CMBL_OP_CN_INV_PIX`,
`cmbl_dataset_noise_inv`, `load_sim(noise_var_map=...)`; src/dataset.jl:37-47, 76-80, src/proj_lambert.jl:337-342), against
tests/_pixnoise_ref.py (the oracle's data set with a map-diagonal `Cn` dropped in) on identical inputs.

Cases (tests/_pixnoise_ref.py CASES): a 32 x 32 QU, two planes of V, two slots; b 32 x 64 IQU, three planes (Ny != Nx, two column tiles); c 64 x 32 I,
two slots; d 36 x 60 I and e 40 x 48 QU with ONE plane for both pol slices, two slots (the any-size path); t 2048 x 32 QU in float32 (the tall
column tile).  V ramps 30x across the patch, distinct per plane, with a few pixels of infinite variance (weight exactly 0).

Tolerances: the literal class bounds the same quantities carry in tests/test_gpu_parity.py and tests/test_gpu_lensop_dataset.py (float32 / float64):
pinv(Cn) z 5e-6 / 1e-12 (a diagonal operator between two transforms), ∇f 1e-4 / 4e-10, logpdf 5e-8 / 1e-10, ∇ϕ 3e-4 / 1e-9, ∇f° 2e-4 / 1e-9,
∇ϕ° 6e-6 / 3e-9, 8-step CG residuals 1e-3 / 1e-8 and iterate 4e-6 / 1e-9, native against composed drivers 2e-5 / 1e-10.  Every comparison goes
through tests/_tol.py."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _pixnoise_ref as R
from _tol import close, scalars_close

DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
TOL = {"f32": dict(noise_inv=5e-6, gradf=1e-4, logpdf=5e-8, gradphi=3e-4, gradfo=2e-4, gradpo=6e-6, hist=1e-3, wf=4e-6, native=2e-5),
       "f64": dict(noise_inv=1e-12, gradf=4e-10, logpdf=1e-10, gradphi=1e-9, gradfo=1e-9, gradpo=3e-9, hist=1e-8, wf=1e-9, native=1e-10)}
SMALL = ["a", "b", "c", "d", "e"]


def _pkg():
    import cmblensing_jl_amd as C
    return C


def npy(x):
    return x.arr.cpu().numpy() if hasattr(x, "arr") else np.asarray(x)


def check(prec, case, q, got, want, kind=None):
    t = TOL[prec][kind or q]
    e = scalars_close((case, q), npy(got), want, rtol=t) if (kind or q) in ("logpdf", "hist") else close((case, q), npy(got), want, t)
    print(f"{prec} {case} {q}: {e:.3e} (tolerance {t:.1e})")


_dev = {}


def device(prec, case, L=None, pix=True):
    """(C, load_sim dict, F, f, ϕ, d) of a case on the device with the reference's V (pix) or without the new operator, and the reference's data;
    one per (prec, case, operator, pix), shared by the tests"""
    C = _pkg()
    key = (prec, case, L, pix)
    Nside, pol, npl, B = R.CASES[case]
    ods, so = R.dataset(case)
    if key not in _dev:
        cls = {g: {k: C.Cls(v.ell, v.cl) for k, v in so["cls"][g].items()} for g in ("unlensed_scalar", "tensor", "total")}
        make = {None: None, "BilinearLens": C.BilinearLens}[L]
        _dev[key] = C.load_sim(3.0, Nside, pol, cls, T=DT[prec][0], beam_fwhm=3.0, pixel_mask=R.PM, Nbatch=1, Nphi=ods.Nphi * 2, L=make,
                               noise_var_map=so["V"] if pix else None)
    sd = _dev[key]
    p = sd["proj"]
    F = lambda a, b: C.Field(p, p.tensor(a), b)
    d = F(so["d"], C.HARMONIC)
    sd["ds"].set_data(d)
    return C, sd, F, F(so["f"], C.HARMONIC), F(so["phi"], C.FOURIER), d


def hist_array(h):
    return np.array([np.atleast_1d(r) for _, r in h])


@pytest.mark.parametrize("case,prec", [(c, pr) for c in SMALL for pr in ("f32", "f64")] + [("t", "f32")])
def test_noise_inv_and_gradientf(prec, case):
    """pinv(Cn) z (also in place) and the three forms of gradientf_logpdf: f and d given, f = 0, d = 0 (t: the tall column tile of float32)"""
    C, sd, F, f, phi, d = device(prec, case)
    ds, ref = sd["ds"], R.quantities(case)
    assert ds.ops["Cn_inv_pix"].shape[0] == R.CASES[case][2]
    w = ds.ops["Cn_inv_pix"]
    assert int((w == 0).sum()) == 2 * w.shape[0] and float(w.max() / w[w > 0].min()) > 29      # exact zeros, 30x range
    check(prec, case, "noise_inv", ds.noise_inv(d), ref["noise_inv"])
    z = d.arr.clone()
    from cmblensing_jl_amd.lib import check as ok
    ok(ds.lib.cmbl_dataset_noise_inv(ds._h, ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(z.data_ptr()), z.shape[0]))
    assert torch.equal(z, ds.noise_inv(d).arr)                                                   # in place: the same bits
    check(prec, case, "gradf", ds.gradientf_logpdf(f, phi), ref["gradf"])
    zero = F(np.zeros_like(ref["gradf"]), C.HARMONIC)
    check(prec, case, "gradf_f0", ds.gradientf_logpdf(zero, phi), ref["gradf_f0"], "gradf")
    check(prec, case, "gradf_d0", ds.gradientf_logpdf(f, phi, zero_d=True), ref["gradf_d0"], "gradf")


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", ["a", "b", "d"])
def test_constant_variance_equals_the_fourier_form(prec, case):
    """V = v everywhere: the sandwich is the Fourier-diagonal operator v⁻¹ of the same data set, up to the rounding of two transforms"""
    C, sd, F, f, phi, d = device(prec, case)
    ds, p = sd["ds"], sd["proj"]
    P = ds.P
    keep_pix, keep_cn = ds.ops["Cn_inv_pix"].clone(), ds.ops["Cn_inv"].clone()
    try:
        ds.set_op("Cn_inv_pix", np.full((R.CASES[case][2], p.Nx, p.Ny), 1 / R.V0))
        got = ds.noise_inv(d).arr.cpu().numpy()
        ds.set_op("Cn_inv_pix", None)
        one = np.ones((p.Nx, p.Nyh)) / R.V0
        ds.set_op("Cn_inv", np.stack([one, 0 * one, 0 * one, one, one] if P == 3 else [one] * P))
        want = ds.noise_inv(d).arr.cpu().numpy()
        close((case, "constant V"), got, want, TOL[prec]["noise_inv"])
    finally:
        ds.set_op("Cn_inv", keep_cn)
        ds.set_op("Cn_inv_pix", keep_pix)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", SMALL)
def test_posterior_and_wiener_filter(prec, case):
    """logpdf with ∇f and ∇ϕ (cmbl_grad_logpdf_op), the composed logpdf, the 8-step CG history, and in float64 the iterations to tol = 1e-1"""
    C, sd, F, f, phi, d = device(prec, case)
    ds, ref = sd["ds"], R.quantities(case)
    lp, gf, gp = ds.grad_logpdf(f, phi)
    check(prec, case, "logpdf", lp, ref["logpdf"])
    check(prec, case, "gradf", gf, ref["gradf"])
    check(prec, case, "gradphi", gp, ref["gradphi"])
    check(prec, case, "logpdf (composed)", ds.logpdf(f, phi), ref["logpdf"], "logpdf")
    check(prec, case, "gradphi (composed)", ds.gradientphi_logpdf(f, phi), ref["gradphi"], "gradphi")
    fw, h = ds.argmaxf_logpdf(phi, tol=0.0, nsteps=8)
    assert len(h) == 8
    check(prec, case, "hist", hist_array(h), ref["hist"])
    check(prec, case, "wf", fw, ref["wf"])
    if prec == "f64":
        fw, h = ds.argmaxf_logpdf(phi, tol=1e-1, nsteps=500)
        assert abs(len(h) - R.CG_ITERS[case]) <= 1, (len(h), R.CG_ITERS[case])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", SMALL)
def test_logpdf_mixed_and_gradient(prec, case):
    C, sd, F, f, phi, d = device(prec, case)
    ds, ref = sd["ds"], R.quantities(case)
    ds.set_data(C.Field(sd["proj"], d.arr[:1].contiguous(), C.HARMONIC))
    fo, po = F(ref["mix_f"], C.MAP), F(ref["mix_phi"], C.FOURIER)
    check(prec, case, "logpdf_mixed", ds.logpdf_mixed(fo, po), ref["logpdf_mixed"], "logpdf")
    lp, gfo, gpo = ds.gradient_logpdf_mixed(fo, po, alias_quirk=False)
    check(prec, case, "logpdf_mixed from the gradient call", lp, ref["logpdf_mixed"], "logpdf")
    check(prec, case, "gradfo", gfo, ref["gradfo"])
    check(prec, case, "gradpo", gpo, ref["gradpo"])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", ["a", "e"])
def test_native_drivers_equal_the_composed_drivers(prec, case):
    """one cmbl_map_joint_step and one cmbl_hmc_step with given white maps and log u against the Python-composed drivers on the same data set
    (bounds of tests/test_gpu_drivers.py::test_native_driver_exports_equal_the_python_drivers)"""
    C, sd, F, f, phi, d = device(prec, case)
    ds, proj = sd["ds"], sd["proj"]
    B = d.arr.shape[0]
    tight = TOL[prec]["native"]
    phiB = C.Field(proj, phi.arr.expand(B, -1, -1, -1).contiguous(), C.FOURIER)
    fo, po = ds.mix(f, phiB)
    rng = np.random.default_rng(5)
    wp, logu = rng.standard_normal((B, 1, proj.Nx, proj.Ny)), np.log(rng.random(B))
    x_p, dH_p, acc_p = C.hmc_step(ds, fo, po, wp, logu, N=3, eps=0.02)
    x_n, dH_n, acc_n = C.hmc_step_native(ds, fo, po, white_p=wp, log_u=logu, N=3, eps=0.02)
    close((case, "native hmc_step: phi°"), npy(x_n), npy(x_p), tight)
    np.testing.assert_allclose(dH_n, dH_p, atol=(0.5 if prec == "f32" else 1e-6))
    assert acc_n.tolist() == acc_p.tolist()
    p0 = C.Field(proj, torch.zeros_like(po.arr), C.FOURIER)
    st_p = C.MAP_joint_step(ds, p0, alpha_tol=1e-4, cg_tol=0.0, cg_nsteps=8)
    st_n = C.MAP_joint_step_native(ds, p0, alpha_tol=1e-4, cg_tol=0.0, cg_nsteps=8)
    assert st_n["ncg"] == len(st_p["cg_hist"]) == 8
    close((case, "native MAP_joint step: f"), npy(st_n["f"]), npy(st_p["f"]), tight)
    assert abs(st_n["alpha"] - st_p["alpha"]) < (2e-3 if prec == "f32" else 1e-6) * max(1.0, st_p["alpha"]), (st_n["alpha"], st_p["alpha"])
    close((case, "native MAP_joint step: phi"), npy(st_n["phi"]), npy(st_p["phi"]), 5e-3 if prec == "f32" else 1e-6)
    scalars_close((case, "native MAP_joint step: logpdf"), st_n["logpdf"], st_p["logpdf"], rtol=2e-6 if prec == "f32" else 1e-10)


_bl = {}


def bilinear_reference(case):
    import _lensop_ds_ref as LR
    if case not in _bl:
        ods, so = R.dataset(case)
        ds = LR.LensOpDataSet.of(ods, "BilinearLens")
        f, phi = so["f"], so["phi"]
        ds.d = ds.mean(ds.L(phi), f) + so["n"]
        zero = np.zeros_like(ds.d)
        out = {"d": ds.d, "gradf": ds.gradientf_logpdf(f, ds.L(phi), ds.d), "gradf_f0": ds.gradientf_logpdf(zero, ds.L(phi), ds.d),
               "gradf_d0": ds.gradientf_logpdf(f, ds.L(phi), zero), "logpdf": np.atleast_1d(ds.logpdf(f, phi, ds.d)),
               "gradphi": ds.gradientphi_logpdf(f, phi, ds.d)}
        fw, h = ds.argmaxf_logpdf(phi, d=ds.d, tol=0.0, nsteps=8)
        out["wf"], out["hist"] = fw, hist_array(h)
        _bl[case] = out
    return _bl[case]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", ["a", "d"])
def test_bilinear_lens_in_the_slot(prec, case):
    """the three forms of ∇f, logpdf with both gradients and the 8-step CG with a BilinearLens in the L slot (power-of-two and any-size)"""
    C, sd, F, f, phi, d = device(prec, case, "BilinearLens")
    ds, ref = sd["ds"], bilinear_reference(case)
    assert isinstance(ds.L, C.BilinearLens) and "Cn_inv_pix" in ds.ops
    ds.set_data(F(ref["d"], C.HARMONIC))
    check(prec, case, "BilinearLens gradf", ds.gradientf_logpdf(f, phi), ref["gradf"], "gradf")
    zero = F(np.zeros_like(ref["gradf"]), C.HARMONIC)
    check(prec, case, "BilinearLens gradf_f0", ds.gradientf_logpdf(zero, phi), ref["gradf_f0"], "gradf")
    check(prec, case, "BilinearLens gradf_d0", ds.gradientf_logpdf(f, phi, zero_d=True), ref["gradf_d0"], "gradf")
    lp, gf, gp = ds.grad_logpdf(f, phi)
    check(prec, case, "BilinearLens logpdf", lp, ref["logpdf"], "logpdf")
    check(prec, case, "BilinearLens gradf from grad_logpdf", gf, ref["gradf"], "gradf")
    check(prec, case, "BilinearLens gradphi", gp, ref["gradphi"], "gradphi")
    fw, h = ds.argmaxf_logpdf(phi, tol=0.0, nsteps=8)
    check(prec, case, "BilinearLens hist", hist_array(h), ref["hist"], "hist")
    check(prec, case, "BilinearLens wf", fw, ref["wf"], "wf")


def _snapshot(C, sd, f, phi, d):
    ds = sd["ds"]
    B = d.arr.shape[0]
    phiB = C.Field(sd["proj"], phi.arr.expand(B, -1, -1, -1).contiguous(), C.FOURIER)
    fo = ds.L(phi) * f
    lp, gfo, gpo = ds.gradient_logpdf_mixed(fo, phiB)
    fw, h = ds.argmaxf_logpdf(phi, tol=0.0, nsteps=4)
    return [torch.from_numpy(np.asarray(lp)), gfo.arr.clone(), gpo.arr.clone(), fw.arr.clone(), torch.from_numpy(hist_array(h)),
            ds.gradientf_logpdf(f, phi).arr.clone()]


def _launches(p, fn):
    p.prof_enable(True)
    p.prof_reset()
    try:
        fn()
        p.synchronize() if hasattr(p, "synchronize") else torch.cuda.synchronize()
        return {k: n for k, (ms, n) in p.prof_table().items()}
    finally:
        p.prof_enable(False)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", ["a", "c", "d"])
def test_clearing_restores_the_fourier_form_and_the_gate_holds(prec, case):
    """nplanes = 0 restores the Fourier-form results bit for bit; a data set that never had the operator gives the same bits and, on a
    power-of-two map, still runs the fused Wiener filter, which a data set with the operator does not"""
    C, sd, F, f, phi, d = device(prec, case)
    ds, p = sd["ds"], sd["proj"]
    assert p.get_option("fused_harm") == 1
    keep = ds.ops["Cn_inv_pix"].clone()
    with_pix = _snapshot(C, sd, f, phi, d)
    try:
        ds.set_op("Cn_inv_pix", None)
        assert "Cn_inv_pix" not in ds.ops
        cleared = _snapshot(C, sd, f, phi, d)
    finally:
        ds.set_op("Cn_inv_pix", keep)
    again = _snapshot(C, sd, f, phi, d)
    assert all(torch.equal(a, b) for a, b in zip(with_pix, again))
    assert not torch.equal(with_pix[-1], cleared[-1])
    # never set: the same Cn̂ in the Fourier slot, the same data
    C2, sd2, F2, f2, phi2, d2 = device(prec, case, pix=False)
    ds2 = sd2["ds"]
    ds2.set_op("Cn_inv", ds.ops["Cn_inv"])
    ds2.set_op("precond_inv", ds.ops["precond_inv"]); ds2.set_op("D", ds.ops["D"]); ds2.set_op("D_inv", ds.ops["D_inv"])
    ds2.set_logdet(ds.logdet_sum)
    never = _snapshot(C2, sd2, f2, phi2, d2)
    for name, a, b in zip(("logpdf_mixed", "∇f°", "∇ϕ°", "4-step iterate", "4-step history", "∇f"), cleared, never):
        assert torch.equal(a, b), name
    # the launches of a 3-iteration solve with the operator as it is set (no set_phi inside the window): the fused iteration is the only user of the
    # flat harmonic carrier (class "harm_dot": start, and three per iteration)
    run = lambda s: (lambda: s["ds"].argmaxf_logpdf(None, tol=0.0, nsteps=3))
    ds.L(phi); ds2.L(phi2)
    n_pix, n_never = _launches(p, run(sd)), _launches(sd2["proj"], run(sd2))
    assert "harm_dot" not in n_pix and n_pix.get("cg_update", 0) > 0, n_pix
    if case != "d":
        assert n_never.get("harm_dot", 0) >= 4 and "mask_mul" in n_never, n_never      # the fused iteration, with its pixel-mask column launches
        one = _launches(p, lambda: ds.noise_inv(d))
        assert (one.get("x_harm"), one.get("mask_mul"), one.get("harm_apply", 0)) == (2, 1, 0), one      # the three-launch sandwich
    else:
        assert "harm_dot" not in n_never


def test_wrong_number_of_planes_is_a_shape_error():
    C, sd, F, f, phi, d = device("f64", "a")
    ds, p = sd["ds"], sd["proj"]
    assert ds.P == 2
    t = p.tensor(np.ones((3, p.Nx, p.Ny)))
    rc = ds.lib.cmbl_dataset_set_op(ds._h, 10, ctypes.c_void_p(t.data_ptr()), 3)
    assert rc == 2, (rc, ds.lib.cmbl_last_error())                          # CMBL_ERR_SHAPE
    ref = R.quantities("a")
    check("f64", "a", "noise_inv after the refused call", ds.noise_inv(d), ref["noise_inv"], "noise_inv")     # the operator is as it was
    ds2 = C.BaseDataSet(p, 2, {})
    with pytest.raises(C.CmblError) as e:
        ds2.noise_inv(d)
    assert e.value.code == 5                                                # CMBL_ERR_STATE: neither form is set


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_load_sim_noise_follows_the_variance_map(prec):
    """load_sim(noise_var_map=V) with V = v on one half of the patch and 30 v on the other: the sample variances of the noise d - M B L f on the
    two halves are in the ratio 30 within 4 sqrt(2/n) (the relative standard error of a sample variance of n Gaussian draws is sqrt(2/n)); and
    logpdf_mixed_theta at the fiducial θ is logpdf_mixed"""
    C = _pkg()
    from bench import synthetic_cls
    Ny, Nx, P = 64, 128, 2
    V = np.full((1, Nx, Ny), R.V0)
    V[:, Nx // 2:] *= 30
    s = C.load_sim(3.0, (Ny, Nx), "P", synthetic_cls(), T=DT[prec][0], beam_fwhm=2.0, pixel_mask=dict(pad_deg=0.4, apod_deg=0.4), Nphi="flat", noise_var_map=V)
    ds = s["ds"]
    n = (s["d"] - ds.mean(s["f"], s["phi"])).to(C.MAP).arr.cpu().numpy().astype(np.float64)
    assert n.shape == (1, P, Nx, Ny)
    npix = P * (Nx // 2) * Ny
    ratio = n[:, :, Nx // 2:].var() / n[:, :, :Nx // 2].var()
    print(f"variance ratio {ratio:.3f} (30 expected, margin {30 * 4 * np.sqrt(2 / npix):.3f})")
    assert abs(ratio / 30 - 1) < 4 * np.sqrt(2 / npix), ratio
    np.testing.assert_allclose(ds.host["logdet_Cn"], P * np.sum(np.log(V)), rtol=1e-13)                  # summed on the host in double
    lv = 1 / np.mean(1 / V)
    np.testing.assert_allclose(ds.host["Cn"].p, lv, rtol=1e-14)
    assert np.array_equal(ds.host["Cn_pix"], V)
    fo, po = ds.mix(s["f"], s["phi"])
    base = ds.logpdf_mixed(fo, po)
    np.testing.assert_allclose(C.logpdf_mixed_theta(ds, fo, po), base, rtol=1e-12)
    C.set_theta(ds)
    # the simulation helper draws the same noise from the same white map
    w = C.sim.white_noise(3, (1, P, Nx, Ny))
    close("noise_from_white", C.noise_from_white(ds, w).arr.cpu().numpy(), s["n"].arr.cpu().numpy(), 1e-6 if prec == "f32" else 1e-12)
