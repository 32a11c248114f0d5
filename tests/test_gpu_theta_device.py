"""The Gibbs θ pass on the device: `logpdf_mixed_theta_grid` (cmbl_dataset_theta_model / cmbl_logpdf_mixed_theta, the θ-operator kernel of
csrc/kernels_theta.hpp) against the float64 oracle of the θ layer (oracle/theta.py), against the host θ path (theta.set_theta, unchanged
code) and, plane by plane, against the host algebra `theta._ops` that defines every formula.

Bounds.  Values: the project's own for this comparison on the host path (tests/test_gpu_drivers.py::test_theta_layer): rtol 3e-5 (fp32),
1e-10 (fp64).  Planes, fp32: device and host both round ONCE to float doubles that agree far below a float ulp, so they differ by at most one
float ulp, |a - b| <= 2^-23 |b|; fp64: the project's 1e-10 for θ-dependent quantities, elementwise.  Exact zeros of the host are exact zeros
of the device in either precision."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_parity import _dataset_pair, DT, scalars_close

RT = {"f32": 3e-5, "f64": 1e-10}
SHAPES = {"64x64": dict(Nside=(64, 64), mask=True, beam=1.0),          # fused path, mask and beam
          "32x64": dict(Nside=(32, 64), mask=True, beam=1.0),          # non-square: the λ weights run along ky
          "96x80": dict(Nside=(96, 80), mask=False, beam=1.0)}         # any-size path
THETAS = (dict(), dict(r=0.2, Aphi=1.0), dict(r=0.35), dict(Aphi=0.8), dict(r=0.1, Aphi=1.25))
LE = [100, 600, 1500, 3000]
AMP = np.array([1.3, 1.0, 0.8])
BANDS = {"P": ({"EE": (LE, "AEE")}, {"AEE": ([0], LE)}),
         "IP": ({"TT": (LE, "ATT"), "TE": (LE, "ATE"), "EE": (LE, "AEE")}, {"ATT": ([0], LE), "ATE": ([1, 2], LE), "AEE": ([3], LE)})}


@functools.lru_cache(maxsize=None)
def _pair(prec, pol, shape, B=1):
    """one data set pair per case, shared by the tests of this file; every test leaves the device data set at fiducial θ, without bands"""
    C, so, sd = _dataset_pair(prec, pol, B=B, **SHAPES[shape])
    p = sd["proj"]
    F = lambda a, b: C.Field(p, p.tensor(a), b)
    sd["ds"].set_data(F(so["d"], C.HARMONIC))
    fo_o, po_o = so["ds"].mix(so["f"], so["phi"])
    return C, so, sd, (fo_o, po_o), (F(fo_o, C.MAP), F(po_o, C.FOURIER))


@functools.lru_cache(maxsize=None)
def _oracle_values(pol, shape, banded):
    """the oracle is float64 whatever the device precision: its values are computed once per (pol, shape)"""
    from oracle.theta import ThetaDataSet
    _, so, _, (fo_o, po_o), _ = _pair("f64", pol, shape)
    if not banded:
        th = ThetaDataSet(so["ds"], so["Cfs"], so["Cten"])
        return np.array([th.logpdf_mixed(fo_o, po_o, **kw) for kw in THETAS])
    th = ThetaDataSet(so["ds"], so["Cfs"], so["Cten"], bands=BANDS[pol][1])
    return np.array([th.logpdf_mixed(fo_o, po_o, **kw) for kw in _band_thetas(pol)])


def _band_thetas(pol):
    names = list(BANDS[pol][1])
    alone = {n: AMP for n in names}
    return (dict(), alone, dict(alone, r=0.3, Aphi=1.1), {names[-1]: np.array([0.9, 1.1, 1.0]), "r": 0.35})


def _state(ds):
    return {k: v.clone() for k, v in ds.ops.items()}, dict(ds.theta) if getattr(ds, "theta", None) is not None else None, ds.logdet_sum, ds.logdet_mix


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("pol", ["I", "P", "IP"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_grid_against_oracle_and_host_path(prec, pol, shape):
    """items 1, 2 and 4: the grid against ThetaDataSet.logpdf_mixed and against logpdf_mixed_theta (host path); the data set is untouched by a
    grid call and a second call is bit-identical (the reduction's determinism)"""
    C, so, sd, _, (fo, po) = _pair(prec, pol, shape)
    ds = sd["ds"]
    before, lp0 = _state(ds), ds.logpdf_mixed(fo, po)
    got = C.logpdf_mixed_theta_grid(ds, fo, po, THETAS)
    assert got.shape == (len(THETAS), 1)
    again = C.logpdf_mixed_theta_grid(ds, fo, po, THETAS)
    assert np.array_equal(got, again)
    after = _state(ds)
    assert np.array_equal(ds.logpdf_mixed(fo, po), lp0)
    assert before[1:] == after[1:] and all(torch.equal(before[0][k], after[0][k]) for k in before[0]) and before[0].keys() == after[0].keys()
    want = _oracle_values(pol, shape, False)
    print(f"\n[{prec} {pol} {shape}] device vs oracle, max rel: {np.max(np.abs(got - want) / np.abs(want)):.3e}")
    np.testing.assert_allclose(got, want, rtol=RT[prec])
    try:
        host = np.array([C.logpdf_mixed_theta(ds, fo, po, **kw) for kw in THETAS])
    finally:
        C.set_theta(ds)
    print(f"[{prec} {pol} {shape}] device vs host path, max rel: {np.max(np.abs(got - host) / np.abs(host)):.3e}")
    scalars_close("grid vs host path", got.ravel(), host.ravel(), rtol=RT[prec])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("pol", ["P", "IP"])
def test_bandpower_grid(prec, pol):
    """bandpower amplitudes (one band on EE for P; on TT, TE, EE for IP), alone and together with r and Aϕ"""
    C, so, sd, _, (fo, po) = _pair(prec, pol, "64x64")
    ds = sd["ds"]
    cls = {k: C.Cls(v.ell, v.cl) for k, v in so["cls"]["unlensed_scalar"].items()}
    C.use_bandpowers(ds, BANDS[pol][0], cls)
    try:
        ths = _band_thetas(pol)
        got = C.logpdf_mixed_theta_grid(ds, fo, po, ths)
        want = _oracle_values(pol, "64x64", True)
        print(f"\n[{prec} {pol}] bands, device vs oracle, max rel: {np.max(np.abs(got - want) / np.abs(want)):.3e}")
        np.testing.assert_allclose(got, want, rtol=RT[prec])
        host = np.array([C.logpdf_mixed_theta(ds, fo, po, **kw) for kw in ths])
        print(f"[{prec} {pol}] bands, device vs host path, max rel: {np.max(np.abs(got - host) / np.abs(host)):.3e}")
        scalars_close("banded grid vs host path", got.ravel(), host.ravel(), rtol=RT[prec])
        # a wrong amplitude count is refused by the library
        with pytest.raises(C.CmblError) as e:
            C.logpdf_mixed_theta_grid(ds, fo, po, [{list(BANDS[pol][1])[0]: np.ones(2)}])
        assert e.value.code == 2                                   # CMBL_ERR_SHAPE
    finally:
        ds.host.pop("Cfs_bands")
        C.set_theta(ds)


def _cut_cls(C, lmax):
    """the spectra of the fixture cut at lmax: whole rings of modes of a 3' map (Nyquist 3600) then have Cf = Cϕ = 0"""
    from bench import synthetic_cls
    out = {}
    for g, d in synthetic_cls().items():
        out[g] = {k: C.Cls(v.ell[v.ell <= lmax], v.cl[v.ell <= lmax]) for k, v in d.items()}
    return out


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("pol", ["I", "P", "IP"])
@pytest.mark.parametrize("Nside", [(64, 64), (32, 64), (96, 80)])
def test_operator_planes(prec, pol, Nside):
    """item 3: the four scratch operator sets against theta._ops cast to the context's dtype, elementwise, with spectra cut at ℓ = 1500
    (rings of exactly-zero covariance, where pinv is discontinuous) and one band on the last rescalable spectrum"""
    import cmblensing_jl_amd as C
    from cmblensing_jl_amd.theta import _ops
    cls = _cut_cls(C, 1500)
    s = C.load_sim(3.0, Nside, pol, cls, T=DT[prec][0], beam_fwhm=1.0, Nphi="flat")
    ds = s["ds"]
    bands = None
    if pol != "I":
        C.use_bandpowers(ds, {"EE": (LE, "AEE")}, cls["unlensed_scalar"])
        bands = dict(AEE=AMP)
    worst = 0.0
    for kw in (dict(), dict(r=0.35, Aphi=0.8), dict(r=0.05)):
        ds.host.setdefault("Cphi0", np.asarray(ds.host["Cphi"], float).copy())
        ops, logdet_sum, logdet_mix, _ = _ops(ds, kw.get("r"), kw.get("Aphi"), bands)
        for name in ("Cf_inv", "D_inv", "Cphi_inv", "G_inv"):
            dev, sums = C.theta_ops_device(ds, name, **kw, **(bands or {}))
            want = np.asarray(ops[name]).astype(DT[prec][1])
            got = dev.cpu().numpy()
            assert got.shape == want.shape
            assert np.all(np.isfinite(got))
            zero = want == 0
            assert zero.any() or name == "G_inv"                    # the cut really leaves exact zeros
            assert np.all(got[zero] == 0), f"{name} {kw}: {np.count_nonzero(got[zero])} modes that are exactly 0 on the host are not on the device"
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            bound = (2.0 ** -23 if prec == "f32" else 1e-10) * np.abs(want.astype(np.float64))
            rel = float(np.max(err[~zero] / np.abs(want[~zero].astype(np.float64)))) if (~zero).any() else 0.0
            worst = max(worst, rel)
            assert np.all(err <= bound), f"{name} {kw}: max elementwise relative difference {rel:.3e}"
        logdet_cn = ds.host["logdet_Cn"] if ds.host.get("logdet_Cn") is not None else ds.host["Cn"].logdet(ds.proj)
        # the sums: the same double terms added in another order -- the project's 1e-10 for θ-dependent quantities, relative to the scale of
        # the summed logarithms (logdet_sum); a parameter that is not named contributes exactly 0
        np.testing.assert_allclose(sums[0] + logdet_cn, logdet_sum, rtol=1e-10)
        np.testing.assert_allclose(sums[1] + sums[2], logdet_mix, rtol=1e-10, atol=1e-10 * abs(logdet_sum))
        if kw.get("r") is None:
            assert sums[1] == 0.0
        if kw.get("Aphi") is None:
            assert sums[2] == 0.0
    print(f"\n[{prec} {pol} {Nside}] planes vs _ops, max elementwise rel: {worst:.3e}")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_gibbs_pass_on_device(prec):
    """item 5: gibbs_sample_theta(on="device") against the oracle's grid_and_sample with the same uniform, at test_theta_layer's bounds"""
    from oracle.theta import ThetaDataSet, grid_and_sample as o_gas
    C, so, sd, (fo_o, po_o), (fo, po) = _pair(prec, "P", "64x64")
    ds = sd["ds"]
    th = ThetaDataSet(so["ds"], so["Cfs"], so["Cten"])
    xs = np.linspace(0.6, 1.6, 9)
    val, lp_grid = C.gibbs_sample_theta(ds, fo, po, dict(r=None, Aphi=None), "Aphi", xs, [0.37], on="device")
    lps_o = np.array([th.logpdf_mixed(fo_o, po_o, Aphi=a)[0] for a in xs])
    want, _, lp_o = o_gas(lps_o, xs, 0.37)
    np.testing.assert_allclose(lp_grid[0], lp_o, atol=5e-2 if prec == "f32" else 1e-6)
    assert abs(val[0] - want) < (2e-2 if prec == "f32" else 1e-6)
    assert xs[0] < val[0] < xs[-1]
    assert ds.logdet_mix == 0.0                                     # the data set did not move


def test_sample_joint_theta_on_device():
    """item 5: three steps of sample_joint with the θ pass on the device give the θ chain of the host pass"""
    import cmblensing_jl_amd as C
    from bench import synthetic_cls
    xs = np.linspace(0.5, 2.0, 12)
    chains = {}
    for on in ("host", "device"):
        s = C.load_sim(3.0, (64, 64), "P", synthetic_cls(), T=torch.float64, beam_fwhm=1.0, Nphi="flat")
        out = C.sample_joint(s["ds"], 3, chain_ids=(0,), base_seed=5, N=3, eps=0.01, rng="device", theta_ranges=dict(Aphi=xs), phi_start=s["phi"], theta_on=on)
        chains[on] = np.array([t["Aphi"] for t in out["theta"]])
    assert len(chains["device"]) == 3 and len(set(chains["device"])) > 1
    np.testing.assert_allclose(chains["device"], chains["host"], rtol=1e-6)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_batch_slots(prec):
    """item 6: with B = 2 slots of (f°, ϕ°), row b of the grid is the B = 1 result of that slot"""
    C, so, sd, _, (fo, po) = _pair(prec, "P", "64x64", B=2)
    ds, p = sd["ds"], sd["proj"]
    ths = THETAS[1:]
    both = C.logpdf_mixed_theta_grid(ds, fo, po, ths)
    assert both.shape == (len(ths), 2)
    d = ds.d
    try:
        for b in range(2):
            ds.set_data(C.Field(p, d.arr[b:b + 1].contiguous(), d.basis))
            one = C.logpdf_mixed_theta_grid(ds, C.Field(p, fo.arr[b:b + 1].contiguous(), C.MAP), C.Field(p, po.arr[b:b + 1].contiguous(), C.FOURIER), ths)
            print(f"\n[{prec}] slot {b}: B = 2 row vs B = 1, max rel {np.max(np.abs(both[:, b] - one[:, 0]) / np.abs(one[:, 0])):.3e}")
            scalars_close(("batch slot", b), both[:, b], one[:, 0], rtol=RT[prec])
    finally:
        ds.set_data(d)
    assert abs(both[0, 0] - both[0, 1]) > 1e-3 * abs(both[0, 0])    # the slots really differ


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_map_diagonal_noise(prec):
    """a data set with CMBL_OP_CN_INV_PIX (composed posterior; logdet Cn is the scalar given at install) against the host path"""
    import cmblensing_jl_amd as C
    from bench import synthetic_cls
    Ny, Nx = 32, 64
    x, y = np.linspace(0, 1, Nx)[:, None], np.linspace(0, 1, Ny)[None, :]
    V = np.stack([7.5 * (1 + 3 * (0.5 + 0.5 * np.sin(2 * np.pi * (x * (k + 1) + y)))) for k in range(2)])
    s = C.load_sim(3.0, (Ny, Nx), "P", synthetic_cls(), T=DT[prec][0], beam_fwhm=1.0, Nphi="flat", noise_var_map=V)
    ds = s["ds"]
    assert "Cn_inv_pix" in ds.ops and ds.host["logdet_Cn"] is not None
    fo, po = ds.mix(s["f"], s["phi"])
    got = C.logpdf_mixed_theta_grid(ds, fo, po, THETAS)
    try:
        host = np.array([C.logpdf_mixed_theta(ds, fo, po, **kw) for kw in THETAS])
    finally:
        C.set_theta(ds)
    print(f"\n[{prec}] map-diagonal noise, device vs host path, max rel: {np.max(np.abs(got - host) / np.abs(host)):.3e}")
    scalars_close("grid vs host path, pixel noise", got.ravel(), host.ravel(), rtol=RT[prec])


def test_errors():
    """item 7: evaluating before a model is installed is CMBL_ERR_STATE; another operator than a LenseFlow is refused before any library call"""
    import cmblensing_jl_amd as C
    from cmblensing_jl_amd.lib import check
    from bench import synthetic_cls
    s = C.load_sim(3.0, (32, 32), "P", synthetic_cls(), T=torch.float32, beam_fwhm=1.0, Nphi="flat")
    ds, p = s["ds"], s["proj"]
    fo, po = ds.mix(s["f"], s["phi"])
    fo, po = fo.to(C.MAP), po.to(C.FOURIER)
    pd = ctypes.POINTER(ctypes.c_double)
    r, A, lp = np.array([0.2]), np.array([1.0]), np.empty(1)
    with pytest.raises(C.CmblError) as e:
        check(ds.lib.cmbl_logpdf_mixed_theta(ds._h, ds.L._h, ctypes.c_void_p(fo.arr.data_ptr()), ctypes.c_void_p(po.arr.data_ptr()), 1, 1,
                                             r.ctypes.data_as(pd), A.ctypes.data_as(pd), None, 0, lp.ctypes.data_as(pd)))
    assert e.value.code == 5                                        # CMBL_ERR_STATE
    with pytest.raises(C.CmblError) as e:
        check(ds.lib.cmbl_dataset_theta_ops(ds._h, 0.2, 1.0, None, 0, 0, None, None))
    assert e.value.code == 5
    flow = ds.L
    ds.L = C.BilinearLens
    try:
        with pytest.raises(ValueError):
            C.logpdf_mixed_theta_grid(ds, fo, po, [dict(r=0.3)])
        assert getattr(ds, "_theta_model", None) is None            # nothing was installed: raised before any library call
    finally:
        ds.L = flow
    assert np.all(np.isfinite(C.logpdf_mixed_theta_grid(ds, fo, po, [dict(r=0.3)])))
