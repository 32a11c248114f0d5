"""CPU side of the flat-sky NoLensingDataSet: the fixtures of tests/_nolensing_ref.py that tests/test_gpu_nolensing.py runs the device against,
pinned with the float64 oracle, and the parts of the feature that need no GPU (the binding, the signatures, the slot check).
  * the identity in the L slot gives exactly what a LenseFlow at ϕ = 0 gives (the way to this answer before the identity existed);
  * pol = "P", tol = 0.1: the history lengths of _nolensing_ref.STOPS, each stop decided with at least 3 % on either side, and float32 stops at
    the same length;
  * without a pixel mask the operator is diagonal mode by mode: the CG's second residual is ~1e-25 of the first and the solve is the closed form;
  * gradientf_logpdf is the gradient of logpdf (central differences along random directions)."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import oracle as O
import _nolensing_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("pol", N.POLS)
def test_identity_equals_lenseflow_at_zero_phi(pol):
    s = N.sim(pol, (32, 32))
    lens = s["so"]["ds"]                                                     # the lensing data set on the same operators
    L0 = lens.L(np.zeros_like(s["so"]["phi"]))
    g_id = s["ds"].gradientf_logpdf(s["f"], N.IDENTITY, s["d"])
    g_flow = lens.gradientf_logpdf(s["f"], L0, s["d"])
    assert np.max(np.abs(g_id - g_flow)) == 0.0
    assert np.array_equal(s["ds"].mean(N.IDENTITY, s["f"]), lens.mean(L0, s["f"]))


@pytest.mark.parametrize("shape,B", sorted(N.STOPS))
def test_stop_lengths_and_margins_of_the_table(shape, B):
    n, last, prev = N.STOPS[(shape, B)]
    x, h = N.solve("P", shape, np.float64, B, True, 500, N.TOL)
    assert len(h) == n
    assert h[-1].max() == pytest.approx(last, rel=2e-3) and h[-2].max() == pytest.approx(prev, rel=5e-3)
    assert h[-1].max() < N.TOL / 1.03 and h[-2].max() > N.TOL * 1.03          # the stop is decided with 3 % to spare on each side
    assert all(hh.max() > N.TOL * 1.03 for hh in h[:-1])
    if B == 2:
        assert len(N.solve("P", shape, np.float32, B, True, 500, N.TOL)[1]) == n


@pytest.mark.parametrize("pol", N.POLS)
def test_without_a_mask_the_solve_is_the_closed_form(pol):
    s = N.sim(pol, (32, 32), mask=False)
    x, h = N.solve(pol, (32, 32), mask=False, nsteps=500, tol=N.TOL)
    assert len(h) == 2 and np.all(h[1] < 1e-20 * h[0])                       # the preconditioner is the inverse of the operator
    want = N.closed_form(s["ds"], s["d"])
    assert np.max(np.abs(x - want)) <= 1e-12 * np.max(np.abs(want))           # mode by mode


@pytest.mark.parametrize("pol", N.POLS)
def test_gradientf_is_the_gradient_of_logpdf(pol):
    s = N.sim(pol, (32, 32))
    ds, f, d = s["ds"], s["f"], s["d"]
    g = ds.gradientf_logpdf(f, N.IDENTITY, d)
    rng = np.random.Generator(np.random.PCG64(5))
    P, Ny, Nx = f.shape[1], 32, 32
    v = O.dataset.to_harm(ds.proj, rng.standard_normal((2, P, Nx, Ny)))       # a direction that is the spectrum of a real map
    v *= np.sqrt(np.sum(np.abs(f) ** 2) / np.sum(np.abs(v) ** 2))
    eps = 1e-4
    fd = (ds.logpdf(f + eps * v, d) - ds.logpdf(f - eps * v, d)) / (2 * eps)
    an = ds.dot(v, g)                                                         # logpdf is quadratic: central differences are exact up to rounding
    assert np.allclose(fd, an, rtol=1e-7, atol=0), (fd, an)


def test_logpdf_has_no_phi_term():
    s = N.sim("P", (32, 32))
    lens = s["so"]["ds"]
    zero = np.zeros_like(s["so"]["phi"])
    full = lens.logpdf(s["f"], zero, s["d"])                                  # ϕ = 0: the ϕ term is logdet Cϕ / 2 alone
    ldp = O.flatsky.logdet_fourier(lens.proj, lens.Cphi[None, None])
    assert np.allclose(s["ds"].logpdf(s["f"]), full + ldp / 2, rtol=1e-12)


def test_signatures_and_defaults():
    import cmblensing_jl_amd as C
    sig = inspect.signature(C.load_nolensing_sim)
    assert list(sig.parameters) == ["theta_pix", "Nside", "pol", "cls", "lensed_covariance", "lensed_data", "load_sim_kwargs"]
    assert sig.parameters["lensed_covariance"].default is False and sig.parameters["lensed_data"].default is False
    assert sig.parameters["load_sim_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    sig = inspect.signature(C.MAP_joint)
    assert list(sig.parameters) == ["ds", "nsteps", "phi_start", "fstart", "kw"] and sig.parameters["nsteps"].default == 20
    sig = inspect.signature(C.NoLensingDataSet.__init__)
    assert list(sig.parameters) == ["self", "proj", "P", "ops", "d", "logdet_sum"] and sig.parameters["logdet_sum"].default == 0.0
    sig = inspect.signature(C.NoLensingDataSet.argmaxf_logpdf)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [("d", None), ("fstart", None), ("tol", 1e-1), ("nsteps", 500)]
    sig = inspect.signature(C.NoLensingDataSet.gradientf_logpdf)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [("f", inspect.Parameter.empty), ("d", None), ("zero_d", False)]
    for name in ("mean", "simulate_data", "logpdf", "set_op", "set_data", "set_logdet", "noise_inv"):
        assert callable(getattr(C.NoLensingDataSet, name)), name
    assert set(C.NoLensingDataSet._ids) == {"Cf_inv", "Cn_inv", "B", "Mf", "precond_inv", "Mpix", "Cn_inv_pix"}      # nothing about ϕ
    assert C.BaseDataSet._ids["Cphi_inv"] == 7 and len(C.BaseDataSet._ids) == 11                                  # ... and BaseDataSet's did not move


def test_header_declares_and_binding_prototypes_the_new_symbols():
    from cmblensing_jl_amd import lib
    with open(os.path.join(ROOT, "include", "cmblens.h")) as f:
        header = f.read()
    assert re.search(r"^int cmbl_lensop_identity\(cmbl_ctx\* ctx, cmbl_lensop\*\* out\);", header, re.M)
    assert re.search(r"^int cmbl_nolensing_logpdf\(cmbl_dataset\* ds, const void\* f, const void\* d, double\* lp_host, void\* gf_out[^,]*, int nbatch\);", header, re.M)
    assert "cmbl_lensop_identity" in lib.SYMBOLS and len(lib.SIGNATURES["cmbl_lensop_identity"]) == 2
    assert "cmbl_nolensing_logpdf" in lib.SYMBOLS and len(lib.SIGNATURES["cmbl_nolensing_logpdf"]) == 6
    assert re.search(r"#define CMBL_ABI_VERSION 3\b", header) and lib.ABI_VERSION == 3       # additions do not bump it


def test_identity_passes_the_slot_check_and_has_no_pullback():
    import cmblensing_jl_amd as C
    from cmblensing_jl_amd import engine
    proj = types.SimpleNamespace(Ny=32, Nx=32, T="float32")
    L = C.IdentityLens.__new__(C.IdentityLens)                                # no device here: the slot check reads the type and the projection
    L._h, L.proj, L._phi = None, proj, None
    engine._check_lens_slot(proj, L, allow_factory=False)
    engine._check_lens_slot(proj, C.IdentityLens, allow_factory=True)         # as load_nolensing_sim hands it to load_sim
    with pytest.raises(ValueError):
        engine._check_lens_slot(types.SimpleNamespace(), L, allow_factory=False)
    assert L(None) is L and L.set_phi(None) is L                              # L(ϕ) returns itself
    ds = C.BaseDataSet.__new__(C.BaseDataSet)
    ds._h, ds.proj, ds._L = None, proj, L
    with pytest.raises(NotImplementedError, match=r"pullback of `L \\ f`"):
        C.MAP_joint(ds)
    with pytest.raises(NotImplementedError, match=r"pullback of `L \\ f`"):
        C.gibbs_step(ds, None, None, None, None, None)
