"""Pins tests/_theta_grad_ref.py (the float64 restatement of the θ-gradient) to the oracle: Richardson central differences of
`ThetaDataSet.logpdf_mixed` and of `ThetaDataSet.at(...)[0].logpdf` at two step sizes, h and h/2.

    D(h) = (lp(θ + h) − lp(θ − h)) / 2h,   R(h) = (4 D(h/2) − D(h)) / 3        (error O(h⁴))
The yardstick's own error is ε = |R(h) − R(h/2)| plus the rounding floor 4·eps·|lp|/h.  Asserted per parameter:
|ref − R(h/2)| <= 3ε + floor, and that bound is below 1e-6·S with S = |explicit| + |cross| + |logdet term| (for r and Aϕ the last two are
10³–10⁴ times the result and nearly cancel, so nothing is stated relative to the result itself).  h is 1 % of the parameter's value.

The number of ODE steps of the oracle's LenseFlow is 40 here, not the default 7.  The cross term of Aϕ uses the oracle's gϕ°, which is the RK4
δ-flow (the transpose of the continuous flow, src/flowops.jl:40-68), not the derivative of the discrete forward flow the differences see; the
two meet as nsteps⁻⁴.  Measured |ref − R(h/2)| for Aϕ, QU 32x32: 8.0e-6 (7 steps), 6.7e-7 (14), 5.0e-8 (28), against 3ε + floor = 1.5e-7 --
at 7 steps that is 1e-8·S, the δ-flow's own error, and nothing of the θ formulas.  r, the amplitudes and the unmixed form do not involve gϕ°
and meet the bound at any step count."""
import functools

import numpy as np
import pytest

import oracle as O
from oracle.theta import ThetaDataSet

from _theta_grad_ref import ThetaGradRef

LE = [100, 600, 1500, 3000]                       # the three bands of tests/test_gpu_theta_device.py
BANDS = {"P": None, "IP": {"ATT": ([0], LE), "ATE": ([1, 2], LE), "AEE": ([3], LE)}}
AMPS = {"P": None, "IP": {"ATT": np.array([1.3, 1.0, 0.8]), "ATE": np.array([0.9, 1.1, 1.0]), "AEE": np.array([1.2, 0.85, 1.05])}}
CASES = {"QU 32x32": ("P", (32, 32)), "T+QU 32x64": ("IP", (32, 64))}
R, APHI = 0.25, 1.1
NSTEPS = 40
EPS = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def _case(name):
    pol, Nside = CASES[name]
    so = O.load_sim(3.0, Nside, pol, np.float64, beam_fwhm=1.0, pixel_mask=dict(pad_deg=0.4, apod_deg=0.4), nsteps=NSTEPS)
    ref = ThetaGradRef(so["ds"], so["Cfs"], so["Cten"], bands=BANDS[pol])
    th = ThetaDataSet(so["ds"], so["Cfs"], so["Cten"], bands=BANDS[pol])
    fo, po = so["ds"].mix(so["f"], so["phi"])
    return so, ref, th, fo, po, AMPS[pol]


def _richardson(fun, h):
    """(R(h), R(h/2), |lp|) of the scalar function `fun` of a step"""
    D = lambda s: (fun(s) - fun(-s)) / (2 * s)
    d1, d2, d4 = D(h), D(h / 2), D(h / 4)
    return (4 * d2 - d1) / 3, (4 * d4 - d2) / 3, abs(fun(0.0))


def _params(amps):
    out = [("r", None, R), ("Aphi", None, APHI)]
    for name, a in (amps or {}).items():
        out += [(name, i, float(a[i])) for i in range(len(a))]
    return out


def _theta(amps, key, i, step):
    kw = dict(r=R, Aphi=APHI, **{k: v.copy() for k, v in (amps or {}).items()})
    if i is None:
        kw[key] += step
    else:
        kw[key][i] += step
    return kw


def _check(label, got, S, fun, value):
    h = 0.01 * abs(value)
    r1, r2, lp = _richardson(fun, h)
    eps_r = abs(r1 - r2)
    floor = 4 * EPS * lp / h
    bound = 3 * eps_r + floor
    diff = abs(got - r2)
    print(f"[{label}] ref {got:+.9e}  R(h/2) {r2:+.9e}  diff {diff:.2e}  eps {eps_r:.2e}  floor {floor:.2e}  S {S:.3e}  bound/S {bound / S:.2e}")
    assert bound < 1e-6 * S, f"{label}: the yardstick's own error {bound:.3e} is not below 1e-6 S = {1e-6 * S:.3e}"
    assert diff <= bound, f"{label}: |ref - R(h/2)| = {diff:.3e} > 3 eps + floor = {bound:.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_chain_is_the_oracles(name):
    """the restated chain gives the oracle's own value and gradient (it only exposes the intermediates)"""
    so, ref, th, fo, po, amps = _case(name)
    lp, _, ch = ref.mixed(fo, po, R, APHI, amps)
    ds, ldD, ldG = th.at(R, APHI, **(amps or {}))
    lp_o, gfo_o, gpo_o = ds.grad_logpdf_mixed(fo, po)
    assert np.array_equal(lp, lp_o - ldD - ldG)
    assert np.array_equal(ch["gphio"], gpo_o) and np.array_equal(ch["gfo"].astype(gfo_o.dtype), gfo_o)
    assert np.array_equal(lp, th.logpdf_mixed(fo, po, r=R, Aphi=APHI, **(amps or {})))


@pytest.mark.parametrize("name", list(CASES))
def test_mixed_gradient_against_richardson(name):
    so, ref, th, fo, po, amps = _case(name)
    _, grad, _ = ref.mixed(fo, po, R, APHI, amps)
    print()
    for key, i, value in _params(amps):
        g = grad[key]
        got, S = (g["total"][0], g["S"][0]) if i is None else (g["total"][0, i], g["S"][0, i])
        fun = lambda s: float(th.logpdf_mixed(fo, po, **_theta(amps, key, i, s))[0])
        _check(f"{name} mixed {key}{'' if i is None else [i]}", got, S, fun, value)


@pytest.mark.parametrize("name", list(CASES))
def test_unmixed_gradient_against_richardson(name):
    so, ref, th, fo, po, amps = _case(name)
    f, phi = so["f"], so["phi"]
    grad = ref.unmixed(f, phi, R, APHI, amps)
    print()
    for key, i, value in _params(amps):
        g = grad[key]
        got, S = (g["total"][0], g["S"][0]) if i is None else (g["total"][0, i], g["S"][0, i])
        fun = lambda s: float(th.at(**_theta(amps, key, i, s))[0].logpdf(f, phi)[0])
        _check(f"{name} unmixed {key}{'' if i is None else [i]}", got, S, fun, value)


def test_one_parameter_named():
    """a parameter that θ does not name has no entry, and naming r alone leaves Aϕ's operators fiducial"""
    so, ref, th, fo, po, _ = _case("QU 32x32")
    _, grad, _ = ref.mixed(fo, po, r=R)
    assert list(grad) == ["r"]
    g = grad["r"]
    fun = lambda s: float(th.logpdf_mixed(fo, po, r=R + s)[0])
    _check("QU 32x32 mixed r alone", g["total"][0], g["S"][0], fun, R)
