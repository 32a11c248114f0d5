"""θ layer: the parameter-dependent operators of `load_sim` and the Gibbs θ pass of `sample_joint`.

    src/dataset.jl:272-274,316-328   Cf(r) = Cfs + (r/r₀) Cft,  Cϕ(Aϕ) = Aϕ Cϕ₀,  G(Aϕ) = G₀⁻¹ sqrt(I + 2 Nϕ Cϕ(Aϕ)⁻¹),
                                     D(r) = sqrt((Cf(r) + σ²len + 2 Cn̂) Cf(r)⁻¹)
    src/dataset.jl:84-87             logpdf(Mixed; θ) = logpdf(ds; unmix(θ)) − logdet(D,θ) − logdet(G,θ)
    src/generic.jl:264-271           logdet(L,θ) = logdet(L()⁻¹ L(θ)) when θ names a parameter of L, else 0
    src/sampling.jl:80-135,427-437   grid_and_sample, gibbs_sample_slice_θ!
Like the reference's ParamDependentOp (src/specialops.jl:314-330: recompute on the host side of the storage, then adapt) the ℓ-space
planes are recomputed on the host for each θ and uploaded (a handful of (Nx, Ny/2+1) planes); every field operation stays on the
device.  The grid of a Gibbs θ pass need not go that way: `logpdf_mixed_theta_grid` (`gibbs_sample_theta(on="device")`) installs what `_ops`
reads on the device once and has a kernel make the four operator sets and the log-determinants of every grid point there (csrc/kernels_theta.hpp;
`_ops` stays the definition of every formula).  The smoothing / quadrature inside grid_and_sample are Loess.jl / QuadGK / Roots in the reference -- third-party numerics
whose outputs are not pinned; here: local-quadratic LOESS with tricube weights and a trapezoid CDF on a fine grid.
"""
import ctypes

import numpy as np
import torch

from .engine import LenseFlow, MAP, FOURIER, HARMONIC, _ptr
from .lib import check
from .sim import HarmOp, _pinv


# ---- bandpower amplitudes (src/proj_lambert.jl:374-411) ----------------------------------------------------------------------
def findbin(ledges, l):
    """bin index (0-based) of every ℓ in the half-open bins [ℓedges[i], ℓedges[i+1]); out of range -> len(ledges) - 1, the slot of
    the constant amplitude 1 that `bandpower_rescale` appends (src/proj_lambert.jl:402-404)"""
    ledges, l = np.asarray(ledges, float), np.asarray(l, float)
    idx = np.searchsorted(ledges, l, side="right") - 1               # findfirst(>(ℓ), ℓedges) - 1
    return np.where((l < ledges[0]) | (l >= ledges[-1]), len(ledges) - 1, idx)


def bandpower_rescale(plane, bin_idx, amplitudes):
    """`[amplitudes; 1][ℓbin_indices] .* arr` (src/proj_lambert.jl:405-408)"""
    a = np.append(np.asarray(amplitudes, float), 1.0)
    return a[bin_idx] * plane


class BinRescaledCov:
    """`Cℓ_to_Cov(pol, proj, (Cℓ, ℓedges, θname), ...)`: a covariance whose TT / EE / TE planes are rescaled by one amplitude per
    ℓ-bin (ParamDependentOp over the amplitude vectors; BB is never rescaled, like the reference).  `bands` maps a spectrum
    ("TT", "EE", "TE") to (ℓedges, θname); `op(**θ)` gives the HarmOp at the named amplitudes (default: all ones)."""

    def __init__(self, pol, proj, cls, bands):
        self.C0 = HarmOp.from_cls(pol, proj, cls)
        self.pol = pol
        plane_of = {"I": {"TT": [0]}, "P": {"EE": [0]}, "IP": {"TT": [0], "TE": [1, 2], "EE": [3]}}[pol]
        self.bands = {}
        for spec, (ledges, name) in bands.items():
            if spec not in plane_of:
                raise ValueError(f"no rescalable {spec} spectrum for pol={pol} (BB is fixed, src/proj_lambert.jl:385-393)")
            self.bands[name] = (plane_of[spec], findbin(ledges, proj.lmag), len(ledges) - 1)
        self.names = list(self.bands)

    def __call__(self, **theta):
        p = self.C0.p.copy()
        for name, (planes, idx, nb) in self.bands.items():
            amps = theta.get(name)
            amps = np.ones(nb) if amps is None else np.asarray(amps, float)
            assert amps.shape == (nb,), f"{name}: expected {nb} amplitudes"
            for k in planes:
                p[k] = bandpower_rescale(self.C0.p[k], idx, amps)
        return HarmOp(p)


def _ops(ds, r, Aphi, bands=None):
    h = ds.host
    proj = ds.proj
    out, logdet_mix = {}, 0.0
    Cfs = h["Cfs_bands"](**(bands or {})) if "Cfs_bands" in h else h["Cfs"]       # bandpower amplitudes rescale the scalar part
    Cf = Cfs + h["Cten"].scale((h["r0"] if r is None else r) / h["r0"])
    Cphi0 = np.asarray(h.get("Cphi0", h["Cphi"]), float)
    Cphi = Cphi0 * (h["Aphi0"] if Aphi is None else Aphi) / h["Aphi0"]
    Dof = lambda C: ((C + (h["Cn"].scale(2) + h["s2len"])) @ C.pinv()).sqrt()
    # D closes over the covariance load_sim built and names r only (src/dataset.jl:322-328): bandpower amplitudes do not enter it
    D = Dof(h["Cfs"] + h["Cten"].scale((h["r0"] if r is None else r) / h["r0"]))
    if r is not None:
        D0 = Dof(h["Cfs"] + h["Cten"])
        logdet_mix += (D0.pinv() @ D).logdet(proj)
    Nphi = np.asarray(h["Nphi"], float)
    G = np.ones_like(Cphi0) if "G_user" not in h else np.asarray(h["G_user"], float)
    if Aphi is not None and "G_user" not in h:      # a user-supplied G stays constant: `if G == nothing` (src/dataset.jl:317-320), logdet(G,θ) = 0
        g0 = np.sqrt(1 + 2 * Nphi * _pinv(Cphi0))
        G = _pinv(g0) * np.sqrt(1 + 2 * Nphi * _pinv(Cphi))
        logdet_mix += HarmOp([G]).logdet(proj)
    precond = Cf.pinv() + (h["B"].T() @ h["Mf"].T() @ h["Cn"].pinv() @ h["Mf"] @ h["B"])
    out = dict(Cf_inv=Cf.pinv().p, D=D.p, D_inv=D.pinv().p, precond_inv=precond.pinv().p, Cphi_inv=_pinv(Cphi)[None], G_inv=_pinv(G)[None])
    logdet_Cn = h["logdet_Cn"] if h.get("logdet_Cn") is not None else h["Cn"].logdet(proj)     # Σ log V of a map-diagonal Cn (load_sim(noise_var_map=...))
    logdet_sum = Cf.logdet(proj) + logdet_Cn + HarmOp([Cphi]).logdet(proj)
    return out, logdet_sum, logdet_mix, dict(Cf=Cf, Cphi=Cphi, D=D, G=G, precond=precond)


def use_bandpowers(ds, bands, cls_scalar):
    """Make the scalar part of `ds.Cf` a bandpower-rescaled covariance: `bands` = {"EE": (ℓedges, "AEE"), ...}
    (`ds.Cf = Cℓ_to_Cov(pol, proj, (Cℓ, ℓedges, :AEE), ...)` in the reference).  The amplitude vectors then are parameters of
    `set_theta` / `logpdf_mixed_theta` / the Gibbs θ pass, next to r and Aϕ."""
    pol = {1: "I", 2: "P", 3: "IP"}[ds.P]
    ds.host["Cfs_bands"] = BinRescaledCov(pol, ds.proj, cls_scalar, bands)


def set_theta(ds, r=None, Aphi=None, **bands):
    """Evaluate the dataset's ParamDependentOps at θ = (r, Aϕ[, bandpower amplitude vectors]) (`ds(θ)`, src/dataset.jl:23-31) and
    make them current on the device; a parameter left None is 'not named in θ': its operators stay fiducial and its logdet term is
    0.  `set_theta(ds)` restores the fiducial dataset."""
    h = ds.host
    h.setdefault("Cphi0", np.asarray(h["Cphi"], float).copy())
    if bands and "Cfs_bands" not in h:
        raise ValueError("bandpower amplitudes given but the dataset has no bandpower covariance (theta.use_bandpowers)")
    ops, logdet_sum, logdet_mix, host = _ops(ds, r, Aphi, bands)
    for k, v in ops.items():
        ds.set_op(k, v)
    ds.set_logdet(logdet_sum)
    ds.logdet_mix = float(logdet_mix)
    h.update(host)
    ds.L.invalidate()
    ds.theta = dict(r=r, Aphi=Aphi, **bands)


def logpdf_mixed_theta(ds, fo, po, r=None, Aphi=None, **bands):
    """logpdf(Mixed(ds); f°, ϕ°, θ) (src/dataset.jl:84-87), per batch slot; leaves the dataset at θ"""
    set_theta(ds, r, Aphi, **bands)
    return ds.logpdf_mixed(fo, po)


# ---- the θ layer on the device (cmbl_dataset_theta_model / cmbl_logpdf_mixed_theta, include/cmblens.h) ---------------------------------
_pd = ctypes.POINTER(ctypes.c_double)
_pi = ctypes.POINTER(ctypes.c_int)
_MODEL_KEYS = ("Cfs", "Cten", "Cn", "Cphi0", "Nphi", "Cfs_bands", "G_user", "logdet_Cn")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _dp(a):
    return None if a is None else a.ctypes.data_as(_pd)


def _install_theta_model(ds):
    """install on the device what `_ops` reads (once; again when one of the host entries it was built from is another object)"""
    h = ds.host
    h.setdefault("Cphi0", np.asarray(h["Cphi"], float).copy())
    key = tuple(h.get(k) for k in _MODEL_KEYS)
    scal = (float(h["s2len"]), float(h["r0"]), float(h["Aphi0"]))
    old = getattr(ds, "_theta_model", None)
    if old is not None and all(a is b for a, b in zip(old[0], key)) and old[1] == scal:
        return
    Cfs, Cten, Cn = (_f64(h[k].p) for k in ("Cfs", "Cten", "Cn"))
    cb = h.get("Cfs_bands")
    C0 = planes = idx = nbins = None
    nbands = 0
    if cb is not None:
        C0 = _f64(cb.C0.p)
        nbands = len(cb.bands)
        planes = np.array([sum(1 << k for k in pl) for pl, _, _ in cb.bands.values()], dtype=np.int32)
        idx = np.ascontiguousarray(np.stack([i for _, i, _ in cb.bands.values()]) if nbands else np.zeros(0), dtype=np.int32)
        nbins = np.array([nb for _, _, nb in cb.bands.values()], dtype=np.int32)
    Cphi0, Nphi = _f64(h["Cphi0"]), _f64(h["Nphi"])
    G = _f64(h["G_user"]) if "G_user" in h else None
    logdet_Cn = h["logdet_Cn"] if h.get("logdet_Cn") is not None else h["Cn"].logdet(ds.proj)
    check(ds.lib.cmbl_dataset_theta_model(ds._h, _dp(Cfs), Cfs.shape[0], _dp(C0), nbands, None if planes is None else planes.ctypes.data_as(_pi),
                                          None if idx is None else ctypes.c_void_p(idx.ctypes.data), None if nbins is None else nbins.ctypes.data_as(_pi),
                                          _dp(Cten), _dp(Cn), scal[0], scal[1], _dp(Cphi0), scal[2], _dp(Nphi), _dp(G), float(logdet_Cn)))
    ds._theta_model = (key, scal)


def _theta_rows(ds, thetas):
    """(r, Aϕ, amplitude rows or None) of a list of θ dicts; a parameter that is None or absent is 'not named': NaN / ones"""
    cb = ds.host.get("Cfs_bands")
    names = list(cb.bands) if cb is not None else []
    nan = float("nan")
    r = np.array([nan if th.get("r") is None else float(th["r"]) for th in thetas], dtype=np.float64)
    A = np.array([nan if th.get("Aphi") is None else float(th["Aphi"]) for th in thetas], dtype=np.float64)
    for th in thetas:
        extra = [k for k in th if k not in ("r", "Aphi") and k not in names]
        if extra:
            raise ValueError(f"bandpower amplitudes {extra} given but the dataset has no such bandpower covariance (theta.use_bandpowers)")
    if not names or all(th.get(n) is None for th in thetas for n in names):
        return r, A, None
    rows = [np.concatenate([np.ones(cb.bands[n][2]) if th.get(n) is None else np.asarray(th[n], float).ravel() for n in names]) for th in thetas]
    if len({len(x) for x in rows}) != 1:
        raise ValueError("the θ of one grid call must give each amplitude vector with the same length")
    return r, A, _f64(np.stack(rows))


def logpdf_mixed_theta_grid(ds, fo, po, thetas):
    """logpdf(Mixed(ds); f°, ϕ°, θ) for every θ of `thetas` (dicts as `set_theta` takes them) -> (len(thetas), B), in ONE library call: per θ a
    pointwise kernel makes pinv(Cf), pinv(D), pinv(Cϕ), pinv(G) and the log-determinants on the device from the resident model and the value is
    the library's `logpdf_mixed`; only scalars cross to the host.  `ds.ops`, `ds.host`, `ds.theta`, `ds.logdet_sum` and `ds.logdet_mix` are not
    touched: the data set stays at the θ it had.  The model is installed on first use and kept while the host entries it was built from
    (`Cfs`, `Cten`, `Cn`, `Cphi0`, `Nphi`, `Cfs_bands`, `G_user`, `logdet_Cn`) are the same objects."""
    if not isinstance(ds.L, LenseFlow):
        raise ValueError(f"logpdf_mixed_theta_grid: the library's logpdf_mixed is defined for a LenseFlow in ds.L, not {type(ds.L).__name__}")
    thetas = list(thetas)
    fo, po = fo.to(MAP), po.to(FOURIER)
    _install_theta_model(ds)
    r, A, amps = _theta_rows(ds, thetas)
    B, n = fo.arr.shape[0], len(thetas)
    lp = np.empty((n, B), dtype=np.float64)
    ds.L.invalidate()
    check(ds.lib.cmbl_logpdf_mixed_theta(ds._h, ds.L._h, _ptr(fo.arr), _ptr(po.arr), B, n, _dp(r), _dp(A), _dp(amps), 0 if amps is None else amps.shape[1], _dp(lp)))
    return lp


WANT_R, WANT_APHI, WANT_AMPS = 1, 2, 4          # CMBL_THETA_R, _APHI, _AMPS


def _theta_grad_call(ds, theta, B):
    """what the two θ-gradient calls share: the model, the row of θ, the `want` mask of the parameters θ names and the output array"""
    _install_theta_model(ds)
    theta = {k: v for k, v in dict(theta).items() if v is not None}
    r, A, amps = _theta_rows(ds, [theta])
    want = (WANT_R if "r" in theta else 0) | (WANT_APHI if "Aphi" in theta else 0) | (WANT_AMPS if amps is not None else 0)
    if not want:
        raise ValueError("the θ-gradient needs a θ that names at least one parameter")
    namps = 0 if amps is None else amps.shape[1]
    return theta, float(r[0]), float(A[0]), amps, namps, want, np.zeros((B, 2 + namps), dtype=np.float64)


def _theta_grad_dict(ds, theta, grad):
    """rows of [d/dr, d/dAϕ, bands concatenated in install order] -> {name: (B,) or (B, nbins)} for the parameters θ names"""
    out = {}
    if "r" in theta:
        out["r"] = grad[:, 0].copy()
    if "Aphi" in theta:
        out["Aphi"] = grad[:, 1].copy()
    cb, off = ds.host.get("Cfs_bands"), 2
    for name in (cb.names if cb is not None else []):
        nb = cb.bands[name][2]
        if name in theta:
            out[name] = grad[:, off:off + nb].copy()
        off += nb
    return out


def grad_theta_logpdf(ds, f, phi, theta):
    """∂/∂θ logpdf(ds; f, ϕ, θ) at fixed fields, per batch slot: {name: (B,) for r and Aϕ, (B, nbins) for a bandpower amplitude vector}, for
    the parameters `theta` (a dict as `set_theta` takes it) names -- what the reference gets by automatic differentiation for MUSE's
    ∇θ_logLike (ext/CMBLensingMuseInferenceExt.jl:52-54).  One library call (cmbl_grad_theta_logpdf): a kernel differentiates the formulas of
    the θ operators in forward mode; no lensing operator is involved, the data term does not depend on θ.  The model is installed as
    `logpdf_mixed_theta_grid` does; `ds.ops`, `ds.host`, `ds.theta`, `ds.logdet_sum` and `ds.logdet_mix` are not touched."""
    f, phi = f.to(HARMONIC), phi.to(FOURIER)
    B = f.arr.shape[0]
    if phi.arr.shape[0] != B:
        if phi.arr.shape[0] != 1:
            raise ValueError(f"grad_theta_logpdf: {phi.arr.shape[0]} planes of ϕ for {B} slots of f")
        phi = type(phi)(phi.proj, phi.arr.expand(B, *phi.arr.shape[1:]).contiguous(), FOURIER)
    theta, r, A, amps, namps, want, grad = _theta_grad_call(ds, theta, B)
    fa, pa = f.arr.contiguous(), phi.arr.contiguous()
    check(ds.lib.cmbl_grad_theta_logpdf(ds._h, _ptr(fa), _ptr(pa), B, r, A, _dp(amps), namps, want, _dp(grad)))
    return _theta_grad_dict(ds, theta, grad)


def grad_theta_logpdf_mixed(ds, fo, po, theta):
    """(logpdf(Mixed(ds); f°, ϕ°, θ) (B,), its θ-gradient {name: (B,) or (B, nbins)}) at one θ, in ONE library call
    (cmbl_grad_theta_logpdf_mixed): the operators of θ are made on the device as in `logpdf_mixed_theta_grid`, the library's gradient of
    logpdf(Mixed) runs on them, and one more pass forms, next to the explicit derivative, −⟨ĝ, ∂D/∂r f⟩ − ∂logdet(D₀⁻¹D)/∂r for r and
    −⟨gϕ°, ∂lnG/∂Aϕ ϕ°⟩ − ∂logdet G/∂Aϕ for Aϕ.  Those two terms are 10³–10⁴ times the result and nearly cancel: the result is as accurate as
    they are.  The value is bit for bit the grid's at that θ.  The data set stays at the θ it had."""
    if not isinstance(ds.L, LenseFlow):
        raise ValueError(f"grad_theta_logpdf_mixed: the library's gradient of logpdf(Mixed) is defined for a LenseFlow in ds.L, not {type(ds.L).__name__}")
    fo, po = fo.to(MAP), po.to(FOURIER)
    B = fo.arr.shape[0]
    theta, r, A, amps, namps, want, grad = _theta_grad_call(ds, theta, B)
    lp = np.empty(B, dtype=np.float64)
    ds.L.invalidate()
    check(ds.lib.cmbl_grad_theta_logpdf_mixed(ds._h, ds.L._h, _ptr(fo.arr), _ptr(po.arr), B, r, A, _dp(amps), namps, want, _dp(lp), _dp(grad)))
    return lp, _theta_grad_dict(ds, theta, grad)


def theta_ops_device(ds, which, r=None, Aphi=None, **bands):
    """TESTING AID (`cmbl_dataset_theta_ops`): the operator set `which` ("Cf_inv", "D_inv", "Cphi_inv", "G_inv") that the θ kernel makes at one θ,
    as a device tensor in the reference layout, and the three sums (logdet Cf + logdet Cϕ, logdet(D0⁻¹ D), logdet G)"""
    _install_theta_model(ds)
    rr, A, amps = _theta_rows(ds, [dict(r=r, Aphi=Aphi, **bands)])
    npl = ds.host["Cfs"].p.shape[0] if which in ("Cf_inv", "D_inv") else 1
    out = torch.empty((npl, ds.proj.Nx, ds.proj.Nyh), dtype=ds.proj.T, device=ds.proj.device)
    sums = np.empty(3)
    check(ds.lib.cmbl_dataset_theta_ops(ds._h, float(rr[0]), float(A[0]), _dp(amps), 0 if amps is None else amps.shape[1], ds._ids[which], _ptr(out), _dp(sums)))
    return out, sums


def loess(xs, ys, x, span=0.25, degree=2):
    """local polynomial regression, tricube weights over the ceil(span·n) nearest points, evaluated at x"""
    xs, ys, x = np.asarray(xs, float), np.asarray(ys, float), np.atleast_1d(np.asarray(x, float))
    n = len(xs)
    q = int(min(n, max(degree + 1, np.ceil(span * n))))
    out = np.empty_like(x)
    for i, x0 in enumerate(x):
        d = np.abs(xs - x0)
        idx = np.argpartition(d, q - 1)[:q]
        hmax = d[idx].max()
        w = np.maximum((1 - (d[idx] / hmax) ** 3) ** 3 if hmax > 0 else np.ones(q), 1e-12)
        A = np.vander(xs[idx] - x0, degree + 1, increasing=True)
        out[i] = np.linalg.lstsq(A * np.sqrt(w)[:, None], ys[idx] * np.sqrt(w), rcond=None)[0][0]
    return out


def grid_and_sample(logpdfs, xs, u, span=0.25, nfine=2001):
    """`grid_and_sample(logpdfs, xs)` (src/sampling.jl:91-131) with the uniform draw `u` injected: trim non-finite ends, subtract
    the maximum, smooth the log pdf, normalise, inverse-transform sample.  -> (sample, (x_fine, log pdf), log pdf at xs)"""
    xs, lp = np.asarray(xs, float), np.asarray(logpdfs, float)
    fin = np.flatnonzero(np.isfinite(lp))
    xs, lp = xs[fin[0]:fin[-1] + 1], lp[fin[0]:fin[-1] + 1]
    lp = lp - lp.max()
    xf = np.linspace(xs[0], xs[-1], nfine)
    sm = loess(xs, lp, xf, span)
    p = np.nan_to_num(np.exp(sm))
    cdf = np.concatenate([[0.0], np.cumsum((p[1:] + p[:-1]) / 2 * np.diff(xf))])
    logA = np.log(cdf[-1])
    return float(np.interp(u, cdf / cdf[-1], xf)), (xf, sm - logA), loess(xs, lp, xs, span) - logA


def gibbs_sample_theta(ds, fo, po, theta, key, xs, u, span=0.25, on="host"):
    """`gibbs_sample_slice_θ!(k)` (src/sampling.jl:427-437): conditional of θ[key] given (f°, ϕ°) and the other parameters, on the grid
    `xs`, one draw per batch slot with uniforms `u`.  Returns (new value per slot, log pdf grid (nslots, len(xs))).
    on="host": every grid point through `set_theta` (the data set is left at the last one); on="device": the whole grid from one
    `logpdf_mixed_theta_grid` call, the data set stays where it was."""
    if on not in ("host", "device"):
        raise ValueError(f'on must be "host" or "device", got {on!r}')
    grid = [dict(theta, **{key: float(x)}) for x in xs]
    if on == "device":
        lps = logpdf_mixed_theta_grid(ds, fo, po, grid).T       # (B, nx)
    else:
        lps = np.array([logpdf_mixed_theta(ds, fo, po, **th) for th in grid]).T
    out = [grid_and_sample(lps[b], xs, u[b], span) for b in range(lps.shape[0])]
    return np.array([o[0] for o in out]), np.array([o[2] for o in out])
