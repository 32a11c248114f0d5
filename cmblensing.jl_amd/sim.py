"""`load_sim` and the host-side operator algebra that feeds the device dataset.

Mirrors src/dataset.jl:186-338 (load_sim), src/cls.jl:11-35,288-309 (Cℓs, noiseCℓs, beamCℓs),
src/specialops.jl:61-118,232-241 (BlockDiagIEB, BandPass), src/proj_lambert.jl:173-175,361-371
(Cℓ_to_2D / Cℓ_to_Cov) and src/field_vectors.jl:64-84 (2x2 sqrt/pinv with the reference's symmetric-matrix
assumption).  Like the reference's own GPU extension (ext/CMBLensingCUDAExt.jl:46-49) the ℓ-space operator
planes are built once on the host; everything applied per iteration lives on the device.
"""
import numpy as np
import torch

from .engine import ProjLambert, BaseDataSet, Field, MAP, FOURIER, HARMONIC, make_mask


class Cls:
    """Tabulated spectrum with linear interpolation, NaN outside the table (src/cls.jl:11-29)."""

    def __init__(self, ell, cl):
        ell, cl = np.asarray(ell, float), np.asarray(cl, float)
        ok = ~np.isnan(cl)
        self.ell, self.cl = ell[ok], cl[ok]

    def __call__(self, l):
        l = np.asarray(l, float)
        out = np.interp(l, self.ell, self.cl)
        out[(l < self.ell[0]) | (l > self.ell[-1])] = np.nan
        return out


def _pinv(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = 1.0 / x
    r[~np.isfinite(r)] = 0
    return r


def cl_to_2d(cl, proj, units=None, dtype=np.float64):
    """nan2zero(Cℓ(ℓmag)) / units on the half-plane grid [x, ky] (src/proj_lambert.jl:173-175,362-364)."""
    v = cl(proj.lmag)
    v[~np.isfinite(v)] = 0
    return (v / (proj.Opix if units is None else units)).astype(dtype)


def noise_cls(muK_arcmin_T=3.0, lknee=100.0, alphaknee=3.0, lmax=8000):
    """src/cls.jl:288-299 with beamFWHM = 0"""
    ell = np.arange(2, lmax + 1)
    base = np.deg2rad(muK_arcmin_T / 60) ** 2 * (1 + (lknee / ell) ** alphaknee)
    return {"TT": Cls(ell, base), "EE": Cls(ell, 2 * base), "BB": Cls(ell, 2 * base), "TE": Cls(ell, 0 * base)}


def beam_cls(beam_fwhm=0.0, lmax=8000):
    """src/cls.jl:307-309"""
    ell = np.arange(2, lmax + 1, dtype=float)
    return Cls(ell, np.exp(-ell ** 2 * np.deg2rad(beam_fwhm / 60) ** 2 / (8 * np.log(2))))


def lowpass(l, dl=50):
    """LowPass(ℓ; Δℓ) (src/specialops.jl:236-240)"""
    ramp_up = (np.cos(np.linspace(np.pi, 0, dl)) + 1) / 2
    return Cls(np.arange(l + 1), np.r_[np.ones(l - dl + 1), 1 - ramp_up])


def border_mask(proj, pad_deg=1.0, apod_deg=1.0):
    """Deterministic cosine-apodised border mask [x, y] (input data; the reference's make_mask,
    src/masking.jl:1-25, additionally punches random point-source holes)."""
    def prof(n):
        d = (np.minimum(np.arange(n), n - 1 - np.arange(n)) + 0.5) * proj.theta_pix / 60
        t = np.clip((d - pad_deg) / max(apod_deg, 1e-30), 0, 1)
        return (1 - np.cos(np.pi * t)) / 2
    return np.outer(prof(proj.Nx), prof(proj.Ny))


class HarmOp:
    """Host-side real operator, diagonal in ℓ in the harmonic basis: npol diagonal planes, or for npol = 3 the
    BlockDiagIEB planes (TT, TE, ET, EE, BB) (src/specialops.jl:61-118)."""

    def __init__(self, planes):
        self.p = np.asarray(planes, dtype=np.float64)
        self.block = self.p.shape[0] == 5

    @staticmethod
    def from_cls(pol, proj, cls, units=None, te_zero=False):
        get = (lambda k: cls[k]) if isinstance(cls, dict) else (lambda k: cls)
        c = lambda k: cl_to_2d(get(k), proj, units)
        if pol == "I":
            return HarmOp([c("TT")])
        if pol == "P":
            return HarmOp([c("EE"), c("BB")])
        tt = c("TT")
        te = np.zeros_like(tt) if te_zero else c("TE")
        return HarmOp([tt, te, te, c("EE"), c("BB")])

    def __add__(self, o):
        if np.isscalar(o):
            q = self.p.copy()
            q[[0, 3, 4] if self.block else slice(None)] += o
            return HarmOp(q)
        return HarmOp(self.p + o.p)

    def scale(self, s):
        return HarmOp(self.p * s)

    def __matmul__(self, o):
        if not self.block:
            return HarmOp(self.p * o.p)
        a, b, c, d, e = self.p
        A, B, C, D, E = o.p
        return HarmOp([a * A + b * C, a * B + b * D, c * A + d * C, c * B + d * D, e * E])

    def T(self):
        return HarmOp(self.p[[0, 2, 1, 3, 4]]) if self.block else self

    def pinv(self):
        if not self.block:
            return HarmOp(_pinv(self.p))
        a, _, c, d, e = self.p                      # reads A[2,1] for both off-diagonals (src/field_vectors.jl:80-84)
        idet = _pinv(a * d - c * c)
        return HarmOp([d * idet, -(c * idet), -(c * idet), a * idet, _pinv(e)])

    def sqrt(self):
        if not self.block:
            return HarmOp(np.sqrt(self.p))
        a, _, c, d, e = self.p                      # src/field_vectors.jl:68-73
        s = np.sqrt(a * d - c * c)
        t = _pinv(np.sqrt(a + (d + 2 * s)))
        return HarmOp([t * (a + s), t * c, t * c, t * (d + s), np.sqrt(e)])

    def logdet(self, proj):
        """Σ λ·log|d| skipping non-finite (src/proj_lambert.jl:331-336, src/specialops.jl:96)"""
        planes = [self.p[0] * self.p[3] - self.p[2] * self.p[2], self.p[4]] if self.block else list(self.p)
        tot = 0.0
        for d in planes:
            with np.errstate(divide="ignore"):
                v = np.log(np.abs(d)) * proj.lam[None, :]
            tot += v[np.isfinite(v)].sum()
        return tot


def white_noise(seed, shape):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(shape)


def noise_from_white(ds, white):
    """n ~ 𝒩(0, Cn) from unit white-noise maps (B,P,Nx,Ny), HARMONIC: sqrt(Cn)·rfft(white) with the Fourier-diagonal `ds.host["Cn"]`
    (src/specialops.jl:6), or sqrt(V) ⊙ white in map space when the data set has the map-diagonal Cn = Diagonal(V) (`ds.host["Cn_pix"]`,
    load_sim(noise_var_map=...))."""
    proj, h = ds.proj, ds.host
    w = proj.tensor(white)
    if h.get("Cn_pix") is None:
        return Field(proj, proj.diag_apply(h["Cn"].sqrt().p, proj.rfft(w), HARMONIC, HARMONIC), HARMONIC)
    with np.errstate(invalid="ignore"):
        s = np.sqrt(h["Cn_pix"])
    s = proj.tensor(np.where(np.isfinite(s), s, 0.0))          # pixels of infinite variance carry no weight: no draw is made there
    return Field(proj, proj.map_fma(w, s.unsqueeze(0).expand(*w.shape).contiguous()), MAP).to(HARMONIC)


def load_sim(theta_pix, Nside, pol, cls, T=torch.float32, device=0, muK_arcmin_T=3.0, lknee=100.0, alphaknee=3.0,
             beam_fwhm=0.0, pixel_mask=None, bandpass_lmax=3000, nsteps=7, Nbatch=1, seeds=(1, 2, 3),
             Nphi=None, Nphi_fac=2, G=None, rng="host", pixel_mask_kwargs=None, L=None, noise_var_map=None, Cnhat=None):
    # Nphi: None / "qe" -> N⁰ of the quadratic estimator like the reference; "flat" -> cheap flat level; or an [x,ky] plane
    """`load_sim` (src/dataset.jl:186-338).  `cls`: dict group -> dict {TT,EE,BB,TE,pp} of Cls for the groups
    'unlensed_scalar', 'tensor', 'total' (e.g. decoded from the reference's dat/default_camb_Cls.jld2).
    `pixel_mask_kwargs`: a dict of `make_mask` keywords: Mpix = make_mask(proj; ...) made on the device (:279-281), its point sources drawn
    with `seed` = seeds[0] unless the dict says otherwise (the reference hands make_mask a copy of the simulation's rng).  `pixel_mask`: the
    keywords of the deterministic `border_mask` instead; giving both is a ValueError.
    `L`: the lensing operator of the data set (`load_sim(L = BilinearLens)`, :223): None = `LenseFlow(proj, nsteps)`, or a callable
    `proj -> operator` such as `BilinearLens` or `lambda p: PowerLens(p, 4)` (`BaseDataSet` has what each operator covers).
    `noise_var_map`: a noise variance map V in μK² per pixel, shape (P or 1, Nx, Ny) (host array or device tensor; one plane is shared by all
    pol slices): the noise covariance is then Cn = Diagonal(V) in the I/QU map basis, the inhomogeneous noise of a hit-count map (`BaseDataSet.Cn`
    is any operator, src/dataset.jl:37-47).  logdet Cn = Σ log V (`logdet(Diagonal(::Map))`, src/proj_lambert.jl:337-342; a shared plane counts P
    times; pixels of zero or infinite variance, whose weight pinv(V) is 0, are left out of the sum and get no noise draw), the noise realisation is
    sqrt(V) ⊙ white from the same white draws and seeds, and `muK_arcmin_T`, `lknee`, `alphaknee` are NOT read.
    `Cnhat`: the approximate, Fourier-diagonal Cn̂ (a `HarmOp`) that the preconditioner, the mixing matrix D, `quadratic_estimate` and
    `ds.host["Cn"]` read (:41, 129-132, 316-328); None = white noise at the harmonic-mean level 1 / mean(1/V) per plane, over the pixels with finite
    positive V.  (The reference defaults to Cn̂ = Cn, which is not diagonal in Cf's basis and so cannot be inverted mode by mode inside the
    preconditioner: the harmonic-mean default is this port's choice.)  V is kept as `ds.host["Cn_pix"]`, Σ log V as `ds.host["logdet_Cn"]`.
    Returns dict(f, phi, ftilde, d, ds, proj) with Fields on the device."""
    if pixel_mask is not None and pixel_mask_kwargs is not None:
        raise ValueError("load_sim: give pixel_mask (border_mask) or pixel_mask_kwargs (make_mask), not both")
    Ny, Nx = (Nside, Nside) if np.isscalar(Nside) else Nside
    proj = ProjLambert(Ny, Nx, theta_pix, T, device)
    P = {"I": 1, "P": 2, "IP": 3}[pol]
    lmax = proj.lmax
    ncl = noise_cls(muK_arcmin_T, lknee, alphaknee, lmax)
    mk = lambda c, **kw: HarmOp.from_cls(pol, proj, c, **kw)

    Cphi = cl_to_2d(cls["total"]["pp"], proj)                                   # :267
    Cfs, Cten = mk(cls["unlensed_scalar"]), mk(cls["tensor"])                  # :268-269
    Cf = Cfs + Cten                                                             # :273 at r = r₀
    Cn = mk(ncl)                                                                # :271-272
    Cn_pix = Cn_inv_pix = logdet_Cn = None
    if noise_var_map is not None:                                               # Cn = Diagonal(V) in the map basis; `Cn` below is Cn̂
        V = noise_var_map.detach().cpu().numpy() if torch.is_tensor(noise_var_map) else np.asarray(noise_var_map)
        Cn_pix = np.array(V, dtype=np.float64).reshape(-1, Nx, Ny)
        if Cn_pix.shape[0] not in (1, P):
            raise ValueError(f"load_sim: noise_var_map has {Cn_pix.shape[0]} planes, expected 1 or {P}")
        Cn_inv_pix = _pinv(Cn_pix)
        seen = np.isfinite(Cn_pix) & (Cn_pix > 0)                                 # pixels of zero or infinite variance carry no weight and no logdet term
        # summed here in double like the logdets of the Fourier-diagonal operators next to it (HarmOp.logdet): `proj.logdet_diag(V, MAP)` of a
        # float32 context rounds V and takes float32 logarithms, -1.5e-7 per pixel on average -- -9e-4 of 26793 at 32 x 64 T+QU, a third of the
        # float32 error of logpdf there
        logdet_Cn = float(np.sum(np.log(Cn_pix[seen]))) * (P // Cn_pix.shape[0])
        if Cnhat is None:
            good = [v[np.isfinite(v) & (v > 0)] for v in np.broadcast_to(Cn_pix, (P, Nx, Ny))]
            lv = [1.0 / np.mean(1.0 / g) for g in good]
            one = np.ones_like(Cphi)
            Cnhat = HarmOp([lv[0] * one, 0 * one, 0 * one, lv[1] * one, lv[2] * one] if P == 3 else [l * one for l in lv])
        Cn = Cnhat
    elif Cnhat is not None:
        raise ValueError("load_sim: Cnhat is the approximation of a map-diagonal noise covariance; it needs noise_var_map")
    Mf = mk(lowpass(bandpass_lmax), units=1, te_zero=True)                      # :279
    bcl = beam_cls(beam_fwhm, lmax)
    Bop = mk(Cls(bcl.ell, np.sqrt(bcl.cl)), units=1, te_zero=True)              # :300
    Mpix = border_mask(proj, **pixel_mask) if pixel_mask is not None else None
    if pixel_mask_kwargs is not None:
        Mpix = make_mask(proj, **{"seed": seeds[0], **pixel_mask_kwargs}).arr[0, 0].cpu().numpy().astype(np.float64)   # host form [x, y], like border_mask's

    qe_nphi = Nphi is None or (isinstance(Nphi, str) and Nphi == "qe")
    if qe_nphi or (isinstance(Nphi, str) and Nphi == "flat"):                   # provisional flat level until the data exist (see below)
        sel = (proj.lmag > 100) & (proj.lmag < 2000)
        Nphi = np.where(Cphi > 0, np.exp(np.mean(np.log(Cphi[sel]))), 0.0)
    Nphi = np.asarray(Nphi, float) / Nphi_fac
    Gp = np.ones_like(Cphi) if G is None else np.asarray(G, float)              # G(θ) ≡ I at fiducial θ (:317-320)
    s2len = np.deg2rad(5 / 60) ** 2
    D = ((Cf + (Cn.scale(2) + s2len)) @ Cf.pinv()).sqrt()                       # :322-328
    precond = Cf.pinv() + (Bop.T() @ Mf.T() @ Cn.pinv() @ Mf @ Bop)             # src/dataset.jl:129-132
    logdet_sum = Cf.logdet(proj) + (Cn.logdet(proj) if logdet_Cn is None else logdet_Cn) + HarmOp([Cphi]).logdet(proj)
    ops = dict(Cf_inv=Cf.pinv().p, Cn_inv=Cn.pinv().p, B=Bop.p, Mf=Mf.p, D=D.p, D_inv=D.pinv().p,
               precond_inv=precond.pinv().p, Cphi_inv=_pinv(Cphi)[None], G_inv=_pinv(Gp)[None], Mpix=Mpix, Cn_inv_pix=Cn_inv_pix)
    ds = BaseDataSet(proj, P, ops, logdet_sum=logdet_sum, nsteps=nsteps, L=L)
    Cft = mk(cls["total"])                                                     # Cf̃ (:270)
    ds.host = dict(Cf=Cf, Cn=Cn, Cphi=Cphi, Mf=Mf, B=Bop, D=D, Nphi=Nphi, G=Gp, Mpix=Mpix, precond=precond, Cftilde=Cft,
                   Cfs=Cfs, Cten=Cten, r0=0.2, Aphi0=1.0, s2len=s2len, Cn_pix=Cn_pix, logdet_Cn=logdet_Cn)
    if G is not None:
        ds.host["G_user"] = Gp.copy()                                           # theta.set_theta keeps a user-supplied G at fiducial Aϕ           # θ layer (theta.py): r₀ = Cℓ.params.r, Aϕ₀ = 1 (:239,250)

    # simulate: x = sqrt(C)·rfft(white)   (src/specialops.jl:6), white ~ NumPy PCG64(seed) uploaded, or with rng="device"
    # drawn on the GPU (cmbl_randn: Philox4x32-10, batch slot b keyed by seed + 1000003*b)
    def sim(op_planes, seed, Pp):
        if rng == "device":
            w = proj.randn([seed + 1000003 * b for b in range(Nbatch)], 0, Pp)
        else:
            w = proj.tensor(white_noise(seed, (Nbatch, Pp, Nx, Ny)))
        return Field(proj, proj.diag_apply(op_planes, proj.rfft(w), HARMONIC, HARMONIC), HARMONIC)
    f = sim(Cf.sqrt().p, seeds[0], P)
    phi = sim(np.sqrt(Cphi)[None], seeds[1], 1)
    phi = Field(proj, phi.arr, FOURIER)
    if Cn_pix is None:
        n = sim(Cn.sqrt().p, seeds[2], P)
    else:                                                                        # sqrt(V) ⊙ white, the same white draw
        n = noise_from_white(ds, proj.randn([seeds[2] + 1000003 * b for b in range(Nbatch)], 0, P) if rng == "device"
                             else white_noise(seeds[2], (Nbatch, P, Nx, Ny)))
    ftilde = ds.L(phi) * f                                                       # map
    d = ds.mean(f, phi) + n                                                      # M·B·L(ϕ)·f + n  (src/dataset.jl:59-66)
    ds.set_data(d)
    if qe_nphi:                                                                 # ds.Nϕ = quadratic_estimate(ds).Nϕ / Nϕ_fac   (:316)
        from .drivers import quadratic_estimate
        ds.host["Nphi"] = quadratic_estimate(ds)["Nphi"] / Nphi_fac
    return dict(f=f, phi=phi, ftilde=ftilde, d=d, n=n, ds=ds, proj=proj)
