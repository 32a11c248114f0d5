"""The reference side of the pixel-noise tests: a float64 NumPy yardstick for a noise covariance that is diagonal in the I/QU MAP basis,
Cn = Diagonal(V) with V a variance per pixel (`BaseDataSet.Cn` is any operator, src/dataset.jl:37-47; `pinv(Cn(θ))` is all `gradientf_logpdf`
asks of it, :76-80; `logdet(Diagonal(::Map))`, src/proj_lambert.jl:337-342).  `oracle.dataset.DataSet` is duck-typed in `Cn`: it calls
`.pinv()`, `.sqrt()` (callables on harmonic arrays) and `.logdet(proj)` and nothing else, so `PixNoise` drops in and the data model, the Wiener
filter and the posterior are the oracle's own code.  The approximate, Fourier-diagonal Cn̂ is passed explicitly (`Cnhat`): the preconditioner
and the mixing matrix D read it.  tests/test_pixnoise_ref.py pins this file by properties."""
import numpy as np

import oracle as O
from oracle.dataset import HarmOp, DataSet, to_harm, from_harm


class PixNoise:
    """Diagonal(V)^power in the I/QU map basis acting on harmonic arrays (B,P,Nx,Nyh): harmonic -> map -> x V^power (non-finite -> 0) -> harmonic.
    V: (P or 1, Nx, Ny); P: the pol slices the operator acts on (default: the planes of V) -- a plane shared by P slices counts P times in logdet."""

    def __init__(self, proj, V, power=1.0, P=None):
        self.proj, self.V, self.power = proj, np.asarray(V, np.float64), power
        self.P = self.V.shape[0] if P is None else P

    def weights(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            w = self.V ** self.power
        return np.where(np.isfinite(w), w, 0.0).astype(self.proj.T)

    def __call__(self, fh):
        return to_harm(self.proj, self.weights() * from_harm(self.proj, fh)).astype(fh.dtype)

    def pinv(self):
        return PixNoise(self.proj, self.V, -self.power, self.P)

    def sqrt(self):
        return PixNoise(self.proj, self.V, 0.5 * self.power, self.P)

    def logdet(self, proj):
        """power x Σ log|V| over the pixels of finite positive variance (`logdet(Diagonal(::Map))`, src/proj_lambert.jl:337-342)"""
        V = np.broadcast_to(self.V, (self.P,) + self.V.shape[1:])
        return self.power * float(np.sum(np.log(V[np.isfinite(V) & (V > 0)])))


class PixDataSet(DataSet):
    """oracle data set with Cn = PixNoise: the noise of a simulation is sqrt(V) ⊙ white in map space; the rest is the oracle's"""

    def simulate_data(self, phi_l, white_f, white_n):
        f = self.Cf.sqrt()(O.rfft2(white_f).astype(O.ctype(self.proj.T)))
        return self.mean(self.L(phi_l), f) + self.noise(white_n)

    def noise(self, white_n):
        return to_harm(self.proj, self.Cn.sqrt().weights() * np.asarray(white_n, self.proj.T)).astype(O.ctype(self.proj.T))


def const_op(P, levels, like):
    """the HarmOp of white noise at `levels[k]` in plane k (I | E,B | I,E,B): the Fourier diagonal of a map-space v·I is the constant v"""
    one = np.ones_like(like)
    if P == 3:
        return HarmOp(3, te=(levels[0] * one, 0 * one, 0 * one, levels[1] * one), bb=levels[2] * one)
    return HarmOp(P, diag=np.stack([levels[k] * one for k in range(P)]))


def hmean_levels(V, P):
    """1 / mean(1/V) per pol slice over the pixels of finite positive variance: the default Cn̂ of load_sim(noise_var_map=...)"""
    return [1.0 / np.mean(1.0 / v[np.isfinite(v) & (v > 0)]) for v in np.broadcast_to(V, (P,) + V.shape[1:])]


V0 = 7.5          # μK² per pixel: the level of the 3 μK-arcmin default at 3' pixels is 1 for I, 2 for Q, U


def var_map(nplanes, Nx, Ny, holes=True):
    """variance maps that ramp 30x across the patch, distinct per plane; `holes`: a few pixels of infinite variance (weight exactly 0), off the
    diagonal so that x and y cannot be exchanged unnoticed"""
    x, y = np.linspace(0, 1, Nx)[:, None], np.linspace(0, 1, Ny)[None, :]
    V = np.stack([V0 * (1 + 29 * (0.5 + 0.5 * np.sin(2 * np.pi * (x * (k + 1) + y)))) for k in range(nplanes)])
    if holes:
        for k in range(nplanes):
            V[k, (3 + 5 * k) % Nx, (Ny // 3 + k) % Ny] = np.inf
            V[k, Nx - 2, (7 * (k + 1)) % Ny] = np.inf
    return V


PM = dict(pad_deg=0.3, apod_deg=0.35)
# (Nside = (Ny, Nx), pol, planes of V, batch slots): power-of-two shapes with Ny != Nx and more than one column tile, two any-size shapes and the tall
# column (t, float32)
CASES = {"a": ((32, 32), "P", 2, 2), "b": ((32, 64), "IP", 3, 1), "c": ((64, 32), "I", 1, 2), "d": ((36, 60), "I", 1, 1), "e": ((40, 48), "P", 1, 2),
         "t": ((2048, 32), "P", 2, 1)}
_made = {}


def dataset(case, T=np.float64, V=None):
    """(PixDataSet with its data set, the oracle's sim dict with `V`, `levels`) of a case; the float32 run has the float64 run's fields, rounded.
    One ϕ for all slots.  Made once, never modified."""
    key = (case, np.dtype(T).name, None if V is None else id(V))
    if key in _made:
        return _made[key]
    Nside, pol, npl, B = CASES[case]
    so = dict(O.load_sim(3.0, Nside, pol, T, beam_fwhm=3.0, pixel_mask=PM, Nbatch=B))
    ds0, proj = so["ds"], so["proj"]
    P = ds0.P
    Vm = var_map(npl, Nside[1], Nside[0]) if V is None else V
    levels = hmean_levels(Vm, P)
    Ch = const_op(P, levels, ds0.Cphi)
    s2len = proj.T(np.deg2rad(5 / 60) ** 2)
    D = ((ds0.Cf + (Ch.scale(2) + s2len)) @ ds0.Cf.pinv()).sqrt()
    ds = PixDataSet(proj, P, ds0.Cf, PixNoise(proj, Vm, P=P), ds0.Cphi, ds0.Mf, ds0.B, Mpix=ds0.Mpix, Cnhat=Ch, D=D, G=ds0.G, Nphi=ds0.Nphi,
                    Cftilde=ds0.Cftilde)
    if np.dtype(T) == np.float64:
        so["phi"] = so["phi"][:1].copy()
        so["white_n"] = O.white_noise(3, (B, P, Nside[1], Nside[0]), np.float64)
        so["n"] = ds.noise(so["white_n"])
        ds.d = ds.mean(ds.L(so["phi"]), so["f"]) + so["n"]
    else:
        d64, s64 = dataset(case, np.float64, V)
        C = O.ctype(T)
        so["f"], so["phi"], so["n"], so["white_n"] = s64["f"].astype(C), s64["phi"].astype(C), s64["n"].astype(C), s64["white_n"]
        ds.d = d64.d.astype(C)
    so["V"], so["levels"], so["d"] = Vm, levels, ds.d
    _made[key] = (ds, so)
    return _made[key]


# conjugate-gradient iterations of the Wiener filter to tol = 1e-1 (float64, fstart = 0) per case: recorded from this file on the CPU
# (tests/test_pixnoise_ref.py recomputes them); the device must land within one of them in float64
CG_ITERS = {"a": 8, "b": 131, "c": 176, "d": 132, "e": 12}


def hist_array(h):
    return np.array([np.atleast_1d(r) for _, r in h])


_q = {}


def quantities(case, T=np.float64):
    """what the GPU tests compare for a case, made once per (case, precision): pinv(Cn) d, the three forms of ∇f, logpdf, ∇ϕ, the 8-step Wiener
    filter, and for the small cases logpdf_mixed with its gradient"""
    key = (case, np.dtype(T).name)
    if key in _q:
        return _q[key]
    ds, so = dataset(case, T)
    f, phi, d = so["f"], so["phi"], ds.d
    L = ds.L(phi)
    zero = np.zeros_like(d)
    out = {"noise_inv": ds.Cn.pinv()(d), "gradf": ds.gradientf_logpdf(f, L, d), "gradf_f0": ds.gradientf_logpdf(zero, L, d),
           "gradf_d0": ds.gradientf_logpdf(f, L, zero)}
    if case != "t":                                                              # t: one kernel path, pinv(Cn) and ∇f suffice
        out["logpdf"] = np.atleast_1d(ds.logpdf(f, phi, d))
        out["gradphi"] = ds.gradientphi_logpdf(f, phi, d)
        fw, h = ds.argmaxf_logpdf(phi, d=d, tol=0.0, nsteps=8)
        out["wf"], out["hist"] = fw, hist_array(h)
        fo, po = ds.mix(f[:1], phi)                                              # the mixed posterior on the first slot: one ϕ° per slot there
        out["mix_f"], out["mix_phi"] = fo, po
        lp, gfo, gpo = ds.grad_logpdf_mixed(fo, po, d[:1])
        out["logpdf_mixed"], out["gradfo"], out["gradpo"] = np.atleast_1d(lp), gfo, gpo
    _q[key] = out
    return out
