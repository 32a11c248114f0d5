"""The reference side of the tests of the flat-sky no-lensing data set, d = M B f + n (NoLensingDataSet, src/dataset.jl:37-47, 68-73; its Wiener
filter src/maximization.jl:17-42, 235; load_nolensing_sim src/dataset.jl:341-352): the oracle's `DataSet` with `L()` overridden to an identity
object and `logpdf` without the ϕ term.  Nothing else is restated: the solves are `oracle.DataSet.argmaxf_logpdf` over
`oracle.cg.conjugate_gradient`, the data are d = M B f + n from `oracle.load_sim`'s f and n.  Settings: θpix = 3', no beam, the border mask of
tests/_cg_rules_ref.py, Nbatch = 2 (17 for the case that takes the B > 16 branch of the fused iteration).  The float32 run takes the float64 run's
d, rounded.  tests/test_nolensing_ref.py pins the fixtures on the CPU, tests/test_gpu_nolensing.py runs the device against them,
tools/make_nolensing_budget.py records the float32 budget."""
import copy

import numpy as np

import oracle as O
from _cg_rules_ref import slot_rel, distance, CLASS, THETA, BEAM, PM                              # noqa: F401  (one rule for every budget of the CG)

POLS = ("I", "P", "IP")
POW2 = [(32, 32), (32, 64), (64, 32)]               # (Ny, Nx): the smallest the fused kernels take, non-square both ways; Nyh = 17 / 33 leave a tail row group
ANYSIZE = (24, 40)                                  # composed form only
NSHORT = 8                                          # steps of the tol = 0 solves every pol is compared over
TOL = 0.1
# pol = "P", tol = 0.1, nsteps = 500 in float64: (Ny, Nx), B -> (history length, last residual, the one before it; the largest over the slots)
STOPS = {((32, 32), 2): (16, 0.0896, 0.117), ((32, 32), 17): (17, 0.0968, 0.126), ((32, 64), 2): (21, 0.0918, 0.112),
         ((64, 32), 2): (20, 0.0855, 0.114), ((24, 40), 2): (16, 0.0827, 0.131)}


class _Identity:
    """L = I: what `DataSet` asks of its lensing operator"""

    def apply(self, m):
        return m

    def adj(self, F):
        return F

    def inv(self, m):
        return m


IDENTITY = _Identity()


class NoLensing(O.DataSet):
    """the oracle's data set with the identity for L(ϕ), whatever ϕ, and the posterior of f alone"""

    @classmethod
    def of(cls, ds):
        new = copy.copy(ds)
        new.__class__ = cls
        return new

    def L(self, phi_l=None):
        return IDENTITY

    def logpdf(self, fh, d=None):
        """−½ [f'Cf⁻¹f + logdet Cf + (MBf − d)'Cn⁻¹(MBf − d) + logdet Cn]   (src/dataset.jl:68-73, src/distributions.jl:11-15)"""
        d = self.d if d is None else d
        z = self.mean(IDENTITY, fh) - d
        return -(self.dot(fh, self.Cf.solve(fh)) + self.Cf.logdet(self.proj)) / 2 - (self.dot(z, self.Cn.pinv()(z)) + self.Cn.logdet(self.proj)) / 2

    def sample_f(self, white_f, white_n, d=None, tol=TOL, nsteps=500):
        """sample_f (src/maximization.jl:56-62) from injected white draws: (f, history)"""
        d = self.d if d is None else d
        ct = O.flatsky.ctype(self.proj.T)
        fs = self.Cf.sqrt()(O.flatsky.rfft2(white_f).astype(ct))
        ns = self.Cn.sqrt()(O.flatsky.rfft2(white_n).astype(ct))
        df, hist = self.argmaxf_logpdf(None, d=d - (self.mean(IDENTITY, fs) + ns), tol=tol, nsteps=nsteps)
        return fs + df, hist


_KIND = {"x": "x", "hist": "hist", "grad": "x", "mean": "x", "logpdf": "hist"}       # fields take the class bound of an iterate, scalars that of a residual


def bound(budget, prec, case, run, q):
    """tests/_cg_rules_ref.bound for this budget's quantities: double precision the class bound, single max(class bound, 3 x the float32 oracle's own
    distance from the float64 oracle)"""
    c = CLASS[prec][_KIND[q]]
    return c if prec == "f64" else max(c, 3 * budget["cases"][case][run][q])


def case_key(pol, shape, B=2, mask=True):
    return f"{pol}_{shape[0]}x{shape[1]}_B{B}" + ("" if mask else "_nomask")


_sims, _solves = {}, {}


def sim(pol, shape, T=np.float64, B=2, mask=True):
    """dict(ds, d, f, n, so) of a case in precision T: `so` is oracle.load_sim's result (so["ds"] the lensing data set on the same operators), ds
    its no-lensing twin with d = M B f + n.  Made once, never modified."""
    key = (pol, tuple(shape), np.dtype(T).name, B, mask)
    if key not in _sims:
        so = O.load_sim(THETA, tuple(shape), pol, T, beam_fwhm=BEAM, pixel_mask=PM if mask else None, Nbatch=B)
        ds = NoLensing.of(so["ds"])
        if np.dtype(T) == np.float64:
            d = ds.M(ds.B(so["f"])) + so["n"]
        else:
            d = sim(pol, shape, np.float64, B, mask)["d"].astype(np.complex64)
        ds.d = d
        d.flags.writeable = False
        _sims[key] = dict(ds=ds, d=d, f=so["f"], n=so["n"], so=so)
    return _sims[key]


def solve(pol, shape, T=np.float64, B=2, mask=True, nsteps=NSHORT, tol=0.0):
    """(best iterate (B, P, Nx, Nyh), residual history (length, B)) of the oracle's Wiener filter.  Made once per argument set, read-only."""
    key = (pol, tuple(shape), np.dtype(T).name, B, mask, nsteps, tol)
    if key not in _solves:
        s = sim(pol, shape, T, B, mask)
        x, hist = s["ds"].argmaxf_logpdf(None, d=s["d"], tol=tol, nsteps=nsteps)
        x, h = np.array(x), np.array([np.atleast_1d(r) for _, r in hist])
        x.flags.writeable = h.flags.writeable = False
        _solves[key] = (x, h)
    return _solves[key]


def closed_form(ds, d):
    """without a pixel mask every factor is diagonal (or the IEB block) in the harmonic basis: f = (Cf⁻¹ + B'Mf'Cn⁻¹MfB)⁻¹ B'Mf'Cn⁻¹ d, mode by mode"""
    assert ds.Mpix is None
    A = ds.Cf.pinv() + (ds.B.T_() @ ds.Mf.T_() @ ds.Cn.pinv() @ ds.Mf @ ds.B)
    return A.pinv()(ds.B.T_()(ds.Mf.T_()(ds.Cn.pinv()(d))))


def whites(pol, shape, B=2, seeds=(11, 12)):
    """the injected unit white-noise maps (B, P, Nx, Ny) of the sample_f comparison, float64"""
    P = {"I": 1, "P": 2, "IP": 3}[pol]
    shp = (B, P, shape[1], shape[0])
    return tuple(np.random.Generator(np.random.PCG64(s)).standard_normal(shp) for s in seeds)


def with_imag_selfconj(fh, eps=0.3):
    """a copy of the spectrum fh (B, P, Nx, Nyh) with imaginary parts put into its four self-conjugate modes (kx, ky in {0, Nyquist}): no real map
    has such a spectrum, and c2r drops them"""
    g = np.array(fh)
    Nx, Nyh = g.shape[-2], g.shape[-1]
    scale = np.sqrt(np.mean(np.abs(g) ** 2))
    for x in (0, Nx // 2):
        for y in (0, Nyh - 1):
            g[..., x, y] += 1j * eps * scale
    return g
