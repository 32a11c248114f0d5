"""`NoLensingDataSet` and `load_nolensing_sim` on the flat sky (src/dataset.jl:37-47, 68-73, 341-352): the data model without lensing,
d = M·B·f + n.  It is what Wiener-filters a masked map, draws constrained realisations (`drivers.sample_f`) and forms the filtered inputs of a
power-spectrum or quadratic estimate; `drivers.MAP_joint` of one is its Wiener filter (src/maximization.jl:235).  The `L` slot of the device data
set holds the identity (`IdentityLens`, `cmbl_lensop_identity`): on power-of-two maps the Wiener filter then runs without any flow.
"""
import ctypes

import numpy as np

from .engine import _DataSetOps, _ptr, IdentityLens, LenseFlow, Field, HARMONIC
from .lib import check
from .sim import load_sim, noise_from_white

_OPS = ("Cf_inv", "Cn_inv", "B", "Mf", "precond_inv", "Mpix", "Cn_inv_pix")


class NoLensingDataSet(_DataSetOps):
    """`NoLensingDataSet` at fiducial θ (src/dataset.jl:37-47) with the operators resident on the device.

    ops: dict name -> real planes (numpy/torch, reference layout):
        'Cf_inv','Cn_inv','B','Mf','precond_inv' : (P or 5, Nx, Nyh)   harmonic basis
        'Mpix' : (Nx, Ny) optional ;  'Cn_inv_pix' : (P or 1, Nx, Ny) optional, as in `BaseDataSet`
    There is nothing about ϕ.  d: harmonic-basis data (B,P,Nx,Nyh); logdet_sum: logdet Cf + logdet Cn.
    """
    _ids = {k: _DataSetOps._ids[k] for k in _OPS}

    def __init__(self, proj, P, ops, d=None, logdet_sum=0.0):
        self.proj, self.P = proj, int(P)
        extra = sorted(set(ops) - set(_OPS))
        if extra:
            raise ValueError(f"NoLensingDataSet takes the operators {', '.join(_OPS)}; got {', '.join(extra)}")
        self._open(proj.lib, "cmbl_dataset_create", proj._h, self.P)
        self.L = IdentityLens(proj)
        self._load(ops, d, logdet_sum)
        check(self.lib.cmbl_dataset_set_logdet(self._h, self.logdet_sum))

    def mean(self, f):
        """μ = M·B·f (src/dataset.jl:68-73)"""
        return self._mask(self._apply("B", f))

    def simulate_data(self, white_f, white_n):
        """`simulate(rng, ds).d`: f ~ 𝒩(0,Cf), n ~ 𝒩(0,Cn), d = M·B·f + n from unit white-noise maps (B,P,Nx,Ny); needs the host operators
        `ds.host` that `load_nolensing_sim` leaves.  Returns d (HARMONIC)."""
        return self.mean(self._draw_f(white_f)) + noise_from_white(self, white_n)

    def _draw_f(self, white_f):
        proj = self.proj
        return Field(proj, proj.diag_apply(self.host["Cf"].sqrt().p, proj.rfft(proj.tensor(white_f)), HARMONIC, HARMONIC), HARMONIC)

    def _logpdf(self, f, d, want_grad):
        f = f.to(HARMONIC)
        B = f.arr.shape[0]
        dd = None if d is None else d.to(HARMONIC).arr
        lp = (ctypes.c_double * B)()
        gf = self.proj.empty(HARMONIC, self.P, B) if want_grad else None
        check(self.lib.cmbl_nolensing_logpdf(self._h, _ptr(f.arr), _ptr(dd), lp, _ptr(gf), B))
        return np.array(lp[:]), (Field(self.proj, gf, HARMONIC) if want_grad else None)

    def logpdf(self, f, d=None):
        """logpdf(ds; f) (src/dataset.jl:68-73, src/distributions.jl:11-15) per batch slot; d = None: the data of the data set"""
        return self._logpdf(f, d, False)[0]

    def logpdf_and_gradient(self, f, d=None):
        """(logpdf(ds; f) per batch slot, gradientf_logpdf [HARMONIC]) from one pass (`cmbl_nolensing_logpdf`)"""
        return self._logpdf(f, d, True)

    def gradientf_logpdf(self, f, d=None, zero_d=False):
        """B'M'Cn⁻¹(d − M·B·f) − Cf⁻¹f (src/dataset.jl:76-80)"""
        return self._gradientf(self.L, f, d, zero_d)

    def argmaxf_logpdf(self, d=None, fstart=None, tol=1e-1, nsteps=500):
        """Wiener filter (src/maximization.jl:17-42 with L = I): returns (f [HARMONIC], history [(i, res_per_batch)])"""
        return self._wiener(self.L, d, fstart, tol, nsteps)


def load_nolensing_sim(theta_pix, Nside, pol, cls, lensed_covariance=False, lensed_data=False, **load_sim_kwargs):
    """`load_nolensing_sim` (src/dataset.jl:341-352): `load_sim` with `L = LenseFlow if lensed_data else IdentityLens`, then the `NoLensingDataSet` of
    its d, Cn, Cn̂, M, M̂, B, B̂ with Cf = Cf̃ when `lensed_covariance` (the preconditioner is recomputed for that Cf) and logdet_sum = logdet Cf +
    logdet Cn.  The quadratic estimate's Nϕ is of no use to this data set and is not computed: `load_sim` gets Nphi="flat" unless told otherwise.
    Returns dict(f, ftilde, phi, d, ds, proj) with Fields on the device; `ds.host` holds the host operators."""
    if "L" in load_sim_kwargs:
        raise TypeError("load_nolensing_sim chooses L itself: lensed_data=True lenses the simulated data with a LenseFlow")
    kw = dict(load_sim_kwargs)
    kw.setdefault("Nphi", "flat")
    nsteps = kw.get("nsteps", 7)
    sd = load_sim(theta_pix, Nside, pol, cls, L=(lambda p: LenseFlow(p, nsteps)) if lensed_data else IdentityLens, **kw)
    ds0, proj = sd["ds"], sd["proj"]
    h = ds0.host
    Cf, Cn, Mf, Bop = (h["Cftilde"] if lensed_covariance else h["Cf"]), h["Cn"], h["Mf"], h["B"]
    precond = Cf.pinv() + (Bop.T() @ Mf.T() @ Cn.pinv() @ Mf @ Bop)             # src/dataset.jl:129-132 for this Cf
    logdet_Cn = Cn.logdet(proj) if h["logdet_Cn"] is None else h["logdet_Cn"]
    ops = dict(Cf_inv=Cf.pinv().p, Cn_inv=Cn.pinv().p, B=Bop.p, Mf=Mf.p, precond_inv=precond.pinv().p, Mpix=h["Mpix"],
               Cn_inv_pix=ds0.ops.get("Cn_inv_pix"))
    ds = NoLensingDataSet(proj, ds0.P, ops, d=sd["d"], logdet_sum=Cf.logdet(proj) + logdet_Cn)
    ds.host = dict(Cf=Cf, Cn=Cn, Mf=Mf, B=Bop, Mpix=h["Mpix"], precond=precond, Cn_pix=h["Cn_pix"], logdet_Cn=h["logdet_Cn"])
    return dict(f=sd["f"], ftilde=sd["ftilde"], phi=sd["phi"], d=sd["d"], ds=ds, proj=proj)
