"""The reference side of the data-set tests with another operator than LenseFlow in the `L` slot (`load_sim(L = BilinearLens)`,
src/dataset.jl:223, 306, 333): `oracle.dataset.DataSet` with `L(phi_l)` returning an adapter over tests/_bilinear_ref.BilinearLens or
tests/_powerlens_ref.PowerLens / Taylens, in the precision of the data set.  The adapter has the members the oracle's methods call --
`apply(map)`, `adj(QU-Fourier)`, `grad_apply(f~, Δ) -> (_, δf, δϕ)`, `inv(map)` -- and nothing else is restated: the data model, the Wiener
filter, MAP_marg are the oracle's own code.  tests/test_lensop_ds_ref.py pins this file by properties."""
import copy

import numpy as np

import oracle as O
import _bilinear_ref as BR
import _powerlens_ref as PR


class OpAdapter:
    """a lensing operator of tests/_bilinear_ref.py / tests/_powerlens_ref.py with the surface of oracle.lenseflow.LenseFlow"""

    def __init__(self, proj, kind, phi_l=None, defl=None, order=None):
        self.proj, self.kind, self.T = proj, kind, proj.T
        Ny, Nx, th = proj.Ny, proj.Nx, proj.theta_pix
        phi = None
        if defl is None:
            # d = Ł(∇ * ϕ) of the FOURIER field as it is (src/bilinearlens.jl:43, src/powerlens.jl:23): not through a map of ϕ, which would drop what
            # a real map cannot hold (the imaginary parts that iℓ of the Nyquist rows of a gradient leaves in MAP_marg's ϕ) before ∇ turns it real
            g = BR.Geom(Ny, Nx, th, proj.T)
            pl = np.asarray(phi_l)[0, 0].astype(BR.ctype(proj.T))
            if not np.any(pl):
                phi = np.zeros((Nx, Ny), dtype=proj.T)                           # norm(ϕ) == 0: the identity (src/bilinearlens.jl:34)
            else:
                gx, gy = g.grad(pl)
                unit = g.dx if kind == "BilinearLens" else proj.T(1)             # BilinearLens: pixels; PowerLens / Taylens: radians
                defl = ((O.irfft2(gy, Ny) / unit).astype(proj.T), (O.irfft2(gx, Ny) / unit).astype(proj.T))
        if kind == "BilinearLens":
            self.op = BR.BilinearLens(Ny, Nx, th, proj.T, phi=phi, defl=defl)
        else:
            self.op = PR.KINDS[kind](Ny, Nx, th, proj.T, order, phi=phi, defl=defl)

    def apply(self, m):
        return self.op.mul(m)

    def adj(self, gl):
        if self.kind == "Taylens":
            raise NotImplementedError("src/taylens.jl defines no adjoint")
        g = O.irfft2(gl, self.proj.Ny).astype(self.T)
        if self.kind == "BilinearLens":
            return O.rfft2(self.op.adj(g)).astype(BR.ctype(self.T))             # Lϕ' * Ł(g), back as a Fourier field
        return self.op.adj(g)                                                    # src/powerlens.jl:54: the Fourier field itself

    def grad_apply(self, ftilde, delta_l, alias_quirk=False):
        if self.kind != "BilinearLens":
            raise NotImplementedError("the reference has no pullback of PowerLens / Taylens with respect to ϕ")
        dphi, df = self.op.pullback(ftilde, O.irfft2(delta_l, self.proj.Ny).astype(self.T))    # src/bilinearlens.jl:165-171
        return None, O.rfft2(df).astype(BR.ctype(self.T)), dphi.astype(BR.ctype(self.T))

    def inv(self, m):
        if self.kind != "BilinearLens":
            raise NotImplementedError("the reference defines no inverse of PowerLens / Taylens")
        return self.op.ldiv(m)


class LensOpDataSet(O.DataSet):
    """an oracle data set whose lensing operator is `kind` (BilinearLens, PowerLens, Taylens).  `defl`: fixed (dy, dx) maps instead of ∇ϕ
    (BilinearLens: pixels; PowerLens / Taylens: radians), used whatever ϕ is passed"""

    @classmethod
    def of(cls, ds, kind, order=None, defl=None):
        new = copy.copy(ds)
        new.__class__ = cls
        new.kind, new.order, new.defl, new._L = kind, order, defl, None
        return new

    def L(self, phi_l):
        key = phi_l.tobytes()
        if self._L is None or self._L[0] != key:
            self._L = (key, OpAdapter(self.proj, self.kind, None if self.defl is not None else phi_l, self.defl, self.order))
        return self._L[1]


PM = dict(pad_deg=0.4, apod_deg=0.4)
# the cases of tests/test_gpu_lensop_dataset.py: (Nside, pol, pixel mask, batch slots of f and n)
CASES = {"A": ((64, 128), "P", True, 2), "B": ((36, 60), "I", True, 1), "C": ((32, 64), "IP", True, 1), "D": ((32, 64), "P", False, 1)}
RMS_PX = 0.7                                             # rms of each component of the deflection, pixels
_sims = {}


def sim(case, T=np.float64, theta=3.0, beam=3.0):
    """oracle.load_sim of a case in precision T, with one ϕ for all slots, scaled to RMS_PX: dict(ds, f, phi, d, n, proj, ...).  The fields
    of the float32 run are the float64 run's, rounded: identical inputs on both sides of a budget.  Made once, never modified."""
    key = (case, np.dtype(T).name)
    if key not in _sims:
        Nside, pol, mask, B = CASES[case]
        so = O.load_sim(theta, Nside, pol, T, beam_fwhm=beam, pixel_mask=PM if mask else None, Nbatch=B)
        if np.dtype(T) == np.float64:
            phi = so["phi"][:1].copy()
            g = BR.Geom(Nside[0], Nside[1], theta, np.float64)
            dy, dx = BR.deflection(g, O.irfft2(phi[0, 0], Nside[0]))
            phi *= RMS_PX / np.sqrt(0.5 * (np.mean(dy ** 2) + np.mean(dx ** 2)))
            so["phi"] = phi
        else:
            s64 = sim(case, np.float64, theta, beam)
            C = BR.ctype(T)
            so["f"], so["phi"], so["n"] = s64["f"].astype(C), s64["phi"].astype(C), s64["n"].astype(C)
        _sims[key] = so
    return _sims[key]


def dataset(case, kind="BilinearLens", T=np.float64, order=None, defl=None):
    """(LensOpDataSet with data d = M B L(ϕ) f + n set, the sim dict) of a case"""
    so = sim(case, T)
    ds = LensOpDataSet.of(so["ds"], kind, order=order, defl=defl)
    if np.dtype(T) == np.float64:
        ds.d = ds.mean(ds.L(so["phi"]), so["f"]) + so["n"]
    else:                                                                        # identical inputs: the float64 data, rounded
        ds.d = dataset(case, kind, np.float64, order, defl)[0].d.astype(BR.ctype(T))
    return ds, so


def big_deflection(Ny, Nx, rms_px=6.0, seed=5):
    """(dy, dx) pixel-unit maps (Nx, Ny) of `rms_px` rms: positions wrap more than once across both edges (case D)"""
    rng = np.random.default_rng(seed)
    return tuple(rms_px * rng.standard_normal((Nx, Ny)) for _ in range(2))


def quantities(ds, so, nsteps=8, with_phi=True, start=None):
    """what the parity tests compare for a case: ∇f at the true f, the `nsteps`-iteration Wiener filter (iterate, residual history), the solve
    restarted from that iterate, logpdf, and ∇ϕ at the iterate"""
    # (float32: `start` is the float64 run's iterate)
    f, phi, d = so["f"], so["phi"], ds.d
    L = ds.L(phi)
    out = {"gradf": ds.gradientf_logpdf(f, L, d)}
    fw, hist = ds.argmaxf_logpdf(phi, d=d, tol=0.0, nsteps=nsteps)
    out["wf"], out["hist"] = fw, np.array([np.atleast_1d(r) for _, r in hist])
    # the restart and ∇ϕ from `start` (default: this run's iterate): the float32 run is given the float64 run's iterate, identical inputs again
    fs = fw if start is None else start.astype(fw.dtype)
    fw2, hist2 = ds.argmaxf_logpdf(phi, d=d, fstart=fs, tol=0.0, nsteps=nsteps)
    out["wf2"], out["hist2"] = fw2, np.array([np.atleast_1d(r) for _, r in hist2])
    if with_phi:
        out["logpdf"] = np.atleast_1d(ds.logpdf(f, phi, d))
        out["gradphi"] = ds.gradientphi_logpdf(fs, phi, d)
    return out


# ---- everything the GPU parity tests compare, per precision: made once per (precision), shared by the tests and by the budget generator ----
NSIMS, MARG_KW = 4, dict(nsteps=2, nsteps_with_meanfield_update=1, alpha=0.2, cg_tol=0.0, cg_nsteps=8)
_all = {}


def whites(P, Nx, Ny):
    """the injected unit white maps of the MAP_marg comparison: (white_f, white_n), each (NSIMS, P, Nx, Ny) float64"""
    return tuple(O.white_noise(s, (NSIMS, P, Nx, Ny), np.float64) for s in (50, 51))


def reference(T=np.float64):
    """dict name -> dict quantity -> array, in precision T: cases A, B, C (BilinearLens), D (BilinearLens of a fixed 6 px deflection, ∇f and
    the fixed-length solve only), "A/PowerLens4", and for A also the converged solve, logpdf_mixed and two MAP_marg steps"""
    key = np.dtype(T).name
    if key in _all:
        return _all[key]
    out = {}
    r64 = None if key == "float64" else reference(np.float64)
    st = lambda name: None if r64 is None else r64[name]["wf"]
    for case in ("A", "B", "C"):
        ds, so = dataset(case, T=T)
        out[case] = quantities(ds, so, start=st(case))
    # A: converged solve, logpdf_mixed (unmix by the reference gmres), MAP_marg on the first data slot
    ds, so = dataset("A", T=T)
    fw, hist = ds.argmaxf_logpdf(so["phi"], d=ds.d, tol=1e-1, nsteps=500)
    out["A"]["wf_conv"], out["A"]["n_conv"] = fw, len(hist)
    fo, po = ds.mix(so["f"], so["phi"])
    out["A"]["mix_f"], out["A"]["mix_phi"] = fo, po
    out["A"]["logpdf_mixed"] = np.atleast_1d(ds.logpdf_mixed(fo, po, ds.d))
    ds1 = LensOpDataSet.of(ds, "BilinearLens")
    ds1.d = ds.d[:1]
    (Ny, Nx), P = CASES["A"][0], ds.P
    wf, wn = whites(P, Nx, Ny)
    for spb in (1, 4):
        phi, tr = O.map_marg(ds1, wf.astype(T), wn.astype(T), sims_per_batch=spb, **MARG_KW)
        out[f"A/MAP_marg{spb}"] = {"phi1": tr[0]["phi"], "phi2": phi, "g_norm": np.array([t["g_norm"] for t in tr])}
    # D: a fixed deflection of 6 px rms
    Ny, Nx = CASES["D"][0]
    ds, so = dataset("D", T=T, defl=big_deflection(Ny, Nx))
    out["D"] = quantities(ds, so, with_phi=False, start=st("D"))
    ds, so = dataset("A", "PowerLens", T=T, order=4)
    out["A/PowerLens4"] = quantities(ds, so, with_phi=False, start=st("A/PowerLens4"))
    out["A/PowerLens4"]["d"] = ds.d
    for case in ("A", "B", "C", "D"):
        out[case]["d"] = dataset(case, T=T, defl=big_deflection(*CASES["D"][0]) if case == "D" else None)[0].d
    _all[key] = out
    return out


SCALARS = ("hist", "hist2", "logpdf", "logpdf_mixed", "g_norm")        # compared by their largest relative error; every other quantity by relative L2
NOT_COMPARED = ("d", "n_conv", "mix_f", "mix_phi")


def distance(q, a, b):
    a, b = np.asarray(a), np.asarray(b)
    if q in SCALARS:
        return float(np.max(np.abs(a.astype(np.float64) - b) / np.abs(b)))
    return float(np.linalg.norm((a.astype(b.dtype) - b).ravel()) / np.linalg.norm(b.ravel()))
