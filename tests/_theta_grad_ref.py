"""Float64 NumPy restatement of the θ-gradient of logpdf(ds; f, ϕ, θ) and of logpdf(Mixed(ds); f°, ϕ°, θ)  (TEST INFRASTRUCTURE).

The operators are the oracle's (oracle/theta.py, oracle/dataset.py: Cf(r, amplitudes), Cϕ(Aϕ), D(r), G(Aϕ), the 2 x 2 block sqrt / pinv / det
that read the ET plane for both off-diagonals, pinv = 1/x with non-finite results replaced by 0, logdet = Σ λ log|x| with non-finite terms
skipped).  Every helper here works on `Du`, a value with ONE tangent, so the derivative is the forward-mode derivative of exactly those
formulas: pinv keeps its discontinuity (tangent 0 where the value is replaced by 0), a skipped log term has tangent 0, sqrt(0) has tangent 0.

With lp(f, ϕ, θ) = logpdf(ds; f, ϕ, θ),  ϕ = G⁻¹ϕ°,  f̂ = L(ϕ)⁻¹ f°,  f = D⁻¹ f̂,  ĝ = ∂lp/∂f̂ = D' \\ ∂lp/∂f  and  gϕ° = ∂lp/∂ϕ°:
    d lpm/dr       = ∂lp/∂r|_(f,ϕ)      − ⟨ĝ, (∂D/∂r) f⟩          − Σ λ tr(D⁻¹ ∂D/∂r)
    d lpm/dAϕ      = ∂lp/∂Aϕ|_(f,ϕ)     − ⟨gϕ°, (∂lnG/∂Aϕ) ϕ°⟩    − Σ λ ∂lnG/∂Aϕ
    d lpm/dA_{k,b} = ∂lp/∂A_{k,b}|_(f,ϕ)
`theta_grad` returns per parameter the three parts (explicit, cross, logdet), their sum and S = |explicit| + |cross| + |logdet|: for r and Aϕ
the last two are 10³–10⁴ times the sum and nearly cancel, so every accuracy statement about the sum is relative to S.
tests/test_theta_grad_ref.py pins this file to Richardson central differences of the oracle's logpdf."""
import numpy as np

from oracle.dataset import harm_to_qu, qu_to_harm, to_harm, from_harm
from oracle.flatsky import nan2zero, irfft2
from oracle.theta import ThetaDataSet


class Du:
    """value and one tangent, elementwise"""
    __array_ufunc__ = None                     # ndarray (op) Du defers to Du's reflected operator

    def __init__(self, v, d=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.d = np.zeros_like(self.v) if d is None else np.asarray(d, dtype=np.float64) + np.zeros_like(self.v)

    @staticmethod
    def of(x):
        return x if isinstance(x, Du) else Du(x)

    def __add__(self, o):
        o = Du.of(o)
        return Du(self.v + o.v, self.d + o.d)

    __radd__ = __add__

    def __sub__(self, o):
        o = Du.of(o)
        return Du(self.v - o.v, self.d - o.d)

    def __neg__(self):
        return Du(-self.v, -self.d)

    def __mul__(self, o):
        o = Du.of(o)
        return Du(self.v * o.v, self.d * o.v + self.v * o.d)

    __rmul__ = __mul__


def d_pinv(x):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = 1 / x.v
        ok = np.isfinite(r)
        r = np.where(ok, r, 0.0)
        return Du(r, np.where(ok, -(x.d * r) * r, 0.0))


def d_sqrt(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.sqrt(x.v)
        return Du(v, np.where(v > 0, x.d / (2 * v), 0.0))


def d_logterm(x, lam):
    """one term of Σ λ log|x| per mode; skipped (value and tangent 0) where it is not finite"""
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.log(np.abs(x.v)) * lam
        ok = np.isfinite(v)
        return Du(np.where(ok, v, 0.0), np.where(ok, x.d / x.v * lam, 0.0))


# ---- operators as lists of planes: [d_0 .. d_{P-1}] (diagonal) or [a, b, c, d, e] (BlockDiagIEB) ----
def op_add(x, y):
    return [p + q for p, q in zip(x, y)]


def op_scale(x, s):
    return [p * s for p in x]


def op_add_scalar(x, s):
    """`+ UniformScaling`: TT, EE, BB of the block form, every plane of a diagonal operator"""
    if len(x) == 5:
        a, b, c, d, e = x
        return [a + s, b, c, d + s, e + s]
    return [p + s for p in x]


def op_det(x):
    a, _, c, d, _ = x
    return a * d - c * c


def op_pinv(x):
    if len(x) != 5:
        return [d_pinv(p) for p in x]
    a, _, c, d, e = x
    idet = d_pinv(op_det(x))
    o = -(c * idet)
    return [d * idet, o, o, a * idet, d_pinv(e)]


def op_sqrt(x):
    if len(x) != 5:
        return [d_sqrt(p) for p in x]
    a, _, c, d, e = x
    s = d_sqrt(op_det(x))
    t = d_pinv(d_sqrt(a + (d + 2 * s)))
    o = t * c
    return [t * (a + s), o, o, t * (d + s), d_sqrt(e)]


def op_mm(x, y):
    if len(x) != 5:
        return [p * q for p, q in zip(x, y)]
    a, b, c, d, e = x
    A, B, C, D, E = y
    return [a * A + b * C, a * B + b * D, c * A + d * C, c * B + d * D, e * E]


def op_logterms(x, lam):
    if len(x) != 5:
        out = d_logterm(x[0], lam)
        for p in x[1:]:
            out = out + d_logterm(p, lam)
        return out
    return d_logterm(op_det(x), lam) + d_logterm(x[4], lam)


def op_apply(x, f):
    """operator (planes of plain arrays) on a harmonic field (B, P, Nx, Nyh)"""
    if len(x) != 5:
        return np.stack(x)[None] * f
    a, b, c, d, e = x
    return np.stack([a * f[:, 0] + b * f[:, 1], c * f[:, 0] + d * f[:, 1], e * f[:, 2]], axis=1)


def op_quad(x, f):
    """Re(f† (operator f)) per mode and slot -> Du (B, Nx, Nyh)"""
    re = lambda u, w: np.real(np.conj(u) * w)
    if len(x) != 5:
        out = x[0] * re(f[:, 0], f[:, 0])
        for p in range(1, len(x)):
            out = out + x[p] * re(f[:, p], f[:, p])
        return out
    a, b, c, d, e = x
    return a * re(f[:, 0], f[:, 0]) + (b + c) * re(f[:, 0], f[:, 1]) + d * re(f[:, 1], f[:, 1]) + e * re(f[:, 2], f[:, 2])


def _const(op):
    return [Du(np.asarray(p, dtype=np.float64)) for p in op.arrays()]


class ThetaGradRef:
    """the forward-mode operators of one ThetaDataSet (oracle) and the gradient assembled from them"""

    def __init__(self, base, Cfs, Cten, r0=0.2, Aphi0=1.0, bands=None):
        self.th = ThetaDataSet(base, Cfs, Cten, r0=r0, Aphi0=Aphi0, bands=bands)
        self.proj = base.proj
        self.lam = np.asarray(base.proj.lam, dtype=np.float64)
        self.norm = float(base.proj.Ny * base.proj.Nx)

    # -- the four operators with the tangent of `key` ("r", "Aphi" or a band's name) --
    def Cf(self, r, amps, key):
        th = self.th
        planes = _const(th.Cfs0)
        for name, (pls, idx, nb) in th.bands.items():
            a = np.ones(nb) if amps.get(name) is None else np.asarray(amps[name], dtype=np.float64)
            amp = Du(np.append(a, 1.0)[idx], (idx < nb).astype(np.float64) if key == name else None)
            for k in pls:
                planes[k] = amp * planes[k]
        r_eff = th.r0 if r is None else r
        s = Du(np.float64(r_eff / th.r0), np.float64(1 / th.r0) if key == "r" else None)
        return op_add(planes, op_scale(_const(th.Cten), s))

    def D(self, r, key):
        th = self.th
        r_eff = th.r0 if r is None else r
        s = Du(np.float64(r_eff / th.r0), np.float64(1 / th.r0) if key == "r" else None)
        C = op_add(_const(th.Cfs0), op_scale(_const(th.Cten), s))
        N2 = op_add_scalar(op_scale(_const(th.base.Cnhat), 2.0), np.float64(th.s2len))
        return op_sqrt(op_mm(op_add(C, N2), op_pinv(C)))

    def Cphi(self, Aphi, key):
        th = self.th
        A = Du(np.float64(th.Aphi0 if Aphi is None else Aphi), np.float64(1.0) if key == "Aphi" else None)
        return Du(np.asarray(th.Cphi0, dtype=np.float64)) * A

    def G(self, Aphi, key):
        th = self.th
        two_n = 2 * np.asarray(th.base.Nphi, dtype=np.float64)
        g0 = d_sqrt(1 + two_n * d_pinv(Du(np.asarray(th.Cphi0 * th.Aphi0, dtype=np.float64))))
        return d_pinv(g0) * d_sqrt(1 + two_n * d_pinv(self.Cphi(Aphi, key)))

    def _sum(self, per_mode, key):
        """per-mode terms (B, Nx, Nyh) -> (B,) for r and Aϕ, (B, nbins) for a band (each mode lies in one bin; the slot `nbins` of the constant
        amplitude 1 belongs to no bin)"""
        if key in ("r", "Aphi"):
            return per_mode.sum(axis=(-1, -2))
        _, idx, nb = self.th.bands[key]
        return np.stack([np.bincount(idx.ravel(), weights=x.ravel(), minlength=nb + 1)[:nb] for x in per_mode])

    def explicit(self, f, phi, key, r=None, Aphi=None, amps=None):
        """∂ logpdf(ds; f, ϕ, θ) / ∂θ_key at fixed (f, ϕ): f harmonic (B, P, Nx, Nyh), ϕ Fourier (B, 1, Nx, Nyh)"""
        amps = amps or {}
        if key == "Aphi":
            cphi = self.Cphi(Aphi, key)
            q = d_pinv(cphi) * np.real(np.conj(phi[:, 0]) * phi[:, 0])
            lt = d_logterm(cphi, self.lam)
        else:
            cf = self.Cf(r, amps, key)
            q = op_quad(op_pinv(cf), f)
            lt = op_logterms(cf, self.lam)
        return self._sum(-0.5 * (q.d * self.lam / self.norm + lt.d), key)

    def chain(self, fo, po, r=None, Aphi=None, amps=None):
        """the steps of DataSet.grad_logpdf_mixed at θ with their intermediates: (lp, f, ϕ, ĝ, gϕ°, logdet(D,θ), logdet(G,θ))"""
        ds, ldD, ldG = self.th.at(r, Aphi, **(amps or {}))
        proj = self.proj
        with np.errstate(divide="ignore", invalid="ignore"):
            phi = nan2zero(po / ds.G)
        L = ds.L(phi)
        fhat = L.inv(fo)
        fh = ds.D.solve(to_harm(proj, fhat))
        ftil = L.apply(from_harm(proj, fh))
        z = ds.M(ds.B(to_harm(proj, ftil))) - ds.d
        Cninv_z = ds.Cn.pinv()(z)
        with np.errstate(divide="ignore", invalid="ignore"):
            Cpinv_p = nan2zero(phi / ds.Cphi)
        dtil = -ds.B.T_()(ds.Mt(Cninv_z))
        _, df1, dphi1 = L.grad_apply(ftil, harm_to_qu(proj, dtil), False)
        gf = qu_to_harm(proj, df1) - ds.Cf.pinv()(fh)
        ghat = ds.D.T_().solve(gf)
        _, df2, dphi2 = L.grad_inv(fhat, harm_to_qu(proj, ghat), False)
        with np.errstate(divide="ignore", invalid="ignore"):
            gphio = nan2zero((dphi1 + dphi2 - Cpinv_p) / ds.G)
        lp = ds.logpdf(fh, phi) - ldD - ldG
        return dict(lp=lp, f=fh, phi=phi, ghat=ghat, gphio=gphio, gfo=irfft2(df2, proj.Ny), ds=ds)

    @staticmethod
    def _pack(e, c, l):
        return dict(explicit=e, cross=c, logdet=l, total=e - c - l, S=np.abs(e) + np.abs(c) + np.abs(l))

    def unmixed(self, f, phi, r=None, Aphi=None, amps=None):
        """{name: parts} of ∇θ logpdf(ds; f, ϕ, θ) for every parameter named"""
        out = {}
        for key in [k for k, v in (("r", r), ("Aphi", Aphi)) if v is not None] + [k for k in (amps or {}) if amps[k] is not None]:
            e = self.explicit(f, phi, key, r, Aphi, amps)
            out[key] = self._pack(e, np.zeros_like(e), np.zeros_like(e))
        return out

    def mixed(self, fo, po, r=None, Aphi=None, amps=None):
        """(lp (B,), {name: parts}) of logpdf(Mixed(ds); f°, ϕ°, θ) and its θ-gradient for every parameter named"""
        ch = self.chain(fo, po, r, Aphi, amps)
        f, phi = ch["f"], ch["phi"]
        out = {}
        if r is not None:
            D = self.D(r, "r")
            D0 = self.D(self.th.r0, None)
            dDf = op_apply([p.d for p in D], f)
            cross = np.sum(np.real(np.conj(ch["ghat"]) * dDf) * self.lam, axis=(-1, -2, -3)) / self.norm
            logdet = op_logterms(op_mm(op_pinv(D0), D), self.lam).d.sum(axis=(-1, -2)) + np.zeros_like(cross)
            out["r"] = self._pack(self.explicit(f, phi, "r", r, Aphi, amps), cross, logdet)
        if Aphi is not None:
            G = self.G(Aphi, "Aphi")
            dlnG = G.d * d_pinv(Du(G.v)).v
            cross = np.sum(np.real(np.conj(ch["gphio"]) * (dlnG * po)) * self.lam, axis=(-1, -2, -3)) / self.norm
            logdet = d_logterm(G, self.lam).d.sum(axis=(-1, -2)) + np.zeros_like(cross)
            out["Aphi"] = self._pack(self.explicit(f, phi, "Aphi", r, Aphi, amps), cross, logdet)
        for key in [k for k in (amps or {}) if amps[k] is not None]:
            e = self.explicit(f, phi, key, r, Aphi, amps)
            out[key] = self._pack(e, np.zeros_like(e), np.zeros_like(e))
        return ch["lp"], out, ch
