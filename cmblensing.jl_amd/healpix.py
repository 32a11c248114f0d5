"""HEALPix fields and the projection between the sphere and a flat patch (src/proj_healpix.jl) on top of the C ABI: `ProjHealpix`,
`HealpixField` / `HealpixMap`, `Projector`, `project` and its transpose `project_adjoint`.

A HEALPix field is a tensor (B, P, npix) == Julia (npix, npol) plus the batch axis, RING ordering, P = 1 (I), 2 (QU) or 3 (IQU).  Pixel
indices are 0-based here (the reference's k - 1).  `project` covers both directions of `method="bilinear"` and of `method="nfft"` for
`ProjLambert` (with its `rotator`) and `ProjEquiRect`; the geometry is computed on the device in double whatever the precision of the
projection.

`method="nfft"` is the reference's `method = :fft` (a non-uniform FFT, src/proj_healpix.jl:229-236, 314-325): trigonometric interpolation
of the band-limited patch at the HEALPix centres one way and its transpose the other way (DESIGN.md 4.8 has the definition).  The spelling
`"fft"` itself still raises NotImplementedError, with its message unchanged: existing tests pin that, and making it an alias of "nfft" is
left to a change that may touch them.

The pullbacks: `project_adjoint` (and `Projector.to_cart_adjoint` / `to_healpix_adjoint`) is the exact transpose of `project`, on the device,
for both methods; `project` on a field whose tensor has `requires_grad` goes through a `torch.autograd.Function` whose backward it is
(the reference's `@adjoint` of :145-150).

NOT here (README "HEALPix projection", out of scope): NEST ordering, lensing of HEALPix fields."""
import ctypes

import numpy as np
import torch

from .lib import load_library, check
from .engine import ProjLambert, Field, MAP, _ptr, _Handle
from .equirect import ProjEquiRect, EquiRectField

_PD = ctypes.POINTER(ctypes.c_double)
_BASES = {"I": 1, "QU": 2, "IQU": 3}
(_COUNTS, _THETA, _PHI, _PSI_CART, _IDX_IN_PATCH, _IDX_TOUCHED, _I, _J, _PSI_HPX) = range(9)
MAX_NSIDE = 8192


def _check_nside(Nside):
    n = int(Nside)
    if n != Nside or n < 1 or n > MAX_NSIDE or n & (n - 1):
        raise ValueError(f"Nside must be a power of two in 1 ... {MAX_NSIDE}, got {Nside!r}")
    return n


def npix2nside(npix):
    """Nside of a map of `npix` pixels; ValueError unless npix = 12 Nside^2 with Nside a power of two"""
    n = int(round(np.sqrt(int(npix) / 12.0)))
    if n < 1 or 12 * n * n != int(npix):
        raise ValueError(f"{npix} is not a HEALPix map length (12 Nside^2)")
    return _check_nside(n)


def pix2ang_ring(Nside, pix=None):
    """pix2angRing (Healpix.jl) of the 0-based RING pixels `pix` (default: all): (θ, ϕ), host, float64 (`cmbl_healpix_pix2ang_host`)"""
    lib = load_library()
    Nside = _check_nside(Nside)
    if pix is None:
        th, ph = np.empty(12 * Nside * Nside), np.empty(12 * Nside * Nside)
        check(lib.cmbl_healpix_pix2ang_host(Nside, 0, th.size, th.ctypes.data_as(_PD), ph.ctypes.data_as(_PD)))
        return th, ph
    pix = np.atleast_1d(np.asarray(pix, dtype=np.int64))
    th, ph = np.empty(pix.size), np.empty(pix.size)
    one_t, one_p = ctypes.c_double(), ctypes.c_double()
    for k, p in enumerate(pix.ravel()):
        check(lib.cmbl_healpix_pix2ang_host(Nside, int(p), 1, ctypes.byref(one_t), ctypes.byref(one_p)))
        th[k], ph[k] = one_t.value, one_p.value
    return th.reshape(pix.shape), ph.reshape(pix.shape)


class ProjHealpix:
    """`ProjHealpix(Nside)` (src/proj_healpix.jl:6-8)"""

    def __init__(self, Nside):
        self.Nside = _check_nside(Nside)
        self.npix = 12 * self.Nside * self.Nside

    def __eq__(self, o):
        return isinstance(o, ProjHealpix) and o.Nside == self.Nside

    def __hash__(self):
        return hash(("ProjHealpix", self.Nside))

    def __repr__(self):
        return f"ProjHealpix({self.Nside})"


class HealpixField:
    """A field on the sphere: `arr` (npix,), (P, npix) or (B, P, npix), NumPy or torch, host or device; `basis` "I", "QU" or "IQU"
    (the reference's HealpixMap / HealpixQUMap / HealpixIQUMap, :13-25)."""

    def __init__(self, proj, arr, basis="I"):
        if basis not in _BASES:
            raise ValueError(f"HealpixField: the basis is one of {sorted(_BASES)}, got {basis!r}")
        t = arr if torch.is_tensor(arr) else torch.from_numpy(np.ascontiguousarray(arr))
        while t.dim() < 3:
            t = t[None]
        if t.dim() != 3 or t.shape[2] != proj.npix or t.shape[1] != _BASES[basis] or not t.dtype.is_floating_point:
            raise ValueError(f"HealpixField: a real array (B, {_BASES[basis]}, {proj.npix}) is needed for basis {basis} at Nside {proj.Nside}, "
                             f"got {tuple(t.shape)} / {t.dtype}")
        self.proj, self.arr, self.basis = proj, t.contiguous(), basis
        self.npol, self.B = int(t.shape[1]), int(t.shape[0])

    Nside = property(lambda s: s.proj.Nside)

    def dot(self, other):
        """dot(a, b) = sum(a.arr .* b.arr) (:49); fields of two Nsides do not combine (:41-47)"""
        if other.proj != self.proj:
            raise ValueError(f"Can't combine Healpix maps with two different Nsides ({self.Nside}, {other.Nside}).")
        if other.basis != self.basis:
            raise ValueError("dot: the two fields differ in basis")
        return float(torch.dot(self.arr.reshape(-1).double(), other.arr.to(self.arr.device).reshape(-1).double()))

    def _sub(self, lo, hi, basis):
        return HealpixField(self.proj, self.arr[:, lo:hi], basis)

    # f.I, f.Q, f.U, f.P: views, no copy
    @property
    def I(self):                                                             # noqa: E743
        if self.basis == "QU":
            raise AttributeError("a QU field has no I")
        return self._sub(0, 1, "I")

    @property
    def Q(self):
        if self.basis == "I":
            raise AttributeError("an I field has no Q")
        return self._sub(self.npol - 2, self.npol - 1, "I")

    @property
    def U(self):
        if self.basis == "I":
            raise AttributeError("an I field has no U")
        return self._sub(self.npol - 1, self.npol, "I")

    @property
    def P(self):
        if self.basis == "I":
            raise AttributeError("an I field has no P")
        return self._sub(self.npol - 2, self.npol, "QU")

    def __getitem__(self, k):
        return {"I": lambda: self.I, "Q": lambda: self.Q, "U": lambda: self.U, "P": lambda: self.P}[k]()


def HealpixMap(arr):
    """`HealpixMap(I)` (:15-17): a spin-0 field, Nside from the length (ValueError on a bad one)"""
    n = (arr.shape if hasattr(arr, "shape") else np.asarray(arr).shape)[-1]
    return HealpixField(ProjHealpix(npix2nside(n)), arr, "I")


_METHODS = {"bilinear": 0, "nfft": 1}          # CMBL_PROJECT_BILINEAR, CMBL_PROJECT_NFFT


def _method(method):
    """the method's number in the C ABI; "fft" (the reference's name of "nfft") is refused as before, see the module docstring"""
    if method == "fft":
        raise NotImplementedError('project(method="fft") needs a non-uniform FFT (src/proj_healpix.jl:229-236, 314-325) and is out of scope, like NEST '
                                  'ordering, the AD rules and lensing of HEALPix fields (README, "HEALPix projection": out)')
    if method not in _METHODS:
        raise ValueError(f'method must be "bilinear" or "nfft" (or "fft", not implemented under that name), got {method!r}')
    return _METHODS[method]


class Projector(_Handle):
    """`Projector(hpx_proj => cart_proj; method)` (:254-306): what both directions of `project` precompute, on the device.  Either order of
    the two projections.  `method`: "bilinear" or "nfft" (the reference's :fft; even Ny, Nx up to 2048 and a patch that holds at least one
    HEALPix centre); `window_width` is the number of fine-grid cells per axis a node touches (0 for "bilinear").  Host readbacks (float64 /
    int64 NumPy, cached): `thetas`, `phis`, `psi_cart` (Ny Nx, Ny fastest: the reference's θs, ϕs, ψpol_θϕs), `hpx_idxs_in_patch`, and for the touched pixels (0 < i < Ny+1, 0 < j < Nx+1) `touched`, `is_`, `js`, `psi_hpx`."""
    _destroy = "cmbl_projector_destroy"

    def __init__(self, hpx_proj, cart_proj, method="bilinear"):
        if isinstance(cart_proj, ProjHealpix):
            hpx_proj, cart_proj = cart_proj, hpx_proj
        code = _method(method)
        if not isinstance(hpx_proj, ProjHealpix) or not isinstance(cart_proj, (ProjLambert, ProjEquiRect)):
            raise TypeError("Projector: a ProjHealpix and a ProjLambert or ProjEquiRect are needed")
        self.hpx_proj, self.cart_proj, self.method = hpx_proj, cart_proj, method
        if isinstance(cart_proj, ProjEquiRect):
            kind, params = 1, list(cart_proj.theta_span) + list(cart_proj.phi_span)
        else:
            kind, params = 0, list(cart_proj.rotator)
        self._open(cart_proj.lib, "cmbl_projector_create_method", cart_proj._h, hpx_proj.Nside, kind, (ctypes.c_double * len(params))(*params), code)
        self._info = {}

    @property
    def window_width(self):
        m, w = ctypes.c_int(), ctypes.c_int()
        check(self.lib.cmbl_projector_method(self._h, ctypes.byref(m), ctypes.byref(w)))
        return w.value

    def _get(self, which, n):
        if which not in self._info:
            out = np.empty(int(n), dtype=np.float64)
            check(self.lib.cmbl_projector_info_host(self._h, which, out.ctypes.data_as(_PD), out.size))
            self._info[which] = out
        return self._info[which]

    n_in_patch = property(lambda s: int(s._get(_COUNTS, 2)[0]))
    n_touched = property(lambda s: int(s._get(_COUNTS, 2)[1]))
    _ncart = property(lambda s: s.cart_proj.Ny * s.cart_proj.Nx)
    thetas = property(lambda s: s._get(_THETA, s._ncart))
    phis = property(lambda s: s._get(_PHI, s._ncart))
    psi_cart = property(lambda s: s._get(_PSI_CART, s._ncart))
    hpx_idxs_in_patch = property(lambda s: s._get(_IDX_IN_PATCH, s.n_in_patch).astype(np.int64))
    touched = property(lambda s: s._get(_IDX_TOUCHED, s.n_touched).astype(np.int64))
    is_ = property(lambda s: s._get(_I, s.n_touched))
    js = property(lambda s: s._get(_J, s.n_touched))
    psi_hpx = property(lambda s: s._get(_PSI_HPX, s.n_touched))

    def _to_cart_raw(self, src, npol, B):
        p = self.cart_proj
        out = torch.empty((B, npol, p.Nx, p.Ny), dtype=p.T, device=p.device)
        check(self.lib.cmbl_project_to_cart(self._h, _ptr(src), _ptr(out), npol, B))
        return out

    def _to_healpix_raw(self, arr, basis, P, B):
        p = self.cart_proj
        out = torch.empty((B, P, self.hpx_proj.npix), dtype=p.T, device=p.device)
        check(self.lib.cmbl_project_to_healpix(self._h, basis, _ptr(arr), _ptr(out), P, B))
        return out

    def _to_cart_adjoint_raw(self, g, npol, B):
        p = self.cart_proj
        out = torch.empty((B, npol, self.hpx_proj.npix), dtype=p.T, device=p.device)
        check(self.lib.cmbl_project_to_cart_adjoint(self._h, _ptr(g), _ptr(out), npol, B))
        return out

    def _to_healpix_adjoint_raw(self, g, npol, B):
        p = self.cart_proj
        out = torch.empty((B, npol, p.Nx, p.Ny), dtype=p.T, device=p.device)
        check(self.lib.cmbl_project_to_healpix_adjoint(self._h, _ptr(g), _ptr(out), npol, B))
        return out

    def _cart_field(self, out):
        # (EquiRectField is spin 0 or spin 2; an IQU result on a ProjEquiRect is a plain MAP Field, the reference's BaseField{IQUMap}, :251)
        p = self.cart_proj
        return EquiRectField(p, out, MAP) if isinstance(p, ProjEquiRect) and out.shape[1] < 3 else Field(p, out, MAP)

    def _dev(self, t):
        """a tensor that autograd follows -> contiguous, on the device, of the projection's precision (differentiable, unlike `tensor`)"""
        p = self.cart_proj
        return t.to(device=p.device, dtype=p.T).contiguous()

    def to_cart(self, f):
        """project(projector, healpix_field => cart_proj) (:221-252).  A field whose tensor has `requires_grad` is followed by autograd;
        the pullback is `to_cart_adjoint`."""
        p = self.cart_proj
        if f.proj != self.hpx_proj:
            raise ValueError(f"Projector built for Nside {self.hpx_proj.Nside}, field has {f.proj.Nside}")
        if f.arr.requires_grad:
            return self._cart_field(_ToCart.apply(self._dev(f.arr), self))
        return self._cart_field(self._to_cart_raw(p.tensor(f.arr), f.npol, f.B))

    def to_healpix(self, f):
        """project(projector, cart_field => hpx_proj) (:308-341): `f` a Field of the ProjLambert (any basis) or an EquiRectField.  A MAP
        field whose tensor has `requires_grad` is followed by autograd; the pullback is `to_healpix_adjoint`."""
        p = self.cart_proj
        if f.proj is not p and f.proj != p:
            raise ValueError("Projector built for another Cartesian projection than the field's")
        if torch.is_tensor(f.arr) and f.arr.requires_grad:
            if f.basis != MAP:
                raise ValueError("Projector.to_healpix: under autograd the field must be in the MAP basis")
            out = _ToHealpix.apply(self._dev(f.arr), self)
            return HealpixField(self.hpx_proj, out, {1: "I", 2: "QU", 3: "IQU"}[int(out.shape[1])])
        if isinstance(f, EquiRectField):
            f = f.to(MAP)
        arr, basis = f.arr, f.basis
        B, P = int(arr.shape[0]), int(arr.shape[1])
        return HealpixField(self.hpx_proj, self._to_healpix_raw(arr, basis, P, B), {1: "I", 2: "QU", 3: "IQU"}[P])

    def to_cart_adjoint(self, g):
        """The transpose (pullback) of `to_cart`: `g` a MAP Field / EquiRectField on the Cartesian projection -> HealpixField.  Bilinear:
        hbar[p] = sum over the (Cartesian pixel, corner) pairs that read p of weight * (the rotation's transpose applied to g there), exactly
        0 where nothing reads; nfft: 1/Npatch sum_g K(x_g - x_p) (R^T g)_g on hpx_idxs_in_patch, exactly 0 elsewhere (include/cmblens.h)."""
        p = self.cart_proj
        if g.proj is not p and g.proj != p:
            raise ValueError("Projector built for another Cartesian projection than the cotangent's")
        if isinstance(g, EquiRectField):
            g = g.to(MAP)
        if g.basis != MAP:
            raise ValueError("Projector.to_cart_adjoint: the cotangent must be in the MAP basis")
        arr = p.tensor(g.arr.detach())
        if arr.dim() != 4 or tuple(arr.shape[2:]) != (p.Nx, p.Ny) or not 1 <= arr.shape[1] <= 3:
            raise ValueError(f"Projector.to_cart_adjoint: a MAP array (B, 1 ... 3, {p.Nx}, {p.Ny}) is needed, got {tuple(arr.shape)}")
        B, P = int(arr.shape[0]), int(arr.shape[1])
        return HealpixField(self.hpx_proj, self._to_cart_adjoint_raw(arr, P, B), {1: "I", 2: "QU", 3: "IQU"}[P])

    def to_healpix_adjoint(self, g):
        """The transpose (pullback) of `to_healpix` on MAP input: `g` a HealpixField -> MAP Field (an EquiRectField on a ProjEquiRect with
        npol < 3, the rule of `to_cart`).  Values of `g` at pixels the projection does not touch are ignored."""
        p = self.cart_proj
        if not isinstance(g, HealpixField) or g.proj != self.hpx_proj:
            raise ValueError(f"Projector built for Nside {self.hpx_proj.Nside}, the cotangent has {getattr(getattr(g, 'proj', None), 'Nside', None)}")
        return self._cart_field(self._to_healpix_adjoint_raw(p.tensor(g.arr.detach()), g.npol, g.B))


class _ToCart(torch.autograd.Function):
    """`Projector.to_cart` for autograd: (B, P, npix) device tensor -> (B, P, Nx, Ny); backward is `cmbl_project_to_cart_adjoint`"""

    @staticmethod
    def forward(ctx, src, projector):
        ctx.projector = projector
        return projector._to_cart_raw(src, int(src.shape[1]), int(src.shape[0]))

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        return ctx.projector._to_cart_adjoint_raw(g, int(g.shape[1]), int(g.shape[0])), None


class _ToHealpix(torch.autograd.Function):
    """`Projector.to_healpix` for autograd, MAP input: (B, P, Nx, Ny) -> (B, P, npix); backward is `cmbl_project_to_healpix_adjoint`"""

    @staticmethod
    def forward(ctx, arr, projector):
        ctx.projector = projector
        return projector._to_healpix_raw(arr, MAP, int(arr.shape[1]), int(arr.shape[0]))

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        return ctx.projector._to_healpix_adjoint_raw(g, int(g.shape[1]), int(g.shape[0])), None


def _pair(field, other_proj, method, projector):
    """the checks `project` and `project_adjoint` share: (projector, is the field on the sphere)"""
    _method(method)
    on_sphere = isinstance(field, HealpixField)
    if on_sphere == isinstance(other_proj, ProjHealpix):
        raise TypeError("project: HealpixField => ProjLambert | ProjEquiRect, or Field | EquiRectField => ProjHealpix")
    hpx, cart = (field.proj, other_proj) if on_sphere else (other_proj, field.proj)
    if projector is None:
        projector = Projector(hpx, cart, method)
    elif projector.hpx_proj != hpx or (projector.cart_proj is not cart and projector.cart_proj != cart):
        raise ValueError("project: the projector was built for another pair of projections")           # the @assert of :222, 309
    elif projector.method != method:
        raise ValueError(f"project: the projector was built for method {projector.method!r}, not {method!r}")   # Projector{method} (:221, 229)
    return projector, on_sphere


def project(field, target_proj, method="bilinear", projector=None):
    """`project(healpix_field => cart_proj)` and `project(cart_field => ProjHealpix(Nside))` (src/proj_healpix.jl:164-219, 300-302): a
    HealpixField lands on `target_proj` (ProjLambert or ProjEquiRect) as a MAP Field / EquiRectField; a Field or EquiRectField lands on the
    sphere as a HealpixField, exactly 0 outside the patch.  QU and IQU fields have their polarisation rotated into the local basis.
    `method`: "bilinear" or "nfft" (module docstring).  `projector`: a cached `Projector` of the same pair and the same method."""
    projector, to_cart = _pair(field, target_proj, method, projector)
    return projector.to_cart(field) if to_cart else projector.to_healpix(field)


def project_adjoint(g, source_proj, method="bilinear", projector=None):
    """The transpose (pullback) of `project(., g's projection)` for an input that lived on `source_proj`: a cotangent on the sphere
    (HealpixField) comes back to the Cartesian `source_proj` as a MAP Field / EquiRectField (`Projector.to_healpix_adjoint`), a cotangent on
    a patch (MAP Field / EquiRectField) comes back to `source_proj = ProjHealpix(Nside)` as a HealpixField (`Projector.to_cart_adjoint`).
    The same pair / method / projector checks as `project`.  This is what autograd runs when `project` is given a field whose tensor has
    `requires_grad`."""
    projector, on_sphere = _pair(g, source_proj, method, projector)
    return projector.to_healpix_adjoint(g) if on_sphere else projector.to_cart_adjoint(g)
