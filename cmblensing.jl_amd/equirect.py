"""The reference's second Cartesian projection (src/proj_equirect.jl) on top of the C ABI: `ProjEquiRect`, fields in the Map / AzFourier
(QUMap / QUAzFourier) bases and the block-diagonal operators `BlockDiagEquiRect`.

Tensor layouts are the reference's arrays read row-major: maps (B, P, Nx, Ny) real == Julia (Ny, Nx, P, B); AzFourier fields (B, Nx//2+1, n)
complex == Julia (n, Nx÷2+1, B) with n = Ny (I) or 2 Ny (QU); operator blocks (Nx//2+1, n, n) indexed [m, q, p] == Julia blocks[p, q, m].
`blocks_from_ref` / `blocks_to_ref` move between that and NumPy arrays indexed [p, q, m] like the reference's.

On the device: the four transforms, `M * f`, `M' * f`, the three operator products, `dot(M1', M2)` and the beams.  `sqrt` (SVD, :313-323),
`pinv`, `logabsdet` / `logdet`, `solve` (`\\`) and `rdiv` (`/`) run once per operator either on the host, in float64 and batched over m
(numpy.linalg; `factor_on="host"`, the default), or on the device (`factor_on="device"`, or `on="device"` for one call: a batched one-sided
Jacobi SVD and a batched LU, one workgroup per block, arithmetic in double, blocks up to n = 2048).  `+`, `-`, scalar `*`, `/` are torch,
elementwise.  `sqrt` / `pinv` / `logabsdet` are cached on the object per path, like the reference's `Ref`s.  `Cl_to_Cov` (:430-503) builds the isotropic covariance blocks on the device, in double, from their definition (the reference
delegates to CirculantCov.jl, whose own numbers are not compared here).  `EquiRectDataSet` is the reference's NoLensingDataSet on this projection with its Wiener filter on the device.  NOT here: the AD rules; lensing on this projection."""
import ctypes

import numpy as np
import torch

from .lib import load_library, check
from .engine import ProjLambert, MAP, _ptr

AZFOURIER = 3
SIDE_LEFT, SIDE_RIGHT = 0, 1                   # CMBL_SIDE_* of cmbl_equirect_block_solve
DEVICE_FACTOR_NMAX = 2048                      # largest block the device factorisations take
PINV_RTOL = 1e-15                              # numpy.linalg.pinv's default cut
_PD = ctypes.POINTER(ctypes.c_double)


def equirect_geometry(Ny, Nx, theta_span, phi_span):
    """ProjEquiRect(; Ny, Nx, θspan, φspan) (src/proj_equirect.jl:71-81, 112-120) on the host in double (`cmbl_equirect_geometry_host`; needs no
    device): dict of theta (Ny), phi (Nx), theta_edges (Ny+1), phi_edges (Nx+1), omega (Ny) and lx (Ny, Nx)."""
    lib = load_library()
    Ny, Nx = int(Ny), int(Nx)
    ts, ps = np.array(theta_span, dtype=np.float64), np.array(phi_span, dtype=np.float64)
    g = {"theta": np.empty(Ny), "phi": np.empty(Nx), "theta_edges": np.empty(Ny + 1), "phi_edges": np.empty(Nx + 1), "omega": np.empty(Ny),
         "lx": np.empty((Nx, Ny))}
    p = lambda a: a.ctypes.data_as(_PD)
    check(lib.cmbl_equirect_geometry_host(Ny, Nx, p(ts), p(ps), p(g["theta"]), p(g["phi"]), p(g["theta_edges"]), p(g["phi_edges"]), p(g["omega"]), p(g["lx"])))
    g["lx"] = np.ascontiguousarray(g["lx"].T)                                # the library writes the Julia array (Ny contiguous)
    return g


class ProjEquiRect:
    """`ProjEquiRect(; Ny, Nx, θspan, φspan, T)` (src/proj_equirect.jl:83-127).  The spans are in radians, in either order.  The geometry fields
    (`theta`, `phi`, `theta_edges`, `phi_edges`, `omega`, `lx`) are NumPy arrays of the precision `T`, like the reference's `T.(…)`."""

    def __init__(self, Ny, Nx, theta_span, phi_span, T=torch.float32, device=0):
        self.Ny, self.Nx, self.Mh = int(Ny), int(Nx), int(Nx) // 2 + 1
        self.theta_span, self.phi_span = tuple(sorted(float(v) for v in theta_span)), tuple(sorted(float(v) for v in phi_span))
        self.T = T
        self.CT = torch.complex64 if T == torch.float32 else torch.complex128
        npT = np.float32 if T == torch.float32 else np.float64
        for k, v in equirect_geometry(Ny, Nx, theta_span, phi_span).items():
            setattr(self, k, v.astype(npT))
        self._ctx = ProjLambert(Ny, Nx, 1.0, T, device)                      # the context: sizes, precision, stream, scratch (its pixel size is not used)
        self.lib, self._h, self.device = self._ctx.lib, self._ctx._h, self._ctx.device

    def __eq__(self, o):
        return isinstance(o, ProjEquiRect) and (self.Ny, self.Nx, self.theta_span, self.phi_span, self.T, self.device) == \
            (o.Ny, o.Nx, o.theta_span, o.phi_span, o.T, o.device)

    __hash__ = None

    def synchronize(self):
        self._ctx.synchronize()

    def tensor(self, a):
        return self._ctx.tensor(a)


def _same_proj(a, b):
    if a is not b and a != b:
        raise ValueError("fields / operators of different ProjEquiRect projections")      # promote_metadata_strict


class EquiRectField:
    """A spin-0 (P = 1) or spin-2 (P = 2) field on a ProjEquiRect in the MAP or AZFOURIER basis.  `arr`: MAP (B, P, Nx, Ny) real; AZFOURIER
    (B, Nx//2+1, P Ny) complex."""

    def __init__(self, proj, arr, basis):
        self.proj, self.basis = proj, int(basis)
        t = proj.tensor(arr)
        if self.basis == MAP:
            if t.dim() == 3:
                t = t[None]
            ok = t.dim() == 4 and t.shape[1] in (1, 2) and tuple(t.shape[2:]) == (proj.Nx, proj.Ny) and t.dtype == proj.T
            self.P = int(t.shape[1]) if ok else 0
        elif self.basis == AZFOURIER:
            if t.dim() == 2:
                t = t[None]
            ok = t.dim() == 3 and t.shape[1] == proj.Mh and t.shape[2] in (proj.Ny, 2 * proj.Ny) and t.dtype == proj.CT
            self.P = int(t.shape[2]) // proj.Ny if ok else 0
        else:
            raise ValueError("EquiRectField: the basis is MAP or AZFOURIER")
        if not ok:
            raise ValueError(f"EquiRectField: array of shape {tuple(t.shape)} / {t.dtype} does not fit a {proj.Ny} x {proj.Nx} projection in basis {basis}")
        if self.P == 2 and proj.Nx % 2:
            raise ValueError("EquiRectField: QU fields need an even Nx (src/proj_equirect.jl:166)")
        self.arr = t.contiguous()
        self.B = int(t.shape[0])

    def to(self, basis):
        """Map <-> AzFourier, QUMap <-> QUAzFourier (src/proj_equirect.jl:149-178)"""
        if basis == self.basis:
            return self
        p = self.proj
        if basis == MAP:
            out = torch.empty((self.B, self.P, p.Nx, p.Ny), dtype=p.T, device=p.device)
        elif basis == AZFOURIER:
            out = torch.empty((self.B, p.Mh, self.P * p.Ny), dtype=p.CT, device=p.device)
        else:
            raise ValueError("EquiRectField.to: the basis is MAP or AZFOURIER")
        check(p.lib.cmbl_equirect_convert(p._h, self.basis, _ptr(self.arr), basis, _ptr(out), self.P, self.B))
        return EquiRectField(p, out, basis)

    def dot(self, other):
        """dot(a, b) = dot(Ł(a).arr, Ł(b).arr) (src/proj_equirect.jl:355): the plain dot product of the map arrays, batch included"""
        _same_proj(self.proj, other.proj)
        return float(torch.dot(self.to(MAP).arr.reshape(-1), other.to(MAP).arr.reshape(-1)))

    def dot_batch(self, other):
        """dot(a, b) per batch slot (src/proj_equirect.jl:355), on the device in double with no transform: of the map arrays, or -- both fields in
        the AZFOURIER basis -- the same number formed there (`cmbl_equirect_field_dot`; exact for images of maps).  NumPy array (B,)."""
        _same_proj(self.proj, other.proj)
        o = other.to(self.basis)
        if o.B != self.B or o.P != self.P:
            raise ValueError("dot_batch: fields of different batch size or spin")
        out = np.empty(self.B)
        check(self.proj.lib.cmbl_equirect_field_dot(self.proj._h, self.basis, _ptr(self.arr), _ptr(o.arr), self.P, self.B, out.ctypes.data_as(_PD)))
        return out

    # f[:Ix], f[:Il] (spin 0); f[:Qx], f[:Ux], f[:Px], f[:Pl] (spin 2) (src/proj_equirect.jl:181-196)
    def __getitem__(self, k):
        if self.P == 1 and k == "Ix":
            return self.to(MAP).arr[:, 0]
        if self.P == 1 and k == "Il":
            return self.to(AZFOURIER).arr
        if self.P == 2 and k in ("Qx", "Ux"):
            return self.to(MAP).arr[:, 0 if k == "Qx" else 1]
        if self.P == 2 and k == "Px":
            m = self.to(MAP).arr
            return torch.complex(m[:, 0], m[:, 1])
        if self.P == 2 and k == "Pl":
            return self.to(AZFOURIER).arr
        raise KeyError(f"invalid index {k!r} for a spin-{0 if self.P == 1 else 2} EquiRectField")

    def __mul__(self, a):
        return EquiRectField(self.proj, self.arr * a, self.basis)

    __rmul__ = __mul__

    def __add__(self, o):
        _same_proj(self.proj, o.proj)
        return EquiRectField(self.proj, self.arr + o.to(self.basis).arr, self.basis)

    def __sub__(self, o):
        _same_proj(self.proj, o.proj)
        return EquiRectField(self.proj, self.arr - o.to(self.basis).arr, self.basis)


def blocks_from_ref(a):
    """NumPy blocks indexed [p, q, m] like the reference's -> the row-major array [m, q, p] the device holds"""
    return np.ascontiguousarray(np.transpose(np.asarray(a), (2, 1, 0)))


def blocks_to_ref(t):
    """device blocks [m, q, p] -> NumPy array indexed [p, q, m]"""
    return np.transpose((t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)), (2, 1, 0))


class _Adjoint:
    def __init__(self, parent):
        self.parent = parent

    @property
    def H(self):
        return self.parent

    def __mul__(self, x):
        if isinstance(x, EquiRectField):
            return self.parent._apply(x, True)
        if isinstance(x, BlockDiagEquiRect):
            return self.parent._matmul(x, True, False)
        if isinstance(x, _Adjoint):
            raise TypeError("the product of two adjoints is not defined (src/proj_equirect.jl:254-269)")
        return (self.parent * np.conj(x)).H                                  # (conj(a) * M.parent)' (:305-306)

    __matmul__ = __mul__

    def dot(self, M2):
        """dot(M1', M2) = Σ conj(M1[q, p, m]) M2[p, q, m] (src/proj_equirect.jl:358-360)"""
        return self.parent._dot(M2)


class BlockDiagEquiRect:
    """`BlockDiagEquiRect{B}(blocks, proj)` (src/proj_equirect.jl:209-222): one n x n block per azimuthal mode m, n = Ny (AzFourier) or 2 Ny
    (QUAzFourier), real or complex.  `blocks`: device tensor or array (Nx//2+1, n, n) indexed [m, q, p] (`blocks_from_ref` converts the
    reference's [p, q, m])."""

    def __init__(self, blocks, proj, basis=AZFOURIER, factor_on="host"):
        if basis != AZFOURIER:
            raise ValueError("BlockDiagEquiRect: the basis is AZFOURIER")
        if factor_on not in ("host", "device"):
            raise ValueError("BlockDiagEquiRect: factor_on is 'host' or 'device'")
        self.factor_on = factor_on
        t = proj.tensor(blocks)
        if t.dim() != 3 or t.shape[0] != proj.Mh or t.shape[1] != t.shape[2] or t.shape[1] not in (proj.Ny, 2 * proj.Ny):
            raise ValueError(f"BlockDiagEquiRect: blocks of shape {tuple(t.shape)}, expected ({proj.Mh}, n, n) with n = Ny or 2 Ny")
        self.proj, self.basis, self.blocks = proj, basis, t.contiguous()
        self.n, self.complex = int(t.shape[1]), bool(t.is_complex())
        self._sqrt, self._pinv, self._logabsdet = {}, {}, {}              # caches, keyed by the path ("host" / "device"; pinv: and rtol)

    # ---- device products
    def _apply(self, f, adjoint):
        _same_proj(self.proj, f.proj)
        f = f.to(AZFOURIER)                                                  # M * B(f) (:228)
        if f.arr.shape[2] != self.n:
            raise ValueError(f"operator blocks of size {self.n} on a field with {f.arr.shape[2]} rows")
        out = torch.empty_like(f.arr)
        p = self.proj
        check(p.lib.cmbl_equirect_block_apply(p._h, _ptr(self.blocks), int(self.complex), self.n, int(adjoint), _ptr(f.arr), _ptr(out), f.B))
        return EquiRectField(p, out, AZFOURIER)

    def _pair(self, o):
        _same_proj(self.proj, o.proj)
        if o.n != self.n:
            raise ValueError("operators of different block sizes")
        a, b = self.blocks, o.blocks
        if self.complex != o.complex:
            a, b = a.to(self.proj.CT), b.to(self.proj.CT)
        return a, b

    def _matmul(self, o, adjA, adjB):
        a, b = self._pair(o)
        out = torch.empty_like(a)
        p = self.proj
        check(p.lib.cmbl_equirect_block_matmul(p._h, _ptr(a), int(adjA), _ptr(b), int(adjB), int(a.is_complex()), self.n, _ptr(out)))
        return BlockDiagEquiRect(out, p)

    def _dot(self, o):
        a, b = self._pair(o)
        out = (ctypes.c_double * 2)()
        p = self.proj
        check(p.lib.cmbl_equirect_block_dot(p._h, _ptr(a), _ptr(b), int(a.is_complex()), self.n, out))
        return complex(out[0], out[1])

    @property
    def H(self):
        return _Adjoint(self)

    def __mul__(self, x):
        if isinstance(x, EquiRectField):
            return self._apply(x, False)
        if isinstance(x, BlockDiagEquiRect):
            return self._matmul(x, False, False)
        if isinstance(x, _Adjoint):
            return self._matmul(x.parent, False, True)
        return BlockDiagEquiRect(self.blocks * x, self.proj)

    __matmul__ = __mul__

    def __rmul__(self, a):
        return BlockDiagEquiRect(self.blocks * a, self.proj)

    def __truediv__(self, x):
        if isinstance(x, BlockDiagEquiRect):
            return self.rdiv(x)
        return BlockDiagEquiRect(self.blocks / x, self.proj)

    def __add__(self, o):
        a, b = self._pair(o)
        return BlockDiagEquiRect(a + b, self.proj)

    def __sub__(self, o):
        a, b = self._pair(o)
        return BlockDiagEquiRect(a - b, self.proj)

    def scale_columns(self, w):
        """blocks[j, k, m] *= w[k] in place (the step of Cℓ_to_Beam(:I), src/proj_equirect.jl:512)"""
        w = np.ascontiguousarray(w, dtype=np.float64)
        p = self.proj
        check(p.lib.cmbl_equirect_block_scale_columns(p._h, _ptr(self.blocks), int(self.complex), self.n, w.ctypes.data_as(_PD), w.size))
        self._sqrt, self._pinv, self._logabsdet = {}, {}, {}
        return self

    # ---- factorisations, once per operator and path: on the host (numpy.linalg, float64, batched over m) or on the device (one workgroup per
    #      block, arithmetic in double, cmbl_equirect_block_svd / _logabsdet / _solve); `on` overrides `factor_on` for one call
    def _on(self, on):
        on = self.factor_on if on is None else on
        if on not in ("host", "device"):
            raise ValueError(f"BlockDiagEquiRect: the factorisations run on 'host' or 'device', not {on!r}")
        if on == "device" and self.n > DEVICE_FACTOR_NMAX:
            raise ValueError(f"BlockDiagEquiRect: the device factorisations take blocks up to n = {DEVICE_FACTOR_NMAX}, these have n = {self.n}: "
                             "the host path remains (on='host')")
        return on

    def _host(self):
        a = self.blocks.detach().cpu().numpy().transpose(0, 2, 1)            # [m, p, q]
        return a.astype(np.complex128 if self.complex else np.float64)

    def _from_host(self, a):
        a = np.ascontiguousarray(np.transpose(a, (0, 2, 1)))
        if not self.complex:
            a = a.real
        return BlockDiagEquiRect(self.proj.tensor(a), self.proj, factor_on=self.factor_on)

    def _device_svd(self, rtol, want_sqrt, want_pinv, want_sv=False):
        """one Jacobi SVD of every block on the device: (sqrt or None, pinv or None, singular values (Mh, n) descending or None)"""
        p = self.proj
        new = lambda: BlockDiagEquiRect(torch.empty_like(self.blocks), p, factor_on=self.factor_on)
        sq, pi = (new() if want_sqrt else None), (new() if want_pinv else None)
        sv = np.empty((p.Mh, self.n)) if want_sv else None
        check(p.lib.cmbl_equirect_block_svd(p._h, _ptr(self.blocks), int(self.complex), self.n, float(rtol), _ptr(sq.blocks) if sq else None,
                                            _ptr(pi.blocks) if pi else None, sv.ctypes.data_as(_PD) if want_sv else None, None))
        return sq, pi, sv

    def sqrt(self, on=None):
        """U * Diagonal(sqrt.(S)) * V' of the SVD of every block (src/proj_equirect.jl:313-323)"""
        on = self._on(on)
        if on not in self._sqrt:
            if on == "host":
                u, s, vh = np.linalg.svd(self._host())
                self._sqrt[on] = self._from_host((u * np.sqrt(s)[:, None, :]) @ vh)
            else:
                self._sqrt[on] = self._device_svd(PINV_RTOL, True, False)[0]
        return self._sqrt[on]

    def pinv(self, rtol=None, on=None):
        """the pseudo-inverse of every block; singular values at or below rtol * the block's largest are dropped (default 1e-15, numpy.linalg.pinv's)"""
        on = self._on(on)
        rtol = PINV_RTOL if rtol is None else float(rtol)
        if (on, rtol) not in self._pinv:
            self._pinv[(on, rtol)] = self._from_host(np.linalg.pinv(self._host(), rcond=rtol)) if on == "host" else self._device_svd(rtol, False, True)[1]
        return self._pinv[(on, rtol)]

    def svdvals(self, on=None):
        """the singular values of every block, descending: NumPy array (Mh, n) of doubles"""
        if self._on(on) == "host":
            return np.linalg.svd(self._host(), compute_uv=False)
        return self._device_svd(PINV_RTOL, False, False, True)[2]

    def logabsdet(self, on=None):
        """(Σ log|det|, Π sign) over the blocks (src/proj_equirect.jl:342-347)"""
        on = self._on(on)
        if on not in self._logabsdet:
            if on == "host":
                sign, lad = np.linalg.slogdet(self._host())
                self._logabsdet[on] = (float(lad.sum()), complex(np.prod(sign)))
            else:
                out = (ctypes.c_double * 3)()
                p = self.proj
                check(p.lib.cmbl_equirect_block_logabsdet(p._h, _ptr(self.blocks), int(self.complex), self.n, out))
                self._logabsdet[on] = (float(out[0]), complex(out[1], out[2]))
        return self._logabsdet[on]

    def logdet(self, on=None):
        l, s = self.logabsdet(on)
        v = l + np.log(s)
        return float(v.real) if abs(v.imag) < 1e-12 else v

    def _device_solve(self, side, rhs, rhs_complex, field, B=1):
        p = self.proj
        out = torch.empty(rhs.shape, dtype=p.CT if (self.complex or rhs_complex) else p.T, device=p.device)
        check(p.lib.cmbl_equirect_block_solve(p._h, _ptr(self.blocks), int(self.complex), self.n, side, _ptr(rhs), int(rhs_complex), int(field), _ptr(out), int(B)))
        return out

    def solve(self, o, on=None):
        """M₁ \\ M₂, blockwise (src/proj_equirect.jl:274-282), or M \\ f for a field (the reference's mapblocks(\\, M, f)): an `EquiRectField`"""
        _same_proj(self.proj, o.proj)
        on = self._on(on)
        if isinstance(o, EquiRectField):
            f = o.to(AZFOURIER)
            if f.arr.shape[2] != self.n:
                raise ValueError(f"operator blocks of size {self.n} on a field with {f.arr.shape[2]} rows")
            if on == "host":
                x = np.linalg.solve(self._host()[None], f.arr.detach().cpu().numpy().astype(np.complex128)[..., None])[..., 0]
                return EquiRectField(self.proj, self.proj.tensor(x.astype(np.complex64 if self.proj.T == torch.float32 else np.complex128)), AZFOURIER)
            return EquiRectField(self.proj, self._device_solve(SIDE_LEFT, f.arr, True, True, f.B), AZFOURIER)
        if o.n != self.n:
            raise ValueError("operators of different block sizes")
        if on == "host":
            r = np.linalg.solve(self._host(), o._host())
            return (self if self.complex or not o.complex else o)._from_host(r)
        return BlockDiagEquiRect(self._device_solve(SIDE_LEFT, o.blocks, o.complex, False), self.proj, factor_on=self.factor_on)

    def rdiv(self, o, on=None):
        """M₁ / M₂ = M₁ M₂⁻¹, blockwise"""
        _same_proj(self.proj, o.proj)
        if self._on(on) == "host":
            a, b = self._host(), o._host()
            r = np.conj(np.transpose(np.linalg.solve(np.conj(np.transpose(b, (0, 2, 1))), np.conj(np.transpose(a, (0, 2, 1)))), (0, 2, 1)))
            return (self if self.complex or not o.complex else o)._from_host(r)
        if o.n != self.n:
            raise ValueError("operators of different block sizes")
        return BlockDiagEquiRect(o._device_solve(SIDE_RIGHT, self.blocks, self.complex, False), self.proj, factor_on=self.factor_on)


def _cl_array(Cl, lmax):
    """nan2zero.(C(0:ℓmax)) of a `Cls`-like callable (anything with `ell` and `__call__`), or an array over ℓ = 0, 1, ...; ℓmax clamped to what it holds"""
    if callable(Cl) and hasattr(Cl, "ell"):
        lmax = min(int(lmax), int(np.floor(np.max(Cl.ell))))
        a = np.asarray(Cl(np.arange(lmax + 1)), dtype=np.float64)
    else:
        a = np.asarray(Cl, dtype=np.float64).ravel()
        lmax = min(int(lmax), a.size - 1)
        a = a[:lmax + 1]
    return np.ascontiguousarray(np.where(np.isnan(a), 0.0, a)), lmax


def Cl_to_Cov(pol, proj, Cl, Cl_BB=None, units=1, lmax=10_000, ngrid=50_000):
    """Cℓ_to_Cov(:I, proj, CI) / Cℓ_to_Cov(:P, proj, CEE, CBB) (src/proj_equirect.jl:436-501): the `BlockDiagEquiRect` covariance of an isotropic
    Gaussian field with the given spectra (`Cls` objects, or arrays over ℓ = 0, 1, ...), built on the device in double and rounded to the
    projection's precision at the store.  `ngrid`: nodes of the correlation-function table on [0, π] (the reference's CirculantCov uses 50 000);
    0 evaluates the recurrences at every separation (exact, slow at large sizes).  The azimuthal span must be 2π/K.  `units` is accepted and
    unused, as in the reference's body."""
    if pol not in ("I", "P"):
        raise ValueError("Cl_to_Cov: pol is 'I' or 'P'")
    if (pol == "P") != (Cl_BB is not None):
        raise ValueError("Cl_to_Cov: 'I' takes one spectrum, 'P' the EE and the BB spectrum")
    a, la = _cl_array(Cl, lmax)
    b, lb = _cl_array(Cl_BB, lmax) if pol == "P" else (None, la)
    l = min(la, lb)
    n = proj.Ny if pol == "I" else 2 * proj.Ny
    out = torch.empty((proj.Mh, n, n), dtype=proj.T if pol == "I" else proj.CT, device=proj.device)
    ts, ps = (np.array(s, dtype=np.float64) for s in (proj.theta_span, proj.phi_span))
    p = lambda x: x.ctypes.data_as(_PD)
    check(proj.lib.cmbl_equirect_cov(proj._h, p(ts), p(ps), 0 if pol == "I" else 2, l, p(a), p(b) if b is not None else None, int(ngrid), _ptr(out)))
    return BlockDiagEquiRect(out, proj)


def Cl_to_Beam(pol, cov_I_blocks, proj, lmax=10_000, ngrid=50_000):
    """Cℓ_to_Beam(:I / :P) (src/proj_equirect.jl:505-533) from the real blocks of Cℓ_to_Cov(:I) -- a `BlockDiagEquiRect`, a block array, or the
    spectrum itself (a `Cls` or an array over ℓ, as in the reference; the covariance is then built here with `lmax`, `ngrid`): `"I"`:
    blocks[j, k, m] * Ω[k]; `"P"`: [B 0; 0 B] * diag(Ω, Ω), complex 2Ny blocks."""
    if (callable(cov_I_blocks) and hasattr(cov_I_blocks, "ell")) or (not isinstance(cov_I_blocks, BlockDiagEquiRect) and np.ndim(cov_I_blocks) == 1):
        cov_I_blocks = Cl_to_Cov("I", proj, cov_I_blocks, lmax=lmax, ngrid=ngrid)
    M = cov_I_blocks if isinstance(cov_I_blocks, BlockDiagEquiRect) else BlockDiagEquiRect(cov_I_blocks, proj)
    _same_proj(M.proj, proj)
    if M.complex or M.n != proj.Ny:
        raise ValueError("Cl_to_Beam: the :I covariance has real Ny x Ny blocks")
    om = np.ascontiguousarray(proj.omega, dtype=np.float64)
    if pol == "I":
        return BlockDiagEquiRect(M.blocks.clone(), proj).scale_columns(om)
    if pol == "P":
        out = torch.empty((proj.Mh, 2 * proj.Ny, 2 * proj.Ny), dtype=proj.CT, device=proj.device)
        check(proj.lib.cmbl_equirect_beam_pol(proj._h, _ptr(M.blocks), om.ctypes.data_as(_PD), _ptr(out)))
        return BlockDiagEquiRect(out, proj)
    raise ValueError("Cl_to_Beam: pol is 'I' or 'P'")


def simulate(M, seed=0, nbatch=1):
    """simulate(rng, M) = sqrt(M) * white map (src/proj_equirect.jl:399-405), the white map from the device generator (Philox keyed by
    seed + slot).  Returns an AZFOURIER field, like the reference's `M * f`."""
    p = M.proj
    P = M.n // p.Ny
    white = p._ctx.randn([int(seed) + b for b in range(int(nbatch))], 0, P)
    return M.sqrt() * EquiRectField(p, white, MAP)


# ---- NoLensingDataSet on ProjEquiRect (src/dataset.jl:37-47, 59-80, 129-132; src/maximization.jl:17-42) ---------------------------------------
EQDS_CF_INV, EQDS_B, EQDS_PRECOND_INV, EQDS_CN_INV = 0, 1, 2, 3           # CMBL_EQDS_* block operators
EQDS_MASK, EQDS_CN_INV_PIX = 0, 1                                          # CMBL_EQDS_* map-diagonal operators


def maps_images_to_images(op):
    """How far the blocks of `op` at columns m = 0 and m = Nx/2 are from mapping images of maps to images of maps: the largest violation over the
    two columns, relative to the block's largest element -- of being real (spin 0), of commuting with v -> S conj(v), S the swap of the two
    halves (spin 2).  0.0 for an operator that qualifies exactly; `EquiRectDataSet` accepts up to 64 ulp of the projection's precision."""
    p = op.proj
    cols = [0, p.Nx // 2] if p.Nx % 2 == 0 else [0]
    worst = 0.0
    for m in cols:
        H = op.blocks[m]
        scale = float(H.abs().max()) or 1.0
        if op.n == p.Ny:
            dev = float(H.imag.abs().max()) if op.complex else 0.0
        else:
            dev = float((H - torch.roll(H, (p.Ny, p.Ny), (0, 1)).conj()).abs().max())
        worst = max(worst, dev / scale)
    return worst


def _sandwich(X, A):
    """A' X A, X and A each a BlockDiagEquiRect or a real scalar (times the identity)"""
    if not isinstance(A, BlockDiagEquiRect):
        return X * (A * A)
    if not isinstance(X, BlockDiagEquiRect):
        return (A.H * A) * X
    return A.H * (X * A)


class EquiRectDataSet:
    """The reference's `NoLensingDataSet` (src/dataset.jl:37-47) on a ProjEquiRect:  d = M B f + noise,  f ~ N(0, Cf),  noise ~ N(0, Cn).

    `Cf`, `B` (None: identity): `BlockDiagEquiRect`.  `M` (None: identity): map-diagonal, planes (P or 1, Nx, Ny) (the reference's
    `Diagonal(::EquiRectMap)`).  `Cn`: a `BlockDiagEquiRect`, or map-diagonal -- a VARIANCE map (P or 1, Nx, Ny) for inhomogeneous white noise.
    `d`: a MAP field, the default data of the methods.  The preconditioner is pinv(pinv(Cf) + B̂' M̂' pinv(Cn̂) M̂ B̂) (:129-132), a `BlockDiagEquiRect`
    formed once; the hats default to the operators where those are block-diagonal, and where `M` / `Cn` is map-diagonal `Mhat=` / `Cnhat=` are
    REQUIRED (a `BlockDiagEquiRect` or a real scalar times the identity): the reference has no default that type-checks, and none is guessed.

    The reference's `argmaxf_logpdf` (src/maximization.jl:17-42) begins with `zero(diag(ds.Cf))` and defines no `diag(::BlockDiagEquiRect)`, so as
    written it does not run on such a data set; this is its algorithm (`conjugate_gradient`, src/numerical_algorithms.jl:73-134) on its own
    operators, started from the zero field of Cf's basis.  PRECONDITION: every block operator maps images of maps to images of maps (see
    `maps_images_to_images`; `Cl_to_Cov` and `Cl_to_Beam` produce such blocks): the solver holds its vectors in the Az basis, which is the
    reference's inner product under that condition only.  The constructor checks the two columns concerned and refuses otherwise."""

    def __init__(self, proj, Cf, Cn, d=None, M=None, B=None, Cnhat=None, Mhat=None, Bhat=None):
        self.proj, self.Cf, self.Cn, self.M, self.B, self.d = proj, Cf, Cn, None, B, None
        if not isinstance(Cf, BlockDiagEquiRect):
            raise ValueError("EquiRectDataSet: Cf is a BlockDiagEquiRect")
        _same_proj(proj, Cf.proj)
        self.P = Cf.n // proj.Ny
        self.cn_block = isinstance(Cn, BlockDiagEquiRect)
        if M is not None:
            self.M = self._planes(M, "M")
        if not self.cn_block:
            self.Cn = self._planes(Cn, "Cn")
        if M is not None and Mhat is None:
            raise ValueError("EquiRectDataSet: M is map-diagonal, so Mhat= is required (a BlockDiagEquiRect or a real scalar): the reference has no default that type-checks")
        if not self.cn_block and Cnhat is None:
            raise ValueError("EquiRectDataSet: Cn is map-diagonal, so Cnhat= is required (a BlockDiagEquiRect or a real scalar): the reference has no default that type-checks")
        self.Bhat = Bhat if Bhat is not None else B
        self.Mhat = Mhat if Mhat is not None else 1.0
        self.Cnhat = Cnhat if Cnhat is not None else Cn
        tol = 64 * torch.finfo(proj.T).eps
        for name, op in (("Cf", Cf), ("B", B), ("Cn", Cn if self.cn_block else None), ("Bhat", self.Bhat), ("Mhat", self.Mhat), ("Cnhat", self.Cnhat)):
            if isinstance(op, BlockDiagEquiRect):
                _same_proj(proj, op.proj)
                if op.n != Cf.n:
                    raise ValueError(f"EquiRectDataSet: {name} has blocks of size {op.n}, Cf of size {Cf.n}")
                v = maps_images_to_images(op)
                if v > tol:
                    raise ValueError(f"EquiRectDataSet: the blocks of {name} at columns 0 and Nx/2 do not map images of maps to images of maps "
                                     f"(relative violation {v:.2e}): real blocks for spin 0, blocks commuting with v -> S conj(v) for spin 2")
        self.CfI = Cf.pinv()
        self.CnI = Cn.pinv() if self.cn_block else (1.0 / self.Cn).contiguous()
        self._precond = None
        self._h = ctypes.c_void_p()
        check(proj.lib.cmbl_eqds_create(proj._h, self.P, ctypes.byref(self._h)))
        self._set_block(EQDS_CF_INV, self.CfI)
        if B is not None:
            self._set_block(EQDS_B, B)
        if self.cn_block:
            self._set_block(EQDS_CN_INV, self.CnI)
        else:
            check(proj.lib.cmbl_eqds_set_pixel_op(self._h, EQDS_CN_INV_PIX, _ptr(self.CnI), int(self.CnI.shape[0])))
        if self.M is not None:
            check(proj.lib.cmbl_eqds_set_pixel_op(self._h, EQDS_MASK, _ptr(self.M), int(self.M.shape[0])))
        ld_n = Cn.logdet() if self.cn_block else float(torch.log(self.Cn.double()).sum()) * (self.P / self.Cn.shape[0])
        self.logdet_sum = float(np.real(Cf.logdet())) + float(np.real(ld_n))
        check(proj.lib.cmbl_eqds_set_logdet(self._h, self.logdet_sum))
        if d is not None:
            self.d = self._data(d)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self.proj.lib.cmbl_eqds_destroy(h)

    def _planes(self, a, name):
        p = self.proj
        t = p.tensor(a.arr[0] if isinstance(a, EquiRectField) else a)
        if t.dim() == 2:
            t = t[None]
        if t.dim() != 3 or t.shape[0] not in (1, self.P) or tuple(t.shape[1:]) != (p.Nx, p.Ny) or t.dtype != p.T:
            raise ValueError(f"EquiRectDataSet: {name} is map-diagonal: planes (P or 1, Nx, Ny) of the projection's precision, not {tuple(t.shape)} / {t.dtype}")
        return t.contiguous()

    def _set_block(self, which, op):
        self._keep = getattr(self, "_keep", {})
        self._keep[which] = op                                               # the library holds a view: keep the array alive
        check(self.proj.lib.cmbl_eqds_set_block_op(self._h, which, _ptr(op.blocks), int(op.complex), op.n))

    def _field(self, f):
        f = f if isinstance(f, EquiRectField) else EquiRectField(self.proj, f, AZFOURIER)
        f = f.to(AZFOURIER)
        if f.P != self.P:
            raise ValueError("EquiRectDataSet: a field of the wrong spin")
        return f

    def _data(self, d, B=None):
        if d is None:
            d = self.d
            if d is None:
                raise ValueError("EquiRectDataSet: no data given and none held")
        d = d if isinstance(d, EquiRectField) else EquiRectField(self.proj, d, MAP)
        d = d.to(MAP)
        if d.P != self.P or (B is not None and d.B != B):
            raise ValueError("EquiRectDataSet: data of the wrong spin or batch size")
        return d

    def mean(self, f):
        """M B f (src/dataset.jl:68-73 without L): a MAP field"""
        f = self._field(f)
        p = self.proj
        out = torch.empty((f.B, self.P, p.Nx, p.Ny), dtype=p.T, device=p.device)
        check(p.lib.cmbl_eqds_mean(self._h, _ptr(f.arr), _ptr(out), f.B))
        return EquiRectField(p, out, MAP)

    def _noise(self, white):
        if self.cn_block:
            return (self.Cn.sqrt() * white).to(MAP)
        return EquiRectField(self.proj, white.arr * torch.sqrt(self.Cn)[None], MAP)

    def simulate(self, seed=0, nbatch=1, white=None):
        """(f, d): f = sqrt(Cf) * white, d = M B f + sqrt(Cn) * white' (src/dataset.jl:49-57), the white maps from the device generator (Philox keyed
        by seed + slot; streams 0 and 1) as in `equirect.simulate`, or given as `white=(wf, wn)` (MAP fields)."""
        p = self.proj
        if white is None:
            seeds = [int(seed) + b for b in range(int(nbatch))]
            white = tuple(EquiRectField(p, p._ctx.randn(seeds, s, self.P), MAP) for s in (0, 1))
        f = self.Cf.sqrt() * white[0]
        return f, self.mean(f) + self._noise(white[1])

    def logpdf(self, f, d=None):
        """-½ [ (d - MBf)' Cn⁻¹ (d - MBf) + f' Cf⁻¹ f + logdet Cn + logdet Cf ] per batch slot (src/dataset.jl:59-66): NumPy array (B,)"""
        f = self._field(f)
        d = self._data(d, f.B)
        out = np.empty(f.B)
        check(self.proj.lib.cmbl_eqds_logpdf(self._h, _ptr(f.arr), _ptr(d.arr), out.ctypes.data_as(_PD), f.B))
        return out

    def gradientf_logpdf(self, f, d=None):
        """B' M' Cn⁻¹ (d - M B f) - Cf⁻¹ f (src/dataset.jl:76-80 without L), an AZFOURIER field.  `f=None`: f = 0; `d=0`: d = 0; `d=None`: the data held."""
        f = None if f is None else self._field(f)
        zero_d = d is not None and not isinstance(d, EquiRectField) and np.ndim(d) == 0 and d == 0
        d = None if zero_d else self._data(d, None if f is None else f.B)
        if f is None and d is None:
            raise ValueError("gradientf_logpdf: f = 0 and d = 0")
        B = f.B if f is not None else d.B
        p = self.proj
        out = torch.empty((B, p.Mh, self.P * p.Ny), dtype=p.CT, device=p.device)
        check(p.lib.cmbl_eqds_gradientf_logpdf(self._h, _ptr(f.arr) if f is not None else None, _ptr(d.arr) if d is not None else None, _ptr(out), B))
        return EquiRectField(p, out, AZFOURIER)

    def preconditioner(self):
        """pinv(pinv(Cf) + B̂' M̂' pinv(Cn̂) M̂ B̂) (src/dataset.jl:129-132), the operator multiplied onto the residual: a `BlockDiagEquiRect`, formed once"""
        if self._precond is None:
            X = self.Cnhat.pinv() if isinstance(self.Cnhat, BlockDiagEquiRect) else 1.0 / float(self.Cnhat)
            X = _sandwich(X, self.Mhat if isinstance(self.Mhat, BlockDiagEquiRect) else float(self.Mhat))
            if self.Bhat is not None:
                X = _sandwich(X, self.Bhat)
            if isinstance(X, BlockDiagEquiRect):
                tot = self.CfI + X
            else:
                eye = torch.eye(self.CfI.n, dtype=self.CfI.blocks.dtype, device=self.proj.device)
                tot = BlockDiagEquiRect(self.CfI.blocks + float(X) * eye[None], self.proj)
            self._precond = tot.pinv()
            self._set_block(EQDS_PRECOND_INV, self._precond)
        return self._precond

    def argmaxf_logpdf(self, d=None, fstart=None, tol=1e-1, nsteps=500):
        """The Wiener filter argmax_f logpdf (src/maximization.jl:17-42) by the reference's preconditioned CG (src/numerical_algorithms.jl:73-134),
        entirely on the device: (f, history), f the best-`res` iterate (AZFOURIER), history the residuals dot(r, z), NumPy (iterations, B).  Stops
        when all(res < tol)."""
        d = self._data(d)
        fs = None if fstart is None else self._field(fstart)
        if fs is not None and fs.B != d.B:
            raise ValueError("argmaxf_logpdf: fstart and d of different batch sizes")
        self.preconditioner()
        p = self.proj
        out = torch.empty((d.B, p.Mh, self.P * p.Ny), dtype=p.CT, device=p.device)
        hist = np.empty((int(nsteps), d.B))
        nit = ctypes.c_int(0)
        check(p.lib.cmbl_eqds_wiener_cg(self._h, _ptr(d.arr), _ptr(fs.arr) if fs is not None else None, float(tol), int(nsteps), _ptr(out),
                                        hist.ctypes.data_as(_PD), ctypes.byref(nit), d.B))
        return EquiRectField(p, out, AZFOURIER), hist[:nit.value].copy()

    def sample_f(self, seed=0, d=None, white=None, offset=False, **kw):
        """A posterior sample of f (src/maximization.jl:56-62): sim.f + argmaxf_logpdf(d - sim.d), sim = simulate(seed, B) or from `white=(wf, wn)`.
        The reference's `offset=true` adds a₀ = gradientf(f = 0, d = 0), identically zero for this model: accepted, does nothing.  `kw` go to
        `argmaxf_logpdf`.  Returns (f, history)."""
        d = self._data(d)
        sf, sd = self.simulate(seed, d.B, white=white)
        f, hist = self.argmaxf_logpdf(d - sd, **kw)
        return sf + f, hist
