"""NumPy restatement of the non-uniform-FFT method of the HEALPix projection (`project(...; method = :fft)`, src/proj_healpix.jl:229-236,
254-294, 314-325), on top of tests/_healpix_ref.py (geometry, lists, QU rotations).  tests/test_nfft_ref.py pins it.

Two things live here.

THE DEFINITION (float64, O(Npatch Ny Nx)): the exact sums that NFFT.jl's plans approximate.  With I_N = {-N/2, ..., N/2 - 1}, the grid nodes
x_g = ((i - Ny÷2 - 1) / Ny, (j - Nx÷2 - 1) / Nx) at the integer pixels, the HEALPix nodes x_p by the same formula at the fractional (i_p, j_p)
of hpx_idxs_in_patch, and K(x) = sum_{l in I_Ny x I_Nx} cos 2π l·x:
    Cartesian -> HEALPix   h_p = 1 / (Ny Nx)  sum_g m_g K(x_g - x_p)   on the patch, 0 elsewhere
    HEALPix -> Cartesian   m_g = 1 / Npatch   sum_p h_p K(x_p - x_g)
QU and IQU rotate by ψ at the HEALPix pixel on the way to the sphere and at the Cartesian pixel on the way to the patch.

THE WINDOW ALGORITHM (`Plan`, any dtype and width): the scheme the device runs -- fine grid 2Ny x 2Nx, exp-of-semicircle window
W(t) = exp(β (sqrt(1 - (2t/w)^2) - 1)) on |t| <= w/2 fine cells, β = 2.3 w, real transforms both ways.  K depends on differences only, so the
algorithm works with x' = x + 1/2, i.e. grid nodes at (i - 1) / Ny and fine-grid coordinates t = 2 (i_p - 1): no phase is needed.  Node
positions and window arguments are float64 and rounded once; window values, grids and transforms are `dtype`.

HEALPix fields are (B, P, npix), maps (B, P, Nx, Ny) (Ny fastest), like _healpix_ref."""
import numpy as np

import _healpix_ref as R

SIGMA = 2
BETA_PER_W = 2.3
WIDTH = {"f32": 8, "f64": 14}                 # cells per axis a node touches, per precision (from tests/golden/nfft_budget.json)
DTYPE = {"f32": np.float32, "f64": np.float64}
_GL = np.polynomial.legendre.leggauss(96)


# ---- the definition ------------------------------------------------------------------------------------------------------------------------
def dirichlet(N, d):
    """sum_{l in I_N} exp(2πi l d), elementwise"""
    l = np.arange(-(N // 2), N // 2)
    return np.exp(2j * np.pi * d[..., None] * l).sum(-1)


def kernel_matrix(Ny, Nx, i, j):
    """K(x_g - x_p) as (Npatch, Nx, Ny); (i, j) the 1-based fractional indices of the nodes"""
    Ey = dirichlet(Ny, (np.arange(1, Ny + 1)[None, :] - i[:, None]) / Ny)          # (Np, Ny)
    Ex = dirichlet(Nx, (np.arange(1, Nx + 1)[None, :] - j[:, None]) / Nx)          # (Np, Nx)
    return (Ex[:, :, None] * Ey[:, None, :]).real


# ---- the window ------------------------------------------------------------------------------------------------------------------------------
def es_window(t, w):
    """W(t), t in fine cells (float64)"""
    z = 2.0 * np.asarray(t, dtype=np.float64) / w
    return np.where(np.abs(z) <= 1.0, np.exp(BETA_PER_W * w * (np.sqrt(np.maximum(1.0 - z * z, 0.0)) - 1.0)), 0.0)


def es_hat(xi, w):
    """∫ W(t) cos(2π ξ t) dt over |t| <= w/2: with t = (w/2) sin θ the integrand is entire in θ; Gauss-Legendre on [0, π/2], doubled"""
    x, wt = _GL
    th = 0.25 * np.pi * (x + 1.0)
    f = np.exp(BETA_PER_W * w * (np.cos(th) - 1.0)) * np.cos(th) * (0.5 * w)
    return 2.0 * 0.25 * np.pi * (wt * f * np.cos(2.0 * np.pi * np.asarray(xi, dtype=np.float64)[..., None] * (0.5 * w) * np.sin(th))).sum(-1)


def _in_I(N, k):
    return (k >= -(N // 2)) & (k < N // 2)


class Plan:
    """the window algorithm for the nodes (i, j) (1-based, fractional, inside [1, Ny] x [1, Nx]) of an Ny x Nx grid"""

    def __init__(self, Ny, Nx, i, j, dtype=np.float64, w=None):
        self.dtype = np.dtype(dtype).type
        self.w = w = int(w if w is not None else WIDTH["f32" if self.dtype is np.float32 else "f64"])
        if Ny % 2 or Nx % 2 or SIGMA * min(Ny, Nx) < w or w % 2:
            raise ValueError("even sides whose fine grid holds one window of even width are needed")
        self.Ny, self.Nx, self.n = Ny, Nx, int(i.size)
        self.k0, self.win = [], []
        for c in (i, j):                                                     # y then x
            t = SIGMA * (np.asarray(c, dtype=np.float64) - 1.0)
            k0 = np.ceil(t - 0.5 * w).astype(np.int64)
            self.k0.append(k0)
            self.win.append(es_window(k0[:, None] + np.arange(w)[None, :] - t[:, None], w).astype(self.dtype))     # (Np, w)
        self.dec = [(1.0 / es_hat(np.arange(N // 2 + 1) / (SIGMA * N), w)).astype(self.dtype) for N in (Ny, Nx)]
        # the modes of the half plane [kx slot][ky], ky >= 0, as signed pairs; Nyquist as its negative (lm) or positive (lp) representative
        Ny2, Nx2 = Ny // 2, Nx // 2
        sx = np.arange(Nx)
        self.lxm, self.lxp = np.where(sx < Nx2, sx, sx - Nx), np.where(sx <= Nx2, sx, sx - Nx)
        ky = np.arange(Ny2 + 1)
        self.kym, self.kyp = np.where(ky < Ny2, ky, -Ny2), ky

    # -- Cartesian -> nodes (type 2) --
    def to_nodes(self, m):
        """(..., Nx, Ny) -> (..., Npatch):  1 / (Ny Nx) sum_g m_g K(x_g - x_p)"""
        Ny, Nx, w, T = self.Ny, self.Nx, self.w, self.dtype
        F = np.fft.rfft2(np.asarray(m, dtype=T), axes=(-2, -1))              # [kx slot][ky], unnormalised
        G = np.zeros(F.shape[:-2] + (2 * Nx, Ny + 1), dtype=F.dtype)
        lx = np.arange(-(Nx // 2), Nx // 2 + 1)
        ky = np.arange(Ny // 2 + 1)
        wgt = 0.5 * (_in_I(Ny, ky)[None, :] & _in_I(Nx, lx)[:, None]) + 0.5 * (_in_I(Ny, -ky)[None, :] & _in_I(Nx, -lx)[:, None])
        dec = self.dec[1][np.abs(lx)][:, None] * self.dec[0][ky][None, :]
        G[..., lx % (2 * Nx), : Ny // 2 + 1] = F[..., lx % Nx, :] * (T(4.0) * wgt.astype(T) * dec)
        g = np.fft.irfft2(G, s=(2 * Nx, 2 * Ny), axes=(-2, -1)).astype(T)      # divides by 4 Ny Nx
        iy = (self.k0[0][:, None] + np.arange(w)) % (2 * Ny)                 # (Np, w)
        ix = (self.k0[1][:, None] + np.arange(w)) % (2 * Nx)
        v = g[..., ix[:, :, None], iy[:, None, :]]                           # (..., Np, wx, wy)
        inner = (v * self.win[0][:, None, :]).sum(-1, dtype=T)
        return (inner * self.win[1]).sum(-1, dtype=T)

    # -- nodes -> Cartesian (type 1, the transpose) --
    def to_grid(self, h):
        """(..., Npatch) -> (..., Nx, Ny):  1 / Npatch sum_p h_p K(x_p - x_g)"""
        Ny, Nx, w, T = self.Ny, self.Nx, self.w, self.dtype
        h = np.asarray(h, dtype=T)
        lead = h.shape[:-1]
        h2 = h.reshape(-1, self.n)
        iy = (self.k0[0][:, None] + np.arange(w)) % (2 * Ny)
        ix = (self.k0[1][:, None] + np.arange(w)) % (2 * Nx)
        wxy = (self.win[1][:, :, None] * self.win[0][:, None, :]).astype(T)   # (Np, wx, wy)
        fine = np.zeros((h2.shape[0], 2 * Nx, 2 * Ny), dtype=T)
        flat = (ix[:, :, None] * (2 * Ny) + iy[:, None, :]).ravel()
        for b in range(h2.shape[0]):
            np.add.at(fine[b].reshape(-1), flat, (wxy * h2[b][:, None, None]).astype(T).ravel())
        Gf = np.fft.rfft2(fine, axes=(-2, -1))                               # (b, 2 Nx, Ny + 1)

        def Hhat(ky, lx):                                                    # the type-1 coefficients at signed (ky, lx), any sign of ky
            neg = ky < 0
            a, b_ = np.where(neg, -ky, ky), np.where(neg, -lx, lx)
            v = Gf[:, b_ % (2 * Nx), a]
            v = np.where(neg, np.conj(v), v)
            return v * (self.dec[1][np.abs(lx)] * self.dec[0][np.abs(ky)])

        KYm, LXm = np.meshgrid(self.kym, self.lxm, indexing="xy")            # (Nx, Nyh)
        KYp, LXp = np.meshgrid(self.kyp, self.lxp, indexing="xy")
        A = (T(0.5) * (Hhat(KYm, LXm) + Hhat(KYp, LXp))).astype(Gf.dtype) * T(Ny * Nx / self.n)
        out = np.fft.irfft2(A, s=(Nx, Ny), axes=(-2, -1)).astype(T)          # divides by Ny Nx
        return out.reshape(lead + (Nx, Ny))


# ---- the projector ---------------------------------------------------------------------------------------------------------------------------
class Projector(R.Projector):
    """_healpix_ref.Projector plus the nodes of the patch and both directions, by the definition (`direct_*`) or by a Plan (`plan(...)`)"""

    def __init__(self, nside, cart):
        super().__init__(nside, cart)
        pos = np.searchsorted(self.touched, self.hpx_idxs_in_patch)
        assert np.array_equal(self.touched[pos], self.hpx_idxs_in_patch)
        self.i_in, self.j_in, self.psi_in = self.is_[pos], self.js[pos], self.psi_hpx[pos]
        self.npatch = int(pos.size)
        self._K, self._plans = None, {}

    @property
    def K(self):
        if self._K is None:
            self._K = kernel_matrix(self.cart.Ny, self.cart.Nx, self.i_in, self.j_in)
        return self._K

    def cut_margin_patch(self):
        """distance, in pixels, of the nearest HEALPix centre from the lines hpx_idxs_in_patch is cut on"""
        Ny, Nx = self.cart.Ny, self.cart.Nx
        i, j = self.i_all, self.j_all
        near = (i > 0) & (i < Ny + 1) & (j > 0) & (j < Nx + 1)
        d = [np.abs(i[near] - v) for v in (1, Ny)] + [np.abs(j[near] - v) for v in (1, Nx)]
        return min((x.min() for x in d if x.size), default=np.inf)

    def plan(self, dtype=np.float64, w=None):
        k = (np.dtype(dtype).name, w)
        if k not in self._plans:
            self._plans[k] = Plan(self.cart.Ny, self.cart.Nx, self.i_in, self.j_in, dtype, w)
        return self._plans[k]

    def _to_healpix(self, m, nodes):
        m = np.asarray(m)
        out = np.zeros(m.shape[:2] + (self.npix,), dtype=np.float64)
        out[..., self.hpx_idxs_in_patch] = R._rotate(np.asarray(nodes(m), dtype=np.float64), self.psi_in, R.rot_to_healpix)
        return out

    def _to_cart(self, h, grid):
        v = np.asarray(grid(np.asarray(h)[..., self.hpx_idxs_in_patch]), dtype=np.float64)      # (B, P, Nx, Ny)
        Nx, Ny = self.cart.Nx, self.cart.Ny
        return R._rotate(v.reshape(v.shape[0], v.shape[1], Nx * Ny), self.psi_cart, R.rot_to_cart).reshape(v.shape)

    def direct_to_healpix(self, m):
        """(B, P, Nx, Ny) -> (B, P, npix), float64, by the definition"""
        return self._to_healpix(m, lambda a: np.einsum("pxy,bkxy->bkp", self.K, np.asarray(a, dtype=np.float64)) / (self.cart.Ny * self.cart.Nx))

    def direct_to_cart(self, h):
        """(B, P, npix) -> (B, P, Nx, Ny), float64, by the definition"""
        return self._to_cart(h, lambda a: np.einsum("pxy,bkp->bkxy", self.K, np.asarray(a, dtype=np.float64)) / self.npatch)

    def window_to_healpix(self, m, dtype=np.float64, w=None):
        return self._to_healpix(m, self.plan(dtype, w).to_nodes)

    def window_to_cart(self, h, dtype=np.float64, w=None):
        return self._to_cart(h, self.plan(dtype, w).to_grid)


# ---- the cases the budget and the device test share -----------------------------------------------------------------------------------------
EQ_SPANS = ((0.9, 1.7), (-0.5, 0.6))            # the spans of the existing HEALPix test
# name: (Nside, Ny, Nx, theta_pix or None for ProjEquiRect, rotator)
CASES = {
    "n16_base": (16, 24, 32, 120.0, (0, 90, 0)),
    "n32_mixed": (32, 30, 44, 60.0, (40, -20, 10)),
    "n8_wrap": (8, 8, 12, 240.0, (0, 30, 0)),
    "n16_equirect": (16, 24, 32, None, None),
    "n32_pow2": (32, 32, 64, 60.0, (0, 90, 0)),      # powers of two >= 32: both contexts run the fused transforms, not the any-size path
}
_proj = {}


def projector(case):
    """the restatement's projector of a case: computed once, shared, never modified"""
    if case not in _proj:
        nside, Ny, Nx, theta, rot = CASES[case]
        with np.errstate(all="ignore"):                                      # a HEALPix centre at the patch's antipode maps to infinity
            _proj[case] = Projector(nside, R.EquiRect(Ny, Nx, *EQ_SPANS) if theta is None else R.Lambert(Ny, Nx, theta, rot))
    return _proj[case]


def rel_planes(got, want):
    """relative L2 error of each of the P planes of (B, P, ...) arrays, over the batch"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    P = want.shape[1]
    d = np.moveaxis(got - want, 1, 0).reshape(P, -1)
    return np.linalg.norm(d, axis=1) / np.linalg.norm(np.moveaxis(want, 1, 0).reshape(P, -1), axis=1)
