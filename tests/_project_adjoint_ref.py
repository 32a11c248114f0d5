"""Float64 NumPy restatement of the transposes (pullbacks) of the HEALPix projection, written from their formulas on top of
tests/_healpix_ref.py (geometry, tables, rotations) and tests/_nfft_ref.py (K, the window algorithm).  tests/test_project_adjoint_ref.py pins
it against the forward restatements.

With c, s = cos 2ψ, sin 2ψ at the pixel named, Rc: Q' = Qc - Us, U' = Uc + Qs (src/proj_healpix.jl:243-244, `R.rot_to_cart`) and
Rh: Q' = Qc + Us, U' = Uc - Qs (:332-333, `R.rot_to_healpix`) act on the last two planes when npol >= 2; Rcᵀ has the form of Rh and Rhᵀ that
of Rc, each at its own ψ.

    (1) bilinear to_cartᵀ      h̄[p] = Σ_{(c,k): pix[c][k] = p} w[c][k] (Rc(ψ_c)ᵀ m̄[c])                    0 where no Cartesian pixel reads
    (2) bilinear to_healpixᵀ   m̄[c] = Σ_{(t,k): c_tk = c} v[t][k] (Rh(ψ_t)ᵀ h̄[p_t])                      corners outside the map dropped
    (3) nfft to_healpixᵀ       m̄_g = 1/(Ny Nx) Σ_{p in patch} K(x_p - x_g) (Rh(ψ_p)ᵀ h̄)_p
    (4) nfft to_cartᵀ          h̄_p = 1/Npatch Σ_g K(x_g - x_p) (Rc(ψ_g)ᵀ m̄)_g   on hpx_idxs_in_patch, 0 elsewhere

HEALPix arrays are (B, P, npix), maps (B, P, Nx, Ny) (Ny fastest), like the two modules underneath.  `r` is a `_healpix_ref.Projector`
((1), (2)) or a `_nfft_ref.Projector` ((3), (4))."""
import numpy as np

import _healpix_ref as R
import _nfft_ref as N


# ---- the bilinear cases the CPU and the device tests share ---------------------------------------------------------------------------------
EQ_SPANS = ((0.9, 1.7), (-0.5, 0.6))
# name: (Nside, Ny, Nx, theta_pix or None for ProjEquiRect, rotator): the shapes of tests/test_gpu_healpix.py, and n64_coarse, where a
# Cartesian pixel of 400' collects a few hundred HEALPix corners (long rows of (2)); n64 has the long rows of (1)
BILINEAR_CASES = {
    "n1": (1, 16, 24, 400.0, (0, 90, 0)),
    "n2": (2, 16, 24, 400.0, (0, 90, 0)),
    "n4_odd": (4, 33, 20, 120.0, (40, -20, 10)),
    "n16_phi0": (16, 64, 48, 30.0, (0, 90, 0)),
    "n16_south": (16, 64, 48, 30.0, (0, 0, 0)),
    "n16_north": (16, 64, 48, 30.0, (0, 180, 0)),
    "n64": (64, 48, 64, 10.0, (0, 30, 0)),
    "n16_equirect": (16, 24, 32, None, None),
    "n64_coarse": (64, 16, 24, 400.0, (0, 90, 0)),
}
_ref = {}


def ref(case):
    """the restatement's Projector of a bilinear case: computed once, shared, never modified"""
    if case not in _ref:
        nside, Ny, Nx, theta, rot = BILINEAR_CASES[case]
        with np.errstate(all="ignore"):                                      # a HEALPix centre at the patch's antipode maps to infinity
            _ref[case] = R.Projector(nside, R.EquiRect(Ny, Nx, *EQ_SPANS) if theta is None else R.Lambert(Ny, Nx, theta, rot))
    return _ref[case]


# ---- the tables, restated --------------------------------------------------------------------------------------------------------------
def cart_table(r):
    """(pix (4, Ny Nx) int64, w (4, Ny Nx)) of the Cartesian pixels: what (1) transposes"""
    if not hasattr(r, "_adj_cart"):
        r._adj_cart = R.interp_weights(r.nside, r.thetas, r.phis)
    return r._adj_cart


def flat_corners(r):
    """the four corners of every touched pixel as `R.flat_bilinear` has them: (flat map index (4, n_touched), weight (4, n_touched),
    inside (4, n_touched) bool); flat index = (x - 1) Ny + (y - 1)"""
    if not hasattr(r, "_adj_hpx"):
        Ny, Nx = r.cart.Ny, r.cart.Nx
        i, j = r.is_, r.js
        fi, fj, ci, cj = np.floor(i), np.floor(j), np.ceil(i), np.ceil(j)
        idx, wt, ok = [], [], []
        for y, wy in ((fi, 1 - i + fi), (ci, i - fi)):
            for x, wx in ((fj, 1 - j + fj), (cj, j - fj)):
                inside = (y >= 1) & (y <= Ny) & (x >= 1) & (x <= Nx)
                idx.append(np.where(inside, (x.astype(np.int64) - 1) * Ny + (y.astype(np.int64) - 1), 0))
                wt.append(np.where(inside, wy * wx, 0.0))
                ok.append(inside)
        r._adj_hpx = (np.stack(idx), np.stack(wt), np.stack(ok))
    return r._adj_hpx


def _scatter(out, idx, val):
    """out[..., idx] += val with repeated indices summed"""
    np.add.at(out, (slice(None), slice(None), idx), val)


# ---- (1), (2): bilinear ------------------------------------------------------------------------------------------------------------------
def to_cart_T(r, g):
    """(1): (B, P, Nx, Ny) -> (B, P, npix)"""
    g = np.asarray(g, dtype=np.float64)
    pix, w = cart_table(r)
    v = R._rotate(g.reshape(g.shape[0], g.shape[1], -1), r.psi_cart, R.rot_to_healpix)           # Rcᵀ has the form of Rh
    out = np.zeros(g.shape[:2] + (r.npix,))
    for k in range(4):
        _scatter(out, pix[k], w[k] * v)
    return out


def to_healpix_T(r, h):
    """(2): (B, P, npix) -> (B, P, Nx, Ny)"""
    h = np.asarray(h, dtype=np.float64)
    idx, wt, ok = flat_corners(r)
    v = R._rotate(h[..., r.touched], r.psi_hpx, R.rot_to_cart)                                   # Rhᵀ has the form of Rc
    out = np.zeros(h.shape[:2] + (r.cart.Nx * r.cart.Ny,))
    for k in range(4):
        _scatter(out, idx[k][ok[k]], wt[k][ok[k]] * v[..., ok[k]])
    return out.reshape(h.shape[:2] + (r.cart.Nx, r.cart.Ny))


def _abs_planes(g):
    """|g| for an I plane, |Q| + |U| in place of each pol plane: (B, P, n)"""
    a = np.abs(np.asarray(g, dtype=np.float64))
    P = a.shape[1]
    if P >= 2:
        s = a[:, P - 2] + a[:, P - 1]
        a = a.copy()
        a[:, P - 2], a[:, P - 1] = s, s
    return a


def envelope(r, g, which):
    """E(g): the I-plane transpose of (1) (`which` = "to_cart") or (2) ("to_healpix") applied to |g|, with |Q̄| + |Ū| in place of the pol
    planes -- the weights are non-negative, so |every partial sum of a row| <= E.  Returns (E shaped like the output, L, S): L the number of
    entries of every row and S the sum of its weights, over the flat output index."""
    if which == "to_cart":
        pix, w = cart_table(r)
        a = _abs_planes(np.asarray(g).reshape(g.shape[0], g.shape[1], -1))
        E, L, S = np.zeros(a.shape[:2] + (r.npix,)), np.zeros(r.npix, dtype=np.int64), np.zeros(r.npix)
        for k in range(4):
            _scatter(E, pix[k], w[k] * a)
            np.add.at(L, pix[k], 1)
            np.add.at(S, pix[k], w[k])
        return E, L, S
    idx, wt, ok = flat_corners(r)
    a = _abs_planes(np.asarray(g)[..., r.touched])
    n = r.cart.Nx * r.cart.Ny
    E, L, S = np.zeros(a.shape[:2] + (n,)), np.zeros(n, dtype=np.int64), np.zeros(n)
    for k in range(4):
        _scatter(E, idx[k][ok[k]], wt[k][ok[k]] * a[..., ok[k]])
        np.add.at(L, idx[k][ok[k]], 1)
        np.add.at(S, idx[k][ok[k]], wt[k][ok[k]])
    shape = a.shape[:2] + (r.cart.Nx, r.cart.Ny)
    return E.reshape(shape), L, S


# ---- (3), (4): nfft, by the definition --------------------------------------------------------------------------------------------------
def nfft_to_healpix_T(r, h):
    """(3): (B, P, npix) -> (B, P, Nx, Ny), float64, through K"""
    v = R._rotate(np.asarray(h, dtype=np.float64)[..., r.hpx_idxs_in_patch], r.psi_in, R.rot_to_cart)
    return np.einsum("pxy,bkp->bkxy", r.K, v) / (r.cart.Ny * r.cart.Nx)


def nfft_to_cart_T(r, g):
    """(4): (B, P, Nx, Ny) -> (B, P, npix), float64, through K"""
    g = np.asarray(g, dtype=np.float64)
    v = R._rotate(g.reshape(g.shape[0], g.shape[1], -1), r.psi_cart, R.rot_to_healpix).reshape(g.shape)
    out = np.zeros(g.shape[:2] + (r.npix,))
    out[..., r.hpx_idxs_in_patch] = np.einsum("pxy,bkxy->bkp", r.K, v) / r.npatch
    return out


# ---- (3), (4): the window algorithm in a dtype (what the budget is made of) ---------------------------------------------------------------
def _rotate_T(f, psi, rot, T):
    """the rotation with cos 2ψ, sin 2ψ and the products rounded to T"""
    P = f.shape[1]
    f = np.asarray(f, dtype=T)
    if P < 2:
        return f
    c, s = np.cos(2 * psi).astype(T), np.sin(2 * psi).astype(T)
    sign = T(1) if rot is R.rot_to_healpix else T(-1)
    Q, U = f[:, P - 2], f[:, P - 1]
    out = f.copy()
    out[:, P - 2], out[:, P - 1] = (Q * c + sign * U * s).astype(T), (U * c - sign * Q * s).astype(T)
    return out


def window_to_healpix_T(r, h, dtype=np.float64, w=None):
    """(3) through `_nfft_ref.Plan.to_grid` (the type-1 transform, 1/Npatch inside) rescaled to 1/(Ny Nx)"""
    T = np.dtype(dtype).type
    v = _rotate_T(np.asarray(h)[..., r.hpx_idxs_in_patch], r.psi_in, R.rot_to_cart, T)
    return np.asarray(r.plan(dtype, w).to_grid(v), dtype=np.float64) * (r.npatch / (r.cart.Ny * r.cart.Nx))


def window_to_cart_T(r, g, dtype=np.float64, w=None):
    """(4) through `_nfft_ref.Plan.to_nodes` (the type-2 transform, 1/(Ny Nx) inside) rescaled to 1/Npatch"""
    T = np.dtype(dtype).type
    g = np.asarray(g)
    v = _rotate_T(g.reshape(g.shape[0], g.shape[1], -1), r.psi_cart, R.rot_to_healpix, T).reshape(g.shape)
    out = np.zeros(g.shape[:2] + (r.npix,))
    out[..., r.hpx_idxs_in_patch] = np.asarray(r.plan(dtype, w).to_nodes(v), dtype=np.float64) * (r.cart.Ny * r.cart.Nx / r.npatch)
    return out


def identity_mismatch(Ax, y, x, ATy):
    """|<A x, y> - <x, Aᵀ y>| / (|A x| |y|), dots in float64"""
    Ax, y, x, ATy = (np.asarray(a, dtype=np.float64).ravel() for a in (Ax, y, x, ATy))
    return float(abs(np.dot(Ax, y) - np.dot(x, ATy)) / (np.linalg.norm(Ax) * np.linalg.norm(y)))
