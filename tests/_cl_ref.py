"""float64 NumPy restatement of the reference's `get_Cℓ` (src/proj_lambert.jl:470-503), `get_ρℓ` (src/cls.jl:88-97) and `cov_to_Cℓ`
(src/proj_lambert.jl:415-419), for the tests of cmbl_clbins_* / cmbl_get_cl.  Independent of the engine: nothing here imports the package.

Array layouts are the engine's host layouts: a Fourier half plane is (..., Nx, Ny//2+1) complex == Julia (Ny÷2+1, Nx, ...), the unnormalised
rfft over both axes; a full plane is (..., Nx, Ny).  Two routes to the five binned sums:
  sums_full   the reference as written: `unfold` to the full plane (src/util_fft.jl:83-97), strict mask, left-closed histogram
  sums_half   the λ-weighted half-plane sum the engine computes (λ = 1 on ky = 0 and on the Nyquist row of an even Ny, 2 elsewhere)
tests/test_cl_ref.py shows them equal.  Empty bins come out as NaN (0/0), which the reference's `Cℓs` constructor drops (src/cls.jl:18-23)."""
import numpy as np


def kfreq(N):
    i = np.arange(N)
    return np.where(i < (N + 1) // 2, i, i - N)


def alpha(Ny, Nx, theta_pix):
    """:473  α = Nx·Ny/Δx²"""
    return Nx * Ny / np.deg2rad(theta_pix / 60) ** 2


def lmag(Ny, Nx, theta_pix):
    """ℓmag on the half plane, (Nx, Ny//2+1) (src/proj_lambert.jl:58-66)"""
    dx = np.deg2rad(theta_pix / 60)
    ly, lx = kfreq(Ny)[:Ny // 2 + 1] * 2 * np.pi / (Ny * dx), kfreq(Nx) * 2 * np.pi / (Nx * dx)
    return np.sqrt(lx[:, None] ** 2 + ly[None, :] ** 2)


def lam(Ny):
    """λ_rfft (src/util_fft.jl:137-143): how many full-plane modes a half-plane row stands for"""
    l = np.full(Ny // 2 + 1, 2.0)
    l[0] = 1
    if Ny % 2 == 0:
        l[-1] = 1
    return l


def unfold(Tl, Ny):
    """src/util_fft.jl:83-97 for an even Nx: rows ky = 1 ... ⌈Ny/2⌉-1 mirrored, Tlu[-k] = conj(Tl[k]).  (For an odd Nx the reference's `n2 = n+3`
    indexes one past the row under @inbounds; only the Hermitian mirror it intends is defined, and that is what this returns for any Nx.)"""
    Tl = np.asarray(Tl)
    Nx, m = Tl.shape[-2], Tl.shape[-1]
    assert m == Ny // 2 + 1
    out = np.empty(Tl.shape[:-1] + (Ny,), dtype=Tl.dtype)
    out[..., :m] = Tl
    xm = (Nx - np.arange(Nx)) % Nx
    for y in range(m, Ny):
        out[..., y] = np.conj(Tl[..., xm, Ny - y])
    return out


def nan2zero(x):                                         # src/util.jl:32
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isfinite(x), x, 0.0)


def weight(L, Clfid=None):
    """:482  w = nan2zero((2 Cℓfid(L)² / (2L+1))⁻¹); Cℓfid = None is the default ℓ -> 1"""
    L = np.asarray(L, dtype=np.float64)
    if Clfid is None:
        return (2 * L + 1) / 2
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return nan2zero(1.0 / (2 * np.asarray(Clfid(L), dtype=np.float64) ** 2 / (2 * L + 1)))


def _hist(L, x, ledges):
    """fit(Histogram, L, Weights(x), ℓedges) (:484): left-closed bins [e_i, e_i+1)"""
    b = np.searchsorted(ledges, L, side="right") - 1
    return np.bincount(b, weights=x, minlength=len(ledges) - 1)[:len(ledges) - 1].astype(np.float64)


def sums_full(F1, F2, L_half, w_half, Ny, al, ledges):
    """the literal route: (A, S1, Sℓ, count, S2), each [nbins], for ONE pair of half planes (Nx, Ny//2+1)"""
    ledges = np.asarray(ledges, dtype=np.float64)
    L, w = unfold(L_half, Ny), unfold(w_half, Ny)
    mask = (L > ledges.min()) & (L < ledges.max())       # :476
    CL = (np.conj(unfold(F1, Ny)) * unfold(F2, Ny)).real[mask] / al
    L, w = L[mask], w[mask]
    return _hist(L, w, ledges), _hist(L, w * CL, ledges), _hist(L, w * L, ledges), _hist(L, np.ones_like(w), ledges), _hist(L, w * CL ** 2, ledges)


def sums_half(F1, F2, L_half, w_half, Ny, al, ledges):
    """the λ-weighted half-plane route"""
    ledges = np.asarray(ledges, dtype=np.float64)
    l = np.broadcast_to(lam(Ny)[None, :], L_half.shape)
    mask = (L_half > ledges.min()) & (L_half < ledges.max())
    CL = (np.conj(F1) * F2).real[mask] / al
    L, w, l = L_half[mask], w_half[mask], l[mask]
    return _hist(L, l * w, ledges), _hist(L, l * w * CL, ledges), _hist(L, l * w * L, ledges), _hist(L, l, ledges), _hist(L, l * w * CL ** 2, ledges)


def default_edges(dl=50):
    return np.arange(0, 16000 + 1, dl, dtype=np.float64)    # 0:Δℓ:16000


def get_cl(F1, F2, L_half, Ny, theta_pix, ledges=None, Clfid=None, w_half=None, route=sums_half):
    """get_Cℓ for one pair of half planes.  `L_half`: the ℓmag the bins are decided on (lmag(...) here, or the context's own numbers).
    Returns a dict: A, Sl, count, S1, S2 (the sums), ell = Sℓ/A, cl = S1/A, s2 = S2/A, and sigma = sqrt((S2/A − (S1/A)²)/N), N = count/2 --
    the evident intent of :498, which as written subtracts the UN-normalised S1² (negative for any populated bin with A > 1)."""
    F1, F2 = np.asarray(F1, dtype=np.complex128), np.asarray(F1 if F2 is None else F2, dtype=np.complex128)
    Nx = F1.shape[-2]
    ledges = default_edges() if ledges is None else np.asarray(ledges, dtype=np.float64)
    w = weight(L_half, Clfid) if w_half is None else np.asarray(w_half, dtype=np.float64)
    A, S1, Sl, cnt, S2 = route(F1, F2, np.asarray(L_half, dtype=np.float64), w, Ny, alpha(Ny, Nx, theta_pix), ledges)
    with np.errstate(divide="ignore", invalid="ignore"):
        ell, cl, s2 = Sl / A, S1 / A, S2 / A
        sigma = np.sqrt(np.maximum(s2 - cl ** 2, 0) / (cnt / 2))
    return dict(A=A, Sl=Sl, count=cnt, S1=S1, S2=S2, ell=ell, cl=cl, s2=s2, sigma=sigma)


def get_rhol(F1, F2, L_half, Ny, theta_pix, **kw):
    """src/cls.jl:92-97"""
    c1, c2, cx = (get_cl(a, b, L_half, Ny, theta_pix, **kw) for a, b in ((F1, None), (F2, None), (F1, F2)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return c1["ell"], cx["cl"] / np.sqrt(c1["cl"] * c2["cl"])


def cov_to_cl(diag_half, L_half, Ny, theta_pix, **kw):
    """:415-419, literally: get_Cℓ(sqrt.(diag(C))) * sqrt(α)"""
    r = get_cl(np.sqrt(np.asarray(diag_half, dtype=np.float64)), None, L_half, Ny, theta_pix, **kw)
    return r["ell"], r["cl"] * np.sqrt(alpha(Ny, np.asarray(diag_half).shape[-2], theta_pix))

