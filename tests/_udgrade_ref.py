"""float64 NumPy restatement of the reference's `ud_grade` (src/proj_lambert.jl:533-592) and `pixwin` (:194-200), for the tests of
cmbl_ud_grade.  Independent of the engine: nothing here imports the package.

Array layouts are the engine's host layouts: map (..., Nx, Ny) real == Julia (Ny, Nx, ...); Fourier (..., Nx, Ny//2+1) complex, the
unnormalised rfft over both axes (src/util_fft.jl:20-25).  Leading axes (pol, batch) are carried along: every step acts per plane."""
import numpy as np


def rfft2(m):                                            # m_rfft (src/util_fft.jl:20)
    return np.fft.rfft2(m, axes=(-2, -1))


def irfft2(F, Ny):                                       # m_irfft (src/util_fft.jl:25): x first, then c2r along y
    return np.fft.irfft2(F, s=(F.shape[-2], Ny), axes=(-2, -1))


def kfreq(N):
    """integer frequency of every index of a full axis, 0 ... ⌈N/2⌉-1 then -⌊N/2⌋ ... -1 (src/proj_lambert.jl:58-60)"""
    i = np.arange(N)
    return np.where(i < (N + 1) // 2, i, i - N)


def pixwin(theta_pix, ell):
    """:200  the window of square pixels of width θpix at ℓ: the normalised sinc (sin(πx)/(πx), Julia's and NumPy's `sinc`) of ℓ Δx / 2π"""
    return np.sinc(np.asarray(ell, dtype=np.float64) * np.deg2rad(theta_pix / 60) / (2 * np.pi))


def ells(Ny, Nx, theta_pix):
    """(ℓy of the half plane [Ny//2+1], ℓx [Nx]) of a grid (src/proj_lambert.jl:58-62)"""
    dx = np.deg2rad(theta_pix / 60)
    return kfreq(Ny)[:Ny // 2 + 1] * 2 * np.pi / (Ny * dx), kfreq(Nx) * 2 * np.pi / (Nx * dx)


def pixwin_plane(Ny, Nx, theta_pix):
    """pixwin(θ, ℓy) * pixwin(θ, ℓx)' on the half plane, (Nx, Ny//2+1)"""
    ly, lx = ells(Ny, Nx, theta_pix)
    return pixwin(theta_pix, lx)[:, None] * pixwin(theta_pix, ly)[None, :]


def pwf(Ny_new, Nx_new, theta_new, theta):
    """:552  PWF: the separable window of the new pixels over that of the old pixels, both at the ℓ of the NEW grid"""
    ly, lx = ells(Ny_new, Nx_new, theta_new)
    return (pixwin(theta_new, lx)[:, None] * pixwin(theta_new, ly)[None, :]) / (pixwin(theta, lx)[:, None] * pixwin(theta, ly)[None, :])


def nan2zero(x):                                         # src/util.jl:32
    return np.where(np.isfinite(x), x, 0)


def geometry(Ny, Nx, theta, theta_new):
    """:545-548  (downgrade?, fac, Ny_new, Nx_new); ValueError unless the step is an integer"""
    down = theta_new > theta
    ratio = theta_new / theta if down else theta / theta_new
    fac = int(round(ratio))
    if fac < 2 or abs(ratio - fac) > 1e-6 * ratio:
        raise ValueError("Can only ud_grade in integer steps")          # :546
    if down:
        if Ny % fac or Nx % fac:
            raise ValueError("Can only ud_grade in integer steps")      # the reshape of :561 fails
        return True, fac, Ny // fac, Nx // fac
    return False, fac, Ny * fac, Nx * fac


def antialias_mask(Ny, Nx, Ny_new, Nx_new):
    """:557  keep = !(|ℓy| >= nyquist_new || |ℓx| >= nyquist_new) on the SOURCE half plane (Nx, Ny//2+1), decided by integer index:
    |ℓ| >= nyquist_new  <=>  |k| 2π/(N Δx) >= π/(fac Δx)  <=>  2|k| >= N_new"""
    ky, kx = kfreq(Ny)[:Ny // 2 + 1], kfreq(Nx)
    return ~((2 * np.abs(kx)[:, None] >= Nx_new) | (2 * np.abs(ky)[None, :] >= Ny_new))


def block_mean(m, fac):
    """:561  the map reshaped to (fac, Ny_new, fac, Nx_new) blocks and averaged over the two block axes"""
    Nx, Ny = m.shape[-2:]
    return m.reshape(m.shape[:-2] + (Nx // fac, fac, Ny // fac, fac)).mean(axis=(-3, -1))


def truncate(F, Ny_new, Nx_new):
    """:566  rows ky = 0 ... Ny_new÷2; columns: the first ⌈Nx_new/2⌉ (kx >= 0) and the last ⌊Nx_new/2⌋ (kx < 0) of the source"""
    Nx = F.shape[-2]
    cols = list(range(Nx_new // 2 + 1 if Nx_new % 2 else Nx_new // 2)) + list(range(Nx - Nx_new // 2, Nx))
    return F[..., cols, :Ny_new // 2 + 1]


def replicate(m, fac):
    """:575-580  every pixel fac x fac times"""
    return np.repeat(np.repeat(m, fac, axis=-1), fac, axis=-2)


def ud_grade(arr, basis, Ny, Nx, theta, theta_new, mode="map", deconv_pixwin=None, anti_aliasing=None):
    """The reference's sequence, literally.  `basis` "map" | "fourier" says what `arr` is.  Returns (array, basis, Ny_new, Nx_new) in the
    basis the reference returns: map for map mode without deconvolution, Fourier otherwise."""
    arr = np.asarray(arr, dtype=np.complex128 if basis == "fourier" else np.float64)
    if theta_new == theta:                                               # :542
        return arr, basis, Ny, Nx
    if mode not in ("map", "fourier"):                                   # :543
        raise ValueError("mode must be map or fourier")
    deconv_pixwin = (mode == "map") if deconv_pixwin is None else deconv_pixwin      # :537-538
    anti_aliasing = (mode == "map") if anti_aliasing is None else anti_aliasing
    down, fac, Ny_new, Nx_new = geometry(Ny, Nx, theta, theta_new)
    as_map = lambda a, b: a if b == "map" else irfft2(a, Ny)
    as_fourier = lambda a, b: a if b == "fourier" else rfft2(a)
    if down:                                                             # :554
        if anti_aliasing:                                                # :556-558  a 0/1 Fourier-diagonal operator applied to f
            arr, basis = as_fourier(arr, basis) * antialias_mask(Ny, Nx, Ny_new, Nx_new), "fourier"
        if mode == "map":                                                # :559-563
            new, nb = block_mean(as_map(arr, basis), fac), "map"
        else:                                                            # :564-568
            new, nb = truncate(as_fourier(arr, basis), Ny_new, Nx_new), "fourier"
        if deconv_pixwin:                                                # :570-572  the diagonal operator PWF divided out in Fourier space, NaN -> 0 (src/specialops.jl:10)
            new = rfft2(new) if nb == "map" else new
            new, nb = nan2zero(new / pwf(Ny_new, Nx_new, theta_new, theta)), "fourier"
        return new, nb, Ny_new, Nx_new
    if mode == "map":                                                    # :575-583
        new = replicate(as_map(arr, basis), fac)
        if deconv_pixwin:
            raise ValueError("Not implemented")                          # :582
        return new, "map", Ny_new, Nx_new
    raise ValueError("Not implemented")                                  # :585


def block_sum_factor(N, N_new, fac):
    """D(k) = Σ_{a<fac} exp(2πi k a / N) at the frequencies of every index of an N_new-point axis"""
    k = kfreq(N_new)
    return np.exp(2j * np.pi * np.outer(k, np.arange(fac)) / N).sum(axis=1)


def ud_grade_fused(F, Ny, Nx, theta, theta_new, deconv_pixwin=True):
    """The default downgrade (map mode, anti-aliasing) as ONE Fourier-space step on the rfft `F` of the field: after anti-aliasing no two
    surviving frequencies alias onto one another, so the rfft of the block mean is F_new[k] = F[k] D_y(ky) D_x(kx) / fac^4.  Returns the
    Fourier array on the new grid."""
    down, fac, Ny_new, Nx_new = geometry(Ny, Nx, theta, theta_new)
    assert down
    new = truncate(np.asarray(F, dtype=np.complex128) * antialias_mask(Ny, Nx, Ny_new, Nx_new), Ny_new, Nx_new)
    Dy, Dx = block_sum_factor(Ny, Ny_new, fac)[:Ny_new // 2 + 1], block_sum_factor(Nx, Nx_new, fac)
    new = new * (Dx[:, None] * Dy[None, :]) / fac ** 4
    return nan2zero(new / pwf(Ny_new, Nx_new, theta_new, theta)) if deconv_pixwin else new
