"""float64 restatement of the reference's make_mask (src/masking.jl:1-67) with SciPy, independent of the engine: what tests/test_gpu_mask.py
compares cmbl_edt_sq and cmbl_make_mask with, pinned on its own by tests/test_mask_ref.py.

Arrays have the layout of a map plane, [x, y] (shape (Nx, Ny)): the memory order of the reference's (Ny, Nx) column-major arrays.  Widths are in
pixels; `deg2npix` / `arcmin2npix` are the reference's conversions.  ImageMorphology's feature_transform + norm is
scipy.ndimage.distance_transform_edt (exact: d^2 is taken as rint(d * d)); ImageFiltering's imfilter(d, Kernel.gaussian(s)) is the separable
correlation with 4 ceil(s) + 1 taps exp(-x^2 / 2 s^2) per axis, normalised to sum 1, border "replicate" (scipy's mode="nearest")."""
import math

import numpy as np
from scipy import ndimage


def deg2npix(x, theta_pix):
    return int(round(x / theta_pix * 60))                        # round(Int, x/θpix*60), half to even like Julia's (:11)


def arcmin2npix(x, theta_pix):
    return int(round(x / theta_pix))                             # :12


def default_num_ptsrcs(Ny, Nx, theta_pix):
    return int(round(Ny * Nx * (theta_pix / 60) ** 2 * 120 / 100))   # :8


def gaussian_taps(sigma):
    """KernelFactors.gaussian(σ, 4⌈σ⌉+1)"""
    w = 2 * math.ceil(sigma)
    x = np.arange(-w, w + 1, dtype=np.float64)
    g = np.exp(-x ** 2 / (2.0 * sigma ** 2))
    return g / g.sum()


def boundarymask(Ny, Nx, pad):
    m = np.ones((Nx, Ny), dtype=bool)                            # :31-38
    if pad > 0:
        m[:pad, :] = False
        m[:, :pad] = False
        m[Nx - pad:, :] = False
        m[:, Ny - pad:] = False
    return m


def distance(feat):
    """Euclidean distance (float64) of every pixel to the nearest True pixel of `feat`"""
    feat = np.asarray(feat, dtype=bool)
    if not feat.any():
        raise ValueError("no feature")
    return ndimage.distance_transform_edt(~feat)


def edt_sq(feat):
    d = distance(feat)
    return np.rint(d * d).astype(np.int64)


def edt_sq_brute(feat):
    feat = np.asarray(feat, dtype=bool)
    fx, fy = np.nonzero(feat)
    x, y = np.indices(feat.shape)
    return ((x[..., None] - fx) ** 2 + (y[..., None] - fy) ** 2).min(axis=-1)


def bleed(img, w):
    return edt_sq(img) < w * w                                   # norm(nearest - [i, j]) < w (:43), exact on integers


def cos_apod(img, w, smooth=0):
    d = distance(~np.asarray(img, dtype=bool))                   # to the nearest FALSE pixel of img (:48-49)
    if smooth:                                                   # `smooth_distance != false`: 0 means no filter (:50)
        taps = gaussian_taps(smooth)
        d = ndimage.correlate1d(ndimage.correlate1d(d, taps, axis=0, mode="nearest"), taps, axis=1, mode="nearest")
    return (1 - np.cos(np.minimum(d, w) / w * np.pi)) / 2        # :53


def sim_ptsrcs(Ny, Nx, src_yx):
    m = np.zeros((Nx, Ny), dtype=bool)
    for y, x in np.asarray(src_yx, dtype=np.int64).reshape(-1, 2):
        m[x, y] = True
    return m


def make_mask(Ny, Nx, src_yx, pad, apod_w, round_w, src_w):
    """:14-23 in pixel units, `src_yx`: (n, 2) 0-based (y, x) positions.  float32 (Nx, Ny)"""
    nsrc = len(np.asarray(src_yx).reshape(-1, 2))
    boundary = boundarymask(Ny, Nx, pad)
    ptsrc = ~bleed(sim_ptsrcs(Ny, Nx, src_yx), src_w) if nsrc else None
    if apod_w == 0:
        m = boundary if ptsrc is None else boundary & ptsrc
    else:
        m = cos_apod(boundary, apod_w, round_w)
        if ptsrc is not None:
            m = m * cos_apod(ptsrc, src_w)
    return np.asarray(m, dtype=np.float64).astype(np.float32)


def make_mask_deg(Ny, Nx, theta_pix, src_yx, edge_padding_deg=2, edge_rounding_deg=1, apodization_deg=1, ptsrc_radius_arcmin=7):
    apod_w = 0 if apodization_deg in (False, 0) else deg2npix(apodization_deg, theta_pix)
    return make_mask(Ny, Nx, src_yx, deg2npix(edge_padding_deg, theta_pix), apod_w, deg2npix(edge_rounding_deg, theta_pix),
                     arcmin2npix(ptsrc_radius_arcmin, theta_pix))


# ---- the cases of tests/test_gpu_mask.py: (Ny, Nx, pad, apod_w, round_w, src_w, nsrc), sources from a fixed NumPy seed
MASK_CASES = [(64, 128, 8, 6, 4, 3, 12), (90, 50, 5, 7, 3, 2, 9), (45, 75, 4, 5, 0, 3, 6), (32, 32, 3, 4, 10, 2, 3), (128, 128, 40, 20, 20, 2, 49)]


def case_sources(Ny, Nx, n, seed=1234):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, Ny, n), rng.integers(0, Nx, n)], axis=1).astype(np.int32)
