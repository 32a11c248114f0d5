"""cmbl_edt_sq and cmbl_make_mask on the device against tests/_mask_ref.py, the SciPy restatement of the reference's make_mask (src/masking.jl;
pinned on its own by tests/test_mask_ref.py), in both context precisions.  Every shape has at most 1e5 pixels.

cmbl_edt_sq is compared bit for bit (integers).  Shapes (Ny x Nx): 64 x 128 and 128 x 64 (an axis mix-up shows), 90 x 50 and 45 x 75 (odd, no
power of two), 320 x 288 with one feature in a corner (d2 > 65535, distances > 255: narrow integer types), 4096 x 16 and 16 x 4096 with three
features (the line buffers and the scans at the largest side, 16 elements per thread), a full plane, features on one edge only, an empty plane.

cmbl_make_mask, tolerance DERIVED, not measured: both sides round a double in [0, 1] to float32; the doubles differ by ~1e-13 (order of the
filter's sum, last bits of cos), which can only move that rounding by one step, so max |difference| <= 2 float32 ulps at 1.0 = 2^-22 = 2.4e-7.  The
boolean path (apod_w = 0) is exactly equal.  In a float64 context every value must besides be a float32 number.  Measured on MI355X:
profiles/make_mask_parity.txt (CMBL_PARITY_LOG)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _mask_ref as R
import _tol

DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
TOL = 2.0 * 2.0 ** -23                          # 2 float32 ulps at 1.0
ERR_ARG = 1
NOSRC = np.zeros((0, 2), dtype=np.int32)


def _pkg():
    import cmblensing_jl_amd as C
    return C


_projs = {}


def proj(Ny, Nx, prec, theta=3.0):
    k = (Ny, Nx, prec, theta)
    if k not in _projs:
        _projs[k] = _pkg().ProjLambert(Ny, Nx, theta, DT[prec][0])
    return _projs[k]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


# ---- cmbl_edt_sq ---------------------------------------------------------------------------------------------------------------------
def _random(Ny, Nx, seed):
    return np.random.default_rng(seed).random((Nx, Ny)) < 0.01


def _points(Ny, Nx, pts):
    f = np.zeros((Nx, Ny), dtype=bool)
    for y, x in pts:
        f[x, y] = True
    return f


def _edge(Ny, Nx, which):
    f = np.zeros((Nx, Ny), dtype=bool)
    if which == "x0":
        f[0, :] = True
    elif which == "y1":
        f[:, Ny - 1] = True
    return f


EDT_CASES = {
    "64x128": lambda: _random(64, 128, 1),
    "128x64": lambda: _random(128, 64, 2),
    "90x50": lambda: _random(90, 50, 3),
    "45x75": lambda: _random(45, 75, 4),
    "320x288 corner": lambda: _points(320, 288, [(319, 287)]),
    "4096x16": lambda: _points(4096, 16, [(0, 3), (2500, 15), (4095, 0)]),
    "16x4096": lambda: _points(16, 4096, [(3, 0), (15, 2500), (0, 4095)]),
    "45x75 full": lambda: np.ones((75, 45), dtype=bool),
    "90x50 edge x=0": lambda: _edge(90, 50, "x0"),
    "90x50 edge y=Ny-1": lambda: _edge(90, 50, "y1"),
    "2x2": lambda: _points(2, 2, [(1, 0)]),
}
_edt_want = {}


def edt_want(case):
    if case not in _edt_want:
        _edt_want[case] = R.edt_sq(EDT_CASES[case]())
    return _edt_want[case]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", list(EDT_CASES))
def test_edt_sq_is_exact(case, prec):
    feat = EDT_CASES[case]()
    Nx, Ny = feat.shape
    got = _pkg().engine.edt_sq(proj(Ny, Nx, prec), feat)
    assert got.dtype == torch.int32 and tuple(got.shape) == (Nx, Ny)
    got, want = got.cpu().numpy().astype(np.int64), edt_want(case)
    print(f"edt_sq {case} {prec}: max d2 {want.max()}, mismatches {int((got != want).sum())}")
    if case == "320x288 corner":
        assert want.max() == 319 ** 2 + 287 ** 2 > 65535
    assert np.array_equal(got, want)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_edt_sq_of_an_empty_plane_is_an_argument_error(prec):
    C = _pkg()
    p = proj(45, 75, prec)
    feat = torch.zeros((75, 45), dtype=torch.uint8, device=p.device)
    out = torch.empty((75, 45), dtype=torch.int32, device=p.device)
    assert p.lib.cmbl_edt_sq(p._h, ptr(feat), ptr(out)) == ERR_ARG and b"no feature" in p.lib.cmbl_last_error()
    with pytest.raises(ValueError):
        C.engine.edt_sq(p, np.zeros((75, 45)))
    feat[7, 3] = 1                                                        # a valid call afterwards succeeds
    assert p.lib.cmbl_edt_sq(p._h, ptr(feat), ptr(out)) == 0
    assert np.array_equal(out.cpu().numpy(), R.edt_sq(feat.cpu().numpy()))


# ---- cmbl_make_mask ------------------------------------------------------------------------------------------------------------------
def make_mask_rc(p, yx, pad, apod_w, round_w, src_w, out=None):
    yx = np.ascontiguousarray(yx, dtype=np.int32).reshape(-1, 2)
    out = p.empty(0, 1, 1) if out is None else out
    rc = p.lib.cmbl_make_mask(p._h, yx.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if len(yx) else None, len(yx), pad, apod_w, round_w, src_w, ptr(out))
    return rc, out


def make_mask(p, yx, pad, apod_w, round_w, src_w):
    rc, out = make_mask_rc(p, yx, pad, apod_w, round_w, src_w)
    assert rc == 0, p.lib.cmbl_last_error()
    return out[0, 0].cpu().numpy()


def compare(what, got, want, prec, exact=False):
    """`got`: the engine's plane in the context's precision, `want`: the restatement's float32 plane"""
    assert got.dtype == DT[prec][1] and got.shape == want.shape
    assert np.array_equal(got.astype(np.float32).astype(got.dtype), got)           # float32 numbers whatever the precision
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    frac = float(np.mean((want > 0) & (want < 1)))
    tol = 0.0 if exact else TOL
    print(f"make_mask {what} {prec}: max |diff| {err:.3e} (tolerance {tol:.3e}), {int((got != want).sum())} of {want.size} differ, fraction in (0, 1) {frac:.2f}")
    _tol._record(_tol._key(what), err, tol)
    assert err <= tol
    assert got.min() >= 0 and got.max() <= 1


_mask_want = {}


def mask_want(Ny, Nx, yx, pad, apod_w, round_w, src_w):
    k = (Ny, Nx, np.asarray(yx).tobytes(), pad, apod_w, round_w, src_w)
    if k not in _mask_want:
        _mask_want[k] = R.make_mask(Ny, Nx, yx, pad, apod_w, round_w, src_w)
    return _mask_want[k]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", R.MASK_CASES, ids=lambda c: "x".join(map(str, c[:2])))
def test_make_mask_parity(case, prec):
    Ny, Nx, pad, apod_w, round_w, src_w, nsrc = case
    yx = R.case_sources(Ny, Nx, nsrc)
    p = proj(Ny, Nx, prec)
    want = mask_want(Ny, Nx, yx, pad, apod_w, round_w, src_w)
    assert np.mean((want > 0) & (want < 1)) > 0.2                                  # a non-trivial mask
    compare(f"case {case}", make_mask(p, yx, pad, apod_w, round_w, src_w), want, prec)


FURTHER = {
    "no sources": (64, 128, NOSRC, 8, 6, 4, 3),
    "no sources, no filter": (45, 75, NOSRC, 4, 5, 0, 3),
    "duplicate sources": (90, 50, [[40, 20], [40, 20], [41, 20], [40, 20]], 5, 7, 3, 2),
    "corners and inside the pad": (45, 75, [[0, 0], [44, 0], [0, 74], [44, 74], [2, 30], [20, 1], [22, 37]], 4, 5, 2, 3),
    "2 pad >= Ny": (32, 64, [[5, 6]], 16, 4, 2, 2),
    "2 pad > Nx": (45, 21, NOSRC, 11, 4, 0, 2),
}


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", list(FURTHER))
def test_make_mask_further_cases(name, prec):
    Ny, Nx, yx, pad, apod_w, round_w, src_w = FURTHER[name]
    want = mask_want(Ny, Nx, np.asarray(yx, dtype=np.int32), pad, apod_w, round_w, src_w)
    got = make_mask(proj(Ny, Nx, prec), yx, pad, apod_w, round_w, src_w)
    compare(name, got, want, prec)
    if name.startswith("2 pad"):
        assert not got.any()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", R.MASK_CASES[:3] + [(32, 64, 16, 0, 0, 2, 1), (45, 75, 4, 0, 0, 3, 0)], ids=lambda c: "x".join(map(str, c[:2])) + f"n{c[6]}")
def test_make_mask_boolean_path_is_exact(case, prec):
    Ny, Nx, pad, _, round_w, src_w, nsrc = case
    yx = R.case_sources(Ny, Nx, nsrc)
    got = make_mask(proj(Ny, Nx, prec), yx, pad, 0, round_w, src_w)
    compare(f"boolean {case}", got, mask_want(Ny, Nx, yx, pad, 0, round_w, src_w), prec, exact=True)
    assert set(np.unique(got)) <= {0.0, 1.0}


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_make_mask_is_deterministic(prec):
    Ny, Nx, pad, apod_w, round_w, src_w, nsrc = R.MASK_CASES[0]
    yx = R.case_sources(Ny, Nx, nsrc)
    p = proj(Ny, Nx, prec)
    a, b = make_mask(p, yx, pad, apod_w, round_w, src_w), make_mask(p, yx, pad, apod_w, round_w, src_w)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_make_mask_argument_errors(prec):
    Ny, Nx = 45, 75
    p = proj(Ny, Nx, prec)
    src = [[3, 4]]
    out = p.empty(0, 1, 1)
    bad = {
        "apodisation without padding": (NOSRC, 0, 5, 0, 0),
        "sources without a radius": (src, 4, 5, 0, 0),
        "sources without a radius, boolean": (src, 4, 0, 0, 0),
        "negative pad": (NOSRC, -1, 5, 0, 3),
        "negative apod_w": (NOSRC, 4, -5, 0, 3),
        "negative round_w": (NOSRC, 4, 5, -2, 3),
        "negative src_w": (src, 4, 5, 0, -3),
        "source y = Ny": ([[Ny, 0]], 4, 5, 0, 3),
        "source x = Nx": ([[0, Nx]], 4, 5, 0, 3),
        "source y < 0": ([[-1, 0]], 4, 5, 0, 3),
        "source x < 0": ([[3, 4], [0, -1]], 4, 5, 0, 3),
    }
    for what, (yx, pad, apod_w, round_w, src_w) in bad.items():
        rc, _ = make_mask_rc(p, yx, pad, apod_w, round_w, src_w, out)
        assert rc == ERR_ARG and p.lib.cmbl_last_error().startswith(b"make_mask"), what
    yx = np.asarray(src, dtype=np.int32)
    assert p.lib.cmbl_make_mask(p._h, None, 1, 4, 5, 0, 3, ptr(out)) == ERR_ARG          # nsrc > 0 without positions
    assert p.lib.cmbl_make_mask(p._h, yx.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1, 4, 5, 0, 3, None) == ERR_ARG
    compare("valid call after the errors", make_mask(p, yx, 4, 5, 0, 3), mask_want(Ny, Nx, yx, 4, 5, 0, 3), prec)


# ---- Python ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_python_make_mask(prec):
    C = _pkg()
    N, theta = 128, 3.0
    m = C.make_mask(N, theta, seed=1, T=DT[prec][0])
    assert m.basis == C.MAP and tuple(m.arr.shape) == (1, 1, N, N) and m.arr.dtype == DT[prec][0]
    n = R.default_num_ptsrcs(N, N, theta)
    assert n == 49
    yx = C.engine.draw_ptsrcs(N, N, n, seed=1)
    rng = np.random.Generator(np.random.PCG64(1))                                  # y, then x, per source
    assert [int(rng.integers(0, N)) for _ in range(4)] == [int(v) for v in yx[:2].ravel()]
    assert C.engine.mask_npix(theta) == (40, 20, 20, 2)
    want = R.make_mask_deg(N, N, theta, yx)
    compare("python defaults 128 at 3'", m.arr[0, 0].cpu().numpy(), want, prec)
    # a ProjLambert in place of (Nside, θpix); ptsrcs= overrides seed
    p = proj(90, 50, prec, theta=2.0)
    pts = np.array([[10, 12], [70, 30], [70, 30]])
    kw = dict(edge_padding_deg=0.2, edge_rounding_deg=0.1, apodization_deg=0.25, ptsrc_radius_arcmin=5)
    a = C.make_mask(p, ptsrcs=pts, seed=5, **kw)
    b = C.make_mask(p, ptsrcs=pts, seed=6, **kw)
    assert a.proj is p and torch.equal(a.arr, b.arr)
    compare("python proj, ptsrcs", a.arr[0, 0].cpu().numpy(), R.make_mask_deg(90, 50, 2.0, pts, **kw), prec)
    assert not torch.equal(C.make_mask(p, num_ptsrcs=3, seed=5, **kw).arr, C.make_mask(p, num_ptsrcs=3, seed=6, **kw).arr)
    c = C.make_mask(p, ptsrcs=pts, **{**kw, "apodization_deg": 0})                 # the boolean mask
    compare("python boolean", c.arr[0, 0].cpu().numpy(), R.make_mask_deg(90, 50, 2.0, pts, **{**kw, "apodization_deg": 0}), prec, exact=True)
    with pytest.raises(ValueError):
        C.make_mask(p, num_ptsrcs=0, **{**kw, "apodization_deg": 0.01})            # rounds to 0 pixels: 0 / 0
    with pytest.raises(ValueError):
        C.make_mask(p, num_ptsrcs=0, **{**kw, "edge_padding_deg": 0})
    with pytest.raises(ValueError):
        C.make_mask(p, ptsrcs=[[90, 0]], **kw)


def test_load_sim_with_pixel_mask_kwargs():
    C = _pkg()
    from bench import synthetic_cls
    cls = synthetic_cls()
    kw = dict(edge_padding_deg=0.5, apodization_deg=0.4, edge_rounding_deg=0.2, num_ptsrcs=5)
    common = dict(theta_pix=3.0, Nside=64, pol="P", cls=cls, Nphi="flat", seeds=(1, 2, 3))
    s = C.load_sim(pixel_mask_kwargs=kw, **common)
    ds = s["ds"]
    M = ds.host["Mpix"]
    assert M.shape == (64, 64) and M.dtype == np.float64
    yx = C.engine.draw_ptsrcs(64, 64, 5, seed=1)                                          # seed defaults to seeds[0]
    want = R.make_mask_deg(64, 64, 3.0, yx, edge_padding_deg=0.5, apodization_deg=0.4, edge_rounding_deg=0.2)
    compare("load_sim Mpix", M.astype(np.float32), want, "f32")
    assert np.array_equal(M.astype(np.float32).astype(np.float64), M)
    assert np.array_equal(ds.ops["Mpix"][0].cpu().numpy().astype(np.float64), M)
    lp = ds.logpdf(s["f"], s["phi"])
    assert np.all(np.isfinite(lp))
    # pixel_mask= alone is today's border_mask, bit for bit; both together are refused
    s2 = C.load_sim(pixel_mask=dict(pad_deg=0.5, apod_deg=0.4), **common)
    assert np.array_equal(s2["ds"].host["Mpix"], C.border_mask(s2["proj"], pad_deg=0.5, apod_deg=0.4))
    with pytest.raises(ValueError):
        C.load_sim(pixel_mask=dict(pad_deg=0.5, apod_deg=0.4), pixel_mask_kwargs=kw, **common)
