"""cmbl_clbins_* / cmbl_get_cl and the Python get_Cl family on the device against tests/_cl_ref.py, the float64 restatement of the reference's get_Cℓ
(src/proj_lambert.jl:470-513; pinned on its own by tests/test_cl_ref.py), on identical inputs: B = 2 with distinct data per slice; complex inputs are
the rfft of real maps, rounded to the working precision.  The bins are decided on the context's own ℓmag (cmbl_ctx_geometry_host(which = 5)) compared
with the double edges, by the library and by the helper alike, so the two agree mode for mode in both precisions.

Shapes: the smallest at which each layout branch can go wrong --
  64x64     fused power-of-two path (bit-reversed kx in the internal layout a MAP input is read from)
  64x128    rectangular
  96x96     any-size path with compile-time plans, natural kx, tiled scratch
  90x50     run-time plans
  45x75     odd Ny: no Nyquist row, λ = 2 to the end
Every shape runs P in {1, 2, 3} x basis in {MAP, FOURIER, HARMONIC} x auto / cross x two edge sets (the default 0:50:16000 and a non-uniform set that
holds exact ties with ℓmag values) with both moments, plus the two weight planes (Cℓfid = ℓ -> 1/ℓ², infinite at ℓ = 0; a Cls table that ends inside the
grid), in both precisions: a call is a few launches on at most 128 x 64 pixels, the whole file takes seconds.

Tolerances (relative L2 over the populated bins, tests/_tol.py): the transform class bounds of DESIGN.md §3, 1.5e-6 in single and 1e-12 in double
precision -- a MAP input carries one transform, complex inputs only the double accumulation.  NOT YET RUN on an MI355X: the errors of a first run belong in profiles/get_cl_parity.txt (CMBL_PARITY_LOG, tools/parity_report.py --collapse)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _cl_ref as R
from _tol import close

DT = {"f32": (torch.float32, np.float32, np.complex64), "f64": (torch.float64, np.float64, np.complex128)}
TOL = {"f32": 1.5e-6, "f64": 1e-12}
THETA = 2.0
B = 2
SHAPES = [(64, 64), (64, 128), (96, 96), (90, 50), (45, 75)]                 # (Ny, Nx)
MAP, FOURIER, HARMONIC = 0, 1, 2
ARG, SHAPE = 1, 2
PAIRS = {1: [(0, 0)], 2: [(0, 0), (1, 1), (0, 1)], 3: [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]}    # II | EE BB EB (QQ UU QU) | II EE BB IE IB EB
PD = ctypes.POINTER(ctypes.c_double)


def _pkg():
    import cmblensing_jl_amd as C
    return C


_projs, _inputs, _plans = {}, {}, {}


def proj(Ny, Nx, prec, theta=THETA):
    k = (Ny, Nx, prec, theta)
    if k not in _projs:
        _projs[k] = _pkg().ProjLambert(Ny, Nx, theta, DT[prec][0])
    return _projs[k]


def inputs(Ny, Nx, prec, seed=0):
    """(maps (B, 3, Nx, Ny), their rffts) rounded to the working precision: computed once per shape, never modified"""
    k = (Ny, Nx, prec, seed)
    if k not in _inputs:
        m = np.random.default_rng(Ny * 10007 + Nx + 77 * seed).standard_normal((B, 3, Nx, Ny)).astype(DT[prec][1])
        _inputs[k] = (m, np.fft.rfft2(m.astype(np.float64), axes=(-2, -1)).astype(DT[prec][2]))
    return _inputs[k]


def tie_edges(L):
    """non-uniform edges of which three ARE ℓmag values of the grid (the context's own numbers): ky = 3, 5, 9 at kx = 0"""
    e = np.array([L[0, 3], L[0, 5], 0.5 * (L[0, 5] + L[0, 9]), L[0, 9], 1.7 * L[0, 9], 4.0 * L[0, 9]])
    assert np.all(np.diff(e) > 0)
    return e


def weights(p, kind):
    if kind is None:
        return None
    L = p.lmag
    if kind == "1/l^2":
        return R.weight(L, lambda l: 1 / l ** 2)                              # infinite at ℓ = 0: w zeroed there
    table = _pkg().Cls(np.arange(2, 2001), 1e-3 / np.arange(2, 2001.0))       # ends inside the grid (ℓ up to ~7600): NaN, so w = 0, beyond 2000
    return R.weight(L, table)


class Plan:
    def __init__(self, p, ledges, w=None, nw=None):
        self.p, self.h = p, ctypes.c_void_p()
        self.ledges = np.ascontiguousarray(ledges, dtype=np.float64)
        self.w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        self.rc = p.lib.cmbl_clbins_create(p._h, self.ledges.ctypes.data_as(PD), len(self.ledges), None if w is None else self.w.ctypes.data_as(PD),
                                           (0 if w is None else self.w.size) if nw is None else nw, ctypes.byref(self.h))
        self.nbins = len(self.ledges) - 1

    def info(self, which, n=None):
        out = np.empty(self.nbins if n is None else n)
        rc = self.p.lib.cmbl_clbins_info_host(self.h, which, out.ctypes.data_as(PD), out.size)
        return rc, out

    def __del__(self):
        if self.h:
            self.p.lib.cmbl_clbins_destroy(self.h)


def plan(p, key, ledges_fn, wkind=None):
    k = (id(p), key, wkind)
    if k not in _plans:
        _plans[k] = Plan(p, ledges_fn(), weights(p, wkind))
        assert _plans[k].rc == 0, p.lib.cmbl_last_error()
    return _plans[k]


def raw(p, pl, basis, t1, t2, pairs, moments, P=None, nb=None):
    """the entry point itself: (return code, out (B, npairs, moments, nbins) on the host)"""
    nb, P = t1.shape[0] if nb is None else nb, t1.shape[1] if P is None else P
    out = torch.zeros((max(nb, 1), max(len(pairs), 1), max(moments, 1), pl.nbins), dtype=torch.float64, device=p.device)
    flat = (ctypes.c_int * max(2 * len(pairs), 2))(*[i for ab in pairs for i in ab])
    rc = p.lib.cmbl_get_cl(p._h, pl.h, basis, ctypes.c_void_p(t1.data_ptr()), None if t2 is None else ctypes.c_void_p(t2.data_ptr()), P, nb,
                           flat, len(pairs), moments, ctypes.c_void_p(out.data_ptr()))
    return rc, out


def check_against_ref(what, p, pl, got, F1, F2, pairs, prec):
    """got (B, npairs, 2, nbins) against the helper on the float64 planes F1, F2 (B, P, Nx, Nyh)"""
    got = got.cpu().numpy()
    for b in range(got.shape[0]):
        for k, (i, j) in enumerate(pairs):
            ref = R.get_cl(F1[b, i], (F1 if F2 is None else F2)[b, j], p.lmag, p.Ny, p.theta_pix, ledges=pl.ledges, w_half=pl.w)
            ok = ref["A"] > 0
            assert ok.any()
            assert not np.any(got[b, k][:, ref["count"] == 0])                   # empty bins hold 0
            close((what, "Σw·CL/A"), got[b, k, 0][ok] / ref["A"][ok], ref["cl"][ok], TOL[prec])
            close((what, "Σw·CL²/A"), got[b, k, 1][ok] / ref["A"][ok], ref["s2"][ok], TOL[prec])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx", SHAPES)
def test_plan_sums_match_the_reference(Ny, Nx, prec):
    """A, Sℓ, the counts and the set of populated bins: host double arithmetic on the same numbers"""
    p = proj(Ny, Nx, prec)
    for key, fn in (("default", R.default_edges), ("tie", lambda: tie_edges(p.lmag))):
        for wkind in (None, "1/l^2", "table"):
            pl = plan(p, key, fn, wkind)
            one = np.ones((Nx, Ny // 2 + 1))
            ref = R.get_cl(one, None, p.lmag, Ny, THETA, ledges=pl.ledges, w_half=pl.w)
            (ra, A), (rs, Sl), (rc, cnt) = pl.info(0), pl.info(1), pl.info(2)
            assert ra == rs == rc == 0
            assert np.array_equal(cnt, ref["count"]) and np.array_equal(cnt > 0, ref["count"] > 0)
            assert np.array_equal(A > 0, ref["A"] > 0)
            np.testing.assert_allclose(A, ref["A"], rtol=1e-13)
            np.testing.assert_allclose(Sl, ref["Sl"], rtol=1e-13)
            if key == "default" and wkind is None:
                assert cnt.sum() == Nx * Ny - 1                                  # every mode but ℓ = 0
            if wkind == "table" and key == "default":
                assert np.any((cnt > 0) & (A == 0))                              # bins beyond the table: populated, weightless


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx", SHAPES)
def test_binned_sums(Ny, Nx, prec):
    p = proj(Ny, Nx, prec)
    (m1, F1), (m2, F2) = inputs(Ny, Nx, prec), inputs(Ny, Nx, prec, seed=1)
    for P in (1, 2, 3):
        host = {MAP: (m1[:, :P], m2[:, :P]), FOURIER: (F1[:, :P], F2[:, :P]), HARMONIC: (F1[:, :P], F2[:, :P])}
        dev = {b: tuple(p.tensor(np.ascontiguousarray(a)) for a in ab) for b, ab in host.items() if b != HARMONIC}
        dev[HARMONIC] = dev[FOURIER]
        # what the sums are formed from, in float64: a map's exact transform; complex planes as given
        ref = {b: tuple(np.fft.rfft2(a.astype(np.float64), axes=(-2, -1)) if b == MAP else a.astype(np.complex128) for a in ab) for b, ab in host.items()}
        for key, fn in (("default", R.default_edges), ("tie", lambda: tie_edges(p.lmag))):
            pl = plan(p, key, fn)
            for basis in (MAP, FOURIER, HARMONIC):
                for cross in (False, True):
                    rc, out = raw(p, pl, basis, dev[basis][0], dev[basis][1] if cross else None, PAIRS[P], 2)
                    assert rc == 0, p.lib.cmbl_last_error()
                    check_against_ref(("get_cl", "map" if basis == MAP else "complex", key, "cross" if cross else "auto"),
                                      p, pl, out, ref[basis][0], ref[basis][1] if cross else None, PAIRS[P], prec)
                    if not cross and key == "tie" and basis == FOURIER:          # moments = 1 is the first moment of moments = 2, bit for bit
                        rc, one = raw(p, pl, basis, dev[basis][0], None, PAIRS[P], 1)
                        assert rc == 0 and torch.equal(one[:, :, 0], out[:, :, 0])
    # the weight planes, P = 2, cross
    dev2 = tuple(p.tensor(np.ascontiguousarray(a[:, :2])) for a in (F1, F2))
    for wkind in ("1/l^2", "table"):
        pl = plan(p, "tie", lambda: tie_edges(p.lmag), wkind)
        rc, out = raw(p, pl, FOURIER, dev2[0], dev2[1], PAIRS[2], 2)
        assert rc == 0, p.lib.cmbl_last_error()
        check_against_ref(("get_cl weights", "inverse square" if wkind == "1/l^2" else wkind), p, pl, out, F1[:, :2].astype(np.complex128), F2[:, :2].astype(np.complex128), PAIRS[2], prec)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx", SHAPES)
def test_delta_map_closed_form(Ny, Nx, prec):
    """f = 1 at one pixel: Cℓ = 1/α in every populated bin, and no scatter"""
    p = proj(Ny, Nx, prec)
    m = np.zeros((1, 1, Nx, Ny))
    m[0, 0, 3, 5] = 1.0
    pl = plan(p, "default", R.default_edges)
    rc, out = raw(p, pl, MAP, p.tensor(m), None, [(0, 0)], 2)
    assert rc == 0, p.lib.cmbl_last_error()
    A, al = pl.info(0)[1], R.alpha(Ny, Nx, THETA)
    ok = A > 0
    s1, s2 = (out[0, 0, i].cpu().numpy()[ok] / A[ok] for i in (0, 1))
    close("get_cl delta map", s1 * al, np.ones(ok.sum()), TOL[prec])
    assert np.all(np.abs(s2 - s1 ** 2) * al ** 2 <= 4 * TOL[prec])               # σℓ = 0 to the rounding of one transform


@pytest.mark.parametrize("Ny,Nx", [(64, 64), (90, 50)])
def test_determinism_and_batch_independence(Ny, Nx):
    p = proj(Ny, Nx, "f32")
    m, F = inputs(Ny, Nx, "f32")
    m3, F3 = (np.concatenate([a, a[:1] * 0.5 + 1], axis=0) for a in (m, F))      # B = 3
    pl = plan(p, "default", R.default_edges)
    for basis, a in ((MAP, m3), (FOURIER, F3)):
        t = p.tensor(a)
        other = p.tensor(a[::-1].copy())
        for t2 in (None, other):
            rc1, o1 = raw(p, pl, basis, t, t2, PAIRS[3], 2)
            rc2, o2 = raw(p, pl, basis, t, t2, PAIRS[3], 2)
            assert rc1 == 0 and rc2 == 0 and torch.equal(o1, o2)                 # the same call twice: bit-identical
            rc3, o3 = raw(p, pl, basis, t[:1].contiguous(), None if t2 is None else t2[:1].contiguous(), PAIRS[3], 2)
            assert rc3 == 0 and torch.equal(o3[0], o1[0])                        # slot 0 of B = 3 == the same field alone


def test_error_codes():
    C = _pkg()
    p, q = proj(64, 64, "f32"), proj(64, 128, "f32")
    lib = p.lib
    F = p.tensor(inputs(64, 64, "f32")[1])
    e = R.default_edges()

    def bad(rc, code):
        assert rc == code and len(lib.cmbl_last_error()) > 0, (rc, lib.cmbl_last_error())

    bad(Plan(p, [0.0]).rc, ARG)                                                  # nedges < 2
    bad(Plan(p, np.arange(65537.0)).rc, ARG)                                     # nedges > 65536
    bad(Plan(p, [0.0, 10.0, 10.0, 20.0]).rc, ARG)                                # not strictly increasing
    bad(Plan(p, [0.0, np.nan, 20.0]).rc, ARG)
    bad(Plan(p, [0.0, 10.0, np.inf]).rc, ARG)
    bad(Plan(p, e, np.ones(q.lmag.shape)).rc, SHAPE)                             # weight plane of another grid
    w = np.ones(p.lmag.shape)
    w[3, 3] = np.inf
    bad(Plan(p, e, w).rc, ARG)
    assert Plan(p, np.arange(65536.0)).rc == 0                                   # the largest edge set
    pl = Plan(p, e)
    assert pl.rc == 0
    bad(pl.info(3)[0], ARG)
    bad(pl.info(0, n=pl.nbins + 1)[0], SHAPE)
    bad(raw(p, pl, FOURIER, F, None, [(0, 3)], 1)[0], ARG)                       # plane index outside [0, npol)
    bad(raw(p, pl, FOURIER, F, None, [(-1, 0)], 1)[0], ARG)
    bad(raw(p, pl, FOURIER, F, None, [(0, 2)], 1, P=2)[0], ARG)
    bad(raw(p, pl, FOURIER, F, None, [], 1)[0], ARG)                             # npairs < 1
    bad(raw(p, pl, FOURIER, F, None, [(0, 0)] * 10, 1)[0], ARG)                  # more than every ordered pair of three planes
    bad(raw(p, pl, FOURIER, F, None, [(0, 0)], 0)[0], ARG)                       # moments
    bad(raw(p, pl, FOURIER, F, None, [(0, 0)], 3)[0], ARG)
    bad(raw(p, pl, 3, F, None, [(0, 0)], 1)[0], ARG)                             # basis
    bad(raw(p, pl, FOURIER, F, None, [(0, 0)], 1, nb=257)[0], ARG)               # nbatch > 256 (rejected before anything is read)
    Fq = q.tensor(inputs(64, 128, "f32")[1])
    bad(raw(q, pl, FOURIER, Fq, None, [(0, 0)], 1)[0], SHAPE)                    # a plan used with a context of another size
    bad(raw(proj(64, 64, "f32", 3.0), pl, FOURIER, F, None, [(0, 0)], 1)[0], SHAPE)    # ... of another pixel size
    bad(raw(proj(64, 64, "f64"), pl, FOURIER, F, None, [(0, 0)], 1)[0], ARG)     # ... of another precision
    # the calls above left the library usable
    rc, out = raw(p, pl, FOURIER, F, None, PAIRS[3], 2)
    assert rc == 0 and torch.isfinite(out).all()
    del C


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_python_layer(prec, monkeypatch):
    C = _pkg()
    Ny, Nx = 90, 50
    p = C.ProjLambert(Ny, Nx, THETA, DT[prec][0])                                # a context of its own: its plan cache starts empty
    made = []
    create = p.lib.cmbl_clbins_create
    monkeypatch.setattr(p.lib, "cmbl_clbins_create", lambda *a: (made.append(1), create(*a))[1])
    m, _ = inputs(Ny, Nx, prec)
    qu = C.Field(p, p.tensor(np.ascontiguousarray(m[:, 1:])), C.MAP)             # B = 2, QU maps
    got = C.get_Cl(qu)
    assert isinstance(got, list) and len(got) == B and sorted(got[0]) == ["BB", "EE"] and made == [1]
    EB = p.convert(qu.arr, C.MAP, C.HARMONIC).cpu().numpy().astype(np.complex128)    # the engine's own (separately tested) QU -> EB
    for b in range(B):
        for k, n in enumerate(("EE", "BB")):
            ref = R.get_cl(EB[b, k], None, p.lmag, Ny, THETA)
            ok = ~np.isnan(ref["cl"])
            assert isinstance(got[b][n], C.Cls) and np.allclose(got[b][n].ell, ref["ell"][ok], rtol=1e-13, atol=0)
            close(("python get_Cl", n), got[b][n].cl, ref["cl"][ok], TOL[prec])
    again = C.get_Cl(qu, which=("QQ", "UU", "QU", "EB"))                         # Q / U and E / B pairs: two calls, ONE plan, found in the cache
    assert made == [1] and sorted(again[0]) == ["EB", "QQ", "QU", "UU"]
    Fq = np.fft.rfft2(m[:, 1:].astype(np.float64), axes=(-2, -1))
    close("python get_Cl QU", again[1]["QU"].cl, (lambda r: r["cl"][~np.isnan(r["cl"])])(R.get_cl(Fq[1, 0], Fq[1, 1], p.lmag, Ny, THETA)), TOL[prec])
    close("python get_Cl EB", again[1]["EB"].cl, (lambda r: r["cl"][~np.isnan(r["cl"])])(R.get_cl(EB[1, 0], EB[1, 1], p.lmag, Ny, THETA)), TOL[prec])
    # rotation invariance: EE + BB == QQ + UU mode by mode, so bin by bin
    close("python EE+BB", got[0]["EE"].cl + got[0]["BB"].cl, again[0]["QQ"].cl + again[0]["UU"].cl, TOL[prec])

    t = C.Field(p, p.tensor(np.ascontiguousarray(m[:1, :1])), C.MAP)             # spin 0, B = 1
    one = C.get_Cl(t, dl=200)
    assert isinstance(one, C.Cls) and made == [1, 1]
    fid = C.Cls(np.arange(2, 3001), 1.0 / np.arange(2, 3001.0) ** 2)
    c1, s1 = C.get_Cl(t, dl=200, Clfid=fid, err_estimate=True)
    c2, _ = C.get_Cl(t, dl=200, Clfid=fid, err_estimate=True)                    # the same Clfid: the plan is found
    C.get_Cl(t, dl=200, Clfid=lambda l: fid(l))                                  # another callable with the same weight plane: found by its bytes
    assert made == [1, 1, 1] and np.array_equal(c1.cl, c2.cl) and s1.shape == c1.cl.shape and np.all(s1 >= 0)
    F0 = np.fft.rfft2(m[0, 0].astype(np.float64))
    ref = R.get_cl(F0, None, p.lmag, Ny, THETA, ledges=R.default_edges(200), Clfid=fid)
    ok = ~np.isnan(ref["cl"])
    assert c1.ell.max() < 3000 + 200                                             # nothing beyond the table
    close("python Clfid cl", c1.cl, ref["cl"][ok], TOL[prec])
    # σℓ² N = S2/A − (S1/A)² is a difference of two sums that each carry the transform's error: compared on the scale of S2/A, over all bins
    N = ref["count"][ok] / 2
    assert np.linalg.norm((s1 ** 2 - ref["sigma"][ok] ** 2) * N) <= 4 * TOL[prec] * np.linalg.norm(ref["s2"][ok])
    # ρℓ, Dℓ, ℓ⁴Cℓ, cov_to_Cℓ
    rho = C.get_rhol(t, t, dl=200)
    np.testing.assert_allclose(rho.cl, 1.0, rtol=1e-15)
    rq = C.get_rhol(qu, which="EB")
    assert len(rq) == B and np.all(np.abs(rq[0].cl) <= 1 + 1e-6)
    np.testing.assert_allclose(C.get_Dl(t, dl=200).cl, one.ell ** 2 * one.cl / (2 * np.pi), rtol=1e-14)
    np.testing.assert_allclose(C.get_l4Cl(t, dl=200).cl, one.ell ** 4 * one.cl, rtol=1e-14)
    flat = C.Cls(np.arange(0, 20001), np.full(20001, 3.7e-5))
    back = C.cov_to_Cl(C.cl_to_2d(flat, p), p)
    np.testing.assert_allclose(back.cl, 3.7e-5 / (np.deg2rad(THETA / 60) * np.sqrt(Nx * Ny)), rtol=1e-6 if prec == "f32" else 1e-12)
    for wrong in (lambda: C.get_Cl(qu, which="QE"), lambda: C.get_Cl(qu, which="II"), lambda: C.get_Cl(t, which="EE"), lambda: C.get_rhol(qu)):
        with pytest.raises(ValueError):
            wrong()
