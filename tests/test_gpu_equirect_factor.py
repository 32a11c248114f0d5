"""sqrt, pinv, svdvals, logabsdet / logdet, solve and rdiv of BlockDiagEquiRect on the DEVICE path (cmbl_equirect_block_svd, _logabsdet, _solve;
`on="device"`) against the float64 NumPy oracles `op_*` of tests/_equirect_ref.py, in both context precisions.  The inputs are those of
tests/_equirect_factor_ref.py (all float32-representable, so both precisions factorise the same numbers); tests/test_equirect_factor_ref.py runs
the NumPy restatement of the Jacobi scheme on every one of them.

Bounds: float64 contexts 1e-12 (the project's float64 class bound, `_tol.close`); float32 contexts relative L2 <= 2^-23 (one rounding of a double
result at 2^-24 per element, with room for the double error); singular values max|σ - σ_numpy| <= 1e-12 σmax; the sign of the determinant
|s - s_ref| <= 8 Mh n 2^-53 (a product of Mh n unit phases, each good to a few ulp, on both sides).  Residuals |A X - B|_F and |S S - A|_F per
block: at most 3 x (tests/_tol.py's margin) that of NumPy on the same inputs, with the floor n 2^-52 |A|_F |X|_F; a float32 context adds the
rounding of its final store, 2^-24 |A|_F |X|_F.  Every figure is printed before it is asserted.

Shapes: n in {2, 3, 4, 6, 17, 33, 34, 64, 65, 66, 128, 130}: a single 2 x 2 rotation, the dummy column of an odd n, one past a wavefront, one past
a 16-wide LU panel and a 64-wide trailing tile."""
import numpy as np
import pytest
import torch

import _equirect_factor_ref as F
import _equirect_ref as R
import _tol

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
TID = ["f32", "f64"]
KINDS = [(Ny, Nx, n, cplx) for Ny, Nx in F.SHAPES for n, cplx in F.kinds(Ny)]
KID = [f"{Ny}x{Nx}_{'c' if c else 'r'}{n}" for Ny, Nx, n, c in KINDS]
BIG = KINDS[-1]                                            # complex n = 130
F32_BOUND = 2.0 ** -23


@pytest.fixture(scope="module")
def C():
    import cmblensing_jl_amd as C
    return C


_projs, _once_cache = {}, {}


def proj_of(C, Ny, Nx, T):
    if (Ny, Nx, T) not in _projs:
        _projs[(Ny, Nx, T)] = C.ProjEquiRect(Ny, Nx, (1.0, 2.0), (0.0, 2 * np.pi), T=T)
    return _projs[(Ny, Nx, T)]


def once(key, fn):
    """references are computed once, shared and never modified"""
    if key not in _once_cache:
        _once_cache[key] = fn()
    return _once_cache[key]


def op(C, blocks, Ny, Nx, T, **kw):
    p = proj_of(C, Ny, Nx, T)
    b = blocks.astype((np.complex64 if T == torch.float32 else np.complex128) if np.iscomplexobj(blocks) else (np.float32 if T == torch.float32 else np.float64))
    return C.BlockDiagEquiRect(p.tensor(b), p, **kw)


def host(M):
    a = (M.blocks if hasattr(M, "blocks") else M.arr).cpu().numpy()
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def close(what, got, want, T):
    if T == torch.float64:
        e = _tol.close(what, got, want, 1e-12)
    else:
        e = _tol.rel(got, want)
        assert e <= F32_BOUND, f"{what}: relative L2 error {e:.3e} > 2^-23"
    print(f"{what}: relative L2 error {e:.3e}")


def residual_ok(what, A, X, B, Xnp, T):
    """per block: |A X - B|_F of the device result against 3 x NumPy's, floor n 2^-52 |A| |X| (+ the float32 store)"""
    n = A.shape[-1]
    fro = lambda a: np.sqrt(np.sum(np.abs(a) ** 2, axis=(1, 2)))
    got, ref = fro(A @ X - B), fro(A @ Xnp - B)
    bound = np.maximum(3.0 * ref, (n * 2.0 ** -52 + (2.0 ** -24 if T == torch.float32 else 0.0)) * fro(A) * fro(X))
    k = int(np.argmax(got / bound))
    print(f"{what}: worst residual / bound = {got[k] / bound[k]:.3f} (block {k}: device {got[k]:.3e}, NumPy {ref[k]:.3e}, bound {bound[k]:.3e})")
    assert np.all(got <= bound), what


def inputs(kind, n, Mh, cplx):
    return once((kind, n, Mh, cplx), lambda: {"general": F.general_blocks, "gauss": F.gauss_blocks, "halfrank": F.half_rank_blocks,
                                              "psdhalf": F.psd_half_rank_blocks, "spd": lambda n, Mh, c: R.case_blocks(n, Mh, c, spd=True)}[kind](n, Mh, cplx))


def test_gaussian_seeds_are_well_conditioned():
    for Ny, Nx, n, cplx in KINDS:
        k = np.linalg.cond(R._ref(inputs("gauss", n, Nx // 2 + 1, cplx))).max()
        assert k <= 1e3, (n, cplx, k)


@pytest.mark.parametrize("T", DTYPES, ids=TID)
@pytest.mark.parametrize("kind", ["general", "spd", "gauss"])
@pytest.mark.parametrize("case", KINDS, ids=KID)
def test_sqrt_pinv_svdvals(C, case, kind, T):
    Ny, Nx, n, cplx = case
    b = inputs(kind, n, Nx // 2 + 1, cplx)
    M = op(C, b, Ny, Nx, T)
    assert M.factor_on == "host"
    close("sqrt", host(M.sqrt(on="device")), once(("sqrt", kind, case), lambda: R.op_sqrt(b)), T)
    close("pinv", host(M.pinv(on="device")), once(("pinv", kind, case), lambda: R.op_pinv(b)), T)
    sv, ref = M.svdvals(on="device"), once(("sv", kind, case), lambda: np.linalg.svd(R._ref(b), compute_uv=False))
    e = np.max(np.abs(sv - ref) / ref.max(axis=1, keepdims=True))
    print(f"svdvals: max |σ - σ_numpy| / σmax = {e:.3e}")
    assert sv.shape == (Nx // 2 + 1, n) and e <= 1e-12
    if kind == "spd":
        S, A = R._ref(host(M.sqrt(on="device"))), R._ref(b)
        Snp = R._ref(once(("sqrt", kind, case), lambda: R.op_sqrt(b)))
        residual_ok("S S - A", S, S, A, Snp, T)


@pytest.mark.parametrize("T", DTYPES, ids=TID)
@pytest.mark.parametrize("kind", ["general", "spd", "gauss"])
@pytest.mark.parametrize("case", KINDS, ids=KID)
def test_solve_rdiv(C, case, kind, T):
    Ny, Nx, n, cplx = case
    Mh = Nx // 2 + 1
    a, b2 = inputs(kind, n, Mh, cplx), inputs("general", n, Mh, cplx)
    A, B = op(C, a, Ny, Nx, T), op(C, b2, Ny, Nx, T)
    X = A.solve(B, on="device")
    assert X.blocks.dtype == A.blocks.dtype
    close("solve(M2)", host(X), once(("solve", kind, case), lambda: R.op_solve(a, b2)), T)
    close("rdiv(M2)", host(B.rdiv(A, on="device")), once(("rdiv", kind, case), lambda: R.op_rdiv(b2, a)), T)
    Xnp = once(("solve", kind, case), lambda: R.op_solve(a, b2))
    residual_ok("A X - B", R._ref(a), R._ref(host(X)), R._ref(b2), R._ref(Xnp), T)
    _, az = R.case_fields(Ny, Nx, 3, 2 if cplx else 0, seed=4)               # three batch slots
    p = proj_of(C, Ny, Nx, T)
    f = C.EquiRectField(p, p.tensor(az.astype(np.complex64 if T == torch.float32 else np.complex128)), C.AZFOURIER)
    x = A.solve(f, on="device")
    assert isinstance(x, C.EquiRectField) and x.basis == C.AZFOURIER and x.arr.dtype == p.CT
    want = np.linalg.solve(R._ref(a).astype(np.complex128)[None], az[..., None])[..., 0]
    close("solve(field)", host(x), want, T)


@pytest.mark.parametrize("T", DTYPES, ids=TID)
@pytest.mark.parametrize("case", KINDS, ids=KID)
def test_mixed_element_types(C, case, T):
    """real \\ complex and complex \\ real blocks (the result is complex), against the oracle"""
    Ny, Nx, n, cplx = case
    if not cplx:
        return
    Mh = Nx // 2 + 1
    ar, bc = once(("mixr", n, Mh), lambda: F.general_blocks(n, Mh, False, seed=3)), inputs("general", n, Mh, True)
    A, B = op(C, ar, Ny, Nx, T), op(C, bc, Ny, Nx, T)
    close("real \\ complex", host(A.solve(B, on="device")), R.op_solve(ar, bc), T)
    close("complex \\ real", host(B.solve(A, on="device")), R.op_solve(bc, ar), T)
    close("real / complex", host(A.rdiv(B, on="device")), R.op_rdiv(ar, bc), T)


@pytest.mark.parametrize("T", DTYPES, ids=TID)
@pytest.mark.parametrize("case", KINDS, ids=KID)
def test_logabsdet_logdet(C, case, T):
    Ny, Nx, n, cplx = case
    Mh = Nx // 2 + 1
    for kind in ("spd", "general"):
        b = inputs(kind, n, Mh, cplx)
        M = op(C, b, Ny, Nx, T)
        l, s = M.logabsdet(on="device")
        lr, sr = once(("lad", kind, case), lambda: R.op_logabsdet(b))
        print(f"{kind}: log|det| {l:.15e} (NumPy {lr:.15e}), |s - s_ref| = {abs(s - sr):.3e}, bound {8 * Mh * n * 2.0 ** -53:.3e}")
        if kind == "spd":
            _tol.scalars_close("log|det|", l, lr, 1e-12)
        assert abs(s - sr) <= 8 * Mh * n * 2.0 ** -53
        v = l + np.log(s)
        ld = M.logdet(on="device")
        assert ld == (float(v.real) if abs(v.imag) < 1e-12 else v)


@pytest.mark.parametrize("T", DTYPES, ids=TID)
@pytest.mark.parametrize("case", KINDS, ids=KID)
def test_rank_deficient(C, case, T):
    Ny, Nx, n, cplx = case
    Mh = Nx // 2 + 1
    b = inputs("halfrank", n, Mh, cplx)
    r = n - n // 2
    sv = once(("sv", "halfrank", case), lambda: np.linalg.svd(R._ref(b), compute_uv=False))
    assert sv[:, r - 1].min() >= 0.5 and (r == n or sv[:, r:].max() <= 1e-14)          # the cut at 1e-10 is unambiguous
    M = op(C, b, Ny, Nx, T)
    want = once(("pinv", "halfrank", case), lambda: R._ref(np.linalg.pinv(R._ref(b), rcond=1e-10)))
    close("pinv of half rank", host(M.pinv(rtol=1e-10, on="device")), want, T)
    close("pinv of half rank, host path with the same rtol", host(M.pinv(rtol=1e-10)), want, T)
    h = inputs("psdhalf", n, Mh, cplx)
    S = R._ref(host(op(C, h, Ny, Nx, T).sqrt(on="device")))
    residual_ok("S S - A, half rank", S, S, R._ref(h), R._ref(once(("sqrt", "psdhalf", case), lambda: R.op_sqrt(h))), T)


@pytest.mark.parametrize("T", DTYPES, ids=TID)
@pytest.mark.parametrize("case", [KINDS[1], KINDS[4], BIG], ids=[KID[1], KID[4], KID[-1]])
def test_zero_block(C, case, T):
    from cmblensing_jl_amd.lib import CmblError
    Ny, Nx, n, cplx = case
    Mh = Nx // 2 + 1
    b = F.with_zero_block(inputs("general", n, Mh, cplx), 1)
    M = op(C, b, Ny, Nx, T)
    sq, pi = M.sqrt(on="device").blocks, M.pinv(on="device").blocks
    assert not sq[1].any() and not pi[1].any() and sq[0].any() and pi[2].any()
    close("pinv beside a zero block", host(M.pinv(on="device")), R.op_pinv(b), T)
    l, s = M.logabsdet(on="device")
    assert l == -np.inf and s == 0
    with pytest.raises(CmblError) as e:
        M.solve(M, on="device")
    assert e.value.code == 4 and "block 1" in str(e.value)                    # CMBL_ERR_NAN


def _bits(t):
    return torch.view_as_real(t) if t.is_complex() else t


@pytest.mark.parametrize("T", DTYPES, ids=TID)
@pytest.mark.parametrize("case", [KINDS[4], BIG], ids=[KID[4], KID[-1]])
def test_repeats_and_slabs_are_bit_identical(C, case, T):
    Ny, Nx, n, cplx = case
    Mh = Nx // 2 + 1
    a, b2 = inputs("gauss", n, Mh, cplx), inputs("general", n, Mh, cplx)
    p = proj_of(C, Ny, Nx, T)

    def run():
        A, B = op(C, a, Ny, Nx, T, factor_on="device"), op(C, b2, Ny, Nx, T)
        return [_bits(x) for x in (A.sqrt().blocks, A.pinv().blocks, A.solve(B).blocks, B.rdiv(A, on="device").blocks)] + [A.logabsdet(), A.svdvals()]

    first, again = run(), run()
    old = p._ctx.set_option("eq_factor_scratch_mb", 0)                       # one block per slab
    try:
        slabbed = run()
    finally:
        p._ctx.set_option("eq_factor_scratch_mb", old)
    for other in (again, slabbed):
        for x, y in zip(first[:4], other[:4]):
            assert torch.equal(x, y)
        assert first[4] == other[4] and np.array_equal(first[5], other[5])


@pytest.mark.parametrize("T", DTYPES, ids=TID)
def test_caches_are_kept_per_path(C, T):
    Ny, Nx, n, cplx = KINDS[2]
    M = op(C, inputs("spd", n, Nx // 2 + 1, cplx), Ny, Nx, T)
    h, d = M.sqrt(), M.sqrt(on="device")
    assert h is M.sqrt() and d is M.sqrt(on="device") and h is not d
    assert M.pinv() is M.pinv(on="host") and M.pinv(on="device") is not M.pinv() and M.pinv(rtol=1e-3, on="device") is not M.pinv(on="device")
    assert M.logabsdet(on="device") is M.logabsdet(on="device")
    for fn in (M.sqrt, M.pinv, M.logabsdet, M.logdet, M.svdvals, lambda on: M.solve(M, on=on), lambda on: M.rdiv(M, on=on)):
        with pytest.raises(ValueError):
            fn(on="gpu")
    with pytest.raises(ValueError):
        C.BlockDiagEquiRect(M.blocks, M.proj, factor_on="gpu")


def _rel(a, b):
    a, b = (x.arr.cpu().numpy().astype(np.complex128).ravel() for x in (a, b))
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(a), np.linalg.norm(b)))


@pytest.mark.parametrize("T", DTYPES, ids=TID)
def test_reference_properties_on_the_device_path(C, T):
    """test/runtests.jl:698-720 with every factorisation on the device, at the reference's rtol = 1e-4"""
    import _equirect_cov_ref as RC
    case = RC.GPU_CASES[3]
    Ny, Nx = case[:2]
    p = once(("refproj", T), lambda: C.ProjEquiRect(case[0], case[1], case[2], case[3], T=T))
    tt, ee, bb = once("cl", lambda: RC.camb_total(2000))
    rng = np.random.default_rng(5)
    for Cf, P in ((C.Cl_to_Cov("I", p, tt, lmax=2000), 1), (C.Cl_to_Cov("P", p, ee, bb, lmax=2000), 2)):
        Cf.factor_on = "device"
        f = C.EquiRectField(p, p.tensor(rng.standard_normal((1, P, Nx, Ny))), C.MAP).to(C.AZFOURIER)
        errs = {"pinv": _rel(Cf.pinv() * (Cf * f), f), "solve": _rel(Cf.solve(Cf) * f, f), "rdiv": _rel(Cf.rdiv(Cf) * f, f),
                "solve(field)": _rel(Cf.solve(Cf * f), f), "sqrt": _rel(Cf.sqrt() * (Cf.sqrt() * f), Cf * f)}
        print(f"spin {0 if P == 1 else 2}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= 1e-4, (P, k, v)
        assert abs(Cf.logdet() - Cf.logabsdet()[0]) <= 1e-8 * abs(Cf.logabsdet()[0])
        g = C.simulate(Cf, seed=3)
        assert isinstance(g, C.EquiRectField) and g.basis == C.AZFOURIER and g.arr.dtype == p.CT
        assert "device" in Cf._sqrt and "host" not in Cf._sqrt                # simulate followed factor_on


def test_error_codes(C):
    import ctypes
    from cmblensing_jl_amd.lib import CmblError
    Ny, Nx, n, cplx = KINDS[2]
    Mh = Nx // 2 + 1
    T = torch.float64
    p = proj_of(C, Ny, Nx, T)
    M = op(C, inputs("general", n, Mh, cplx), Ny, Nx, T)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.empty_like(M.blocks)
    three = (ctypes.c_double * 3)()
    assert p.lib.cmbl_equirect_block_svd(p._h, vp(M.blocks), 0, n + 1, 1e-15, vp(out), None, None, None) == 2          # a wrong n: CMBL_ERR_SHAPE
    assert p.lib.cmbl_equirect_block_logabsdet(p._h, vp(M.blocks), 0, n + 1, three) == 2
    assert p.lib.cmbl_equirect_block_solve(p._h, vp(M.blocks), 0, n + 1, 0, vp(M.blocks), 0, 0, vp(out), 1) == 2
    assert p.lib.cmbl_equirect_block_svd(p._h, vp(M.blocks), 0, n, 1e-15, vp(M.blocks), None, None, None) == 1          # out aliases the input: CMBL_ERR_ARG
    assert p.lib.cmbl_equirect_block_svd(p._h, vp(M.blocks), 0, n, 1e-15, vp(out), vp(out), None, None) == 1
    assert p.lib.cmbl_equirect_block_solve(p._h, vp(M.blocks), 0, n, 0, vp(out), 0, 0, vp(out), 1) == 1
    assert p.lib.cmbl_equirect_block_solve(p._h, vp(M.blocks), 0, n, 0, vp(out), 0, 0, vp(M.blocks), 1) == 1
    assert p.lib.cmbl_equirect_block_solve(p._h, vp(M.blocks), 0, n, 2, vp(M.blocks), 0, 0, vp(out), 1) == 1          # a side that does not exist
    assert p.lib.cmbl_equirect_block_svd(p._h, vp(M.blocks), 0, n, -1.0, vp(out), None, None, None) == 1
    bad = M.blocks.clone()
    bad[Mh - 1, n - 1, n - 2] = float("nan")
    N = C.BlockDiagEquiRect(bad, p)
    for fn in (lambda: N.sqrt(on="device"), lambda: N.logabsdet(on="device"), lambda: N.solve(M, on="device"), lambda: M.solve(N, on="device")):
        assert pytest.raises(CmblError, fn).value.code == 4                   # CMBL_ERR_NAN
    bad[Mh - 1, n - 1, n - 2] = float("inf")
    assert pytest.raises(CmblError, lambda: C.BlockDiagEquiRect(bad, p).pinv(on="device")).value.code == 4
    # n > 2048 is refused before anything is read or allocated: the pointers below are far too small for such blocks
    big = proj_of(C, 4096, 2, T)
    assert big.lib.cmbl_equirect_block_svd(big._h, vp(M.blocks), 0, 4096, 1e-15, vp(out), None, None, None) == 2
    assert big.lib.cmbl_equirect_block_logabsdet(big._h, vp(M.blocks), 0, 4096, three) == 2
    assert big.lib.cmbl_equirect_block_solve(big._h, vp(M.blocks), 0, 4096, 0, vp(M.blocks), 0, 0, vp(out), 1) == 2
