"""The two oracles of Cℓ_to_Cov on ProjEquiRect (tests/_equirect_cov_ref.py) against each other and against the properties the reference's
own test set asks of the operators (test/runtests.jl:680-720); no GPU.  `python tests/test_equirect_cov_ref.py` rewrites
tests/golden/equirect_cov_budget.json (minutes: the (32, 64) case runs in np.longdouble)."""
import json
import os

import numpy as np
import pytest

import _equirect_cov_ref as R

BUDGET = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "equirect_cov_budget.json")
TABLE_CASES = [R.GPU_CASES[1], R.GPU_CASES[3]]                              # (5, 12) K = 3 and the reference's (32, 64)
TABLE_NGRID = (50_000, 2001)


def blocks(case, pol, dt=np.float64, table=None, lmax=R.LMAX_TEST):
    """oracle (a) on a GPU case with the total CAMB spectra"""
    Ny, Nx, ts, ps = case
    tt, ee, bb = R.camb_total(lmax)
    theta = R.geometry(Ny, Nx, ts, ps)["theta"]
    if pol == "I":
        return R.cov_I(theta, ps, Nx, tt, dt, None if table is None else R.make_table(table, tt))
    return R.cov_P(theta, ps, Nx, ee, bb, dt, None if table is None else R.make_table(table, ee, bb))


# ---- (a) == (b): the test that fixes every sign -------------------------------------------------------------------------------------------
# Both sides are float64 sums of a few thousand terms; the defining sum of Wigner-d alternates with terms up to binom(24, 12) ≈ 2.7e6 at
# ℓ = 12, i.e. up to 2.7e6 · 2^-53 ≈ 3e-10 of cancellation error in the worst case.  A wrong sign or convention is an error of order 1.
AB_TOL = 1e-9


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("shape", [(4, 8), (5, 12)])
@pytest.mark.parametrize("kind", ["I", "P", "E", "B"])
def test_real_space_equals_harmonic_space(shape, K, kind):
    Ny, Nx = shape
    lmax = 12
    rng = np.random.default_rng([Ny, Nx, K])
    ts, ps = (0.5, 1.7), (0.2, 0.2 + 2 * np.pi / K)
    theta = R.geometry(Ny, Nx, ts, ps)["theta"]
    cl, ee, bb = (rng.random(lmax + 1) + 0.1 for _ in range(3))
    ee[:2] = bb[:2] = 0
    if kind == "I":
        a, (b, off) = R.cov_I(theta, ps, Nx, cl), R.harmonic_I(Ny, Nx, ts, ps, cl)
        assert np.abs(b.imag).max() <= AB_TOL * np.abs(b).max()             # real blocks
    else:
        ee, bb = (ee if kind in "PE" else 0 * ee), (bb if kind in "PB" else 0 * bb)
        a, (b, off) = R.cov_P(theta, ps, Nx, ee, bb), R.harmonic_P(Ny, Nx, ts, ps, ee, bb)
    scale = np.abs(b).max()
    assert off <= AB_TOL * scale                                             # block-diagonal in m
    assert np.abs(a - b).max() <= AB_TOL * scale


# ---- structure ----------------------------------------------------------------------------------------------------------------------------
def _budget():
    with open(BUDGET) as f:
        return json.load(f)


@pytest.mark.parametrize("case", R.GPU_CASES[:3], ids=R.case_id)
@pytest.mark.parametrize("pol", ["I", "P"])
def test_structure(case, pol):
    """real symmetric / Hermitian, and positive semi-definite up to the rounding of the oracle: by Weyl's inequality an error Δ of the n x n block
    moves an eigenvalue by at most ||Δ||₂ <= n max|Δ| <= n · budget[m] · max|block| <= n · budget[m] · λ_max"""
    C = blocks(case, pol)
    bud = np.array(_budget()["oracle"][f"{R.case_id(case)}_{pol}"])
    n = C.shape[1]
    CH = np.conj(np.transpose(C, (0, 2, 1)))
    if pol == "I":
        assert not np.iscomplexobj(C) and np.array_equal(C, CH)
    else:
        assert np.all(np.abs(C - CH).reshape(C.shape[0], -1).max(axis=1) <= 2 * bud * np.abs(C).reshape(C.shape[0], -1).max(axis=1))
    ev = np.linalg.eigvalsh((C + CH) / 2)
    assert np.all(ev.min(axis=1) >= -n * bud * ev.max(axis=1)), (ev.min(axis=1) / ev.max(axis=1), bud)


@pytest.mark.parametrize("pol", ["I", "P"])
def test_periodisation_identity(pol):
    """the blocks of a K = 3, Nx = 8 projection are the blocks at modes 3m of the K = 1, Nx = 24 projection on the same rings"""
    Ny, lmax = 5, 40
    rng = np.random.default_rng(7)
    ts, p3, p1 = (0.4, 1.9), (0.3, 0.3 + 2 * np.pi / 3), (0.3, 0.3 + 2 * np.pi)
    theta = R.geometry(Ny, 8, ts, p3)["theta"]
    assert np.array_equal(theta, R.geometry(Ny, 24, ts, p1)["theta"])
    cl, bb = rng.random(lmax + 1), rng.random(lmax + 1)
    if pol == "I":
        a, b = R.cov_I(theta, p3, 8, cl), R.cov_I(theta, p1, 24, cl)
        sel = b[[0, 3, 6, 9, 12]]
    else:
        a, b = R.cov_P(theta, p3, 8, cl, bb), R.cov_P(theta, p1, 24, cl, bb)
        # mode 12 = 3 · 4 is its own mirror in both; modes 3m, m < 4, keep their mirrors 24 - 3m = 3 (8 - m)
        sel = b[[0, 3, 6, 9, 12]]
    # the same 24 numbers c per ring pair, summed in another order: each side errs by at most 24 · 2^-53 · Σ|c| <= 24² · 2^-53 · max|c|, and
    # max|c| <= max|b| by Parseval
    d = np.abs(a - sel).max() / np.abs(b).max()
    print("periodisation", pol, d)
    assert d <= 2 * 24 ** 2 * 2.0 ** -53


# ---- the reference's own properties on oracle blocks (test/runtests.jl:691-720, rtol = 1e-4) ------------------------------------------------
# Run at ℓmax = 10 000 and at ℓmax = 2000 on the (32, 64) projection of the reference's test: every property holds at both with errors below
# 1e-12 (the blocks' condition numbers stay below 200), so the tests use ℓmax = 2000 = _equirect_cov_ref.LMAX_TEST, the cheapest allowed.
@pytest.fixture(scope="module")
def ref_blocks():
    return {pol: blocks(R.GPU_CASES[3], pol) for pol in "IP"}


@pytest.mark.parametrize("pol", ["I", "P"])
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_reference_properties(ref_blocks, pol, dt):
    C = ref_blocks[pol]
    C = C.astype(dt if pol == "I" else (np.complex64 if dt is np.float32 else np.complex128))      # the blocks as a context of that precision holds them
    for name, err in R.reference_properties(C, 0 if pol == "I" else 2, 64).items():
        assert err <= 1e-4, (name, err)


# ---- the budget file ----------------------------------------------------------------------------------------------------------------------
def sampled_interp_error(pol, lmax=10_000, ngrid=50_000, Ny=512, Nx=1024, npairs=64):
    """table lookup against the direct sum at the default ℓmax on `npairs` ring pairs drawn from the 512 x 1024 grid of the reference's spans:
    (max |Δc| / max |c| in real space, max over m of max_pairs |Δ_m| / max_pairs |ref_m| of the periodised transforms)"""
    tt, ee, bb = R.camb_total(lmax)
    theta = R.geometry(Ny, Nx, R.REF_THETA_SPAN, R.REF_PHI_SPAN)["theta"]
    rng = np.random.default_rng(11)
    j, k = rng.integers(0, Ny, npairs), rng.integers(0, Ny, npairs)
    K = R.span_K(R.REF_PHI_SPAN)[0]
    h = R._separations(theta, K, Nx, j, k, np.float64)[0]
    if pol == "I":
        d, t = (R.correlation(h, tt, None, np.float64, tab) for tab in (None, R.make_table(ngrid, tt)))
        d, t = [d], [t]
    else:
        d, t = (R.correlation(h, ee, bb, np.float64, tab) for tab in (None, R.make_table(ngrid, ee, bb)))
    real = max(float(np.abs(a - b).max() / np.abs(a).max()) for a, b in zip(d, t))
    spec = 0.0
    for a, b in zip(d, t):
        Fa, Fb = (np.fft.fft(R._periodise(v, K, Nx), axis=1) for v in (a, b))
        spec = max(spec, float((np.abs(Fa - Fb).max(axis=0) / np.abs(Fa).max(axis=0)).max()))
    return {"real_space": real, "per_mode_max": spec}


def compute_budget():
    out = {"lmax": R.LMAX_TEST, "spectra": "total TT / EE, BB of tests/golden/camb_cls.npz",
           "oracle": {}, "interp": {}, "interp_lmax10000_ngrid50000": {}}
    for case in R.GPU_CASES:
        for pol in "IP":
            out["oracle"][f"{R.case_id(case)}_{pol}"] = R.err_per_m(blocks(case, pol), blocks(case, pol, np.longdouble)).tolist()
    for case in TABLE_CASES:
        for pol in "IP":
            direct = blocks(case, pol)
            for ngrid in TABLE_NGRID:
                out["interp"][f"{R.case_id(case)}_{pol}_{ngrid}"] = R.err_per_m(blocks(case, pol, table=ngrid), direct).tolist()
    for pol in "IP":
        out["interp_lmax10000_ngrid50000"][pol] = sampled_interp_error(pol)
    return out


def test_budget_file_covers_every_case():
    b = _budget()
    assert b["lmax"] == R.LMAX_TEST
    for case in R.GPU_CASES:
        for pol in "IP":
            v = np.array(b["oracle"][f"{R.case_id(case)}_{pol}"])
            assert v.shape == (case[1] // 2 + 1,) and np.all(v > 0) and np.all(v < 1e-6)
    for case in TABLE_CASES:
        for pol in "IP":
            for ngrid in TABLE_NGRID:
                v = np.array(b["interp"][f"{R.case_id(case)}_{pol}_{ngrid}"])
                assert v.shape == (case[1] // 2 + 1,) and np.all(v > 0)
    assert set(b["interp_lmax10000_ngrid50000"]) == {"I", "P"}


if __name__ == "__main__":
    with open(BUDGET, "w") as f:
        json.dump(compute_budget(), f, indent=1)
        f.write("\n")
