"""Every any-size transform kernel and launch branch, from 2 to 4096 points (csrc/engine_gen.hpp Ctx::gen_dft, tables of Ctx::build_axis).

A length without a compile-time plan (kernels_ct.hpp) takes
  * k_gen_dft_mr<T, big> (run-time mixed-radix plan) when it is 13-smooth: big = a radix 7, 11 or 13; the twiddle table sits in LDS unless
    the two ping-pong buffers and the table exceed 158 KiB (double precision, one sequence: 48 N bytes > 161 792 for N >= 3371); a strided
    side without a big radix widens to Smin sequences (64 bytes: 8 in single, 4 in double precision) when the launch is large enough;
  * k_gen_dft<T, LGL> (chirp-z) otherwise, or for every length with CMBL_GEN_BLUESTEIN=1: a convolution of length L = 2^LGL >= 2N - 1,
    LGL = max(3, ceil(log2(2N - 1))), compiled for LGL 3 ... 13 (CMBL_GEN_LIST of engine.hpp).
SIZES lists the lengths that reach each of them; tests/test_boundary.py recomputes the branch of each length and fails when one is missing.
Tolerances are the class bounds of tests/test_gpu_parity.py (single precision at the long sides: tests/test_gpu_anysize.py TOL32_PATCH)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as O
import test_gpu_parity as TP
from test_gpu_parity import DT, TOL, sims, _pkg, close
from test_gpu_anysize import TOL32_PATCH


@pytest.fixture(scope="module")
def camb():
    return O.load_camb()


# (N, forced): forced = 1 runs the length through the chirp-z kernel with CMBL_GEN_BLUESTEIN=1 (and CMBL_FORCE_GENERIC=1)
SIZES = (
    # chirp-z, natural (a prime factor > 13): L = 2^LGL >= 2N - 1
    (17, 0),      # prime;          2*17 - 1 = 33     -> L = 64    (LGL 6), smallest of LGL 6
    (31, 0),      # prime;          2*31 - 1 = 61     -> L = 64    (LGL 6), largest
    (37, 0),      # prime;          73                -> L = 128   (LGL 7), odd
    (62, 0),      # 2*31;           123               -> L = 128   (LGL 7), largest, even
    (67, 0),      # prime;          133               -> L = 256   (LGL 8), smallest
    (127, 0),     # prime;          253               -> L = 256   (LGL 8), largest
    (129, 0),     # 3*43;           257               -> L = 512   (LGL 9), smallest
    (254, 0),     # 2*127;          507               -> L = 512   (LGL 9), even
    (255, 0),     # 3*5*17;         509               -> L = 512   (LGL 9), largest
    (257, 0),     # prime;          513               -> L = 1024  (LGL 10), smallest
    (510, 0),     # 2*3*5*17;       1019              -> L = 1024  (LGL 10), even
    (511, 0),     # 7*73;           1021              -> L = 1024  (LGL 10), largest
    (513, 0),     # 3^3*19;         1025              -> L = 2048  (LGL 11), smallest
    (1022, 0),    # 2*7*73;         2043              -> L = 2048  (LGL 11), even
    (1023, 0),    # 3*11*31;        2045              -> L = 2048  (LGL 11), largest
    (1025, 0),    # 5^2*41;         2049              -> L = 4096  (LGL 12), smallest
    (2038, 0),    # 2*1019;         4075              -> L = 4096  (LGL 12), even
    (2039, 0),    # prime;          4077              -> L = 4096  (LGL 12)
    (2047, 0),    # 23*89;          4093              -> L = 4096  (LGL 12), largest
    (2049, 0),    # 3*683;          4097              -> L = 8192  (LGL 13), smallest
    (4093, 0),    # prime;          8185              -> L = 8192  (LGL 13); double precision: 8704 padded slots * 16 B = 139 280 B of LDS
    (4094, 0),    # 2*23*89;        8187              -> L = 8192  (LGL 13), largest, even
    # chirp-z, forced (CMBL_GEN_BLUESTEIN=1): the lengths that otherwise have a plan
    (2, 1),       # 2*2 - 1 = 3     -> L = 8     (LGL 3)
    (3, 1),       # 5               -> L = 8     (LGL 3)
    (4, 1),       # 7               -> L = 8     (LGL 3), largest
    (5, 1),       # 9               -> L = 16    (LGL 4)
    (8, 1),       # 15              -> L = 16    (LGL 4), largest
    (16, 1),      # 31              -> L = 32    (LGL 5), largest
    (4096, 1),    # 8191            -> L = 8192  (LGL 13) exactly 2N
    # run-time plans with a big radix, twiddles in LDS
    (1001, 0),    # 7*11*13
    (2002, 0),    # 2*7*11*13
    (2197, 0),    # 13^3
    # run-time plans, twiddles in global memory in double precision (48 N > 158 * 1024 = 161 792 at one sequence per workgroup)
    (3375, 0),    # 3^3*5^3:        48*3375 = 162 000
    (4000, 0),    # 2^5*5^3:        192 000
    (4095, 0),    # 3^2*5*7*13:     196 560, big radix too
    (3584, 0),    # 2^9*7:          172 032, big radix too
    # run-time plans with many stages of one radix
    (2187, 0),    # 3^7
    (3125, 0),    # 5^5
    (2401, 0),    # 7^4, big
    (1331, 0),    # 11^3, big
    # smallest sizes (all below 32: the any-size path even for powers of two)
    (2, 0),       # radix 2
    (3, 0),       # radix 3
    (4, 0),       # radix 4
    (5, 0),       # radix 5
    (7, 0),       # radix 7, big
    (8, 0),       # 4*2
    (16, 0),      # 4*4
)


def _ctx(C, Ny, Nx, tT, forced):
    """a context; forced: every length a chirp-z transform (the variables are read once, at construction)"""
    if not forced:
        return C.ProjLambert(Ny, Nx, 2.0, tT)
    os.environ["CMBL_GEN_BLUESTEIN"] = "1"
    os.environ["CMBL_FORCE_GENERIC"] = "1"
    try:
        return C.ProjLambert(Ny, Nx, 2.0, tT)
    finally:
        os.environ.pop("CMBL_GEN_BLUESTEIN")
        os.environ.pop("CMBL_FORCE_GENERIC")


def _transforms(prec, Ny, Nx, forced=0, seed=0):
    """rfft2 against NumPy in float64, the round trip, irfft2 of a non-Hermitian half plane (FFTW c2r: odd Ny has no Nyquist column), and
    MAP -> HARMONIC -> FOURIER / MAP with P = 2 (QU <-> EB); forced: the chirp-z results also against the default plans of the same shape"""
    C = _pkg()
    tT, nT = DT[prec]
    p = _ctx(C, Ny, Nx, tT, forced)
    op = O.Proj(Ny, Nx, 2.0, np.float64)
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((1, 2, Nx, Ny)).astype(nT)
    ref = np.fft.rfft2(m.astype(np.float64), axes=(-2, -1))
    junk = rng.standard_normal(ref.shape) + 1j * rng.standard_normal(ref.shape)
    t, ht = TOL[prec]["fft"], 3 * TOL[prec]["fft"]
    tag = f"{Ny}x{Nx}"
    fl = p.rfft(p.tensor(m))
    h = p.convert(p.tensor(m), C.MAP, C.HARMONIC)
    got = [fl.cpu().numpy(), p.irfft(fl).cpu().numpy(), p.irfft(p.tensor(junk)).cpu().numpy(), h.cpu().numpy(),
           p.convert(h, C.HARMONIC, C.FOURIER).cpu().numpy(), p.convert(h, C.HARMONIC, C.MAP).cpu().numpy()]
    close(f"rfft2 {tag}", got[0], ref, t)
    close(f"irfft2(rfft2) {tag}", got[1], m, t)
    close(f"irfft2 non-hermitian {tag}", got[2], O.irfft2(junk, Ny), t)
    close(f"MAP->HARMONIC {tag}", got[3], O.to_harm(op, m.astype(np.float64)), ht)
    close(f"HARMONIC->FOURIER {tag}", got[4], O.rfft2(m.astype(np.float64)), ht)
    close(f"HARMONIC->MAP {tag}", got[5], m, ht)
    if forced:
        q = _ctx(C, Ny, Nx, tT, 0)
        fq = q.rfft(q.tensor(m))
        hq = q.convert(q.tensor(m), C.MAP, C.HARMONIC)
        want = [fq.cpu().numpy(), q.irfft(fq).cpu().numpy(), q.irfft(q.tensor(junk)).cpu().numpy(), hq.cpu().numpy()]
        for name, a, b in zip(("rfft2", "irfft2(rfft2)", "irfft2 non-hermitian", "MAP->HARMONIC"), got, want):
            close(f"chirp-z vs default plans {name} {tag}", a, b, t if name != "MAP->HARMONIC" else ht)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("N,forced", SIZES)
def test_every_transform_branch_against_numpy(prec, N, forced):
    """each length of SIZES on the column side (N x 48) and on the row side (48 x N, 45 x N for odd N); 48 = 3*4*4 and 45 = 3*3*5 have run-time
    plans and no compile-time plan, so the partner side also runs k_gen_dft_mr (k_gen_dft<T, 7> when forced).  (Even Ny with odd Nx
    has no reference: ProjLambert's Nyquist-column copy of sin2phi, src/proj_lambert.jl:69-71, has Nx÷2 - 1 sources for Nx - Nx÷2 - 1 slots.)"""
    for Ny, Nx in ((N, 48), (48 if N % 2 == 0 else 45, N)):
        _transforms(prec, Ny, Nx, forced, seed=N)


# 1080 = 2^3*3^3*5 has no compile-time plan and no big radix.  In a 1080^2 P = 2 transform the column pass covers 1080 sequences per slice
# (2160 in all, at least Smin * 256 CUs / 2 = 1024 in single, 512 in double precision), starts at S = max(1, min(2048 / 1080, 2160 / 1024)) = 1
# sequence per workgroup and writes with a stride: S widens to Smin (8 / 4; two buffers 2 * Smin * 1080 * sizeof(cx) = 138 240 B <= 150 KiB).
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx", [(2, 2), (3, 2), (2, 4), (5, 2), (5, 3), (1080, 1080)])
def test_smallest_maps_and_the_widened_strided_plan(prec, Ny, Nx):
    _transforms(prec, Ny, Nx, 0, seed=Ny * Nx)


# one thin shape per new class: chirp-z L = 8192 on either side, a big radix with global twiddles (double precision), 3^7, both sides chirp-z
# LGL 6, a 3 x 2 map.  The long strips are 96 pixels wide, as in test_gpu_anysize.py.  Strips of 136 degrees are not single-precision parity
# cases: their lowest ly modes deflect by many pixels and the flow amplifies rounding (measured L*f 2.2e-3 at 4093 x 96, 9e-3 at 4093 x 32),
# although the transforms of those lengths meet the bounds of test_every_transform_branch_against_numpy; nor are 32- and 40-pixel-wide strips
# (L'g 7.7e-4 at 2187 x 40).  So single precision reaches L = 8192 at the shortest chirp-z lengths that need it, 2049 and 2050 (68 degrees), and
# double precision at 4093 and 4094 (test_gpu_anysize.py test_largest_row_length_double_precision: the same holds for 45 x 4095).
FLOW_SHAPES = [("f32", 2049, 96), ("f64", 4093, 96), ("f32", 96, 2050), ("f64", 96, 4094), ("f64", 45, 4095), ("f32", 2187, 96), ("f64", 2187, 96),
               ("f32", 17, 19), ("f64", 17, 19), ("f32", 3, 2), ("f64", 3, 2)]


@pytest.mark.parametrize("prec,Ny,Nx", FLOW_SHAPES)
def test_flows_and_gradient_at_every_kernel_class(camb, prec, Ny, Nx, monkeypatch):
    """flows, adjoints and the delta-flow gradient against the oracle.  Single precision at the survey-patch bounds (TOL32_PATCH), doubled on sides
    above 1920, and there the four flows checked as in test_gpu_anysize.py test_longest_compile_time_plan_in_the_flows: the error of a thin patch
    grows with its long side (the device-side adjoint identity of test_lenseflow_ops, single-precision bound 2.5e-5, measured 4.0e-5 at 96 x 2050)"""
    long_side = prec == "f32" and max(Ny, Nx) > 1920
    if prec == "f32":
        monkeypatch.setitem(TP.TOL, "f32", {k: (2.0 if long_side else 1.0) * v for k, v in TOL32_PATCH.items()})
    if long_side:
        C = _pkg()
        tT, nT = DT[prec]
        tol = TP.TOL[prec]
        oproj, simf, simp = sims(camb, Ny, Nx, 2, 1)
        f, g, phi = simf(1).astype(nT).astype(np.float64), simf(11).astype(nT).astype(np.float64), simp(2, 1).astype(nT).astype(np.float64)
        OL = TP.OLenseFlow(oproj, phi, 7)
        p = C.ProjLambert(Ny, Nx, 2.0, tT)
        F = lambda a, b: C.Field(p, p.tensor(a), b)
        L = C.LenseFlow(p, 7)(F(phi, C.MAP))
        gl = O.rfft2(g)
        close("L*f", (L * F(f, C.MAP)).arr.cpu().numpy(), OL.apply(f), tol["flow"])
        close("L\\f", L.ldiv(F(f, C.MAP)).arr.cpu().numpy(), OL.inv(f), tol["flow"])
        close("L'g", (L.adjoint * F(gl, C.FOURIER)).arr.cpu().numpy(), OL.adj(gl), tol["adj"])
        close("L'\\g", L.adjoint.ldiv(F(gl, C.FOURIER)).arr.cpu().numpy(), OL.invadj(gl), tol["adj"])
    else:
        TP.test_lenseflow_ops(camb, prec, Ny, Nx, 2, 1, 1, 7)
    TP.test_lenseflow_gradient(camb, prec, Ny, Nx, 2, 1, 1, "fwd", 7)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_chirp_z_flows_equal_the_run_time_plans(camb, prec):
    """90 x 60 QU (both sides run-time plans) with every transform forced through the chirp-z kernel (CMBL_GEN_BLUESTEIN=1) against the default
    plans: flows, adjoint and the delta-flow gradient agree to rounding (single precision: the bounds of test_anysize_path_equals_fused_path)"""
    C = _pkg()
    tT, nT = DT[prec]
    Ny, Nx, P, n = 90, 60, 2, 7
    oproj, simf, simp = sims(camb, Ny, Nx, P, 1)
    f, g, phi = simf(1).astype(nT), simf(5).astype(nT), simp(2, 1).astype(nT)
    delta = O.rfft2(simf(7).astype(np.float64)).astype(np.complex64 if prec == "f32" else np.complex128)
    res = {}
    for forced in (0, 1):
        p = _ctx(C, Ny, Nx, tT, forced)
        F = lambda a, b: C.Field(p, p.tensor(a), b)
        L = C.LenseFlow(p, n)(F(phi, C.MAP))
        Lf = L * F(f, C.MAP)
        gdp, gdf, gf0 = L.gradient(C.FLOW_FWD, Lf, F(delta, C.FOURIER))
        res[forced] = [x.cpu().numpy() for x in (Lf.arr, L.ldiv(F(f, C.MAP)).arr, (L.adjoint * F(g, C.MAP).to(C.FOURIER)).arr, gdp.arr, gdf.arr, gf0.arr)]
    t32 = {"L*f": 1.1e-5, "L\\f": 1.1e-5, "L'g": 6.5e-5, "dphi": 1.5e-4, "df": 6.5e-5, "f0": 1.2e-6}
    for name, a, b in zip(("L*f", "L\\f", "L'g", "dphi", "df", "f0"), res[1], res[0]):
        close(f"chirp-z vs run-time plans {name}", a, b, t32[name] if prec == "f32" else 1e-12)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx", [(45, 75), (75, 45), (127, 60), (4094, 32), (91, 52), (5, 3)])
def test_reductions_and_diag_ops_off_the_fused_path(prec, Ny, Nx):
    """the reductions and operator applies of test_gpu_parity.py on the any-size path (kx in natural order): odd and even Ny (no Nyquist
    column at odd Ny: lam = 2 up to the last), a chirp-z side, big radices (91 = 7*13, 52 = 4*13) and a 5 x 3 map"""
    TP.reductions_and_diag_ops(prec, Ny, Nx)
