"""Time per conjugate-gradient iteration of the Wiener filter (argmaxf_logpdf, src/maximization.jl:17-42) with LenseFlow(7) and with BilinearLens in
the L slot of a data set, from one process: 1024^2 QU fp32 and 2048^2 QU fp64, B = 1 and B = 8 data slots against one phi, pixel mask on.

Variants, alternated, each repeated REPS times (median, spread = max - min and [min, max] of the repeats):
  (i)   LenseFlow(7) through cmbl_wiener_cg
  (ii)  BilinearLens as a CG loop written here from operations the library exported before the `_op` entry points existed (L * f, L.adjoint * g,
        diag_apply, map_fma, dot, axpby): the baseline; this variant also runs on a checkout without them
  (iii) BilinearLens through cmbl_wiener_cg_op, lens_fused = 0 (the composition from the stand-alone launches)
  (iv)  BilinearLens through cmbl_wiener_cg_op, lens_fused = 1 (gather / CSR row sum inside the column pass)
A solve is fixed-length (tol = 0); the time per iteration is the time of k solves of 12 iterations minus that of k solves of 4, over 8 k, with k chosen so
that the longer window lasts >= 0.5 s, every window synchronised (set-up and the first residual cancel in the difference).
Then one profiled solve of (iv): the share of the kernel class "lens_y" (cmbl_timer_report's classes), its bytes computed from shapes (per slice:
the table as the kernel fetches it -- 4 + 2 sizeof(T) bytes per pixel for L, 4 + 4 (4 + sizeof(T)) for the CSR of L' -- one map in, one mixed
plane out) over its kernel time, against the streaming-copy rate measured in this run.

    python tools/gpu_lensop_wf_time.py > profiles/lensop_wf_times.txt"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cmblensing_jl_amd as C      # noqa: E402
from bench import synthetic_cls    # noqa: E402

REPS, WINDOW = 3, 0.5
SIZES = [(1024, torch.float32, "fp32"), (2048, torch.float64, "fp64")]
if os.environ.get("LENSOP_WF_SMALL"):                       # rehearsal at a toy size
    SIZES, WINDOW = [(128, torch.float32, "fp32"), (64, torch.float64, "fp64")], 0.05
HAS_OP = hasattr(C.load_library(), "cmbl_wiener_cg_op")


def python_cg(ds, L, phi, d, nsteps):
    """conjugate_gradient (src/numerical_algorithms.jl:73-134) on A f = Cf^-1 f + L'B'M'Cn^-1 M B L f, b = L'B'M'Cn^-1 d, from Python calls"""
    p = ds.proj
    L(phi)

    def adj_data(z):                                          # L'B'M'Cn^-1 z  (harmonic)
        w = ds._applyT("B", ds._maskT(ds._apply("Cn_inv", z)), basis_out=C.FOURIER)
        return (L.adjoint * w.to(C.MAP)).to(C.HARMONIC)

    A = lambda f: ds._apply("Cf_inv", f) + adj_data(ds._mask(ds._apply("B", L * f.to(C.MAP))))
    b = adj_data(d)
    x = C.Field(p, torch.zeros_like(b.arr), C.HARMONIC)
    r = b
    z = ds._apply("precond_inv", r)
    pv = z
    res = r.dot(z)
    for _ in range(2, nsteps + 1):
        Ap = A(pv)
        alpha = res / pv.dot(Ap)
        x = p.axpby(1.0, x, alpha, pv)
        r = p.axpby(1.0, r, -alpha, Ap)
        z = ds._apply("precond_inv", r)
        res_new = r.dot(z)
        pv = p.axpby(1.0, z, res_new / res, pv)
        res = res_new
    return x


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


NLONG, NSHORT = 12, 4                                        # iterations of the two fixed-length solves (far from convergence: no 0 / 0 at tol = 0)


def per_iteration(solve):
    """(seconds per iteration, k): (T(k solves of NLONG) - T(k solves of NSHORT)) / (k (NLONG - NSHORT)) with the long window >= WINDOW"""
    solve(NSHORT)                                             # warm-up: code objects, scratch, tables
    k = 1
    while True:
        tl = wall(lambda: [solve(NLONG) for _ in range(k)])
        if tl >= WINDOW:
            break
        k = max(k + 1, int(np.ceil(k * 1.2 * WINDOW / max(tl, 1e-4))))
    ts = wall(lambda: [solve(NSHORT) for _ in range(k)])
    return (tl - ts) / (k * (NLONG - NSHORT)), k


def main():
    dev = torch.cuda.get_device_name(0)
    print(f"# Wiener-filter CG iteration, LenseFlow(7) and BilinearLens in the L slot; {dev}; pixel mask on; ms per iteration, median of {REPS} (spread = max - min)")
    a = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    copy_s = float(np.median([wall(lambda: b.copy_(a)) for _ in range(10)]))
    copy_rate = 2 * a.numel() * 4 / copy_s
    print(f"streaming copy (256 MB read + 256 MB write): {copy_s * 1e3:.3f} ms = {copy_rate / 1e9:.0f} GB/s")
    del a, b
    for N, T, tag in SIZES:
        s = C.load_sim(2.0, N, "P", synthetic_cls(), T=T, beam_fwhm=3.0, pixel_mask=dict(pad_deg=0.4, apod_deg=0.6), Nbatch=1, Nphi="flat")
        ds, p = s["ds"], s["proj"]
        LF, LB = ds.L, C.BilinearLens(p)
        phi = s["phi"]
        for B in (1, 8):
            d = C.Field(p, torch.cat([torch.roll(s["d"].arr, 5 * k, dims=2) * (1.0 + 0.1 * k) for k in range(B)]).contiguous(), C.HARMONIC)

            def native(L, fused):
                def solve(n):
                    ds.L = L
                    if fused is not None:
                        p.set_option("lens_fused", fused)
                    ds.argmaxf_logpdf(phi, d=d, tol=0.0, nsteps=n)
                return solve

            variants = [("(i)   LenseFlow(7), cmbl_wiener_cg", native(LF, None)),
                        ("(ii)  BilinearLens, CG loop from Python calls", lambda n: python_cg(ds, LB, phi, d, n))]
            if HAS_OP:
                variants += [("(iii) BilinearLens, cmbl_wiener_cg_op, lens_fused = 0", native(LB, 0)),
                             ("(iv)  BilinearLens, cmbl_wiener_cg_op, lens_fused = 1", native(LB, 1))]
            times = {name: [] for name, _ in variants}
            iters = {}
            for _ in range(REPS):
                for name, solve in variants:                  # alternated
                    t, n = per_iteration(solve)
                    times[name].append(t * 1e3)
                    iters[name] = n
            print(f"{N}^2 QU {tag}, B = {B}")
            med = {}
            for name, _ in variants:
                v = times[name]
                med[name] = float(np.median(v))
                print(f"  {name:58s} {med[name]:9.3f} ms   spread {max(v) - min(v):7.3f}   [{min(v):.3f}, {max(v):.3f}]   (k ={iters[name]} solves of {NLONG} and of {NSHORT} iterations)")
            base = [k for k in med if k.startswith("(ii)")][0]
            for name in med:
                if name != base:
                    print(f"  {name[:5]} against (ii): {med[base] / med[name]:6.2f} x")
            if HAS_OP:
                # kernel-class shares of one profiled solve of (iv)
                ds.L = LB
                p.set_option("lens_fused", 1)
                nprof = 12
                ds.argmaxf_logpdf(phi, d=d, tol=0.0, nsteps=nprof)
                p.prof_reset()
                p.prof_enable(True)
                ds.argmaxf_logpdf(phi, d=d, tol=0.0, nsteps=nprof)
                p.prof_enable(False)
                tab = p.prof_table()
                total = sum(ms for ms, _ in tab.values())
                ms, nl = tab.get("lens_y", (0.0, 0))
                sz = 4 if T == torch.float32 else 8
                S, npix, mpl = 2 * B, N * N, ((N // 2 + 1 + 3) & ~3) * N * 2 * sz
                per_fwd = S * (npix * (4 + 2 * sz) + npix * sz + mpl)
                per_adj = S * (npix * (4 + 4 * (4 + sz)) + npix * sz + mpl)
                nbytes = (nl // 2) * (per_fwd + per_adj)
                print(f"  profiled solve of (iv), {nprof} iterations: kernel time {total:.3f} ms in all classes; lens_y {ms:.3f} ms in {nl} launches = {100 * ms / max(total, 1e-9):.1f} % of the kernel time")
                if nl:
                    rate = nbytes / (ms * 1e-3)
                    print(f"  lens_y bytes from shapes (table per slice, map in, mixed plane out): {nbytes / 1e6:.1f} MB -> {rate / 1e9:.0f} GB/s = {rate / copy_rate:.2f} of the copy rate")
                top = sorted(tab.items(), key=lambda kv: -kv[1][0])[:6]
                print("  largest classes: " + ", ".join(f"{k} {v[0]:.3f} ms / {v[1]}" for k, v in top))
                p.set_option("lens_fused", 0)
            ds.L = LF
        del s, ds, LF, LB
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
