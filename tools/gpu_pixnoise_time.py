"""Cost of a map-diagonal noise covariance (CMBL_OP_CN_INV_PIX, load_sim(noise_var_map=...)) at 1024^2 QU fp32, LenseFlow(7), border mask, from one
process: one conjugate-gradient iteration of the Wiener filter (argmaxf_logpdf, src/maximization.jl:17-42) and one gradient of logpdf(Mixed)
(the "∇lnP" step), each under

  (a) Fourier-diagonal noise, fused posterior and fused CG (option fused_harm = 1: the default path of a data set without the new operator)
  (b) Fourier-diagonal noise, fused_harm = 0: the composed forms, which are what a data set with pixel noise runs
  (c) pixel noise: the composed forms with pinv(Cn) as the three-launch sandwich (row carrier, k_y_weight, row carrier)

on ONE data set (the operator is set and cleared, the option flipped), alternated, REPS times each (median, spread = max - min).  (b) is the
composed path as it was before the operator existed, measured by the same library in the same run: (c) / (b) is the cost of the sandwich, the
target is (c) <= 1.10 (b).  (c) / (a) is what giving up the fused forms costs; it is reported, not bounded.
CG: a solve is fixed-length (tol = 0); the time per iteration is (k solves of 12 iterations - k solves of 4) / 8k with the longer window >= 0.5 s.
Then the per-kernel-class times (cmbl_timer_report's classes) of one profiled 12-iteration solve of (b) and of (c).

    python tools/gpu_pixnoise_time.py        (prints its table)

Has been run on MI355X: DESIGN.md §5 has the figures."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cmblensing_jl_amd as C      # noqa: E402
from bench import synthetic_cls    # noqa: E402

REPS, WINDOW, N, T = 3, 0.5, 1024, torch.float32
if os.environ.get("PIXNOISE_SMALL"):                        # rehearsal at a toy size
    WINDOW, N = 0.05, 128
NLONG, NSHORT = 12, 4


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def per_call(fn, nlong=1, nshort=0):
    """seconds per unit: (T(k fn(nlong)) - T(k fn(nshort))) / (k (nlong - nshort)), the long window >= WINDOW; nshort = 0: no short window"""
    fn(nshort or nlong)
    k = 1
    while True:
        tl = wall(lambda: [fn(nlong) for _ in range(k)])
        if tl >= WINDOW:
            break
        k = max(k + 1, int(np.ceil(k * 1.2 * WINDOW / max(tl, 1e-4))))
    ts = wall(lambda: [fn(nshort) for _ in range(k)]) if nshort else 0.0
    return (tl - ts) / (k * (nlong - nshort))


def main():
    print(f"# pixel-diagonal noise against Fourier-diagonal noise; {torch.cuda.get_device_name(0)}; {N}^2 QU fp32, LenseFlow(7), border mask; ms, median of {REPS} (spread = max - min)")
    x, y = np.linspace(0, 1, N)[:, None], np.linspace(0, 1, N)[None, :]
    V = np.stack([7.5 * (1 + 29 * (0.5 + 0.5 * np.sin(2 * np.pi * (x * (k + 1) + y)))) for k in range(2)])
    s = C.load_sim(2.0, N, "P", synthetic_cls(), T=T, beam_fwhm=3.0, pixel_mask=dict(pad_deg=0.4, apod_deg=0.6), Nbatch=1, Nphi="flat", noise_var_map=V)
    ds, p, phi = s["ds"], s["proj"], s["phi"]
    w = ds.ops["Cn_inv_pix"].clone()
    fo, po = ds.mix(s["f"], phi)

    def mode(name):
        ds.set_op("Cn_inv_pix", w if name == "c" else None)
        p.set_option("fused_harm", 1 if name == "a" else 0)

    names = {"a": "(a) Fourier noise, fused", "b": "(b) Fourier noise, fused_harm = 0", "c": "(c) pixel noise"}
    work = {"CG iteration": lambda n: ds.argmaxf_logpdf(phi, tol=0.0, nsteps=n), "grad logpdf(Mixed)": lambda n: ds.gradient_logpdf_mixed(fo, po)}
    times = {(wk, m): [] for wk in work for m in names}
    try:
        for _ in range(REPS):
            for m in names:                                   # alternated
                mode(m)
                times[("CG iteration", m)].append(per_call(work["CG iteration"], NLONG, NSHORT) * 1e3)
                times[("grad logpdf(Mixed)", m)].append(per_call(work["grad logpdf(Mixed)"]) * 1e3)
        for wk in work:
            med = {m: float(np.median(times[(wk, m)])) for m in names}
            print(wk)
            for m in names:
                v = times[(wk, m)]
                print(f"  {names[m]:36s} {med[m]:9.3f} ms   spread {max(v) - min(v):7.3f}")
            print(f"  (c) / (b) = {med['c'] / med['b']:.3f}   (target <= 1.10)      (c) / (a) = {med['c'] / med['a']:.3f}   (reported)")
        for m in ("b", "c"):
            mode(m)
            ds.argmaxf_logpdf(phi, tol=0.0, nsteps=NLONG)
            p.prof_reset()
            p.prof_enable(True)
            ds.argmaxf_logpdf(phi, tol=0.0, nsteps=NLONG)
            p.prof_enable(False)
            tab = p.prof_table()
            print(f"profiled {NLONG}-iteration solve of {names[m]}: kernel time {sum(ms for ms, _ in tab.values()):.3f} ms in {sum(n for _, n in tab.values())} launches")
            print(p.timer_report())
    finally:
        mode("c")
        p.set_option("fused_harm", 1)


if __name__ == "__main__":
    main()
