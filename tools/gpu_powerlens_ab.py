"""PowerLens and Taylens next to LenseFlow(n = 7) and BilinearLens at 1024^2 QU fp32, B = 1 and B = 8, from one process: L*f of PowerLens and
Taylens at orders 2 and 4, PowerLens L'g, and L*f of LenseFlow(7) and BilinearLens, with the same ϕ (0.7 px rms per component) and the same f.

Timing: every operator and shape is warmed up first (3 calls); a sample is the host clock around REPS back-to-back calls that end in one device
synchronise, divided by REPS; the operators are visited in turn, ROUNDS times, so that a drift of the shared host touches all of them alike; the
table has the median and the spread (min .. max) of the samples in ms.  Each operator's distance from LenseFlow(7) on the same inputs (relative L2
of the lensed maps; white-noise f, for which a truncated Taylor series is at its worst, and a red-spectrum f, CMB-like) is recorded with the times.

    python tools/gpu_powerlens_ab.py > profiles/powerlens_times.txt"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cmblensing_jl_amd as C      # noqa: E402

N, THETA, P = 1024, 2.0, 2
REPS, ROUNDS, WARM = 10, 7, 3


def sample(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / REPS * 1e3


def red(rng, shape, power):
    k = np.hypot(np.fft.fftfreq(N)[:, None], np.fft.rfftfreq(N)[None, :])
    return np.fft.irfft2(np.fft.rfft2(rng.standard_normal(shape)) * np.where(k > 0, 1 / np.maximum(k, 1e-30) ** power, 0), s=(N, N))


def rel(a, b):
    return float(torch.linalg.norm((a - b).double().ravel()) / torch.linalg.norm(b.double().ravel()))


def main():
    p = C.ProjLambert(N, N, THETA, torch.float32)
    rng = np.random.default_rng(0)
    phi = red(rng, (N, N), 3)
    gy, gx = np.gradient(phi)
    phi *= 0.7 * np.deg2rad(THETA / 60) / np.sqrt(0.5 * (np.mean(gx ** 2) + np.mean(gy ** 2)))          # ~0.7 px rms per component
    phi = C.Field(p, p.tensor(phi[None, None]), C.MAP)
    ops = {"LenseFlow(7)": C.LenseFlow(p, 7), "BilinearLens": C.BilinearLens(p)}
    for o in (2, 4):
        ops[f"PowerLens({o})"], ops[f"Taylens({o})"] = C.PowerLens(p, o), C.Taylens(p, o)
    for L in ops.values():
        L(phi)
    print(f"# PowerLens / Taylens vs LenseFlow(7) and BilinearLens, {N}^2 QU fp32, {torch.cuda.get_device_name(0)}")
    print(f"# ms per call: median (min .. max) of {ROUNDS} samples of {REPS} back-to-back calls ending in one synchronise, operators interleaved")
    for B in (1, 8):
        f = C.Field(p, p.tensor(rng.standard_normal((B, P, N, N))), C.MAP)
        rows = [(name + " L*f", (lambda L=L: L * f)) for name, L in ops.items()]
        rows += [(f"PowerLens({o}) L'g", (lambda L=ops[f"PowerLens({o})"]: L._apply(C.FLOW_ADJ, f, basis_out=C.FOURIER))) for o in (2, 4)]
        for _, fn in rows:
            for _ in range(WARM):
                fn()
        ts = {name: [] for name, _ in rows}
        for _ in range(ROUNDS):
            for name, fn in rows:
                ts[name].append(sample(fn))
        print(f"B = {B}")
        ref = float(np.median(ts["LenseFlow(7) L*f"]))
        for name, _ in rows:
            m = float(np.median(ts[name]))
            print(f"  {name:20s} {m:8.3f}  ({min(ts[name]):.3f} .. {max(ts[name]):.3f})   LenseFlow(7) L*f / this = {ref / m:5.2f}")
    print("distance from LenseFlow(7) L*f on the same inputs (relative L2, B = 1)")
    for label, arr in (("white f", rng.standard_normal((1, P, N, N))), ("red f (k^-2)", red(rng, (1, P, N, N), 2))):
        f = C.Field(p, p.tensor(arr), C.MAP)
        want = (ops["LenseFlow(7)"] * f).arr
        print(f"  {label}: " + "  ".join(f"{name} {rel((L * f).arr, want):.2e}" for name, L in ops.items() if name != "LenseFlow(7)"))


if __name__ == "__main__":
    main()
