"""BilinearLens next to LenseFlow(n = 7) at 1024^2 QU fp32, B = 1 and B = 8, from one process: set_phi, L*f, L'g and L\\f of both operators (median
wall time of synchronised calls), the ratio to LenseFlow (the reference documents "at least an order of magnitude" for * and '), and the bytes of
the gather and of the transposed gather over their time against the streaming-copy rate of the part measured here (a device-to-device copy of
256 MB, read + write).  Bytes counted: the table (12 B per pixel; the CSR of the transpose: 36 B per pixel) plus the P*B maps in and out.

    python tools/gpu_bilinear_ab.py > profiles/bilinear_times.txt"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cmblensing_jl_amd as C      # noqa: E402

N, THETA, P = 1024, 2.0, 2


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    p = C.ProjLambert(N, N, THETA, torch.float32)
    rng = np.random.default_rng(0)
    k = np.hypot(np.fft.fftfreq(N)[:, None], np.fft.rfftfreq(N)[None, :])
    phi = np.fft.irfft2(np.fft.rfft2(rng.standard_normal((N, N))) * np.where(k > 0, 1 / np.maximum(k, 1e-30) ** 3, 0), s=(N, N))
    gy, gx = np.gradient(phi)
    phi *= 0.7 * np.deg2rad(THETA / 60) / np.sqrt(0.5 * (np.mean(gx ** 2) + np.mean(gy ** 2)))          # ~0.7 px rms per component
    a = torch.empty(64 << 20, dtype=torch.float32, device=p.device)
    b = torch.empty_like(a)
    copy_ms = timed(lambda: b.copy_(a))
    copy_rate = 2 * a.numel() * 4 / (copy_ms * 1e-3) / 1e9
    print(f"# BilinearLens vs LenseFlow(7), {N}^2 QU fp32, {torch.cuda.get_device_name(0)}; median of 20 synchronised calls, ms")
    print(f"streaming copy (256 MB read + 256 MB write): {copy_ms:.3f} ms = {copy_rate:.0f} GB/s")
    phis = [C.Field(p, p.tensor(phi[None, None] * s), C.MAP) for s in (1.0, 1.0)]
    LB, LF = C.BilinearLens(p), C.LenseFlow(p, 7)
    flip = [0]

    def set_phi(L):
        flip[0] ^= 1
        L(phis[flip[0]])                                              # a different object each call: the tables are rebuilt
    print(f"set_phi: BilinearLens {timed(lambda: set_phi(LB)):.3f}  LenseFlow {timed(lambda: set_phi(LF)):.3f}")
    for B in (1, 8):
        f = C.Field(p, p.tensor(rng.standard_normal((B, P, N, N))), C.MAP)
        g = C.Field(p, p.tensor(rng.standard_normal((B, P, N, N))), C.MAP)
        LB(phis[0]), LF(phis[0])
        ft = LB * f
        rows = [("L*f", lambda: LB * f, lambda: LF * f), ("L'g", lambda: LB._apply(C.FLOW_ADJ, g), lambda: LF._apply(C.FLOW_ADJ, g, basis_out=C.MAP)),
                ("L\\f", lambda: LB.ldiv(ft), lambda: LF.ldiv(ft))]
        print(f"B = {B}")
        for name, fb, ff in rows:
            tb, tf = timed(fb), timed(ff)
            line = f"  {name:5s} BilinearLens {tb:8.3f}  LenseFlow {tf:8.3f}  ratio {tf / tb:6.1f} x"
            if name != "L\\f":
                nbytes = N * N * ((12 if name == "L*f" else 36) + 2 * 4 * P * B)
                line += f"   {nbytes / (tb * 1e-3) / 1e9:6.0f} GB/s = {nbytes / (tb * 1e-3) / 1e9 / copy_rate:.2f} of the copy rate"
            print(line)


if __name__ == "__main__":
    main()
