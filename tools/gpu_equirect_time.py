"""ProjEquiRect on the device: M * f (nbatch 1 and 8), M1 * M2 and the four transforms at Ny x Nx = 128 x 512 and 256 x 1024, I with real blocks and
QU (complex 2Ny blocks), fp32, each next to torch on the very same tensors (torch.einsum / torch.bmm: the installed rocBLAS path, the only
yardstick on the box).

The driver starts one child process per shape and spin under `timeout` and stops at the first failure.  A child warms every call up, then takes
REPS samples of it between two events on the stream the library uses; median and spread (min .. max).  M * f is reported as bytes of blocks / time
next to a device-to-device copy of the same bytes measured in the same process (read + write: 2 x bytes / time); M1 * M2 as real FLOP/s (8 n³
per complex block product, 2 n³ per real one).  These are records; nothing is asserted on them.

    python tools/gpu_equirect_time.py > profiles/equirect_times.txt"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SHAPES = ((128, 512), (256, 1024))
WARM, REPS = 3, 9
STEP_LIMIT = 240


def timed(fn):
    import torch
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def fmt(t):
    return f"{t[0]:9.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def step(Ny, Nx, spin):
    import torch
    sys.path.insert(0, ROOT)
    import cmblensing_jl_amd as C
    T = torch.float32
    p = C.ProjEquiRect(Ny, Nx, (np.pi / 2 - 0.2, np.pi / 2 + 0.2), (0.0, 2 * np.pi), T=T)
    Mh, n, cplx = Nx // 2 + 1, (Ny if spin == 0 else 2 * Ny), spin == 2
    g = torch.Generator(device=p.device).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, dtype=T, device=p.device, generator=g)
    blocks = (torch.complex(rnd(Mh, n, n), rnd(Mh, n, n)) if cplx else rnd(Mh, n, n)) / np.sqrt(n)
    M, M2 = C.BlockDiagEquiRect(blocks, p), C.BlockDiagEquiRect(blocks.flip(0).contiguous(), p)
    nbytes = blocks.numel() * blocks.element_size()
    print(f"{Ny} x {Nx} {'QU' if cplx else 'I '}: n = {n}, {Mh} blocks, {'complex' if cplx else 'real'}, {nbytes / 1e6:.1f} MB of blocks")
    dst = torch.empty_like(blocks)
    tc = timed(lambda: dst.copy_(blocks))
    print(f"  copy of the blocks (read + write)     {fmt(tc)}   {2 * nbytes / tc[0] / 1e6:8.1f} GB/s")
    for B in (1, 8):
        f = C.EquiRectField(p, torch.complex(rnd(B, Mh, n), rnd(B, Mh, n)), C.AZFOURIER)
        t1 = timed(lambda: M * f)
        bt = blocks.to(p.CT) if not cplx else blocks
        t2 = timed(lambda: torch.einsum("mqp,bmq->bmp", bt, f.arr))
        t3 = timed(lambda: M.H * f)
        err = float((torch.einsum("mqp,bmq->bmp", bt, f.arr) - (M * f).arr).abs().max())
        print(f"  M * f   B = {B}                          {fmt(t1)}   {nbytes / t1[0] / 1e6:8.1f} GB/s of blocks")
        print(f"  M' * f  B = {B}                          {fmt(t3)}   {nbytes / t3[0] / 1e6:8.1f} GB/s of blocks")
        print(f"  torch.einsum (blocks as complex)  B = {B} {fmt(t2)}   {bt.numel() * bt.element_size() / t2[0] / 1e6:8.1f} GB/s of ITS blocks   max |diff| {err:.2e}")
    flop = (8.0 if cplx else 2.0) * n ** 3 * Mh
    t1 = timed(lambda: M * M2)
    Ar, Br = blocks.transpose(1, 2), M2.blocks.transpose(1, 2)               # [m, p, q]
    t2 = timed(lambda: torch.bmm(Ar, Br))
    err = float((torch.bmm(Ar, Br).transpose(1, 2) - (M * M2).blocks).abs().max())
    print(f"  M1 * M2 (MFMA)                        {fmt(t1)}   {flop / t1[0] / 1e9:8.2f} TFLOP/s")
    print(f"  torch.bmm                             {fmt(t2)}   {flop / t2[0] / 1e9:8.2f} TFLOP/s   max |diff| {err:.2e}")
    for B in (1, 8):
        P = 1 if spin == 0 else 2
        m = C.EquiRectField(p, rnd(B, P, Nx, Ny), C.MAP)
        a = m.to(C.AZFOURIER)
        mb = m.arr.numel() * 4 + a.arr.numel() * 8
        tf, ti = timed(lambda: m.to(C.AZFOURIER)), timed(lambda: a.to(C.MAP))
        print(f"  Map -> AzFourier  B = {B}                {fmt(tf)}   {mb / tf[0] / 1e6:8.1f} GB/s of field in + out")
        print(f"  AzFourier -> Map  B = {B}                {fmt(ti)}   {mb / ti[0] / 1e6:8.1f} GB/s of field in + out")
        if spin == 0:
            tt = timed(lambda: torch.fft.rfft(m.arr, dim=2))
            print(f"  torch.fft.rfft along the same axis B = {B} {fmt(tt)}")
        else:
            z = torch.complex(m.arr[:, 0], m.arr[:, 1])
            tt = timed(lambda: torch.fft.fft(z, dim=1))
            print(f"  torch.fft.fft along the same axis  B = {B} {fmt(tt)}")
    sys.stdout.flush()


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--step":
        return step(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    import torch
    print(f"# ProjEquiRect, fp32 context, {torch.cuda.get_device_name(0)}; median (min .. max) of {REPS} event-timed calls after {WARM} warm-up calls")
    sys.stdout.flush()
    for Ny, Nx in SHAPES:
        for spin in (0, 2):
            r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", str(Ny), str(Nx), str(spin)])
            if r.returncode != 0:
                print(f"# step {Ny} x {Nx} spin {spin} ended with status {r.returncode}: stopping")
                sys.exit(r.returncode)


if __name__ == "__main__":
    main()
