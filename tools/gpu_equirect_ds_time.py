#!/usr/bin/env python
"""Times one CG iteration of cmbl_eqds_wiener_cg (the Wiener filter of a data set on ProjEquiRect, all on the device) next to the same iteration
composed in Python from the entry points that existed before it: cmbl_equirect_block_apply and cmbl_equirect_convert through `BlockDiagEquiRect`
/ `EquiRectField`, torch for the pointwise steps, `EquiRectField.dot` (two transforms and a host read-back) for the dots.  Not part of any test.

Sizes 64 x 128 and 512 x 1024, I and QU, float32, nbatch 1 and 8; mask, beam and a variance map present.  The operators are synthetic (identity plus
a small random part: positive definite, so the residuals stay finite and no iteration becomes a no-op); their values do not matter for the time.
ms per iteration = (time of a solve of K2 steps - time of a solve of K1 steps) / (K2 - K1), which removes the set-up; tol = 0 so no solve stops
early.  Each figure: one warm-up, then `--repeats` repeats; the median and the min-max spread are reported, and the block bytes an iteration reads
(|Cf^-1| + 2 |B| + |P^-1|) divided by the median time.

    python tools/gpu_equirect_ds_time.py [--sizes 64x128,512x1024] [--repeats 5] [--json out.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cmblensing_jl_amd as C  # noqa: E402
from cmblensing_jl_amd.engine import MAP, _ptr  # noqa: E402
from cmblensing_jl_amd.lib import check  # noqa: E402

_PD = ctypes.POINTER(ctypes.c_double)


def blocks(p, n, cplx, scale, gen):
    """scale * (I + small Hermitian-free random part), on the device; columns 0 and Nx/2 are left as they are (values do not matter for the time)"""
    b = 0.02 / np.sqrt(n) * torch.randn((p.Mh, n, n), dtype=p.CT if cplx else p.T, device=p.device, generator=gen)
    b += torch.eye(n, dtype=b.dtype, device=p.device)[None]
    return C.BlockDiagEquiRect(b * scale, p)


def setup(Ny, Nx, spin, B):
    p = C.ProjEquiRect(Ny, Nx, (1.0, 2.0), (0.0, 2 * np.pi), T=torch.float32)
    gen = torch.Generator(device=p.device).manual_seed(1)
    P = 1 if spin == 0 else 2
    n = P * Ny
    ops = {"CfI": blocks(p, n, spin == 2, 1.0, gen), "B": blocks(p, n, spin == 2, 0.7, gen), "PI": blocks(p, n, spin == 2, 0.4, gen)}
    x = torch.linspace(0, 1, Nx, device=p.device)[:, None] * torch.ones(Ny, device=p.device)[None]
    ops["M"] = (0.5 - 0.5 * torch.cos(2 * np.pi * x)).to(p.T).expand(P, Nx, Ny).contiguous()
    ops["CnI"] = (1.0 / (0.25 * (1 + 0.5 * torch.sin(2 * np.pi * x)))).to(p.T).expand(P, Nx, Ny).contiguous()
    ops["d"] = torch.randn((B, P, Nx, Ny), dtype=p.T, device=p.device, generator=gen)
    h = ctypes.c_void_p()
    check(p.lib.cmbl_eqds_create(p._h, P, ctypes.byref(h)))
    for which, k in ((0, "CfI"), (1, "B"), (2, "PI")):
        check(p.lib.cmbl_eqds_set_block_op(h, which, _ptr(ops[k].blocks), int(ops[k].complex), n))
    check(p.lib.cmbl_eqds_set_pixel_op(h, 0, _ptr(ops["M"]), P))
    check(p.lib.cmbl_eqds_set_pixel_op(h, 1, _ptr(ops["CnI"]), P))
    return p, h, ops, P, n


def fused_solve(p, h, ops, P, n, B, steps):
    out = torch.empty((B, p.Mh, n), dtype=p.CT, device=p.device)
    hist, nit = np.empty((steps, B)), ctypes.c_int(0)
    check(p.lib.cmbl_eqds_wiener_cg(h, _ptr(ops["d"]), None, 0.0, steps, _ptr(out), hist.ctypes.data_as(_PD), ctypes.byref(nit), B))
    assert nit.value == steps and np.all(np.isfinite(hist)), "a solve stopped early or left the finite range: its time would not be that of its steps"
    return hist


def composed_solve(p, h, ops, P, n, B, steps):
    """the reference's conjugate_gradient (src/numerical_algorithms.jl:73-134) on the Python surface, one scalar for the whole batch as `dot` gives it"""
    F = lambda a, basis: C.EquiRectField(p, a, basis)
    W = ops["M"] * ops["CnI"] * ops["M"]

    def A(x):
        t = (ops["B"] * x).to(MAP)
        return F((ops["CfI"] * x).arr + (ops["B"].H * F(t.arr * W[None], MAP)).arr, C.AZFOURIER)

    b = ops["B"].H * F(ops["d"] * (ops["M"] * ops["CnI"])[None], MAP)
    x, r = F(torch.zeros_like(b.arr), C.AZFOURIER), b
    z = ops["PI"] * r
    pv, res = z, r.dot(z)
    for _ in range(2, steps + 1):
        Ap = A(pv)
        alpha = res / pv.dot(Ap)
        x, r = x + pv * alpha, r - Ap * alpha
        z = ops["PI"] * r
        res2 = r.dot(z)
        pv = z + pv * (res2 / res)
        res = res2
    p.synchronize()
    return res


def per_iteration(fn, args, k1, k2, repeats):
    def timed(k):
        args[0].synchronize()
        t0 = time.perf_counter()
        fn(*args, k)
        args[0].synchronize()
        return time.perf_counter() - t0
    timed(k1)                                                                # warm-up: scratch, transform plans, code objects
    ms = sorted(1e3 * (timed(k2) - timed(k1)) / (k2 - k1) for _ in range(repeats))
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64x128,512x1024")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for size in a.sizes.split(","):
        Ny, Nx = (int(v) for v in size.split("x"))
        k1, k2 = 4, 24
        for spin in (0, 2):
            for B in (1, 8):
                p, h, ops, P, n = setup(Ny, Nx, spin, B)
                args = (p, h, ops, P, n, B)
                bytes_it = sum(ops[k].blocks.numel() * ops[k].blocks.element_size() * w for k, w in (("CfI", 1), ("B", 2), ("PI", 1)))
                fused = per_iteration(fused_solve, args, k1, k2, a.repeats)
                comp = per_iteration(composed_solve, args, k1, k2, a.repeats)
                row = {"Ny": Ny, "Nx": Nx, "spin": spin, "nbatch": B, "block_bytes_per_iteration": bytes_it, "fused": fused, "composed": comp,
                       "fused_GBps": bytes_it / fused["median_ms"] / 1e6, "composed_GBps": bytes_it / comp["median_ms"] / 1e6}
                rows.append(row)
                print(f"{Ny}x{Nx} spin {spin} B {B}: fused {fused['median_ms']:.3f} ms/it [{fused['min_ms']:.3f}, {fused['max_ms']:.3f}] ({row['fused_GBps']:.0f} GB/s of blocks); "
                      f"composed {comp['median_ms']:.3f} ms/it [{comp['min_ms']:.3f}, {comp['max_ms']:.3f}] ({row['composed_GBps']:.0f} GB/s)", flush=True)
                check(p.lib.cmbl_eqds_destroy(h))
                del ops, p
                torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
