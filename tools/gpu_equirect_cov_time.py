"""Cℓ_to_Cov on ProjEquiRect on the device: `Cl_to_Cov("I")` and `Cl_to_Cov("P")` at Ny x Nx = 256 x 512 and 512 x 1024 with the reference's
spans (K = 3), ℓmax = 10 000, fp32 context (the arithmetic is double in either precision), in table mode (ngrid = 50 000, the default) and in
exact mode (ngrid = 0), next to oracle (a) of tests/_equirect_cov_ref.py on the host.

The host oracle is timed on SAMPLE ring pairs (all their K Nx separations, the same sums, periodisation and np.fft) and scaled to the number of
ring pairs the device computes -- the full oracle would run for hours at these sizes, like the reference's serial double loop; the line says so.
The driver starts one child process per shape, spin and mode under `timeout` and stops at the first failure.  Table mode: median and spread of
REPS wall-clock calls after WARM warm-up calls (the call synchronises its stream before it returns).  Exact mode: ONE call, no warm-up -- it is
the slow reference mode.  These are records; nothing is asserted on them.

    python tools/gpu_equirect_cov_time.py > profiles/equirect_cov_times.txt"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SHAPES = ((256, 512), (512, 1024))
LMAX, NGRID = 10_000, 50_000
WARM, REPS, SAMPLE = 1, 5, 16
STEP_LIMIT = 900


def step(Ny, Nx, pol, ngrid):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cmblensing_jl_amd as C
    import _equirect_cov_ref as R
    tt, ee, bb = R.camb_total(LMAX)
    p = C.ProjEquiRect(Ny, Nx, R.REF_THETA_SPAN, R.REF_PHI_SPAN, T=torch.float32)
    call = (lambda: C.Cl_to_Cov("I", p, tt, lmax=LMAX, ngrid=ngrid)) if pol == "I" else (lambda: C.Cl_to_Cov("P", p, ee, bb, lmax=LMAX, ngrid=ngrid))
    ts = []
    for i in range((WARM + REPS) if ngrid else 1):
        t = time.perf_counter()
        M = call()
        p.synchronize()
        if not ngrid or i >= WARM:
            ts.append(time.perf_counter() - t)
    npairs = Ny * (Ny + 1) // 2 if pol == "I" else Ny * Ny
    K = R.span_K(R.REF_PHI_SPAN)[0]
    mode = f"table, ngrid = {ngrid}" if ngrid else "exact (ngrid = 0)"
    print(f"{Ny} x {Nx} {pol}, {mode}: device {np.median(ts):10.4f} s ({min(ts):.4f} .. {max(ts):.4f}; {len(ts)} call(s))   "
          f"{npairs} ring pairs x {K * Nx} separations, {M.blocks.numel() * M.blocks.element_size() / 1e6:.1f} MB of blocks")
    # the host oracle on SAMPLE ring pairs, scaled
    theta = R.geometry(Ny, Nx, R.REF_THETA_SPAN, R.REF_PHI_SPAN)["theta"]
    rng = np.random.default_rng(1)
    j, k = rng.integers(0, Ny, SAMPLE), rng.integers(0, Ny, SAMPLE)
    t = time.perf_counter()
    table = None if not ngrid else (R.make_table(ngrid, tt) if pol == "I" else R.make_table(ngrid, ee, bb))
    t_table = time.perf_counter() - t
    t = time.perf_counter()
    h = R._separations(theta, K, Nx, j, k, np.float64)[0]
    c = R.correlation(h, tt if pol == "I" else ee, None if pol == "I" else bb, np.float64, table)
    for v in (c if pol == "P" else (c,)):
        np.fft.fft(R._periodise(v, K, Nx), axis=1)
    t_pairs = (time.perf_counter() - t) / SAMPLE
    print(f"    host oracle (a), NumPy float64: table {t_table:.2f} s + {t_pairs * 1e3:.3f} ms per ring pair (measured on {SAMPLE} pairs, without the "
          f"bearing phases) -> {t_table + t_pairs * npairs:.1f} s for {npairs} pairs (scaled, not run)")
    sys.stdout.flush()


def main():
    if len(sys.argv) == 6 and sys.argv[1] == "--step":
        return step(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5]))
    import torch
    print(f"# Cl_to_Cov on ProjEquiRect, lmax = {LMAX}, fp32 context, {torch.cuda.get_device_name(0)}; wall clock of whole calls")
    sys.stdout.flush()
    for ngrid in (NGRID, 0):                                                 # the table mode of every size first: the exact mode may hit the limit
        for Ny, Nx in SHAPES:
            for pol in "IP":
                r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", str(Ny), str(Nx), pol, str(ngrid)])
                if r.returncode != 0:
                    print(f"# step {Ny} x {Nx} {pol} ngrid {ngrid} ended with status {r.returncode}: stopping")
                    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
