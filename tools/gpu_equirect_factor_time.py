"""The factorisations of BlockDiagEquiRect, host path against device path at the same commit: `svd -> sqrt + pinv` (one call of
cmbl_equirect_block_svd with both outputs; on the host numpy.linalg.svd and the two products), `logabsdet` and `solve(M, M)`, on the `:I` (real
n = Ny) and `:P` (complex n = 2 Ny) blocks of `Cl_to_Cov` (ℓmax = 10 000, the reference's spans, fp32 context: the arithmetic is double in either
precision) at Ny x Nx = 64 x 128, 256 x 512 and 512 x 1024.

The host is timed on a SAMPLE of the blocks where the whole operator would take minutes and scaled to all Nx/2+1 of them; `--max-blocks` does the
same on the device (the sampled blocks go through a projection with fewer azimuthal modes: a block's cost depends on n alone, but fewer blocks than
CUs leave most of the chip idle, so such a figure is no throughput).  Every scaled figure is labelled.  The driver starts one child process per
size and block type under a time limit and stops at the first failure.  These are records; nothing is asserted on them.

    python tools/gpu_equirect_factor_time.py [--sizes 64x128,256x512] [--max-blocks 8]      (writes profiles/equirect_factor_time.json)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SIZES = "64x128,256x512,512x1024"
LMAX, REPS, HOST_BUDGET = 10_000, 3, 2.0e10           # host: sample the blocks when Mh n^3 (x 4 for complex) exceeds the budget
STEP_LIMIT = 1500


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def step(Ny, Nx, pol, max_blocks):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cmblensing_jl_amd as C
    import _equirect_cov_ref as R
    tt, ee, bb = R.camb_total(LMAX)
    p = C.ProjEquiRect(Ny, Nx, R.REF_THETA_SPAN, R.REF_PHI_SPAN, T=torch.float32)
    M = C.Cl_to_Cov("I", p, tt, lmax=LMAX) if pol == "I" else C.Cl_to_Cov("P", p, ee, bb, lmax=LMAX)
    Mh, n = p.Mh, M.n
    rec = {"Ny": Ny, "Nx": Nx, "pol": pol, "n": n, "blocks": Mh, "complex": M.complex}
    # device: all blocks, or the first `max_blocks` through a projection with that many azimuthal modes
    nd = Mh if not max_blocks or max_blocks >= Mh else max(2, max_blocks)
    q = p if nd == Mh else C.ProjEquiRect(Ny, 2 * (nd - 1), R.REF_THETA_SPAN, R.REF_PHI_SPAN, T=torch.float32)
    blocks = M.blocks[:nd].contiguous()
    fresh = lambda: C.BlockDiagEquiRect(blocks, q, factor_on="device")      # a new operator per call: nothing comes from a cache
    dev = {}
    for name, fn in (("svd_sqrt_pinv", lambda: fresh()._device_svd(C.equirect.PINV_RTOL, True, True)), ("logabsdet", lambda: fresh().logabsdet()),
                     ("solve", lambda: (lambda A: A.solve(A))(fresh()))):
        try:
            fn()                                                             # warm-up (every call synchronises its stream before it returns)
            dev[name] = timed(fn, REPS) * Mh / nd
        except Exception as e:                                               # e.g. a block that has not converged: recorded, not hidden
            dev[name] = None
            rec.setdefault("device_errors", {})[name] = str(e)
    rec["device_s"], rec["device_blocks_timed"], rec["device_scaled"] = dev, nd, nd != Mh
    # host: numpy.linalg in float64 as equirect.py calls it, on a sample of the blocks where the operator is large
    nh = Mh if Mh * n ** 3 * (4 if M.complex else 1) <= HOST_BUDGET else 4
    a = C.BlockDiagEquiRect(M.blocks[:nh].contiguous(), p if nh == Mh else C.ProjEquiRect(Ny, 2 * (nh - 1), R.REF_THETA_SPAN, R.REF_PHI_SPAN, T=torch.float32))._host()

    def host_svd():
        u, s, vh = np.linalg.svd(a)
        (u * np.sqrt(s)[:, None, :]) @ vh
        np.linalg.pinv(a, rcond=C.equirect.PINV_RTOL)

    rec["host_s"] = {"svd_sqrt_pinv": timed(host_svd, 1) * Mh / nh, "logabsdet": timed(lambda: np.linalg.slogdet(a), 1) * Mh / nh,
                     "solve": timed(lambda: np.linalg.solve(a, a), 1) * Mh / nh}
    rec["host_blocks_timed"], rec["host_scaled"] = nh, nh != Mh
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=SIZES)
    ap.add_argument("--max-blocks", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equirect_factor_time.json"))
    ap.add_argument("--step", nargs=3)
    a = ap.parse_args()
    if a.step:
        step(int(a.step[0]), int(a.step[1]), a.step[2], a.max_blocks)
        return 0
    recs = []
    for size in a.sizes.split(","):
        Ny, Nx = (int(v) for v in size.split("x"))
        for pol in "IP":
            r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--max-blocks", str(a.max_blocks),
                                "--step", str(Ny), str(Nx), pol], capture_output=True, text=True)
            sys.stderr.write(r.stderr[-2000:])
            if r.returncode != 0:
                print(f"{size} {pol}: the step ended with status {r.returncode}; stopping", flush=True)
                return r.returncode
            rec = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RECORD "))[7:])
            recs.append(rec)
            lab = lambda scaled, k: f" (scaled from {k} blocks)" if scaled else ""
            for op in ("svd_sqrt_pinv", "logabsdet", "solve"):
                d, h = rec["device_s"][op], rec["host_s"][op]
                print(f"{size} {pol} n = {rec['n']:4d} x {rec['blocks']} blocks  {op:14s} device {'failed' if d is None else f'{d:10.4f} s'}"
                      f"{lab(rec['device_scaled'], rec['device_blocks_timed'])}   host {h:10.4f} s{lab(rec['host_scaled'], rec['host_blocks_timed'])}", flush=True)
    json.dump({"tool": "tools/gpu_equirect_factor_time.py", "lmax": LMAX, "reps": REPS, "context": "float32", "records": recs}, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
