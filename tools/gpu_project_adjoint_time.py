"""The four pullbacks of the HEALPix projection at Nside 2048 <-> 1024^2 (1' pixels, rotator (0, 90, 0): the size of tools/gpu_healpix_time.py
and tools/gpu_nfft_time.py), fp32 and fp64, I and QU, each next to the FORWARD of the opposite direction on the same projector -- the call
that moves data the same way (to_cartᵀ and to_healpix both end on the sphere, to_healpixᵀ and to_cart both end on the patch).

Per precision (one child process each, under a time limit; the parent stops at the first failure) and method: the construction of the
projector, the FIRST adjoint call of each direction (host clock; it builds and caches the transposed table of the bilinear method, on the
host, and synchronises), then the device time of one call with everything cached -- WARM calls first, then REPS samples of the host clock
around ITERS back-to-back calls between two synchronises -- as median (min .. max) in microseconds.

These times are records; nothing is asserted on them.  Appends to profiles/project_adjoint_times.txt:

    python tools/gpu_project_adjoint_time.py"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
OUT = os.path.join(ROOT, "profiles", "project_adjoint_times.txt")
NSIDE, N, THETA = 2048, 1024, 1.0
WARM, REPS, ITERS = 3, 7, 10
CHILD_LIMIT = 420


def timed(fn, torch):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ITERS):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / ITERS * 1e6)
    return np.median(ts), min(ts), max(ts)


def child(prec):
    import torch
    sys.path.insert(0, ROOT)
    import cmblensing_jl_amd as C
    T = torch.float32 if prec == "f32" else torch.float64
    p = C.ProjLambert(N, N, THETA, T)
    hp = C.ProjHealpix(NSIDE)
    g = torch.Generator(device="cpu").manual_seed(0)
    for method in ("bilinear", "nfft"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P = C.Projector(hp, p, method=method)
        print(f"{prec} {method}: Projector(Nside {NSIDE} => {N}^2 at {THETA}') built in {(time.perf_counter() - t0) * 1e3:.1f} ms; "
              f"{P.n_in_patch} pixels in the patch, {P.n_touched} touched", flush=True)
        first = True
        for npol, name in ((1, "I"), (2, "QU")):
            h = C.HealpixField(hp, torch.randn((1, npol, hp.npix), generator=g, dtype=T).to(p.device), name)
            m = C.Field(p, torch.randn((1, npol, N, N), generator=g, dtype=T).to(p.device), C.MAP)
            if first:
                for label, fn in (("to_cart^T", lambda: P.to_cart_adjoint(m)), ("to_healpix^T", lambda: P.to_healpix_adjoint(h))):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    print(f"  {prec} {method} first {label} call (tables built and cached): {(time.perf_counter() - t0) * 1e3:.1f} ms", flush=True)
                first = False
            rows = [("to_cart^T   ", lambda: P.to_cart_adjoint(m), "to_healpix  ", lambda: P.to_healpix(m)),
                    ("to_healpix^T", lambda: P.to_healpix_adjoint(h), "to_cart     ", lambda: P.to_cart(h))]
            for la, fa, lf, ff in rows:
                med, lo, hi = timed(fa, torch)
                medf, lof, hif = timed(ff, torch)
                print(f"  {prec} {method:8s} {name:2s} {la} {med:9.1f} us ({lo:.1f} .. {hi:.1f})   {lf} {medf:9.1f} us ({lof:.1f} .. {hif:.1f})   "
                      f"ratio {med / medf:.2f}", flush=True)


def main():
    if len(sys.argv) > 1:
        child(sys.argv[1])
        return
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(f"# pullbacks of the HEALPix projection, Nside {NSIDE} <-> {N}^2 at {THETA}', {time.strftime('%Y-%m-%d')}; us per call, "
                f"median (min .. max) of {REPS} x {ITERS} calls; each adjoint next to the forward of the opposite direction\n")
        for prec in ("f32", "f64"):
            r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), prec], capture_output=True, text=True)
            f.write(r.stdout)
            f.flush()
            print(r.stdout, end="")
            if r.returncode != 0:
                f.write(f"# {prec}: child ended with status {r.returncode}; stopping\n{r.stderr[-2000:]}\n")
                print(r.stderr[-2000:], file=sys.stderr)
                sys.exit(r.returncode)


if __name__ == "__main__":
    main()
