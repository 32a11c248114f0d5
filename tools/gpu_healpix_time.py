"""The HEALPix projection at Nside 2048 <-> 1024^2 (1' pixels, rotator (0, 90, 0)), fp32 and fp64, I and QU, next to a `torch` gather of the
very same tables.

Per precision (one child process each, under a time limit; the parent stops at the first failure): the construction of the `Projector` (host
clock around the call, which synchronises), then per direction and spin the device time of one `project` call with a cached projector --
WARM calls first, then REPS samples of the host clock around ITERS back-to-back calls between two synchronises -- as median (min .. max) in
microseconds and as bytes / time, bytes = the tables read once plus four gathered values and one stored value per output element and slice.
The `torch` lines do the same arithmetic with `index_select`, a multiply and a sum over the four (pixels, weights) of tests/_healpix_ref.py,
the restatement's tables for the same projector (QU rotation not included: they are a floor for a framework gather, not a competitor).

These times are records; nothing is asserted on them.  Appends to profiles/healpix_times.txt:

    python tools/gpu_healpix_time.py"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
OUT = os.path.join(ROOT, "profiles", "healpix_times.txt")
NSIDE, N, THETA = 2048, 1024, 1.0
WARM, REPS, ITERS = 3, 7, 20
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
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cmblensing_jl_amd as C
    import _healpix_ref as R
    T = torch.float32 if prec == "f32" else torch.float64
    el = 4 if prec == "f32" else 8
    p = C.ProjLambert(N, N, THETA, T)
    hp = C.ProjHealpix(NSIDE)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    P = C.Projector(hp, p)
    t_build = (time.perf_counter() - t0) * 1e3
    print(f"{prec}: Projector(Nside {NSIDE} => {N}^2 at {THETA}') built in {t_build:.1f} ms (scan of {hp.npix} pixels in double); "
          f"{P.n_in_patch} pixels in the patch, {P.n_touched} touched", flush=True)
    ncart, nt = N * N, P.n_touched
    # the same tables for torch: the restatement's ring lookup at the device's own (θ, ϕ), and the flat corners of the device's own (i, j)
    pix, w = R.interp_weights(NSIDE, P.thetas, P.phis)
    pix_t = torch.from_numpy(pix).to(p.device)
    w_t = torch.from_numpy(w).to(device=p.device, dtype=T)
    i, j = P.is_, P.js
    corners, cw = [], []
    for y, wy in ((np.floor(i), 1 - i + np.floor(i)), (np.ceil(i), i - np.floor(i))):
        for x, wx in ((np.floor(j), 1 - j + np.floor(j)), (np.ceil(j), j - np.floor(j))):
            ok = (y >= 1) & (y <= N) & (x >= 1) & (x <= N)
            corners.append(np.where(ok, (x - 1) * N + (y - 1), 0).astype(np.int64))
            cw.append(np.where(ok, wy * wx, 0.0))
    c_t = torch.from_numpy(np.stack(corners)).to(p.device)
    cw_t = torch.from_numpy(np.stack(cw)).to(device=p.device, dtype=T)
    touched_t = torch.from_numpy(P.touched).to(p.device)
    g = torch.Generator(device="cpu").manual_seed(0)
    for npol, name in ((1, "I"), (2, "QU")):
        h = C.HealpixField(hp, torch.randn((1, npol, hp.npix), generator=g, dtype=T).to(p.device), name)
        m = C.Field(p, torch.randn((1, npol, N, N), generator=g, dtype=T).to(p.device), C.MAP)
        b_cart = ncart * (16 + 4 * el + 2 * el) + npol * ncart * 5 * el
        b_hpx = nt * (4 + 16 + 2 * el) + npol * (nt * 5 * el + hp.npix * el)
        rows = [
            ("to_cart    device", lambda: P.to_cart(h), b_cart),
            ("to_cart    torch ", lambda: sum(w_t[k] * h.arr[0].index_select(1, pix_t[k]) for k in range(4)), b_cart),
            ("to_healpix device", lambda: P.to_healpix(m), b_hpx),
            ("to_healpix torch ", lambda: torch.zeros((npol, hp.npix), dtype=T, device=p.device).index_copy_(
                1, touched_t, sum(cw_t[k] * m.arr[0].reshape(npol, -1).index_select(1, c_t[k]) for k in range(4))), b_hpx),
        ]
        for label, fn, nbytes in rows:
            med, lo, hi = timed(fn, torch)
            print(f"  {prec} {name:2s} {label}  {med:9.1f} us  ({lo:.1f} .. {hi:.1f})   {nbytes / med / 1e3:8.1f} GB/s of {nbytes / 1e6:.1f} MB", flush=True)


def main():
    if len(sys.argv) > 1:
        child(sys.argv[1])
        return
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(f"# HEALPix projection, Nside {NSIDE} <-> {N}^2 at {THETA}', {time.strftime('%Y-%m-%d')}; us per call, median (min .. max) of {REPS} x {ITERS} calls\n")
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
