"""The non-uniform-FFT method of the HEALPix projection at Nside 2048 <-> 1024^2 (1' pixels, rotator (0, 90, 0)), fp32 and fp64, I and QU, both
directions, next to the bilinear projector of the same pair.

Per precision (one child process each, under a time limit; the parent stops at the first failure): a streaming-copy rate (device-to-device
copy of 256 MiB, bytes read + written over time), the construction of both projectors (host clock around the call, which synchronises), then
per direction and spin
  * the device time of one `project` call with a cached projector -- WARM calls first, then REPS samples of the host clock around ITERS
    back-to-back calls between two synchronises -- as median (min .. max) in microseconds, for "nfft" and for "bilinear";
  * the stages of the "nfft" call: the library's per-launch event timing (cmbl_prof_*) of the context gives the node kernel (nfft_spread or
    nfft_interp), the mode kernel (nfft_modes: embed or extract, and the QU rotation) and the coarse transform with its layout step (all
    other classes); the fine-grid transform runs on a context the projector owns, so it is timed as the very same call (cmbl_rfft /
    cmbl_irfft, transform plus layout step) on a context of the fine grid's size.  Per stage: microseconds, the bytes the stage must move
    (each array it reads or writes once; for the extract, only the quarter of the fine half plane it reads), and bytes / time as a fraction
    of the streaming-copy rate.  "the rest" is the call's time less its stages: launch gaps and, towards the sphere, the clearing of the output
    (a few microseconds below zero where the fine transform, timed in calls of its own, runs slower there than inside the projection).

The two methods compute different things; these times are records and nothing is asserted on them.  Appends to profiles/nfft_times.txt:

    python tools/gpu_nfft_time.py"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
OUT = os.path.join(ROOT, "profiles", "nfft_times.txt")
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
    el = 4 if prec == "f32" else 8
    buf = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(buf)
    copy_us = timed(lambda: dst.copy_(buf), torch)[0]
    rate = 2 * buf.numel() / copy_us / 1e3                                    # GB/s, read + written
    del buf, dst
    print(f"{prec}: streaming copy {rate:.0f} GB/s (256 MiB device-to-device, bytes read + written)", flush=True)
    p = C.ProjLambert(N, N, THETA, T)
    fine = C.ProjLambert(2 * N, 2 * N, THETA / 2, T)                          # a context of the fine grid's size, for the stage times only
    hp = C.ProjHealpix(NSIDE)
    built = {}
    for method in ("bilinear", "nfft"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        built[method] = C.Projector(hp, p, method=method)
        print(f"{prec}: Projector(Nside {NSIDE} => {N}^2 at {THETA}', {method}) built in {(time.perf_counter() - t0) * 1e3:.1f} ms", flush=True)
    P, Pb = built["nfft"], built["bilinear"]
    ni = P.n_in_patch
    print(f"{prec}: {ni} pixels in the patch, {P.n_touched} touched; window width {P.window_width}, fine grid {2 * N}^2", flush=True)
    g = torch.Generator(device="cpu").manual_seed(0)
    ncart, nfine = N * N, 4 * N * N
    half_c, half_f = N * (N // 2 + 1) * 2 * el, 2 * N * (N + 1) * 2 * el           # bytes of a coarse / fine half plane
    for npol, name in ((1, "I"), (2, "QU")):
        h = C.HealpixField(hp, torch.randn((1, npol, hp.npix), generator=g, dtype=T).to(p.device), name)
        m = C.Field(p, torch.randn((1, npol, N, N), generator=g, dtype=T).to(p.device), C.MAP)
        fm = fine.tensor(torch.randn((1, npol, 2 * N, 2 * N), generator=g, dtype=T))
        fF = fine.rfft(fm)
        node_tab = ni * (16 + 4 + 2 * el)
        stages = {
            "to_cart": [("nfft_spread", npol * (ni * el + nfine * el) + node_tab),
                        ("fine rfft + layout", npol * (nfine * el + half_f)),
                        ("nfft_modes", npol * (half_c + half_c) + (npol == 2) * ncart * 6 * el),
                        ("coarse irfft + layout", npol * (half_c + ncart * el))],
            "to_healpix": [("coarse rfft + layout", npol * (ncart * el + half_c)),
                           ("nfft_modes", npol * (half_c + half_f)),
                           ("fine irfft + layout", npol * (half_f + nfine * el)),
                           ("nfft_interp", npol * (nfine * el + ni * el) + node_tab)],
        }
        for direction, fn, fnb in (("to_cart", lambda: P.to_cart(h), lambda: Pb.to_cart(h)), ("to_healpix", lambda: P.to_healpix(m), lambda: Pb.to_healpix(m))):
            med, lo, hi = timed(fn, torch)
            medb, lob, hib = timed(fnb, torch)
            print(f"  {prec} {name:2s} {direction:10s} nfft {med:9.1f} us ({lo:.1f} .. {hi:.1f})   bilinear {medb:9.1f} us ({lob:.1f} .. {hib:.1f})", flush=True)
            p.prof_enable(True)
            p.prof_reset()
            for _ in range(ITERS):
                fn()
            tab = p.prof_table()
            p.prof_enable(False)
            own = {k: v[0] * 1e3 / ITERS for k, v in tab.items()}
            coarse = sum(v for k, v in own.items() if not k.startswith("nfft_"))
            fine_us = timed((lambda: fine.rfft(fm)) if direction == "to_cart" else (lambda: fine.irfft(fF)), torch)[0]
            rest = med
            for label, nbytes in stages[direction]:
                us = own.get(label, 0.0) if label.startswith("nfft_") else fine_us if label.startswith("fine") else coarse
                rest -= us
                frac = nbytes / us / 1e3 / rate if us > 0 else float("nan")
                print(f"      {label:22s} {us:9.1f} us   {nbytes / 1e6:8.1f} MB   {100 * frac:5.1f} % of the copy rate", flush=True)
            what = f"clearing the output ({npol * hp.npix * el / 1e6:.1f} MB written) and gaps" if direction == "to_healpix" else "gaps between launches"
            print(f"      {'the rest':22s} {rest:9.1f} us   {what}", flush=True)


def main():
    if len(sys.argv) > 1:
        child(sys.argv[1])
        return
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(f"# HEALPix projection by non-uniform FFT, Nside {NSIDE} <-> {N}^2 at {THETA}', {time.strftime('%Y-%m-%d')}; us per call, median (min .. max) of {REPS} x {ITERS} calls\n")
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
