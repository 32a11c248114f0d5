"""make_mask on the device next to its SciPy restatement on the host: the reference's default arguments at 1024^2 (2' pixels) and 4096^2 (1'),
fp32 context, sources from `draw_ptsrcs(seed = 0)`.

Device: a call is warmed up first (WARM calls); a sample is the host clock around ONE call, which ends in a synchronise of its own (the entry point
frees its scratch), REPS samples, median and spread (min .. max) in ms.  The three phases -- distance transforms (`edt`, three per mask: border,
sources, bled sources), the two passes of the Gaussian filter (`mask_gauss`) and the pointwise kernels (`make_mask`: feature planes and the
profile) -- and the tiled transposes between passes (`layout`) are the per-kernel-class event timings of ONE further call (cmbl_prof_*).
Host: tests/_mask_ref.py on the same inputs, one run (HOST_REPS at 1024^2), and the largest difference between the two masks.

These times are records; nothing is asserted on them.

    python tools/gpu_make_mask_time.py > profiles/make_mask_times.txt"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cmblensing_jl_amd as C      # noqa: E402
import _mask_ref as R              # noqa: E402

CASES = ((1024, 2.0), (4096, 1.0))
WARM, REPS = 2, 7
PHASES = ("edt", "mask_gauss", "make_mask", "layout")


def main():
    print(f"# make_mask, reference defaults (edge_padding_deg = 2, edge_rounding_deg = 1, apodization_deg = 1, ptsrc_radius_arcmin = 7), fp32 context, {torch.cuda.get_device_name(0)}")
    print(f"# device: ms per call, median (min .. max) of {REPS} calls, each ending in its own synchronise; phases: kernel time of one further call, by kernel class")
    print("# the distance transform's second pass is the outward scan over the row of g^2 in LDS; the lower-envelope form was not built, so there is no A/B")
    for N, theta in CASES:
        p = C.ProjLambert(N, N, theta, torch.float32)
        n = R.default_num_ptsrcs(N, N, theta)
        yx = C.engine.draw_ptsrcs(N, N, n, seed=0)
        pad, apod_w, round_w, src_w = C.engine.mask_npix(theta)
        call = lambda: C.make_mask(p, ptsrcs=yx)
        for _ in range(WARM):
            m = call()
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = call()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        p.prof_reset()
        p.prof_enable(True)
        call()
        p.prof_enable(False)
        prof = p.prof_table()
        print(f"{N}^2 at {theta}': pad {pad}, apod_w {apod_w}, round_w {round_w} ({4 * round_w + 1} taps), src_w {src_w}, {n} sources")
        print(f"  device make_mask      {np.median(ts):9.3f}  ({min(ts):.3f} .. {max(ts):.3f})")
        for k in PHASES:
            ms, cnt = prof.get(k, (0.0, 0))
            print(f"    {k:12s} {ms:9.3f}  in {cnt} launches")
        reps = 3 if N <= 1024 else 1
        th = []
        for _ in range(reps):
            t0 = time.perf_counter()
            want = R.make_mask(N, N, yx, pad, apod_w, round_w, src_w)
            th.append((time.perf_counter() - t0) * 1e3)
        got = m.arr[0, 0].cpu().numpy()
        print(f"  host tests/_mask_ref  {np.median(th):9.1f}  ({reps} run(s))   host / device = {np.median(th) / np.median(ts):.0f}")
        print(f"  max |device - host| = {float(np.abs(got.astype(np.float64) - want).max()):.3e}, {int((got != want).sum())} of {got.size} pixels differ")
        del p


if __name__ == "__main__":
    main()
