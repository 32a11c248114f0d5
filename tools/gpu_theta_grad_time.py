"""The θ-gradient of logpdf(Mixed(ds); f°, ϕ°, θ) on the device (`grad_theta_logpdf_mixed`, one cmbl_grad_theta_logpdf_mixed call) at 1024^2
fp32, LenseFlow(7), border mask -- QU with θ = (r, Aϕ), and T+QU with three bands of 10 bins (θ = r, Aϕ and 30 amplitudes) -- next to

  * one `gradient_logpdf_mixed` call (cmbl_grad_logpdf_mixed): what the θ-gradient runs inside, and
  * the cheapest existing alternative: central differences through ONE `logpdf_mixed_theta_grid` call with 2 (2 + namps) points,

in ONE process on ONE data set, alternated, REPS times each after one warm-up of each (median, spread = max - min).  A call is timed with the
host clock between two device synchronisations.  Also printed: the largest difference of the two gradients relative to the larger of the two
in that parameter group (the central differences carry their truncation and, in fp32, their rounding error: a figure, not a check).

    python tools/gpu_theta_grad_time.py            (prints its table)

Has been run on MI355X: DESIGN.md §5 has the figures."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cmblensing_jl_amd as C      # noqa: E402
from bench import synthetic_cls    # noqa: E402

REPS, N, NBINS, T = 5, 1024, 10, torch.float32
if os.environ.get("THETA_SMALL"):                           # rehearsal at a toy size
    REPS, N, NBINS = 2, 64, 3
FD_STEP = 1e-2


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fd_points(theta):
    """the 2 (2 + namps) points of the central differences, and per parameter its step"""
    pts, steps = [], []
    for k, v in theta.items():
        v = np.asarray(v, float)
        for idx in (np.ndindex(*v.shape) if v.ndim else [()]):
            h = FD_STEP * abs(float(v[idx]))
            for sgn in (1, -1):
                w = v.copy()
                w[idx] += sgn * h
                pts.append({**theta, k: (float(w) if v.ndim == 0 else w)})
            steps.append((k, idx, h))
    return pts, steps


def main():
    print(f"# θ-gradient of logpdf(Mixed); {torch.cuda.get_device_name(0)}; {N}^2 fp32, LenseFlow(7), border mask; ms per call, median of {REPS} "
          f"(spread = max - min)")
    ledges = list(np.linspace(100, 3000, NBINS + 1))
    for pol, name, bands in (("P", "QU", None), ("IP", "T+QU", {"TT": (ledges, "ATT"), "TE": (ledges, "ATE"), "EE": (ledges, "AEE")})):
        cls = synthetic_cls()
        s = C.load_sim(2.0, N, pol, cls, T=T, beam_fwhm=3.0, pixel_mask=dict(pad_deg=0.4, apod_deg=0.6), Nbatch=1, Nphi="flat")
        ds = s["ds"]
        fo, po = ds.mix(s["f"], s["phi"])
        theta = dict(r=0.25, Aphi=1.1)
        if bands:
            C.use_bandpowers(ds, bands, cls["unlensed_scalar"])
            theta.update({n: np.linspace(0.9, 1.1, NBINS) for _, n in bands.values()})
        pts, steps = fd_points(theta)

        def fd():
            lp = C.logpdf_mixed_theta_grid(ds, fo, po, pts)[:, 0]
            return np.array([(lp[2 * i] - lp[2 * i + 1]) / (2 * h) for i, (_, _, h) in enumerate(steps)])

        runs = {"grad_theta_logpdf_mixed": lambda: C.grad_theta_logpdf_mixed(ds, fo, po, theta),
                "gradient_logpdf_mixed": lambda: ds.gradient_logpdf_mixed(fo, po),
                f"central differences, grid of {len(pts)}": fd}
        times, res = {k: [] for k in runs}, {}
        for k, fn in runs.items():                            # warm-up: code objects, scratch, the installed model
            res[k] = fn()
        for _ in range(REPS):
            for k, fn in runs.items():                        # alternated
                times[k].append(wall(fn)[0] * 1e3)
        med = {k: float(np.median(v)) for k, v in times.items()}
        print(f"{name}, {len(steps)} parameters")
        for k, v in times.items():
            print(f"  {k:40s} {med[k]:10.2f} ms   spread {max(v) - min(v):8.2f}")
        g = res["grad_theta_logpdf_mixed"][1]
        dev = np.concatenate([np.ravel(g[k][0]) for k in theta])
        fdv = res[f"central differences, grid of {len(pts)}"]
        print(f"  θ-gradient / gradient_logpdf_mixed = {med['grad_theta_logpdf_mixed'] / med['gradient_logpdf_mixed']:.2f}")
        print(f"  device against central differences (step {FD_STEP:g} relative), max |difference| / max |gradient|: "
              f"{np.max(np.abs(dev - fdv)) / np.max(np.abs(dev)):.2e}")
        del s, ds, fo, po
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
