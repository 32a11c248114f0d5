"""One Gibbs θ pass of sample_joint -- gibbs_sample_theta over 20 values of Aϕ, then over 20 values of r -- at 1024^2, QU and T+QU, fp32,
LenseFlow(7), border mask, with the grid evaluated on the host path (`on="host"`: theta.set_theta per grid point, the code before the device
path existed and the yardstick here) and on the device (`on="device"`: one cmbl_logpdf_mixed_theta call per parameter), in ONE process on ONE
data set, alternated, REPS times each after one warm-up pass of each (median, spread = max - min).  A pass is timed with the host clock between
two device synchronisations; it ends with the `set_theta` at the sampled θ that sample_joint makes in either mode, which is not part of the
timed region.  Also printed: the largest difference of the two normalised log-pdf grids (the results must not change), and the part of a
device pass that is the θ-operator kernel itself (cmbl_dataset_theta_ops at 40 θ, no posterior evaluation).

    python tools/gpu_theta_time.py            (prints its table)

Has been run on MI355X: DESIGN.md §5 has the figures."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cmblensing_jl_amd as C      # noqa: E402
from bench import synthetic_cls    # noqa: E402

REPS, N, NGRID, T = 5, 1024, 20, torch.float32
if os.environ.get("THETA_SMALL"):                           # rehearsal at a toy size
    REPS, N, NGRID = 2, 64, 4


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    print(f"# Gibbs θ pass, {NGRID} values of Aphi then {NGRID} of r; {torch.cuda.get_device_name(0)}; {N}^2 fp32, LenseFlow(7), border mask; "
          f"ms per pass, median of {REPS} (spread = max - min)")
    grids = dict(Aphi=np.linspace(0.6, 1.6, NGRID), r=np.linspace(0.05, 0.5, NGRID))
    for pol, name in (("P", "QU"), ("IP", "T+QU")):
        s = C.load_sim(2.0, N, pol, synthetic_cls(), T=T, beam_fwhm=3.0, pixel_mask=dict(pad_deg=0.4, apod_deg=0.6), Nbatch=1, Nphi="flat")
        ds = s["ds"]
        fo, po = ds.mix(s["f"], s["phi"])

        def one_pass(on):
            theta, lps = dict(r=None, Aphi=None), []
            for key, xs in grids.items():
                val, lp = C.gibbs_sample_theta(ds, fo, po, theta, key, xs, [0.37], on=on)
                theta[key] = float(val[0])
                lps.append(lp[0])
            return theta, np.concatenate(lps)

        def fixed(on):
            """the two grids at the SAME θ of the other parameter (in a pass the second grid sits at the first one's draw, whose last bits differ
            between the modes -- and d logpdf / d Aphi is 1e5..1e6 here)"""
            return np.concatenate([C.gibbs_sample_theta(ds, fo, po, dict(r=None, Aphi=None), key, xs, [0.37], on=on)[1][0] for key, xs in grids.items()])

        times, res = {"host": [], "device": []}, {}
        try:
            for on in times:                                  # warm-up: code objects, scratch, the installed model
                one_pass(on)
                res[on] = fixed(on)
                C.set_theta(ds)
            for _ in range(REPS):
                for on in times:                              # alternated
                    t, _ = wall(lambda: one_pass(on))
                    times[on].append(t * 1e3)
                    C.set_theta(ds)
            tk, _ = wall(lambda: [C.theta_ops_device(ds, "Cphi_inv", r=float(x), Aphi=1.0) for x in np.linspace(0.05, 0.5, 2 * NGRID)])
        finally:
            C.set_theta(ds)
        med = {on: float(np.median(v)) for on, v in times.items()}
        print(f"{name}")
        for on, v in times.items():
            print(f"  on={on:7s} {med[on]:10.2f} ms   spread {max(v) - min(v):8.2f}")
        print(f"  host / device = {med['host'] / med['device']:.1f}      θ-operator kernel + sums + one plane read-back, {2 * NGRID} θ: {tk * 1e3:.2f} ms")
        print(f"  normalised log-pdf grids, device against host: max absolute difference {np.max(np.abs(res['device'] - res['host'])):.2e}")
        del s, ds, fo, po
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
