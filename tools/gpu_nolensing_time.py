"""Time per conjugate-gradient iteration of the Wiener filter of the no-lensing model d = M B f + n (argmaxf_logpdf, src/maximization.jl:17-42;
NoLensingDataSet, src/dataset.jl:37-47) at 1024^2, fp32, border mask, QU and T+QU, B = 1 and 8, from one process, in three forms:

  (i)   a BaseDataSet with a LenseFlow(7) at phi = 0: the only way to this answer before the identity existed (two identity flows per iteration)
  (ii)  a NoLensingDataSet, composed form: the identity NoLens<T> in the L slot, option fused_harm = 0
  (iii) a NoLensingDataSet, fused form (the default): CgSolver::solve_fused around Dataset::nolens_adjoint, 7 launches per iteration

A solve is fixed-length (tol = 0); the time per iteration is (T(nsteps = 60) - T(nsteps = 10)) / 50 after a warm-up of both lengths, the forms
alternated, REPS repetitions each (median; spread = max - min; [min, max]).  The condition on (iii): not slower than (ii) by more than the spread.
Form (i) needs nothing of the no-lensing feature, so the same file measures it on a commit that does not have it (there (ii) and (iii) are left out).

    python tools/gpu_nolensing_time.py        (prints its table; profiles/nolensing_cg_time.txt is a run of it)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cmblensing_jl_amd as C      # noqa: E402
from bench import synthetic_cls    # noqa: E402

REPS, N, T = 5, 1024, torch.float32
if os.environ.get("NOLENSING_SMALL"):                       # rehearsal at a toy size
    N = 128
NLONG, NSHORT = 60, 10
KW = dict(T=T, beam_fwhm=3.0, pixel_mask=dict(pad_deg=0.4, apod_deg=0.6), Nphi="flat")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def per_iteration(solve):
    return (wall(lambda: solve(NLONG)) - wall(lambda: solve(NSHORT))) / (NLONG - NSHORT)


def forms(pol, B):
    """name -> solve(nsteps) of every form this commit has"""
    cls = synthetic_cls()
    s = C.load_sim(2.0, N, pol, cls, Nbatch=B, **KW)
    ds, p = s["ds"], s["proj"]
    phi0 = C.Field(p, torch.zeros_like(s["phi"].arr[:1]), C.FOURIER)
    out = {"(i)   BaseDataSet, LenseFlow(7) at phi = 0": lambda n: ds.argmaxf_logpdf(phi0, tol=0.0, nsteps=n)}
    if hasattr(C, "load_nolensing_sim"):
        nl = C.load_nolensing_sim(2.0, N, pol, cls, Nbatch=B, **KW)
        nds, q = nl["ds"], nl["proj"]

        def composed(n):
            q.set_option("fused_harm", 0)
            try:
                return nds.argmaxf_logpdf(tol=0.0, nsteps=n)
            finally:
                q.set_option("fused_harm", 1)
        out["(ii)  NoLensingDataSet, composed"] = composed
        out["(iii) NoLensingDataSet, fused"] = lambda n: nds.argmaxf_logpdf(tol=0.0, nsteps=n)
    return out


def main():
    print(f"# Wiener-filter CG iteration without lensing; {torch.cuda.get_device_name(0)}; {N}^2 fp32, border mask; ms per iteration = (T({NLONG}) - T({NSHORT})) / "
          f"{NLONG - NSHORT}, median of {REPS} (spread = max - min)")
    for pol, B in (("P", 1), ("P", 8), ("IP", 1), ("IP", 8)):
        fs = forms(pol, B)
        for solve in fs.values():                           # warm-up: both lengths of every form
            solve(NSHORT), solve(NLONG)
        times = {k: [] for k in fs}
        for _ in range(REPS):
            for k, solve in fs.items():                     # alternated
                times[k].append(per_iteration(solve) * 1e3)
        print(f"{'QU' if pol == 'P' else 'T+QU'}, B = {B}")
        med = {}
        for k, v in times.items():
            med[k] = float(np.median(v))
            print(f"  {k:44s} {med[k]:9.4f} ms   spread {max(v) - min(v):7.4f}   [{min(v):.4f}, {max(v):.4f}]")
        ks = list(med)
        if len(ks) == 3:
            print(f"  (iii) / (ii) = {med[ks[2]] / med[ks[1]]:.3f}      (i) / (iii) = {med[ks[0]] / med[ks[2]]:.2f}")
        del fs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
