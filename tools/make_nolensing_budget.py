#!/usr/bin/env python
"""Writes tests/golden/nolensing_budget.json: the float32 error budget of tests/test_gpu_nolensing.py.  Per case of tests/_nolensing_ref.py (pol,
shape, batch size, with or without the pixel mask) and per quantity the GPU tests compare: the distance of the oracle's no-lensing data set run in
float32 from the same run in float64 on identical inputs (the float64 run's d, rounded) -- the largest relative error of scalars (a residual history,
logpdf: "hist"), the largest per-slot relative L2 of fields (an iterate, a gradient, a mean: "x").  The figure never comes from the device: the GPU
tests allow the device max(class bound, 3 x it) in single precision (tests/_cg_rules_ref.bound, the rule of tests/golden/cg_rules_budget.json).

    python tools/make_nolensing_budget.py            (CPU, under a minute)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _nolensing_ref as N  # noqa: E402


def cases():
    """(pol, shape, B, mask) of every data set the GPU tests make"""
    out = [(pol, shape, 2, True) for pol in N.POLS for shape in N.POW2 + [N.ANYSIZE]]
    out += [("P", (32, 32), 17, True)]
    out += [(pol, (32, 32), 2, False) for pol in N.POLS]
    return out


def runs(pol, shape, B, mask):
    """run name -> {"hist": ..., "x": ...} of one case"""
    s32, s64 = N.sim(pol, shape, np.float32, B, mask), N.sim(pol, shape, np.float64, B, mask)
    r = {}
    f32 = s64["f"].astype(np.complex64)
    model = lambda s, f: (s["ds"].gradientf_logpdf(f, N.IDENTITY, s["d"]), s["ds"].mean(N.IDENTITY, f), s["ds"].logpdf(f))
    (g32, m32, l32), (g64, m64, l64) = model(s32, f32), model(s64, s64["f"])
    r["model"] = {"grad": N.distance("x", g32, g64), "mean": N.distance("x", m32, m64), "logpdf": N.distance("hist", l32, l64)}
    if not mask:
        (x32, h32), (x64, h64) = (N.solve(pol, shape, T, B, mask, 500, N.TOL) for T in (np.float32, np.float64))
        assert len(h32) == len(h64) == 2
        r["tol"] = {"hist": N.distance("hist", h32[:1], h64[:1]), "x": N.distance("x", x32, x64)}          # (the second residual is rounding noise)
        return r
    (x32, h32), (x64, h64) = (N.solve(pol, shape, T, B, mask, N.NSHORT, 0.0) for T in (np.float32, np.float64))
    r[f"n{N.NSHORT}"] = {"hist": N.distance("hist", h32, h64), "x": N.distance("x", x32, x64)}
    if pol == "P":
        (x32, h32), (x64, h64) = (N.solve(pol, shape, T, B, mask, 500, N.TOL) for T in (np.float32, np.float64))
        assert len(h32) == len(h64) == N.STOPS[(tuple(shape), B)][0]
        r["tol"] = {"hist": N.distance("hist", h32, h64), "x": N.distance("x", x32, x64)}
    if tuple(shape) == (32, 32) and B == 2:
        wf, wn = N.whites(pol, shape, B)
        a, _ = s32["ds"].sample_f(wf.astype(np.float32), wn.astype(np.float32), tol=0.0, nsteps=N.NSHORT)
        b, _ = s64["ds"].sample_f(wf, wn, tol=0.0, nsteps=N.NSHORT)
        r["sample_f"] = {"x": N.distance("x", a, b)}
    return r


def main():
    out = {"what": "distance of the oracle's no-lensing data set (tests/_nolensing_ref.py) in float32 from the same in float64, d rounded to float32: "
                   "largest relative error of scalars (hist, logpdf), largest per-slot relative L2 of fields (x, grad, mean); run n<k>: tol = 0, nsteps = k; "
                   "run tol: tol = 0.1, nsteps = 500; run sample_f: tol = 0, nsteps = 8 from injected white draws",
           "theta_pix": N.THETA, "beam_fwhm": N.BEAM, "pixel_mask": N.PM, "cases": {}}
    for pol, shape, B, mask in cases():
        out["cases"][N.case_key(pol, shape, B, mask)] = runs(pol, shape, B, mask)
    path = os.path.join(ROOT, "tests", "golden", "nolensing_budget.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["cases"], indent=1))


if __name__ == "__main__":
    main()
