#!/usr/bin/env python
"""Writes tests/golden/cg_rules_budget.json: the float32 error budget of tests/test_gpu_cg_rules.py.  Per case (I, P, IP of tests/_cg_rules_ref.py)
and per solve the GPU tests compare (tol = 0 at every `nsteps` of the case; the solve stopped by its tolerance equals the one of that length): the
distance of the oracle's Wiener filter run in float32 from the same run in float64 on identical inputs (the float64 run's d and ϕ, rounded) -- the
largest relative error of the residual history, the largest per-slot relative L2 of the returned iterate.  The figure never comes from the device:
the GPU tests allow the device max(class bound, 3 x it) in single precision (the rule of tests/golden/bilinear_budget.json).

    python tools/make_cg_rules_budget.py            (CPU, a few seconds)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _cg_rules_ref as R  # noqa: E402


def main():
    out = {"what": "distance of oracle.DataSet.argmaxf_logpdf in float32 from the same in float64, d and phi rounded to float32: largest relative "
                   "error (hist), largest per-slot relative L2 (x); run n<k>: tol = 0, nsteps = k",
           "shape": list(R.SHAPE), "theta_pix": R.THETA, "beam_fwhm": R.BEAM, "pixel_mask": R.PM, "nbatch": R.NB, "cases": {}}
    for case in sorted(R.CASES):
        out["cases"][case] = {}
        for n in R.nsteps_of(case):
            (x32, h32), (x64, h64) = R.solve(case, np.float32, n), R.solve(case, np.float64, n)
            out["cases"][case][f"n{n}"] = {"hist": R.distance("hist", h32, h64), "x": R.distance("x", x32, x64)}
    path = os.path.join(ROOT, "tests", "golden", "cg_rules_budget.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["cases"], indent=1))


if __name__ == "__main__":
    main()
