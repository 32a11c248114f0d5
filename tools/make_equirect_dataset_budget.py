#!/usr/bin/env python
"""Writes tests/golden/equirect_dataset_budget.json: the float32 error budget of tests/test_gpu_equirect_ds.py.  Per case and quantity: the distance
of the NumPy oracle of the ProjEquiRect data set (tests/_equirect_ds_ref.py) run in float32 from the same oracle run in float64 on identical,
float32-representable inputs -- relative L2 for fields, the largest relative error for per-slot scalars (logpdf, residual histories).  The figure
never comes from the device.  The GPU tests allow the device 3 x it in a float32 context and 3 x it x 2^-29 (the ratio of the unit roundoffs), floor
1e-12, in a float64 context.

    python tools/make_equirect_dataset_budget.py            (CPU, seconds)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _equirect_ds_ref as D  # noqa: E402


def main():
    out = {"what": "distance of tests/_equirect_ds_ref.py in float32 from the same in float64, inputs float32-representable: relative L2 (fields), "
                   "largest relative error (logpdf, hist, hist_fs)", "nsteps": D.NSTEPS, "cases": {}}
    for c in D.CASES:
        r64, r32 = D.reference(c, np.float64), D.reference(c, np.float32)
        assert r32["n_stop"] == r64["n_stop"] < 50, (c, r32["n_stop"], r64["n_stop"])
        out["cases"][D.case_id(c)] = {q: D.distance(q, r32[q], r64[q]) for q in r64 if q not in ("tol_stop", "n_stop")}
        out["cases"][D.case_id(c)]["n_stop"] = r64["n_stop"]
    for spin in (0, 2):                                                      # Cf = Cℓ_to_Cov at the reference's test size, from its NumPy restatement
        o = D.cl_case(spin, D.cl_blocks_numpy(spin))
        r64, r32 = D.cl_reference(o, np.float64), D.cl_reference(o, np.float32)
        assert np.all(r64["hist"][-1] >= 1e-6 * r64["hist"][0])
        out["cases"][f"cl_{D.CL_NY}x{D.CL_NX}_s{spin}"] = {q: D.distance(q, r32[q], r64[q]) for q in r64}
    path = os.path.join(ROOT, "tests", "golden", "equirect_dataset_budget.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["cases"], indent=1))


if __name__ == "__main__":
    main()
