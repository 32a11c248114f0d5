#!/usr/bin/env python
"""Writes tests/golden/lensop_dataset_budget.json: the float32 error budget of the data-set tests with BilinearLens / PowerLens in the L slot
(tests/test_gpu_lensop_dataset.py).  Per case and quantity: the distance of the CPU restatement (tests/_lensop_ds_ref.py: the oracle's data set
over tests/_bilinear_ref.py / tests/_powerlens_ref.py) run in float32 from the same restatement run in float64 on identical inputs (the float64
run's fields, rounded) -- relative L2 for fields, the largest relative error for per-slot scalars (residual histories, logpdf, gradient norms).
The figure never comes from the device: the GPU tests allow the device 3 x it in single precision (the rule of tests/golden/bilinear_budget.json).

    python tools/make_lensop_dataset_budget.py            (CPU, under a minute)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _lensop_ds_ref as R  # noqa: E402


def main():
    r64, r32 = R.reference(np.float64), R.reference(np.float32)
    out = {"what": "distance of tests/_lensop_ds_ref.py in float32 from the same in float64, inputs rounded to float32: relative L2 (fields), "
                   "largest relative error (hist, hist2, logpdf, logpdf_mixed, g_norm)",
           "theta_pix": 3.0, "beam_fwhm": 3.0, "rms_px": R.RMS_PX, "cases": {}}
    for name in r64:
        out["cases"][name] = {q: R.distance(q, r32[name][q], r64[name][q]) for q in r64[name] if q not in R.NOT_COMPARED}
        out["cases"][name]["n_conv"] = {"f32": r32[name]["n_conv"], "f64": r64[name]["n_conv"]} if "n_conv" in r64[name] else None
        if out["cases"][name]["n_conv"] is None:
            del out["cases"][name]["n_conv"]
    path = os.path.join(ROOT, "tests", "golden", "lensop_dataset_budget.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["cases"], indent=1))


if __name__ == "__main__":
    main()
