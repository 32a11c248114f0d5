#!/usr/bin/env python
"""Writes tests/golden/project_adjoint_budget.json: what the window algorithm loses on the two TRANSPOSES of the non-uniform-FFT projection
(tests/_project_adjoint_ref.py `window_to_healpix_T` / `window_to_cart_T`, the scheme the device runs) against the exact sums through K
(`nfft_to_healpix_T` / `nfft_to_cart_T`), per case and precision, at the width of that precision.  The convention of
tools/make_nfft_budget.py: a margin over the restatement, never over the code under test.

Per entry: the LARGEST relative L2 error of a plane over NDRAW random IQU cotangents with nbatch 3, the window restatement in that dtype
against the float64 sums.  "identity_to_cart" / "identity_to_healpix": the largest |<A x, y> - <x, Aᵀ y>| / (|A x| |y|) the window restatement
shows in that dtype with A the forward of that name and Aᵀ its transpose, IQU, dots in float64 -- the base of the bound of the same identity
on the device.  tests/test_gpu_project_adjoint.py allows the device 3 x these figures (floor 1e-12).

    python tools/make_project_adjoint_budget.py            (CPU, a few seconds)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _nfft_ref as N  # noqa: E402
import _project_adjoint_ref as A  # noqa: E402

NDRAW = 16


def main():
    out = {"_comment": "tools/make_project_adjoint_budget.py: relative L2 error of the window restatement of the transposes "
                       "(tests/_project_adjoint_ref.py) against the sums through K; identity_*: its own adjoint mismatch",
           "ndraw": NDRAW, "cases": {}}
    for case in N.CASES:
        P = N.projector(case)
        Ny, Nx = P.cart.Ny, P.cart.Nx
        g = np.random.default_rng(31000 + len(case))
        fields = [(g.standard_normal((3, 3, Nx, Ny)), g.standard_normal((3, 3, P.npix))) for _ in range(NDRAW)]
        entry = {"npatch": P.npatch, "Ny": Ny, "Nx": Nx}
        for prec in ("f32", "f64"):
            T, w = N.DTYPE[prec], N.WIDTH[prec]
            eh = ec = ih = ic = 0.0
            for m, h in fields:
                m, h = m.astype(T), h.astype(T)                                # the exact sums see the rounded inputs too
                wh, wc = A.window_to_healpix_T(P, h, T), A.window_to_cart_T(P, m, T)
                eh = max(eh, float(N.rel_planes(wh, A.nfft_to_healpix_T(P, h)).max()))
                ec = max(ec, float(N.rel_planes(wc, A.nfft_to_cart_T(P, m)).max()))
                # x = h, y = m for A = to_cart; x = m, y = h for A = to_healpix
                ic = max(ic, A.identity_mismatch(P.window_to_cart(h, T), m, h, wc))
                ih = max(ih, A.identity_mismatch(P.window_to_healpix(m, T), h, m, wh))
            entry[prec] = {"width": w, "to_healpix_adjoint": eh, "to_cart_adjoint": ec, "identity_to_healpix": ih, "identity_to_cart": ic}
            print(f"{case:14s} {prec} w {w:2d}  to_healpix^T {eh:.3e}  to_cart^T {ec:.3e}  identity to_healpix {ih:.3e}  to_cart {ic:.3e}")
        out["cases"][case] = entry
    path = os.path.join(ROOT, "tests", "golden", "project_adjoint_budget.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
