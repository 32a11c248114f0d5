#!/usr/bin/env python
"""Writes tests/golden/nfft_budget.json: what the window algorithm of the non-uniform-FFT projection (tests/_nfft_ref.py `Plan`, the scheme
the device runs) loses against the exact sums it approximates, per case, direction and precision, at the width of that precision.

Per entry: the LARGEST relative L2 error of a plane over NDRAW random IQU fields with nbatch 3 (QU rotated, as `project` returns them), the
window restatement in that dtype against the float64 direct sums.  tests/test_gpu_nfft.py allows the device 3 x that figure (floor 1e-12),
tests/test_nfft_ref.py holds the restatement itself to it.  "transpose": the relative mismatch of
Ny Nx dot(to_healpix(m), h) = Npatch dot(m, to_cart(h)) the restatement shows in that dtype for I fields, as a fraction of
Ny Nx |to_healpix(m)| |h on the patch| (dots in float64): the bound's base for the same identity on the device.  "widths" is the scan that justifies the widths (float64 arithmetic, case n16_base): truncation error against w.

    python tools/make_nfft_budget.py            (CPU, a few seconds)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _nfft_ref as N  # noqa: E402

NDRAW = 16


def main():
    out = {"_comment": "tools/make_nfft_budget.py: relative L2 error of the window restatement (tests/_nfft_ref.py) against the direct sums",
           "sigma": N.SIGMA, "beta_per_w": N.BETA_PER_W, "ndraw": NDRAW, "cases": {}, "widths": {}}
    for case in N.CASES:
        P = N.projector(case)
        Ny, Nx = P.cart.Ny, P.cart.Nx
        g = np.random.default_rng(20240 + len(case))
        fields = [(g.standard_normal((3, 3, Nx, Ny)), g.standard_normal((3, 3, P.npix))) for _ in range(NDRAW)]
        entry = {"npatch": P.npatch, "Ny": Ny, "Nx": Nx}
        for prec in ("f32", "f64"):
            T, w = N.DTYPE[prec], N.WIDTH[prec]
            eh = ec = et = 0.0
            for m, h in fields:
                m, h = m.astype(T), h.astype(T)                                # the exact sums see the rounded inputs too
                wh, wc = P.window_to_healpix(m, T), P.window_to_cart(h, T)
                eh = max(eh, float(N.rel_planes(wh, P.direct_to_healpix(m)).max()))
                ec = max(ec, float(N.rel_planes(wc, P.direct_to_cart(h)).max()))
                hI = h[:, :1].astype(np.float64)
                lhs = Ny * Nx * np.sum(wh[:, 0] * hI[:, 0], axis=-1)
                rhs = P.npatch * np.sum(m[:, 0].astype(np.float64) * wc[:, 0], axis=(-2, -1))
                scale = Ny * Nx * np.linalg.norm(wh[:, 0], axis=-1) * np.linalg.norm(hI[:, 0][:, P.hpx_idxs_in_patch], axis=-1)
                et = max(et, float(np.max(np.abs(lhs - rhs) / scale)))
            entry[prec] = {"width": w, "to_healpix": eh, "to_cart": ec, "transpose": et}
            print(f"{case:14s} {prec} w {w:2d}  to_healpix {eh:.3e}  to_cart {ec:.3e}  transpose {et:.3e}")
        out["cases"][case] = entry
    P = N.projector("n16_base")
    g = np.random.default_rng(7)
    m, h = g.standard_normal((1, 1, P.cart.Nx, P.cart.Ny)), g.standard_normal((1, 1, P.npix))
    dh, dc = P.direct_to_healpix(m), P.direct_to_cart(h)
    for w in (6, 8, 10, 12, 14, 16):
        out["widths"][str(w)] = {"to_healpix": float(N.rel_planes(P.window_to_healpix(m, np.float64, w), dh)[0]),
                                 "to_cart": float(N.rel_planes(P.window_to_cart(h, np.float64, w), dc)[0])}
        print(f"width {w:2d}: {out['widths'][str(w)]}")
    path = os.path.join(ROOT, "tests", "golden", "nfft_budget.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
