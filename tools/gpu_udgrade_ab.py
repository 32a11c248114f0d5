"""A/B of the default ud_grade downgrade (map mode, anti-aliasing and pixel-window deconvolution on, map in, Fourier out):
  fused    one cmbl_ud_grade call: rfft at the source size, the gather kernel with the block mean as a Fourier-space weight
  literal  the reference's sequence assembled from the same library: the anti-aliasing mask as a Fourier-diagonal operator on the map
           (cmbl_diag_apply MAP -> MAP: rfft + irfft at the source size), then cmbl_ud_grade without anti-aliasing (block mean, rfft at
           the new size, 1 / PWF)
at 1024^2 -> 512^2 and 2048^2 -> 512^2, QU, single precision, B = 1 and 8.  Blocks of the two alternate; warm-up runs until two successive
blocks of each agree to 1 %; the figure is the median block.  Beside each time: the compulsory bytes of that path (what its calls must read
and write once: fused = source map + new half plane; literal = source map + filtered map, written and read again, + new half plane) over
the 8 TB/s peak of the memory.  The two results are compared as well.
   python tools/gpu_udgrade_ab.py [output file]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import cmblensing_jl_amd as C
import _udgrade_ref as R

PEAK = 8e12
BLOCK_MS, BLOCKS, MAX_WARM = 50.0, 7, 30                 # a block lasts about 50 ms: its calls are counted from a first short block
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def block(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


say("ud_grade default downgrade, QU fp32: fused (one transform at the source size) vs literal (the reference's three-transform sequence), ms per call")
say(f"{'shape':>16} {'B':>2} {'fused':>8} {'floor':>7} {'literal':>8} {'floor':>7} {'literal/fused':>13} {'rel. diff':>10}")
slower = []
for N, fac in ((1024, 2), (2048, 4)):
    Nn = N // fac
    ps, pd = C.ProjLambert(N, N, 2.0, torch.float32), C.ProjLambert(Nn, Nn, 2.0 * fac, torch.float32)
    mask = ps.tensor(np.broadcast_to(R.antialias_mask(N, N, Nn, Nn).astype(np.float32), (2, N, N // 2 + 1)).copy())
    for B in (1, 8):
        f = C.Field(ps, ps.randn(list(range(1, B + 1)), 0, 2), C.MAP)
        fused = lambda: C.ud_grade(f, 2.0 * fac, proj_new=pd)
        literal = lambda: C.ud_grade(C.Field(ps, ps.diag_apply(mask, f.arr, C.FOURIER, C.MAP, C.MAP), C.MAP), 2.0 * fac, anti_aliasing=False, proj_new=pd)
        a, b = fused().arr, literal().arr
        diff = float(torch.linalg.norm(a - b) / torch.linalg.norm(b))
        nf, nl = (max(10, int(BLOCK_MS / block(fn, 10))) for fn in (fused, literal))
        last, warm = None, 0
        while warm < MAX_WARM:
            now = (block(fused, nf), block(literal, nl))
            warm += 1
            if last and all(abs(x - y) <= 0.01 * y for x, y in zip(now, last)):
                break
            last = now
        tf, tl = [], []
        for _ in range(BLOCKS):
            tf.append(block(fused, nf))
            tl.append(block(literal, nl))
        tf, tl = float(np.median(tf)), float(np.median(tl))
        src, out = 2 * B * N * N * 4, 2 * B * Nn * (Nn // 2 + 1) * 8
        say(f"{N:>6}^2->{Nn:>4}^2 {B:>2} {tf:8.4f} {1e3 * (src + out) / PEAK:7.4f} {tl:8.4f} {1e3 * (3 * src + out) / PEAK:7.4f} {tl / tf:13.2f} {diff:10.2e}"
            f"   (warm-up blocks: {warm}; calls per block: {nf} / {nl})")
        if tf > tl:
            slower.append((N, B))
say("fused is slower at: " + (", ".join(f"{n}^2 B={b}" for n, b in slower) if slower else "no shape"))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
