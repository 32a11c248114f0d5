"""get_Cl on the device against what a caller had to do without it, at 1024^2 QU fp32 (B = 1 and 8) and 2048^2 QU fp64 (B = 1); MAP fields, the
default which = (EE, BB), the default edges 0:50:16000:
  device     C.get_Cl(f): MAP -> EB half planes (the context's transform and rotation), cmbl_get_cl, the copy of the binned sums to the host
  copy       the copy of the field to the host alone -- pageable (`f.arr.cpu()`) and into a pinned buffer -- which is what had to happen before ANY binning
  copy+host  the pageable copy plus tests/_cl_ref.py on the host (NumPy rfft2 and the QQ, UU spectra of every slot; the QU -> EB rotation is left out,
             in the host's favour)
One process; every GPU step runs under its own time limit (SIGALRM: the process ends there and nothing more is started).  Blocks of about 50 ms,
warm-up until two successive blocks agree to 1 %, the figure is the median block.  Also: the time of the kernel class `get_cl` per call (HIP events,
cmbl_prof_*) beside the bytes its launches must move -- the field planes once, 4 + 8 bytes of index and coefficient per listed mode, the chunk
partials -- over the 8 TB/s peak of the memory (the transform and rotation before them are of other classes).
   python tools/gpu_get_cl_ab.py [output file]"""
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import cmblensing_jl_amd as C
import _cl_ref as R

PEAK = 8e12
BLOCK_MS, BLOCKS, MAX_WARM, STEP_LIMIT = 50.0, 7, 30, 120
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timeout(sig, frm):
    say("a GPU step exceeded its time limit: stopping here")
    os._exit(124)


signal.signal(signal.SIGALRM, timeout)


def block(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def measure(fn):
    """median ms per call of `fn` (which leaves its result on the host), one step under the time limit"""
    signal.alarm(STEP_LIMIT)
    fn()
    n = max(3, int(BLOCK_MS / block(fn, 3)))
    last, warm = None, 0
    while warm < MAX_WARM:
        now = block(fn, n)
        warm += 1
        if last and abs(now - last) <= 0.01 * last:
            break
        last = now
    t = float(np.median([block(fn, n) for _ in range(BLOCKS)]))
    signal.alarm(0)
    return t, warm, n


say("get_Cl of a QU MAP field, which = (EE, BB), edges 0:50:16000: ms per call, result on the host")
say(f"{'shape':>8} {'prec':>4} {'B':>2} {'device':>8} {'copy':>8} {'pinned':>8} {'copy+host':>10} {'copy/device':>11} {'pinned/device':>13} | {'kernels':>8} {'floor':>7} {'MB moved':>9}")
lost = []
for N, T, Bs in ((1024, torch.float32, (1, 8)), (2048, torch.float64, (1,))):
    p = C.ProjLambert(N, N, 2.0, T)
    el = 4 if T == torch.float32 else 8
    for B in Bs:
        f = C.Field(p, p.randn(list(range(1, B + 1)), 0, 2), C.MAP)
        pin = torch.empty(f.arr.shape, dtype=f.arr.dtype, pin_memory=True)
        device = lambda: C.get_Cl(f)
        copy = lambda: f.arr.cpu()
        pinned = lambda: (pin.copy_(f.arr, non_blocking=True), torch.cuda.synchronize())

        def host():
            m = f.arr.cpu().numpy().astype(np.float64)
            F = np.fft.rfft2(m, axes=(-2, -1))
            return [R.get_cl(F[b, k], None, p.lmag, N, 2.0) for b in range(B) for k in range(2)]

        td, wd, nd = measure(device)
        tc, _, _ = measure(copy)
        tp, _, _ = measure(pinned)
        signal.alarm(STEP_LIMIT)
        t0 = time.perf_counter()
        host()
        th = (time.perf_counter() - t0) * 1e3
        signal.alarm(0)
        # the kernel class alone
        signal.alarm(STEP_LIMIT)
        p.prof_reset()
        p.prof_enable(True)
        for _ in range(20):
            device()
        p.prof_enable(False)
        ms, launches = p.prof_table().get("get_cl", (0.0, 0))
        signal.alarm(0)
        L = p.lmag
        listed = int(np.sum((L > 0) & (L < 16000)))                             # half-plane modes inside the edges
        moved = B * listed * (2 * 2 * el + 12)                                  # two complex planes + index and coefficient, per slot
        tk = ms / 20
        say(f"{N:>6}^2 {'f32' if el == 4 else 'f64':>4} {B:>2} {td:8.4f} {tc:8.4f} {tp:8.4f} {th:10.1f} {tc / td:11.2f} {tp / td:13.2f} | {tk:8.4f} {1e3 * moved / PEAK:7.4f} {moved / 1e6:9.2f}"
            f"   (warm-up blocks: {wd}; calls per block: {nd}; {launches // 20} launches of the class per call)")
        if min(tc, tp) < td:
            lost.append((N, B))
say("the device call is slower than the bare copy of the field at: " + (", ".join(f"{n}^2 B={b}" for n, b in lost) if lost else "no shape"))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
