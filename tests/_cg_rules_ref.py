"""The reference side of the tests of the conjugate gradient's data-dependent rules (src/numerical_algorithms.jl:106-125): `all(res < bestres)`
keeps the best iterate of ALL batch slots together, `all(res < tol)` stops the solve, and nothing changes after the stop.  Three two-slot data
sets at 32 x 32 whose slots disagree in the steps 10 ... 14 (found with the float64 oracle on the CPU), the oracle's solves of them in float64 and
float32 on identical inputs, and a replay of a residual history under the reference's rules and under the wrong ones a port could have.
Nothing is restated: the solves are `oracle.DataSet.argmaxf_logpdf` over `oracle.cg.conjugate_gradient`.  tests/test_cg_rules_ref.py pins the
fixtures, tests/test_gpu_cg_rules.py runs the device against them, tools/make_cg_rules_budget.py records the float32 budget."""
import copy

import numpy as np

import oracle as O

SHAPE, THETA, BEAM, PM, NB = (32, 32), 3.0, 0.0, dict(pad_deg=0.4, apod_deg=0.4), 2      # = test_gpu_parity._dataset_pair(prec, pol, SHAPE, theta=3.0, mask=True, beam=0.0, B=2)

# per case: the oracle's residuals res = r'z (float64, 5 digits) by 0-based history index (index i is CG step i + 1), slot 0 and slot 1;
# held (a, b): nsteps = b returns the iterate of nsteps = a, bit for bit;  moved (a, b, rel): nsteps = b is `rel` (relative L2) away from nsteps = a;
# tol, stop: `tol` with nsteps = 500 gives a history of length `stop`;  wrong_stop: the lengths an `any`, a slot-0-only and a slot-1-only rule give
CASES = {
    "I": dict(pol="I", table={9: (184.15, 125.27), 10: (119.48, 146.12), 11: (146.33, 87.203), 12: (60.307, 125.54), 13: (58.664, 74.967)},
              held=[(10, 11), (12, 13)], moved=[(11, 12, 0.111)], tol=100.0, stop=14, wrong_stop=dict(any=12, slot0=13, slot1=12)),
    "P": dict(pol="P", table={8: (0.41445, 0.30509), 9: (0.53483, 0.22745), 10: (0.23476, 0.16259)},
              held=[(9, 10)], moved=[(10, 11, 0.122)], tol=0.35, stop=11, wrong_stop=dict(any=9)),
    "IP": dict(pol="IP", table={9: (186.38, 1145.2), 10: (121.88, 1115.6), 11: (148.56, 388.70), 12: (60.808, 314.36), 13: (59.227, 217.49)},
               held=[(11, 12)], moved=[(12, 13, 0.093)], tol=250.0, stop=14, wrong_stop=dict(slot0=10)),
}
NSTEPS_MAX = 14
MARGIN = 0.10                                  # every comparison that decides a branch clears it by 10 % ...
NARROW = {("IP", 10): 0.02}                    # ... but the update of case IP at index 10: 1115.6 < 1145.2, 2.6 %


def nsteps_of(case):
    """every `nsteps` a test solves the case with at tol = 0: both sides of each pair, and the length of the stopped solve"""
    c = CASES[case]
    return sorted({n for pair in c["held"] + [m[:2] for m in c["moved"]] for n in pair} | {c["stop"]})


class _Remembering(O.DataSet):
    """the oracle's data set with `gradientf_logpdf` remembered by its arguments: the solves of a case at consecutive `nsteps`, and the stopped
    one, walk the same iterates, so each A p is evaluated once (conjugate_gradient itself runs every time: its rules are the subject)"""

    @classmethod
    def of(cls, ds):
        new = copy.copy(ds)
        new.__class__ = cls
        new._seen, new._L = {}, None
        return new

    def gradientf_logpdf(self, fh, L, d):
        key = (id(L), fh.tobytes(), d.tobytes())
        if key not in self._seen:
            self._seen[key] = super().gradientf_logpdf(fh, L, d)
        return self._seen[key]


_sims, _solves = {}, {}


def sim(case, T=np.float64):
    """oracle.load_sim of a case in precision T: dict(ds, d, phi, ...) with a ϕ per slot.  The float32 run's d and ϕ are the float64 run's, rounded
    (identical inputs on both sides of a budget, and what the device in single precision is handed).  Made once, never modified."""
    key = (case, np.dtype(T).name)
    if key not in _sims:
        so = O.load_sim(THETA, SHAPE, CASES[case]["pol"], T, beam_fwhm=BEAM, pixel_mask=PM, Nbatch=NB)
        if np.dtype(T) != np.float64:
            s64 = sim(case)
            so["d"], so["phi"] = s64["d"].astype(np.complex64), s64["phi"].astype(np.complex64)
        so["ds"] = _Remembering.of(so["ds"])
        for k in ("d", "phi"):
            so[k].flags.writeable = False
        _sims[key] = so
    return _sims[key]


def solve(case, T=np.float64, nsteps=NSTEPS_MAX, tol=0.0):
    """(best iterate (NB, P, Nx, Nyh), residual history (length, NB)) of the oracle's Wiener filter.  Made once per argument set, read-only."""
    key = (case, np.dtype(T).name, nsteps, tol)
    if key not in _solves:
        so = sim(case, T)
        x, hist = so["ds"].argmaxf_logpdf(so["phi"], d=so["d"], tol=tol, nsteps=nsteps)
        x, h = np.array(x), np.array([np.atleast_1d(r) for _, r in hist])
        x.flags.writeable = h.flags.writeable = False
        _solves[key] = (x, h)
    return _solves[key]


def replay(hist, rule="all", tol=None):
    """A residual history (n, B) under a best-iterate / stop rule: (best[i] = the history index whose iterate is held after entry i, length of the
    history with the stop at `tol`).  "all" is the reference's (:110-112, :119-121: every slot must improve, all stored bests are replaced together;
    every slot below tol); "any": one slot suffices; "slot0" / "slot1": that slot alone; "per_slot" (best only): a best residual per slot, replaced
    slot by slot, the iterate taken when all improve on it."""
    hist = np.asarray(hist)
    pick = {"all": np.all, "any": np.any, "slot0": lambda v: v[0], "slot1": lambda v: v[1], "per_slot": np.all}[rule]
    bestres, best, length = hist[0].copy(), [0], len(hist)
    for i in range(1, len(hist)):
        better = hist[i] < bestres
        if pick(better):
            bestres = hist[i].copy()
        elif rule == "per_slot":
            bestres = np.where(better, hist[i], bestres)
        best.append(i if pick(better) else best[-1])
        if tol is not None and pick(hist[i] < tol):
            length = i + 1
            break
    return best, length


def margins(hist, tol=None):
    """by how much the comparison that decides each branch of the reference's rules clears it, per history index >= 1: an update needs every
    slot below the stored best (the narrowest slot decides), a hold needs one slot not below it (the clearest slot decides); likewise the stop.
    Returns (dict index -> margin of the best-iterate branch, dict index -> margin of the stop branch up to the stop)."""
    hist = np.asarray(hist, float)
    bestres, mb, ms = hist[0].copy(), {}, {}
    for i in range(1, len(hist)):
        if np.all(hist[i] < bestres):
            mb[i] = float(np.min(bestres / hist[i] - 1))
            bestres = hist[i].copy()
        else:
            mb[i] = float(np.max(hist[i] / bestres - 1))
    for i in range(1, len(hist)) if tol is not None else ():
        if np.all(hist[i] < tol):
            ms[i] = float(np.min(tol / hist[i] - 1))
            break
        ms[i] = float(np.max(hist[i] / tol - 1))
    return mb, ms


def slot_rel(a, b):
    """relative L2 distance per batch slot"""
    a, b = np.asarray(a), np.asarray(b)
    ax = tuple(range(1, a.ndim))
    return np.sqrt(np.sum(np.abs(a - b) ** 2, axis=ax) / np.sum(np.abs(b) ** 2, axis=ax))


def distance(q, a, b):
    """the figure of the budget: the largest relative error of a residual history ("hist"), the largest per-slot relative L2 of an iterate ("x")"""
    a, b = np.asarray(a), np.asarray(b)
    if q == "hist":
        return float(np.max(np.abs(a.astype(np.float64) - b) / np.abs(b)))
    return float(np.max(slot_rel(a.astype(b.dtype), b)))


# single precision: the larger of the class bound (cgtol of test_gpu_parity.test_dataset_gradientf_and_wiener) and 3 x the float32 oracle's own
# distance from the float64 oracle (another FFT, another summation order: the rule of tests/golden/bilinear_budget.json); double: the class bound
CLASS = {"f32": dict(hist=1e-3, x=4e-6), "f64": dict(hist=1e-8, x=1e-9)}


def bound(budget, prec, case, run, q):
    return CLASS[prec][q] if prec == "f64" else max(CLASS[prec][q], 3 * budget["cases"][case][run][q])
