"""The data-dependent rules of the Wiener filter's conjugate gradient (src/numerical_algorithms.jl:106-125) in both hand-written forms of the
iteration: `all(res < bestres)` replaces the best iterate and the stored best residual of ALL batch slots together; `all(res < tol)` stops the
solve; what the host had enqueued past the stop changes nothing.
  fused    : CgSolver::solve_fused with PwCgStart / PwCgXr / PwCgP and k_cg_init around Dataset::flow_Ap (PwCgAp; a LenseFlow on a power-of-two map; the default)
  composed : CgSolver::solve with k_cg_start / alpha / xr / beta / p / keep_best (here: option fused_harm off, CMBL_NO_FUSED_HARM=1)
on the three two-slot data sets of tests/_cg_rules_ref.py (32 x 32, I / P / IP, theta = 3', mask, no beam), whose slots disagree between the
steps 10 and 14: tests/test_cg_rules_ref.py asserts every branch used here with its margin, on the CPU.  A per-slot or `any` rule, a best
residual replaced slot by slot, a parity mix-up of the double-buffered state, a stop that reads some slots only, or a latch that lets one more
iteration through moves a returned iterate by about 10 % or changes a history length.
Bounds (tests/_cg_rules_ref.bound): double precision the class bounds of test_gpu_parity.test_dataset_gradientf_and_wiener (residual 1e-8,
iterate 1e-9); single precision max(class bound 1e-3 / 4e-6, 3 x the float32 oracle's own distance from the float64 oracle, which
tests/golden/cg_rules_budget.json records per case and solve).  Measured: profiles/cg_rules_parity.txt."""
import contextlib
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _cg_rules_ref as R
import test_gpu_parity as TP
from _tol import close, scalars_close

PRECS, FORMS = ["f32", "f64"], ["fused", "composed"]
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cg_rules_budget.json")) as _f:
    BUDGET = json.load(_f)
ERR_NAN = 4                                                  # CMBL_ERR_NAN (include/cmblens.h)


@contextlib.contextmanager
def _form_env(form):
    """option fused_harm is read from CMBL_NO_FUSED_HARM when a context is created"""
    old = os.environ.pop("CMBL_NO_FUSED_HARM", None)
    if form == "composed":
        os.environ["CMBL_NO_FUSED_HARM"] = "1"
    try:
        yield
    finally:
        os.environ.pop("CMBL_NO_FUSED_HARM", None)
        if old is not None:
            os.environ["CMBL_NO_FUSED_HARM"] = old


_devices = {}


class Device:
    """the device data set of a case in one precision and one form of the iteration, made once; d and ϕ are the oracle's"""

    def __init__(self, prec, case, form):
        with _form_env(form):
            self.C, so, sd = TP._dataset_pair(prec, R.CASES[case]["pol"], R.SHAPE, theta=R.THETA, mask=True, beam=R.BEAM, B=R.NB)
        ref = R.sim(case)
        assert np.array_equal(so["d"], ref["d"]) and np.array_equal(so["phi"], ref["phi"])       # the data set of the fixtures
        self.ds, self.p, self.form = sd["ds"], sd["proj"], form
        self.d, self.phi = self.p.tensor(np.array(ref["d"])), self.p.tensor(np.array(ref["phi"]))
        self.check_form()

    def solve(self, nsteps, tol=0.0, d=None, phi=None):
        """(iterate tensor (B, P, Nx, Nyh), history (length, B))"""
        C, p = self.C, self.p
        fw, hist = self.ds.argmaxf_logpdf(C.Field(p, self.phi if phi is None else phi, C.FOURIER), d=C.Field(p, self.d if d is None else d, C.HARMONIC),
                                          tol=tol, nsteps=nsteps)
        return fw.arr, np.array([r for _, r in hist]).reshape(len(hist), -1)

    def check_form(self):
        """the form really runs: the fused iteration launches row-carrier kernels (class x_harm), the composed one none"""
        self.p.prof_enable()
        self.p.prof_reset()
        self.solve(3)
        table = self.p.prof_table()
        self.p.prof_enable(False)
        assert ("x_harm" in table) == (self.form == "fused"), (self.form, sorted(table))
        assert "cg_update" in table, sorted(table)


def device(prec, case, form):
    key = (prec, case, form)
    if key not in _devices:
        _devices[key] = Device(prec, case, form)
    return _devices[key]


def against_oracle(prec, case, n, x, hist, slots=(0, 1)):
    """a device solve of length n against the float64 oracle's tol = 0, nsteps = n solve: history exact in length, every entry and the iterate of
    every slot within the bound.  slots: the device slots that carry the oracle's slot 0 and slot 1."""
    xo, ho = R.solve(case, np.float64, n)
    assert hist.shape[0] == ho.shape[0] == n, (hist.shape, n)
    sl = list(slots)
    scalars_close(("hist", case, n), hist[:, sl], ho, rtol=R.bound(BUDGET, prec, case, f"n{n}", "hist"))
    xs = x[sl].cpu().numpy()
    for k in range(2):
        close(("x", case, n, "slot", k), xs[k], xo[k], R.bound(BUDGET, prec, case, f"n{n}", "x"))


def held_and_moved(prec, case, solves):
    """solves: nsteps -> (iterate, history).  Where the rule holds the iterate, one more step returns it bit for bit in every slot; where it
    replaces it, every slot moves (about 10 %; a held slot would be at 0)."""
    c = R.CASES[case]
    for a, b in c["held"]:
        assert torch.equal(solves[a][0], solves[b][0]), f"nsteps = {b} does not return the nsteps = {a} iterate"
    for a, b, _ in c["moved"]:
        moved = R.slot_rel(solves[b][0].cpu().numpy(), solves[a][0].cpu().numpy())
        print("moved", case, a, b, moved)
        assert np.all(moved > 0.05), (a, b, moved)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", sorted(R.CASES))
@pytest.mark.parametrize("prec", PRECS)
def test_best_iterate_is_replaced_when_all_slots_improve(prec, case, form):
    dev = device(prec, case, form)
    ns = sorted({n for pair in R.CASES[case]["held"] + [m[:2] for m in R.CASES[case]["moved"]] for n in pair})
    solves = {n: dev.solve(n) for n in ns}
    for n in ns:
        against_oracle(prec, case, n, *solves[n])
    held_and_moved(prec, case, solves)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", sorted(R.CASES))
@pytest.mark.parametrize("prec", PRECS)
def test_stop_when_all_slots_are_below_tol_and_nothing_after(prec, case, form):
    c = R.CASES[case]
    dev = device(prec, case, form)
    x, h = dev.solve(500, tol=c["tol"])
    print("stopped", case, len(h), h[-2:])
    assert len(h) == c["stop"], (len(h), c["stop"])
    assert np.all(h[-1] < c["tol"]) and not np.all(h[-2] < c["tol"]), h[-2:]
    # the iterations enqueued past the stop changed nothing: the solve of exactly that length, which never stops early
    xn, hn = dev.solve(len(h), tol=0.0)
    assert torch.equal(x, xn) and np.array_equal(h, hn)
    x2, h2 = dev.solve(500, tol=c["tol"])                                                            # and again: nothing is left behind
    assert torch.equal(x, x2) and np.array_equal(h, h2)
    against_oracle(prec, case, c["stop"], x, h)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B", [16, 17])
@pytest.mark.parametrize("prec", PRECS)
def test_more_slots_the_last_one_disagrees(prec, B, form):
    """case I with B = 16 (the last B whose r'z the fused PwCgP sums in its prologue) and B = 17 (the first with k_finish_parts and rz_fin): slots
    0 ... B - 2 carry slot 0's d and ϕ, the last slot carries slot 1's, so a rule that reads the first slots only (or the first 16) sees no
    disagreement at all"""
    case, c = "I", R.CASES["I"]
    dev = device(prec, case, form)
    pick = [0] * (B - 1) + [1]
    d, phi = dev.d[pick].contiguous(), dev.phi[pick].contiguous()
    solves = {n: dev.solve(n, d=d, phi=phi) for n in (10, 11, 12, 13)}
    solves[14] = dev.solve(500, tol=c["tol"], d=d, phi=phi)
    assert len(solves[14][1]) == c["stop"] == 14
    xn, hn = dev.solve(14, d=d, phi=phi)
    assert torch.equal(solves[14][0], xn) and np.array_equal(solves[14][1], hn)
    for n, (x, h) in solves.items():
        assert x.shape[0] == B and h.shape == (n, B)
        for k in range(1, B - 1):                                                                    # the copies are copies
            assert torch.equal(x[k], x[0]) and np.array_equal(h[:, k], h[:, 0]), (n, k)
        against_oracle(prec, case, n, x, h, slots=(0, B - 1))
    held_and_moved(prec, case, solves)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("prec", PRECS)
def test_a_slot_of_zero_data_is_a_nan_error_and_leaves_nothing_behind(prec, form):
    """case I with d[1] = 0: res = r'z = 0 in slot 1, so alpha = 0 / 0 at step 2 and the residual is NaN from there.  The solve returns CMBL_ERR_NAN
    (an error return on NaN values, the kernels run to completion), and the next valid solve on the same data set is the one before it, bit for bit."""
    dev = device(prec, "I", form)
    before = dev.solve(13)
    d0 = dev.d.clone()
    d0[1] = 0
    with pytest.raises(dev.C.CmblError) as e:
        dev.solve(20, d=d0)
    assert e.value.code == ERR_NAN and "NaN residual" in str(e.value), str(e.value)
    after = dev.solve(13)
    assert torch.equal(before[0], after[0]) and np.array_equal(before[1], after[1])
