"""Guards the fixtures of tests/test_gpu_cg_rules.py on the CPU (tests/_cg_rules_ref.py): three two-slot data sets at 32 x 32 on which the
conjugate gradient's `all(res < bestres)` and `all(res < tol)` (src/numerical_algorithms.jl:110-121) decide differently from a per-slot, an `any`
or a one-slot rule.  Every branch the GPU tests rely on is asserted here with its margin, in the float64 oracle and in the float32 one, so a
fixture that goes stale (a changed simulation, spectrum or mask) fails here and not as a device mismatch."""
import json
import os

import numpy as np
import pytest

import _cg_rules_ref as R

CASES = sorted(R.CASES)
lt = lambda lo, hi: hi / lo - 1                # by how much lo < hi holds (negative: it does not)


@pytest.mark.parametrize("case", CASES)
def test_residuals_are_those_of_the_table(case):
    x, h = R.solve(case)
    assert h.shape == (R.NSTEPS_MAX, R.NB) and x.shape[0] == R.NB
    for i, row in R.CASES[case]["table"].items():
        np.testing.assert_allclose(h[i], row, rtol=1e-4, err_msg=f"history index {i}")          # 5 digits in the table


def test_case_I_branches():
    h = R.solve("I")[1]
    m = R.MARGIN
    # step 11 (index 10): slot 0 falls, slot 1 rises -> no update, in either slot
    assert lt(h[10, 0], h[9, 0]) > m and lt(h[9, 1], h[10, 1]) > m
    # step 12 (index 11): slot 0 is above its own residual of step 11 but below the STORED best (index 9); slot 1 falls -> update
    assert lt(h[10, 0], h[11, 0]) > m and lt(h[11, 0], h[9, 0]) > m and lt(h[11, 1], h[9, 1]) > m
    # step 13 (index 12): slot 1 rises -> no update;  step 14 (index 13): both below index 11 -> update
    assert lt(h[11, 1], h[12, 1]) > m and lt(h[12, 0], h[11, 0]) > m
    assert lt(h[13, 0], h[11, 0]) > m and lt(h[13, 1], h[11, 1]) > m
    assert R.replay(h, "all")[0][9:] == [9, 9, 11, 11, 13]
    assert R.replay(h, "any")[0][9:] == [9, 10, 11, 12, 13] and R.replay(h, "per_slot")[0][9:] == [9, 9, 9, 9, 13]
    # tol = 100: slot 1 is below at index 11 and back above at index 12; both below at index 13
    assert lt(h[11, 1], 100) > m and lt(100, h[11, 0]) > m and lt(100, h[12, 1]) > m and lt(h[12, 0], 100) > m
    assert lt(h[13, 0], 100) > m and lt(h[13, 1], 100) > m


def test_case_P_branches():
    h = R.solve("P")[1]
    m = R.MARGIN
    assert lt(h[8, 0], h[9, 0]) > m and lt(h[9, 1], h[8, 1]) > m                                   # index 9: slot 0 rises, slot 1 falls -> no update
    assert lt(h[10, 0], h[8, 0]) > m and lt(h[10, 1], h[8, 1]) > m                                 # index 10: update
    assert R.replay(h, "all")[0][8:11] == [8, 8, 10] and R.replay(h, "any")[0][8:11] == [8, 9, 10]
    assert lt(h[8, 1], 0.35) > m and lt(0.35, h[8, 0]) > m and lt(0.35, h[9, 0]) > m              # tol = 0.35: slot 1 alone is below from index 8 on
    assert lt(h[10, 0], 0.35) > m and lt(h[10, 1], 0.35) > m


def test_case_IP_branches():
    h = R.solve("IP")[1]
    m = R.MARGIN
    assert lt(h[10, 0], h[9, 0]) > m and lt(h[10, 1], h[9, 1]) > R.NARROW[("IP", 10)]             # index 10: update, slot 1 by 2.6 %
    assert lt(h[10, 1], h[9, 1]) < m                                                                # (the narrow one: it is why the bound is 2 % here)
    assert lt(h[10, 0], h[11, 0]) > m and lt(h[11, 1], h[10, 1]) > m                               # index 11: slot 0 rises, slot 1 falls -> no update
    assert lt(h[12, 0], h[10, 0]) > m and lt(h[12, 1], h[10, 1]) > m                               # index 12: update
    assert R.replay(h, "all")[0][9:13] == [9, 10, 10, 12] and R.replay(h, "any")[0][9:13] == [9, 10, 11, 12]
    assert lt(h[9, 0], 250) > m and lt(250, h[9, 1]) > m and lt(250, h[12, 1]) > m                # tol = 250: slot 0 alone is below from index 9 on
    assert lt(h[13, 0], 250) > m and lt(h[13, 1], 250) > m


@pytest.mark.parametrize("case", CASES)
def test_every_branch_up_to_the_last_step_used_is_clear(case):
    """the branches the tables do not show (the residuals fall in both slots up to index 8) decide which iterate is held before the events: each
    clears its comparison by 2 % at the least, twenty times the single-precision bound on a residual (1e-3); the stop comparisons by 10 %"""
    c = R.CASES[case]
    h = R.solve(case)[1]
    mb, ms = R.margins(h[: max(R.nsteps_of(case))], c["tol"])
    assert min(mb.values()) > 0.02, mb
    assert min(ms.values()) > R.MARGIN and max(ms) + 1 == c["stop"], ms


@pytest.mark.parametrize("case", CASES)
def test_stop_lengths_and_what_the_wrong_rules_give(case):
    c = R.CASES[case]
    h = R.solve(case)[1]
    assert R.replay(h, "all", c["tol"])[1] == c["stop"]
    for rule, n in c["wrong_stop"].items():
        assert R.replay(h, rule, c["tol"])[1] == n != c["stop"], rule
    xs, hs = R.solve(case, nsteps=500, tol=c["tol"])                                                # the oracle itself, stopping
    xn, hn = R.solve(case, nsteps=c["stop"])
    assert len(hs) == c["stop"] and np.array_equal(hs, hn) and np.array_equal(xs, xn)
    assert np.all(hs[-1] < c["tol"]) and not np.all(hs[-2] < c["tol"])


@pytest.mark.parametrize("T", [np.float64, np.float32])
@pytest.mark.parametrize("case", CASES)
def test_consecutive_nsteps(case, T):
    """where the rule holds the iterate, one more step returns the same array bit for bit, in BOTH slots; where it moves, each slot moves by
    about 10 %; a shorter solve's history is the start of a longer one's"""
    c = R.CASES[case]
    for a, b in c["held"]:
        assert np.array_equal(R.solve(case, T, a)[0], R.solve(case, T, b)[0]), (a, b)
    for a, b, want in c["moved"]:
        d = R.slot_rel(R.solve(case, T, b)[0], R.solve(case, T, a)[0])
        assert np.all(d > 0.05), d
        if T is np.float64:
            whole = float(np.linalg.norm(R.solve(case, T, b)[0] - R.solve(case, T, a)[0]) / np.linalg.norm(R.solve(case, T, b)[0]))   # over both slots
            assert abs(whole - want) < 0.001, (whole, want)
    for n in R.nsteps_of(case):
        assert np.array_equal(R.solve(case, T, n)[1], R.solve(case, T)[1][:n])


@pytest.mark.parametrize("case", CASES)
def test_the_float32_oracle_takes_the_same_branches(case):
    c = R.CASES[case]
    h64, h32 = R.solve(case)[1], R.solve(case, np.float32)[1]
    assert h32.dtype == np.float32 and R.solve(case, np.float32)[0].dtype == np.complex64
    assert R.replay(h32, "all", c["tol"]) == R.replay(h64, "all", c["tol"])
    assert R.replay(h32, "all") == R.replay(h64, "all")
    assert len(R.solve(case, np.float32, nsteps=500, tol=c["tol"])[1]) == c["stop"]
    assert R.distance("hist", h32, h64) < 1e-5 and R.distance("x", R.solve(case, np.float32)[0], R.solve(case)[0]) < 1e-5


def test_the_budget_is_the_float32_oracle_s_own_error():
    """tests/golden/cg_rules_budget.json holds what tools/make_cg_rules_budget.py computes (never a device figure), for every run a GPU test compares"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cg_rules_budget.json")) as f:
        budget = json.load(f)
    for case in CASES:
        runs = {f"n{n}" for n in R.nsteps_of(case)}
        assert set(budget["cases"][case]) == runs
        for n in R.nsteps_of(case):
            for q, i in (("x", 0), ("hist", 1)):
                now = R.distance(q, R.solve(case, np.float32, n)[i], R.solve(case, np.float64, n)[i])
                assert 0.5 * now <= budget["cases"][case][f"n{n}"][q] <= 2 * now, (case, n, q)             # (another FFT build moves the last bits of a float32 run)
                assert R.bound(budget, "f32", case, f"n{n}", q) < 10 * R.CLASS["f32"][q]                   # the budget does not open the class bound up
