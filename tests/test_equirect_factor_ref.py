"""The one-sided Jacobi scheme of csrc/kernels_equirect_factor.hpp, restated in NumPy (tests/_equirect_factor_ref.py: the same pair schedule,
threshold, skip rules and noise floor), on the CPU: the schedule visits every pair once per sweep in rounds of disjoint pairs; on EVERY input
of tests/test_gpu_equirect_factor.py it converges in at most 30 sweeps -- half the cap of 60, so the cap cannot hide a failure -- and agrees
with LAPACK to 1e-12; it terminates on the zero block and on the rank-deficient blocks."""
import numpy as np
import pytest

import _equirect_factor_ref as F
import _equirect_ref as R

CASES = [(Ny, Nx, n, cplx) for Ny, Nx in F.SHAPES for n, cplx in F.kinds(Ny)]


def test_every_pair_once_per_sweep_in_disjoint_rounds():
    for n in range(2, 132):
        rounds = F.schedule(n)
        assert len(rounds) == n + (n & 1) - 1
        seen = set()
        for pr in rounds:
            cols = [c for p in pr for c in p]
            assert len(cols) == len(set(cols)) and len(pr) == n // 2           # disjoint; an odd n rests one column per round
            assert all(0 <= i < j < n for i, j in pr)
            seen.update(pr)
        assert len(seen) == n * (n - 1) // 2 == sum(len(pr) for pr in rounds)  # every pair, exactly once


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("case", CASES, ids=[f"{'c' if c else 'r'}{n}" for _, _, n, c in CASES])
def test_restatement_converges_and_agrees_with_lapack(case):
    Ny, Nx, n, cplx = case
    Mh = Nx // 2 + 1
    ins = F.svd_inputs(n, Mh, cplx)
    assert np.linalg.cond(R._ref(ins["gauss"])).max() <= 1e3
    A = np.concatenate([R._ref(ins[k]) for k in F.KINDS])                    # the blocks are independent: one run for all of them
    G, V, sig, sweeps, done = F.jacobi_svd(A)
    r = n - n // 2
    for i, kind in enumerate(F.KINDS):
        sl = slice(i * Mh, (i + 1) * Mh)
        a, rtol = A[sl], (1e-10 if kind == "halfrank" else 1e-15)
        print(f"{kind}: sweeps {sweeps[sl].max()}")
        assert done[sl].all() and sweeps[sl].max() <= 30, (kind, sweeps[sl])
        sq, pi = F.assemble(G[sl], V[sl], sig[sl], rtol)
        ref = np.linalg.svd(a, compute_uv=False)
        assert np.max(np.abs(-np.sort(-sig[sl], axis=1) - ref)) <= 1e-12 * ref.max()
        assert _rel(pi, np.linalg.pinv(a, rcond=rtol)) <= 1e-12, kind
        if kind in ("general", "spd", "gauss"):
            assert _rel(sq, R._ref(R.op_sqrt(R._ref(a)))) <= 1e-12, kind
        elif kind == "zeroblock":
            assert not sq[1].any() and not pi[1].any() and sweeps[sl][1] == 1    # nothing to rotate: one clean sweep
        elif kind == "halfrank":
            assert ref[:, r - 1].min() >= 0.5 and (r == n or ref[:, r:].max() <= 1e-14)
        else:                                                                # Hermitian PSD of half rank: S S = A to rounding
            assert np.linalg.norm(sq @ sq - a) <= n * 2.0 ** -52 * np.linalg.norm(sq) ** 2 * Mh
