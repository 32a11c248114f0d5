"""Every lensing operator in every basis pair against itself in its native pair, through the public Python API.

Each operator carries its data in one basis pair (the native pair); an argument or a result in another basis passes the boundary shell of the
library first (Ctx::as_maps / from_maps / convert).  The shell must be a plain basis conversion: for every operator, mode,
bi, bo in {MAP, FOURIER, HARMONIC}

    op(mode, x_bi, basis_out=bo)  ==  convert(op(mode, convert(x_bi, bi -> ni), basis_out=no), no -> bo)

with (ni, no) the native pair, `convert` = ProjLambert.convert.  The native pair is what the class carries: MAP -> MAP for L*f and L\\f of every
class and for all four actions of BilinearLens (it multiplies maps), FOURIER -> FOURIER for the adjoint actions of LenseFlow and PowerLens.
BilinearLens' adjoint actions are checked against the FOURIER -> FOURIER route as well, within the class bound.

EXACT (torch.equal) where both sides launch the same kernels on the same numbers; an F2ref followed by a ref2F is a permutation and back and
does not count.  That is the case unless one side passes a transform pair that the other does not (irfft2 then rfft2, or the reverse, of
data the other side uses as given):
  BilinearLens     all four actions and the in-place MAP -> MAP call; with ϕ = 0 (the operator is then the conversion bi -> bo) unless both
                   bi and bo are Fourier bases
  LenseFlow        L*f, L\\f: all;  L'g, L'\\g: a FOURIER / HARMONIC argument
  PowerLens(0)     L*f: unless both bi and bo are Fourier bases (the operator is the conversion);  L'g: all
  PowerLens(2)     L*f: a MAP argument;  L'g: a FOURIER / HARMONIC argument
  Taylens(1)       L*f: a MAP argument
  project => ProjHealpix(2)   all (input side only)
Everything else runs an equivalent sequence and is held to the transform class bound of DESIGN.md §3 through tests/_tol.py: relative L2 error
1.5e-6 in float32, 1e-12 in float64.  Measured on MI355X: profiles/operator_bases_parity.txt.

Grid: shapes 32 x 32 (power-of-two transforms, one-launch small flow), 32 x 128 (power-of-two, staged flow), 12 x 20 (any-size transforms);
P in {1, 2, 3}, B in {1, 2}, both precisions; ϕ seeded with 0.5 px rms deflection (tests/_bilinear_ref.py make_phi).  With CMBL_DIGEST_LOG=<path>
every output of the operator under test appends `key sha256(bytes)`, and every test case closes with `= case sha256(its lines)`: two builds
that launch the same kernels write the same file.  profiles/operator_shell_digests.txt holds the `=` lines of the current library (`grep '^='`
of the log; 5904 outputs): a case whose line moves is found by comparing the two full logs."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _bilinear_ref as R
from _tol import close

DT = {"f32": torch.float32, "f64": torch.float64}
BOUND = {"f32": 1.5e-6, "f64": 1e-12}
MAP, FOURIER, HARMONIC = 0, 1, 2
BASES = (MAP, FOURIER, HARMONIC)
FWD, INV, ADJ, INVADJ = 0, 1, 2, 3
SHAPES = [(32, 32), (32, 128), (12, 20)]                # (Ny, Nx)
PB = [(P, B) for P in (1, 2, 3) for B in (1, 2)]
fourier = lambda b: b != MAP


def _pkg():
    import cmblensing_jl_amd as C
    return C


_projs, _phis = {}, {}


def proj(Ny, Nx, prec, theta=R.THETA):
    k = (Ny, Nx, prec, theta)
    if k not in _projs:
        _projs[k] = _pkg().ProjLambert(Ny, Nx, theta, DT[prec])
    return _projs[k]


def phi_of(p, zero=False):
    k = (id(p), zero)
    if k not in _phis:
        a = np.zeros((p.Nx, p.Ny)) if zero else R.make_phi(p.Ny, p.Nx, p.theta_pix, 0.5, p.Ny + p.Nx)
        _phis[k] = _pkg().Field(p, p.tensor(a[None, None]), MAP)
    return _phis[k]


_case = [hashlib.sha256()]              # over the lines of the running test case


def _log(line):
    path = os.environ.get("CMBL_DIGEST_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line)


def digest(key, t):
    line = f"{key} {hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}\n"
    _case[0].update(line.encode())
    _log(line)


def close_case(name):
    _log(f"= {name} {_case[0].hexdigest()}\n")
    _case[0] = hashlib.sha256()


class Op:
    """name, constructor, {mode name: (mode, native pair)}, exact(mode, bi, bo), and the call"""

    def __init__(self, name, make, modes, exact, zero_phi=False):
        self.name, self.make, self.modes, self.exact, self.zero_phi = name, make, modes, exact, zero_phi

    def call(self, L, mode, x, bo):
        return L._apply(mode, x, basis_out=bo)


MM, FF = (MAP, MAP), (FOURIER, FOURIER)
OPS = [
    Op("LenseFlow1", lambda C, p: C.LenseFlow(p, nsteps=1), {"L*f": (FWD, MM), "L\\f": (INV, MM), "L'g": (ADJ, FF), "L'\\g": (INVADJ, FF)},
       lambda m, bi, bo: m in (FWD, INV) or fourier(bi)),
    Op("BilinearLens", lambda C, p: C.BilinearLens(p), {"L*f": (FWD, MM), "L\\f": (INV, MM), "L'g": (ADJ, MM), "L'\\g": (INVADJ, MM)},
       lambda m, bi, bo: True),
    Op("BilinearLens_phi0", lambda C, p: C.BilinearLens(p), {"L*f": (FWD, MM), "L\\f": (INV, MM), "L'g": (ADJ, MM), "L'\\g": (INVADJ, MM)},
       lambda m, bi, bo: not (fourier(bi) and fourier(bo)), zero_phi=True),
    Op("PowerLens2", lambda C, p: C.PowerLens(p, 2), {"L*f": (FWD, MM), "L'g": (ADJ, FF)},
       lambda m, bi, bo: (bi == MAP) if m == FWD else fourier(bi)),
    Op("PowerLens0", lambda C, p: C.PowerLens(p, 0), {"L*f": (FWD, MM), "L'g": (ADJ, FF)},
       lambda m, bi, bo: m == ADJ or not (fourier(bi) and fourier(bo))),
    Op("Taylens1", lambda C, p: C.Taylens(p, 1), {"L*f": (FWD, MM)}, lambda m, bi, bo: bi == MAP),
]


def arguments(p, P, B):
    """white noise in the three bases, made once per (P, B): {basis: Field}"""
    C = _pkg()
    x = np.random.default_rng(1000 * p.Ny + 10 * P + B).standard_normal((B, P, p.Nx, p.Ny))
    xm = C.Field(p, p.tensor(x), MAP)
    return {b: xm.to(b) for b in BASES}


def compare(bad, key, exact, got, want, prec):
    """got, want: tensors.  Collects a failure instead of raising: every comparison of the case is made and logged."""
    if exact:
        if not torch.equal(got, want):
            d = (got - want).abs().max().item()
            bad.append(f"{key}: not bit-identical (max abs difference {d:.3e})")
        return
    g, w = got.cpu().numpy(), want.cpu().numpy()
    try:
        close(key, g, w, BOUND[prec])
    except AssertionError as e:
        bad.append(str(e))


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx", SHAPES)
@pytest.mark.parametrize("op", OPS, ids=[o.name for o in OPS])
def test_every_basis_pair_is_the_native_pair_converted(op, Ny, Nx, prec):
    C = _pkg()
    p = proj(Ny, Nx, prec)
    L = op.make(C, p)(phi_of(p, op.zero_phi))
    bad = []
    for P, B in PB:
        x = arguments(p, P, B)
        for q, (mode, (ni, no)) in op.modes.items():
            via_ff = op.name == "BilinearLens" and mode in (ADJ, INVADJ)        # ... through the FOURIER -> FOURIER route as well
            for bi in BASES:
                native = op.call(L, mode, x[bi].to(ni), no)
                want = {bo: native.to(bo).arr for bo in BASES}
                alt = {bo: op.call(L, mode, x[bi].to(FOURIER), FOURIER).to(bo).arr for bo in BASES} if via_ff else None
                for bo in BASES:
                    key = f"{op.name}|{Ny}x{Nx}|{prec}|P{P}B{B}|{q}|{bi}->{bo}"
                    got = op.call(L, mode, x[bi], bo)
                    assert got.basis == bo
                    digest(key, got.arr)
                    compare(bad, key, op.exact(mode, bi, bo), got.arr, want[bo], prec)
                    if alt is not None:
                        compare(bad, key + "|via F->F", False, got.arr, alt[bo], prec)
    close_case(f"{op.name}|{Ny}x{Nx}|{prec}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx", SHAPES)
def test_bilinear_in_place_map_to_map(Ny, Nx, prec):
    """`out` is the argument: the gathers cannot run in place, the result passes a scratch map"""
    C = _pkg()
    p = proj(Ny, Nx, prec)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for zero in (False, True):
        L = C.BilinearLens(p)(phi_of(p, zero))
        for P, B in PB:
            x = arguments(p, P, B)[MAP]
            for mode in (FWD, INV, ADJ, INVADJ):
                want = L._apply(mode, x, basis_out=MAP).arr
                buf = x.arr.clone()
                assert p.lib.cmbl_bilinear_apply(L._h, mode, MAP, ptr(buf), MAP, ptr(buf), P, B, 5) == 0
                digest(f"BilinearLens{'_phi0' if zero else ''}|{Ny}x{Nx}|{prec}|P{P}B{B}|mode{mode}|in place", buf)
                assert torch.equal(buf, want), (zero, P, B, mode)
    close_case(f"BilinearLens in place|{Ny}x{Nx}|{prec}")


def hpx_theta(Ny, Nx):
    """pixel size in arcmin at which the longer half side of the patch is 1.2 rad: Nside 2 pixels (30 degrees apart) fall inside"""
    return float(np.rad2deg(1.2 / (max(Ny, Nx) / 2 + 0.5)) * 60)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Ny,Nx", SHAPES)
def test_project_to_healpix_input_bases(Ny, Nx, prec):
    C = _pkg()
    p = proj(Ny, Nx, prec, hpx_theta(Ny, Nx))
    hp = C.ProjHealpix(2)
    pr = C.Projector(hp, p)
    assert pr.n_touched > 0
    bad = []
    for P, B in PB:
        x = arguments(p, P, B)
        want = C.project(x[MAP], hp, projector=pr).arr
        assert torch.count_nonzero(want) > 0
        for bi in BASES:
            key = f"ProjHealpix2|{Ny}x{Nx}|{prec}|P{P}B{B}|{bi}"
            got = C.project(x[bi], hp, projector=pr).arr
            digest(key, got)
            # the native argument is the MAP field: convert(x_bi, bi -> MAP) first
            via = C.project(x[bi].to(MAP), hp, projector=pr).arr
            compare(bad, key, True, got, via, prec)
            if bi == MAP:
                compare(bad, key + "|itself", True, got, want, prec)
    close_case(f"ProjHealpix2|{Ny}x{Nx}|{prec}")
    assert not bad, "\n".join(bad)
