"""CPU-side checks of the θ-gradient on the device: the header declares its entry points and the built library exports them, lib.py binds
them with the header's argument count, the Julia glue wraps them, the package exports the two functions, and the MUSE adapter still
differentiates by central differences unless asked otherwise."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cmbl_grad_theta_logpdf", "cmbl_grad_theta_logpdf_mixed")


def test_entry_points_declared_exported_and_bound():
    import __graft_entry__ as g
    hdr = open(os.path.join(ROOT, "include", "cmblens.h"), encoding="utf-8").read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(g.build())
    from cmblensing_jl_amd.lib import SIGNATURES
    glue = open(os.path.join(ROOT, "julia", "CMBLensingHIPExt.jl"), encoding="utf-8").read()
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in include/cmblens.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert len(SIGNATURES[name]) == len(m.group(1).split(",")), name        # the ctypes binding has the header's argument count
        assert len(re.findall(r"\b%s\b" % name, hdr)) >= 2, f"{name} is not documented in the header"   # the declaration and its comment block
        assert f":{name}," in glue, f"{name} has no ccall wrapper in julia/CMBLensingHIPExt.jl"
    for flag, value in (("CMBL_THETA_R", 1), ("CMBL_THETA_APHI", 2), ("CMBL_THETA_AMPS", 4)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (flag, value), code), flag


def test_python_surface():
    import cmblensing_jl_amd as C
    from cmblensing_jl_amd import theta
    assert C.grad_theta_logpdf is theta.grad_theta_logpdf and C.grad_theta_logpdf_mixed is theta.grad_theta_logpdf_mixed
    assert list(inspect.signature(C.grad_theta_logpdf).parameters) == ["ds", "f", "phi", "theta"]
    assert list(inspect.signature(C.grad_theta_logpdf_mixed).parameters) == ["ds", "fo", "po", "theta"]
    assert (theta.WANT_R, theta.WANT_APHI, theta.WANT_AMPS) == (1, 2, 4)


def test_muse_default_is_finite_differences():
    import pytest
    import cmblensing_jl_amd as C
    assert inspect.signature(C.CMBLensingMuseProblem.__init__).parameters["grad"].default == "fd"

    class _DS:                                                     # the constructor only keeps the data set and reads its data
        d = None
    assert C.CMBLensingMuseProblem(_DS()).grad == "fd"
    assert C.CMBLensingMuseProblem(_DS(), grad="device").grad == "device"
    with pytest.raises(ValueError):
        C.CMBLensingMuseProblem(_DS(), grad="autodiff")
