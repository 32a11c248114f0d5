"""CPU-side checks of the θ layer on the device: the header declares its entry points and the built library exports them, the Python surface
has the new switches with unchanged defaults, and the package exports the grid call."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cmbl_dataset_theta_model", "cmbl_logpdf_mixed_theta", "cmbl_dataset_theta_ops")


def test_entry_points_declared_exported_and_bound():
    import __graft_entry__ as g
    hdr = open(os.path.join(ROOT, "include", "cmblens.h"), encoding="utf-8").read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(g.build())
    from cmblensing_jl_amd.lib import SIGNATURES
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in include/cmblens.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert len(SIGNATURES[name]) == len(m.group(1).split(",")), name        # the ctypes binding has the header's argument count
        assert hdr.count(name) >= 2, f"{name} is not documented in the header"       # the declaration and its comment block
    glue = open(os.path.join(ROOT, "julia", "CMBLensingHIPExt.jl"), encoding="utf-8").read()
    for name in ENTRY_POINTS:
        assert f":{name}" in glue, f"{name} has no ccall wrapper in julia/CMBLensingHIPExt.jl"


def test_python_surface_defaults_are_host():
    import cmblensing_jl_amd as C
    assert callable(C.logpdf_mixed_theta_grid) and callable(C.theta_ops_device)
    assert inspect.signature(C.gibbs_sample_theta).parameters["on"].default == "host"
    assert inspect.signature(C.sample_joint).parameters["theta_on"].default == "host"
    assert list(inspect.signature(C.logpdf_mixed_theta_grid).parameters) == ["ds", "fo", "po", "thetas"]
