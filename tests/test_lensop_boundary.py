"""CPU-side checks of the `L` slot of a data set (load_sim(L = BilinearLens), src/dataset.jl:223): the header declares and the library exports the
`cmbl_lensop_*` / `cmbl_*_op` entry points, the fused column pass is a documented option with a translation unit of its own, `load_sim` and
`BaseDataSet` take `L`, and a wrong object in the slot is refused by the type check alone, before any library call."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cmbl_lensop_from_lenseflow", "cmbl_lensop_from_bilinear", "cmbl_lensop_from_powerlens", "cmbl_lensop_destroy",
       "cmbl_gradientf_logpdf_op", "cmbl_wiener_cg_op", "cmbl_grad_logpdf_op"]


@pytest.fixture(scope="module")
def libpath():
    import __graft_entry__ as g
    return g.build()


def test_header_declares_and_library_exports_the_entry_points(libpath):
    hdr = open(os.path.join(ROOT, "include", "cmblens.h"), encoding="utf-8").read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(libpath)
    from cmblensing_jl_amd.lib import SIGNATURES
    for s in NEW:
        assert re.search(r"\bint %s\s*\(" % s, code), s
        assert hasattr(lib, s), s
        assert s in SIGNATURES, s
    assert "typedef struct cmbl_lensop cmbl_lensop;" in code
    assert re.search(r"#define CMBL_ABI_VERSION 3\b", hdr)               # additive: the revision stays
    # the old entry points keep their flow-typed signatures
    assert re.search(r"int cmbl_wiener_cg\(cmbl_dataset\* ds, cmbl_flow\* L,", code) and re.search(r"int cmbl_hmc_step\(cmbl_dataset\* ds, cmbl_flow\* L,", code)
    # the reference's file:line next to the declarations, and the integration guide lists them
    assert "src/dataset.jl:223" in hdr and "src/bilinearlens.jl:165-171" in hdr
    guide = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    for s in NEW:
        assert s in guide, s


def test_lens_fused_is_a_documented_option_with_its_own_translation_unit():
    eng = open(os.path.join(ROOT, "cmblensing.jl_amd", "csrc", "engine.hpp"), encoding="utf-8").read()
    hdr = open(os.path.join(ROOT, "include", "cmblens.h"), encoding="utf-8").read()
    assert 'if (k == "lens_fused") return &opts.lens_fused;' in eng and "CMBL_LENS_FUSED" in eng
    assert '"lens_fused"' in hdr and "CMBL_LENS_FUSED" in hdr
    assert '"lens_y"' in eng and "K_LENS_Y" in eng                       # a kernel class of its own for cmbl_timer_report
    from cmblensing_jl_amd.lib import UNITS
    for u in ("tu_lensop_f32", "tu_lensop_f64"):
        assert u in UNITS and os.path.exists(os.path.join(ROOT, "cmblensing.jl_amd", "csrc", u + ".hip")), u
    # the instances live there and nowhere else: the other units do not include the kernel
    for f in os.listdir(os.path.join(ROOT, "cmblensing.jl_amd", "csrc")):
        src = open(os.path.join(ROOT, "cmblensing.jl_amd", "csrc", f), encoding="utf-8").read()
        if '#include "kernels_lensop.hpp"' in src:
            assert f == "engine_lensop.hpp", f
        if '#include "engine_lensop.hpp"' in src:
            assert f in ("tu_lensop_f32.hip", "tu_lensop_f64.hip"), f


def test_load_sim_and_basedataset_take_L():
    import cmblensing_jl_amd as C
    for fn in (C.load_sim, C.BaseDataSet.__init__):
        p = inspect.signature(fn).parameters
        assert "L" in p and p["L"].default is None, fn
    assert isinstance(C.BaseDataSet.L, property) and C.BaseDataSet.L.fset is not None


def _bare(cls, **attrs):
    """an instance without a handle: what the type check of the slot looks at, no library call"""
    o = object.__new__(cls)
    o._h = None
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_a_wrong_object_in_the_slot_is_refused_before_any_library_call():
    import cmblensing_jl_amd as C

    class FakeProj:
        Ny, Nx, T = 64, 64, "float32"

    p1, p2 = FakeProj(), FakeProj()
    ds = _bare(C.BaseDataSet, proj=p1)
    ds.lib = None                                                        # any library call would raise AttributeError, not the errors below
    for bad in (3, "BilinearLens", object(), None):
        with pytest.raises(TypeError):
            ds.L = bad
    with pytest.raises(ValueError):
        ds.L = _bare(C.BilinearLens, proj=p2)                           # an operator of another projection
    with pytest.raises(TypeError):
        ds.L = lambda proj: 42                                           # a factory that makes no operator
    with pytest.raises(ValueError):
        ds.L = lambda proj: _bare(C.PowerLens, proj=p2)
    for cls in (C.LenseFlow, C.BilinearLens, C.PowerLens, C.Taylens):
        op = _bare(cls, proj=p1)
        ds.L = op
        assert ds.L is op
        ds.L = lambda proj, op=op: op                                    # a callable proj -> operator (load_sim(L = BilinearLens))
        assert ds.L is op
    # the constructor checks before it creates anything on the device
    with pytest.raises(TypeError):
        C.BaseDataSet(p1, 2, {}, L=3)
    with pytest.raises(ValueError):
        C.BaseDataSet(p1, 2, {}, L=_bare(C.BilinearLens, proj=p2))


def test_drivers_that_need_the_pullback_of_the_inverse_refuse_up_front():
    """MAP_joint, sample_joint, HMC need ∇ logpdf(Mixed(ds)), a pullback of L \\ f: src/bilinearlens.jl has a rule for L * f alone"""
    import cmblensing_jl_amd as C

    class FakeProj:
        Ny, Nx, T = 64, 64, "float32"

    p = FakeProj()
    ds = _bare(C.BaseDataSet, proj=p)
    ds.lib = None
    for cls in (C.BilinearLens, C.PowerLens, C.Taylens):
        ds.L = _bare(cls, proj=p)
        for call in (lambda: C.MAP_joint(ds), lambda: C.sample_joint(ds, 1), lambda: C.MAP_joint_step(ds, None), lambda: C.MAP_joint_step_native(ds, None),
                     lambda: C.hmc_step(ds, None, None, None, None), lambda: C.hmc_step_native(ds, None, None),
                     lambda: C.gibbs_step(ds, None, None, None, None, None), lambda: ds.gradient_logpdf_mixed(None, None)):
            with pytest.raises(NotImplementedError, match=r"pullback of `L \\ f`"):
                call()
