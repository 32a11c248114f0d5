"""ctypes loader for libcmblens_hip.so and the in-tree build recipe."""
import ctypes
import os
import subprocess
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# The binding: every function include/cmblens.h declares, once.  SIGNATURES: the functions that return a status code (int), with their
# argument types; OTHER_RETURNS: (restype, argtypes) of the few that return something else.  tests/test_boundary.py checks that SYMBOLS is
# exactly what the header declares and the .so exports.
_vp, _ci, _cd, _sz, _l, _u64, _str = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t, ctypes.c_long, ctypes.c_uint64, ctypes.c_char_p
_pvp, _pci, _pd, _pl, _pu64 = (ctypes.POINTER(t) for t in (_vp, _ci, _cd, _l, _u64))
OTHER_RETURNS = {
    "cmbl_last_error": (_str, []),
    "cmbl_version": (_ci, []),
    "cmbl_abi_version": (_ci, []),
    "cmbl_prof_count": (_ci, []),
    "cmbl_prof_name": (_str, [_ci]),
}
SIGNATURES = {
    "cmbl_ctx_create": [_ci, _ci, _cd, _ci, _ci, _vp, _pvp],
    "cmbl_ctx_destroy": [_vp],
    "cmbl_ctx_set_option": [_vp, _str, _ci],
    "cmbl_ctx_get_option": [_vp, _str, _pci],
    "cmbl_ctx_synchronize": [_vp],
    "cmbl_ctx_geometry_host": [_vp, _ci, _pd, _sz],
    "cmbl_prof_enable": [_vp, _ci],
    "cmbl_prof_reset": [_vp],
    "cmbl_prof_get": [_vp, _ci, _pd, _pl],
    "cmbl_rfft": [_vp, _vp, _vp, _ci, _ci],
    "cmbl_irfft": [_vp, _vp, _vp, _ci, _ci],
    "cmbl_convert": [_vp, _ci, _vp, _ci, _vp, _ci, _ci],
    "cmbl_diag_apply": [_vp, _ci, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _ci],
    "cmbl_blockdiag_ieb_apply": [_vp, _vp, _ci, _ci, _vp, _ci, _vp, _ci],
    "cmbl_dot": [_vp, _ci, _vp, _vp, _ci, _ci, _pd],
    "cmbl_logdet": [_vp, _vp, _ci, _pd],
    "cmbl_lenseflow_create": [_vp, _ci, _pvp],
    "cmbl_lenseflow_destroy": [_vp],
    "cmbl_lenseflow_set_phi": [_vp, _ci, _vp, _ci],
    "cmbl_lenseflow_apply": [_vp, _ci, _ci, _vp, _ci, _vp, _ci, _ci],
    "cmbl_lenseflow_grad": [_vp, _ci, _vp, _ci, _vp, _vp, _ci, _vp, _vp, _ci, _ci, _ci],
    "cmbl_max_lensing_step": [_vp, _ci, _vp, _vp, _ci, _pd],
    "cmbl_axpby": [_vp, _ci, _pd, _vp, _pd, _vp, _vp, _ci, _ci],
    "cmbl_qe_leg": [_vp, _vp, _ci, _ci, _ci, _vp, _ci],
    "cmbl_fourier_lmul": [_vp, _vp, _ci, _ci, _ci, _vp, _ci],
    "cmbl_map_fma": [_vp, _vp, _vp, _cd, _vp, _ci, _ci],
    "cmbl_randn": [_vp, _pu64, _ci, _u64, _vp, _l],
    "cmbl_dataset_create": [_vp, _ci, _pvp],
    "cmbl_dataset_destroy": [_vp],
    "cmbl_dataset_set_op": [_vp, _ci, _vp, _ci],
    "cmbl_dataset_noise_inv": [_vp, _vp, _vp, _ci],
    "cmbl_dataset_set_data": [_vp, _vp, _ci],
    "cmbl_dataset_set_logdet": [_vp, _cd],
    "cmbl_gradientf_logpdf": [_vp, _vp, _vp, _vp, _ci, _vp, _ci],
    "cmbl_wiener_cg": [_vp, _vp, _vp, _vp, _cd, _ci, _vp, _pd, _pci, _ci],
    "cmbl_lensop_from_lenseflow": [_vp, _pvp],
    "cmbl_lensop_from_bilinear": [_vp, _pvp],
    "cmbl_lensop_from_powerlens": [_vp, _pvp],
    "cmbl_lensop_identity": [_vp, _pvp],
    "cmbl_lensop_destroy": [_vp],
    "cmbl_gradientf_logpdf_op": [_vp, _vp, _vp, _vp, _ci, _vp, _ci],
    "cmbl_wiener_cg_op": [_vp, _vp, _vp, _vp, _cd, _ci, _vp, _pd, _pci, _ci],
    "cmbl_grad_logpdf_op": [_vp, _vp, _vp, _vp, _vp, _pd, _vp, _vp, _ci, _ci],
    "cmbl_nolensing_logpdf": [_vp, _vp, _vp, _pd, _vp, _ci],
    "cmbl_logpdf_mixed": [_vp, _vp, _vp, _vp, _pd, _ci],
    "cmbl_grad_logpdf_mixed": [_vp, _vp, _vp, _vp, _pd, _vp, _vp, _ci, _ci],
    "cmbl_dataset_theta_model": [_vp, _pd, _ci, _pd, _ci, _pci, _vp, _pci, _pd, _pd, _cd, _cd, _pd, _cd, _pd, _pd, _cd],
    "cmbl_logpdf_mixed_theta": [_vp, _vp, _vp, _vp, _ci, _ci, _pd, _pd, _pd, _ci, _pd],
    "cmbl_dataset_theta_ops": [_vp, _cd, _cd, _pd, _ci, _ci, _vp, _pd],
    "cmbl_grad_theta_logpdf": [_vp, _vp, _vp, _ci, _cd, _cd, _pd, _ci, _ci, _pd],
    "cmbl_grad_theta_logpdf_mixed": [_vp, _vp, _vp, _vp, _ci, _cd, _cd, _pd, _ci, _ci, _pd, _pd],
    "cmbl_hmc_step": [_vp, _vp, _vp, _vp, _vp, _vp, _pd, _pu64, _u64, _ci, _cd, _ci, _ci, _ci, _vp, _pd, _pci],
    "cmbl_quadratic_estimate": [_vp, _ci, _pd, _pd, _pd, _pd, _pd, _ci, _pd, _vp, _pd, _ci],
    "cmbl_map_joint_step": [_vp, _vp, _vp, _vp, _vp, _cd, _cd, _cd, _ci, _ci, _ci, _vp, _vp, _pd, _pd, _pci, _pci],
    "cmbl_norm": [_vp, _ci, _vp, _ci, _ci, _pd],
    "cmbl_logdet_diag": [_vp, _ci, _vp, _ci, _ci, _pd],
    "cmbl_tr_diag": [_vp, _ci, _vp, _ci, _ci, _pd],
    "cmbl_set_sum_accuracy_mode": [_vp, _ci],
    "cmbl_timer_report": [_vp, _str, _sz],
    "cmbl_device_malloc": [_vp, _sz, _pvp],
    "cmbl_device_free": [_vp, _vp],
    "cmbl_copy_to_device": [_vp, _vp, _vp, _sz],
    "cmbl_copy_to_host": [_vp, _vp, _vp, _sz],
    "cmbl_ud_grade": [_vp, _vp, _ci, _ci, _ci, _ci, _vp, _ci, _vp, _ci, _ci],
    "cmbl_pixwin_host": [_vp, _pd, _sz],
    "cmbl_clbins_create": [_vp, _pd, _ci, _pd, _sz, _pvp],
    "cmbl_clbins_destroy": [_vp],
    "cmbl_clbins_info_host": [_vp, _ci, _pd, _sz],
    "cmbl_get_cl": [_vp, _vp, _ci, _vp, _vp, _ci, _ci, _pci, _ci, _ci, _vp],
    "cmbl_bilinear_create": [_vp, _pvp],
    "cmbl_bilinear_destroy": [_vp],
    "cmbl_bilinear_set_phi": [_vp, _ci, _vp, _ci],
    "cmbl_bilinear_set_deflection": [_vp, _vp, _vp],
    "cmbl_bilinear_apply": [_vp, _ci, _ci, _vp, _ci, _vp, _ci, _ci, _ci],
    "cmbl_bilinear_grad": [_vp, _vp, _ci, _vp, _vp, _ci, _vp, _ci, _ci],
    "cmbl_powerlens_create": [_vp, _ci, _ci, _pvp],
    "cmbl_powerlens_destroy": [_vp],
    "cmbl_powerlens_set_phi": [_vp, _ci, _vp, _ci],
    "cmbl_powerlens_set_deflection": [_vp, _vp, _vp],
    "cmbl_powerlens_apply": [_vp, _ci, _ci, _vp, _ci, _vp, _ci, _ci],
    "cmbl_edt_sq": [_vp, _vp, _vp],
    "cmbl_make_mask": [_vp, _pci, _ci, _ci, _ci, _ci, _ci, _vp],
    "cmbl_equirect_geometry_host": [_ci, _ci, _pd, _pd, _pd, _pd, _pd, _pd, _pd, _pd],
    "cmbl_equirect_convert": [_vp, _ci, _vp, _ci, _vp, _ci, _ci],
    "cmbl_equirect_block_apply": [_vp, _vp, _ci, _ci, _ci, _vp, _vp, _ci],
    "cmbl_equirect_block_matmul": [_vp, _vp, _ci, _vp, _ci, _ci, _ci, _vp],
    "cmbl_equirect_block_dot": [_vp, _vp, _vp, _ci, _ci, _pd],
    "cmbl_equirect_block_scale_columns": [_vp, _vp, _ci, _ci, _pd, _ci],
    "cmbl_equirect_beam_pol": [_vp, _vp, _pd, _vp],
    "cmbl_equirect_block_svd": [_vp, _vp, _ci, _ci, _cd, _vp, _vp, _pd, _pci],
    "cmbl_equirect_block_logabsdet": [_vp, _vp, _ci, _ci, _pd],
    "cmbl_equirect_block_solve": [_vp, _vp, _ci, _ci, _ci, _vp, _ci, _ci, _vp, _ci],
    "cmbl_equirect_cov": [_vp, _pd, _pd, _ci, _ci, _pd, _pd, _ci, _vp],
    "cmbl_eqds_create": [_vp, _ci, _pvp],
    "cmbl_eqds_destroy": [_vp],
    "cmbl_eqds_set_block_op": [_vp, _ci, _vp, _ci, _ci],
    "cmbl_eqds_set_pixel_op": [_vp, _ci, _vp, _ci],
    "cmbl_eqds_set_logdet": [_vp, _cd],
    "cmbl_eqds_mean": [_vp, _vp, _vp, _ci],
    "cmbl_eqds_gradientf_logpdf": [_vp, _vp, _vp, _vp, _ci],
    "cmbl_eqds_logpdf": [_vp, _vp, _vp, _pd, _ci],
    "cmbl_eqds_wiener_cg": [_vp, _vp, _vp, _cd, _ci, _vp, _pd, _pci, _ci],
    "cmbl_equirect_field_dot": [_vp, _ci, _vp, _vp, _ci, _ci, _pd],
    "cmbl_healpix_pix2ang_host": [_ci, _l, _l, _pd, _pd],
    "cmbl_projector_create": [_vp, _ci, _ci, _pd, _pvp],
    "cmbl_projector_create_method": [_vp, _ci, _ci, _pd, _ci, _pvp],
    "cmbl_projector_destroy": [_vp],
    "cmbl_projector_method": [_vp, _pci, _pci],
    "cmbl_projector_info_host": [_vp, _ci, _pd, _sz],
    "cmbl_project_to_cart": [_vp, _vp, _vp, _ci, _ci],
    "cmbl_project_to_healpix": [_vp, _ci, _vp, _vp, _ci, _ci],
    "cmbl_project_to_cart_adjoint": [_vp, _vp, _vp, _ci, _ci],
    "cmbl_project_to_healpix_adjoint": [_vp, _vp, _vp, _ci, _ci],
}
SYMBOLS = list(OTHER_RETURNS) + list(SIGNATURES)


ABI_VERSION = 3          # CMBL_ABI_VERSION of include/cmblens.h this binding was written against


class CmblError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libcmblens_hip error {code}: {msg}")
        self.code = code


def library_path():
    """In-tree library; CMBL_LIB points at an alternative build of the same sources (tile-shape experiments)."""
    return os.environ.get("CMBL_LIB") or os.path.join(_HERE, "libcmblens_hip.so")


# translation units of the library (csrc/api_decl.hpp has the map): the entry points, and per precision the typed bodies with the
# power-of-two kernels, the any-size transform launches and (tu_cty / tu_ctx, two halves of the list of lengths) their compile-time-plan kernels.
# One object each, then linked.
# (longest first: the build is a pool of as many compilers as the host has cores)
UNITS = ["tu_cty_f32_b", "tu_cty_f64_b", "tu_ctx_f32_b", "tu_ctx_f64_b", "tu_cty_f32_a", "tu_cty_f64_a", "tu_main_f32", "tu_main_f64",
         "tu_ctx_f32_a", "tu_ctx_f64_a", "tu_small_f32", "tu_small_f64", "tu_gen_f32", "tu_gen_f64", "tu_lensop_f32", "tu_lensop_f64", "api"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]


def build(force=False, verbose=False, jobs=None, extra_flags=(), out=None, objdir=None):
    """hipcc cross-compiles for gfx950 without a GPU.  In-tree output: cmblensing.jl_amd/libcmblens_hip.so

    One object per translation unit under build/obj (git-ignored), compiled `jobs` at a time (default: one per core, the longest units first), re-compiled only when a source it includes (-MMD dependency file) or the flags changed.  `extra_flags`
    / `out` / `objdir`: variant builds of the same sources (tools/devbuild.py)."""
    csrc = os.path.join(_HERE, "csrc")
    out = out or library_path()
    objdir = objdir or os.path.join(_HERE, "..", "build", "obj")
    os.makedirs(objdir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = HIPCC_FLAGS + list(extra_flags)
    stamp = " ".join([hipcc] + flags)

    def stale(unit):
        obj, dep, flg = (os.path.join(objdir, unit + e) for e in (".o", ".d", ".flags"))
        if force or not (os.path.exists(obj) and os.path.exists(dep) and os.path.exists(flg)) or open(flg).read() != stamp:
            return True
        deps = open(dep).read().replace("\\\n", " ").split(":", 1)[1].split()
        t = os.path.getmtime(obj)
        return any((not os.path.exists(d)) or os.path.getmtime(d) > t for d in deps)

    todo = [u for u in UNITS if stale(u)]
    procs, failed = [], []
    jobs = jobs or int(os.environ.get("CMBL_BUILD_JOBS", "0")) or min(len(UNITS), os.cpu_count() or 8)

    def reap(block):
        """collect the compilers that have finished; block: wait until at least one has"""
        while True:
            done = [item for item in procs if item[1].poll() is not None]
            for unit, p, log in done:
                log.close()
                procs.remove((unit, p, log))
                if p.returncode != 0:
                    failed.append(unit)
                else:
                    open(os.path.join(objdir, unit + ".flags"), "w").write(stamp)
            if done or not block or not procs:
                return
            time.sleep(0.2)

    for unit in todo:
        while len(procs) >= jobs:
            reap(True)
        obj = os.path.join(objdir, unit + ".o")
        cmd = [hipcc] + flags + ["-MMD", "-MF", os.path.join(objdir, unit + ".d"), "-c", os.path.join(csrc, unit + ".hip"), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        for e in (".flags",):
            if os.path.exists(os.path.join(objdir, unit + e)):
                os.remove(os.path.join(objdir, unit + e))
        log = open(os.path.join(objdir, unit + ".log"), "w")
        procs.append((unit, subprocess.Popen(cmd, stdout=log, stderr=subprocess.STDOUT), log))
    while procs:
        reap(True)
    if failed:
        msgs = "".join(f"\n--- {u} ---\n" + open(os.path.join(objdir, u + ".log")).read()[-4000:] for u in failed)
        raise RuntimeError("hipcc failed for " + ", ".join(failed) + msgs)
    objs = [os.path.join(objdir, u + ".o") for u in UNITS]
    if todo or not os.path.exists(out) or any(os.path.getmtime(o) > os.path.getmtime(out) for o in objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return out


def load_library():
    """Load the HIP library; fails loudly when it has not been built (no fallback path exists)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in list(OTHER_RETURNS.items()) + [(n, (_ci, a)) for n, a in SIGNATURES.items()]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.cmbl_abi_version() != ABI_VERSION:
        raise ImportError(f"{path}: ABI version {lib.cmbl_abi_version()} but this package binds version {ABI_VERSION} (include/cmblens.h): rebuild")
    _LIB = lib
    return lib


def check(code):
    if code != 0:
        raise CmblError(code, load_library().cmbl_last_error().decode("utf-8", "replace"))
