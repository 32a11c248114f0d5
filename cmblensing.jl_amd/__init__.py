"""MI355X-native flat-sky CMB lensing field engine (host-side mirror of the CMBLensing.jl operator surface).

The compute path is the hand-written HIP library `libcmblens_hip.so` (csrc/, C ABI in include/cmblens.h).
This package is plumbing: it loads the library with ctypes, holds device memory in torch tensors, and mirrors
the reference's names (ProjLambert, LenseFlow, BaseDataSet, argmaxf_logpdf, ...) for the path in scope.
There is NO CPU fallback: without the built library or without a GPU every compute call raises.
"""
from .lib import load_library, library_path, CmblError, build            # noqa: F401
from .engine import (ProjLambert, LenseFlow, BilinearLens, PowerLens, Taylens, IdentityLens, antilensing, BaseDataSet, Field, MAP, FOURIER, HARMONIC,   # noqa: F401
                     FLOW_FWD, FLOW_INV, FLOW_ADJ, FLOW_INVADJ, reference_exact, ud_grade, pixwin, UD_MAP, UD_FOURIER,
                     get_Cl, get_Dl, get_l4Cl, get_rhol, cov_to_Cl, make_mask)
from .equirect import (ProjEquiRect, EquiRectField, BlockDiagEquiRect, AZFOURIER, Cl_to_Beam, Cl_to_Cov, simulate, equirect_geometry,   # noqa: F401
                       blocks_from_ref, blocks_to_ref, EquiRectDataSet)
from .healpix import (ProjHealpix, HealpixField, HealpixMap, Projector, project, project_adjoint, pix2ang_ring, npix2nside)   # noqa: F401
from .sim import (Cls, load_sim, noise_from_white, noise_cls, beam_cls, lowpass, cl_to_2d, HarmOp, border_mask)   # noqa: F401
from .nolensing import NoLensingDataSet, load_nolensing_sim               # noqa: F401
from .chains import partition_chains, chain_seed, gather_chain_values, allreduce_sum   # noqa: F401
from .drivers import (quadratic_estimate, MAP_joint, MAP_joint_step, hmc_step, sample_f, gibbs_step, symplectic_integrate,   # noqa: F401
                      mass_matrix_phi, brent_minimize, sample_joint, MAP_marg, simulate_data, hmc_step_native, MAP_joint_step_native, quadratic_estimate_native)
from . import rng                                                         # noqa: F401
from .chainfile import load_chains, Chain, Chains                         # noqa: F401
from .theta import (set_theta, logpdf_mixed_theta, logpdf_mixed_theta_grid, theta_ops_device, grid_and_sample, gibbs_sample_theta, findbin, bandpower_rescale,   # noqa: F401
                    BinRescaledCov, use_bandpowers, grad_theta_logpdf, grad_theta_logpdf_mixed)
from .muse import CMBLensingMuseProblem                                   # noqa: F401
