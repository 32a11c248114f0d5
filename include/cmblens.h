/* libcmblens_hip.so -- C ABI of the MI355X-native flat-sky lensing field engine.
 *
 * Drop-in boundary for the LenseFlow / Wiener-filter hot path of marius311/CMBLensing.jl
 * (reference @ v0.10.1; citations are `file:line` under /root/reference).  The reference has no
 * FFI for this path -- its "plugin" surface is the array storage type `A` of `BaseField{B,M,T,A}`
 * (src/base_fields.jl:14) plus the operator slot `ds.L` (src/dataset.jl:55).  Each entry point
 * below replaces the reference method(s) it cites; INTEGRATION.md shows the Julia `ccall` glue.
 *
 * Conventions
 *   - every function returns 0 (CMBL_OK) or a CMBL_ERR_* code; cmbl_last_error() gives the text
 *     (thread-local).  Nothing throws across the ABI.
 *   - all field pointers are DEVICE pointers (HIP) unless the name ends in `_host`.
 *   - array layouts are the reference's (src/proj_cartesian.jl:13-36, column-major, Ny fastest):
 *       map     : real    (Ny, Nx, npol, nbatch)
 *       fourier : complex (Ny/2+1, Nx, npol, nbatch)   interleaved (re,im)
 *     npol = 1 (I), 2 (QU), 3 (IQU).  Operators diagonal in l are real (Ny/2+1, Nx) planes.
 *   - dtype: CMBL_F32 or CMBL_F64 (the whole context works in one precision).
 *   - Ny, Nx: any integers in [2, 4096], like the reference's FFTW plans (src/util_fft.jl:32-35).  Powers of two >= 32 on both
 *     sides run the fused kernels; other sizes the any-size path (mixed-radix / chirp-z transforms, csrc/kernels_generic.hpp),
 *     same results, ~5x slower per pixel.  Sides above 4096 return CMBL_ERR_SHAPE.
 *   - nbatch (chains / simulations as batch slots of one call): up to 256 per call for the entry points that return per-slot scalars
 *     (reductions, cmbl_wiener_cg, cmbl_logpdf_mixed, cmbl_grad_logpdf_mixed); more return CMBL_ERR_ARG.  The flows have no such limit.
 *   - a handle is used by one host thread at a time; different contexts are independent.
 *   - calls are asynchronous on the context's stream unless they return host values (`*_host` outputs), i.e. every
 *     field-to-field entry point is already the `_async` form; cmbl_ctx_synchronize() waits for the stream.
 */
#ifndef CMBLENS_H
#define CMBLENS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cmbl_ctx cmbl_ctx;
typedef struct cmbl_flow cmbl_flow;
typedef struct cmbl_dataset cmbl_dataset;
typedef struct cmbl_clbins cmbl_clbins;
typedef struct cmbl_bilinear cmbl_bilinear;
typedef struct cmbl_powerlens cmbl_powerlens;
typedef struct cmbl_lensop cmbl_lensop;

enum { CMBL_OK = 0, CMBL_ERR_ARG = 1, CMBL_ERR_SHAPE = 2, CMBL_ERR_HIP = 3, CMBL_ERR_NAN = 4,
       CMBL_ERR_STATE = 5, CMBL_ERR_ALLOC = 6 };
enum { CMBL_F32 = 0, CMBL_F64 = 1 };

/* bases (src/generic.jl:42-98): MAP = Map/QUMap/IQUMap (LenseBasis), FOURIER = Fourier/QUFourier/
 * IQUFourier (DerivBasis), HARMONIC = Fourier/EBFourier/IEBFourier (basis covariances are diagonal in).
 * AZFOURIER = AzFourier/QUAzFourier of ProjEquiRect (src/proj_equirect.jl:149-178): accepted by cmbl_equirect_convert only */
enum { CMBL_MAP = 0, CMBL_FOURIER = 1, CMBL_HARMONIC = 2, CMBL_AZFOURIER = 3 };

/* LenseFlow operator modes (src/flowops.jl:11-14) */
enum { CMBL_FLOW_FWD = 0,     /* L * f   : velocity,  t 0->1 */
       CMBL_FLOW_INV = 1,     /* L \ f   : velocity,  t 1->0 */
       CMBL_FLOW_ADJ = 2,     /* L' * f  : velocityH, t 1->0 */
       CMBL_FLOW_INVADJ = 3   /* L' \ f  : velocityH, t 0->1 */ };

/* diagonal operator application kinds (src/specialops.jl:9-10) */
enum { CMBL_DIAG_MUL = 1, CMBL_DIAG_DIV_NAN2ZERO = 3 };

/* ABI revision of this header.  Bumped whenever an existing entry point changes its signature or meaning (additions do not bump
 * it): 2 = cmbl_device_malloc / cmbl_device_free take the context (round 3); 3 = behaviour switches are read from the environment
 * once per context and changed through cmbl_ctx_set_option (round 4).  A caller compiled against this header checks
 * cmbl_abi_version() == CMBL_ABI_VERSION before anything else (julia/CMBLensingHIPExt.jl __init__, tests/c_abi/ *.c). */
#define CMBL_ABI_VERSION 3

const char* cmbl_last_error(void);
int cmbl_version(void);          /* library release, 100 * major + minor */
int cmbl_abi_version(void);      /* the CMBL_ABI_VERSION the library was built with */

/* ---- context: replaces the memoized ProjLambert + FFT plans
 *      (src/proj_lambert.jl:48-75, src/util_fft.jl:32-39).  `stream` is a hipStream_t the caller owns
 *      (e.g. torch's current stream); NULL is the legacy default stream. */
int cmbl_ctx_create(int Ny, int Nx, double theta_pix_arcmin, int dtype, int device, void* stream, cmbl_ctx** out);
int cmbl_ctx_destroy(cmbl_ctx* ctx);
int cmbl_ctx_synchronize(cmbl_ctx* ctx);
/* geometry queries, host output, double: which = 0 lx[Nx], 1 ly[Ny/2+1], 2 lambda_rfft[Ny/2+1],
 * 3 sin2phi[(Ny/2+1)*Nx], 4 cos2phi[...], 5 lmag[...]  (planes in the reference layout) */
int cmbl_ctx_geometry_host(cmbl_ctx* ctx, int which, double* out_host, size_t n);

/* ---- behaviour switches of a context (A/B and profiling aids; none changes results beyond rounding).  Each starts from the
 *      environment variable named below, read ONCE when the context is created, and afterwards changes only through this call:
 *        "slice_streams"         CMBL_SLICE_STREAMS (4)            launch chains per flow: pol slices / batch-slot groups on their own streams; 1 = one launch over all slices
 *        "slice_streams_min_pix" CMBL_SLICE_STREAMS_MIN_PIX (2^19) pixels a launch chain of a delta flow must carry (all its slices together); map and adjoint flows, and three or more chains: twice that
 *        "pcache"                !CMBL_NO_PCACHE (1)               cache p(t_k) at the 2n+1 stage times per phi (src/lenseflow.jl:45-46,131-142); read by cmbl_lenseflow_set_phi
 *        "pcache_max_mb"         CMBL_PCACHE_MAX_MB (16384)
 *        "fused_harm"            !CMBL_NO_FUSED_HARM (1)           harmonic-space operator chains inside one row pass
 *        "gen_separable", "gen_prologue", "gen_xderiv_fused"       any-size path stage fusions (CMBL_GEN_SEPARABLE / _PROLOGUE / _XDERIV_FUSED, all 1)
 *                                                                   (these, gen_yy, gen_xmerge and gen_tiled are read in ONE place, once per flow: Ctx::gen_form in
 *                                                                   csrc/engine.hpp turns them and the two side lengths into the stage form every launch of the flow follows)
 *        "gen_ct"                                                   any-size path: compile-time-plan transforms for the lengths 2^a 3^b 5^c of
 *                                                                   CMBL_CT_LIST (CMBL_GEN_CT, 1; 0 = the run-time-planned kernel for every length)
 *        "gen_ct_rows"                                              any-size path: x-pass launches with fewer row groups than CUs take groups of 4 / 2 rows instead
 *                                                                   of 8 (CMBL_GEN_CT_ROWS, 1; results bit-identical either way)
 *        "gen_ct_cols"                                              any-size flows: half-width column groups (4 instead of 8 columns in single precision) in the fused y
 *                                                                   launches: 0 never, 1 (default) always on tiled hand-off arrays (gen_tiled) in single precision and
 *                                                                   otherwise for launches below 0.4 workgroups per CU, 2 always; gen_ct_rows = 0 switches it off too
 *                                                                   (CMBL_GEN_CT_COLS; results bit-identical)
 *        "gen_xmerge"                                               any-size flows: the row update that closes an adjoint-type stage also runs the x passes that open the
 *                                                                   next stage (CMBL_GEN_XMERGE, 1: 2 instead of 3 launches per stage; results bit-identical either way)
 *        "gen_tiled"                                                any-size flows (both axes with a compile-time plan): the half planes the fused stages hand between their
 *                                                                   column and row launches are stored as [x/4][ky][x%4] blocks instead of [ky][x]; bit mask 1 = map flows,
 *                                                                   2 = adjoint flows, 4 = delta flows, 8 = the scratch of the 2-D basis transforms (CMBL_GEN_TILED, 7: bit 8 measured neutral; results bit-identical to 0)
 *        "gen_yy"                                                   any-size flows: the passes of a stage that can share a launch do, where the axes have
 *                                                                   compile-time plans (CMBL_GEN_YY, 1; results bit-identical either way)
 *        "gen_slice_streams", "gen_streams_min_pix"                 any-size flows: launch chains over groups of slices when every chain carries at least this many
 *                                                                   4-byte pixels, a third more from three chains on (CMBL_GEN_SLICE_STREAMS 1, CMBL_GEN_STREAMS_MIN_PIX 300000)
 *        "occupancy_tiles"       CMBL_OCCUPANCY_TILES (3)          small maps: bit 0 = two-column tiles when four-column tiles leave CUs idle or unevenly loaded, bit 1 = shorter row groups
 *        "fill_target"           CMBL_FILL_TARGET (0)              > 0: narrow the column tiles below that many tiles per launch instead of the built-in rule
 *        "row_fill_target"       CMBL_ROW_FILL_TARGET (0 = CUs/2)  shorten the row groups below that many groups per launch
 *        "col_prefetch"          CMBL_COL_PREFETCH (-1)            touch prefetch of the double-precision >= 2048-row column kernels: -1 = built-in distance, 0 = off, > 0 = blocks ahead
 *        "small_flow"            CMBL_SMALL_FLOW (1)               maps of 32..128 pixels per side: L*f, L\f, L'g, L'\g as ONE launch, one workgroup per (pol, batch) slice with
 *                                                                   the half plane resident in LDS (csrc/kernels_small.hpp): 0 = off, 1 = up to 64 x 64 pixels (faster at every
 *                                                                   batch size), 2 = wherever compiled (up to 128 x 128 in single, 64 x 64 in double precision).  Results agree
 *                                                                   with the staged path to rounding, not bit for bit (tests/test_gpu_small.py)
 *        "lens_fused"            CMBL_LENS_FUSED (0)               a BilinearLens in the L slot of a data set (cmbl_*_op), power-of-two maps: 1 = the bilinear gather and the row sum
 *                                                                   of the transpose run inside the column pass of the transform behind them (csrc/kernels_lensop.hpp), one launch
 *                                                                   instead of gather, map, y_r2c; 0 = the composition from the stand-alone launches.  Other sizes always take the
 *                                                                   composition.  The two agree to rounding (tests/test_gpu_lensop_dataset.py).
 *                                                                   Default 0 at every size: measured on MI355X, the Wiener-filter CG iteration with 0 / with 1 takes 0.215 / 0.227 ms at 1024^2 QU fp32 B = 1,
 *                                                                   0.934 / 1.063 ms at B = 8, 1.186 / 1.417 ms at 2048^2 QU fp64 B = 1, 8.367 / 10.320 ms at B = 8 (profiles/lensop_wf_times.txt):
 *                                                                   the fused pass is slower everywhere and stays an option.
 *        "eq_cov_scratch_mb"     CMBL_EQ_COV_SCRATCH_MB (256)      cmbl_equirect_cov: cap in MiB of the scratch of one slab of ring pairs (at least one pair per slab);
 *                                                                   changes no result (tests/test_gpu_equirect_cov.py)
 *        "eq_factor_scratch_mb"  CMBL_EQ_FACTOR_SCRATCH_MB (8192)  cmbl_equirect_block_svd / _logabsdet / _solve: cap in MiB of the double working copies of one slab of
 *                                                                   blocks (at least one block per slab); changes no result (tests/test_gpu_equirect_factor.py)
 *      (the launch-geometry and prefetch switches change no result at all: tests/test_gpu_boundary.py, tests/test_gpu_fullsize.py)
 *      Unknown names return CMBL_ERR_ARG.  The reference has no counterpart (its switches are Julia keyword arguments). */
int cmbl_ctx_set_option(cmbl_ctx* ctx, const char* name, int value);
int cmbl_ctx_get_option(cmbl_ctx* ctx, const char* name, int* value_host);

/* ---- optional per-launch timing of the library's kernel classes with HIP events on the context's stream
 *      (the reference wraps the same call sites in TimerOutputs `@⌛`, src/util.jl:351-390).  Disabled by default. */
int cmbl_prof_enable(cmbl_ctx* ctx, int on);
int cmbl_prof_reset(cmbl_ctx* ctx);
int cmbl_prof_count(void);
const char* cmbl_prof_name(int kernel_class);
int cmbl_prof_get(cmbl_ctx* ctx, int kernel_class, double* total_ms_host, long* launches_host);

/* report of the accumulated timings as text ("name launches total_ms mean_us" lines), like TimerOutputs' table; returns the
 * number of bytes the full report needs (excluding the terminator) -- call with buf = NULL to size the buffer. */
int cmbl_timer_report(cmbl_ctx* ctx, char* buf, size_t buflen);

/* ---- device memory helpers for callers that do not link HIP themselves (a Julia process without AMDGPU.jl, the plain-C
 *      test): every field pointer of this API is a device pointer; these give a host program the means to own some.
 *      Buffers live on the context's device (the call selects it: the caller cannot, it does not link HIP).
 *      Copies are ordered on the context's stream and complete on return. */
int cmbl_device_malloc(cmbl_ctx* ctx, size_t bytes, void** out);
int cmbl_device_free(cmbl_ctx* ctx, void* p);
int cmbl_copy_to_device(cmbl_ctx* ctx, void* dst_device, const void* src_host, size_t bytes);
int cmbl_copy_to_host(cmbl_ctx* ctx, void* dst_host, const void* src_device, size_t bytes);

/* ---- basis transforms: m_rfft / m_irfft and the Basis conversion lattice
 *      (src/util_fft.jl:20-31, src/proj_lambert.jl:245-300) */
int cmbl_rfft(cmbl_ctx* ctx, const void* map, void* fourier, int npol, int nbatch);
int cmbl_irfft(cmbl_ctx* ctx, const void* fourier, void* map, int npol, int nbatch);
int cmbl_convert(cmbl_ctx* ctx, int basis_in, const void* in, int basis_out, void* out, int npol, int nbatch);

/* ---- ud_grade(f, θnew; mode, deconv_pixwin, anti_aliasing) (src/proj_lambert.jl:533-592): the field `in` on the grid of `src` is brought to the
 *      grid of `dst`.  The only entry point with two contexts: they must share dtype, device and stream (else CMBL_ERR_ARG); the work is
 *      ordered on that stream like every other entry point; `in` and `out` must not alias.
 *      Geometry: an integer fac >= 2 with src.N = fac * dst.N on both axes and theta_dst = fac * theta_src (relative 1e-6) is a downgrade, the
 *      mirror image an upgrade, anything else CMBL_ERR_SHAPE ("Can only ud_grade in integer steps", :546).  Equal geometry (`θnew == θ &&
 *      return f`, :542) is a copy, or the plain basis conversion asked for.
 *      Bases: every step acts on each (pol, batch) plane separately, pol components are never mixed.  basis_in / basis_out: CMBL_MAP or a complex
 *      basis, independently; CMBL_HARMONIC only on both sides at once and only in Fourier mode (the planes are then treated like FOURIER planes,
 *      what the reference does with EB fields in :fourier mode); any other mix with CMBL_HARMONIC is CMBL_ERR_ARG -- the engine has no EB-map basis.
 *      A complex input is taken to be the transform of real maps, as every reference Field is: where the reference goes through Map(f), the
 *      imaginary parts a c2r transform would drop (ky = 0 and Nyquist after the x pass) are NOT dropped by the paths that stay in Fourier space.
 *      Semantics -- the reference's, quirks included:
 *        downgrade, CMBL_UD_MAP:      [anti_aliasing] -> mean over fac x fac pixel blocks (:561) -> [deconv_pixwin: divide by
 *                                     PWF = pixwin(θnew) / pixwin(θ) on the new grid, nan2zero (:552, 571)]
 *        downgrade, CMBL_UD_FOURIER:  [anti_aliasing] -> keep rows ky = 0 ... Ny_new/2 and columns kx = 0 ... ceil(Nx_new/2) - 1, -floor(Nx_new/2) ... -1
 *                                     of the half plane (:566) -> [divide by PWF].  NOT rescaled by 1/fac^2 although the transforms are unnormalised
 *                                     (src/util_fft.jl:20-25): the map of the result is fac^2 times too large, as in the reference
 *        upgrade, CMBL_UD_MAP:        every pixel replicated fac x fac (:575-580); anti_aliasing is ignored; deconv_pixwin is CMBL_ERR_ARG
 *                                     ("Not implemented", :582)
 *        upgrade, CMBL_UD_FOURIER:    CMBL_ERR_ARG ("Not implemented", :585)
 *        anti_aliasing:               zeroes every coefficient of the input with |ly| >= nyquist_new or |lx| >= nyquist_new (:557), decided by INTEGER
 *                                     index: 2 |ky| >= Ny_new or 2 |kx| >= Nx_new (the reference compares rounded floats that are equal at the boundary)
 *      With anti_aliasing the map-mode block mean is applied as a Fourier-space multiply (no aliased term survives): one transform at the source
 *      size (none for complex input) and one at the new size only for a MAP output; equal to the reference's three-transform sequence up to rounding. */
enum { CMBL_UD_MAP = 0, CMBL_UD_FOURIER = 1 };
int cmbl_ud_grade(cmbl_ctx* src, cmbl_ctx* dst, int mode, int deconv_pixwin, int anti_aliasing,
                  int basis_in, const void* in, int basis_out, void* out, int npol, int nbatch);
/* pixwin(θpix, ℓ) (src/proj_lambert.jl:200) on the context's half plane: sinc(ly Δx / 2π) * sinc(lx Δx / 2π) = sinc(ky / Ny) * sinc(kx / Nx),
 * real (Ny/2+1, Nx) plane in the reference layout, host, double; n = (Ny/2+1) * Nx. */
int cmbl_pixwin_host(cmbl_ctx* ctx, double* out_host, size_t n);

/* ---- get_Cℓ(f1, f2 = f1; Δℓ, ℓedges, Cℓfid, err_estimate) (src/proj_lambert.jl:470-513; get_Dℓ, get_ℓ⁴Cℓ, get_ρℓ of src/cls.jl:85-97 and cov_to_Cℓ,
 *      :415-419, are host arithmetic on its result): binned auto- and cross-power spectra on the device.  Per mode of the FULL plane the reference forms
 *      ℓ = ℓmag, CL = Re(conj(f1) f2) / α with α = Nx Ny / Δx², and w = nan2zero((2 Cℓfid(ℓ)² / (2ℓ+1))⁻¹); keeps the modes with
 *      min(ℓedges) < ℓ < max(ℓedges) (BOTH strict, :476); histograms them into the left-closed bins [e_i, e_i+1) and returns, per bin,
 *      ℓ = Sℓ / A and Cℓ = S1 / A with A = Σ w, Sℓ = Σ w ℓ, S1 = Σ w CL and, for err_estimate, N = (Σ 1) / 2 and S2 = Σ w CL².
 *      ℓ and CL are equal at a mode and at its Hermitian mirror, so each sum is the HALF-plane sum weighted by λ (1 on ky = 0 and on the Nyquist row of an
 *      even Ny, 2 elsewhere; `unfold`, src/util_fft.jl:83-97, which for odd Nx indexes one past the row -- the mirror it intends is what is computed).
 *      A, Sℓ and the counts depend on the grid, the edges and the weight only: they are made ONCE with the binning plan, on the host, in double.
 *   cmbl_clbins_create: `ledges_host`: nedges doubles, 2 <= nedges <= 65536, finite and strictly increasing (else CMBL_ERR_ARG).  `w_host`: the per-mode
 *      weight w on the half plane, real (Ny/2+1, Nx) plane in the reference layout, nw = (Ny/2+1) * Nx finite doubles (another nw: CMBL_ERR_SHAPE; a
 *      non-finite value: CMBL_ERR_ARG), or NULL (nw ignored) for Cℓfid = 1, w = (2ℓ+1)/2.  Bin membership is decided here, in double, by comparing the
 *      numbers cmbl_ctx_geometry_host(which = 5) returns with the edges -- the reference compares a working-precision ℓmag, which in single precision
 *      moves a few modes per megapixel across an edge.  The plan belongs to the geometry of `ctx`: used with a context of another size, pixel size or
 *      layout it returns CMBL_ERR_SHAPE, of another precision or device CMBL_ERR_ARG.  It may outlive the context.
 *   cmbl_clbins_info_host: per bin (n = nedges - 1, else CMBL_ERR_SHAPE) A, Sℓ, or the number of full-plane modes Σ λ (N is half of it).
 *   cmbl_get_cl: `f1`, `f2` (NULL: f2 = f1): device fields of npol planes per batch slot in `basis`, ABI layouts.  CMBL_MAP fields are transformed into the
 *      context's scratch first; complex fields are read where they lie, and CMBL_FOURIER / CMBL_HARMONIC only say what the planes mean to the caller.
 *      `pairs_host`: npairs (1 ... 9, else CMBL_ERR_ARG) index pairs (a, b) into the npol planes OF THAT BASIS: plane a of f1 against plane b of f2 (an
 *      index outside [0, npol): CMBL_ERR_ARG).  `moments`: 1 (S1) or 2 (S1 and S2), else CMBL_ERR_ARG.  nbatch <= 256.
 *      `out`: DEVICE doubles [nbatch][npairs][moments][nedges - 1], S1 = Σ λ w CL and S2 = Σ λ w CL², written asynchronously on the context's stream
 *      (empty bins hold 0; the caller divides by A).  All pairs come out of one pass over the fields.  Accumulation is in double in either precision and
 *      deterministic (fixed summation order, no atomics): equal calls give bit-identical output, and a batch slot's numbers do not depend on the others.
 *      err_estimate: the reference's line :498 forms S2/A − S1² with the un-normalised S1 (negative for any populated bin with A > 1, so its sqrt throws);
 *      the evident intent is σℓ = sqrt((S2/A − (S1/A)²) / N), which the Python layer returns. */
enum { CMBL_CL_A = 0, CMBL_CL_SL = 1, CMBL_CL_COUNT = 2 };
int cmbl_clbins_create(cmbl_ctx* ctx, const double* ledges_host, int nedges, const double* w_host, size_t nw, cmbl_clbins** out);
int cmbl_clbins_destroy(cmbl_clbins* bins);
int cmbl_clbins_info_host(cmbl_clbins* bins, int which, double* out_host, size_t n);
int cmbl_get_cl(cmbl_ctx* ctx, cmbl_clbins* bins, int basis, const void* f1, const void* f2, int npol, int nbatch,
                const int* pairs_host, int npairs, int moments, double* out);

/* ---- diagonal operators: DiagOp `*` and `\` with automatic basis conversion, BlockDiagIEB
 *      (src/specialops.jl:9-10, 61-118; src/field_vectors.jl:64-66).
 *      diag: real (Ny/2+1, Nx, npol) planes, diagonal in `basis_diag` (FOURIER or HARMONIC). */
int cmbl_diag_apply(cmbl_ctx* ctx, int kind, int basis_diag, const void* diag,
                    int basis_in, const void* in, int basis_out, void* out, int npol, int nbatch);
/* te_bb: 5 real planes (TT, TE, ET, EE, BB): (i,e) = [TT TE; ET EE](I,E), b = BB*B */
int cmbl_blockdiag_ieb_apply(cmbl_ctx* ctx, const void* te_bb, int transpose,
                             int basis_in, const void* in, int basis_out, void* out, int nbatch);

/* ---- per-batch reductions: dot, logdet (src/proj_lambert.jl:318-342) */
int cmbl_dot(cmbl_ctx* ctx, int basis, const void* a, const void* b, int npol, int nbatch, double* out_host);
int cmbl_logdet(cmbl_ctx* ctx, const void* diag_fourier, int nplanes, double* out_host);
/* norm(f) = sqrt(dot(f,f)) (src/generic.jl:373), one value per batch slot */
int cmbl_norm(cmbl_ctx* ctx, int basis, const void* a, int npol, int nbatch, double* out_host);
/* logdet / tr of Diagonal(field) (src/proj_lambert.jl:331-353), per batch slot.  basis MAP: `diag` is a real map,
 * logdet = sum log|d| + log(prod sign d) -- NaN for an odd number of negative entries (Julia's log(-1.0) throws), -Inf with a
 * zero entry; FOURIER / HARMONIC: `diag` is a complex half-plane field, logdet = sum lambda_rfft * log|d| (non-finite terms
 * dropped), tr = sum lambda_rfft * Re d. */
int cmbl_logdet_diag(cmbl_ctx* ctx, int basis, const void* diag, int npol, int nbatch, double* out_host);
int cmbl_tr_diag(cmbl_ctx* ctx, int basis, const void* diag, int npol, int nbatch, double* out_host);
/* set_sum_accuracy_mode! (src/util.jl:288-316) for every reduction of this context (dot, norm, logdet, tr, the quadratic forms
 * of logpdf, the conjugate-gradient residuals).  Every term is formed in the working precision like the reference's broadcast;
 * the mode selects how the terms are added: WORKING = plain sum in the working precision (the reference's default `nothing`),
 * FLOAT64 = sum(Float64.(A)), KAHAN = compensated (sum_kbn).  The engine's default is FLOAT64: the reductions are HBM-bound
 * and double accumulation is free, whereas fp32 accumulation of ~1e6 terms loses the O(1) differences HMC accepts on. */
enum { CMBL_SUM_WORKING = 0, CMBL_SUM_FLOAT64 = 1, CMBL_SUM_KAHAN = 2 };
int cmbl_set_sum_accuracy_mode(cmbl_ctx* ctx, int mode);

/* ---- LenseFlow: LenseFlow / CachedLenseFlow, precompute!!, the four flow operators and the two
 *      Zygote pullbacks (src/lenseflow.jl:19-214, src/flowops.jl:11-14, 40-68) */
int cmbl_lenseflow_create(cmbl_ctx* ctx, int nsteps, cmbl_flow** out);
int cmbl_lenseflow_destroy(cmbl_flow* L);
/* precompute!(L): phi in `basis` (MAP or FOURIER), (.., 1, nbatch_phi) */
int cmbl_lenseflow_set_phi(cmbl_flow* L, int basis, const void* phi, int nbatch_phi);
int cmbl_lenseflow_apply(cmbl_flow* L, int mode, int basis_in, const void* in, int basis_out, void* out,
                         int npol, int nbatch);
/* pullback of  mode=FWD: ftilde = L*f   (delta flow t 1->0 from (ftilde, delta, 0))
 *              mode=INV: f = L\ftilde   (delta flow t 0->1 from (f, delta, 0)).
 * f_end: the OUTPUT of the primal op (MAP basis); delta: cotangent in basis_delta.
 * outputs: dphi (FOURIER, (Ny/2+1,Nx,1,nbatch)), df (basis_df), f_start (MAP; may be NULL).
 * alias_quirk != 0 reproduces the reference's in-place aliasing (src/lenseflow.jl:198-200 with
 * src/field_vectors.jl:48-49); 0 gives the mathematically consistent gradient.
 * dphi is formed as the RK4 quadrature sum over all stages (its velocity never depends on dphi itself), which equals the reference's
 * stage-by-stage update up to the order of floating-point summation.  The handle keeps 4*nsteps*2 maps of scratch per (pol,batch)
 * slice for it (448 MB at 1024^2 QU fp32, nsteps = 7).  Streams: the handle owns a few internal streams that it forks from / joins
 * into the context's stream inside a call (independent pol slices / batch groups run as concurrent launch chains); on return all
 * work is ordered on the context's stream as for every other entry point. */
int cmbl_lenseflow_grad(cmbl_flow* L, int mode, const void* f_end, int basis_delta, const void* delta,
                        void* dphi_out, int basis_df, void* df_out, void* f_start_out,
                        int npol, int nbatch, int alias_quirk);

/* get_max_lensing_step(phi, eta) (src/lenseflow.jl:242-256): largest alpha keeping I + grad grad(phi + alpha eta)
 * non-singular, one value per batch slot. */
int cmbl_max_lensing_step(cmbl_flow* L, int basis, const void* phi, const void* eta, int nbatch, double* out_host);

/* ---- BilinearLens: lensing by bilinear interpolation (src/bilinearlens.jl) with the reference's gmres (src/numerical_algorithms.jl:193-214).
 * One phi, any number of (pol, batch) slices of f; pixel (i, j) -- i along Ny, j along Nx -- reads its four neighbours at
 * (i + d_y phi / dx, j + d_x phi / dx), wrapped periodically, with the closed-form bilinear weights (:42-74).  The pixel index is added in integers
 * after floor and fraction are taken from the deflection alone (the reference adds 1:Ny in the working precision, :44-45).
 *   cmbl_bilinear_create / _destroy: BilinearLens (:24-28) on a context.
 *   cmbl_bilinear_set_phi: BilinearLens(phi) (:31-87).  nbatch_phi != 1 is CMBL_ERR_SHAPE (:40).  norm(phi) == 0 makes every action a copy (:34).
 *        The tables of BilinearLens(-phi) (:92-97) and the transposed operators are made on first use and kept until the next set_phi.
 *   cmbl_bilinear_set_deflection: the same operator from two device MAPs (Nx x Ny reals each, the context's precision) of the deflection in
 *        PIXELS (cmbl_powerlens_set_deflection takes radians) along Ny (dy_px) and along Nx (dx_px) -- lensing by an arbitrary displacement (compute_row!, :55-74, on given positions).
 *   cmbl_bilinear_apply: mode CMBL_FLOW_FWD L*f (:107-115), _ADJ L'*f (:117-125; summed in a fixed order: bit-identical between runs), _INV L\f
 *        (:127-138) and _INVADJ L'\f (:140-151): per slice gmres(A, b, Pl = BilinearLens(-phi), maxiter), formed as Arnoldi with modified
 *        Gram-Schmidt; 1 <= maxiter <= 16 (the reference uses 5), ignored by the other modes.  Fields in any basis, ABI
 *        layouts; the work is done on maps (:109).  Before any set_phi / set_deflection: CMBL_ERR_STATE, as cmbl_lenseflow_apply.
 *   cmbl_bilinear_grad: the pullback of L*f (:165-171) from the primal output f_lensed (MAP) and the cotangent delta (basis_delta):
 *        df_out = L' delta in basis_df, dphi_out = grad' . (sum_pol delta * grad f_lensed) (FOURIER, (Ny/2+1, Nx, 1, nbatch)), with the spectral
 *        gradient of f_lensed as in the reference. */
int cmbl_bilinear_create(cmbl_ctx* ctx, cmbl_bilinear** out);
int cmbl_bilinear_destroy(cmbl_bilinear* L);
int cmbl_bilinear_set_phi(cmbl_bilinear* L, int basis, const void* phi, int nbatch_phi);
int cmbl_bilinear_set_deflection(cmbl_bilinear* L, const void* dy_px, const void* dx_px);
int cmbl_bilinear_apply(cmbl_bilinear* L, int mode, int basis_in, const void* in, int basis_out, void* out,
                        int npol, int nbatch, int maxiter);
int cmbl_bilinear_grad(cmbl_bilinear* L, const void* f_lensed, int basis_delta, const void* delta,
                       void* dphi_out, int basis_df, void* df_out, int npol, int nbatch);

/* ---- PowerLens and Taylens: lensing by a Taylor series in the deflection (src/powerlens.jl, src/taylens.jl).
 * With d = (dx, dy) the deflection and the derivatives applied in Fourier space as (i lx)^a (i ly)^b:
 *   PowerLens(order) f  = f + sum_{n=1..order} sum_{a+b=n} dx^a dy^b / (a! b!) irfft((i lx)^a (i ly)^b rfft f)             (src/powerlens.jl:40-48)
 *   PowerLens(order)' g = rfft g + sum_n (-1)^n sum_{a+b=n} (i lx)^a (i ly)^b rfft(dx^a dy^b g) / (a! b!)                   (:50-58)
 *   Taylens(order) f    = the same sum with the residual d - round(d / dx_pix) dx_pix in place of d, f and every derivative map read at
 *                         the pixel round(d / dx_pix) away, round half to even (src/taylens.jl:25-66).  Taylens(0) is that permutation alone.
 * The engine forms every term in pixel units (l dx_pix and d / dx_pix): the same number term for term, and no power leaves the range of
 * single precision (as written, l^10 overflows Float32 at 2' pixels).  One deflection, any number of (pol, batch) slices of f; nothing
 * synchronises with the host and the sums run in a fixed order: results are bit-identical between runs.
 *   cmbl_powerlens_create: order in [0, 12], kind CMBL_POWERLENS or CMBL_TAYLENS; anything else is CMBL_ERR_ARG.
 *   cmbl_powerlens_set_phi: PowerLens(phi, order) (:23), d = grad phi.  nbatch_phi != 1 is CMBL_ERR_SHAPE (require_unbatched, :25).
 *   cmbl_powerlens_set_deflection: PowerLens(d::FieldVector, order) (:24) from two device MAPs (Nx x Ny reals each, the context's precision)
 *        of the deflection along Ny (dy_rad) and along Nx (dx_rad), argument order as cmbl_bilinear_set_deflection -- but in RADIANS, the
 *        unit of the reference's constructor, where cmbl_bilinear_set_deflection takes pixels.
 *   cmbl_powerlens_apply: mode CMBL_FLOW_FWD L*f or, for a PowerLens, CMBL_FLOW_ADJ L'*g (which the reference returns in the Fourier
 *        basis).  _ADJ on a Taylens and _INV / _INVADJ on either are CMBL_ERR_ARG: the reference defines none of them.  Fields in any
 *        basis, ABI layouts, `in` and `out` may be the same array.  Before any set_phi / set_deflection: CMBL_ERR_STATE.
 * antilensing(L) (:36-38; the line as written cannot run) is the operator of -d: set_phi / set_deflection of a second handle with the negated
 * argument. */
enum { CMBL_POWERLENS = 0, CMBL_TAYLENS = 1 };
int cmbl_powerlens_create(cmbl_ctx* ctx, int order, int kind, cmbl_powerlens** out);
int cmbl_powerlens_destroy(cmbl_powerlens* L);
int cmbl_powerlens_set_phi(cmbl_powerlens* L, int basis, const void* phi, int nbatch_phi);
int cmbl_powerlens_set_deflection(cmbl_powerlens* L, const void* dy_rad, const void* dx_rad);
int cmbl_powerlens_apply(cmbl_powerlens* L, int mode, int basis_in, const void* in, int basis_out, void* out,
                         int npol, int nbatch);

/* ---- make_mask(Nside, θpix; edge_padding_deg, edge_rounding_deg, apodization_deg, ptsrc_radius_arcmin, num_ptsrcs) (src/masking.jl:1-67;
 *      load_sim's pixel_mask_kwargs, src/dataset.jl:279-281): apodised border and point-source mask on the device.  Widths are in PIXELS: the
 *      host converts with deg2npix(x) = round(x / θpix * 60) and arcmin2npix(x) = round(x / θpix), round half to even (:11-12).  All arithmetic
 *      is int32 or double whatever the context's precision; nothing is accumulated with atomics, results are bit-identical between runs.
 *   cmbl_edt_sq: d2[x][y] (int32, laid out like a map plane) = squared Euclidean distance from pixel (y, x) to the nearest non-zero byte of
 *      feat[x][y] (ImageMorphology.feature_transform + norm, :42-43, 48-49), exact.  A plane without a feature is CMBL_ERR_ARG (d2 is then
 *      not meaningful).  Synchronises the context's stream.
 *   cmbl_make_mask: `src_yx_host`: nsrc pairs (y, x), 0-based, on the HOST (sim_ptsrcs, :60-67, with the positions given; duplicates allowed);
 *      `out_map_dev`: one map plane (Ny, Nx, 1, 1) in the context's precision.  With boundary = all pixels but the outer `pad` rows and columns
 *      (:31-38), bleed = d(nearest source) < src_w (:40-44, decided as d2 < src_w^2 on integers), ptsrc = !bleed and
 *      cos_apod(img, w, s) = (1 - cos(min(d, w) / w * pi)) / 2, d the distance to the nearest false pixel of img, filtered (s > 0) BEFORE the
 *      clamp with Kernel.gaussian(s) of ImageFiltering.jl: per axis 4 s + 1 taps exp(-x^2 / 2 s^2) normalised to sum 1, border "replicate" (:46-54):
 *        apod_w == 0:  boundary & ptsrc, values in {0, 1} (:17; round_w is ignored)
 *        apod_w  > 0:  cos_apod(boundary, apod_w, round_w) * cos_apod(ptsrc, src_w) (:19-20); round_w == 0: no filter (`0 != false` is false)
 *      nsrc == 0: the point-source factor is 1 (:14, 19).  The result is rounded to float32 whatever the precision (Float32.(...), :23; a
 *      float64 context stores those values widened, T.(...) in src/dataset.jl:280).  2 pad >= min(Ny, Nx) is legal: an all-zero mask.
 *      What the reference leaves undefined is CMBL_ERR_ARG, checked before any launch: a negative width or count; apod_w > 0 with pad == 0 (no
 *      false pixel to measure to); nsrc > 0 with src_w == 0; a source outside the map; nsrc > 0 without positions.  round_w > 1024 (4097 taps,
 *      wider than any map) is CMBL_ERR_ARG as well.  Synchronises the context's stream; the scratch planes live for the call only. */
int cmbl_edt_sq(cmbl_ctx* ctx, const uint8_t* feat_dev, int32_t* d2_dev);
int cmbl_make_mask(cmbl_ctx* ctx, const int32_t* src_yx_host, int nsrc, int pad, int apod_w, int round_w, int src_w, void* out_map_dev);

/* ---- ProjEquiRect (src/proj_equirect.jl): the equirectangular projection, its azimuthal Fourier bases and block-diagonal operators.
 *      Arrays are the reference's, column-major: maps (Ny, Nx, npol, nbatch) with θ contiguous; AzFourier fields (n, Nx/2+1, nbatch) complex with
 *      n = Ny (I) or 2 Ny (QU); operators `blocks` (n, n, Nx/2+1), row index contiguous, real (blocks_complex = 0) or complex elements of the
 *      context's precision.  The context supplies Ny, Nx, precision, stream and scratch; its pixel size is not used.  Nothing is accumulated with
 *      atomics, results are bit-identical between runs.  NOT included: the AD rules (:242-248, 349-351), IQUAzFourier (an alias without a
 *      transform), lensing on this projection.
 *   cmbl_equirect_geometry_host: ProjEquiRect(; Ny, Nx, θspan, φspan) (:71-81, 112-120) on the host in double, no context and no device needed.  The
 *      spans are sorted.  theta_edges = range(θspan, Ny+1) (Ny+1 values), theta = its midpoints (Ny); phi_edges (Nx+1) and phi (Nx) = rem2pi(·, RoundDown)
 *      of the equispaced edges and midpoints, in [0, 2π); omega[j] = rem2pi(phi_edges[1] − phi_edges[0]) (cos θedges[j] − cos θedges[j+1]) (Ny);
 *      lx[j + Ny i] = ifftshift(−Nx÷2 … (Nx−1)÷2)[i] · 2π / (Nx Δx[j]), Δx[j] = sin θ[j] |φspan₂ − φspan₁| / Nx (Ny × Nx).  Any output may be NULL.
 *      Ny, Nx outside [2, 4096]: CMBL_ERR_SHAPE.
 *   cmbl_equirect_convert: basis_in / basis_out: CMBL_MAP or CMBL_AZFOURIER (others: CMBL_ERR_ARG); equal bases copy.  npol = 1: AzFourier(f) =
 *      rfft along φ / √Nx and Map(f) = irfft along φ · √Nx (:149-157; FFTW's c2r rule: the imaginary parts of m = 0, and of m = Nx/2 for even Nx, are
 *      never read); any Nx.  npol = 2: QUAzFourier (:160-168): F = fft_φ(Q + iU) / √Nx, rows 0 … Ny−1 of column m hold F[:, m], rows Ny … 2Ny−1
 *      conj(F[:, (Nx − m) mod Nx]); QUMap (:170-178): F[:, 0 … Nx/2] = the top rows, THEN F[:, (Nx − m) mod Nx] = conj(bottom rows of column m) -- columns
 *      0 and Nx/2 are assigned twice and the second assignment wins, as in the reference -- then Q + iU = ifft_φ(F) · √Nx.  Odd Nx with npol = 2 is
 *      CMBL_ERR_SHAPE (the reference throws a dimension mismatch, :166); npol = 3 is CMBL_ERR_ARG; `in == out` is CMBL_ERR_ARG.
 *   cmbl_equirect_block_apply: M * f (:230-233), out[p, m, b] = Σ_q M[p, q, m] f[q, m, b]; adjoint != 0: M' * f (:237-240), with conj(M[q, p, m]).
 *      n must be Ny or 2 Ny (CMBL_ERR_SHAPE).  Real blocks are read as real.  Every block element is fetched once per 8 batch slots.  `in == out` is
 *      CMBL_ERR_ARG.
 *   cmbl_equirect_block_matmul: M₁ * M₂, M₁' * M₂ (adjA), M₁ * M₂' (adjB) (:254-269), on the matrix cores (exact f32 / f64 MFMA).  Both adjoints, or
 *      `out` aliasing an input: CMBL_ERR_ARG.  A, B and out share n and element type.
 *   cmbl_equirect_block_dot: dot(M₁', M₂) = Σ conj(A[q, p, m]) B[p, q, m] (:358-360), accumulated in double in a fixed order; out_host = (re, im).
 *      Synchronises the context's stream.
 *   cmbl_equirect_block_scale_columns: blocks[j, k, m] *= w[k] in place, w rounded to the context's precision (Cℓ_to_Beam(:I), :505-515); nw != n
 *      is CMBL_ERR_SHAPE.
 *   cmbl_equirect_beam_pol: out (2Ny, 2Ny, Nx/2+1) complex = [B 0; 0 B] · diag(Ω, Ω) from the real blocks B (Ny, Ny, Nx/2+1) (Cℓ_to_Beam(:P), :517-533);
 *      omega_host: Ny doubles.  The two beam calls copy their weights to the device before they return (one blocking copy).
 *   cmbl_equirect_cov: Cℓ_to_Cov(:I) (pol = 0) and Cℓ_to_Cov(:P) (pol = 2) (:430-503).  The reference delegates the arithmetic to CirculantCov.jl; here the
 *      blocks are DEFINED as the covariance of the AzFourier / QUAzFourier coefficients of an isotropic Gaussian field with the given spectra (DESIGN
 *      §4.7; P = Q + iU = -Σ (E + iB)ℓm ₂Yℓm with respect to (e_θ, e_φ)) on the geometry of cmbl_equirect_geometry_host(Ny, Nx, theta_span, phi_span)
 *      -- the context holds the sizes, not the spans, hence the two span arguments.  The azimuthal span must be 2π/K for an integer K >= 1
 *      (|K - round K| <= 1e-9 K), else CMBL_ERR_SHAPE: no other span has a block-diagonal covariance.  cl_a (TT, or EE) and cl_b (BB; NULL for pol = 0):
 *      HOST arrays of lmax + 1 doubles, C_ℓ at ℓ = 0 ... lmax (the caller interpolates and sets NaN to 0 like nan2zero.(C(ℓ)); a value that is not
 *      finite is CMBL_ERR_NAN).  blocks_out: DEVICE array (Nx/2+1) n n of the context's precision indexed [m][q][p] like every operator here, real
 *      n = Ny (pol 0) or complex n = 2 Ny (pol 2: [j, k] = γ_m, [j, k+Ny] = ξ_m, [j+Ny, k] = conj ξ_J(m), [j+Ny, k+Ny] = conj γ_J(m), :488-494).
 *      ngrid = 0: the correlation functions by their three-term recurrences at every separation (exact mode); ngrid >= 4: from a table on ngrid
 *      uniform nodes of [0, π] by 4-point Lagrange interpolation (the reference's CirculantCov uses a spline on 50 000 nodes); 1 ... 3:
 *      CMBL_ERR_SHAPE.  Odd Nx or lmax < 2 with pol = 2, lmax > 100000: CMBL_ERR_SHAPE.  All arithmetic is double in either precision; only the store rounds.
 *      Bit-identical between runs and for every "eq_cov_scratch_mb".  Synchronises the context's stream.
 *   The three factorisation calls below (sqrt, pinv, logabsdet, \ and / of BlockDiagEquiRect, :274-282, 313-347) share these rules: one workgroup
 *      factorises one block, synchronising by the workgroup barrier alone, every loop bounded at launch; ALL arithmetic is double (real or complex) in
 *      either precision and only the final store rounds to the block type; the double working copies go through slabs of "eq_factor_scratch_mb";
 *      results are bit-identical between runs and for every slab size.  n must be Ny or 2 Ny and at most 2048 (CMBL_ERR_SHAPE, checked before
 *      anything is allocated); an input element that is not finite is CMBL_ERR_NAN, before anything is factorised; an output aliasing an input is
 *      CMBL_ERR_ARG.  Each call synchronises the context's stream.
 *   cmbl_equirect_block_svd: one-sided Jacobi SVD of every block (Hestenes: G = A, V = I, column pairs in a round-robin order rotated while
 *      |g_i' g_j| > n 2^-53 |g_i| |g_j|; a pair whose columns both lie at or below n 2^-53 |A|_F, one of whose columns lies at or below 2^-106 |A|_F, or with an exactly zero norm or product, is
 *      skipped), until a sweep rotates nothing or 60 sweeps -- then CMBL_ERR_STATE, the message names the block.  σ_k = |g_k|.  out_sqrt (may be
 *      NULL) = U √S V' = G diag(σ^-1/2) V' with the term dropped where σ_k = 0 exactly and no other cut-off (:313-323); out_pinv (may be NULL) =
 *      V diag(σ^-2) G' with the term dropped where σ_k <= rtol max σ.  sv_host (may be NULL): (Nx/2+1) n doubles, the singular values of every block
 *      in descending order; sweeps_host (may be NULL): Nx/2+1 ints, the sweeps each block took.  rtol negative or not finite: CMBL_ERR_ARG.
 *   cmbl_equirect_block_logabsdet: LU with partial pivoting (largest modulus, a tie to the lowest row) of every block; out_host = (Σ log|u_kk|,
 *      Re s, Im s), s = Π u_kk / |u_kk| times the permutation parities, summed on the host in double in the order (m, k) (:342-347).  An exactly
 *      zero pivot gives (-inf, 0, 0) like slogdet and is no error.
 *   cmbl_equirect_block_solve: side = CMBL_SIDE_LEFT: out = A \ rhs; CMBL_SIDE_RIGHT: out = rhs / A (the left solve with A' on the
 *      conjugate-transposed right-hand sides).  rhs_kind = CMBL_RHS_BLOCKS: rhs and out are block arrays like A (M₁ \ M₂, M₁ / M₂, :274-282; nbatch
 *      is ignored); CMBL_RHS_FIELD: AzFourier fields (n, Nx/2+1, nbatch), complex, left side only (M \ f).  a_complex / rhs_complex give the two
 *      element types; out is complex when either is.  An exactly zero pivot is CMBL_ERR_NAN and the message names the block. */
int cmbl_equirect_geometry_host(int Ny, int Nx, const double* theta_span, const double* phi_span, double* theta, double* phi,
                                double* theta_edges, double* phi_edges, double* omega, double* lx);
int cmbl_equirect_convert(cmbl_ctx* ctx, int basis_in, const void* in, int basis_out, void* out, int npol, int nbatch);
int cmbl_equirect_block_apply(cmbl_ctx* ctx, const void* blocks, int blocks_complex, int n, int adjoint, const void* in, void* out, int nbatch);
int cmbl_equirect_block_matmul(cmbl_ctx* ctx, const void* A, int adjA, const void* B, int adjB, int blocks_complex, int n, void* out);
int cmbl_equirect_block_dot(cmbl_ctx* ctx, const void* A, const void* B, int blocks_complex, int n, double* out_host);
int cmbl_equirect_block_scale_columns(cmbl_ctx* ctx, void* blocks, int blocks_complex, int n, const double* w_host, int nw);
int cmbl_equirect_beam_pol(cmbl_ctx* ctx, const void* blocksI_real, const double* omega_host, void* out_complex);
enum { CMBL_SIDE_LEFT = 0, CMBL_SIDE_RIGHT = 1 };
enum { CMBL_RHS_BLOCKS = 0, CMBL_RHS_FIELD = 1 };
int cmbl_equirect_block_svd(cmbl_ctx* ctx, const void* blocks, int blocks_complex, int n, double rtol, void* out_sqrt, void* out_pinv,
                            double* sv_host, int* sweeps_host);
int cmbl_equirect_block_logabsdet(cmbl_ctx* ctx, const void* blocks, int blocks_complex, int n, double* out_host);
int cmbl_equirect_block_solve(cmbl_ctx* ctx, const void* A, int a_complex, int n, int side, const void* rhs, int rhs_complex, int rhs_kind,
                              void* out, int nbatch);
int cmbl_equirect_cov(cmbl_ctx* ctx, const double* theta_span, const double* phi_span, int pol, int lmax, const double* cl_a, const double* cl_b,
                      int ngrid, void* blocks_out);

/* ---- NoLensingDataSet on ProjEquiRect (src/dataset.jl:37-47, 68-80): d = M B f + noise, f ~ N(0, Cf), noise ~ N(0, Cn), and its Wiener filter.
 * Cf^-1, B, the preconditioner and (block form) Cn^-1 are BlockDiagEquiRect arrays [m][q][p] of the context's precision; M and (pixel form) Cn^-1 are
 * map-diagonal: nplanes = 1 or npol planes (Ny, Nx), the reference's Diagonal(::EquiRectMap).  Fields are CMBL_AZFOURIER arrays (n, Nx/2+1, nbatch),
 * n = npol Ny; data are CMBL_MAP arrays (Ny, Nx, npol, nbatch).  nbatch <= 256.
 *   The reference's argmaxf_logpdf (src/maximization.jl:17-42) begins with zero(diag(ds.Cf)) and defines no diag(::BlockDiagEquiRect), so as written
 *   it does not run on such a data set: what is built here is its algorithm (conjugate_gradient, src/numerical_algorithms.jl:73-134) on its operators
 *   (model :68-73, hand gradient :76-80 without L, preconditioner :129-132), with the zero field of Cf's basis as the start.
 *   PRECONDITION of every entry point below: each block operator maps images of maps to images of maps -- spin-0 blocks are real at columns m = 0 and
 *   m = Nx/2; spin-2 blocks at those columns commute with v -> S conj(v), S the swap of the two halves of the 2 Ny vector (the [[G, X], [conj X, conj G]]
 *   blocks of cmbl_equirect_cov and cmbl_equirect_beam_pol).  The CG vectors are held in the Az basis and their dot products are the map dot
 *   (src/proj_equirect.jl:355) formed there, which is the reference's inner product under this precondition only.  It is not checked here.
 *   cmbl_eqds_create: npol = 1 (spin 0) or 2 (spin 2; an odd Nx is CMBL_ERR_SHAPE, :166), else CMBL_ERR_ARG.
 *   cmbl_eqds_set_block_op: a NON-OWNING view (the arrays are gigabytes): the caller keeps `blocks_dev` alive and unchanged while the data set uses it.
 *      n != npol Ny is CMBL_ERR_SHAPE.  blocks_dev == NULL unsets CMBL_EQDS_B (identity) or CMBL_EQDS_CN_INV; for the others it is CMBL_ERR_ARG.
 *      CMBL_EQDS_PRECOND_INV is the operator MULTIPLIED onto the residual: pinv(pinv(Cf) + B^' M^' pinv(Cn^) M^ B^) (:129-132).
 *   cmbl_eqds_set_pixel_op: the planes are COPIED.  map_dev == NULL unsets.  nplanes other than 1 or npol: CMBL_ERR_SHAPE.  CMBL_EQDS_CN_INV_PIX holds 1 / variance.
 *   cmbl_eqds_set_logdet: logdet Cn + logdet Cf, set by the caller like cmbl_dataset_set_logdet.
 *   cmbl_eqds_mean: d_out = M B f (:68-73 without L).
 *   cmbl_eqds_gradientf_logpdf: B' M' Cn^-1 (d - M B f) - Cf^-1 f (:76-80 without L).  f_az == NULL: f = 0; d_map == NULL: d = 0; both: CMBL_ERR_ARG.
 *   cmbl_eqds_logpdf: lp_host[b] = -1/2 [ (d - MBf)' Cn^-1 (d - MBf) + f' Cf^-1 f + logdet ] (:59-66).  Synchronises.
 *   cmbl_eqds_wiener_cg: preconditioned CG on A = Cf^-1 + B'M'Cn^-1 M B, b = B'M'Cn^-1 d with the semantics of cmbl_wiener_cg: res = dot(r, z), stop when
 *      all(res < tol), the best-res iterate goes to f_out, res_hist_host (maxit * nbatch doubles) gets *nit_host residual vectors, a NaN residual is
 *      CMBL_ERR_NAN.  fstart_az == NULL starts from zero.  Scalars, history and flags live on the device; no host synchronisation inside an iteration.
 *      Every output has one writer and one order of operations: two runs are bit-identical.
 *   State: CMBL_ERR_STATE when CMBL_EQDS_CF_INV is missing, when no form or both forms of Cn^-1 are set (mean needs none), or (wiener_cg) when
 *      CMBL_EQDS_PRECOND_INV is missing.  nbatch outside [1, 256]: CMBL_ERR_SHAPE.
 *   cmbl_equirect_field_dot: out_host[b] = dot(a_b, b_b) (src/proj_equirect.jl:355) per batch slot, in double, two stages, fixed order.  basis CMBL_MAP:
 *      the plain dot of the map arrays; CMBL_AZFOURIER: the same number for images of maps, spin 0: sum_m w_m Re(conj(a) b) with w = 1 at m = 0 and
 *      m = Nx/2 (even Nx), 2 elsewhere; spin 2: over all 2 Ny rows with w = 1/2 at columns 0 and Nx/2, 1 elsewhere.  Synchronises. */
typedef struct cmbl_eqds cmbl_eqds;
enum { CMBL_EQDS_CF_INV = 0, CMBL_EQDS_B = 1, CMBL_EQDS_PRECOND_INV = 2, CMBL_EQDS_CN_INV = 3 };   /* block operators */
enum { CMBL_EQDS_MASK = 0, CMBL_EQDS_CN_INV_PIX = 1 };                                               /* map-diagonal operators */
int cmbl_eqds_create(cmbl_ctx* ctx, int npol, cmbl_eqds** out);
int cmbl_eqds_destroy(cmbl_eqds* ds);
int cmbl_eqds_set_block_op(cmbl_eqds* ds, int which, const void* blocks_dev, int blocks_complex, int n);
int cmbl_eqds_set_pixel_op(cmbl_eqds* ds, int which, const void* map_dev, int nplanes);
int cmbl_eqds_set_logdet(cmbl_eqds* ds, double logdet_sum);
int cmbl_eqds_mean(cmbl_eqds* ds, const void* f_az, void* d_out_map, int nbatch);
int cmbl_eqds_gradientf_logpdf(cmbl_eqds* ds, const void* f_az, const void* d_map, void* out_az, int nbatch);
int cmbl_eqds_logpdf(cmbl_eqds* ds, const void* f_az, const void* d_map, double* lp_host, int nbatch);
int cmbl_eqds_wiener_cg(cmbl_eqds* ds, const void* d_map, const void* fstart_az, double tol, int maxit, void* f_out_az, double* res_hist_host,
                        int* nit_host, int nbatch);
int cmbl_equirect_field_dot(cmbl_ctx* ctx, int basis, const void* a, const void* b, int npol, int nbatch, double* out_host);

/* ---- small helpers used by the drivers above the hot kernels
 * axpby: out = a[b]*x + b[b]*y per batch slot (y may be NULL) -- the FieldTuple / Field broadcasts of the CG, line-search
 *        and leapfrog updates (src/numerical_algorithms.jl:102-107, src/sampling.jl:29-31).
 * qe_leg: Map(nan2zero(in * (i lx)^p1 (i ly)^p2 / |l|^n)) (src/quadratic_estimate.jl:89-91), in: Fourier S0.
 * fourier_lmul: (i lx)^p1 (i ly)^p2 * rfft(map) or (take_abs) its modulus in the real part (src/quadratic_estimate.jl:97,118).
 * map_fma: out = [out +] scale * a * b on maps (products of legs). */
int cmbl_axpby(cmbl_ctx* ctx, int basis, const double* a_host, const void* x, const double* b_host, const void* y, void* out,
               int npol, int nbatch);
int cmbl_qe_leg(cmbl_ctx* ctx, const void* in_fourier, int n, int p1, int p2, void* out_map, int nbatch);
int cmbl_fourier_lmul(cmbl_ctx* ctx, const void* in_map, int p1, int p2, int take_abs, void* out_fourier, int nbatch);
int cmbl_map_fma(cmbl_ctx* ctx, const void* a, const void* b, double scale, void* out, int accumulate, int nslices);

/* ---- white noise for `simulate` / `randn!` (src/specialops.jl:6,93: sqrt(D) * randn!(rng, similar(diag(D)));
 * src/base_fields.jl:169-170: randn! fills the Map array).  Replaces the reference's host RNG + upload
 * (ext/CMBLensingCUDAExt.jl:72-73) / CURAND stream.  Slot b of `out` (n_per_slot reals of the context's dtype, e.g. one
 * chain's (Ny,Nx,P) map block) is filled with N(0,1) draws of the counter-based generator Philox4x32-10 keyed by
 * seeds_host[b]; `stream` selects an independent sequence of the same key (e.g. a running draw counter).  Element j of a slot
 * depends only on (seed, stream, j): counter (j/4, stream), Box-Muller in fp64 on u = (w + 0.5)/2^32 of word pairs. */
int cmbl_randn(cmbl_ctx* ctx, const uint64_t* seeds_host, int nslots, uint64_t stream, void* out, long n_per_slot);

/* ---- data model, Wiener filter and posterior (src/dataset.jl:37-137, src/maximization.jl:17-42,
 *      src/numerical_algorithms.jl:73-134).  Operators are set as real planes in the reference
 *      layout; *_INV operators are the caller's pinv() of the reference operators. */
enum { CMBL_OP_CF_INV = 0,     /* pinv(Cf)                                   harmonic, npol planes (5 for IQU) */
       CMBL_OP_CN_INV = 1,     /* pinv(Cn)                                                                      */
       CMBL_OP_B = 2,          /* beam / transfer function                                                      */
       CMBL_OP_MF = 3,         /* Fourier-space mask                                                            */
       CMBL_OP_D = 4,          /* mixing matrix D                                                               */
       CMBL_OP_D_INV = 5,      /* operator applied for `D \ f` (pinv(D), or D itself with DIV semantics)        */
       CMBL_OP_PRECOND_INV = 6,/* pinv(Cf^-1 + B'M'Cn^-1 M B)  (src/dataset.jl:129-132)                          */
       CMBL_OP_CPHI_INV = 7,   /* pinv(Cphi), 1 plane                                                           */
       CMBL_OP_G_INV = 8,      /* pinv(G), 1 plane                                                              */
       CMBL_OP_MPIX = 9,       /* pixel mask, real (Ny,Nx) map; optional                                        */
       CMBL_OP_CN_INV_PIX = 10,/* pinv(V) of Cn = Diagonal(V), real (Ny,Nx) maps; optional (see below)          */
       CMBL_OP_COUNT = 11 };
/* CMBL_OP_CN_INV_PIX: a noise covariance that is diagonal in the I/QU MAP basis, Cn = Diagonal(V) with V the variance per pixel -- the
 * inhomogeneous noise of a survey's hit-count map.  BaseDataSet.Cn is "any operator" (src/dataset.jl:37-47), pinv(Cn(theta)) is all that
 * gradientf_logpdf asks of it (:76-80), and logdet(Diagonal(::Map)) exists for it (src/proj_lambert.jl:337-342).  planes: device maps
 * (nplanes, Ny, Nx) in the layout of CMBL_OP_MPIX and of MAP fields, nplanes = 1 (one map for all pol slices) or npol (I | Q,U | I,Q,U);
 * anything else is CMBL_ERR_SHAPE.  They are the caller's pinv of the variance: 0 where the variance is 0 or infinite.  No batch axis.
 * While set, this IS the data set's noise operator and CMBL_OP_CN_INV is read by no entry point; nplanes = 0 (planes may be NULL) clears it.
 * pinv(Cn) z is then rfft2(w .* irfft2(z)) between the EB <-> QU basis changes; z' pinv(Cn) z stays a Fourier-domain dot (the default `dot`,
 * src/proj_lambert.jl:328), so the sum-accuracy modes keep their meaning.  The fused forms of the posterior and of the Wiener CG (option
 * fused_harm) are not used while it is set: every entry point below runs its composed form.  The approximate, Fourier-diagonal Cn^ (what the
 * preconditioner, D and the quadratic estimator read, :41, 129-132, 316-328) stays with the caller, inside CMBL_OP_PRECOND_INV / CMBL_OP_D.
 * cmbl_dataset_noise_inv: out = pinv(Cn) * in with whichever form is set (HARMONIC in and out, nbatch slots, in place allowed);
 * CMBL_ERR_STATE if neither is. */
int cmbl_dataset_create(cmbl_ctx* ctx, int npol, cmbl_dataset** out);
int cmbl_dataset_destroy(cmbl_dataset* ds);
int cmbl_dataset_set_op(cmbl_dataset* ds, int which, const void* planes, int nplanes);
int cmbl_dataset_noise_inv(cmbl_dataset* ds, const void* in_harmonic, void* out_harmonic, int nbatch);
int cmbl_dataset_set_data(cmbl_dataset* ds, const void* d_harmonic, int nbatch);
/* sum of the three logdet terms of logpdf (logdet Cf + logdet Cphi + logdet Cn), per batch identical */
int cmbl_dataset_set_logdet(cmbl_dataset* ds, double logdet_sum);

/* gradientf_logpdf (src/dataset.jl:76-80): f, out HARMONIC; d = NULL uses ds.d; use_zero_d != 0 uses d = 0 */
int cmbl_gradientf_logpdf(cmbl_dataset* ds, cmbl_flow* L, const void* f, const void* d, int use_zero_d,
                          void* out, int nbatch);
/* argmaxf_logpdf (src/maximization.jl:17-42) by conjugate_gradient (src/numerical_algorithms.jl:73-134):
 * fstart may be NULL; res_hist_host has room for maxit*nbatch doubles; *nit_host = history length. */
int cmbl_wiener_cg(cmbl_dataset* ds, cmbl_flow* L, const void* d, const void* fstart, double tol, int maxit,
                   void* f_out, double* res_hist_host, int* nit_host, int nbatch);
/* ---- any lensing operator in the L slot of a data set (load_sim(L = ...), src/dataset.jl:223, 306, 333; src/bilinearlens.jl:10-17) --------
 * A cmbl_lensop is a typed, NON-OWNING view of an operator handle: destroying the view leaves the operator untouched, and the operator must
 * outlive its views (cmbl_lensop_identity is the exception: there is no operator handle behind it).  The operator and the data set must live on the same context (CMBL_ERR_ARG).  What the reference does not define for an
 * operator is refused with CMBL_ERR_ARG and a message, never approximated: the adjoint of a Taylens (so cmbl_gradientf_logpdf_op /
 * cmbl_wiener_cg_op with it, src/taylens.jl:51), the pullback with respect to phi of a PowerLens / Taylens (gphi_out, src/powerlens.jl).
 * Through a view of a LenseFlow the first two calls run the very code of cmbl_gradientf_logpdf / cmbl_wiener_cg, bit for bit.
 * cmbl_hmc_step, cmbl_map_joint_step and cmbl_*logpdf_mixed stay with cmbl_flow*: src/bilinearlens.jl has no pullback of L \ f. */
int cmbl_lensop_from_lenseflow(cmbl_flow* L, cmbl_lensop** out);
int cmbl_lensop_from_bilinear(cmbl_bilinear* L, cmbl_lensop** out);
int cmbl_lensop_from_powerlens(cmbl_powerlens* L, cmbl_lensop** out);
/* The identity for the L slot: `L = lensed_data ? LenseFlow : I` of load_nolensing_sim (src/dataset.jl:341-352), the operator of NoLensingDataSet,
 * d = M B f + n (src/dataset.jl:37-47, 68-73).  The one view that owns what is behind it; cmbl_lensop_destroy frees it.  It has no phi (a phi handed
 * to cmbl_grad_logpdf_op is ignored by the operator) and no pullback with respect to one: cmbl_grad_logpdf_op with a gphi_out is CMBL_ERR_ARG.
 * cmbl_gradientf_logpdf_op and cmbl_wiener_cg_op take it as any other view; on power-of-two maps with the option "fused_harm" and a
 * Fourier-diagonal noise operator they run without any flow (csrc/kernels_harm.hpp PwNlAp / PwNlDiag): per CG iteration 7 launches with a
 * pixel mask and 3 without; otherwise the composition around device copies. */
int cmbl_lensop_identity(cmbl_ctx* ctx, cmbl_lensop** out);
int cmbl_lensop_destroy(cmbl_lensop* op);            /* the operator itself is untouched */
/* gradientf_logpdf (src/dataset.jl:76-80) and argmaxf_logpdf (src/maximization.jl:17-42): layouts and semantics of cmbl_gradientf_logpdf /
 * cmbl_wiener_cg.  The operator is used as it was last set (set_phi / set_deflection); CMBL_ERR_STATE before either. */
int cmbl_gradientf_logpdf_op(cmbl_dataset* ds, cmbl_lensop* L, const void* f, const void* d, int use_zero_d, void* out, int nbatch);
int cmbl_wiener_cg_op(cmbl_dataset* ds, cmbl_lensop* L, const void* d, const void* fstart, double tol, int maxit,
                      void* f_out, double* res_hist_host, int* nit_host, int nbatch);
/* logpdf(ds; f, phi) (src/dataset.jl:59-66) per batch slot to lp_host, and where asked for its gradient with respect to f (gf_out, HARMONIC) and
 * phi (gphi_out, FOURIER, nbatch planes) at once: the phi part is the pullback of L*f (src/flowops.jl:40-54, src/bilinearlens.jl:165-171)
 * applied to B'M'Cn^-1 (d - M B L f), minus Cphi^-1 phi -- gradient(phi -> logpdf(ds; f, phi), phi) of MAP_marg (src/maximization.jl:307).
 * Sets the operator's phi from `phi` (FOURIER, one plane).  f HARMONIC; d = NULL uses ds.d; gf_out and gphi_out may each be NULL.
 * alias_quirk is read by the LenseFlow view only.  Synchronises the context's stream. */
int cmbl_grad_logpdf_op(cmbl_dataset* ds, cmbl_lensop* L, const void* f, const void* phi, const void* d,
                        double* lp_host, void* gf_out, void* gphi_out, int nbatch, int alias_quirk);

/* logpdf(ds; f) of a NoLensingDataSet (src/dataset.jl:68-73, src/distributions.jl:11-15) per batch slot to lp_host:
 *   -1/2 [ f'Cf^-1 f + (M B f - d)'Cn^-1 (M B f - d) + logdet_sum ],   logdet_sum (cmbl_dataset_set_logdet) = logdet Cf + logdet Cn here,
 * and with gf_out != NULL its gradient gradientf_logpdf = B'M'Cn^-1 (d - M B f) - Cf^-1 f (src/dataset.jl:76-80) from the same pass.  f, gf_out
 * HARMONIC; d = NULL uses ds.d.  Reads CMBL_OP_CF_INV, the noise operator, CMBL_OP_B, CMBL_OP_MF and CMBL_OP_MPIX alone: the operators of phi and
 * of the mixing need not be set.  Any map size.  Synchronises the context's stream. */
int cmbl_nolensing_logpdf(cmbl_dataset* ds, const void* f, const void* d, double* lp_host, void* gf_out /*NULL: value only*/, int nbatch);

/* logpdf(Mixed(ds); f°, phi°) and its gradient (src/dataset.jl:84-117, src/maximization.jl:178):
 * fo MAP, phio FOURIER; gfo MAP, gphio FOURIER.  L's phi is overwritten with G \ phi°. */
int cmbl_logpdf_mixed(cmbl_dataset* ds, cmbl_flow* L, const void* fo, const void* phio, double* lp_host, int nbatch);
int cmbl_grad_logpdf_mixed(cmbl_dataset* ds, cmbl_flow* L, const void* fo, const void* phio, double* lp_host,
                           void* gfo, void* gphio, int nbatch, int alias_quirk);

/* ---- the θ layer on the device: the ParamDependentOps of load_sim (src/dataset.jl:272-274, 316-328) and logpdf(Mixed(ds); f°, phi°, θ) (:84-87,
 *      src/generic.jl:264-271) over a grid of θ -- the inner loop of gibbs_sample_slice_θ! (src/sampling.jl:427-437).  θ = (r, Aphi, bandpower amplitudes):
 *        Cf(θ) = Cfs(amplitudes) + (r / r0) Cten,   Cphi(Aphi) = Cphi0 Aphi / Aphi0,   D(r) = sqrt((C + 2 Cn^ + σ²len) pinv(C)) with C = Cfs + (r / r0) Cten
 *        (the amplitudes enter Cf, not D),   G(Aphi) = pinv(g0) sqrt(1 + 2 Nphi pinv(Cphi(Aphi))),  g0 the same root at Aphi0.
 *      The definition of every formula is the host algebra of the Python layer (theta._ops, sim.HarmOp): the 2 x 2 TE block of an IQU data set reads its ET
 *      plane for both off-diagonals, `+ scalar` touches TT, EE and BB, pinv is 1 / x with every non-finite result replaced by 0, logdet is
 *      Σ λ log|x| over the half plane with non-finite terms skipped.  All arithmetic is double in either precision, no product is fused into a sum or
 *      difference (pinv is discontinuous at a determinant that is exactly 0), and only the store of an operator plane rounds.
 *   cmbl_dataset_theta_model: installs, once per data set, what the operators are made of.  Every pointer is a HOST pointer to doubles in the reference
 *      layout, real (Ny/2+1, Nx) planes, and is copied (as cmbl_clbins_create copies its weights); a second call replaces the first.
 *      Cfs_host, Cten_host, Cn_host: scalar and tensor signal covariance and the Fourier-diagonal noise Cn^, `nplanes` = npol planes each (5 for IQU: TT, TE,
 *      ET, EE, BB); another count is CMBL_ERR_SHAPE.  C0_host (NULL without bands): the base covariance the bandpower amplitudes rescale (it replaces Cfs
 *      inside Cf, not inside D).  nbands in [0, 3]; per band k: band_planes_host[k] a bit mask of the planes of C0 it rescales (bit p = plane p; BB of the
 *      block form is never rescaled), band_idx_host + k * plane the bin index of every mode (int32, decided by the caller; the value band_nbins_host[k]
 *      names the constant amplitude 1 of modes outside the edges; anything outside [0, nbins] is CMBL_ERR_ARG), band_nbins_host[k] its number of bins.
 *      Cphi0_host, Nphi_host: one plane each; G_host: a fixed G plane or NULL -- with it G is that plane at every θ and logdet G is 0 (`if G == nothing`, :317).
 *      logdet_Cn: the constant third term of logdet_sum (also what a data set with CMBL_OP_CN_INV_PIX uses: Σ log V).  D(r0) and g0 are derived here.
 *   cmbl_logpdf_mixed_theta: lp_host[i * nbatch + b] = logpdf(Mixed(ds); f°_b, phi°_b, θ_i), i < ntheta; fo, phio as for cmbl_logpdf_mixed.  r_host[i] / Aphi_host[i]:
 *      NaN means "not named in θ_i": the operators stay fiducial and the parameter's term of the mixing log-determinant is exactly 0; with Aphi not named,
 *      or with a fixed G, G is 1 (or the fixed plane).  amps_host: ntheta rows of namps doubles, the amplitude vectors of the bands concatenated in
 *      the order of the install, or NULL with namps = 0 (all ones); another namps than the model's Σ nbins is CMBL_ERR_SHAPE.  Per θ: one pointwise pass
 *      writes pinv(Cf), pinv(D), pinv(Cphi), pinv(G) into scratch sets owned by the data set and reduces logdet Cf + logdet Cphi, logdet(D(r0)^-1 D) and
 *      logdet G in double (two stages, fixed order, no atomics: bit-identical between runs); CMBL_OP_CF_INV, _D_INV, _CPHI_INV, _G_INV and logdet_sum of
 *      the data set point at them while cmbl_logpdf_mixed's own code runs (whichever path the context takes), and the two mixing log-determinants are
 *      subtracted.  The data set is put back as it was on every way out, an error included.  Only scalars cross to the host per θ; nothing is allocated
 *      after the first call.  A NaN logpdf is a value, not an error.  Before any cmbl_dataset_theta_model: CMBL_ERR_STATE.  L's phi is overwritten.
 *   cmbl_dataset_theta_ops: a TESTING AID.  Evaluates the pass at one θ and copies the scratch set `which` (CMBL_OP_CF_INV, _D_INV: npol or 5 planes;
 *      CMBL_OP_CPHI_INV, _G_INV: 1 plane; else CMBL_ERR_ARG) to out_dev (device, the context's precision, reference layout; may be NULL) and the three sums,
 *      in the order above, to sums_host (may be NULL).  The data set's own operators are not touched.  Synchronises. */
int cmbl_dataset_theta_model(cmbl_dataset* ds, const double* Cfs_host, int nplanes, const double* C0_host, int nbands, const int* band_planes_host,
                             const int32_t* band_idx_host, const int* band_nbins_host, const double* Cten_host, const double* Cn_host, double s2len,
                             double r0, const double* Cphi0_host, double Aphi0, const double* Nphi_host, const double* G_host, double logdet_Cn);
int cmbl_logpdf_mixed_theta(cmbl_dataset* ds, cmbl_flow* L, const void* fo, const void* phio, int nbatch, int ntheta, const double* r_host,
                            const double* Aphi_host, const double* amps_host, int namps, double* lp_host);
int cmbl_dataset_theta_ops(cmbl_dataset* ds, double r, double Aphi, const double* amps_host, int namps, int which, void* out_dev, double* sums_host);

/* ---- the θ-gradient on the device: what ∇θ_logLike of the MUSE adapter (ext/CMBLensingMuseInferenceExt.jl:52-54) gets by automatic differentiation of
 *      logpdf(ds; z..., θ, d), and the same for logpdf(Mixed(ds); f°, phi°, θ).  θ, the model and the NaN / NULL conventions are those of
 *      cmbl_logpdf_mixed_theta; a cmbl_dataset_theta_model must have been installed (else CMBL_ERR_STATE).  One pointwise pass per batch slot evaluates the
 *      very formulas of the operator kernel on a value with tangents (forward mode: r, Aphi and one amplitude per band, since a mode lies in one bin per
 *      band), so the derivative is that of the operators as defined: pinv keeps its discontinuity (tangent 0 where the value is replaced by 0), a skipped
 *      log term contributes 0.  The fields are read once in the context's precision, all sums are double, in two stages and a fixed order; the per-bin
 *      sums run over per-band mode lists sorted by bin at install, cut into chunks that never straddle a bin -- no atomics: equal calls give bit-identical
 *      output and a slot's numbers do not depend on the other slots.  The data term does not depend on θ: Cn, the mask and the beam play no part.
 *   grad_host: nbatch rows of 2 + namps doubles, with the namps of THIS call (rows of 2 when amps_host is NULL, whatever bands the model holds):
 *      d/dr, d/dAphi, then the amplitudes of the bands concatenated in install order.  want: a mask of
 *      CMBL_THETA_R, CMBL_THETA_APHI, CMBL_THETA_AMPS; what it leaves out is not computed and written as 0.  The derivative with respect to a parameter that
 *      θ does not name (r or Aphi NaN, amps_host NULL), or an empty mask, is CMBL_ERR_ARG; another namps than the model's Σ nbins (0 with amps_host NULL) is
 *      CMBL_ERR_SHAPE.  Only scalars cross to the host; nothing is allocated after the first call.  Both calls synchronise.
 *   cmbl_grad_theta_logpdf: ∂/∂θ logpdf(ds; f, phi, θ) at fixed fields.  f: HARMONIC (Ny/2+1, Nx, npol, nbatch), phi: FOURIER, one plane per slot.
 *        ∂/∂θ_k = ½ Σ λ [u† (∂Cf/∂θ_k) u / (Ny Nx) − tr(pinv(Cf) ∂Cf/∂θ_k)],  u = pinv(Cf) f,  plus the same with (phi, Cphi) for Aphi.
 *      No lensing operator is involved and the data set's operators are not read.
 *   cmbl_grad_theta_logpdf_mixed: lp_host[b] = logpdf(Mixed(ds); f°_b, phi°_b, θ) (bit for bit what cmbl_logpdf_mixed_theta gives at that θ) and its
 *      θ-gradient; fo, phio as for cmbl_grad_logpdf_mixed, L a LenseFlow.  The operators of θ go to the scratch sets as in cmbl_logpdf_mixed_theta,
 *      cmbl_grad_logpdf_mixed's own code runs on them (whichever path the context takes, alias_quirk off: the true gradient), and with f = D \ (L \ f°),
 *      phi = G \ phi°, ĝ = ∂lp/∂(L \ f°) (copied device-to-device between the two delta flows, only in this call) and gphi° = ∂lp/∂phi°:
 *        d/dr = ∂lp/∂r − ⟨ĝ, (∂D/∂r) f⟩ − ∂/∂r logdet(D(r0)⁻¹ D),   d/dAphi = ∂lp/∂Aphi − ⟨gphi°, (∂lnG/∂Aphi) phi°⟩ − ∂/∂Aphi logdet G   (the last two
 *        vanish with a fixed G),   d/dA = ∂lp/∂A (the amplitudes enter neither D nor G).
 *      For r and Aphi the last two terms are 10³–10⁴ times the result and nearly cancel: the accuracy of the result is that of the terms.
 *      gphi° is the library's, i.e. the RK4 delta flow -- the transpose of the continuous flow, not the derivative of the discrete forward flow; the
 *      two meet as nsteps⁻⁴.  d/dAphi is therefore not exactly the derivative of the lp_host returned with it: with 7 steps the two differ by about
 *      1e-8 of the size of the terms (8e-6 on a result of 1.0 at 32 x 32 QU), as differences of cmbl_logpdf_mixed_theta show; r, the amplitudes and
 *      cmbl_grad_theta_logpdf do not involve gphi° and carry no such term.
 *      The data set is put back as it was on every way out, an error included.  L's phi is overwritten. */
enum { CMBL_THETA_R = 1, CMBL_THETA_APHI = 2, CMBL_THETA_AMPS = 4 };
int cmbl_grad_theta_logpdf(cmbl_dataset* ds, const void* f, const void* phi, int nbatch, double r, double Aphi, const double* amps_host, int namps,
                           int want, double* grad_host);
int cmbl_grad_theta_logpdf_mixed(cmbl_dataset* ds, cmbl_flow* L, const void* fo, const void* phio, int nbatch, double r, double Aphi,
                                 const double* amps_host, int namps, int want, double* lp_host, double* grad_host);

/* ---- loop bodies of the reference's drivers, for hosts that are neither Julia (which keeps src/maximization.jl:116-233 and
 *      src/sampling.jl:388-464 itself on top of the entry points above) nor Python (cmblensing.jl_amd/drivers.py).  Control flow on the
 *      host inside the library, every field operation one of the launches above; both return when their host outputs are final.
 *
 * hmc_step (src/sampling.jl:405-418; leapfrog = symplectic_integrate, :14-46): one HMC update of phi° at fixed f° with
 *   U = logpdf(Mixed(ds)).  mass = Lambda, the real (Ny/2+1, Nx) plane of mass_matrix_phi (:422-425).  The momentum is
 *   p0 = sqrt(Lambda) .* rfft(white_p), white_p a unit white-noise MAP (Ny, Nx, 1, nbatch); white_p == NULL draws it on the device and
 *   log_u_host == NULL draws log(rand()) from the engine's counter-based generator with the stream convention of the Python drivers:
 *   batch slot b uses key seeds_host[b], momentum stream 2 + 16 step, uniform stream 3 + 16 step (a chain is reproducible whatever
 *   GPU or launch geometry runs it).  accept = always_accept || log_u < dH; a NaN dH (diverged trajectory) rejects.
 *   phio_out (FOURIER, may alias phio) = accepted ? proposal : phio, per batch slot. */
int cmbl_hmc_step(cmbl_dataset* ds, cmbl_flow* L, const void* fo, const void* phio, const void* mass, const void* white_p,
                  const double* log_u_host, const uint64_t* seeds_host, uint64_t step, int nleap, double eps, int always_accept,
                  int alias_quirk, int nbatch, void* phio_out, double* dH_host, int* accept_host);
/* MAP_joint loop body (src/maximization.jl:160-206) with G = I as the reference sets it (:146; the dataset's own G is put back on
 *   return): f = argmaxf_logpdf(phi; fstart, cg_tol, cg_maxit) [HARMONIC]; (f°, phi°) = mix(f, phi); g = d logpdf(Mixed) / d phi°;
 *   step direction hinv .* g, hinv the real plane pinv(Cphi^-1 + Nphi^-1) (src/dataset.jl:134-137); alpha = argmin over [0, alpha_max]
 *   of -sum_b logpdf(Mixed; f°, phi° + alpha * step) by Brent's method (abs_tol = alpha_tol, rel_tol = sqrt(eps(T)), a NaN logpdf is
 *   penalised as (alpha / alpha_max) * floatmax(T), :194-199); phi_out = unmix(phi° + alpha * step).  One alpha for all batch slots.
 *   Outputs: f_out HARMONIC (the Wiener-filtered f), phi_out FOURIER, logpdf_host[nbatch] at the new point, *alpha_host,
 *   *ncg_host = CG iterations, *nls_host = logpdf evaluations of the line search. */
int cmbl_map_joint_step(cmbl_dataset* ds, cmbl_flow* L, const void* phi, const void* fstart, const void* hinv, double alpha_max,
                        double alpha_tol, double cg_tol, int cg_maxit, int alias_quirk, int nbatch, void* f_out, void* phi_out,
                        double* logpdf_host, double* alpha_host, int* ncg_host, int* nls_host);
/* quadratic_estimate(ds, which) (src/quadratic_estimate.jl:29-200) on the dataset's data: which = 0 TT, 1 EE, 2 EB (the pairs the
 *   reference implements, :41).  The *_host arguments are real (Ny/2+1, Nx) planes in double precision, one per component the
 *   estimator uses (TT: T; EE: E; EB: E then B): Cf (unlensed), Cftilde (lensed), Cn, and TF = Mf .* B, the Fourier-diagonal
 *   approximations of mask x beam and noise the reference uses (`ds.M̂`, `ds.B̂`, `ds.Cn̂`), plus Cphi.  AL_in_host != NULL skips the
 *   normalisation sums and uses that plane (:38).  Outputs: phiqe_out FOURIER (Ny/2+1, Nx, 1, nbatch) = (wiener_filtered ?
 *   Cphi/(Cphi+AL) : 1) .* AL .* unnormalised estimate; AL_out_host (may be NULL) the normalisation = N0 bias plane.
 *   Every plane argument (inputs and AL_out_host) may be a HOST or a DEVICE pointer (detected with hipPointerGetAttributes): a caller that
 *   keeps the planes of a dataset on the device -- they change only with theta -- pays no transfer per call.  All plane algebra runs on
 *   the device in double precision, rounded once to the working precision, exactly as the host algebra of the reference does. */
int cmbl_quadratic_estimate(cmbl_dataset* ds, int which, const double* Cf_host, const double* Cftilde_host, const double* Cn_host,
                            const double* TF_host, const double* Cphi_host, int wiener_filtered, const double* AL_in_host,
                            void* phiqe_out, double* AL_out_host, int nbatch);

/* ---- HEALPix <-> Cartesian projection (src/proj_healpix.jl): project(healpix_field => cart_proj) and project(cart_field => ProjHealpix(Nside)),
 *      method = :bilinear.  RING ordering; pixel indices are 0-based here (the reference's k - 1).  HEALPix fields are (npix, npol, nbatch)
 *      arrays of the context's dtype, npix = 12 Nside^2 fastest: the reference's (npix, npol) plus the batch axis.  npol = 1 (I), 2 (QU),
 *      3 (IQU); QU are rotated by the angle psi between the two coordinate bases ("polarization flattening", :238-252, 327-341).
 *      ALL geometry is double on the device whatever the context's dtype (the reference computes it in T); values, weights and
 *      cos 2 psi / sin 2 psi are of the context's dtype.  NOT here: NEST ordering.
 *
 *      The METHOD belongs to the projector (the reference's Projector{method}); cmbl_project_to_cart / _to_healpix dispatch on it.
 *      CMBL_PROJECT_BILINEAR is described below.  CMBL_PROJECT_NFFT is method = :fft (:229-236, 314-325), a non-uniform FFT: with
 *      I_N = {-N/2 ... N/2-1}, K(x) = sum_{l in I_Ny x I_Nx} cos 2 pi l.x, grid nodes x_g = ((i - Ny/2 - 1)/Ny, (j - Nx/2 - 1)/Nx) and the same
 *      formula at the fractional (i_p, j_p) of the Npatch pixels of hpx_idxs_in_patch,
 *        project_to_healpix  h_p = 1/(Ny Nx) sum_g m_g K(x_g - x_p) on the patch, exactly 0 elsewhere,
 *        project_to_cart     m_g = 1/Npatch sum_p h_p K(x_p - x_g),
 *      transposes of each other up to Ny Nx / Npatch, with the same QU rotations as the bilinear method.  Computed through an oversampled
 *      grid (sigma = 2) and a window of cmbl_projector_method's `window_width` cells per axis (8 in float32, 14 in float64), to the rounding
 *      floor of the dtype; bit-identical between runs.  Ny, Nx must be even, hold one window on the fine grid (2N >= width)
 *      and be at most 2048, else CMBL_ERR_SHAPE; a patch without a HEALPix pixel centre is CMBL_ERR_ARG.
 *
 * healpix_pix2ang_host: pix2angRing of the pixels first ... first + n - 1 (host, double, no device).
 * projector_create: Projector(ProjHealpix(nside) => cart_proj) (:254-294) for the Cartesian projection of `ctx` (its Ny, Nx).  cart_kind
 *   CMBL_PROJ_LAMBERT: params = rotator[3] in degrees (RotZYX, the reference's default is (0, 90, 0)), pixel size the context's;
 *   CMBL_PROJ_EQUIRECT: params = theta_span[2], phi_span[2] in radians.  Nside: a power of two in 1 ... 8192, else CMBL_ERR_SHAPE.  A
 *   Cartesian pixel whose colatitude is outside [0, pi] is CMBL_ERR_ARG (healpy.get_interp_val refuses it).  Synchronises.
 * projector_create_method: the same with the method named; projector_create means CMBL_PROJECT_BILINEAR.  Another method number is CMBL_ERR_ARG.
 * projector_method: the projector's method and the window width in use (0 for CMBL_PROJECT_BILINEAR).
 * projector_info_host: doubles.  CMBL_PROJ_COUNTS: n = 2, {pixels in the patch, touched pixels}.  _THETA, _PHI, _PSI_CART: n = Ny Nx, at
 *   the Cartesian pixel centres, Ny fastest.  _IDX_IN_PATCH: hpx_idxs_in_patch (1 <= i <= Ny, 1 <= j <= Nx, :270), ascending.  _IDX_TOUCHED,
 *   _I, _J, _PSI_HPX: the pixels with 0 < i < Ny+1, 0 < j < Nx+1 (every other pixel of a projection to the sphere is exactly 0), ascending,
 *   their fractional (i, j) (1-based like the reference's) and psi.
 * project_to_cart: hpx (npix, npol, nbatch) -> map_out MAP (Ny, Nx, npol, nbatch): healpy.get_interp_val at the pixel centres.
 * project_to_healpix: `in` in basis_in (converted to MAP first; a ProjEquiRect context takes MAP only) -> hpx_out (npix, npol, nbatch):
 *   Images.bilinear_interpolation, a corner outside the map counts as zero.  Neither call synchronises.
 *
 * The transposes (pullbacks) of the two calls, for either method (the call dispatches on the projector's).  Maps are MAP basis,
 * (Ny, Nx, npol, nbatch); HEALPix arrays (npix, npol, nbatch); both of the context's dtype.  With c, s = cos 2 psi, sin 2 psi at the pixel named,
 * Rc: Q' = Q c - U s, U' = U c + Q s (:243-244) and Rh: Q' = Q c + U s, U' = U c - Q s (:332-333) acting on the last two planes when
 * npol >= 2 (Rc^T has the form of Rh and Rh^T that of Rc, each at its own psi):
 *   bilinear, project_to_cart (m[c] = Rc(psi_c) sum_k w[c][k] h[pix[c][k]]):
 *     project_to_cart_adjoint     hbar[p] = sum_{(c, k): pix[c][k] = p} w[c][k] (Rc(psi_c)^T mbar[c]); exactly 0 at a pixel no Cartesian pixel
 *                                 reads; duplicates in pix[c][.] (polar caps) are separate entries and are summed.
 *   bilinear, project_to_healpix (h[p_t] = Rh(psi_t) sum_corners v[t][k] m[c_tk] over the touched pixels, corners outside the map dropped):
 *     project_to_healpix_adjoint  mbar[c] = sum_{(t, k): c_tk = c} v[t][k] (Rh(psi_t)^T hbar[p_t]); every map pixel is written, one without
 *                                 entries gets 0; cotangent values at untouched pixels are ignored (the forward is constant 0 there).
 *   nfft:
 *     project_to_healpix_adjoint  mbar_g = 1/(Ny Nx) sum_{p in patch} K(x_p - x_g) (Rh(psi_p)^T hbar)_p
 *     project_to_cart_adjoint     hbar_p = 1/Npatch sum_g K(x_g - x_p) (Rc(psi_g)^T mbar)_g on hpx_idxs_in_patch, exactly 0 elsewhere.
 * The bilinear rows are summed by ascending input pixel, then corner, in the context's dtype with one fma per entry and no atomics: results
 * are bit-identical between runs.  The transposed tables are built on the first adjoint call of each direction (that call synchronises once)
 * and cached in the projector; after that neither call synchronises.  The input is never modified.  npol outside 1 ... 3 or nbatch < 1 is
 * CMBL_ERR_SHAPE, as for the forward calls. */
typedef struct cmbl_projector cmbl_projector;
enum { CMBL_PROJ_LAMBERT = 0, CMBL_PROJ_EQUIRECT = 1 };
enum { CMBL_PROJECT_BILINEAR = 0, CMBL_PROJECT_NFFT = 1 };
enum { CMBL_PROJ_COUNTS = 0, CMBL_PROJ_THETA = 1, CMBL_PROJ_PHI = 2, CMBL_PROJ_PSI_CART = 3, CMBL_PROJ_IDX_IN_PATCH = 4, CMBL_PROJ_IDX_TOUCHED = 5,
       CMBL_PROJ_I = 6, CMBL_PROJ_J = 7, CMBL_PROJ_PSI_HPX = 8 };
int cmbl_healpix_pix2ang_host(int nside, long first, long n, double* theta, double* phi);
int cmbl_projector_create(cmbl_ctx* ctx, int nside, int cart_kind, const double* params, cmbl_projector** out);
int cmbl_projector_create_method(cmbl_ctx* ctx, int nside, int cart_kind, const double* params, int method, cmbl_projector** out);
int cmbl_projector_destroy(cmbl_projector* P);
int cmbl_projector_method(cmbl_projector* P, int* method, int* window_width);
int cmbl_projector_info_host(cmbl_projector* P, int which, double* out_host, size_t n);
int cmbl_project_to_cart(cmbl_projector* P, const void* hpx, void* map_out, int npol, int nbatch);
int cmbl_project_to_healpix(cmbl_projector* P, int basis_in, const void* in, void* hpx_out, int npol, int nbatch);
int cmbl_project_to_cart_adjoint(cmbl_projector* P, const void* map_cot, void* hpx_out, int npol, int nbatch);
int cmbl_project_to_healpix_adjoint(cmbl_projector* P, const void* hpx_cot, void* map_out, int npol, int nbatch);

#ifdef __cplusplus
}
#endif
#endif
