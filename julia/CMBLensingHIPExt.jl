# CMBLensingHIPExt.jl -- glue that puts libcmblens_hip.so (MI355X / gfx950) behind CMBLensing.jl's operator surface.
#
# STATUS: written against CMBLensing.jl v0.10.1 by reading its sources; **never executed** -- no Julia runtime exists in the build
# image or on the GPU boxes.  What IS executed is the same set of C entry points through the Python mirror
# (cmblensing.jl_amd/, ctypes) and through the plain-C callers tests/c_abi/*.c.  Citations are file:line of the reference.
# julia/test_hipext.jl (also unexecuted) is the first thing to run on a machine that has Julia + AMDGPU.jl (it compares every binding below with the
# reference's own CPU path); julia/make_reference_fixtures.jl needs no GPU at all.
#
# What plugs in where
#   1. storage level, the twin of ext/CMBLensingCUDAExt.jl:42-93 for `ROCArray`: `gpu`, `is_gpu_backed`, `Cℓ_to_2D`, `pinv` / `inv`
#      of Diagonals, `fill!`, `sum`, CPU-RNG `randn!` into device memory, `unsafe_free!`.  With these alone the
#      reference runs on the GPU through AMDGPU.jl broadcasts + rocFFT plans (AbstractFFTs dispatches on the array type,
#      src/util_fft.jl:32-35); everything below replaces the hot path on top.
#   2. `HIPLenseFlow <: FlowOpWithAdjoint` takes the `ds.L` operator slot (src/dataset.jl:55, `load_sim(L = HIPLenseFlow)`):
#      `L(ϕ)*f`, `L(ϕ)\f`, `L(ϕ)'*g`, `L(ϕ)'\g` (src/flowops.jl:11-14) and the two Zygote pullbacks (src/flowops.jl:40-68) are one
#      `ccall` each.  MAP_joint / MAP_marg / sample_joint / argmaxf_logpdf run unmodified on top (they only use that surface).
#   3. `HIPDataSet` wraps a `BaseDataSet` and overrides the performance hooks `gradientf_logpdf` (src/dataset.jl:76-80) and
#      `argmaxf_logpdf` (src/maximization.jl:17-42, the Wiener-filter CG) with `cmbl_gradientf_logpdf` / `cmbl_wiener_cg`, and the
#      mixed posterior `logpdf(Mixed(ds); f°, ϕ°)` with its gradient (src/dataset.jl:84-87; called by MAP_joint at
#      src/maximization.jl:178,197,205 and by hmc_step through src/sampling.jl:399) with `cmbl_logpdf_mixed` /
#      `cmbl_grad_logpdf_mixed` -- the call bench.py times.  Everything else is forwarded to the wrapped dataset.
# Fields cross the boundary as device pointers of `ROCArray`-backed `.arr` (AMDGPU.jl); layouts are the reference's own
# (Ny, Nx, Npol, Nbatch) column-major arrays (src/proj_cartesian.jl:13-36), so nothing is copied or permuted.  Every array whose
# pointer is passed is rooted with `GC.@preserve` for the duration of the call (calls are stream-ordered: a temporary that is
# only an INPUT of an asynchronous call is additionally kept until `cmbl_ctx_synchronize`, see `keepalive`).
module CMBLensingHIPExt

using CMBLensing, AMDGPU, Adapt, LinearAlgebra, Random, Zygote
using CMBLensing: FlowOpWithAdjoint, ImplicitOp, BaseDataSet, NoLensingDataSet, DataSet, Mixed, Field, BaseField, ProjLambert, Map, Fourier, EBFourier, IEBFourier,
                  QUFourier, IQUFourier, Ł, Ð, BlockDiagIEB, LazyBinaryOp, FieldTuple, batch_length, batch, unbatch, nan2zero, diag
import CMBLensing: precompute!!, getϕ, gradientf_logpdf, argmaxf_logpdf, logpdf
import Base: *, \, adjoint

const lib = get(ENV, "CMBL_LIB", joinpath(@__DIR__, "..", "cmblensing.jl_amd", "libcmblens_hip.so"))

# DEFAULT ARITHMETIC OF THIS GLUE = THE REFERENCE'S, AS WRITTEN: the δϕ velocity with the in-place aliasing of src/lenseflow.jl:198-200 and
# plain sums in the working precision (`sum_accuracy_mode = nothing`, src/util.jl:288-316) -- a user who swaps `LenseFlow` for
# `HIPLenseFlow` gets the reference's numbers, not the library's "consistent" variant (DESIGN.md §3 Q1: that one matches finite differences
# to 2e-8 and differs from the reference by ~3e-4 in the ϕ gradient).  The consistent form stays a keyword (`alias_quirk=false`), Float64 /
# Kahan accumulation a call (`set_sum_accuracy_mode!`); CMBL_CONSISTENT=1 makes both the default of a session.
reference_exact() = get(ENV, "CMBL_CONSISTENT", "0") in ("", "0")

# ---- status codes -> exceptions (include/cmblens.h: nothing throws across the ABI) ---------------------------------------
chk(rc::Integer) = rc == 0 ? nothing : error("libcmblens_hip error $rc: ", unsafe_string(ccall((:cmbl_last_error, lib), Cstring, ())))
const CMBL_ABI_VERSION = 3          # include/cmblens.h: the revision these ccall signatures were written against
function __init__()
    # CMBL_REFERENCE_EXACT (the switch of the Python host and of earlier revisions of this glue) stays an accepted alias: =0 means CMBL_CONSISTENT=1
    if haskey(ENV, "CMBL_REFERENCE_EXACT") && !haskey(ENV, "CMBL_CONSISTENT")
        ENV["CMBL_CONSISTENT"] = ENV["CMBL_REFERENCE_EXACT"] in ("", "0") ? "1" : "0"
    end
    v = ccall((:cmbl_abi_version, lib), Cint, ())
    v == CMBL_ABI_VERSION || error("libcmblens_hip.so has ABI version $v, this extension binds version $CMBL_ABI_VERSION: rebuild one of them")
end

const MAP, FOURIER, HARMONIC = Cint(0), Cint(1), Cint(2)                  # CMBL_MAP / CMBL_FOURIER / CMBL_HARMONIC
const FLOW_FWD, FLOW_INV, FLOW_ADJ, FLOW_INVADJ = Cint(0), Cint(1), Cint(2), Cint(3)
dtype(::Type{Float32}) = Cint(0)
dtype(::Type{Float64}) = Cint(1)

const ROCBaseField{B,M,T,A<:ROCArray} = BaseField{B,M,T,A}
devptr(a::ROCArray) = Ptr{Cvoid}(UInt(pointer(a)))
npol(f::BaseField) = size(f.arr, 3)
nbatch(f::BaseField) = size(f.arr, 4)

# the library's basis tag of a field: Map-like, QU/IQU-Fourier ("FOURIER") or EB/IEB-Fourier ("HARMONIC"); spin-0 Fourier is both
basis_tag(::BaseField{B}) where {B<:CMBLensing.SpatialBasis{Map}} = MAP
basis_tag(::BaseField{B}) where {B<:Union{Fourier,QUFourier,IQUFourier}} = FOURIER
basis_tag(::BaseField{B}) where {B<:Union{EBFourier,IEBFourier}} = HARMONIC
# the basis covariances are diagonal in.  NB `CMBLensing.HarmonicBasis(f)` keeps the pol basis (QU stays QU, src/generic.jl:94-98),
# so the conversion is spelled out here
harm(f::BaseField) = npol(f) == 1 ? Fourier(f) : npol(f) == 2 ? EBFourier(f) : IEBFourier(f)

# ---- 1. storage-level twins of ext/CMBLensingCUDAExt.jl:42-93 --------------------------------------------------------------
CMBLensing.is_gpu_backed(::ROCBaseField) = true                                                   # :42
CMBLensing.gpu(x) = Adapt.adapt_structure(ROCArray, x)                                            # :43
function CMBLensing.Cℓ_to_2D(Cℓ, proj::ProjLambert{T,<:ROCArray}) where {T}                       # :46-49 (through the CPU, like upstream)
    CMBLensing.gpu(T.(nan2zero.(Cℓ.(CMBLensing.cpu(proj.ℓmag)))))
end
LinearAlgebra.pinv(D::Diagonal{T,<:ROCBaseField}) where {T} = Diagonal(@. ifelse(isfinite(inv(D.diag)), inv(D.diag), $zero(T)))   # :55
LinearAlgebra.inv(D::Diagonal{T,<:ROCBaseField}) where {T} =
    any(Array((D.diag .== 0)[:])) ? throw(SingularException(-1)) : Diagonal(inv.(D.diag))        # :56
Base.fill!(f::ROCBaseField, x) = (fill!(f.arr, x); f)                                             # :57
Base.sum(f::ROCBaseField; dims=:) =
    (dims == :) ? CMBLensing.sum_dropdims(f.arr) : (1 in dims) ? error("Sum over invalid dims of a flat field.") : f      # :58
Random.randn!(rng::MersenneTwister, A::ROCArray) = (A .= adapt(ROCArray, randn!(rng, adapt(Array, A))))   # :72-73 host RNG + upload (upstream's own "minor type-piracy", kept: `simulate` with the CPU generator needs it)
CMBLensing.unsafe_free!(x::ROCArray) = AMDGPU.unsafe_free!(x)                                     # :88
# (:91-93, `dot(x::CuArray, y::CuArray) = sum(conj.(x) .* y)`, works around a CUDA.jl / Zygote issue and has no twin here: AMDGPU.jl's own
# `dot` is left alone -- redefining it for two ROCArrays would be type piracy on a package this module does not own)

# ---- context: replaces the memoized ProjLambert + FFT plans (src/proj_lambert.jl:48-75, src/util_fft.jl:32-39) ----------------
mutable struct HIPContext
    h    :: Ptr{Cvoid}
    keep :: Vector{Any}              # inputs of calls that are still in flight on the stream (see `keepalive`)
    function HIPContext(proj::ProjLambert{T}) where {T}
        h = Ref{Ptr{Cvoid}}()
        # AMDGPU.jl: `AMDGPU.stream()` is the task-local HIPStream, `.stream` its hipStream_t; `AMDGPU.device_id` is 1-based
        chk(ccall((:cmbl_ctx_create, lib), Cint, (Cint, Cint, Cdouble, Cint, Cint, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}),
                  proj.Ny, proj.Nx, proj.θpix, dtype(real(T)), AMDGPU.device_id(AMDGPU.device()) - 1,
                  Ptr{Cvoid}(UInt(Base.unsafe_convert(Ptr{Cvoid}, AMDGPU.stream().stream))), h))
        # the library's own default accumulates in Float64; the reference's is the working precision (src/util.jl:288-316)
        reference_exact() && chk(ccall((:cmbl_set_sum_accuracy_mode, lib), Cint, (Ptr{Cvoid}, Cint), h[], 0))
        finalizer(c -> ccall((:cmbl_ctx_destroy, lib), Cint, (Ptr{Cvoid},), c.h), new(h[], Any[]))
    end
    # a ProjEquiRect (src/proj_equirect.jl:25-58) takes the same context: sizes, precision, stream and scratch; its pixel size is not used
    function HIPContext(proj::CMBLensing.ProjEquiRect{T}) where {T}
        h = Ref{Ptr{Cvoid}}()
        chk(ccall((:cmbl_ctx_create, lib), Cint, (Cint, Cint, Cdouble, Cint, Cint, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}),
                  proj.Ny, proj.Nx, 1.0, dtype(real(T)), AMDGPU.device_id(AMDGPU.device()) - 1,
                  Ptr{Cvoid}(UInt(Base.unsafe_convert(Ptr{Cvoid}, AMDGPU.stream().stream))), h))
        finalizer(c -> ccall((:cmbl_ctx_destroy, lib), Cint, (Ptr{Cvoid},), c.h), new(h[], Any[]))
    end
end
const contexts = IdDict{Any,HIPContext}()                                 # one per (memoized, hence ===) ProjLambert
hip_ctx(proj::ProjLambert) = get!(() -> HIPContext(proj), contexts, proj)
hip_ctx(proj::CMBLensing.ProjEquiRect) = get!(() -> HIPContext(proj), contexts, proj)
hip_ctx(f::BaseField) = hip_ctx(f.metadata)
synchronize(ctx::HIPContext) = (chk(ccall((:cmbl_ctx_synchronize, lib), Cint, (Ptr{Cvoid},), ctx.h)); empty!(ctx.keep); nothing)
# a temporary that is only read by an asynchronous call must outlive the call, not just the `ccall`: park it on the context; the
# list is dropped at the next synchronisation (every entry point that returns host values synchronises)
keepalive(ctx::HIPContext, xs...) = (append!(ctx.keep, xs); length(ctx.keep) > 256 && synchronize(ctx); nothing)

# ---- 2. the LenseFlow operator -------------------------------------------------------------------------------------------
# same abstract parent as LenseFlow (src/lenseflow.jl:2,19-31); `nsteps` RK4 steps, t: 0 -> 1
mutable struct HIPLenseFlow{T} <: FlowOpWithAdjoint{T}
    ϕ      :: Union{Nothing,Field}
    nsteps :: Int
    ctx    :: Union{Nothing,HIPContext}
    h      :: Ptr{Cvoid}
    cached :: Any                       # the ϕ object the device cache was built from (src/lenseflow.jl:123-129)
    alias_quirk :: Bool                 # true = the δϕ velocity exactly as written upstream (src/lenseflow.jl:198-200 aliasing)
end
HIPLenseFlow(nsteps::Int=7; alias_quirk=reference_exact()) = ϕ -> HIPLenseFlow(ϕ, nsteps; alias_quirk)
function HIPLenseFlow(ϕ::Field, nsteps::Int=7; alias_quirk=reference_exact())
    T = real(eltype(ϕ))
    ctx = hip_ctx(ϕ.metadata)
    h = Ref{Ptr{Cvoid}}()
    chk(ccall((:cmbl_lenseflow_create, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}), ctx.h, nsteps, h))
    L = HIPLenseFlow{T}(ϕ, nsteps, ctx, h[], nothing, alias_quirk)
    finalizer(L -> ccall((:cmbl_lenseflow_destroy, lib), Cint, (Ptr{Cvoid},), L.h), L)
end
getϕ(L::HIPLenseFlow) = L.ϕ
(L::HIPLenseFlow)(ϕ::Field) = (L.ϕ === ϕ) ? L : (L.ϕ = ϕ; L)              # `L(ϕ)`: re-points the operator, cache rebuilt lazily

# precompute!! (src/lenseflow.jl:80-142).  ϕ is handed over in the basis it arrives in -- `gradhess(ϕ)` differentiates a Fourier ϕ
# WITHOUT projecting it through a map first (src/specialops.jl:184-188, src/lenseflow.jl:135), and a ϕ produced by a gradient step
# has ky = 0 / Nyquist rows that no real map produces; `Map(ϕ)` here would change the next MAP step by 2e-5 (DESIGN.md §3).
function precompute!!(L::HIPLenseFlow, f)
    if L.cached !== L.ϕ
        ϕ = L.ϕ
        ϕ′ = (basis_tag(ϕ) == MAP) ? ϕ : Fourier(ϕ)
        a = ϕ′.arr
        GC.@preserve a chk(ccall((:cmbl_lenseflow_set_phi, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint),
                                 L.h, basis_tag(ϕ′), devptr(a), nbatch(ϕ′)))
        keepalive(L.ctx, a)
        L.cached = ϕ
    end
    L
end

function flow(L::HIPLenseFlow, mode, f::BaseField, out::BaseField)
    precompute!!(L, f)
    a, o = f.arr, out.arr
    GC.@preserve a o chk(ccall((:cmbl_lenseflow_apply, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint),
                               L.h, mode, basis_tag(f), devptr(a), basis_tag(out), devptr(o), npol(f), nbatch(f)))
    keepalive(L.ctx, a)
    out
end
# src/flowops.jl:11-14: L*f, L\f act in the LenseBasis (maps), L'*g, L'\g in the DerivBasis (QU-Fourier); the library converts
*(L::HIPLenseFlow, f::Field) = (g = Ł(f); flow(L, FLOW_FWD, g, similar(g)))
\(L::HIPLenseFlow, f::Field) = (g = Ł(f); flow(L, FLOW_INV, g, similar(g)))
*(L::Adjoint{<:Any,<:HIPLenseFlow}, f::Field) = (g = Ð(f); flow(parent(L), FLOW_ADJ, g, similar(g)))
\(L::Adjoint{<:Any,<:HIPLenseFlow}, f::Field) = (g = Ð(f); flow(parent(L), FLOW_INVADJ, g, similar(g)))

# an uninitialised Fourier spin-0 field with the batch length of `like` (for δϕ: (Ny÷2+1, Nx, 1, Nbatch))
function similar_ϕ(ϕ::Field, like::BaseField)
    ϕf = Fourier(ϕ)
    typeof(ϕf)(similar(ϕf.arr, eltype(ϕf.arr), (size(ϕf.arr, 1), size(ϕf.arr, 2), 1, nbatch(like))), ϕf.metadata)
end

# the δ-flow pullback: (δϕ [Fourier S0], δf [same basis as Δ], f_start [Map]) from the primal OUTPUT f_end and the cotangent Δ
function flow_gradient(L::HIPLenseFlow, mode, f_end::BaseField, Δ::BaseField)
    precompute!!(L, f_end)
    δf, fstart, δϕ = similar(Δ), similar(f_end), similar_ϕ(L.ϕ, f_end)
    a, b, c, d, e = f_end.arr, Δ.arr, δϕ.arr, δf.arr, fstart.arr
    GC.@preserve a b c d e chk(ccall((:cmbl_lenseflow_grad, lib), Cint,
              (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint),
              L.h, mode, devptr(a), basis_tag(Δ), devptr(b), devptr(c), basis_tag(δf), devptr(d),
              devptr(e), npol(f_end), nbatch(f_end), L.alias_quirk ? 1 : 0))
    keepalive(L.ctx, a, b)
    δϕ, δf, fstart
end

# the two Zygote adjoints of src/flowops.jl:40-68, including the :AD_constants shortcut (ϕ held constant -> plain adjoint flow)
Zygote.@adjoint function *(Lϕ::HIPLenseFlow, f::Field{B}) where {B}
    f̃ = Lϕ * f
    function back(Δ)
        if :ϕ in get(task_local_storage(), :AD_constants, ())
            nothing, B(Lϕ' * Δ)
        else
            δϕ, δf, _ = flow_gradient(Lϕ, FLOW_FWD, Ł(f̃), Ð(Δ))          # δ-flow t: 1 -> 0 from (f̃, Δ, 0)
            δϕ, B(δf)
        end
    end
    f̃, back
end
Zygote.@adjoint function \(Lϕ::HIPLenseFlow, f̃::Field{B}) where {B}
    f = Lϕ \ f̃
    function back(Δ)
        if :ϕ in get(task_local_storage(), :AD_constants, ())
            nothing, B(Lϕ' \ Δ)
        else
            δϕ, δf, _ = flow_gradient(Lϕ, FLOW_INV, Ł(f), Ð(Δ))           # δ-flow t: 0 -> 1 from (f, Δ, 0)
            δϕ, B(δf)
        end
    end
    f, back
end
# `L(ϕ)` inside a differentiated function: the cotangent of the operator is the cotangent of ϕ (src/flowops.jl:18-19)
Zygote.@adjoint (Lϕ::HIPLenseFlow)(ϕ′) = Lϕ(ϕ′), Δ -> (nothing, Δ)

# ---- 2b. BilinearLens (src/bilinearlens.jl) ------------------------------------------------------------------------------------
# the reference's second lensing operator: one ϕ (a batched ϕ errors like upstream, :40), `*`, `\`, `'` and the pullback of `*`;
# `load_sim(L = HIPBilinearLens)` takes it where upstream takes `BilinearLens`
mutable struct HIPBilinearLens{T} <: ImplicitOp{T}
    ϕ      :: Field
    ctx    :: HIPContext
    h      :: Ptr{Cvoid}
    cached :: Any                       # the ϕ object the device tables were built from
    maxiter :: Int                      # gmres iterations of `\` (:134, 147)
end
function HIPBilinearLens(ϕ::Field; maxiter::Int=5)
    T = real(eltype(ϕ))
    ctx = hip_ctx(ϕ.metadata)
    h = Ref{Ptr{Cvoid}}()
    chk(ccall((:cmbl_bilinear_create, lib), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), ctx.h, h))
    L = HIPBilinearLens{T}(ϕ, ctx, h[], nothing, maxiter)
    finalizer(L -> ccall((:cmbl_bilinear_destroy, lib), Cint, (Ptr{Cvoid},), L.h), L)
end
getϕ(L::HIPBilinearLens) = L.ϕ
(L::HIPBilinearLens)(ϕ::Field) = (L.ϕ === ϕ) ? L : (L.ϕ = ϕ; L)
function precompute!!(L::HIPBilinearLens)
    if L.cached !== L.ϕ
        ϕ′ = (basis_tag(L.ϕ) == MAP) ? L.ϕ : Fourier(L.ϕ)
        a = ϕ′.arr
        GC.@preserve a chk(ccall((:cmbl_bilinear_set_phi, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint),
                                 L.h, basis_tag(ϕ′), devptr(a), nbatch(ϕ′)))
        keepalive(L.ctx, a)
        L.cached = L.ϕ
    end
    L
end
function bilinear(L::HIPBilinearLens, mode, f::BaseField, out::BaseField)
    precompute!!(L)
    a, o = f.arr, out.arr
    GC.@preserve a o chk(ccall((:cmbl_bilinear_apply, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint, Cint),
                               L.h, mode, basis_tag(f), devptr(a), basis_tag(out), devptr(o), npol(f), nbatch(f), L.maxiter))
    keepalive(L.ctx, a)
    out
end
# all four act on and return Ł fields (:107-151)
*(L::HIPBilinearLens, f::Field) = (g = Ł(f); bilinear(L, FLOW_FWD, g, similar(g)))
\(L::HIPBilinearLens, f::Field) = (g = Ł(f); bilinear(L, FLOW_INV, g, similar(g)))
*(L::Adjoint{<:Any,<:HIPBilinearLens}, f::Field) = (g = Ł(f); bilinear(parent(L), FLOW_ADJ, g, similar(g)))
\(L::Adjoint{<:Any,<:HIPBilinearLens}, f::Field) = (g = Ł(f); bilinear(parent(L), FLOW_INVADJ, g, similar(g)))

# :163-171
Zygote.@adjoint HIPBilinearLens(ϕ) = HIPBilinearLens(ϕ), Δ -> (Δ,)
Zygote.@adjoint function *(Lϕ::HIPBilinearLens, f::Field{B}) where {B}
    f̃ = Lϕ * f
    function back(Δ)
        precompute!!(Lϕ)
        Δm = Ł(Δ)
        δf, δϕ = similar(Δm), similar_ϕ(Lϕ.ϕ, f̃)
        a, b, c, d = f̃.arr, Δm.arr, δϕ.arr, δf.arr
        GC.@preserve a b c d chk(ccall((:cmbl_bilinear_grad, lib), Cint,
                  (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint),
                  Lϕ.h, devptr(a), basis_tag(Δm), devptr(b), devptr(c), basis_tag(δf), devptr(d), npol(f̃), nbatch(f̃)))
        keepalive(Lϕ.ctx, a, b)
        δϕ, B(δf)
    end
    f̃, back
end

# ---- 2c. PowerLens and Taylens (src/powerlens.jl, src/taylens.jl) ---------------------------------------------------------------
# lensing by the Taylor series in ∇ϕ up to `order` (0 ... 12): one ϕ, `*` for both and `'` for PowerLens (the reference defines no more);
# the adjoint returns a Fourier field like upstream (src/powerlens.jl:54)
const KIND_POWERLENS, KIND_TAYLENS = Cint(0), Cint(1)
mutable struct HIPTaylorLens{T,K} <: ImplicitOp{T}
    ϕ      :: Field
    order  :: Int
    ctx    :: HIPContext
    h      :: Ptr{Cvoid}
    cached :: Any                       # the ϕ object the device table was built from
end
const HIPPowerLens{T} = HIPTaylorLens{T,KIND_POWERLENS}
const HIPTaylens{T} = HIPTaylorLens{T,KIND_TAYLENS}
function taylorlens(K, ϕ::Field, order::Int)
    T = real(eltype(ϕ))
    ctx = hip_ctx(ϕ.metadata)
    h = Ref{Ptr{Cvoid}}()
    chk(ccall((:cmbl_powerlens_create, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Cvoid}}), ctx.h, order, K, h))
    L = HIPTaylorLens{T,K}(ϕ, order, ctx, h[], nothing)
    finalizer(L -> ccall((:cmbl_powerlens_destroy, lib), Cint, (Ptr{Cvoid},), L.h), L)
end
HIPPowerLens(ϕ::Field, order::Int) = taylorlens(KIND_POWERLENS, ϕ, order)
HIPTaylens(ϕ::Field, order::Int) = taylorlens(KIND_TAYLENS, ϕ, order)
HIPPowerLens(order::Int) = ϕ -> HIPPowerLens(ϕ, order)
HIPTaylens(order::Int) = ϕ -> HIPTaylens(ϕ, order)
getϕ(L::HIPTaylorLens) = L.ϕ
(L::HIPTaylorLens)(ϕ::Field) = (L.ϕ === ϕ) ? L : (L.ϕ = ϕ; L)
# antilensing (src/powerlens.jl:36-38 cannot run as written: `N` is undefined and ∇1ϕᵖ is passed twice): the operator of -ϕ, as its doc string says
antilensing(L::HIPTaylorLens{T,K}) where {T,K} = taylorlens(K, -L.ϕ, L.order)
function precompute!!(L::HIPTaylorLens)
    if L.cached !== L.ϕ
        ϕ′ = (basis_tag(L.ϕ) == MAP) ? L.ϕ : Fourier(L.ϕ)
        a = ϕ′.arr
        GC.@preserve a chk(ccall((:cmbl_powerlens_set_phi, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint),
                                 L.h, basis_tag(ϕ′), devptr(a), nbatch(ϕ′)))
        keepalive(L.ctx, a)
        L.cached = L.ϕ
    end
    L
end
function taylorlens_apply(L::HIPTaylorLens, mode, f::BaseField, out::BaseField)
    precompute!!(L)
    a, o = f.arr, out.arr
    GC.@preserve a o chk(ccall((:cmbl_powerlens_apply, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint),
                               L.h, mode, basis_tag(f), devptr(a), basis_tag(out), devptr(o), npol(f), nbatch(f)))
    keepalive(L.ctx, a)
    out
end
*(L::HIPTaylorLens, f::Field) = (g = Ł(f); taylorlens_apply(L, FLOW_FWD, g, similar(g)))
*(L::Adjoint{<:Any,<:HIPPowerLens}, f::Field) = (g = Ł(f); taylorlens_apply(parent(L), FLOW_ADJ, g, similar(Ð(g))))

# ---- 3. data model, Wiener filter, mixed posterior ------------------------------------------------------------------------
# include/cmblens.h: CMBL_OP_*
const OP_CF_INV, OP_CN_INV, OP_B, OP_MF, OP_D, OP_D_INV, OP_PRECOND_INV, OP_CPHI_INV, OP_G_INV, OP_MPIX = Cint.(0:9)

"""
    HIPDataSet(ds::BaseDataSet)

`ds` evaluated at its current θ with the Fourier-diagonal operators resident in the library: `gradientf_logpdf`, `argmaxf_logpdf`
(the Wiener filter), `logpdf(Mixed(ds); f°, ϕ°)` and its gradient then run entirely inside libcmblens_hip.  `ds.L` must be a
`HIPLenseFlow` (constructor or instance).  The planes handed over are the `diag(...)` arrays of the reference operators in the
harmonic (E/B) basis -- five planes (TT, TE, ET, EE, BB) for a `BlockDiagIEB` -- with `pinv` taken here exactly as
`Hessian_logpdf_preconditioner(:f, ds)` does (src/dataset.jl:129-132).  `hd(θ)` / `copy(hd)` / `hd.G = I` work like on any
`DataSet` (src/dataset.jl:5,12-18; MAP_joint does all three, src/maximization.jl:145-146) and re-upload what changed.
"""
mutable struct HIPDataSet{DS<:BaseDataSet} <: DataSet
    ds :: DS
    h  :: Ptr{Cvoid}
    L  :: HIPLenseFlow
end
Base.getproperty(d::HIPDataSet, k::Symbol) = k in (:ds, :h, :L) ? getfield(d, k) : getproperty(getfield(d, :ds), k)
function Base.setproperty!(d::HIPDataSet, k::Symbol, v)
    k in (:ds, :h, :L) && return setfield!(d, k, v)
    setproperty!(getfield(d, :ds), k, v)
    upload!(d)                                                            # e.g. `dsθ.G = I` (src/maximization.jl:146)
    v
end
Base.copy(d::HIPDataSet) = HIPDataSet(copy(getfield(d, :ds)))
# ds(θ) (src/dataset.jl:12-18): only when some operator of the wrapped dataset actually depends on a key of θ are the operators
# re-evaluated and uploaded (MAP_joint passes θ to every logpdf call of an already evaluated dsθ, src/maximization.jl:178,197,205)
depends_on_θ(d::HIPDataSet, θ) = !isempty(θ) && any(v -> CMBLensing.depends_on(v, θ), CMBLensing.fieldvalues(getfield(d, :ds)))
(d::HIPDataSet)(θ::NamedTuple) = depends_on_θ(d, θ) ? HIPDataSet(getfield(d, :ds)(θ)) : d
(d::HIPDataSet)(; θ...) = d((; θ...))

# real planes of an operator that is diagonal in the harmonic basis, as ONE (Ny÷2+1, Nx, nplanes) device array
op_planes(D::Diagonal{<:Any,<:BaseField}) = real.(harm(D.diag).arr[:, :, :, 1])
op_planes(D::BlockDiagIEB) = cat((real.(diag(X).arr[:, :, 1, 1]) for X in (D.ΣTE[1,1], D.ΣTE[1,2], D.ΣTE[2,1], D.ΣTE[2,2], D.ΣB))...; dims=3)
op_planes(::UniformScaling, like) = fill!(similar(op_planes(like)), 1)    # `G = I`
function set_op!(hd_h, ctx, which, D, like=nothing)
    p = D isa UniformScaling ? op_planes(D, like) : op_planes(D)
    GC.@preserve p chk(ccall((:cmbl_dataset_set_op, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint), hd_h, which, devptr(p), size(p, 3)))
    keepalive(ctx, p)                                                     # the library copies the planes on its stream
end
function upload!(hd::HIPDataSet)
    ds, h = getfield(hd, :ds), getfield(hd, :h)
    ctx = hip_ctx(ds.d.metadata)
    Cf, Cn, Cϕ, D, G = ds.Cf, ds.Cn, ds.Cϕ, ds.D, ds.G                    # already evaluated at θ by ds(θ)
    set_op!(h, ctx, OP_CF_INV, pinv(Cf));  set_op!(h, ctx, OP_CN_INV, pinv(Cn))
    set_op!(h, ctx, OP_B, ds.B);           set_op!(h, ctx, OP_D, D);   set_op!(h, ctx, OP_D_INV, pinv(D))
    set_op!(h, ctx, OP_PRECOND_INV, pinv(pinv(Cf) + ds.B̂' * ds.M̂' * pinv(ds.Cn̂) * ds.M̂ * ds.B̂))
    set_op!(h, ctx, OP_CPHI_INV, pinv(Cϕ)); set_op!(h, ctx, OP_G_INV, G isa UniformScaling ? G : pinv(G), Cϕ)
    # M = Mfourier * Mpix (src/dataset.jl:279-285) is a LazyBinaryOp{*}(X = Mfourier, Y = Mpix) (src/specialops.jl:364-377) or,
    # without a pixel mask, the Fourier-diagonal operator alone
    M = ds.M
    if M isa LazyBinaryOp
        set_op!(h, ctx, OP_MF, M.X)
        m = Map(diag(M.Y)).arr[:, :, 1, 1]                                # the same mask on every pol plane (src/dataset.jl:281)
        GC.@preserve m chk(ccall((:cmbl_dataset_set_op, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint), h, OP_MPIX, devptr(m), 1))
        keepalive(ctx, m)
    else
        set_op!(h, ctx, OP_MF, M)
    end
    d = harm(ds.d)
    a = d.arr
    GC.@preserve a chk(ccall((:cmbl_dataset_set_data, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint), h, devptr(a), nbatch(d)))
    keepalive(ctx, a)
    chk(ccall((:cmbl_dataset_set_logdet, lib), Cint, (Ptr{Cvoid}, Cdouble), h, logdet(Cf) + logdet(Cϕ) + logdet(Cn)))
    hd
end
function HIPDataSet(ds::BaseDataSet)
    ctx = hip_ctx(ds.d.metadata)
    h = Ref{Ptr{Cvoid}}()
    chk(ccall((:cmbl_dataset_create, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}), ctx.h, size(ds.d.arr, 3), h))
    L = ds.L isa HIPLenseFlow ? ds.L : HIPLenseFlow(zero(diag(ds.Cϕ)), 7)
    hd = HIPDataSet(ds, h[], L)
    finalizer(x -> ccall((:cmbl_dataset_destroy, lib), Cint, (Ptr{Cvoid},), getfield(x, :h)), hd)
    upload!(hd)
end

# src/dataset.jl:76-80:  L'B'M'Cn⁻¹(d − M B L f) − Cf⁻¹ f, one library call
function gradientf_logpdf(hd::HIPDataSet; f, ϕ, θ=(;), d=hd.ds.d)
    depends_on_θ(hd, θ) && return gradientf_logpdf(hd(θ); f, ϕ, d)
    L = precompute!!(hd.L(ϕ), f)
    fh, dh = harm(f), harm(d)
    out = similar(fh)
    zero_d = all(iszero, dh.arr) ? 1 : 0
    a, b, o = fh.arr, dh.arr, out.arr
    GC.@preserve a b o chk(ccall((:cmbl_gradientf_logpdf, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint),
                                 hd.h, L.h, devptr(a), devptr(b), zero_d, devptr(o), nbatch(fh)))
    keepalive(L.ctx, a, b)
    out
end

# src/maximization.jl:17-42: the preconditioned CG of src/numerical_algorithms.jl:73-134 with its scalars on the device;
# returns (f, history) like the reference (`history_keys = (:i, :res)`).  `offset=true` (used by sample_f, src/maximization.jl:56-62)
# adds a₀ = gradientf_logpdf(f = 0, d = 0) to b, which is identically 0 for this linear model.
function argmaxf_logpdf(hd::HIPDataSet, Ω::NamedTuple, d=hd.ds.d; fstart=nothing, preconditioner=:diag,
                        conjgrad_kwargs=(tol=1e-1, nsteps=500), offset=false)
    θ = get(Ω, :θ, (;))
    depends_on_θ(hd, θ) && return argmaxf_logpdf(hd(θ), Base.structdiff(Ω, NamedTuple{(:θ,)}), d; fstart, preconditioner, conjgrad_kwargs, offset)
    L = precompute!!(hd.L(Ω.ϕ), d)
    dh = harm(d)
    out = similar(dh)
    nsteps = get(conjgrad_kwargs, :nsteps, 500)
    B = nbatch(dh)
    hist = Vector{Cdouble}(undef, nsteps * B)
    nit = Ref{Cint}(0)
    fs = isnothing(fstart) ? nothing : harm(fstart).arr
    a, o = dh.arr, out.arr
    GC.@preserve a o fs hist chk(ccall((:cmbl_wiener_cg, lib), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cint, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cint}, Cint),
              hd.h, L.h, devptr(a), isnothing(fs) ? C_NULL : devptr(fs), get(conjgrad_kwargs, :tol, 1e-1), nsteps, devptr(o), hist, nit, B))
    history = [(i=i, res=(B == 1 ? hist[i] : batch(hist[(i-1)*B+1:i*B]))) for i in 1:nit[]]
    out, history
end

# ---- NoLensingDataSet (src/dataset.jl:37-47, 68-73): d = M B f + n, the identity in the L slot (cmbl_lensop_identity) --------------------
"""
    HIPNoLensingDataSet(ds::NoLensingDataSet)

`ds` at its current θ with its Fourier-diagonal operators resident in the library: `gradientf_logpdf`, `argmaxf_logpdf(I, ...)` (the
Wiener filter; `MAP_joint(θ, ds)` is it, src/maximization.jl:235) and `logpdf` run inside libcmblens_hip, on power-of-two maps without
any flow.  Nothing about ϕ is uploaded.
"""
mutable struct HIPNoLensingDataSet{DS<:NoLensingDataSet} <: DataSet
    ds :: DS
    h  :: Ptr{Cvoid}
    id :: Ptr{Cvoid}                                                      # the cmbl_lensop of the identity
end
Base.getproperty(d::HIPNoLensingDataSet, k::Symbol) = k in (:ds, :h, :id) ? getfield(d, k) : getproperty(getfield(d, :ds), k)
function HIPNoLensingDataSet(ds::NoLensingDataSet)
    ctx = hip_ctx(ds.d.metadata)
    h, id = Ref{Ptr{Cvoid}}(), Ref{Ptr{Cvoid}}()
    chk(ccall((:cmbl_dataset_create, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}), ctx.h, size(ds.d.arr, 3), h))
    chk(ccall((:cmbl_lensop_identity, lib), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), ctx.h, id))
    hd = HIPNoLensingDataSet(ds, h[], id[])
    finalizer(hd) do x
        ccall((:cmbl_lensop_destroy, lib), Cint, (Ptr{Cvoid},), getfield(x, :id))
        ccall((:cmbl_dataset_destroy, lib), Cint, (Ptr{Cvoid},), getfield(x, :h))
    end
    Cf, Cn = ds.Cf, ds.Cn
    set_op!(h[], ctx, OP_CF_INV, pinv(Cf));  set_op!(h[], ctx, OP_CN_INV, pinv(Cn));  set_op!(h[], ctx, OP_B, ds.B)
    set_op!(h[], ctx, OP_PRECOND_INV, pinv(pinv(Cf) + ds.B̂' * ds.M̂' * pinv(ds.Cn̂) * ds.M̂ * ds.B̂))
    M = ds.M
    if M isa LazyBinaryOp                                                  # M = Mfourier * Mpix, as in upload!(::HIPDataSet)
        set_op!(h[], ctx, OP_MF, M.X)
        m = Map(diag(M.Y)).arr[:, :, 1, 1]
        GC.@preserve m chk(ccall((:cmbl_dataset_set_op, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint), h[], OP_MPIX, devptr(m), 1))
        keepalive(ctx, m)
    else
        set_op!(h[], ctx, OP_MF, M)
    end
    a = harm(ds.d).arr
    GC.@preserve a chk(ccall((:cmbl_dataset_set_data, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint), h[], devptr(a), nbatch(ds.d)))
    keepalive(ctx, a)
    chk(ccall((:cmbl_dataset_set_logdet, lib), Cint, (Ptr{Cvoid}, Cdouble), h[], logdet(Cf) + logdet(Cn)))
    hd
end
# src/dataset.jl:76-80 with L = I:  B'M'Cn⁻¹(d − M B f) − Cf⁻¹ f
function gradientf_logpdf(hd::HIPNoLensingDataSet; f, θ=(;), d=hd.ds.d)
    fh, dh = harm(f), harm(d)
    out = similar(fh)
    zero_d = all(iszero, dh.arr) ? 1 : 0
    a, b, o = fh.arr, dh.arr, out.arr
    GC.@preserve a b o chk(ccall((:cmbl_gradientf_logpdf_op, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint),
                                 hd.h, hd.id, devptr(a), devptr(b), zero_d, devptr(o), nbatch(fh)))
    keepalive(hip_ctx(fh.metadata), a, b)
    out
end
# src/maximization.jl:17-42 with L = I; returns (f, history) like the reference
function argmaxf_logpdf(hd::HIPNoLensingDataSet, Ω::NamedTuple, d=hd.ds.d; fstart=nothing, preconditioner=:diag,
                        conjgrad_kwargs=(tol=1e-1, nsteps=500), offset=false)
    dh = harm(d)
    out = similar(dh)
    nsteps = get(conjgrad_kwargs, :nsteps, 500)
    B = nbatch(dh)
    hist = Vector{Cdouble}(undef, nsteps * B)
    nit = Ref{Cint}(0)
    fs = isnothing(fstart) ? nothing : harm(fstart).arr
    a, o = dh.arr, out.arr
    GC.@preserve a o fs hist chk(ccall((:cmbl_wiener_cg_op, lib), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cint, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cint}, Cint),
              hd.h, hd.id, devptr(a), isnothing(fs) ? C_NULL : devptr(fs), get(conjgrad_kwargs, :tol, 1e-1), nsteps, devptr(o), hist, nit, B))
    history = [(i=i, res=(B == 1 ? hist[i] : batch(hist[(i-1)*B+1:i*B]))) for i in 1:nit[]]
    out, history
end
CMBLensing.MAP_joint(θ, hd::HIPNoLensingDataSet; kwargs...) = (argmaxf_logpdf(hd, (; θ); kwargs...)[1], nothing)       # src/maximization.jl:235
# logpdf(ds; f) (src/dataset.jl:68-73) and, with `grad = true`, (logpdf, gradientf_logpdf) from one pass
function logpdf(hd::HIPNoLensingDataSet; f, θ=(;), d=hd.ds.d, grad=false)
    fh, dh = harm(f), harm(d)
    B = nbatch(fh)
    lp = Vector{Cdouble}(undef, B)
    g = grad ? similar(fh) : nothing
    a, b = fh.arr, dh.arr
    ga = grad ? g.arr : nothing
    GC.@preserve a b ga lp chk(ccall((:cmbl_nolensing_logpdf, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cvoid}, Cint),
                                     hd.h, devptr(a), devptr(b), lp, grad ? devptr(ga) : C_NULL, B))
    T = real(eltype(fh))
    v = B == 1 ? T(lp[1]) : batch(T.(lp))
    grad ? (v, g) : v
end

# logpdf(Mixed(ds); f°, ϕ°[, θ]) (src/dataset.jl:84-87) and its gradient: unmix (G \ ϕ°, precompute, D \ (L \ f°)), the three
# quadratic forms with their logdets, and for the gradient the chain rule through one inverse and one forward δ-flow -- one call
# each.  The positional helper carries the Zygote adjoint (an `@adjoint` cannot return cotangents of keyword arguments; Zygote
# differentiates the keyword method below down to this call on its own), so `gradient(Ω° -> logpdf(Mixed(ds); f°, Ω°..., θ), Ω°)`
# (src/maximization.jl:178) and `gradient(U, ϕ°)` in hmc_step (src/sampling.jl:405) land on cmbl_grad_logpdf_mixed unmodified.
function hip_logpdf_mixed(hd::HIPDataSet, f°::Field, ϕ°::Field)
    fo, po = Ł(f°), Fourier(ϕ°)
    B = nbatch(fo)
    lp = Vector{Cdouble}(undef, B)
    a, b = fo.arr, po.arr
    GC.@preserve a b lp chk(ccall((:cmbl_logpdf_mixed, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Cint),
                                  hd.h, hd.L.h, devptr(a), devptr(b), lp, B))
    hd.L.cached = nothing                                                 # the library re-pointed the flow at G \ ϕ° (include/cmblens.h)
    T = real(eltype(fo))
    B == 1 ? T(lp[1]) : batch(T.(lp))
end
function hip_grad_logpdf_mixed(hd::HIPDataSet, f°::Field, ϕ°::Field)
    fo, po = Ł(f°), Fourier(ϕ°)
    B = nbatch(fo)
    lp = Vector{Cdouble}(undef, B)
    gf, gϕ = similar(fo), similar_ϕ(po, fo)
    a, b, c, d = fo.arr, po.arr, gf.arr, gϕ.arr
    GC.@preserve a b c d lp chk(ccall((:cmbl_grad_logpdf_mixed, lib), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint),
              hd.h, hd.L.h, devptr(a), devptr(b), lp, devptr(c), devptr(d), B, hd.L.alias_quirk ? 1 : 0))
    hd.L.cached = nothing
    T = real(eltype(fo))
    (B == 1 ? T(lp[1]) : batch(T.(lp))), gf, gϕ
end
Zygote.@adjoint function hip_logpdf_mixed(hd::HIPDataSet, f°::Field{Bf}, ϕ°::Field{Bϕ}) where {Bf,Bϕ}
    lp, gf, gϕ = hip_grad_logpdf_mixed(hd, f°, ϕ°)
    # gradients come back as the reference's do: the f° cotangent in the basis of f°, the ϕ° one in the basis of ϕ° (src/autodiff.jl:105-133)
    lp, Δ -> (nothing, Bf(Δ * gf), Bϕ(Δ * gϕ))
end
function logpdf(mds::Mixed{<:HIPDataSet}; f°, ϕ°, θ=(;), Ω...)
    lp = hip_logpdf_mixed(mds.ds(θ), f°, ϕ°)
    depends_on_θ(mds.ds, θ) ? lp - logdet(mds.ds.ds.D, θ) - logdet(mds.ds.ds.G, θ) : lp      # src/dataset.jl:86, on the θ-dependent originals
end

# ---- the θ layer on the device (include/cmblens.h): the grid of logpdf(Mixed(ds); f°, ϕ°, θ) of gibbs_sample_slice_θ! (src/sampling.jl:427-437) in
# one call.  Thin wrappers over host arrays: planes are Float64 (Ny÷2+1, Nx[, nplanes]) arrays as `diag(op)` of the reference's operators gives
# them, `bands` a vector of (planes = bit mask, idx::Matrix{Int32}, nbins) of a bandpower-rescaled Cf (src/proj_lambert.jl:374-411) or empty.
function hip_theta_model!(hd::HIPDataSet, Cfs::Array{Float64}, Cten::Array{Float64}, Cn̂::Array{Float64}, σ²len, r₀, Cϕ₀::Matrix{Float64}, Aϕ₀,
                          Nϕ::Matrix{Float64}, logdetCn; C₀=nothing, bands=(), G=nothing)
    nb = length(bands)
    masks = Cint[b.planes for b in bands]
    idx = nb == 0 ? Int32[] : reduce(vcat, [vec(Int32.(b.idx)) for b in bands])
    nbins = Cint[b.nbins for b in bands]
    GC.@preserve Cfs Cten Cn̂ Cϕ₀ Nϕ C₀ G masks idx nbins chk(ccall((:cmbl_dataset_theta_model, lib), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Int32}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble,
               Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble),
              hd.h, Cfs, size(Cfs, 3), isnothing(C₀) ? C_NULL : C₀, nb, nb == 0 ? C_NULL : masks, nb == 0 ? C_NULL : idx, nb == 0 ? C_NULL : nbins,
              Cten, Cn̂, σ²len, r₀, Cϕ₀, Aϕ₀, Nϕ, isnothing(G) ? C_NULL : G, logdetCn))
    hd
end
# rs, Aϕs: one value per θ, NaN = "not named in θ"; amps: (Σ nbins, nθ) matrix of amplitude vectors or nothing.  -> (nbatch, nθ) matrix
function hip_logpdf_mixed_theta(hd::HIPDataSet, f°::Field, ϕ°::Field, rs::Vector{Float64}, Aϕs::Vector{Float64}, amps::Union{Nothing,Matrix{Float64}}=nothing)
    fo, po = Ł(f°), Fourier(ϕ°)
    B, nθ = nbatch(fo), length(rs)
    lp = Matrix{Cdouble}(undef, B, nθ)
    a, b = fo.arr, po.arr
    GC.@preserve a b lp rs Aϕs amps chk(ccall((:cmbl_logpdf_mixed_theta, lib), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
              hd.h, hd.L.h, devptr(a), devptr(b), B, nθ, rs, Aϕs, isnothing(amps) ? C_NULL : amps, isnothing(amps) ? 0 : size(amps, 1), lp))
    hd.L.cached = nothing
    lp
end
# testing aid: the operator set `which` (0 Cf⁻¹, 5 D⁻¹, 7 Cϕ⁻¹, 8 G⁻¹) the θ kernel makes at one θ into the device array `out`, and the three sums
function hip_theta_ops!(out, hd::HIPDataSet, which::Integer, r::Float64, Aϕ::Float64, amps::Union{Nothing,Vector{Float64}}=nothing)
    sums = Vector{Cdouble}(undef, 3)
    GC.@preserve out sums amps chk(ccall((:cmbl_dataset_theta_ops, lib), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Ptr{Cdouble}, Cint, Cint, Ptr{Cvoid}, Ptr{Cdouble}),
              hd.h, r, Aϕ, isnothing(amps) ? C_NULL : amps, isnothing(amps) ? 0 : length(amps), which, devptr(out), sums))
    sums
end
# the θ-gradient at one θ (∇θ_logLike of ext/CMBLensingMuseInferenceExt.jl:52-54 without automatic differentiation).  r, Aϕ: NaN = "not named in θ";
# amps: the amplitude vectors concatenated, or nothing; want: a mask of 1 (r), 2 (Aϕ), 4 (amplitudes).  -> (2 + length(amps), nbatch) matrix with rows
# d/dr, d/dAϕ, d/d amplitudes; what `want` leaves out is 0
function hip_grad_theta_logpdf(hd::HIPDataSet, f::Field, ϕ::Field, r::Float64, Aϕ::Float64, amps::Union{Nothing,Vector{Float64}}=nothing;
                               want::Integer=(isnan(r) ? 0 : 1) | (isnan(Aϕ) ? 0 : 2) | (isnothing(amps) ? 0 : 4))
    fh, ϕl = harm(f), Fourier(ϕ)
    B, na = nbatch(fh), isnothing(amps) ? 0 : length(amps)
    g = Matrix{Cdouble}(undef, 2 + na, B)
    a, b = fh.arr, ϕl.arr
    GC.@preserve a b g amps chk(ccall((:cmbl_grad_theta_logpdf, lib), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cdouble, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}),
              hd.h, devptr(a), devptr(b), B, r, Aϕ, isnothing(amps) ? C_NULL : amps, na, want, g))
    g
end
# -> (logpdf(Mixed(ds); f°, ϕ°, θ) per slot, the same matrix for its θ-gradient)
function hip_grad_theta_logpdf_mixed(hd::HIPDataSet, f°::Field, ϕ°::Field, r::Float64, Aϕ::Float64, amps::Union{Nothing,Vector{Float64}}=nothing;
                                     want::Integer=(isnan(r) ? 0 : 1) | (isnan(Aϕ) ? 0 : 2) | (isnothing(amps) ? 0 : 4))
    fo, po = Ł(f°), Fourier(ϕ°)
    B, na = nbatch(fo), isnothing(amps) ? 0 : length(amps)
    lp, g = Vector{Cdouble}(undef, B), Matrix{Cdouble}(undef, 2 + na, B)
    a, b = fo.arr, po.arr
    GC.@preserve a b lp g amps chk(ccall((:cmbl_grad_theta_logpdf_mixed, lib), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cdouble, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
              hd.h, hd.L.h, devptr(a), devptr(b), B, r, Aϕ, isnothing(amps) ? C_NULL : amps, na, want, lp, g))
    hd.L.cached = nothing
    lp, g
end

# ---- reductions and random fields (optional: the generic Julia broadcasts on ROCArrays work too) ------------------------------
# restricted to device-backed flat-sky fields: CPU fields and other projections keep the reference's own `dot`
function LinearAlgebra.dot(a::BaseField{B,<:ProjLambert,<:Any,<:ROCArray}, b::BaseField{B,<:ProjLambert,<:Any,<:ROCArray}) where {B}
    ctx = hip_ctx(a.metadata)
    out = Vector{Cdouble}(undef, nbatch(a))
    x, y = a.arr, b.arr
    GC.@preserve x y out chk(ccall((:cmbl_dot, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}),
                                   ctx.h, basis_tag(a), devptr(x), devptr(y), npol(a), nbatch(a), out))
    nbatch(a) == 1 ? out[1] : batch(out)
end

# `set_sum_accuracy_mode!` (src/util.jl:288-292) for the library's reductions: nothing / Float64 / :kahan
function set_sum_accuracy_mode!(proj::ProjLambert, mode)
    m = mode === nothing ? 0 : mode === Float64 ? 1 : mode === :kahan ? 2 : error("mode must be `nothing`, `:kahan`, `Float64`")
    chk(ccall((:cmbl_set_sum_accuracy_mode, lib), Cint, (Ptr{Cvoid}, Cint), hip_ctx(proj).h, m))
end

# `ud_grade` (src/proj_lambert.jl:533-592) for device-backed flat-sky fields: one `cmbl_ud_grade` call between the contexts of the two grids
# (include/cmblens.h has the semantics: the reference's, with the Nyquist cut decided by integer index).  Keywords, defaults, errors and the basis
# of the result are the reference's.  Map mode acts on maps of the QU components, so an EB field goes through its QU-Fourier form; Fourier mode
# takes the half planes as they come (EB stays EB).
function CMBLensing.ud_grade(f::BaseField{B,<:ProjLambert,<:Any,<:ROCArray}, θnew;
                             mode=:map, deconv_pixwin=(mode==:map), anti_aliasing=(mode==:map)) where {B}
    θ = f.θpix
    θnew == θ && return f
    (mode in (:map, :fourier)) || throw(ArgumentError("Available modes: [:map,:fourier]"))
    down = θnew > θ
    ratio = down ? θnew / θ : θ / θnew
    fac = round(Int, ratio)
    (fac >= 2 && isapprox(ratio, fac; rtol=1e-6)) || throw(ArgumentError("Can only ud_grade in integer steps"))
    (down || mode == :map) || error("Not implemented")
    (down || !deconv_pixwin) || error("Not implemented")
    Ny, Nx = down ? (f.Ny ÷ fac, f.Nx ÷ fac) : (f.Ny * fac, f.Nx * fac)
    proj = ProjLambert(; Ny, Nx, θpix=θnew, T=real(f.T), f.storage, f.rotator)
    g = (mode == :map && basis_tag(f) == HARMONIC) ? Ð(f) : f
    complex_out = mode == :fourier || deconv_pixwin
    tag_out = complex_out ? (basis_tag(g) == HARMONIC ? HARMONIC : FOURIER) : MAP
    Bg = basis_of(g)
    Bout = complex_out ? (basis_tag(g) == MAP ? Fourier(Bg()) : Bg) : Map(Bg())      # as the reference spells it (:560, 565)
    a = g.arr
    out = similar(a, complex_out ? Complex{real(f.T)} : real(f.T), (complex_out ? Ny ÷ 2 + 1 : Ny, Nx, npol(g), nbatch(g)))
    GC.@preserve a out chk(ccall((:cmbl_ud_grade, lib), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint),
              hip_ctx(g.metadata).h, hip_ctx(proj).h, mode == :map ? 0 : 1, deconv_pixwin ? 1 : 0, anti_aliasing ? 1 : 0,
              basis_tag(g), devptr(a), tag_out, devptr(out), npol(g), nbatch(g)))
    keepalive(hip_ctx(g.metadata), a)
    BaseField{Bout}(out, proj)
end
basis_of(::BaseField{B}) where {B} = B

# `get_Cℓ` (src/proj_lambert.jl:470-513) for device-backed flat-sky fields: the binned sums S1 = Σ w·CL (and S2 with `err_estimate`) come from ONE
# `cmbl_get_cl` call per basis instead of `adapt(Array, f)` and a host histogram; A, Sℓ and the mode counts come from the binning plan, made once
# per (ProjLambert, ℓedges, weight plane) on the host in double (include/cmblens.h has the semantics: λ-weighted half plane, bins decided on the
# context's ℓmag in double, σℓ as evidently intended).  Keywords, defaults and the shape of the result are the reference's.
mutable struct HIPClBins
    h :: Ptr{Cvoid}
    A :: Vector{Float64}; Sℓ :: Vector{Float64}; count :: Vector{Float64}
end
const clbins = Dict{Any,HIPClBins}()
function hip_clbins(proj::ProjLambert, ℓedges, Cℓfid)
    edges = collect(Float64, ℓedges)
    w = nothing
    if Cℓfid !== nothing
        L = Float64.(permutedims(CMBLensing.cpu(proj.ℓmag)))                                     # (Nx, Ny÷2+1) row-major == the ABI plane
        w = vec(nan2zero.(inv.(2 .* Cℓfid.(L) .^ 2 ./ (2 .* L .+ 1))))
    end
    get!(clbins, (objectid(proj), edges, w)) do
        h = Ref{Ptr{Cvoid}}()
        chk(ccall((:cmbl_clbins_create, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Csize_t, Ptr{Ptr{Cvoid}}),
                  hip_ctx(proj).h, edges, length(edges), w === nothing ? C_NULL : w, w === nothing ? 0 : length(w), h))
        info = map(0:2) do which
            out = Vector{Float64}(undef, length(edges) - 1)
            chk(ccall((:cmbl_clbins_info_host, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Csize_t), h[], which, out, length(out)))
            out
        end
        finalizer(b -> ccall((:cmbl_clbins_destroy, lib), Cint, (Ptr{Cvoid},), b.h), HIPClBins(h[], info...))
    end
end
cl_plane(f::BaseField, x::Char) = npol(f) == 1 ? 0 : (x == 'I' ? 0 : (x in ('Q', 'E') ? 0 : 1) + (npol(f) == 3 ? 1 : 0))
# the binned sums of the letter pairs `names`, all of ONE basis: (nbins, moments, npairs, batch)
function cl_sums(f1::BaseField, f2::BaseField, names, bins::HIPClBins, moments)
    ctx = hip_ctx(f1.metadata)
    pairs = Cint[cl_plane(f1, c) for n in names for c in n]
    a, b = f1.arr, f2.arr
    out = similar(a, Float64, (length(bins.A), moments, length(names), nbatch(f1)))
    GC.@preserve a b out chk(ccall((:cmbl_get_cl, lib), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Cint}, Cint, Cint, Ptr{Cvoid}),
              ctx.h, bins.h, basis_tag(f1), devptr(a), f2 === f1 ? C_NULL : devptr(b), npol(f1), nbatch(f1), pairs, length(names), moments, devptr(out)))
    keepalive(ctx, a, b)
    Array(out)                                                                                   # synchronises
end
function CMBLensing.get_Cℓ(f₁::BaseField{B1,<:ProjLambert,<:Any,<:ROCArray}, f₂::BaseField{B2,<:ProjLambert,<:Any,<:ROCArray}=f₁;
                           Δℓ=50, ℓedges=0:Δℓ:16000, Cℓfid=nothing, err_estimate=false,
                           which=(npol(f₁) == 1 ? :II : npol(f₁) == 2 ? (:EE,:BB) : (:II,:EE,:BB,:IE,:IB,:EB))) where {B1,B2}
    names = string.(CMBLensing.ensure1d(which))
    bins = hip_clbins(f₁.metadata, ℓedges, Cℓfid)
    moments = err_estimate ? 2 : 1
    isqu(n) = any(in("QU"), n)
    S = Array{Float64}(undef, length(bins.A), moments, length(names), nbatch(f₁))
    for (sel, conv) in ((isqu, f -> basis_tag(f) == HARMONIC ? Ð(f) : f), (!isqu, f -> npol(f) == 1 ? f : harm(f)))
        ks = findall(sel, names)
        isempty(ks) && continue
        g₁ = conv(f₁); g₂ = f₂ === f₁ ? g₁ : conv(f₂)
        basis_tag(g₁) == basis_tag(g₂) || ((g₁, g₂) = (Fourier(g₁), Fourier(g₂)))
        S[:, :, ks, :] = cl_sums(g₁, g₂, names[ks], bins, moments)
    end
    one(k, b) = begin
        Cℓ = S[:, 1, k, b] ./ bins.A
        err_estimate || return Cℓs(bins.Sℓ ./ bins.A, Cℓ)
        σℓ = sqrt.(max.(S[:, 2, k, b] ./ bins.A .- Cℓ .^ 2, 0) ./ (bins.count ./ 2))
        Cℓs(bins.Sℓ ./ bins.A, Cℓ .± σℓ)
    end
    res = map(1:nbatch(f₁)) do b
        which isa Symbol ? one(1, b) : (; (Symbol(n) => one(k, b) for (k, n) in enumerate(names))...)
    end
    nbatch(f₁) == 1 ? res[1] : res
end

# `make_mask` (src/masking.jl:1-24; `make_mask(f::LambertField)`, src/proj_lambert.jl:464) for device-backed flat-sky fields: ONE `cmbl_make_mask`
# call (include/cmblens.h has the semantics) instead of ImageMorphology / ImageFiltering on the host.  Keywords, defaults, the unit conversion and
# the draw of the point sources (`rand(rng, 1:Ny)`, then `rand(rng, 1:Nx)`, per source) are the reference's, so a given `rng` puts the holes where the
# reference does; the mask comes back on the device in the field's precision, its values Float32 numbers like upstream's.
function CMBLensing.make_mask(rng::Random.AbstractRNG, f::BaseField{B,<:ProjLambert,<:Any,<:ROCArray};
                              edge_padding_deg=2, edge_rounding_deg=1, apodization_deg=1, ptsrc_radius_arcmin=7,
                              num_ptsrcs=round(Int, f.Ny * f.Nx * (f.θpix/60)^2 * 120/100)) where {B}
    θpix = f.θpix
    deg2npix(x) = round(Int, x/θpix*60)
    arcmin2npix(x) = round(Int, x/θpix)
    yx = Cint[]
    for i in 1:num_ptsrcs
        push!(yx, rand(rng, 1:f.Ny) - 1)
        push!(yx, rand(rng, 1:f.Nx) - 1)
    end
    boolean = apodization_deg in (false, 0)
    apod_w = boolean ? 0 : deg2npix(apodization_deg)
    (boolean || apod_w > 0) || throw(ArgumentError("apodization_deg is below half a pixel"))
    round_w = edge_rounding_deg == false ? 0 : deg2npix(edge_rounding_deg)
    out = similar(f.arr, real(f.T), (f.Ny, f.Nx))
    GC.@preserve yx out chk(ccall((:cmbl_make_mask, lib), Cint, (Ptr{Cvoid}, Ptr{Cint}, Cint, Cint, Cint, Cint, Cint, Ptr{Cvoid}),
                                  hip_ctx(f.metadata).h, isempty(yx) ? C_NULL : yx, num_ptsrcs, deg2npix(edge_padding_deg), apod_w, round_w,
                                  arcmin2npix(ptsrc_radius_arcmin), devptr(out)))
    BaseField{Map}(out, f.metadata)
end
CMBLensing.make_mask(f::BaseField{B,<:ProjLambert,<:Any,<:ROCArray}; kwargs...) where {B} = CMBLensing.make_mask(Random.default_rng(), f; kwargs...)

# ---- ProjEquiRect (src/proj_equirect.jl) for device-backed fields and operators: the azimuthal transforms (:149-178), `M*f`, `M'*f` (:230-240), the three
# operator products (:254-269, on the matrix cores), `dot(M₁', M₂)` (:358-360) and the beams (:505-533) are one `cmbl_equirect_*` call each
# (include/cmblens.h has the semantics, the two quirks included: QU needs an even Nx, and QUMap's second assignment wins at columns 0 and Nx÷2).
# `sqrt`, `pinv` (:313-333), `logabsdet` (:342-347), `\` and `/` of two operators (:274-282) and `M \ f` factorise the blocks on the device, one workgroup per
# block, in double (`cmbl_equirect_block_svd`, `_logabsdet`, `_solve`; blocks up to n = 2048, larger ones keep the reference's methods), with the reference's
# caches.  `+`, `-` keep the reference's own methods (AMDGPU.jl's broadcasts), and so does `Cℓ_to_Cov` (CirculantCov.jl on the host, then `gpu`).
const AZFOURIER = Cint(3)                                                    # CMBL_AZFOURIER
eq_nbatch(a, nd) = ndims(a) > nd ? size(a, nd + 1) : 1
function CMBLensing.AzFourier(f::BaseField{Map,<:CMBLensing.ProjEquiRect,<:Any,<:ROCArray})                     # :149-152
    a = f.arr; B = eq_nbatch(a, 2); out = similar(a, complex(eltype(a)), (f.Ny, f.Nx ÷ 2 + 1, B))
    GC.@preserve a out chk(ccall((:cmbl_equirect_convert, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint),
                                 hip_ctx(f.metadata).h, MAP, devptr(a), AZFOURIER, devptr(out), 1, B))
    CMBLensing.EquiRectAzFourier(B == 1 ? dropdims(out, dims=3) : out, f.metadata)
end
function CMBLensing.Map(f::BaseField{CMBLensing.AzFourier,<:CMBLensing.ProjEquiRect,<:Any,<:ROCArray})          # :154-157
    a = f.arr; B = eq_nbatch(a, 2); out = similar(a, real(eltype(a)), (f.Ny, f.Nx, B))
    GC.@preserve a out chk(ccall((:cmbl_equirect_convert, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint),
                                 hip_ctx(f.metadata).h, AZFOURIER, devptr(a), MAP, devptr(out), 1, B))
    CMBLensing.EquiRectMap(B == 1 ? dropdims(out, dims=3) : out, f.metadata)
end
function CMBLensing.QUAzFourier(f::BaseField{CMBLensing.QUMap,<:CMBLensing.ProjEquiRect,<:Any,<:ROCArray})      # :160-168
    a = f.arr; B = eq_nbatch(a, 3); out = similar(a, complex(eltype(a)), (2f.Ny, f.Nx ÷ 2 + 1, B))
    GC.@preserve a out chk(ccall((:cmbl_equirect_convert, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint),
                                 hip_ctx(f.metadata).h, MAP, devptr(a), AZFOURIER, devptr(out), 2, B))
    CMBLensing.EquiRectQUAzFourier(B == 1 ? dropdims(out, dims=3) : out, f.metadata)
end
function CMBLensing.QUMap(f::BaseField{CMBLensing.QUAzFourier,<:CMBLensing.ProjEquiRect,<:Any,<:ROCArray})      # :170-178
    a = f.arr; B = eq_nbatch(a, 2); out = similar(a, real(eltype(a)), (f.Ny, f.Nx, 2, B))
    GC.@preserve a out chk(ccall((:cmbl_equirect_convert, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint),
                                 hip_ctx(f.metadata).h, AZFOURIER, devptr(a), MAP, devptr(out), 2, B))
    CMBLensing.EquiRectQUMap(B == 1 ? dropdims(out, dims=4) : out, f.metadata)
end

const ROCBlockDiag{B,T,P,A<:ROCArray} = CMBLensing.BlockDiagEquiRect{B,T,P,A}
function equirect_apply(M::ROCBlockDiag, f::BaseField, adjoint::Bool)
    blocks, a = M.blocks, f.arr
    n = size(blocks, 1); B = eq_nbatch(a, 2)
    out = similar(a)
    GC.@preserve blocks a out chk(ccall((:cmbl_equirect_block_apply, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint),
                                        hip_ctx(M.proj).h, devptr(blocks), eltype(blocks) <: Complex, n, adjoint, devptr(a), devptr(out), B))
    typeof(f)(out, f.metadata)
end
(*)(M::ROCBlockDiag{B}, f::BaseField{B,<:CMBLensing.ProjEquiRect,<:Any,<:ROCArray}) where {B<:CMBLensing.AzBasis} = equirect_apply(M, f, false)                 # :230-233
(*)(M::Adjoint{<:Any,<:ROCBlockDiag{B}}, f::BaseField{B,<:CMBLensing.ProjEquiRect,<:Any,<:ROCArray}) where {B<:CMBLensing.AzBasis} = equirect_apply(M.parent, f, true)   # :237-240
function equirect_matmul(M₁::ROCBlockDiag{B}, adj₁::Bool, M₂::ROCBlockDiag{B}, adj₂::Bool) where {B}
    E = promote_type(eltype(M₁.blocks), eltype(M₂.blocks))
    a, b = E.(M₁.blocks), E.(M₂.blocks)
    out = similar(a)
    GC.@preserve a b out chk(ccall((:cmbl_equirect_block_matmul, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cvoid}),
                                   hip_ctx(M₁.proj).h, devptr(a), adj₁, devptr(b), adj₂, E <: Complex, size(a, 1), devptr(out)))
    CMBLensing.BlockDiagEquiRect{B}(out, M₁.proj)
end
(*)(M₁::ROCBlockDiag{B}, M₂::ROCBlockDiag{B}) where {B<:CMBLensing.AzBasis} = equirect_matmul(M₁, false, M₂, false)                                             # :254-257
(*)(M₁::Adjoint{<:Any,<:ROCBlockDiag{B}}, M₂::ROCBlockDiag{B}) where {B<:CMBLensing.AzBasis} = equirect_matmul(M₁.parent, true, M₂, false)                      # :260-263
(*)(M₁::ROCBlockDiag{B}, M₂::Adjoint{<:Any,<:ROCBlockDiag{B}}) where {B<:CMBLensing.AzBasis} = equirect_matmul(M₁, false, M₂.parent, true)                      # :266-269
function LinearAlgebra.dot(M₁::Adjoint{<:Any,<:ROCBlockDiag{B}}, M₂::ROCBlockDiag{B}) where {B<:CMBLensing.AzBasis}                                             # :358-360
    E = promote_type(eltype(M₁.parent.blocks), eltype(M₂.blocks))
    a, b = E.(M₁.parent.blocks), E.(M₂.blocks)
    out = zeros(Cdouble, 2)
    GC.@preserve a b out chk(ccall((:cmbl_equirect_block_dot, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}),
                                   hip_ctx(M₂.proj).h, devptr(a), devptr(b), E <: Complex, size(a, 1), out))
    E <: Complex ? E(complex(out[1], out[2])) : E(out[1])
end
# sqrt, pinv (:313-333): one Jacobi SVD of every block; pinv cuts at the reference's n eps(T) (LinearAlgebra.pinv's default rtol)
const EQ_FACTOR_NMAX = 2048
function equirect_svd!(M::ROCBlockDiag, out_sqrt, out_pinv)
    blocks = M.blocks
    n = size(blocks, 1)
    rtol = Cdouble(n * eps(real(eltype(blocks))))
    GC.@preserve blocks out_sqrt out_pinv chk(ccall((:cmbl_equirect_block_svd, lib), Cint,
                                                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cint}),
                                                    hip_ctx(M.proj).h, devptr(blocks), eltype(blocks) <: Complex, n, rtol,
                                                    out_sqrt === nothing ? C_NULL : devptr(out_sqrt), out_pinv === nothing ? C_NULL : devptr(out_pinv), C_NULL, C_NULL))
end
function LinearAlgebra.sqrt(M::ROCBlockDiag{B}) where {B<:CMBLensing.AzBasis}
    size(M.blocks, 1) > EQ_FACTOR_NMAX && return invoke(LinearAlgebra.sqrt, Tuple{CMBLensing.BlockDiagEquiRect{B}}, M)
    if !isassigned(M.blocks_sqrt)
        out = similar(M.blocks)
        equirect_svd!(M, out, nothing)
        M.blocks_sqrt[] = out
    end
    CMBLensing.BlockDiagEquiRect{B}(M.blocks_sqrt[], M.proj)
end
function LinearAlgebra.pinv(M::ROCBlockDiag{B}) where {B<:CMBLensing.AzBasis}
    size(M.blocks, 1) > EQ_FACTOR_NMAX && return invoke(LinearAlgebra.pinv, Tuple{CMBLensing.BlockDiagEquiRect{B}}, M)
    if !isassigned(M.blocks_pinv)
        out = similar(M.blocks)
        equirect_svd!(M, nothing, out)
        M.blocks_pinv[] = out
    end
    CMBLensing.BlockDiagEquiRect{B}(M.blocks_pinv[], M.proj)
end
function LinearAlgebra.logabsdet(M::ROCBlockDiag{B,T}) where {B<:CMBLensing.AzBasis,T}                                                                          # :342-347
    size(M.blocks, 1) > EQ_FACTOR_NMAX && return invoke(LinearAlgebra.logabsdet, Tuple{CMBLensing.BlockDiagEquiRect{B}}, M)
    if M.logabsdet[] == (0, 0)
        blocks = M.blocks
        out = zeros(Cdouble, 3)
        GC.@preserve blocks out chk(ccall((:cmbl_equirect_block_logabsdet, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}),
                                          hip_ctx(M.proj).h, devptr(blocks), eltype(blocks) <: Complex, size(blocks, 1), out))
        M.logabsdet[] = (T(out[1]), Complex{T}(out[2], out[3]))
    end
    M.logabsdet[]
end
# M₁ \ M₂ (side 0, CMBL_SIDE_LEFT) and M₁ / M₂ (side 1, CMBL_SIDE_RIGHT: the matrix that is inverted is M₂) (:274-282); rhs_kind 0 = CMBL_RHS_BLOCKS
function equirect_solve(A::ROCBlockDiag{B}, side::Integer, R::ROCBlockDiag{B}) where {B}
    a, r = A.blocks, R.blocks
    out = similar(r, promote_type(eltype(a), eltype(r)))
    GC.@preserve a r out chk(ccall((:cmbl_equirect_block_solve, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Cint),
                                   hip_ctx(A.proj).h, devptr(a), eltype(a) <: Complex, size(a, 1), side, devptr(r), eltype(r) <: Complex, 0, devptr(out), 1))
    CMBLensing.BlockDiagEquiRect{B}(out, A.proj)
end
function Base.:\(M₁::ROCBlockDiag{B}, M₂::ROCBlockDiag{B}) where {B<:CMBLensing.AzBasis}
    size(M₁.blocks, 1) > EQ_FACTOR_NMAX && return invoke(\, Tuple{CMBLensing.BlockDiagEquiRect{B},CMBLensing.BlockDiagEquiRect{B}}, M₁, M₂)
    CMBLensing.promote_metadata_strict(M₁.proj, M₂.proj)
    equirect_solve(M₁, 0, M₂)
end
function Base.:/(M₁::ROCBlockDiag{B}, M₂::ROCBlockDiag{B}) where {B<:CMBLensing.AzBasis}
    size(M₁.blocks, 1) > EQ_FACTOR_NMAX && return invoke(/, Tuple{CMBLensing.BlockDiagEquiRect{B},CMBLensing.BlockDiagEquiRect{B}}, M₁, M₂)
    CMBLensing.promote_metadata_strict(M₁.proj, M₂.proj)
    equirect_solve(M₂, 1, M₁)
end
# M \ f, the reference's mapblocks(\, M, f); rhs_kind 1 = CMBL_RHS_FIELD
function Base.:\(M::ROCBlockDiag{B}, f::BaseField{B,<:CMBLensing.ProjEquiRect,<:Any,<:ROCArray}) where {B<:CMBLensing.AzBasis}
    CMBLensing.promote_metadata_strict(M.proj, f.metadata)
    blocks, a = M.blocks, f.arr
    nb = eq_nbatch(a, 2)
    out = similar(a)
    GC.@preserve blocks a out chk(ccall((:cmbl_equirect_block_solve, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Cint),
                                        hip_ctx(M.proj).h, devptr(blocks), eltype(blocks) <: Complex, size(blocks, 1), 0, devptr(a), true, 1, devptr(out), nb))
    typeof(f)(out, f.metadata)
end
# the Ω steps of Cℓ_to_Beam (:512, 524-530) on device-backed :I covariance blocks
function equirect_beam(pol::Symbol, Cov::ROCBlockDiag{CMBLensing.AzFourier})
    proj = Cov.proj
    Ω = Cdouble.(Array(proj.Ω))
    if pol == :I
        blocks = copy(Cov.blocks)
        GC.@preserve blocks Ω chk(ccall((:cmbl_equirect_block_scale_columns, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cint),
                                        hip_ctx(proj).h, devptr(blocks), eltype(blocks) <: Complex, size(blocks, 1), Ω, length(Ω)))
        return CMBLensing.BlockDiagEquiRect{CMBLensing.AzFourier}(blocks, proj)
    end
    blocks = Cov.blocks
    out = similar(blocks, complex(eltype(blocks)), (2proj.Ny, 2proj.Ny, size(blocks, 3)))
    GC.@preserve blocks Ω out chk(ccall((:cmbl_equirect_beam_pol, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cvoid}),
                                        hip_ctx(proj).h, devptr(blocks), Ω, devptr(out)))
    CMBLensing.BlockDiagEquiRect{CMBLensing.QUAzFourier}(out, proj)
end

# ---- HEALPix <-> Cartesian projection (src/proj_healpix.jl), method = :bilinear and :fft, for a device-backed Cartesian side: the Projector (:254-294) is
# `cmbl_projector_create` -- pix2angRing, θϕ_to_ij / ij_to_θϕ, get_ψpol and the ring lookup of healpy.get_interp_val on the device, in double whatever
# T -- and each direction of `project` one gather kernel with the QU rotation fused in (`cmbl_project_to_cart`, `cmbl_project_to_healpix`): no
# healpy, no Images.jl, nothing through the host.  The library counts pixels from 0 and stores a HEALPix field as (npix, npol, nbatch).
# `method = :fft` is the library's CMBL_PROJECT_NFFT (`cmbl_projector_create_method`): the sums NFFT.jl's plans approximate, through an oversampled
# grid and a window to the rounding floor of T (DESIGN 4.8), so neither NFFT.jl nor CuNFFT.jl is needed; even Ny, Nx up to 2048.  The method
# belongs to the projector, as in the reference.  (Unexecuted, like the rest of this file: there is no Julia on the build machines.)
projector_method(method::Symbol) = method == :bilinear ? Cint(0) : method == :fft ? Cint(1) : error("method = :$method: :bilinear or :fft")   # CMBL_PROJECT_*
mutable struct HIPProjector
    h         :: Ptr{Cvoid}
    cart_proj
    hpx_proj  :: CMBLensing.ProjHealpix
    method    :: Symbol
    function HIPProjector(h, cart_proj, hpx_proj, method)
        P = new(h, cart_proj, hpx_proj, method)
        finalizer(P -> ccall((:cmbl_projector_destroy, lib), Cint, (Ptr{Cvoid},), P.h), P)
    end
end
projector_params(proj::ProjLambert) = (Cint(0), Cdouble[proj.rotator...])                                       # CMBL_PROJ_LAMBERT
projector_params(proj::CMBLensing.ProjEquiRect) = (Cint(1), Cdouble[proj.θspan..., proj.φspan...])              # CMBL_PROJ_EQUIRECT
function HIPProjector((hpx_proj, cart_proj)::Pair{<:CMBLensing.ProjHealpix,<:CMBLensing.CartesianProj}; method::Symbol=:bilinear)   # :254-294
    kind, params = projector_params(cart_proj)
    h = Ref{Ptr{Cvoid}}()
    GC.@preserve params chk(ccall((:cmbl_projector_create_method, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Ptr{Cvoid}}),
                                  hip_ctx(cart_proj).h, hpx_proj.Nside, kind, params, projector_method(method), h))
    HIPProjector(h[], cart_proj, hpx_proj, method)
end
HIPProjector((cart_proj, hpx_proj)::Pair{<:CMBLensing.CartesianProj,<:CMBLensing.ProjHealpix}; method::Symbol=:bilinear) = HIPProjector(hpx_proj => cart_proj; method)   # :304-306
function projector_window_width(P::HIPProjector)                                                                  # cells per axis a node touches; 0 for :bilinear
    m, w = Ref{Cint}(), Ref{Cint}()
    chk(ccall((:cmbl_projector_method, lib), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}), P.h, m, w))
    Int(w[])
end
function projector_info(P::HIPProjector, which::Integer, n::Integer)
    out = Vector{Cdouble}(undef, n)
    chk(ccall((:cmbl_projector_info_host, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Csize_t), P.h, which, out, n))
    out
end
hpx_idxs_in_patch(P::HIPProjector) = Int.(projector_info(P, 4, Int(projector_info(P, 0, 2)[1]))) .+ 1           # the reference's 1-based k (:270)
hpx_npol(::CMBLensing.HealpixField{B}) where {B} = B <: CMBLensing.Basis3Prod ? 3 : B <: CMBLensing.Basis2Prod ? 2 : 1
# project(projector, hpx_map => cart_proj) (:221-252): `hpx_map.arr` (npix, npol) is moved to the device of the projection
function CMBLensing.project(P::HIPProjector, (hpx_map, cart_proj)::Pair{<:CMBLensing.HealpixField,<:CMBLensing.CartesianProj})
    @assert P.hpx_proj == hpx_map.proj && P.cart_proj == cart_proj
    npol = hpx_npol(hpx_map)
    a = ROCArray(cart_proj.T.(hpx_map.arr))
    out = similar(a, (cart_proj.Ny, cart_proj.Nx, npol))
    GC.@preserve a out chk(ccall((:cmbl_project_to_cart, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint), P.h, devptr(a), devptr(out), npol, 1))
    npol == 1 ? BaseMap(dropdims(out, dims=3), cart_proj) : npol == 2 ? BaseField{QUMap}(out, cart_proj) : BaseField{IQUMap}(out, cart_proj)
end
# project(projector, cart_field => hpx_proj) (:308-341): Map(cart_field) is taken by the library (any basis of a ProjLambert field)
function CMBLensing.project(P::HIPProjector, (cart_field, hpx_proj)::Pair{<:BaseField{B,<:CMBLensing.CartesianProj,<:Any,<:ROCArray},<:CMBLensing.ProjHealpix}) where {B}
    @assert P.cart_proj == cart_field.proj && P.hpx_proj == hpx_proj
    f = cart_field.proj isa ProjLambert ? cart_field : Ł(cart_field)
    a = f.arr
    npol = size(a, 3)
    out = similar(a, real(eltype(a)), (12 * hpx_proj.Nside^2, npol))
    GC.@preserve a out chk(ccall((:cmbl_project_to_healpix, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint),
                                 P.h, f.proj isa ProjLambert ? basis_tag(f) : MAP, devptr(a), devptr(out), npol, 1))
    npol == 1 ? CMBLensing.HealpixMap(vec(out), hpx_proj) : npol == 2 ? CMBLensing.HealpixQUMap(out, hpx_proj) : CMBLensing.HealpixIQUMap(out, hpx_proj)
end
function CMBLensing.project((cart_field, hpx_proj)::Pair{<:BaseField{B,<:CMBLensing.CartesianProj,<:Any,<:ROCArray},<:CMBLensing.ProjHealpix}; method::Symbol=:bilinear) where {B}
    CMBLensing.project(HIPProjector(hpx_proj => cart_field.proj; method), cart_field => hpx_proj)
end
# sphere -> patch: the target decides; a projection whose `storage` is a ROCArray gets the device path
function CMBLensing.project((hpx_map, cart_proj)::Pair{<:CMBLensing.HealpixField,<:CMBLensing.CartesianProj}, ::Type{<:ROCArray}; method::Symbol=:bilinear)
    CMBLensing.project(HIPProjector(hpx_map.proj => cart_proj; method), hpx_map => cart_proj)
end

# device RNG for `simulate` / `randn!` (src/specialops.jl:6, src/base_fields.jl:169-170): counter-based Philox4x32-10
mutable struct HIPPhilox <: Random.AbstractRNG
    seed   :: UInt64
    stream :: UInt64
end
function Random.randn!(rng::HIPPhilox, ξ::BaseField{B,<:ProjLambert,<:Any,<:ROCArray}) where {B<:CMBLensing.SpatialBasis{Map}}
    seeds = fill(rng.seed, 1)
    a = ξ.arr
    GC.@preserve a seeds chk(ccall((:cmbl_randn, lib), Cint, (Ptr{Cvoid}, Ptr{UInt64}, Cint, UInt64, Ptr{Cvoid}, Clong),
                                   hip_ctx(ξ.metadata).h, seeds, 1, rng.stream, devptr(a), length(a)))
    rng.stream += 1
    ξ
end

end # module
