# SpinDynamicsMI.jl -- thin `ccall` shim that keeps the user-facing calls of
# javahedi/SpinDynamics.jl (XXZChain / groundstate / time_evolve /
# dynamical_structure_factor, plus the operator seam apply_H!) and routes the
# hot path to libspindyn.so (hand-written HIP for gfx950, include/spindyn.h).
#
# STATUS: written against the C ABI but NOT executed -- there is no Julia
# runtime in the build container or on the GPU box (SURVEY.md 8c).  It is kept
# deliberately thin: every numerical statement lives behind the C ABI, which is
# what the parity tests exercise (through the Python mirror
# spindynamics.jl_amd/, call for call the same entry points).
#
# Reference functions mirrored (file:line in the reference repository):
#   XXZChain, build_model, momenta          src/SpinModel.jl:23-38,63-90,97-99
#   apply_H!, apply_rescaled_H!, Sz_q_vector src/Hamiltonian.jl:211-273,286-301,307-337
#   groundstate, time_evolve, dynamical_structure_factor   src/PublicAPI.jl:25-155
module SpinDynamicsMI

using Random
using Libdl

export Model, build_model, XXZChain, momenta, apply_H!, apply_rescaled_H!, Sz_q_vector, create_spin_operator,
       groundstate, lowest_eigenpairs, time_evolve, structure_factor, dynamical_structure_factor,
       site_project, kpm_site_moments, kpm_reconstruct_signed, kpm_correlation_matrix, kpm_sqw_sites,
       chebyshev_imag_coeffs, chebyshev_terms, thermal_state, spin_current, current_expectation, energy_current_terms, energy_current, energy_current_expectation, pair_correlations, bond_operator, dimer_correlations, symmetry_code, is_symmetric, symmetry_apply, translate, reflect, spin_flip, symmetry_overlaps, momentum_weights, symmetry_combine, symmetry_project, OpTerm, op_string, operator_adjoint, operator_check, hamiltonian_terms, operator_apply, operator_expectations, string_order, basis_moments, participation_entropy, counting_range, counting_statistics, number_entropy, CutBlock, cut_blocks, cut_gram, permute_sites, site_permute_sources, subsystem_permutation, subsystem_gram, sample_uniforms, sample_configurations, typicality_sample, typicality_correlation_function,
       DiagonalDrive, field_drive, gradient_drive, zz_drive, drive_check, diagonal_apply, driven_apply, magnus_schedule, piecewise_schedule, stage_evolve, driven_time_evolve,
       HoppingDrive, exchange_drive, current_drive, hop_drive_check, hopping_apply,
       magnetization_per_site, connected_correlations, structure_factor_Sq,
       domain_wall_state, neel_state, polarized_state, polarized_state_with_flips

const libspindyn = get(ENV, "SPINDYN_LIB", joinpath(@__DIR__, "..", "spindynamics.jl_amd", "libspindyn.so"))

const SD_F64, SD_C128 = Cint(1), Cint(2)
dtype_code(::Type{Float64}) = SD_F64
dtype_code(::Type{ComplexF64}) = SD_C128
dtype_code(::Type{T}) where {T} = throw(ArgumentError("libspindyn supports Float64 and ComplexF64 vectors, got $T"))

# ---- status codes -> the exception types the reference throws ----------------
function check(rc::Cint, ctx::Ptr{Cvoid}=C_NULL)
    rc == 0 && return nothing
    msg = unsafe_string(ccall((:sd_last_error, libspindyn), Cstring, (Ptr{Cvoid},), ctx))
    isempty(msg) && (msg = unsafe_string(ccall((:sd_status_string, libspindyn), Cstring, (Cint,), rc)))
    rc == 1 && throw(ArgumentError(msg))          # src/Basis.jl:10-16, src/SpinModel.jl:80, src/PublicAPI.jl:34,87,152
    rc == 2 && throw(DimensionMismatch(msg))      # src/Hamiltonian.jl:63-66,220,289
    rc == 3 && error("starting vector has zero norm")   # src/Lanczos.jl:210-212
    error("libspindyn status $rc: $msg")
end

# ---- context (one per process / per GPU) ---------------------------------------
mutable struct Context
    h::Ptr{Cvoid}
    function Context(device::Integer=parse(Int, get(ENV, "LOCAL_RANK", "0")))
        r = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:sd_ctx_create, libspindyn), Cint, (Cint, Ref{Ptr{Cvoid}}), device, r))
        c = new(r[])
        finalizer(x -> ccall((:sd_ctx_destroy, libspindyn), Cvoid, (Ptr{Cvoid},), x.h), c)
        return c
    end
end
const _ctx = Ref{Union{Nothing,Context}}(nothing)
default_context() = (_ctx[] === nothing && (_ctx[] = Context()); _ctx[])

# ---- Model: same descriptor fields as SpinModel.Model minus states/idxmap ----------
# Context options (include/spindyn.h): Chebyshev moments two per apply (default) or the reference's one-per-apply loop;
# release of the device vectors a context keeps between calls (staging of sd_apply, pooled work vectors of the recursions).
set_kpm_doubling!(ctx::Context, on::Bool) =
    check(ccall((:sd_ctx_set_kpm_doubling, libspindyn), Cint, (Ptr{Cvoid}, Cint), ctx.h, on ? 1 : 0), ctx.h)
# real psi0: S(q, w) once per pair (q, 2pi - q) (default) or every q on its own as src/KPM_Sqw.jl:218-252 does
set_kpm_pair_q!(ctx::Context, on::Bool) =
    check(ccall((:sd_ctx_set_kpm_pair_q, libspindyn), Cint, (Ptr{Cvoid}, Cint), ctx.h, on ? 1 : 0), ctx.h)
# S(q, w): the momenta's vectors share the launches of their recursions at launch-bound sizes (default), or one momentum at a time
set_q_batch!(ctx::Context, on::Bool) =
    check(ccall((:sd_ctx_set_q_batch, libspindyn), Cint, (Ptr{Cvoid}, Cint), ctx.h, on ? 1 : 0), ctx.h)
# groundstate: full re-orthogonalisation in blocks of 8 columns (default) or column by column as src/Lanczos.jl:116-124
set_gs_blocked!(ctx::Context, on::Bool) =
    check(ccall((:sd_ctx_set_gs_blocked, libspindyn), Cint, (Ptr{Cvoid}, Cint), ctx.h, on ? 1 : 0), ctx.h)
# operator applications the recursion-level calls have queued on this context so far (one per recursion step)
apply_count(ctx::Context) = Int(ccall((:sd_ctx_apply_count, libspindyn), Int64, (Ptr{Cvoid},), ctx.h))
release_scratch!(ctx::Context) = check(ccall((:sd_ctx_release_scratch, libspindyn), Cint, (Ptr{Cvoid},), ctx.h), ctx.h)

mutable struct Model
    L::Int
    nup::Union{Nothing,Int}
    mode::Symbol
    hopping_list::Vector{Tuple{Int,Int,Float64}}
    onsite_field::Vector{Float64}
    zz_list::Vector{Tuple{Int,Int,Float64}}
    ctx::Context
    h::Ptr{Cvoid}
end

function build_model(L::Int; nup::Union{Nothing,Int}=nothing, hopping=[], onsite_field=zeros(L), zz=[])
    ctx = default_context()
    hop = [(Int(i), Int(j), Float64(J)) for (i, j, J) in hopping]
    zzl = [(Int(i), Int(j), Float64(J)) for (i, j, J) in zz]
    hi = Cint[h[1] for h in hop]; hj = Cint[h[2] for h in hop]; hJ = Float64[h[3] for h in hop]
    zi = Cint[z[1] for z in zzl]; zj = Cint[z[2] for z in zzl]; zJ = Float64[z[3] for z in zzl]
    f = Vector{Float64}(onsite_field)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:sd_model_create, libspindyn), Cint,
                (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Float64}, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Float64},
                 Ptr{Float64}, Ref{Ptr{Cvoid}}),
                ctx.h, L, nup === nothing ? -1 : nup, length(hi), hi, hj, hJ, length(zi), zi, zj, zJ, f, r), ctx.h)
    m = Model(L, nup, nup === nothing ? :full : :sector, hop, f, zzl, ctx, r[])
    finalizer(x -> ccall((:sd_model_destroy, libspindyn), Cvoid, (Ptr{Cvoid},), x.h), m)
    return m
end

function XXZChain(L::Int; Jxy::Real=1.0, Jz::Real=1.0, hz::Real=0.0, nup::Union{Nothing,Int}=nothing, boundary::Symbol=:open)
    hopping = [(i, i + 1, Float64(Jxy) / 2) for i in 1:(L - 1)]
    zz = [(i, i + 1, Float64(Jz)) for i in 1:(L - 1)]
    if boundary === :periodic
        if L > 2
            push!(hopping, (L, 1, Float64(Jxy) / 2)); push!(zz, (L, 1, Float64(Jz)))
        end
    elseif boundary !== :open
        throw(ArgumentError("boundary must be :open or :periodic"))
    end
    return build_model(L; nup=nup, hopping=hopping, onsite_field=fill(Float64(hz), L), zz=zz)
end

momenta(model::Model) = 2π .* (0:(model.L - 1)) ./ model.L
Base.length(model::Model) = Int(ccall((:sd_model_dim, libspindyn), Int64, (Ptr{Cvoid},), model.h))

"model.states[start:start+count-1] (1-based start), computed from closed-form unranking"
function states(model::Model, start::Integer=1, count::Integer=length(model))
    out = Vector{UInt64}(undef, count)
    check(ccall((:sd_model_states, libspindyn), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{UInt64}), model.h, start - 1, count, out))
    return out
end

# ---- operator seam: drop-in for Hamiltonian.apply_H! ------------------------------
function apply_H!(out::Vector{T}, ψ::Vector{T}, model::Model) where {T<:Union{Float64,ComplexF64}}
    length(out) == length(ψ) || throw(DimensionMismatch("length(out) != length(ψ)"))
    check(ccall((:sd_apply, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
                model.ctx.h, model.h, dtype_code(T), out, ψ, length(ψ)), model.ctx.h)
    return out
end

function apply_rescaled_H!(out::Vector{T}, ψ::Vector{T}, applyH!, model::Model, a::Float64, b::Float64) where {T<:Union{Float64,ComplexF64}}
    length(out) == length(ψ) || throw(DimensionMismatch("length(out) != length(ψ)"))
    if applyH! !== apply_H!
        # any other callable, as the reference takes it (src/Hamiltonian.jl:285-301): H ψ by the caller's operator, then the
        # rescaling pass on the host with the reference's own arithmetic
        applyH!(out, ψ, model)
        @inbounds for i in eachindex(out)
            out[i] = (out[i] - b * ψ[i]) / a
        end
        return out
    end
    # the built-in operator: apply and rescaling fused in one device pass (same arithmetic per element)
    check(ccall((:sd_apply_rescaled, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Float64),
                model.ctx.h, model.h, dtype_code(T), out, ψ, length(ψ), a, b), model.ctx.h)
    return out
end

function Sz_q_vector(model::Model, psi0::AbstractVector{T}, q::Float64) where {T<:Number}
    x = T <: Complex ? Vector{ComplexF64}(psi0) : Vector{Float64}(psi0)
    phi = Vector{ComplexF64}(undef, length(x))
    check(ccall((:sd_szq, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Float64, Ptr{Cvoid}),
                model.ctx.h, model.h, dtype_code(eltype(x)), x, length(x), q, phi), model.ctx.h)
    return phi
end

# create_spin_operator(site, op_type)  -- src/Hamiltonian.jl:49-136
const _SPIN_OPS = Dict(:z => 0, :plus => 1, :minus => 2, :x => 3, :y => 4)
function create_spin_operator(site::Int, op_type::Symbol)
    site >= 1 || throw(ArgumentError("site must be at least 1"))
    haskey(_SPIN_OPS, op_type) ||
        throw(ArgumentError("unsupported spin operator: $op_type; expected :z, :plus, :minus, :x, or :y"))
    function operator(ψ::AbstractVector{T}, model::Model) where {T}
        x = T <: Complex ? Vector{ComplexF64}(ψ) : Vector{Float64}(ψ)
        out = similar(x)
        check(ccall((:sd_spin_operator, libspindyn), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
                    model.ctx.h, model.h, dtype_code(eltype(x)), site, _SPIN_OPS[op_type], x, length(x), out), model.ctx.h)
        return out
    end
    return operator
end

# ---- Observables (src/Observables.jl) and InitialStates (src/InitialStates.jl) ------
function _obs(fname::Symbol, ψ::AbstractVector, model::Model, nout::Int)
    x = eltype(ψ) <: Complex ? Vector{ComplexF64}(ψ) : Vector{Float64}(ψ)
    outs = [Vector{Float64}(undef, model.L) for _ in 1:nout]
    fptr = Libdl.dlsym(Libdl.dlopen(libspindyn), fname)     # a (name, library) pair must be a literal for ccall: resolve the run-time name here
    if nout == 1
        check(ccall(fptr, Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Float64}),
                    model.ctx.h, model.h, dtype_code(eltype(x)), x, length(x), outs[1]), model.ctx.h)
    else
        check(ccall(fptr, Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}),
                    model.ctx.h, model.h, dtype_code(eltype(x)), x, length(x), outs[1], outs[2]), model.ctx.h)
    end
    return outs
end
magnetization_per_site(ψ::AbstractVector, model::Model) = _obs(:sd_magnetization, ψ, model, 1)[1]
connected_correlations(ψ::AbstractVector, model::Model) = _obs(:sd_connected_correlations, ψ, model, 1)[1]
function structure_factor_Sq(ψ::AbstractVector, model::Model)
    q, S = _obs(:sd_structure_factor, ψ, model, 2)
    return Dict{Float64,Float64}(q[n] => S[n] for n in 1:model.L)       # src/Observables.jl:103-108
end
structure_factor(model::Model, ψ::AbstractVector) = structure_factor_Sq(ψ, model)   # src/PublicAPI.jl:101-106

function _one_hot(model::Model, kind::Integer, flips::Vector{Int}=Int[])
    idx = Ref{Int64}(0)
    f = Cint.(flips)
    check(ccall((:sd_initial_state_index, libspindyn), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}, Cint, Ref{Int64}),
                model.h, kind, f, length(f), idx), model.ctx.h)      # SD_EARG -> ArgumentError, as the reference throws
    ψ0 = zeros(Float64, length(model))
    ψ0[idx[] + 1] = 1.0
    return ψ0
end
domain_wall_state(model::Model) = _one_hot(model, 0)
neel_state(model::Model) = _one_hot(model, 1)
polarized_state(model::Model; up::Bool=true) = _one_hot(model, up ? 2 : 3)
polarized_state_with_flips(model::Model, flips::Vector{Int}) = _one_hot(model, 4, flips)

# ---- PublicAPI (src/PublicAPI.jl) ---------------------------------------------------
# Start vectors: the reference draws them with randn(rng, T, N) (src/Lanczos.jl:39,99).  With `rng` (default
# Random.default_rng(), as in the reference) the shim draws the same vector in Julia and hands it to the library, so the
# reference's random stream -- and with it every un-converged Lanczos output -- is reproduced.  `seed=k` selects the
# library's counter-based device generator instead (no host vector: the choice for L >= 30); `psi0=v` injects a vector.
function groundstate(model::Model; method::Symbol=:lanczos, lanc_m::Int=100, tol::Float64=1e-12,
                     orthogonalize_tol::Float64=1e-10, rng::AbstractRNG=Random.default_rng(),
                     psi0::Union{Nothing,Vector{Float64}}=nothing, seed::Union{Nothing,Integer}=nothing)
    method === :lanczos || throw(ArgumentError("unsupported ground-state method: $method"))
    N = length(model)
    if psi0 === nothing && seed === nothing
        psi0 = randn(rng, Float64, N)                                   # src/Lanczos.jl:99
    end
    E0 = Ref{Float64}(0.0); mact = Ref{Cint}(0)
    gs = Vector{Float64}(undef, N)
    check(ccall((:sd_lanczos_groundstate, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Float64, Float64, Ptr{Float64}, UInt64, Ref{Float64}, Ptr{Float64}, Ref{Cint}),
                model.ctx.h, model.h, lanc_m, tol, orthogonalize_tol, psi0 === nothing ? C_NULL : psi0,
                seed === nothing ? 0 : seed, E0, gs, mact), model.ctx.h)
    return E0[], gs
end

# estimate_energy_bounds does not forward rng in the reference either (src/Lanczos.jl:258,267): both Lanczos runs draw
# from Random.default_rng()
function estimate_energy_bounds(model::Model; lanc_m::Int=80, seed::Union{Nothing,Integer}=nothing)
    lo = Ref{Float64}(0.0); hi = Ref{Float64}(0.0)
    N = length(model)
    va = seed === nothing ? randn(Random.default_rng(), ComplexF64, N) : nothing     # src/Lanczos.jl:39
    vb = seed === nothing ? randn(Random.default_rng(), ComplexF64, N) : nothing
    check(ccall((:sd_energy_bounds, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, UInt64, Ref{Float64}, Ref{Float64}),
                model.ctx.h, model.h, lanc_m, va === nothing ? C_NULL : va, vb === nothing ? C_NULL : vb,
                seed === nothing ? 0 : seed, lo, hi), model.ctx.h)
    return lo[], hi[]
end

# The lowest k eigenpairs by thick-restart Lanczos in basis_size + 1 device vectors (sd_lanczos_eigenpairs; not in the reference,
# which stops at the ground state).  Returns (E, X, info): X is N x converged, info a NamedTuple of the fields of sd_eigs_info
# plus the residuals.  confirm=true looks for further copies of degenerate levels from fresh random vectors.
mutable struct EigsInfo      # sd_eigs_info
    converged::Cint
    restarts::Cint
    applies::Int64
    basis_size::Cint
    workspace_vectors::Cint
    next_level::Float64
    have_next_level::Cint
    scale::Float64
    EigsInfo() = new(0, 0, 0, 0, 0, 0.0, 0, 0.0)
end

function lowest_eigenpairs(model::Model; k::Int=4, basis_size::Union{Nothing,Int}=nothing, tol::Float64=1e-10,
                           max_applies::Int=200000, confirm::Bool=true, psi0::Union{Nothing,Vector{Float64}}=nothing,
                           seed::Integer=0)
    N = length(model)
    bs = basis_size === nothing ? min(N, max(2k + 8, 24)) : basis_size
    E = zeros(Float64, max(k, 1)); res = zeros(Float64, max(k, 1))
    X = zeros(Float64, N, max(k, 1))
    info = EigsInfo()
    check(ccall((:sd_lanczos_eigenpairs, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Float64, Int64, Cint, Ptr{Cvoid}, UInt64, Ptr{Float64}, Ptr{Cvoid},
                 Ptr{Float64}, Ref{EigsInfo}),
                model.ctx.h, model.h, dtype_code(Float64), k, bs, tol, max_applies, confirm ? 1 : 0,
                psi0 === nothing ? C_NULL : psi0, seed, E, X, res, info), model.ctx.h)
    nc = Int(info.converged)
    return E[1:nc], X[:, 1:nc], (converged=nc, restarts=Int(info.restarts), applies=info.applies, basis_size=Int(info.basis_size),
                                 workspace_vectors=Int(info.workspace_vectors), residuals=res[1:nc], scale=info.scale,
                                 next_level=info.have_next_level != 0 ? info.next_level : nothing)
end

# eigen(Symmetric(A)) by cyclic Jacobi rotations (sd_sym_eig, n <= 128) -> (w ascending, Z)
function sym_eig(A::Matrix{Float64})
    n = size(A, 1)
    w = Vector{Float64}(undef, n); Z = Matrix{Float64}(undef, n, n)
    check(ccall((:sd_sym_eig, libspindyn), Cint, (Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), n, A, w, Z))
    return w, Z
end

function time_evolve(model::Model, ψ0::AbstractVector, t::Real; method::Symbol=:krylov, Ebounds=nothing,
                     kry_m::Int=30, cheb_n::Int=100, seed::Union{Nothing,Integer}=nothing)
    N = length(ψ0)
    out = Vector{ComplexF64}(undef, N)
    if method === :krylov
        x = eltype(ψ0) <: Complex ? Vector{ComplexF64}(ψ0) : Vector{Float64}(ψ0)
        check(ccall((:sd_krylov_evolve, libspindyn), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Float64, Cint, Ptr{Cvoid}),
                    model.ctx.h, model.h, dtype_code(eltype(x)), x, N, Float64(t), kry_m, out), model.ctx.h)
        return out
    elseif method === :chebyshev
        eltype(ψ0) <: Complex || throw(ArgumentError("chebyshev needs a ComplexF64 ψ0 (src/TimeEvolution/Chebyshev.jl:36,98)"))
        bounds = Ebounds === nothing ? estimate_energy_bounds(model; seed=seed) : Ebounds
        x = Vector{ComplexF64}(ψ0)
        check(ccall((:sd_chebyshev_evolve, libspindyn), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Cint, Float64, Float64, Ptr{Cvoid}),
                    model.ctx.h, model.h, x, N, Float64(t), cheb_n, Float64(bounds[1]), Float64(bounds[2]), out), model.ctx.h)
        return out
    end
    throw(ArgumentError("unsupported time-evolution method: $method"))
end

# The sector S^-_q (op 2) or S^+_q (op 1) maps model's sector to: the model itself for the full basis, nothing when there is none.
function transverse_target(model::Model, op::Int)
    model.nup === nothing && return model
    t = model.nup + (op == 2 ? -1 : 1)
    (t < 0 || t > model.L) && return nothing
    return build_model(model.L; nup=t, hopping=model.hopping_list, onsite_field=model.onsite_field, zz=model.zz_list)
end

# S^{+-} (op 2), S^{-+} (op 1) as (W x Qn) column-major: sd_kpm_sqw_transverse / sd_lanczos_sqw_transverse on the adjacent sector
function transverse_rows(model::Model, x, q_list, ω_range, op::Int, method::Symbol, lanc_m, eta, br, have, a, b, kpm_m, kern, seed)
    S = zeros(Float64, length(ω_range), length(q_list))
    dst = transverse_target(model, op)
    dst === nothing && return S                                        # no target sector: phi = 0, zero rows
    if method === :lanczos
        check(ccall((:sd_lanczos_sqw_transverse, libspindyn), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Int64, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Cint,
                     Float64, Cint, Ptr{Float64}),
                    model.ctx.h, model.h, dst.h, op, dtype_code(eltype(x)), x, length(x), q_list, length(q_list), ω_range,
                    length(ω_range), lanc_m, eta, br, S), model.ctx.h)
    else
        check(ccall((:sd_kpm_sqw_transverse, libspindyn), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Int64, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Cint,
                     Float64, Float64, Cint, Cint, UInt64, Ptr{Float64}),
                    model.ctx.h, model.h, dst.h, op, dtype_code(eltype(x)), x, length(x), q_list, length(q_list), ω_range,
                    length(ω_range), have, have ? a : 0.0, have ? b : 0.0, kpm_m, kern, seed, S), model.ctx.h)
    end
    return S
end

function dynamical_structure_factor(model::Model, ψ0::AbstractVector, q::AbstractVector, ω::AbstractVector;
                                    method::Symbol=:lanczos, component::Symbol=:zz, lanc_m::Int=200, eta::Float64=0.05,
                                    broaden::Symbol=:lorentz, a::Union{Nothing,Float64}=nothing, b::Union{Nothing,Float64}=nothing,
                                    kpm_m::Int=200, kernel::Symbol=:jackson, seed::Integer=0,
                                    translation_invariant::Bool=false, source::Int=1, ti_tol::Float64=1e-6)
    q_list = Float64.(q); ω_range = Float64.(ω)
    x = eltype(ψ0) <: Complex ? Vector{ComplexF64}(ψ0) : Vector{Float64}(ψ0)
    S = Matrix{Float64}(undef, length(ω_range), length(q_list))      # C row-major (Qn x W) == Julia (W x Qn) column-major
    if component !== :zz
        # transverse spectra: S^{+-} (:pm), S^{-+} (:mp), S^{xx} = S^{yy} = (S^{+-} + S^{-+}) / 4 (:xx)
        ops = component === :pm ? (2,) : component === :mp ? (1,) : component === :xx ? (2, 1) :
              throw(ArgumentError("unknown component: $component; expected :zz, :pm, :mp or :xx"))
        method === :kpm_sites && throw(ArgumentError("method=:kpm_sites computes S^zz only (component=:zz)"))
        (method === :lanczos || method === :kpm) || throw(ArgumentError("unsupported dynamical structure-factor method: $method"))
        br = broaden === :lorentz ? 0 : broaden === :gauss ? 1 : error("unknown broadening: $broaden")
        have = a !== nothing && b !== nothing
        kern = kernel === :jackson ? 0 : kernel === :lorentz ? 1 : 2
        parts = [transverse_rows(model, x, q_list, ω_range, op, method, lanc_m, eta, br, have, a, b, kpm_m, kern, seed) for op in ops]
        S = length(parts) == 2 ? 0.25 .* (parts[1] .+ parts[2]) : parts[1]
        return permutedims(S)
    end
    if method === :kpm_sites                                           # S^zz from the site-resolved moments (kpm_sqw_sites)
        return kpm_sqw_sites(x, model, q_list, ω_range; a=a, b=b, kpm_m=kpm_m, kernel=kernel, seed=seed,
                             translation_invariant=translation_invariant, source=source, ti_tol=ti_tol)
    end
    if method === :lanczos
        br = broaden === :lorentz ? 0 : broaden === :gauss ? 1 : error("unknown broadening: $broaden")
        check(ccall((:sd_lanczos_sqw, libspindyn), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Cint, Float64, Cint, Ptr{Float64}),
                    model.ctx.h, model.h, dtype_code(eltype(x)), x, length(x), q_list, length(q_list), ω_range, length(ω_range),
                    lanc_m, eta, br, S), model.ctx.h)
    elseif method === :kpm
        have = a !== nothing && b !== nothing
        kern = kernel === :jackson ? 0 : kernel === :lorentz ? 1 : 2
        check(ccall((:sd_kpm_sqw, libspindyn), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Cint, Float64, Float64,
                     Cint, Cint, UInt64, Ptr{Float64}),
                    model.ctx.h, model.h, dtype_code(eltype(x)), x, length(x), q_list, length(q_list), ω_range, length(ω_range),
                    have, have ? a : 0.0, have ? b : 0.0, kpm_m, kern, seed, S), model.ctx.h)
    else
        throw(ArgumentError("unsupported dynamical structure-factor method: $method"))
    end
    return permutedims(S)                                              # (length(q), length(ω)) as the reference returns
end

# ---- site-resolved KPM correlations (the quantity of the reference's src/TimeEvolution/KPM.jl) -------------------------
# mu_n^{ij} = <psi0| S^z_i T_n(H~) S^z_j |psi0>: one recursion per source site j gives the moments against all L sites i.
# C row-major arrays come back as Julia column-major arrays with the index order reversed.
hostvec(ψ0::AbstractVector) = eltype(ψ0) <: Complex ? Vector{ComplexF64}(ψ0) : Vector{Float64}(ψ0)

# out[i] = <bra| S^z_i |ket> for every site i (one pass over both vectors)
function site_project(model::Model, bra::AbstractVector, ket::AbstractVector)
    b = hostvec(bra); k = Vector{ComplexF64}(ket)
    length(b) == length(k) || throw(DimensionMismatch("length(bra) != length(ket)"))
    out = Vector{ComplexF64}(undef, model.L)
    check(ccall((:sd_site_project, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}),
                model.ctx.h, model.h, dtype_code(eltype(b)), b, k, length(k), out), model.ctx.h)
    return out
end

# mu[i, n + 1, s] = mu_n^{i j_s}, j_s = sources[s] (1-based), n = 0..M-1
function kpm_site_moments(ψ0::AbstractVector, model::Model, M::Int, a::Real, b::Real; sources=collect(1:model.L))
    x = hostvec(ψ0); src = Cint.(sources)
    mu = Array{ComplexF64}(undef, model.L, M, length(src))
    check(ccall((:sd_kpm_site_moments, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cint}, Cint, Cint, Float64, Float64, Ptr{Float64}),
                model.ctx.h, model.h, dtype_code(eltype(x)), x, length(x), src, length(src), M, Float64(a), Float64(b), mu), model.ctx.h)
    return mu
end

# the unclamped reconstruction (real damped moments)
function kpm_reconstruct_signed(mu_damped::Vector{Float64}, ω::AbstractVector, a::Real, b::Real, E0::Real)
    ω_range = Float64.(ω)
    out = Vector{Float64}(undef, length(ω_range))
    check(ccall((:sd_kpm_reconstruct_signed, libspindyn), Cint,
                (Ptr{Float64}, Cint, Ptr{Float64}, Cint, Float64, Float64, Float64, Ptr{Float64}),
                mu_damped, length(mu_damped), ω_range, length(ω_range), Float64(a), Float64(b), Float64(E0), out))
    return out
end

# C[w, s, i] = <psi0| S^z_i delta(ω_w - (H - E0)) S^z_{j_s} |psi0>, not clamped (the reference's name; its defects are not
# reproduced: DESIGN.md 13)
function kpm_correlation_matrix(ψ0::AbstractVector, model::Model, ω::AbstractVector; sources=collect(1:model.L),
                                a::Union{Nothing,Float64}=nothing, b::Union{Nothing,Float64}=nothing, kpm_m::Int=200,
                                kernel::Symbol=:jackson, seed::Integer=0)
    x = hostvec(ψ0); src = Cint.(sources); ω_range = Float64.(ω)
    have = a !== nothing && b !== nothing
    kern = kernel === :jackson ? 0 : kernel === :lorentz ? 1 : 2
    Cm = Array{ComplexF64}(undef, length(ω_range), length(src), model.L)
    check(ccall((:sd_kpm_site_correlations, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cint}, Cint, Ptr{Float64}, Cint, Cint, Float64, Float64, Cint,
                 Cint, UInt64, Ptr{Float64}),
                model.ctx.h, model.h, dtype_code(eltype(x)), x, length(x), src, length(src), ω_range, length(ω_range), have,
                have ? a : 0.0, have ? b : 0.0, kpm_m, kern, seed, Cm), model.ctx.h)
    return Cm
end

# is the model unchanged by the cyclic shift i -> i + 1 (mod L)?
function shift_invariant(model::Model)
    L = model.L
    function table(bonds)
        t = Dict{Tuple{Int,Int},Float64}()
        for (i, j, J) in bonds
            i == j && continue
            key = (min(i, j), max(i, j))
            t[key] = get(t, key, 0.0) + J
        end
        return filter(kv -> kv.second != 0.0, t)
    end
    shifted(t) = Dict((min(mod1(i + 1, L), mod1(j + 1, L)), max(mod1(i + 1, L), mod1(j + 1, L))) => v for ((i, j), v) in t)
    for bonds in (model.hopping_list, model.zz_list)
        t = table(bonds)
        shifted(t) == t || return false
    end
    return all(==(first(model.onsite_field)), model.onsite_field)
end

# S^zz(q, ω) from the site moments -> (length(q), length(ω)), the rows kpm_sqw returns.  translation_invariant=true: ONE
# recursion from site `source` for all momenta (periodic chain, invariant ψ0); ArgumentError when the lists are not shift
# invariant or the invariance defect the library returns exceeds ti_tol.
function kpm_sqw_sites(ψ0::AbstractVector, model::Model, q::AbstractVector, ω::AbstractVector;
                       a::Union{Nothing,Float64}=nothing, b::Union{Nothing,Float64}=nothing, kpm_m::Int=200,
                       kernel::Symbol=:jackson, seed::Integer=0, translation_invariant::Bool=false, source::Int=1,
                       ti_tol::Float64=1e-6)
    x = hostvec(ψ0); q_list = Float64.(q); ω_range = Float64.(ω)
    if translation_invariant
        shift_invariant(model) || throw(ArgumentError("translation_invariant=true needs lists that the cyclic shift leaves unchanged"))
    end
    src = translation_invariant ? Cint[source] : Cint.(1:model.L)
    have = a !== nothing && b !== nothing
    kern = kernel === :jackson ? 0 : kernel === :lorentz ? 1 : 2
    S = Matrix{Float64}(undef, length(ω_range), length(q_list))
    defect = Ref{Float64}(0.0)
    check(ccall((:sd_kpm_sqw_sites, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Ptr{Cint}, Cint, Cint, Cint,
                 Float64, Float64, Cint, Cint, UInt64, Ptr{Float64}, Ref{Float64}),
                model.ctx.h, model.h, dtype_code(eltype(x)), x, length(x), q_list, length(q_list), ω_range, length(ω_range), src,
                length(src), translation_invariant, have, have ? a : 0.0, have ? b : 0.0, kpm_m, kern, seed, S, defect), model.ctx.h)
    if translation_invariant && !(defect[] <= ti_tol)
        throw(ArgumentError("psi0 is not translation invariant: defect $(defect[]) > ti_tol $ti_tol"))
    end
    return permutedims(S)
end

# ---- finite temperature by dynamical quantum typicality, with the spin current (DESIGN.md 14) -------------------------------
# The quantity of the reference's src/TimeEvolution/QuantumTypicality.jl (never included there, calls undefined names):
# ψ_β = exp(-βH/2) r, num_r(t) = <ψ_β(t)| A |φ(t)>, φ(t) = exp(-iHt) B ψ_β, <A(t)B>_β ≈ Σ_r num_r(t) / Σ_r |ψ_β|².
evolve_code(method::Symbol) = method === :chebyshev ? 0 : method === :krylov ? 1 :
    throw(ArgumentError("unknown evolution method: $method"))

# c_k = (2 - δ_k0) (-1)^k exp(-z) I_k(z), z = a τ; the first k with k > z and exp(-z) I_k(z) < 2^-53 exp(-z) I_0(z) terms
function chebyshev_imag_coeffs(a::Real, τ::Real; n_max::Int=4096)
    c = Vector{Float64}(undef, n_max)
    n_used = Ref{Cint}(0)
    check(ccall((:sd_chebyshev_imag_coeffs, libspindyn), Cint, (Cint, Float64, Float64, Ptr{Float64}, Ref{Cint}),
                n_max, Float64(a), Float64(τ), c, n_used))
    return c[1:n_used[]]
end

# the automatic real-time term count: the first k with k > |z| and |J_k(z)| < 2^-53, z = a Δt (|z| <= 1e6)
function chebyshev_terms(z::Real)
    n = Ref{Cint}(0)
    check(ccall((:sd_chebyshev_terms, libspindyn), Cint, (Float64, Ref{Cint}), Float64(z), n))
    return Int(n[])
end

# (exp(-βH/2) r / |.|, ln |exp(-βH/2) r|)
function thermal_state(model::Model, β::Real, r::AbstractVector; method::Symbol=:chebyshev, cheb_n::Int=0, kry_m::Int=30,
                       Ebounds::Union{Nothing,Tuple{Float64,Float64}}=nothing)
    x = Vector{ComplexF64}(r)
    out = Vector{ComplexF64}(undef, length(x))
    log_norm = Ref{Float64}(0.0)
    lo, hi = Ebounds === nothing ? (0.0, 0.0) : Ebounds
    check(ccall((:sd_imag_evolve, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Float64, Cint, Cint, Cint, Float64, Float64, Ptr{Cvoid}, Ref{Float64}),
                model.ctx.h, model.h, dtype_code(ComplexF64), x, length(x), Float64(β) / 2, evolve_code(method), cheb_n, kry_m, lo, hi,
                out, log_norm), model.ctx.h)
    return out, log_norm[]
end

current_weights(model::Model, weights) = weights === nothing ? Ptr{Float64}(C_NULL) :
    (length(weights) == length(model.hopping_list) ? Vector{Float64}(weights) :
     throw(ArgumentError("weights must have one entry per hop")))

# J_w ψ, J_w = Σ_b w_b i t_b (S⁺_i S⁻_j - S⁻_i S⁺_j) over the model's hop list (weights nothing: the total current)
function spin_current(ψ::AbstractVector, model::Model; weights=nothing)
    x = hostvec(ψ); w = current_weights(model, weights)
    out = Vector{ComplexF64}(undef, length(x))
    check(ccall((:sd_current_apply, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Cvoid}),
                model.ctx.h, model.h, dtype_code(eltype(x)), x, length(x), w, out), model.ctx.h)
    return out
end

# <bra| J_w |ket> without forming J_w ket
function current_expectation(bra::AbstractVector, ket::AbstractVector, model::Model; weights=nothing)
    b = hostvec(bra); k = Vector{ComplexF64}(ket); w = current_weights(model, weights)
    length(b) == length(k) || throw(DimensionMismatch("length(bra) != length(ket)"))
    out = Vector{Float64}(undef, 2)
    check(ccall((:sd_current_bracket, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}),
                model.ctx.h, model.h, dtype_code(eltype(b)), b, k, length(k), w, out), model.ctx.h)
    return complex(out[1], out[2])
end

# ---- energy current: lists of dressed bond currents (DESIGN.md 17) ----
# sd_dterm: the term c S^z_k j'_ij, j'_ij = i (S⁺_i S⁻_j - S⁻_i S⁺_j); k = 0: no S^z factor
struct DTerm
    i::Int32
    j::Int32
    k::Int32
    c::Float64
end

# The energy current J_E of the model's lists as a list of terms, sorted by (i, j, k); boundary :periodic: positions on a ring
function energy_current_terms(model::Model; boundary::Symbol=:open)
    boundary in (:open, :periodic) || throw(ArgumentError("boundary must be :open or :periodic"))
    per = boundary === :periodic ? 1 : 0
    n = Ref{Cint}(0)
    check(ccall((:sd_energy_current_terms, libspindyn), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Cint}),
                model.h, per, C_NULL, 0, n), model.ctx.h)
    out = Vector{DTerm}(undef, n[])
    n[] == 0 && return out
    check(ccall((:sd_energy_current_terms, libspindyn), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Cint}),
                model.h, per, out, length(out), n), model.ctx.h)
    return out
end

dterm_list(model::Model, terms, boundary) = terms === nothing ? energy_current_terms(model; boundary=boundary) :
    DTerm[DTerm(Int32(t[1]), Int32(t[2]), Int32(t[3]), Float64(t[4])) for t in terms]

# J ψ for a list of terms (i, j, k, c); terms nothing: the model's energy current
function energy_current(ψ::AbstractVector, model::Model; terms=nothing, boundary::Symbol=:open)
    x = hostvec(ψ); tl = dterm_list(model, terms, boundary)
    out = Vector{ComplexF64}(undef, length(x))
    check(ccall((:sd_dcurrent_apply, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}),
                model.ctx.h, model.h, dtype_code(eltype(x)), x, length(x), tl, length(tl), out), model.ctx.h)
    return out
end

# <bra| J |ket> without forming J ket
function energy_current_expectation(bra::AbstractVector, ket::AbstractVector, model::Model; terms=nothing, boundary::Symbol=:open)
    b = hostvec(bra); k = Vector{ComplexF64}(ket); tl = dterm_list(model, terms, boundary)
    length(b) == length(k) || throw(DimensionMismatch("length(bra) != length(ket)"))
    out = Vector{Float64}(undef, 2)
    check(ccall((:sd_dcurrent_bracket, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Ptr{Float64}),
                model.ctx.h, model.h, dtype_code(eltype(b)), b, k, length(k), tl, length(tl), out), model.ctx.h)
    return complex(out[1], out[2])
end

# Equal-time pair correlations of psi for all site pairs (DESIGN.md 15): component :pm gives <S^+_i S^-_j>, :zz gives <S^z_i S^z_j>;
# L x L ComplexF64, nothing divided by <psi|psi>
function pair_correlations(psi::AbstractVector, model::Model; component::Symbol=:zz)
    component in (:zz, :pm) || throw(ArgumentError("component must be :zz or :pm"))
    p = hostvec(psi)
    out = Vector{Float64}(undef, 2 * model.L * model.L)
    check(ccall((:sd_pair_correlations, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Cint, Ptr{Float64}),
                model.ctx.h, model.h, dtype_code(eltype(p)), p, length(p), component === :pm ? 1 : 0, out), model.ctx.h)
    return permutedims(reshape(reinterpret(ComplexF64, out), model.L, model.L))     # the ABI is row-major
end

# ---- S^z-basis statistics (DESIGN.md 20): one streaming pass over w_s = |psi_s|^2 each, nothing divided by <psi|psi> ----
# (sum w, sum w ln w, max w, its lowest row (1-based here), [sum w^q for q in qs]); at most 8 exponents, each > 0 and != 1
function basis_moments(psi::AbstractVector, model::Model, qs::AbstractVector{<:Real}=Float64[])
    p = hostvec(psi); q = Vector{Float64}(qs)
    out = Vector{Float64}(undef, 5 + length(q))
    check(ccall((:sd_basis_moments, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Float64}, Cint, Ptr{Float64}),
                model.ctx.h, model.h, dtype_code(eltype(p)), p, length(p), q, length(q), out), model.ctx.h)
    return (out[1], out[2], out[3], Int64(out[4]) + 1, out[6:end])
end

# S_q = ln(sum p^q) / (1 - q) of p = |psi_s|^2 / <psi|psi>; q = 1 the Shannon entropy, q = Inf -ln max p
function participation_entropy(psi::AbstractVector, model::Model; q::Real=2)
    q > 0 || throw(ArgumentError("q must be positive"))
    W, wlnw, wmax, _, sums = basis_moments(psi, model, (q == 1 || isinf(q)) ? Float64[] : [Float64(q)])
    q == 1 && return log(W) - wlnw / W
    isinf(q) && return -log(wmax / W)
    return log(sums[1] / W^q) / (1 - q)
end

site_mask(sites) = reduce(|, (UInt64(1) << (Int(i) - 1) for i in sites); init=UInt64(0))

# the values popcount(s & mask) takes on the basis: (m_min, n_bins)
function counting_range(model::Model, mask::UInt64)
    lo = Ref{Cint}(0); nb = Ref{Cint}(0)
    check(ccall((:sd_counting_range, libspindyn), Cint, (Ptr{Cvoid}, UInt64, Ptr{Cint}, Ptr{Cint}), model.h, mask, lo, nb), model.ctx.h)
    return (Int(lo[]), Int(nb[]))
end

# P[k, m + 1] = probability that subsystem k (a list of 1-based sites) holds m up spins, m = 0..L; at most 256 subsystems per call
function counting_statistics(psi::AbstractVector, model::Model, subsystems; normalize::Bool=true)
    p = hostvec(psi); masks = UInt64[site_mask(A) for A in subsystems]
    out = Vector{Float64}(undef, length(masks) * (model.L + 1))
    check(ccall((:sd_counting_statistics, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{UInt64}, Cint, Ptr{Float64}),
                model.ctx.h, model.h, dtype_code(eltype(p)), p, length(p), masks, length(masks), out), model.ctx.h)
    P = permutedims(reshape(out, model.L + 1, length(masks)))     # the ABI is row-major
    return normalize ? P ./ sum(P[1, :]) : P
end

function number_entropy(psi::AbstractVector, model::Model, subsystem)
    pm = filter(>(0), counting_statistics(psi, model, [subsystem])[1, :])
    return -sum(pm .* log.(pm))
end

# ---- entanglement across a chain cut (DESIGN.md 21): the blocks of rho_A / rho_B as Gram matrices, nothing divided by <psi|psi> ----
struct CutBlock          # sd_cut_block
    m::Int32             # up spins in sites 1..cut (-1: the one block of the full basis)
    side::Int32          # 0 = A (sites 1..cut), 1 = B: the side in effect
    dA::Int64
    dB::Int64
    d::Int64             # dimension of the block on that side
    offset::Int64        # matrix elements before the block in the packed output
end

cut_side(side::Symbol) = side === :A ? Cint(0) : side === :B ? Cint(1) : side === :auto ? Cint(2) : throw(ArgumentError("side must be :A, :B or :auto"))

# the blocks of the reduced density matrix across the cut between sites cut and cut + 1, and the matrix elements of all of them
function cut_blocks(model::Model, cut::Integer; side::Symbol=:auto)
    nb = Ref{Cint}(0); ne = Ref{Int64}(0)
    check(ccall((:sd_cut_blocks, libspindyn), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Int64}),
                model.h, cut, cut_side(side), C_NULL, 0, nb, ne), model.ctx.h)
    out = Vector{CutBlock}(undef, nb[])
    check(ccall((:sd_cut_blocks, libspindyn), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Int64}),
                model.h, cut, cut_side(side), out, nb[], nb, ne), model.ctx.h)
    return (out, ne[])
end

# Dict(m => G_m): side A G_m = Psi_m Psi_m' over the prefixes of popcount m, side B transpose(Psi_m) conj(Psi_m) over the suffixes,
# rows in basis order; Hermitian (ComplexF64) or symmetric (Float64) to the bit
function cut_gram(psi::AbstractVector, model::Model, cut::Integer; side::Symbol=:auto)
    p = hostvec(psi)
    blocks, ne = cut_blocks(model, cut; side=side)
    out = Vector{eltype(p)}(undef, ne)
    check(ccall((:sd_cut_gram, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cvoid}),
                model.ctx.h, model.h, dtype_code(eltype(p)), p, length(p), cut, cut_side(side), out), model.ctx.h)
    # the ABI is row-major; every block equals its conjugate transpose, so the column-major reshape is conj(G_m)
    return Dict(Int(b.m) => conj.(reshape(out[b.offset + 1:b.offset + b.d * b.d], Int(b.d), Int(b.d))) for b in blocks)
end

# ---- site permutations and the entanglement of any set of sites (DESIGN.md 22) ----
# U_pi psi: perm[i] is the site to which the spin of site i moves (1-based, a bijection of 1:L); every entry is one entry of psi
function permute_sites(psi::AbstractVector, model::Model, perm::AbstractVector{<:Integer})
    p = hostvec(psi)
    out = similar(p)
    pm = Vector{Cint}(perm)
    length(pm) == model.L || throw(ArgumentError("perm must have L entries"))
    check(ccall((:sd_site_permute, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cint}, Ptr{Cvoid}),
                model.ctx.h, model.h, dtype_code(eltype(p)), p, length(p), pm, out), model.ctx.h)
    return out
end

# the row of psi (1-based) that each of the rows first .. first + count - 1 (1-based) of U_pi psi copies (host only)
function site_permute_sources(model::Model, perm::AbstractVector{<:Integer}, first::Integer, count::Integer)
    pm = Vector{Cint}(perm)
    length(pm) == model.L || throw(ArgumentError("perm must have L entries"))
    rows = Vector{Int64}(undef, count)
    check(ccall((:sd_site_permute_sources, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cint}, Int64, Int64, Ptr{Int64}),
                model.h, pm, first - 1, count, rows), model.ctx.h)
    return rows .+ 1
end

# the permutation that brings sites[j] to site j, in the order given, and the other sites to length(sites)+1:L in ascending order
function subsystem_permutation(L::Integer, sites::AbstractVector{<:Integer})
    s = Vector{Cint}(sites)
    out = Vector{Cint}(undef, max(L, 1))
    check(ccall((:sd_subsystem_permutation, libspindyn), Cint, (Cint, Ptr{Cint}, Cint, Ptr{Cint}), L, s, length(s), out), C_NULL)
    return Int.(out[1:L])
end

# Dict(m => G_m) of the listed sites: the blocks of cut_gram at cut = length(sites) with sites[j] playing site j
function subsystem_gram(psi::AbstractVector, model::Model, sites::AbstractVector{<:Integer}; side::Symbol=:auto)
    p = hostvec(psi)
    s = Vector{Cint}(sites)
    blocks, ne = cut_blocks(model, length(s); side=side)
    out = Vector{eltype(p)}(undef, ne)
    check(ccall((:sd_subsystem_gram, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cint}, Cint, Cint, Ptr{Cvoid}),
                model.ctx.h, model.h, dtype_code(eltype(p)), p, length(p), s, length(s), cut_side(side), out), model.ctx.h)
    return Dict(Int(b.m) => conj.(reshape(out[b.offset + 1:b.offset + b.d * b.d], Int(b.d), Int(b.d))) for b in blocks)
end

# the uniforms of shots first .. first + n - 1 of stream `seed` (0-based shot numbers)
function sample_uniforms(seed::Integer, first::Integer, n::Integer)
    u = Vector{Float64}(undef, n)
    check(ccall((:sd_sample_uniforms_host, libspindyn), Cint, (UInt64, UInt64, Int64, Ptr{Float64}), seed, first, n, u), C_NULL)
    return u
end

# projective snapshots: (configurations::Vector{UInt64}, rows (1-based)) drawn from |psi_s|^2 / <psi|psi>
function sample_configurations(psi::AbstractVector, model::Model, shots::Integer; seed::Integer=0)
    p = hostvec(psi)
    rows = Vector{Int64}(undef, shots); cfg = Vector{UInt64}(undef, shots)
    check(ccall((:sd_sample_configurations, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, UInt64, Ptr{Int64}, Ptr{UInt64}),
                model.ctx.h, model.h, dtype_code(eltype(p)), p, length(p), shots, seed, rows, cfg), model.ctx.h)
    return (cfg, rows .+ 1)
end

# bonds: a vector of (i, j) site pairs (1-based, i != j), or nothing for the distinct site pairs of the model's hopping list in list order
function bond_list(model::Model, bonds)
    bonds === nothing || return [(Int(b[1]), Int(b[2])) for b in bonds]
    seen = Set{Tuple{Int,Int}}(); out = Tuple{Int,Int}[]
    for h in model.hopping_list
        key = (min(h[1], h[2]), max(h[1], h[2]))
        if h[1] != h[2] && !(key in seen)
            push!(seen, key); push!(out, (Int(h[1]), Int(h[2])))
        end
    end
    return out
end

# D_b psi for the bond b = (i, j): D_b = xy/2 (S^+_i S^-_j + S^-_i S^+_j) + zz S^z_i S^z_j (xy = zz = 1: S_i . S_j)  (DESIGN.md 16)
function bond_operator(psi::AbstractVector, model::Model, i::Integer, j::Integer; xy::Real=1.0, zz::Real=1.0)
    p = hostvec(psi)
    out = similar(p)
    check(ccall((:sd_bond_apply, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Cint, Cint, Float64, Float64, Ptr{Cvoid}),
                model.ctx.h, model.h, dtype_code(eltype(p)), p, length(p), i, j, Float64(xy), Float64(zz), out), model.ctx.h)
    return out
end

# Dimer correlations of psi for a list of B bonds from one pass: (D, e), D[a, b] = <psi| D_a D_b |psi> (B x B ComplexF64, Hermitian),
# e[b] = <psi| D_b |psi>; nothing divided by <psi|psi>
function dimer_correlations(psi::AbstractVector, model::Model; bonds=nothing, xy::Real=1.0, zz::Real=1.0)
    bl = bond_list(model, bonds)
    B = length(bl)
    flat = Cint[x for b in bl for x in b]
    p = hostvec(psi)
    D = Vector{Float64}(undef, 2 * B * B)
    e = Vector{Float64}(undef, B)
    check(ccall((:sd_dimer_correlations, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cint}, Cint, Float64, Float64, Ptr{Float64}, Ptr{Float64}),
                model.ctx.h, model.h, dtype_code(eltype(p)), p, length(p), flat, B, Float64(xy), Float64(zz), D, e), model.ctx.h)
    return permutedims(reshape(reinterpret(ComplexF64, D), B, B)), e     # the ABI is row-major
end

# ---- lattice symmetry operators (DESIGN.md 18): U_g = T^shift R^reflect Z^flip, code = shift | reflect << 8 | flip << 9 ----
symmetry_code(model::Model; shift::Integer=0, reflect::Bool=false, flip::Bool=false) =
    Cint(mod(shift, model.L) | (reflect ? 256 : 0) | (flip ? 512 : 0))

# are the hop, zz and field lists invariant under U_g?  (host only)
function is_symmetric(model::Model; kw...)
    yes = Ref{Cint}(0)
    check(ccall((:sd_model_symmetric, libspindyn), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}), model.h, symmetry_code(model; kw...), yes),
          model.ctx.h)
    return yes[] != 0
end

# U_g psi, or with y the fused U_g psi + c y; a vector of psi's element type
function symmetry_apply(psi::AbstractVector, model::Model; y::Union{Nothing,AbstractVector}=nothing, c::Number=1.0, kw...)
    p = hostvec(psi)
    out = similar(p)
    (y === nothing || length(y) == length(p)) || throw(DimensionMismatch("length(y) != length(psi)"))
    yy = y === nothing ? Ptr{Cvoid}(C_NULL) : Vector{eltype(p)}(y)
    check(ccall((:sd_symmetry_apply, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Cint, Ptr{Cvoid}, Float64, Float64, Ptr{Cvoid}),
                model.ctx.h, model.h, dtype_code(eltype(p)), p, length(p), symmetry_code(model; kw...), yy, Float64(real(c)),
                Float64(imag(c)), out), model.ctx.h)
    return out
end
translate(psi::AbstractVector, model::Model, r::Integer=1) = symmetry_apply(psi, model; shift=r)
reflect(psi::AbstractVector, model::Model) = symmetry_apply(psi, model; reflect=true)
spin_flip(psi::AbstractVector, model::Model) = symmetry_apply(psi, model; flip=true)

# <bra|U_g|psi> for a vector of element codes (symmetry_code) from one pass; bra nothing: psi itself
function symmetry_overlaps(psi::AbstractVector, model::Model, codes::AbstractVector{<:Integer}; bra::Union{Nothing,AbstractVector}=nothing)
    (bra === nothing || length(bra) == length(psi)) || throw(DimensionMismatch("length(bra) != length(psi)"))
    k = bra === nothing ? hostvec(psi) : Vector{ComplexF64}(psi)
    b = bra === nothing ? Ptr{Cvoid}(C_NULL) : Vector{ComplexF64}(bra)
    cl = Vector{Cint}(codes)
    out = Vector{Float64}(undef, 2 * length(cl))
    check(ccall((:sd_symmetry_overlaps, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cint}, Cint, Ptr{Float64}),
                model.ctx.h, model.h, dtype_code(eltype(k)), b, k, length(k), cl, length(cl), out), model.ctx.h)
    return collect(reinterpret(ComplexF64, out))
end

# w_n = <psi|P_n|psi>, n = 0..L-1, P_n = (1/L) sum_r e^{+i k_n r} T^r
function momentum_weights(psi::AbstractVector, model::Model)
    L = model.L
    ov = symmetry_overlaps(psi, model, [symmetry_code(model; shift=r) for r in 0:L-1])
    return [real(sum(cis(2pi * n * r / L) * ov[r + 1] for r in 0:L-1)) / L for n in 0:L-1]
end

# sum_k coef[k] U_{codes[k]} psi in one pass (ComplexF64)
function symmetry_combine(psi::AbstractVector, model::Model, codes::AbstractVector{<:Integer}, coef::AbstractVector{<:Number})
    p = hostvec(psi)
    cl = Vector{Cint}(codes)
    cf = collect(reinterpret(Float64, Vector{ComplexF64}(coef)))
    out = Vector{ComplexF64}(undef, length(p))
    check(ccall((:sd_symmetry_project, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cint}, Ptr{Float64}, Cint, Cint, Ptr{Cvoid}),
                model.ctx.h, model.h, dtype_code(eltype(p)), p, length(p), cl, cf, length(cl), 2, out), model.ctx.h)
    return out
end

# P psi: momentum n (P_n), parity +-1 ((1 +- R)/2), spin_flip +-1 ((1 +- Z)/2); parity with momentum only at n = 0 and n = L/2
function symmetry_project(psi::AbstractVector, model::Model; momentum::Union{Nothing,Integer}=nothing,
                          parity::Union{Nothing,Integer}=nothing, spin_flip::Union{Nothing,Integer}=nothing)
    L = model.L
    (momentum === nothing || 0 <= momentum < L) || throw(ArgumentError("momentum must be in 0..L-1"))
    (parity === nothing || momentum === nothing || momentum == 0 || 2 * momentum == L) ||
        throw(ArgumentError("parity combines with momentum only at n = 0 and n = L/2"))
    codes = Cint[]; coef = ComplexF64[]
    for r in (momentum === nothing ? (0:0) : (0:L-1)), refl in (parity === nothing ? (0:0) : (0:1)), fl in (spin_flip === nothing ? (0:0) : (0:1))
        c = momentum === nothing ? complex(1.0) : cis(2pi * momentum * r / L) / L
        c *= parity === nothing ? 1.0 : 0.5 * (refl == 1 ? parity : 1)
        c *= spin_flip === nothing ? 1.0 : 0.5 * (fl == 1 ? spin_flip : 1)
        push!(codes, Cint(r | (refl << 8) | (fl << 9))); push!(coef, c)
    end
    return symmetry_combine(psi, model, codes, coef)
end

# ---- operator strings: any product of S^+, S^-, S^z, and sums of such products (DESIGN.md 19) ----
# sd_opterm: c prod_{plus} S^+ prod_{minus} S^- prod_{z} S^z as a term of operator `op`; site i is bit i - 1 of the masks
struct OpTerm
    plus::UInt64
    minus::UInt64
    z::UInt64
    c_re::Float64
    c_im::Float64
    op::Int32
    reserved::Int32
end

sitebit(i::Integer) = UInt64(1) << (i - 1)

# coeff * the product of the factors (:+, i), (:-, j), (:z, k), (:x, a), (:y, b) on distinct sites as a list of terms of operator
# `op`; S^x = (S^+ + S^-)/2 and S^y = (S^+ - S^-)/(2i) are expanded here (the S^+ choice first)
function op_string(coeff::Number, factors...; op::Integer=0)
    plus = UInt64(0); minus = UInt64(0); z = UInt64(0); seen = UInt64(0)
    xy = Tuple{Symbol,UInt64}[]
    for (kind, site) in factors
        b = sitebit(site)
        (seen & b) == 0 || throw(ArgumentError("site $site appears twice in one string"))
        seen |= b
        if kind === :+
            plus |= b
        elseif kind === :-
            minus |= b
        elseif kind === :z
            z |= b
        elseif kind === :x || kind === :y
            push!(xy, (kind, b))
        else
            throw(ArgumentError("unknown factor $kind: expected :+, :-, :z, :x or :y"))
        end
    end
    out = OpTerm[]
    for choice in 0:(1 << length(xy)) - 1
        p = plus; m = minus; c = ComplexF64(coeff)
        for (n, (kind, b)) in enumerate(xy)
            lower = (choice >> (length(xy) - n)) & 1 == 1
            if lower
                m |= b
                c = kind === :x ? 0.5 * c : complex(-0.5 * imag(c), 0.5 * real(c))
            else
                p |= b
                c = kind === :x ? 0.5 * c : complex(0.5 * imag(c), -0.5 * real(c))
            end
        end
        push!(out, OpTerm(p, m, z, real(c), imag(c), Int32(op), Int32(0)))
    end
    return out
end

operator_adjoint(terms::Vector{OpTerm}) = OpTerm[OpTerm(t.minus, t.plus, t.z, t.c_re, -t.c_im, t.op, Int32(0)) for t in terms]

# (K, hermitian) of a list against a model: K = 1 + the largest op
function operator_check(model::Model, terms::Vector{OpTerm})
    k = Ref{Cint}(0); h = Ref{Cint}(0)
    check(ccall((:sd_opstring_check, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Cint}),
                model.h, terms, length(terms), k, h), model.ctx.h)
    return Int(k[]), h[] != 0
end

# the model's hop, zz and field lists as strings of op 0, in list order
function hamiltonian_terms(model::Model)
    n = Ref{Cint}(0)
    check(ccall((:sd_hamiltonian_terms, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cint}), model.h, C_NULL, 0, n), model.ctx.h)
    out = Vector{OpTerm}(undef, n[])
    n[] == 0 && return out
    check(ccall((:sd_hamiltonian_terms, libspindyn), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cint}), model.h, out, length(out), n), model.ctx.h)
    return out
end

# O psi for a list whose terms all have op = 0 (ComplexF64), or O psi + b y with y
function operator_apply(psi::AbstractVector, model::Model, terms::Vector{OpTerm}; y::Union{Nothing,AbstractVector}=nothing, b::Number=1.0)
    x = hostvec(psi)
    (y === nothing || length(y) == length(x)) || throw(DimensionMismatch("length(y) != length(psi)"))
    yv = y === nothing ? Ptr{Cvoid}(C_NULL) : Vector{ComplexF64}(y)
    out = Vector{ComplexF64}(undef, length(x))
    check(ccall((:sd_opstring_apply, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Float64, Float64, Cint, Ptr{Cvoid}),
                model.ctx.h, model.h, dtype_code(eltype(x)), x, length(x), terms, length(terms), yv, Float64(real(b)), Float64(imag(b)), 2, out),
          model.ctx.h)
    return out
end

# <bra|O_k|ket> for the K operators of the list from one pass; bra nothing: ket itself
function operator_expectations(ket::AbstractVector, model::Model, terms::Vector{OpTerm}; bra::Union{Nothing,AbstractVector}=nothing)
    (bra === nothing || length(bra) == length(ket)) || throw(DimensionMismatch("length(bra) != length(ket)"))
    k = bra === nothing ? hostvec(ket) : Vector{ComplexF64}(ket)
    b = bra === nothing ? Ptr{Cvoid}(C_NULL) : Vector{ComplexF64}(bra)
    K = isempty(terms) ? 0 : Int(maximum(t.op for t in terms)) + 1
    out = zeros(Float64, 2 * max(K, 1))
    check(ccall((:sd_opstring_expect, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Ptr{Float64}),
                model.ctx.h, model.h, dtype_code(eltype(k)), b, k, length(k), terms, length(terms), out), model.ctx.h)
    return collect(reinterpret(ComplexF64, out))[1:K]
end

# -<S^z_i exp(i pi sum_{i<l<j} S^z_l) S^z_j>: one diagonal term, exp(i pi S^z) = 2i S^z
function string_order(psi::AbstractVector, model::Model, i::Integer, j::Integer)
    1 <= i < j || throw(ArgumentError("string_order needs sites 1 <= i < j"))
    return operator_expectations(psi, model, op_string(-(2im)^(j - i - 1), [(:z, l) for l in i:j]...))[1]
end

# operator descriptors: (:Sz, site), (:Szq, q), :Sz_all (operator_i only), (:current, weights | nothing),
# (:energy_current, :open | :periodic) -> (kind, parameter, weights)
function dqt_operator(model::Model, op)
    op === :Sz_all && return (2, 0.0, Ptr{Float64}(C_NULL))
    op isa Tuple && length(op) == 2 || throw(ArgumentError("unknown operator: $op"))
    op[1] === :Sz && return (0, Float64(op[2]), Ptr{Float64}(C_NULL))
    op[1] === :Szq && return (1, Float64(op[2]), Ptr{Float64}(C_NULL))
    op[1] === :current && return (3, 0.0, current_weights(model, op[2]))
    if op[1] === :energy_current
        op[2] in (:open, :periodic) || throw(ArgumentError("(:energy_current, boundary) takes :open or :periodic"))
        return (4, op[2] === :periodic ? 1.0 : 0.0, Ptr{Float64}(C_NULL))
    end
    throw(ArgumentError("unknown operator: $op"))
end

# One sample: (num[i, k] for the normalised ψ_β, den = |ψ_β|², energy, log_norm); r nothing: the counter-based stream of `seed`.
function typicality_sample(model::Model, β::Real, operator_i, operator_j, t_range::AbstractVector; method::Symbol=:chebyshev,
                           r::Union{Nothing,AbstractVector}=nothing, seed::Integer=0, cheb_n::Int=0, kry_m::Int=30,
                           Ebounds::Union{Nothing,Tuple{Float64,Float64}}=nothing)
    Ak, Ap, Aw = dqt_operator(model, operator_i)
    Bk, Bp, Bw = dqt_operator(model, operator_j)
    Bk == 2 && throw(ArgumentError(":Sz_all is for operator_i only"))
    times = Float64.(t_range)
    nA = Ak == 2 ? model.L : 1
    num = Matrix{ComplexF64}(undef, nA, length(times))
    den = Ref{Float64}(0.0); energy = Ref{Float64}(0.0); log_norm = Ref{Float64}(0.0)
    rr = r === nothing ? Ptr{Cvoid}(C_NULL) : Vector{ComplexF64}(r)
    lo, hi = Ebounds === nothing ? (0.0, 0.0) : Ebounds
    check(ccall((:sd_dqt_correlations, libspindyn), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ptr{Cvoid}, UInt64, Cint, Float64, Ptr{Float64}, Cint, Float64, Ptr{Float64},
                 Ptr{Float64}, Cint, Cint, Cint, Cint, Float64, Float64, Ptr{Float64}, Ref{Float64}, Ref{Float64}, Ref{Float64}),
                model.ctx.h, model.h, Float64(β), rr, seed, Bk, Bp, Bw, Ak, Ap, Aw, times, length(times), evolve_code(method), cheb_n,
                kry_m, lo, hi, num, den, energy, log_norm), model.ctx.h)
    return num, den[], energy[], log_norm[]
end

# <A(t)B>_β ≈ Σ_r num_r(t) / Σ_r den_r over n_samples start vectors (sample k: seed + k) -> (length(t_range),) or (L, length(t_range))
function typicality_correlation_function(model::Model, β::Real, operator_i, operator_j, t_range::AbstractVector;
                                         method::Symbol=:chebyshev, n_samples::Int=1, seed::Integer=0, kw...)
    samples = [typicality_sample(model, β, operator_i, operator_j, t_range; method=method, seed=seed + k, kw...) for k in 0:n_samples-1]
    shift = maximum(s[4] for s in samples)
    wgt = [exp(2 * (s[4] - shift)) for s in samples]
    C = sum(wgt[k] .* samples[k][1] for k in 1:n_samples) ./ sum(wgt)
    return operator_i === :Sz_all ? C : vec(C)
end

# ---- driven dynamics: H(t) = H0 + Σ_k f_k(t) D_k with diagonal drives (include/spindyn.h, "driven dynamics"; DESIGN.md 24) ----
# D = Σ_i site_weights[i] Sᶻ_i + Σ_b bond_weights[b] Sᶻ_i Sᶻ_j over bonds[b] = (i, j), sites 1-based; either part may be missing.
struct DiagonalDrive
    site_weights::Union{Nothing,Vector{Float64}}
    zz_i::Vector{Cint}
    zz_j::Vector{Cint}
    bond_weights::Vector{Float64}
end
function DiagonalDrive(; site_weights=nothing, bonds=Tuple{Int,Int}[], bond_weights=nothing)
    w = bond_weights === nothing ? ones(Float64, length(bonds)) : Vector{Float64}(bond_weights)
    length(w) == length(bonds) || throw(ArgumentError("bond_weights must have one entry per bond"))
    return DiagonalDrive(site_weights === nothing ? nothing : Vector{Float64}(site_weights), Cint[b[1] for b in bonds],
                         Cint[b[2] for b in bonds], w)
end
field_drive(model::Model; weights=nothing) = DiagonalDrive(site_weights=weights === nothing ? ones(model.L) : weights)
gradient_drive(model::Model) = DiagonalDrive(site_weights=collect(1:model.L) .- (model.L + 1) / 2)
zz_drive(model::Model; bonds=nothing, weights=nothing) =
    DiagonalDrive(bonds=bonds === nothing ? [(b[1], b[2]) for b in model.zz_list] : bonds, bond_weights=weights)

struct CDrive                # sd_drive
    site_w::Ptr{Float64}
    n_zz::Cint
    zz_i::Ptr{Cint}
    zz_j::Ptr{Cint}
    zz_w::Ptr{Float64}
end
mutable struct DrivenInfo    # sd_driven_info
    stages::Cint
    applies::Int64
    min_beta::Float64
    DrivenInfo() = new(0, 0, Inf)
end
# the sd_drive array of a list; the pointers are into the drives' own arrays: keep `drives` alive (GC.@preserve) while it is in use
function pack_drives(model::Model, drives::Vector{DiagonalDrive})
    for d in drives
        d.site_weights === nothing || length(d.site_weights) == model.L || throw(ArgumentError("site_weights needs L entries"))
    end
    return CDrive[CDrive(d.site_weights === nothing ? Ptr{Float64}(C_NULL) : pointer(d.site_weights), length(d.zz_i), pointer(d.zz_i),
                         pointer(d.zz_j), pointer(d.bond_weights)) for d in drives]
end

function drive_check(model::Model, drives::Vector{DiagonalDrive})
    GC.@preserve drives begin
        arr = pack_drives(model, drives)
        check(ccall((:sd_drive_check, libspindyn), Cint, (Ptr{Cvoid}, Ptr{CDrive}, Cint), model.h, arr, length(arr)), model.ctx.h)
    end
    return nothing
end

# (Σ_k coefs[k] D_k) ψ, plus y when given
function diagonal_apply(ψ::Vector{T}, model::Model, drives::Vector{DiagonalDrive}, coefs::AbstractVector;
                        y::Union{Nothing,Vector{T}}=nothing) where {T<:Union{Float64,ComplexF64}}
    out = similar(ψ)
    c = Vector{Float64}(coefs)
    GC.@preserve drives begin
        arr = pack_drives(model, drives)
        check(ccall((:sd_diag_apply, libspindyn), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{CDrive}, Cint, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}),
                    model.ctx.h, model.h, dtype_code(T), ψ, length(ψ), arr, length(arr), c, y === nothing ? C_NULL : y, out), model.ctx.h)
    end
    return out
end

# out = (H0 + Σ_k coefs[k] D_k) ψ
function driven_apply(out::Vector{T}, ψ::Vector{T}, model::Model, drives::Vector{DiagonalDrive},
                      coefs::AbstractVector) where {T<:Union{Float64,ComplexF64}}
    c = Vector{Float64}(coefs)
    GC.@preserve drives begin
        arr = pack_drives(model, drives)
        check(ccall((:sd_driven_apply, libspindyn), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{CDrive}, Cint, Ptr{Float64}, Ptr{Cvoid}),
                    model.ctx.h, model.h, dtype_code(T), ψ, length(ψ), arr, length(arr), c, out), model.ctx.h)
    end
    return out
end

# (tau, coef): order 2 the midpoint rule; order 4 the commutator-free Magnus scheme of Alvermann and Fehske, two stages of dt/2 per
# step, the earlier one with c = 2 (α₂ f(t₁) + α₁ f(t₂)), the later one with c = 2 (α₁ f(t₁) + α₂ f(t₂)).  coef is K x stages
# (column-major: stage s holds coef[:, s], which is the layout sd_driven_evolve reads).
function magnus_schedule(functions::Vector, t0::Real, dt::Real, n_steps::Int; order::Int=4)
    order in (2, 4) || throw(ArgumentError("order must be 2 or 4"))
    K = length(functions)
    per = order == 2 ? 1 : 2
    tau = fill(Float64(dt) / per, per * n_steps)
    coef = zeros(Float64, K, per * n_steps)
    a1, a2 = (3 - 2 * sqrt(3)) / 12, (3 + 2 * sqrt(3)) / 12
    for s in 0:n_steps-1
        t = t0 + s * dt
        if order == 2
            coef[:, s+1] = [Float64(f(t + dt / 2)) for f in functions]
        else
            f1 = [Float64(f(t + (1 / 2 - sqrt(3) / 6) * dt)) for f in functions]
            f2 = [Float64(f(t + (1 / 2 + sqrt(3) / 6) * dt)) for f in functions]
            coef[:, 2s+1] = 2 .* (a2 .* f1 .+ a1 .* f2)
            coef[:, 2s+2] = 2 .* (a1 .* f1 .+ a2 .* f2)
        end
    end
    return tau, coef
end

# segments = [(duration, [c_1, ..., c_K]), ...]: a protocol that is constant on intervals
function piecewise_schedule(segments::Vector)
    tau = Float64[s[1] for s in segments]
    coef = zeros(Float64, length(segments[1][2]), length(segments))
    for (k, s) in enumerate(segments)
        coef[:, k] = s[2]
    end
    return tau, coef
end

# ψ <- exp(-i tau[s] (H0 + Σ_k coef[k, s] D_k)) ψ for every stage in one call -> (ψ, info)
function stage_evolve(model::Model, ψ0::AbstractVector, drives::Vector{DiagonalDrive}, tau::Vector{Float64}, coef::Matrix{Float64};
                      kry_m::Int=30)
    x = eltype(ψ0) <: Complex ? Vector{ComplexF64}(ψ0) : Vector{Float64}(ψ0)
    size(coef) == (length(drives), length(tau)) || throw(ArgumentError("coef must be K x stages"))
    out = Vector{ComplexF64}(undef, length(x))
    info = DrivenInfo()
    GC.@preserve drives begin
        arr = pack_drives(model, drives)
        check(ccall((:sd_driven_evolve, libspindyn), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{CDrive}, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Cvoid},
                     Ref{DrivenInfo}),
                    model.ctx.h, model.h, dtype_code(eltype(x)), x, length(x), arr, length(arr), length(tau), tau, coef, kry_m, out,
                    info), model.ctx.h)
    end
    return out, (stages=Int(info.stages), applies=info.applies, min_beta=info.min_beta)
end

# ψ(t0 + n_steps dt) under H(t) = H0 + Σ_k functions[k](t) D_k; measure(t, ψ) is called at t0 and after every measure_every steps
function driven_time_evolve(model::Model, ψ0::AbstractVector, drives::Vector{DiagonalDrive}, functions::Vector, t0::Real, dt::Real,
                            n_steps::Int; order::Int=4, kry_m::Int=30, measure=nothing, measure_every::Int=1)
    tau, coef = magnus_schedule(functions, t0, dt, n_steps; order=order)
    per = length(tau) ÷ n_steps
    ψ = ψ0
    results = Any[]
    measure === nothing || push!(results, measure(Float64(t0), ψ))
    done = 0
    while done < n_steps
        k = measure === nothing ? n_steps : min(measure_every, n_steps - done)
        rng = per*done+1:per*(done+k)
        ψ, _ = stage_evolve(model, ψ, drives, tau[rng], coef[:, rng]; kry_m=kry_m)
        done += k
        measure === nothing || push!(results, measure(t0 + done * dt, ψ))
    end
    return ψ, results
end

# ---- hopping drives: B = Σ_b (z_b S⁺_i S⁻_j + conj(z_b) S⁻_i S⁺_j) beside the diagonal ones (include/spindyn.h, "hopping drives";
# DESIGN.md 25) ----
# bonds[b] = (i, j), sites 1-based, i ≠ j in either orientation; complex weights.  Real weights travel without an im list, so a call
# whose hopping drives are all real runs in real form.
struct HoppingDrive
    hi::Vector{Cint}
    hj::Vector{Cint}
    re::Vector{Float64}
    im::Union{Nothing,Vector{Float64}}
end
function HoppingDrive(bonds, weights=nothing)
    w = weights === nothing ? ones(ComplexF64, length(bonds)) : Vector{ComplexF64}(weights)
    length(w) == length(bonds) || throw(ArgumentError("weights needs one entry per bond"))
    return HoppingDrive(Cint[b[1] for b in bonds], Cint[b[2] for b in bonds], real.(w), all(iszero, imag.(w)) ? nothing : imag.(w))
end
# the model's own hop bonds with their own amplitudes: f(t) is the relative modulation δJ/J
exchange_drive(model::Model) = HoppingDrive([(b[1], b[2]) for b in model.hopping_list], [b[3] for b in model.hopping_list])
# z_b = i w_b t_b: the operator of spin_current
current_drive(model::Model; weights=nothing) =
    HoppingDrive([(b[1], b[2]) for b in model.hopping_list],
                 [im * (weights === nothing ? 1.0 : weights[k]) * b[3] for (k, b) in enumerate(model.hopping_list)])

struct CHopDrive             # sd_hop_drive
    n::Cint
    i::Ptr{Cint}
    j::Ptr{Cint}
    re::Ptr{Float64}
    im::Ptr{Float64}
end
# the sd_hop_drive array of a list; the pointers are into the drives' own arrays: keep `hops` alive (GC.@preserve) while it is in use
pack_hops(hops::Vector{HoppingDrive}) =
    CHopDrive[CHopDrive(length(d.hi), pointer(d.hi), pointer(d.hj), pointer(d.re), d.im === nothing ? Ptr{Float64}(C_NULL) : pointer(d.im))
              for d in hops]

function hop_drive_check(model::Model, hops::Vector{HoppingDrive})
    GC.@preserve hops begin
        arr = pack_hops(hops)
        check(ccall((:sd_hop_drive_check, libspindyn), Cint, (Ptr{Cvoid}, Ptr{CHopDrive}, Cint), model.h, arr, length(arr)), model.ctx.h)
    end
    return nothing
end

# (Σ_k coefs[k] B_k) ψ, plus y when given; a list with complex weights needs a ComplexF64 ψ
function hopping_apply(ψ::Vector{T}, model::Model, hops::Vector{HoppingDrive}, coefs::AbstractVector;
                       y::Union{Nothing,Vector{T}}=nothing) where {T<:Union{Float64,ComplexF64}}
    out = similar(ψ)
    c = Vector{Float64}(coefs)
    GC.@preserve hops begin
        arr = pack_hops(hops)
        check(ccall((:sd_hop_apply, libspindyn), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{CHopDrive}, Cint, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}),
                    model.ctx.h, model.h, dtype_code(T), ψ, length(ψ), arr, length(arr), c, y === nothing ? C_NULL : y, out), model.ctx.h)
    end
    return out
end

# out = (H0 + Σ_k coefs[k] D_k + Σ_k coefs[K + k] B_k) ψ: the diagonal drives' coefficients first
function driven_apply(out::Vector{T}, ψ::Vector{T}, model::Model, drives::Vector{DiagonalDrive}, hops::Vector{HoppingDrive},
                      coefs::AbstractVector) where {T<:Union{Float64,ComplexF64}}
    c = Vector{Float64}(coefs)
    length(c) == length(drives) + length(hops) || throw(ArgumentError("coefs needs one entry per drive, the diagonal ones first"))
    GC.@preserve drives hops begin
        arr = pack_drives(model, drives)
        harr = pack_hops(hops)
        check(ccall((:sd_driven_hop_apply, libspindyn), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{CDrive}, Cint, Ptr{CHopDrive}, Cint, Ptr{Float64}, Ptr{Cvoid}),
                    model.ctx.h, model.h, dtype_code(T), ψ, length(ψ), arr, length(arr), harr, length(harr), c, out), model.ctx.h)
    end
    return out
end

# stage_evolve with both kinds of drive: coef is (K + KH) x stages, the rows of the diagonal drives first -> (ψ, info)
function stage_evolve(model::Model, ψ0::AbstractVector, drives::Vector{DiagonalDrive}, hops::Vector{HoppingDrive}, tau::Vector{Float64},
                      coef::Matrix{Float64}; kry_m::Int=30)
    x = eltype(ψ0) <: Complex ? Vector{ComplexF64}(ψ0) : Vector{Float64}(ψ0)
    size(coef) == (length(drives) + length(hops), length(tau)) || throw(ArgumentError("coef must be (K + KH) x stages"))
    out = Vector{ComplexF64}(undef, length(x))
    info = DrivenInfo()
    GC.@preserve drives hops begin
        arr = pack_drives(model, drives)
        harr = pack_hops(hops)
        check(ccall((:sd_driven_hop_evolve, libspindyn), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{CDrive}, Cint, Ptr{CHopDrive}, Cint, Cint, Ptr{Float64}, Ptr{Float64},
                     Cint, Ptr{Cvoid}, Ref{DrivenInfo}),
                    model.ctx.h, model.h, dtype_code(eltype(x)), x, length(x), arr, length(arr), harr, length(harr), length(tau), tau, coef,
                    kry_m, out, info), model.ctx.h)
    end
    return out, (stages=Int(info.stages), applies=info.applies, min_beta=info.min_beta)
end

end # module
