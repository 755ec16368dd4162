# JWASHip.jl -- ccall binding of libjwas_hip.so (include/jwas_hip.h) for reworkhow/JWAS.jl.
#
# Drop this file next to src/1.JWAS/src/markers/streaming_genotypes.jl and `include` it after that file; the call
# sites to patch are listed in INTEGRATION.md section 2.  Julia is not installed in the image this repository is built
# in, so the file has not been executed there.  What IS checked mechanically (tests/test_abi.py::test_julia_struct_layout):
# the field order, field types and NTuple lengths of HipSweepParams / HipSweepStats below are parsed and their C layout
# (natural alignment, which is what an isbits Julia struct uses) is compared with gcc's offsetof / sizeof of
# jwas_sweep_params / jwas_sweep_stats.
module JWASHip

export HipBackend, HipSweepParams, HipSweepStats, hip_sweep!, hip_sweep_sharded!, hip_comm_unique_id, hip_comm_init!, hip_comm_info, hip_residual_add_scalar!,
       hip_setup_blocks!, hip_set_residual!, hip_get_residual!, hip_accumulate!, hip_posterior, hip_mul_alpha, JWAS_HIP_BAYESC,
       JWAS_HIP_BAYESB, JWAS_HIP_BAYESR, JWAS_HIP_MTBAYESC1, JWAS_HIP_MTBAYESC2, JWAS_HIP_MEGABAYESC, JWAS_HIP_MTBAYESB1,
       JWAS_HIP_MTBAYESB2, JWAS_HIP_MEGABAYESB

const LIBJWAS_HIP = get(ENV, "JWAS_HIP_LIB", "libjwas_hip.so")

const JWAS_HIP_BAYESC, JWAS_HIP_BAYESB, JWAS_HIP_BAYESR = Int32(0), Int32(1), Int32(2)
const JWAS_HIP_MTBAYESC1, JWAS_HIP_MTBAYESC2, JWAS_HIP_MEGABAYESC, JWAS_HIP_MTBAYESB1 = Int32(3), Int32(4), Int32(5), Int32(6)
const JWAS_HIP_MTBAYESB2, JWAS_HIP_MEGABAYESB = Int32(7), Int32(8)     # BayesA/B under sampler II / constraint = true
const JWAS_HIP_GRAM_F64, JWAS_HIP_GRAM_MFMA = Int32(0), Int32(1)

# mirrors of struct jwas_sweep_params / jwas_sweep_stats (isbits, same field order; JWAS_HIP_MAX_TRAITS = 4)
struct HipSweepParams
    method::Int32
    ntraits::Int32
    nreps::Int32
    iteration::UInt32
    seed::UInt64
    marker_offset::UInt32
    independent_blocks::UInt32
    vare::NTuple{16,Float32}
    var_effect::NTuple{16,Float32}
    pi::Float64
    pi_classes::NTuple{4,Float64}
    gamma::NTuple{4,Float64}
    log_prior_states::NTuple{16,Float64}
    var_effect_vec::Ptr{Float32}
    pi_vec::Ptr{Float64}
    pi_matrix::Ptr{Float64}
    log_prior_states_matrix::Ptr{Float64}
    var_effect_matrix::Ptr{Float32}
    vare_f64::NTuple{16,Float64}
    var_effect_f64::NTuple{16,Float64}
    var_effect_vec_f64::Ptr{Float64}
    section_solve::Int32
    group_launch::Int32
end

struct HipSweepStats
    sum_delta::NTuple{4,Float64}
    alpha_ss::NTuple{16,Float64}
    beta_ss::NTuple{16,Float64}
    resid_ss::NTuple{16,Float64}
    resid_sum::NTuple{4,Float64}
    class_counts::NTuple{4,Float64}
    bayesr_ssq::Float64
    bayesr_nnz::Float64
    state_counts::NTuple{16,Float64}
    n_events::Float64
    sweep_ms::Float64
    update_kernel_ms::Float64
    update_kernel_samples::Float64
    update_kernel_bytes::Float64
    event_overhead_ms::Float64
end

mutable struct HipBackend            # the analogue of Packed2BitBackend (streaming_genotypes.jl:7-25)
    ctx::Ptr{Cvoid}
    nObs::Int
    nMarkers::Int
    block_size::Int
end

hip_error(ctx) = unsafe_string(ccall((:jwas_hip_last_error, LIBJWAS_HIP), Cstring, (Ptr{Cvoid},), ctx))
hip_check(ctx, rc) = rc == 0 || error("libjwas_hip: " * hip_error(ctx))      # error(...) like every JWAS check

"Upload a genotype matrix (after align_genotypes, tools4genotypes.jl:310-321) and precompute x'x and the block Grams."
function HipBackend(X::Matrix{Float32}; device::Integer=0, block_size::Integer=512, invweights=nothing,
                    method::Integer=JWAS_HIP_BAYESC, ntraits::Integer=1)
    ctxref = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:jwas_hip_create, LIBJWAS_HIP), Cint, (Cint, Ref{Ptr{Cvoid}}), device, ctxref)
    rc == 0 || error("libjwas_hip: " * hip_error(C_NULL))
    n, p = size(X)          # Julia matrices are column-major == the device's marker-major layout: no re-layout
    b = HipBackend(ctxref[], n, p, block_size)
    finalizer(x -> ccall((:jwas_hip_destroy, LIBJWAS_HIP), Cvoid, (Ptr{Cvoid},), x.ctx), b)
    hip_check(b.ctx, ccall((:jwas_hip_load_dense_f32, LIBJWAS_HIP), Cint,
                           (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Int64), b.ctx, X, n, p, n))
    if invweights !== nothing          # GibbsMats with Rinv (tools4genotypes.jl:253-266)
        w = Vector{Float32}(invweights)
        hip_check(b.ctx, ccall((:jwas_hip_set_weights, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float32}), b.ctx, w))
    end
    hip_check(b.ctx, ccall((:jwas_hip_setup_blocks, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int32),
                           b.ctx, block_size, JWAS_HIP_GRAM_MFMA))
    hip_check(b.ctx, ccall((:jwas_hip_init_state, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int32), b.ctx, method, ntraits))
    return b
end

"fast_blocks = a vector of 1-based block starts, possibly non-uniform (JWAS.jl:298-304): the device runs exactly that partition."
function hip_setup_blocks!(b::HipBackend, starts::AbstractVector{<:Integer})
    s0 = Int64.(starts) .- 1
    hip_check(b.ctx, ccall((:jwas_hip_setup_blocks_explicit, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64, Int32),
                           b.ctx, s0, length(s0), JWAS_HIP_GRAM_MFMA))
    return b
end

hip_set_residual!(b::HipBackend, trait::Integer, r::Vector{Float32}) =
    hip_check(b.ctx, ccall((:jwas_hip_set_residual, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}), b.ctx, trait, r))
hip_get_residual!(b::HipBackend, trait::Integer, r::Vector{Float32}) =
    hip_check(b.ctx, ccall((:jwas_hip_get_residual, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}), b.ctx, trait, r))

"Several genotype categories (`for Mi in mme.M`, MCMC_BayesianAlphabet.jl:224-226): one backend per category; the residual of `src`
(all traits) becomes `dst`'s, device to device, ordered on the two streams without a host wait."
hip_residual_handover!(dst::HipBackend, src::HipBackend) =
    hip_check(dst.ctx, ccall((:jwas_hip_residual_handover, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), dst.ctx, src.ctx))

"Grouped launches for the selected block size: 2 or 4 consecutive blocks per launch of the step kernel (0 frees the buffers); the sweeps
whose HipSweepParams carry group_launch = 1 then use them.  Worth its set-up time from a few thousand iterations on (INTEGRATION.md)."
hip_setup_groups!(b::HipBackend, blocks_per_launch::Integer) =
    hip_check(b.ctx, ccall((:jwas_hip_setup_groups, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int32), b.ctx, blocks_per_launch, JWAS_HIP_GRAM_MFMA))

"A cross-Gram as the device holds it (tests, diagnostics).  level 0: X_{index-1}' X_index of the selected block size; level 1 / 2: the
pair / four cross-Grams of grouped launches (at 4 blocks per launch only the odd pairs exist).  index is 1-based like Julia's blocks:
index = 2 is the first cross-Gram.  Uniform blocks (an explicit partition's block sizes are the caller's: pass rows and cols).
Returns a rows x cols matrix, rows = the markers of the predecessor."
function hip_cross_gram(b::HipBackend, level::Integer, index::Integer;
                        rows::Integer=(1 << level) * b.block_size,
                        cols::Integer=min((1 << level) * b.block_size, b.nMarkers - (index - 1) * (1 << level) * b.block_size))
    out = Matrix{Float32}(undef, max(cols, 1), max(rows, 1))      # the library writes row-major: the transpose in Julia's layout
    hip_check(b.ctx, ccall((:jwas_hip_get_cross_gram, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Float32}), b.ctx, level, index - 1, out))
    return permutedims(out)
end

"Float64 context (runMCMC(double_precision=true), JWAS.jl:349-366): call before loading genotypes; the data entry points are then
jwas_hip_load_dense_f64 / _set_state_f64 / _get_state_f64 / _set_residual_f64 / _get_residual_f64 / _get_posterior_f64 (Ptr{Float64})."
hip_set_precision!(ctx::Ptr{Cvoid}, bits::Integer) =
    hip_check(ctx, ccall((:jwas_hip_set_precision, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32), ctx, bits))

"Float64 context, multi-trait BayesA/B (init_state JWAS_HIP_MTBAYESB1 / MTBAYESB2): the p x t x t per-marker effect covariances in
double, row-major per marker (locus_effect_variances, MTBayesABC.jl:66); the next sweeps invert and use them in place.  A drawn set
(jwas_hip_sample_marker_covariances) is read back with hip_get_marker_covariances_f64!."
hip_set_marker_covariances_f64!(b::HipBackend, m::Array{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_set_marker_covariances_f64, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.ctx, m))
hip_get_marker_covariances_f64!(b::HipBackend, m::Array{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_get_marker_covariances_f64, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.ctx, m))

"Float64 context, the output side (Ptr{Float64} twins of the Float32 calls): Mi.output_genotypes as a second resident matrix
(tools4genotypes.jl:290-296), EBV = output_genotypes * alpha of a saved sample (output.jl:281-306), a saved sample as (index, value)
lists in marker order, and the window sums of the GWAS (GWAS.jl:152-165, :199-217; outs = 2 vectors of nwin, or 5 with val2)."
hip_load_output_dense_f64!(b::HipBackend, X::Matrix{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_load_output_dense_f64, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64),
                           b.ctx, X, size(X, 1), size(X, 2), size(X, 1)))
hip_mul_alpha_output_f64!(b::HipBackend, trait::Integer, out::Vector{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_mul_alpha_output_f64, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), b.ctx, trait, out))
function hip_get_alpha_sparse_f64(b::HipBackend, trait::Integer)
    idx, val, nnz = Vector{Int32}(undef, b.nMarkers), Vector{Float64}(undef, b.nMarkers), Ref{Int64}(0)
    hip_check(b.ctx, ccall((:jwas_hip_get_alpha_sparse_f64, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Int32}, Ptr{Float64}, Ref{Int64}),
                           b.ctx, trait, b.nMarkers, idx, val, nnz))
    return idx[1:nnz[]], val[1:nnz[]]          # 0-based marker indices
end
hip_window_sums_f64!(b::HipBackend, use_output_rows::Bool, wptr::Vector{Int32}, idx::Vector{Int32}, val::Vector{Float64},
                     out_sum::Vector{Float64}, out_ss::Vector{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_window_sums_f64, LIBJWAS_HIP), Cint,
                           (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                           b.ctx, use_output_rows, length(wptr) - 1, wptr, idx, val, out_sum, out_ss))
hip_window_sums2_f64!(b::HipBackend, use_output_rows::Bool, wptr::Vector{Int32}, idx::Vector{Int32}, val1::Vector{Float64},
                      val2::Vector{Float64}, outs::NTuple{5,Vector{Float64}}) =
    hip_check(b.ctx, ccall((:jwas_hip_window_sums2_f64, LIBJWAS_HIP), Cint,
                           (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                            Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                           b.ctx, use_output_rows, length(wptr) - 1, wptr, idx, val1, val2, outs...))

"GWAS session (GWAS.jl:149-173): window variances and local EBVs of the saved samples with everything resident.  `hip_gwas_begin!`
uploads the windows (0-based column ranges [col_start, col_end), as the host's build_windows returns them) once; a sample then goes
in as the ascending 0-based (idx, val) list of its nonzero effects and comes back as (sum, sum of squares) of nwin + 1 entries
(entry 1 = all markers, entry 1 + w = window w; the bits of jwas_hip_window_sums); `hip_gwas_local_ebv` returns the n_rows x nwin
mean of the windows' genomic values over the samples fed so far."
hip_gwas_begin!(b::HipBackend, col_start::Vector{Int32}, col_end::Vector{Int32}; use_output_rows::Bool=false, local_ebv::Bool=false) =
    hip_check(b.ctx, ccall((:jwas_hip_gwas_begin, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Int32),
                           b.ctx, use_output_rows, length(col_start), col_start, col_end, local_ebv))
hip_gwas_sample!(b::HipBackend, idx::Vector{Int32}, val::Vector{Float32}, out_sum::Vector{Float64}, out_ss::Vector{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_gwas_sample, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float32}, Ptr{Float64}, Ptr{Float64}),
                           b.ctx, length(idx), idx, val, out_sum, out_ss))
hip_gwas_sample!(b::HipBackend, idx::Vector{Int32}, val::Vector{Float64}, out_sum::Vector{Float64}, out_ss::Vector{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_gwas_sample_f64, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                           b.ctx, length(idx), idx, val, out_sum, out_ss))
function hip_gwas_local_ebv(b::HipBackend, n_rows::Integer, nwin::Integer)
    out, ns = Matrix{Float64}(undef, n_rows, nwin), Ref{Int64}(0)       # window-major = a column per window
    hip_check(b.ctx, ccall((:jwas_hip_gwas_local_ebv, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Int64}), b.ctx, out, ns))
    return out, ns[]
end
function hip_gwas_geometry(b::HipBackend)
    nsl, wpc, nch = Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0)
    hip_check(b.ctx, ccall((:jwas_hip_gwas_geometry, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}), b.ctx, nsl, wpc, nch))
    return (nslices = nsl[], windows_per_chunk = wpc[], nchunks = nch[])
end
hip_gwas_end!(b::HipBackend) = hip_check(b.ctx, ccall((:jwas_hip_gwas_end, LIBJWAS_HIP), Cint, (Ptr{Cvoid},), b.ctx))
hip_gwas_estimate_bytes(n_rows::Integer, nwin::Integer, max_nnz::Integer, local_ebv::Bool) =
    ccall((:jwas_hip_gwas_estimate_bytes, LIBJWAS_HIP), Int64, (Int64, Int64, Int64, Int32), n_rows, nwin, max_nnz, local_ebv)

"Threshold / censored traits (categorical_and_censored_trait.jl:29-210): the liabilities live on the device beside the residual.
`hip_liability_begin!` after `jwas_hip_init_state`; `hip_liability_set_categorical!` (codes 1..ncat, 0 = missing; thresholds
[-Inf, 0, ..., Inf]) or `hip_liability_set_censored!` per trait; upload the residual as placeholder - cmean with the placeholder
`hip_get_liabilities` returns; `hip_liability_init!` is the set-up draw (:82-88), `hip_liability_sample!` replaces
sample_liabilities! (:166-210), `hip_liability_minmax` gives the support of every threshold draw (:152-155), to be followed by
`hip_liability_set_thresholds!` (:155,160)."
struct HipLiabilityParams
    iteration::UInt32
    ngibbs::Int32
    seed::UInt64
    R::NTuple{16,Float64}
end
function HipLiabilityParams(iter::Integer, seed::Integer, ngibbs::Integer, R::AbstractMatrix)
    Rt = Float64.(permutedims(R))                # row-major t x t, as the header asks
    HipLiabilityParams(UInt32(iter), Int32(ngibbs), UInt64(seed), ntuple(i -> i <= length(Rt) ? Rt[i] : 0.0, 16))
end
HipLiabilityParams(iter::Integer, seed::Integer, ngibbs::Integer, R::Real) =      # single trait: mme.R.val is a scalar
    HipLiabilityParams(iter, seed, ngibbs, fill(Float64(R), 1, 1))
hip_liability_begin!(b::HipBackend, ntraits::Integer) =
    hip_check(b.ctx, ccall((:jwas_hip_liability_begin, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32), b.ctx, ntraits))
hip_liability_set_categorical!(b::HipBackend, trait::Integer, codes::Vector{Int32}, thresholds::Vector{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_liability_set_categorical, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Int32}, Int32, Ptr{Float64}),
                           b.ctx, trait - 1, length(codes), codes, length(thresholds), thresholds))
hip_liability_set_censored!(b::HipBackend, trait::Integer, lower::Vector{Float64}, upper::Vector{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_liability_set_censored, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Ptr{Float64}),
                           b.ctx, trait - 1, length(lower), lower, upper))
hip_liability_set_thresholds!(b::HipBackend, trait::Integer, thresholds::Vector{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_liability_set_thresholds, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}),
                           b.ctx, trait - 1, length(thresholds), thresholds))
hip_liability_init!(b::HipBackend, P::HipLiabilityParams) =
    hip_check(b.ctx, ccall((:jwas_hip_liability_init, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipLiabilityParams}), b.ctx, P))
hip_liability_sample!(b::HipBackend, P::HipLiabilityParams) =
    hip_check(b.ctx, ccall((:jwas_hip_liability_sample, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipLiabilityParams}), b.ctx, P))
function hip_liability_minmax(b::HipBackend, trait::Integer, nthresholds::Integer)
    mx = Vector{Float64}(undef, nthresholds); mn = Vector{Float64}(undef, nthresholds)
    hip_check(b.ctx, ccall((:jwas_hip_liability_minmax, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), b.ctx, trait - 1, mx, mn))
    return mx, mn
end
function hip_get_liabilities(b::HipBackend, trait::Integer)
    out = Vector{Float64}(undef, b.nObs)
    hip_check(b.ctx, ccall((:jwas_hip_get_liabilities, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), b.ctx, trait - 1, out))
    return out
end
hip_liability_end!(b::HipBackend) = hip_check(b.ctx, ccall((:jwas_hip_liability_end, LIBJWAS_HIP), Cint, (Ptr{Cvoid},), b.ctx))

"Location parameters on the device (MCMC/MCMC_BayesianAlphabet.jl:193-220; iterative_solver/solver.jl:143-162 term by term).
`hip_locpar_begin!` after `jwas_hip_init_state` and the weights; the terms trait by trait, term by term (the equation order):
`hip_locpar_add_covariate!` (x = nothing: the intercept) and `hip_locpar_add_factor!` (levels 1..nlevels, 0 = in no level;
random_group 0 = fixed, g >= 1 = member of the g-th set_random effect).  `hip_locpar_step!` replaces the scan and returns the U'U
cross-products sampleVCs reads (variance_components.jl:121-135); `hip_locpar_accumulate!` / `hip_locpar_means` keep the running
means of output.jl:556-560 on the device."
struct HipLocparParams
    iteration::UInt32
    first_term::Int32
    last_term::Int32
    reserved::Int32
    seed::UInt64
    vare::Float64
    Rinv::NTuple{16,Float64}
    Gi::NTuple{128,Float64}
end
struct HipLocparStats
    utu::NTuple{128,Float64}
    step_ms::Float64
end
"vare: the residual variance (one trait) or R (several traits, inverted here); Gi: inv(G) of every random effect, in group order.
Both are symmetrised here, as the library refuses a matrix that is not symmetric bit for bit."
function HipLocparParams(iter::Integer, seed::Integer, R, Gi::Vector{<:AbstractMatrix}; first_term::Integer = 0, last_term::Integer = -1)
    # (the library asks for exactly symmetric matrices; an LU inverse is symmetric up to rounding only)
    sym(M) = (M .+ permutedims(M)) ./ 2
    Rt = R isa Real ? Float64[] : vec(sym(inv(Float64.(R))))
    g = zeros(Float64, 128)
    for (i, M) in enumerate(Gi)
        Mt = vec(sym(Float64.(M)))
        g[16 * (i - 1) + 1:16 * (i - 1) + length(Mt)] .= Mt
    end
    HipLocparParams(UInt32(iter), Int32(first_term), Int32(last_term), Int32(0), UInt64(seed), R isa Real ? Float64(R) : 0.0,
                    ntuple(i -> i <= length(Rt) ? Rt[i] : 0.0, 16), ntuple(i -> g[i], 128))
end
hip_locpar_begin!(b::HipBackend, ntraits::Integer) =
    hip_check(b.ctx, ccall((:jwas_hip_locpar_begin, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32), b.ctx, ntraits))
hip_locpar_add_covariate!(b::HipBackend, trait::Integer, n::Integer, x::Union{Nothing,Vector{Float64}}) =
    hip_check(b.ctx, ccall((:jwas_hip_locpar_add_covariate, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}),
                           b.ctx, trait - 1, n, x === nothing ? C_NULL : x))
hip_locpar_add_factor!(b::HipBackend, trait::Integer, level::Vector{Int32}, nlevels::Integer, random_group::Integer = 0) =
    hip_check(b.ctx, ccall((:jwas_hip_locpar_add_factor, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Int32}, Int64, Int32),
                           b.ctx, trait - 1, length(level), level .- Int32(1), nlevels, random_group - 1))
function hip_locpar_size(b::HipBackend)
    q = Ref{Int64}(0)
    hip_check(b.ctx, ccall((:jwas_hip_locpar_size, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{Int64}), b.ctx, q))
    return q[]
end
hip_locpar_set_sol!(b::HipBackend, sol::Vector{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_locpar_set_sol, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), b.ctx, length(sol), sol))
function hip_locpar_get_sol(b::HipBackend)
    sol = Vector{Float64}(undef, hip_locpar_size(b))
    hip_check(b.ctx, ccall((:jwas_hip_locpar_get_sol, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), b.ctx, length(sol), sol))
    return sol
end
function hip_locpar_step!(b::HipBackend, P::HipLocparParams)
    S = Ref{HipLocparStats}()
    hip_check(b.ctx, ccall((:jwas_hip_locpar_step, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipLocparParams}, Ref{HipLocparStats}), b.ctx, P, S))
    return S[]
end
hip_locpar_accumulate!(b::HipBackend, nsamples::Real) =
    hip_check(b.ctx, ccall((:jwas_hip_locpar_accumulate, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Float64), b.ctx, nsamples))
function hip_locpar_means(b::HipBackend)
    q = hip_locpar_size(b)
    m = Vector{Float64}(undef, q); m2 = Vector{Float64}(undef, q)
    hip_check(b.ctx, ccall((:jwas_hip_locpar_get_means, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}), b.ctx, q, m, m2))
    return m, m2
end
hip_locpar_estimate_bytes(n::Integer, nterms::Integer, total_levels::Integer) =
    ccall((:jwas_hip_locpar_estimate_bytes, LIBJWAS_HIP), Int64, (Int64, Int64, Int64), n, nterms, total_levels)
hip_locpar_end!(b::HipBackend) = hip_check(b.ctx, ccall((:jwas_hip_locpar_end, LIBJWAS_HIP), Cint, (Ptr{Cvoid},), b.ctx))
"The inverse covariance among the levels of the random_group-th set_random effect (the pedigree form: `Float64.(AInverse(ped))`), a
full symmetric `SparseMatrixCSC` -- its columns ARE the rows of the CSR matrix the library takes.  After `hip_locpar_begin!`, before
the effect's first `hip_locpar_add_factor!`.  `hip_locpar_step!` then samples the effect colour by colour and returns U'VU for it."
function hip_locpar_set_group_structure!(b::HipBackend, random_group::Integer, V)
    indptr = Int64.(V.colptr) .- Int64(1)
    indices = Int32.(V.rowval) .- Int32(1)
    values = Float64.(V.nzval)
    hip_check(b.ctx, ccall((:jwas_hip_lp_set_group_structure, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}),
                           b.ctx, random_group - 1, length(indptr) - 1, indptr, indices, values))
end
"(colours 1..ncolors of the nlevels levels, ncolors): the order `hip_locpar_step!` visits the levels of a structured effect in."
function hip_locpar_group_colors(b::HipBackend, random_group::Integer, nlevels::Integer)
    color = Vector{Int32}(undef, nlevels); nc = Ref{Int32}(0)
    hip_check(b.ctx, ccall((:jwas_hip_lp_get_group_colors, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Int32}, Ref{Int32}),
                           b.ctx, random_group - 1, nlevels, color, nc))
    return color .+ Int32(1), Int(nc[])
end
hip_locpar_structure_estimate_bytes(nlevels::Integer, nnz::Integer) =
    ccall((:jwas_hip_lp_structure_estimate_bytes, LIBJWAS_HIP), Int64, (Int64, Int64), nlevels, nnz)

"Multi-trait records that miss some traits (residual.jl:2-73).  `hip_mtmiss_begin!` stores the code of every record (bit k-1 set =
trait k observed); `hip_mtmiss_impute!` replaces sampleMissingResiduals given the per-code tables B and U of the current R
([t, t, 2^t] arrays in Julia's column-major order hold the library's row-major [2^t][t][t]: index them [column, row, code + 1]);
`hip_mtmiss_set_record_weights!` makes `hip_locpar_step!` weight every record with C[code] = the RZ of getRi (nothing: back to
kron(inv(R), diag(w)), MCMC_BayesianAlphabet.jl:357-361)."
struct HipMtmissParams
    iteration::UInt32
    reserved::UInt32
    seed::UInt64
    B::Ptr{Float64}
    U::Ptr{Float64}
end
hip_mtmiss_begin!(b::HipBackend, observed::Vector{Int32}) =
    hip_check(b.ctx, ccall((:jwas_hip_mtmiss_begin, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{Int32}), b.ctx, length(observed), observed))
function hip_mtmiss_impute!(b::HipBackend, iter::Integer, seed::Integer, B::Array{Float64,3}, U::Array{Float64,3})
    GC.@preserve B U begin
        P = HipMtmissParams(UInt32(iter), UInt32(0), UInt64(seed), pointer(B), pointer(U))
        hip_check(b.ctx, ccall((:jwas_hip_mtmiss_impute, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipMtmissParams}), b.ctx, P))
    end
end
hip_mtmiss_set_record_weights!(b::HipBackend, C::Union{Nothing,Array{Float64,3}}) =
    hip_check(b.ctx, ccall((:jwas_hip_mtmiss_set_record_weights, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.ctx, C === nothing ? C_NULL : C))
hip_mtmiss_estimate_bytes(n::Integer) = ccall((:jwas_hip_mtmiss_estimate_bytes, LIBJWAS_HIP), Int64, (Int64,), n)
hip_mtmiss_end!(b::HipBackend) = hip_check(b.ctx, ccall((:jwas_hip_mtmiss_end, LIBJWAS_HIP), Cint, (Ptr{Cvoid},), b.ctx))

"Marker-annotation priors on the device (MCMC/annotation_updates.jl:21-137,181-361; csrc/annot.hpp).  `hip_annot_begin!` opens a
session (kind 0 = annotated BayesC, 1 = BayesR, 2 = the 2-trait tree) with the p x ncols design matrix (column 1 the ones), the
start coefficients (ncols x nsteps) and the table the first sweep reads; `hip_annot_step!` replaces update_marker_annotation_priors!
from the resident delta and leaves the per-marker prior where the next sweep reads it: pass C_NULL for pi_vec / pi_matrix /
log_prior_states_matrix while the session is open.  The shrinkage variances stay the caller's draw (annotation_updates.jl:125-137)."
struct HipAnnotParams
    iteration::UInt32
    reserved::UInt32
    seed::UInt64
    variance::NTuple{3,Float64}
end
struct HipAnnotStats
    coef::NTuple{192,Float64}
    n_active::NTuple{3,Int64}
    means::NTuple{4,Float64}
    step_ms::Float64
end
function hip_annot_begin!(b::HipBackend, kind::Integer, D::Matrix{Float64}, coef::VecOrMat{Float64}, variance::Vector{Float64},
                          start_prior::VecOrMat{Float64})
    Dr = permutedims(D)                                   # row-major p x ncols
    cf = vec(Matrix{Float64}(reshape(coef, size(D, 2), :)))   # column-major ncols x nsteps == the library's [nsteps][ncols]
    sp = start_prior isa Matrix ? vec(permutedims(start_prior)) : start_prior
    hip_check(b.ctx, ccall((:jwas_hip_annot_begin, LIBJWAS_HIP), Cint,
                           (Ptr{Cvoid}, Int32, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                           b.ctx, kind, size(D, 1), size(D, 2), Dr, cf, variance, sp))
end
function hip_annot_step!(b::HipBackend, iter::Integer, seed::Integer, variance)
    v = ntuple(i -> i <= length(variance) ? Float64(variance[i]) : 1.0, 3)
    S = Ref{HipAnnotStats}()
    hip_check(b.ctx, ccall((:jwas_hip_annot_step, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipAnnotParams}, Ref{HipAnnotStats}),
                           b.ctx, HipAnnotParams(UInt32(iter), UInt32(0), UInt64(seed), v), S))
    S[]
end
hip_annot_accumulate!(b::HipBackend, nsamples::Real) =
    hip_check(b.ctx, ccall((:jwas_hip_annot_accumulate, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Float64), b.ctx, nsamples))
function _hip_annot_get(b::HipBackend, sym::Symbol, nvalues::Integer)
    out = Vector{Float64}(undef, nvalues)
    if sym === :prior
        hip_check(b.ctx, ccall((:jwas_hip_annot_get_prior, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), b.ctx, nvalues, out))
    elseif sym === :liability
        hip_check(b.ctx, ccall((:jwas_hip_annot_get_liability, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), b.ctx, nvalues, out))
    else
        hip_check(b.ctx, ccall((:jwas_hip_annot_get_mu, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), b.ctx, nvalues, out))
    end
    out
end
"The resident table as the sweep reads it, row-major (nvalues = p, or 4 p)."
hip_annot_prior(b::HipBackend, nvalues::Integer) = _hip_annot_get(b, :prior, nvalues)
"The liabilities / mu of every step, [nsteps][p] (nvalues = nsteps * p)."
hip_annot_liability(b::HipBackend, nvalues::Integer) = _hip_annot_get(b, :liability, nvalues)
hip_annot_mu(b::HipBackend, nvalues::Integer) = _hip_annot_get(b, :mu, nvalues)
function hip_annot_means(b::HipBackend, nvalues::Integer)
    m, m2 = Vector{Float64}(undef, nvalues), Vector{Float64}(undef, nvalues)
    hip_check(b.ctx, ccall((:jwas_hip_annot_get_means, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}), b.ctx, nvalues, m, m2))
    m, m2
end
hip_annot_estimate_bytes(p::Integer, ncols::Integer, kind::Integer) =
    ccall((:jwas_hip_annot_estimate_bytes, LIBJWAS_HIP), Int64, (Int64, Int32, Int32), p, ncols, kind)
hip_annot_end!(b::HipBackend) = hip_check(b.ctx, ccall((:jwas_hip_annot_end, LIBJWAS_HIP), Cint, (Ptr{Cvoid},), b.ctx))

"Structural equation models on the device (structure_equation_model/SEM.jl:53-165,245-252; csrc/sem.hpp).  `hip_sem_begin!` takes the
phenotypes (n x t, as wArray's columns) and the causal structure; `hip_sem_step!` replaces get_Λ on the resident residual (the
reference's Λycorr) and returns the coefficient matrix Λ (t x t, λ_ij at [i, j]); `hip_sem_accumulate!` takes K = Σ_m Λ^m
(compute_indirect_effect) and keeps the running means of the indirect and overall marker effects."
struct HipSemParams
    iteration::UInt32
    reserved::UInt32
    seed::UInt64
    R_diag::NTuple{4,Float64}
end
struct HipSemStats
    lambda::NTuple{16,Float64}
    mean::NTuple{16,Float64}
    ypr::NTuple{16,Float64}
    step_ms::Float64
end
# the library's matrices are row-major t x t: a Julia matrix goes over as its transpose
_hip_sem_matrix(v, t::Integer) = permutedims(reshape(collect(v[1:t*t]), t, t))
function hip_sem_begin!(b::HipBackend, Y::Matrix{Float64}, causal_structure::AbstractMatrix)
    t = size(Y, 2)
    cs = vec(permutedims(Matrix{Int32}(causal_structure)))
    hip_check(b.ctx, ccall((:jwas_hip_sem_begin, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Ptr{Int32}),
                           b.ctx, t, size(Y, 1), Y, cs))           # column-major n x t == the library's row-major t x n
    t
end
function hip_sem_step!(b::HipBackend, t::Integer, iter::Integer, seed::Integer, R::AbstractMatrix)
    S = Ref{HipSemStats}()
    rd = ntuple(i -> i <= t ? Float64(R[i, i]) : 1.0, 4)
    hip_check(b.ctx, ccall((:jwas_hip_sem_step, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipSemParams}, Ref{HipSemStats}),
                           b.ctx, HipSemParams(UInt32(iter), UInt32(0), UInt64(seed), rd), S))
    _hip_sem_matrix(S[].lambda, t), S[]
end
function hip_sem_lambda(b::HipBackend, t::Integer)
    out = Vector{Float64}(undef, t * t)
    hip_check(b.ctx, ccall((:jwas_hip_sem_get_lambda, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.ctx, out))
    _hip_sem_matrix(out, t)
end
hip_sem_set_lambda!(b::HipBackend, Λ::Matrix{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_sem_set_lambda, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.ctx, vec(permutedims(Λ))))
function hip_sem_gram(b::HipBackend, t::Integer)
    out = Vector{Float64}(undef, t * t)
    hip_check(b.ctx, ccall((:jwas_hip_sem_get_gram, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.ctx, out))
    _hip_sem_matrix(out, t)
end
hip_sem_accumulate!(b::HipBackend, K::Matrix{Float64}, nsamples::Real) =
    hip_check(b.ctx, ccall((:jwas_hip_sem_accumulate, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float64}, Float64), b.ctx, vec(permutedims(K)), nsamples))
"(mean, mean of squares, frequency of non-zero) per marker of trait `trait` (1-based); kind 0 = indirect, 1 = overall."
function hip_sem_effects(b::HipBackend, kind::Integer, trait::Integer, p::Integer)
    m, m2, f = Vector{Float64}(undef, p), Vector{Float64}(undef, p), Vector{Float64}(undef, p)
    hip_check(b.ctx, ccall((:jwas_hip_sem_get_effects, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                           b.ctx, kind, trait - 1, m, m2, f))
    m, m2, f
end
hip_sem_estimate_bytes(n::Integer, p::Integer, ntraits::Integer) =
    ccall((:jwas_hip_sem_estimate_bytes, LIBJWAS_HIP), Int64, (Int64, Int64, Int32), n, p, ntraits)
hip_sem_end!(b::HipBackend) = hip_check(b.ctx, ccall((:jwas_hip_sem_end, LIBJWAS_HIP), Cint, (Ptr{Cvoid},), b.ctx))

"Random regression models on the device (RRM/RRM.jl:43-57,101-158; RRM/MCMC_BayesianAlphabet_RRM.jl; csrc/rrm.hpp).  `hip_rrm_begin!`
takes Φ (T x c), the T x n record indicator (yfull's non-zeros, RRM.jl:12-20) and the block size and builds mΦΦArray and the block
Gram tensor; `hip_rrm_set_residual!` / `hip_rrm_residual` move yfull (n x T in Julia, wArray's columns); `hip_rrm_sweep!` replaces
BayesABCRRM! and returns the statistics samplePi and sample_variance need.  Limits: 2 <= c <= 4, T <= 64, blocks <= 256 markers,
dense genotypes, no residual weights, no shards.  The state index of `log_pi` and `state_counts` has bit q-1 set when coefficient q
is in the model."
struct HipRrmParams
    iteration::UInt32
    reserved::UInt32
    seed::UInt64
    vare::Float64
    G::NTuple{16,Float64}
    log_pi::NTuple{16,Float64}
end
struct HipRrmStats
    state_counts::NTuple{16,Float64}
    beta_ss::NTuple{16,Float64}
    alpha_ss::Float64
    resid_ss::Float64
    n_changed::Float64
    step_ms::Float64
end
function hip_rrm_begin!(b::HipBackend, Φ::Matrix{Float64}, observed::AbstractMatrix{Bool}, block_size::Integer=64)
    T, c = size(Φ)
    n = size(observed, 2)
    mask = zeros(UInt64, n)
    for i in 1:n, t in 1:T
        observed[t, i] && (mask[i] |= UInt64(1) << (t - 1))
    end
    hip_check(b.ctx, ccall((:jwas_hip_rrm_begin, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int32, Int64, Ptr{Float64}, Ptr{UInt64}, Int32),
                           b.ctx, T, c, n, vec(permutedims(Φ)), mask, block_size))
    (T, c)
end
# yfull as an n x T Julia matrix == the library's row-major T x n
hip_rrm_set_residual!(b::HipBackend, W::Matrix{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_rrm_set_residual, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), b.ctx, length(W), W))
function hip_rrm_residual(b::HipBackend, n::Integer, T::Integer)
    W = Matrix{Float64}(undef, n, T)
    hip_check(b.ctx, ccall((:jwas_hip_rrm_get_residual, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), b.ctx, length(W), W))
    W
end
# alpha, beta, delta as p x c Julia matrices (alphaArray's columns) == the library's row-major c x p
hip_rrm_set_state!(b::HipBackend, α::Matrix{Float64}, β::Matrix{Float64}, δ::Matrix{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_rrm_set_state, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.ctx, α, β, δ))
function hip_rrm_state(b::HipBackend, p::Integer, c::Integer)
    α, β, δ = Matrix{Float64}(undef, p, c), Matrix{Float64}(undef, p, c), Matrix{Float64}(undef, p, c)
    hip_check(b.ctx, ccall((:jwas_hip_rrm_get_state, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.ctx, α, β, δ))
    α, β, δ
end
function hip_rrm_sweep!(b::HipBackend, c::Integer, iter::Integer, seed::Integer, vare::Real, G::AbstractMatrix, log_pi::AbstractVector)
    S = Ref{HipRrmStats}()
    Gt = ntuple(i -> i <= c * c ? Float64(G[(i - 1) ÷ c + 1, (i - 1) % c + 1]) : 0.0, 16)
    lp = ntuple(i -> i <= 2^c ? Float64(log_pi[i]) : -Inf, 16)
    hip_check(b.ctx, ccall((:jwas_hip_rrm_sweep, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipRrmParams}, Ref{HipRrmStats}),
                           b.ctx, HipRrmParams(UInt32(iter), UInt32(0), UInt64(seed), Float64(vare), Gt, lp), S))
    S[]
end
hip_rrm_accumulate!(b::HipBackend, nsamples::Real) =
    hip_check(b.ctx, ccall((:jwas_hip_rrm_accumulate, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Float64), b.ctx, nsamples))
"(meanAlpha, meanAlpha2, meanDelta) of coefficient `q` (1-based), p values each."
function hip_rrm_posterior(b::HipBackend, q::Integer, p::Integer)
    m, m2, f = Vector{Float64}(undef, p), Vector{Float64}(undef, p), Vector{Float64}(undef, p)
    hip_check(b.ctx, ccall((:jwas_hip_rrm_get_posterior, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                           b.ctx, q - 1, m, m2, f))
    m, m2, f
end
"X α_q: the genomic values of coefficient `q` (1-based) of the n individuals (getEBV)."
function hip_rrm_mul_alpha(b::HipBackend, q::Integer, n::Integer)
    out = Vector{Float64}(undef, n)
    hip_check(b.ctx, ccall((:jwas_hip_rrm_mul_alpha, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), b.ctx, q - 1, out))
    out
end
"mΦΦArray as c(c+1)/2 x p lower cells (cell(a, b) = a(a+1)/2 + b, 0-based), and the Gram tensor of block `k` (1-based) of `nb` markers."
function hip_rrm_m(b::HipBackend, p::Integer, c::Integer)
    out = Matrix{Float64}(undef, c * (c + 1) ÷ 2, p)
    hip_check(b.ctx, ccall((:jwas_hip_rrm_get_m, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), b.ctx, length(out), out))
    out
end
function hip_rrm_gram(b::HipBackend, k::Integer, nb::Integer, c::Integer)
    out = Array{Float64,3}(undef, c * (c + 1) ÷ 2, nb, nb)
    hip_check(b.ctx, ccall((:jwas_hip_rrm_get_gram, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}), b.ctx, k - 1, length(out), out))
    out
end
hip_rrm_estimate_bytes(n::Integer, p::Integer, T::Integer, c::Integer, block_size::Integer=64) =
    ccall((:jwas_hip_rrm_estimate_bytes, LIBJWAS_HIP), Int64, (Int64, Int64, Int32, Int32, Int32), n, p, T, c, block_size)
hip_rrm_end!(b::HipBackend) = hip_check(b.ctx, ccall((:jwas_hip_rrm_end, LIBJWAS_HIP), Cint, (Ptr{Cvoid},), b.ctx))

"Mega-trait models on the device: constraint = true with up to 64 traits (markers/BayesianAlphabet/BayesABC.jl:1-58; csrc/mega.hpp).
`hip_mega_begin!` opens a session of t independent single-trait chains on the loaded genotypes (x'x and the block Grams);
`hip_mega_set_residual!` / `hip_mega_residual` move one wArray[i]; `hip_mega_impute!` stands for sampleMissingResiduals under a
diagonal R; `hip_mega_sweep!` replaces the Threads.@threads loop of megaBayesABC! and returns what samplePi, the constrained
sample_marker_effect_variance and sample_variance read, one value per trait.  Traits are 1-based here.  Limits: t <= 64, blocks <= 256
markers, dense genotypes, no residual weights, no shards."
struct HipMegaParams
    iteration::UInt32
    reserved::UInt32
    seed::UInt64
    vare::Ptr{Float64}
    var_effect::Ptr{Float64}
    pi::Ptr{Float64}
end
struct HipMegaStats
    sum_delta::Ptr{Float64}
    beta_ss::Ptr{Float64}
    alpha_ss::Ptr{Float64}
    resid_ss::Ptr{Float64}
    resid_sum::Ptr{Float64}
    n_changed::Ptr{Float64}
    step_ms::Float64
end
hip_mega_begin!(b::HipBackend, ntraits::Integer, block_size::Integer=256, first_trait::Integer=0) =
    hip_check(b.ctx, ccall((:jwas_hip_mega_begin, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int32, Int32), b.ctx, ntraits, block_size, first_trait))
# missing: n x t Bool in Julia (mme.missingPattern negated) == the library's row-major t x n bytes
hip_mega_set_missing!(b::HipBackend, missing::AbstractMatrix{Bool}) = (m = Matrix{UInt8}(missing);
    hip_check(b.ctx, ccall((:jwas_hip_mega_set_missing, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{UInt8}), b.ctx, length(m), m)))
hip_mega_set_residual!(b::HipBackend, trait::Integer, r::Vector{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_mega_set_residual, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), b.ctx, trait - 1, r))
function hip_mega_residual(b::HipBackend, trait::Integer, n::Integer)
    r = Vector{Float64}(undef, n)
    hip_check(b.ctx, ccall((:jwas_hip_mega_get_residual, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), b.ctx, trait - 1, r))
    return r
end
hip_mega_set_state!(b::HipBackend, trait::Integer, α::Vector{Float64}, β::Vector{Float64}, δ::Vector{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_mega_set_state, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.ctx, trait - 1, α, β, δ))
function hip_mega_state(b::HipBackend, trait::Integer, p::Integer)
    α, β, δ = (Vector{Float64}(undef, p) for _ in 1:3)
    hip_check(b.ctx, ccall((:jwas_hip_mega_get_state, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.ctx, trait - 1, α, β, δ))
    return α, β, δ
end
function hip_mega_impute!(b::HipBackend, iter::Integer, seed::Integer, vare::Vector{Float64})
    GC.@preserve vare begin
        P = HipMegaParams(UInt32(iter), UInt32(0), UInt64(seed), pointer(vare), Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL))
        hip_check(b.ctx, ccall((:jwas_hip_mega_impute, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipMegaParams}), b.ctx, Ref(P)))
    end
end
function hip_mega_sweep!(b::HipBackend, iter::Integer, seed::Integer, vare::Vector{Float64}, var_effect::Vector{Float64}, pi::Vector{Float64})
    t = length(vare)
    out = [zeros(Float64, t) for _ in 1:6]      # sum_delta, beta_ss, alpha_ss, resid_ss, resid_sum, n_changed
    S = Ref(HipMegaStats(pointer.(out)..., 0.0))
    GC.@preserve vare var_effect pi out begin
        P = HipMegaParams(UInt32(iter), UInt32(0), UInt64(seed), pointer(vare), pointer(var_effect), pointer(pi))
        hip_check(b.ctx, ccall((:jwas_hip_mega_sweep, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipMegaParams}, Ref{HipMegaStats}), b.ctx, Ref(P), S))
    end
    return (sum_delta=out[1], beta_ss=out[2], alpha_ss=out[3], resid_ss=out[4], resid_sum=out[5], n_changed=out[6], step_ms=S[].step_ms)
end
hip_mega_accumulate!(b::HipBackend, nsamples::Real) =
    hip_check(b.ctx, ccall((:jwas_hip_mega_accumulate, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Float64), b.ctx, nsamples))
# Several chains of one model: BayesR chains (BayesR.jl:56-96 in double) and the potential scale reduction factor of the chains.
# gamma, pi: 4 x t in the library's row-major layout, that is a t x 4 Julia matrix.
struct HipMegaRParams
    iteration::UInt32
    reserved::UInt32
    seed::UInt64
    vare::Ptr{Float64}
    var_effect::Ptr{Float64}
    gamma::Ptr{Float64}
    pi::Ptr{Float64}
end
struct HipMegaRStats
    class_counts::Ptr{Float64}
    ssq::Ptr{Float64}
    nnz::Ptr{Float64}
    alpha_ss::Ptr{Float64}
    resid_ss::Ptr{Float64}
    resid_sum::Ptr{Float64}
    n_changed::Ptr{Float64}
    step_ms::Float64
end
function hip_mega_sweep_r!(b::HipBackend, iter::Integer, seed::Integer, vare::Vector{Float64}, var_effect::Vector{Float64}, gamma::Matrix{Float64}, pi::Matrix{Float64})
    t = length(vare)
    counts = zeros(Float64, t, 4)
    out = [zeros(Float64, t) for _ in 1:6]      # ssq, nnz, alpha_ss, resid_ss, resid_sum, n_changed
    S = Ref(HipMegaRStats(pointer(counts), pointer.(out)..., 0.0))
    GC.@preserve vare var_effect gamma pi counts out begin
        P = HipMegaRParams(UInt32(iter), UInt32(0), UInt64(seed), pointer(vare), pointer(var_effect), pointer(gamma), pointer(pi))
        hip_check(b.ctx, ccall((:jwas_hip_mega_sweep_r, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipMegaRParams}, Ref{HipMegaRStats}), b.ctx, Ref(P), S))
    end
    return (class_counts=counts, ssq=out[1], nnz=out[2], alpha_ss=out[3], resid_ss=out[4], resid_sum=out[5], n_changed=out[6], step_ms=S[].step_ms)
end
hip_mega_accumulate_r!(b::HipBackend, nsamples::Real) =
    hip_check(b.ctx, ccall((:jwas_hip_mega_accumulate_r, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Float64), b.ctx, nsamples))
function hip_mega_psrf(b::HipBackend, nsamples::Real, p::Integer)
    out = Vector{Float64}(undef, p)
    hip_check(b.ctx, ccall((:jwas_hip_mega_psrf, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Float64, Ptr{Float64}), b.ctx, nsamples, out))
    return out
end
function hip_mega_posterior(b::HipBackend, trait::Integer, p::Integer)
    m, m2, f = (Vector{Float64}(undef, p) for _ in 1:3)
    hip_check(b.ctx, ccall((:jwas_hip_mega_get_posterior, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.ctx, trait - 1, m, m2, f))
    return m, m2, f
end
"X α_i over the training rows, or (output_rows) over the rows of hip_load_output_dense: n_rows values."
function hip_mega_mul_alpha(b::HipBackend, trait::Integer, n_rows::Integer; output_rows::Bool=false)
    out = Vector{Float64}(undef, n_rows)
    hip_check(b.ctx, ccall((:jwas_hip_mega_mul_alpha, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}), b.ctx, trait - 1, output_rows, out))
    return out
end
function hip_mega_gram(b::HipBackend, k::Integer, nb::Integer)
    G, xpx = Matrix{Float64}(undef, nb, nb), Vector{Float64}(undef, nb)
    hip_check(b.ctx, ccall((:jwas_hip_mega_get_gram, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}), b.ctx, k - 1, length(G), G, xpx))
    return G, xpx
end
hip_mega_estimate_bytes(n::Integer, p::Integer, ntraits::Integer, block_size::Integer=256) =
    ccall((:jwas_hip_mega_estimate_bytes, LIBJWAS_HIP), Int64, (Int64, Int64, Int32, Int32), n, p, ntraits, block_size)
hip_mega_end!(b::HipBackend) = hip_check(b.ctx, ccall((:jwas_hip_mega_end, LIBJWAS_HIP), Cint, (Ptr{Cvoid},), b.ctx))

"Unconstrained multi-trait BayesC with 5 to 8 traits on the device: Gibbs sampler I (_MTBayesABC_samplerI!,
markers/BayesianAlphabet/MTBayesABC.jl:57-127; csrc/mtjoint.hpp) with a full G common to all markers, a full R and Pi over the 2^t
joint states.  `hip_mtj_sweep!` takes Rinv = inv(vare), Ginv = inv(G) (t x t, symmetric) and log.(pi) over the states in the order
state = 1 + sum_k δ_k 2^(k-1), and returns what the Dirichlet and the two inverse-Wishart draws read.  Traits are 1-based here.
Limits: 5 <= t <= 8, blocks <= 256 markers, dense genotypes, complete records, no residual weights, no shards."
struct HipMtjParams
    iteration::UInt32
    reserved::UInt32
    seed::UInt64
    rinv::Ptr{Float64}
    ginv::Ptr{Float64}
    log_pi::Ptr{Float64}
    npi::Int64
end
struct HipMtjStats
    state_counts::Ptr{Float64}
    beta_ss::Ptr{Float64}
    alpha_ss::Ptr{Float64}
    resid_cp::Ptr{Float64}
    resid_sum::Ptr{Float64}
    n_changed::Float64
    step_ms::Float64
end
hip_mtj_begin!(b::HipBackend, ntraits::Integer, block_size::Integer=256) =
    hip_check(b.ctx, ccall((:jwas_hip_mtj_begin, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int32), b.ctx, ntraits, block_size))
hip_mtj_set_residual!(b::HipBackend, trait::Integer, r::Vector{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_mtj_set_residual, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), b.ctx, trait - 1, r))
function hip_mtj_residual(b::HipBackend, trait::Integer, n::Integer)
    r = Vector{Float64}(undef, n)
    hip_check(b.ctx, ccall((:jwas_hip_mtj_get_residual, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), b.ctx, trait - 1, r))
    return r
end
hip_mtj_set_state!(b::HipBackend, trait::Integer, α::Vector{Float64}, β::Vector{Float64}, δ::Vector{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_mtj_set_state, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.ctx, trait - 1, α, β, δ))
function hip_mtj_state(b::HipBackend, trait::Integer, p::Integer)
    α, β, δ = (Vector{Float64}(undef, p) for _ in 1:3)
    hip_check(b.ctx, ccall((:jwas_hip_mtj_get_state, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.ctx, trait - 1, α, β, δ))
    return α, β, δ
end
function hip_mtj_gram(b::HipBackend, k::Integer, nb::Integer)
    G, xpx = Matrix{Float64}(undef, nb, nb), Vector{Float64}(undef, nb)
    hip_check(b.ctx, ccall((:jwas_hip_mtj_gram, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}), b.ctx, k - 1, length(G), G, xpx))
    return G, xpx
end
function hip_mtj_sweep!(b::HipBackend, iter::Integer, seed::Integer, Rinv::Matrix{Float64}, Ginv::Matrix{Float64}, log_pi::Vector{Float64})
    t = size(Rinv, 1)
    counts, bb, aa, cp, rs = zeros(Float64, 2^t), zeros(Float64, t, t), zeros(Float64, t), zeros(Float64, t, t), zeros(Float64, t)
    S = Ref(HipMtjStats(pointer(counts), pointer(bb), pointer(aa), pointer(cp), pointer(rs), 0.0, 0.0))
    GC.@preserve Rinv Ginv log_pi counts bb aa cp rs begin
        P = HipMtjParams(UInt32(iter), UInt32(0), UInt64(seed), pointer(Rinv), pointer(Ginv), pointer(log_pi), Int64(length(log_pi)))
        hip_check(b.ctx, ccall((:jwas_hip_mtj_sweep, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipMtjParams}, Ref{HipMtjStats}), b.ctx, Ref(P), S))
    end
    return (state_counts=counts, beta_ss=bb, alpha_ss=aa, resid_cp=cp, resid_sum=rs, n_changed=S[].n_changed, step_ms=S[].step_ms)
end
hip_mtj_accumulate!(b::HipBackend, nsamples::Real) =
    hip_check(b.ctx, ccall((:jwas_hip_mtj_accumulate, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Float64), b.ctx, nsamples))
function hip_mtj_posterior(b::HipBackend, trait::Integer, p::Integer)
    m, m2, f = (Vector{Float64}(undef, p) for _ in 1:3)
    hip_check(b.ctx, ccall((:jwas_hip_mtj_posterior, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.ctx, trait - 1, m, m2, f))
    return m, m2, f
end
function hip_mtj_mul_alpha(b::HipBackend, trait::Integer, n_rows::Integer; output_rows::Bool=false)
    out = Vector{Float64}(undef, n_rows)
    hip_check(b.ctx, ccall((:jwas_hip_mtj_mul_alpha, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}), b.ctx, trait - 1, output_rows, out))
    return out
end
hip_mtj_end!(b::HipBackend) = hip_check(b.ctx, ccall((:jwas_hip_mtj_end, LIBJWAS_HIP), Cint, (Ptr{Cvoid},), b.ctx))

"Output rows in 2-bit packed storage beside packed training storage (Mi.output_genotypes, tools4genotypes.jl:290-296, for the
output_ID of check_outputID, input_data_validation.jl:143-196): a second packed matrix decoded with the training means and centring.
`payload` is p x stride in the .jgb2 field layout, one marker per COLUMN of the Julia matrix (stride = size(payload, 1) >= cld(n_out, 4)).
`hip_plink_commit_output!` follows a jwas_hip_plink_scan of the output individuals; `selected` is the training selection, 0-based.
`hip_ebv_output` returns getEBV (output.jl:281-306) of all traits, n_out x ntraits, column k the bits of jwas_hip_mul_alpha_output(k)."
hip_load_output_packed2bit!(b::HipBackend, payload::Matrix{UInt8}, n_out::Integer) =
    hip_check(b.ctx, ccall((:jwas_hip_load_output_packed2bit, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int64, Int64, Int64),
                           b.ctx, payload, n_out, size(payload, 2), size(payload, 1)))
hip_plink_commit_output!(b::HipBackend, selected::Vector{Int64}) =
    hip_check(b.ctx, ccall((:jwas_hip_plink_commit_output, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64), b.ctx, selected, length(selected)))
function hip_get_output_packed2bit(b::HipBackend, j0::Integer, m::Integer, n_out::Integer)
    out = Matrix{UInt8}(undef, cld(n_out, 4), m)
    hip_check(b.ctx, ccall((:jwas_hip_get_output_packed2bit, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{UInt8}, Int64), b.ctx, j0, m, out, size(out, 1)))
    return out
end
function hip_ebv_output(b::HipBackend, n_out::Integer, ntraits::Integer)
    out = Matrix{Float32}(undef, n_out, ntraits)
    hip_check(b.ctx, ccall((:jwas_hip_ebv_output, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float32}), b.ctx, out))
    return out
end

"""
GBLUP (markers/readgenotypes.jl:403-408, markers/BayesianAlphabet/GBLUP.jl; csrc/gblup.hpp).  `hip_grm` returns the relationship
matrix (Z Z' + 1e-5 I) / p of the loaded dense matrix, Z = X ./ divisor with divisor = sqrt.(2p .* (1 .- p)) in the matrix's element
type.  After GBLUP_setup has loaded L = eigen(G).vectors as the dense matrix and called jwas_hip_init_state, `hip_gblup_begin!` takes
D = abs.(eigen(G).values) and `hip_gblup_step!` replaces GBLUP! / megaGBLUP! (diagonal = true) / MTGBLUP! on the resident residual and
effects; it returns sum_i alpha_i alpha_i' / D_i (the variance draw), sum r r' and sum r.  vare and G are t x t, row-major.
"""
struct HipGblupParams
    iteration::UInt32
    diagonal::Int32
    seed::UInt64
    first_trait::UInt32
    reserved::UInt32
    vare::NTuple{16,Float64}
    G::NTuple{16,Float64}
end
struct HipGblupStats
    alpha_ss::NTuple{16,Float64}
    resid_ss::NTuple{16,Float64}
    resid_sum::NTuple{4,Float64}
    step_ms::Float64
end
function hip_grm(b::HipBackend, divisor::Vector{T}, n::Integer) where {T<:Union{Float32,Float64}}
    K = Matrix{T}(undef, n, n)
    hip_check(b.ctx, ccall((:jwas_hip_grm, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), b.ctx, divisor, K))
    return K
end
# ... of the context's 2-bit packed genotypes (hip_load_jgb2!, a committed PLINK scan): Float32, the bits of hip_grm on the decoded columns
function hip_grm_packed(b::HipBackend, divisor::Vector{Float32}, n::Integer)
    K = Matrix{Float32}(undef, n, n)
    hip_check(b.ctx, ccall((:jwas_hip_grm_packed2bit, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), b.ctx, divisor, K))
    return K
end
hip_grm_estimate_bytes(n::Integer, p::Integer, bits::Integer=32) =
    ccall((:jwas_hip_grm_estimate_bytes, LIBJWAS_HIP), Int64, (Int64, Int64, Int32), n, p, bits)
hip_gblup_begin!(b::HipBackend, D::Vector{Float64}) =
    hip_check(b.ctx, ccall((:jwas_hip_gblup_begin, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.ctx, D))
function hip_gblup_step!(b::HipBackend, iter::Integer, seed::Integer, vare::Matrix{Float64}, G::Matrix{Float64}; diagonal::Bool=false, first_trait::Integer=0)
    t = size(vare, 1)
    pad(M) = ntuple(i -> i <= t * t ? Float64(permutedims(M)[i]) : 0.0, 16)
    P = HipGblupParams(UInt32(iter), Int32(diagonal || t == 1), UInt64(seed), UInt32(first_trait), UInt32(0), pad(vare), pad(G))
    S = Ref(HipGblupStats(ntuple(_ -> 0.0, 16), ntuple(_ -> 0.0, 16), ntuple(_ -> 0.0, 4), 0.0))
    hip_check(b.ctx, ccall((:jwas_hip_gblup_step, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipGblupParams}, Ref{HipGblupStats}), b.ctx, Ref(P), S))
    sq(v) = permutedims(reshape(collect(v[1:t * t]), t, t))
    return (alpha_ss = sq(S[].alpha_ss), resid_ss = sq(S[].resid_ss), resid_sum = collect(S[].resid_sum[1:t]), step_ms = S[].step_ms)
end
function hip_gblup_rhs(b::HipBackend, n::Integer, t::Integer)
    out = Matrix{Float64}(undef, t, n)                       # (row-major n x t on the C side)
    hip_check(b.ctx, ccall((:jwas_hip_gblup_get_rhs, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), b.ctx, length(out), out))
    return permutedims(out)
end
hip_gblup_estimate_bytes(n::Integer, ntraits::Integer, bits::Integer=32) =
    ccall((:jwas_hip_gblup_estimate_bytes, LIBJWAS_HIP), Int64, (Int64, Int32, Int32), n, ntraits, bits)
hip_gblup_end!(b::HipBackend) = hip_check(b.ctx, ccall((:jwas_hip_gblup_end, LIBJWAS_HIP), Cint, (Ptr{Cvoid},), b.ctx))

"""
Single-step analysis (single_step/SSBR.jl:83-159): the imputation M_n = A^nn \\ (-A^ng M_g) on the device.  `hip_ss_begin!` takes the
factors of A^nn as CSR with 0-based int32 columns ascending within a row (L with its unit diagonal last, U with its diagonal first),
the permutations of Pr A^nn Pc = L U (0-based) and A^ng as CSR; it returns the markers per chunk the byte budget pays for.
`hip_ss_set_rows!` names the rows (0-based, pedigree order [non-genotyped; genotyped]) behind the rows of target 0 (the sweep
matrix) or 1 (the output matrix); `hip_ss_impute!` solves one chunk and writes it into both; `hip_ss_solve_host` returns a few
columns in Float64 (the J vector of make_JVecs).
"""
function hip_ss_begin!(b::HipBackend, n_n::Integer, g::Integer, Lp::Vector{Int64}, Lc::Vector{Int32}, Lv::Vector{Float64},
                       Up::Vector{Int64}, Uc::Vector{Int32}, Uv::Vector{Float64}, perm_r::Vector{Int32}, perm_c::Vector{Int32},
                       Ap::Vector{Int64}, Ac::Vector{Int32}, Av::Vector{Float64}, budget_bytes::Integer)
    ldc = Ref{Int64}(0)
    hip_check(b.ctx, ccall((:jwas_hip_ss_begin, LIBJWAS_HIP), Cint,
                           (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32},
                            Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Int64, Ptr{Int64}),
                           b.ctx, n_n, g, Lp, Lc, Lv, Up, Uc, Uv, perm_r, perm_c, Ap, Ac, Av, budget_bytes, ldc))
    return ldc[]
end
hip_ss_set_rows!(b::HipBackend, target::Integer, prow::Vector{Int32}) =
    hip_check(b.ctx, ccall((:jwas_hip_ss_set_rows, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Int32}), b.ctx, target, length(prow), prow))
"Mg: the g x count block of the genotyped individuals in the context's element type; j0 is 1-based."
hip_ss_impute!(b::HipBackend, j0::Integer, Mg::StridedMatrix{T}) where {T<:Union{Float32,Float64}} =
    hip_check(b.ctx, ccall((:jwas_hip_ss_impute, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64), b.ctx, j0 - 1, size(Mg, 2), Mg, stride(Mg, 2)))
"Columns j0 .. j0 + count - 1 (1-based) of a target with all `ld` rows, pad rows included (for tests)."
function hip_ss_get_columns(b::HipBackend, ::Type{T}, target::Integer, j0::Integer, count::Integer, ld::Integer) where {T<:Union{Float32,Float64}}
    out = Matrix{T}(undef, ld, count)
    hip_check(b.ctx, ccall((:jwas_hip_ss_get_columns, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Int64, Int64, Int64, Ptr{Cvoid}), b.ctx, target, j0 - 1, count, ld, out))
    return out
end
function hip_ss_solve_host(b::HipBackend, Mg::StridedMatrix{Float64}, prow::Vector{Int32})
    out = Matrix{Float64}(undef, length(prow), size(Mg, 2))
    hip_check(b.ctx, ccall((:jwas_hip_ss_solve_host, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int64, Ptr{Int32}, Ptr{Float64}),
                           b.ctx, size(Mg, 2), Mg, stride(Mg, 2), length(prow), prow, out))
    return out
end
hip_ss_estimate_bytes(n_n::Integer, g::Integer, nnz_l::Integer, nnz_u::Integer, nnz_a::Integer, markers_per_chunk::Integer) =
    ccall((:jwas_hip_ss_estimate_bytes, LIBJWAS_HIP), Int64, (Int64, Int64, Int64, Int64, Int64, Int64), n_n, g, nnz_l, nnz_u, nnz_a, markers_per_chunk)
hip_ss_end!(b::HipBackend) = hip_check(b.ctx, ccall((:jwas_hip_ss_end, LIBJWAS_HIP), Cint, (Ptr{Cvoid},), b.ctx))

"ycorr .+= shift on the device: the residual correction of an all-ones design column (intercept step, solver.jl:143-162)."
hip_residual_add_scalar!(b::HipBackend, trait::Integer, shift::Real) =
    hip_check(b.ctx, ccall((:jwas_hip_residual_add_scalar, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Cdouble), b.ctx, trait, shift))

_z16(::Type{T}) where {T} = ntuple(_ -> zero(T), 16)

"Parameters of a single-trait BayesC / BayesR sweep (the multi-trait samplers fill vare / var_effect / log_prior_states row-major)."
function HipSweepParams(method::Integer, iter::Integer, seed::Integer; vare::Real, var_effect::Real, pi::Real=0.0,
                        pi_classes=(0.0, 0.0, 0.0, 0.0), gamma=(0.0, 0.01, 0.1, 1.0), nreps::Integer=1,
                        marker_offset::Integer=0, independent_blocks::Bool=false,
                        pi_vec::Ptr{Float64}=Ptr{Float64}(C_NULL), pi_matrix::Ptr{Float64}=Ptr{Float64}(C_NULL),
                        var_effect_vec::Ptr{Float32}=Ptr{Float32}(C_NULL), section_solve::Bool=false, group_launch::Bool=false)
    HipSweepParams(Int32(method), Int32(1), Int32(nreps), UInt32(iter), UInt64(seed), UInt32(marker_offset),
                   UInt32(independent_blocks), Base.setindex(_z16(Float32), Float32(vare), 1),
                   Base.setindex(_z16(Float32), Float32(var_effect), 1), Float64(pi), NTuple{4,Float64}(pi_classes),
                   NTuple{4,Float64}(gamma), _z16(Float64), var_effect_vec, pi_vec, pi_matrix, Ptr{Float64}(C_NULL),
                   Ptr{Float32}(C_NULL), Base.setindex(_z16(Float64), Float64(vare), 1),
                   Base.setindex(_z16(Float64), Float64(var_effect), 1), Ptr{Float64}(C_NULL),      # (the Float64 context's copies)
                   Int32(section_solve), Int32(group_launch))                                        # Rule T (multi-trait sampler I, dense prior); grouped launches
end

"One marker sweep = one call of BayesABC! / BayesR! / MTBayesABC! (BayesABC.jl:60-80, BayesR.jl:45-97, MTBayesABC.jl:57-127)."
function hip_sweep!(b::HipBackend, P::HipSweepParams)
    S = Ref{HipSweepStats}()
    hip_check(b.ctx, ccall((:jwas_hip_sweep, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipSweepParams}, Ref{HipSweepStats}), b.ctx, Ref(P), S))
    return S[]
end

# ---- marker shards over the GPUs of a node (one Julia process / task per GPU) -----------------------------------------
"128-byte RCCL id: rank 0 creates it and hands it to the other ranks (a file, a socket, MPI.bcast ...)."
function hip_comm_unique_id()
    id = Vector{UInt8}(undef, 128)
    rc = ccall((:jwas_hip_comm_unique_id, LIBJWAS_HIP), Cint, (Ptr{UInt8},), id)
    rc == 0 || error("libjwas_hip: " * hip_error(C_NULL))
    return id
end
hip_comm_init!(b::HipBackend, id::Vector{UInt8}, rank::Integer, world::Integer) =
    hip_check(b.ctx, ccall((:jwas_hip_comm_init, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32, Int32), b.ctx, id, rank, world))

"(rank, world) of the attached communicator as RCCL reports them (ncclCommUserRank / ncclCommCount)."
function hip_comm_info(b::HipBackend)
    r, w = Ref{Int32}(0), Ref{Int32}(1)
    hip_check(b.ctx, ccall((:jwas_hip_comm_info, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}), b.ctx, r, w))
    return Int(r[]), Int(w[])
end

"Sweep of this rank's markers + on-device reconcile (one ncclAllReduce of delta r and the packed statistics, BayesABC.jl:205-253)."
function hip_sweep_sharded!(b::HipBackend, P::HipSweepParams)
    S = Ref{HipSweepStats}()
    hip_check(b.ctx, ccall((:jwas_hip_sweep_sharded, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Ref{HipSweepParams}, Ref{HipSweepStats}), b.ctx, Ref(P), S))
    return S[]
end

# ---- posterior accumulators and EBV ------------------------------------------------------------------------------------
hip_accumulate!(b::HipBackend, nsamples::Real) =
    hip_check(b.ctx, ccall((:jwas_hip_accumulate, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Cdouble), b.ctx, nsamples))

function hip_posterior(b::HipBackend, trait::Integer)
    m, m2, f = (Vector{Float32}(undef, b.nMarkers) for _ in 1:3)
    hip_check(b.ctx, ccall((:jwas_hip_get_posterior, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                           b.ctx, trait, m, m2, f))
    return m, m2, f          # output_posterior_mean_variance (output.jl:568-577): mean(alpha), mean(alpha^2), model frequency
end

function hip_mul_alpha(b::HipBackend, trait::Integer)
    out = Vector{Float32}(undef, b.nObs)
    hip_check(b.ctx, ccall((:jwas_hip_mul_alpha, LIBJWAS_HIP), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}), b.ctx, trait, out))
    return out               # getEBV's X*alpha (output.jl:281-306)
end

"Drop-in for BayesABC!(Mi, ycorr, vare, locus_effect_variances) (BayesABC.jl:10-14) when Mi.storage_mode == :hip."
function BayesABC_hip!(Mi, ycorr::Vector{Float32}, vare::Float32, varEffect::Float32, iter::Integer, seed::Integer)
    b = Mi.hip_backend
    hip_set_residual!(b, 0, ycorr)
    pvec = Mi.π isa AbstractVector ? Vector{Float64}(Mi.π) : Float64[]
    length(pvec) in (0, b.nMarkers) ||                       # bayesabc_pi_vector (BayesABC.jl:16-22)
        error("BayesABC pi vector length $(length(pvec)) must match the number of markers ($(b.nMarkers)).")
    S = GC.@preserve pvec hip_sweep!(b, HipSweepParams(JWAS_HIP_BAYESC, iter, seed; vare=vare, var_effect=varEffect,
                                                       pi=Mi.π isa Number ? Mi.π : 0.0,
                                                       pi_vec=isempty(pvec) ? Ptr{Float64}(C_NULL) : pointer(pvec)))
    hip_get_residual!(b, 0, ycorr)
    return S          # sum_delta -> samplePi (Pi.jl:7-9); alpha_ss -> sample_variance (variance_components.jl:160-162);
end                   # resid_ss -> residual variance (:60-66): no O(p) host pass is needed

end # module
