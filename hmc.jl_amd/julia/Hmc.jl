# Hmc.jl -- Julia host module over libhmcgibbs.so (C ABI: include/hmcg.h).
#
# Drop-in for the data-parallel hot path of joe5saia/Hmc.jl: the same unexported names the
# reference's drivers call (code/run_hmm.jl:77,95,119,120) -- Hmc.estopt, Hmc.estimatemodel,
# Hmc.saveresults, Hmc.startdate/enddate/makey/yobs, Hmc.forecast, makedate -- plus the additive
# batched entry Hmc.estimatewindows.  All sampling happens in hand-written HIP kernels behind a
# thin ccall; this file is plumbing (argument marshalling, Julia-layout result arrays, CSV).
#
# STATUS: written against Julia >= 1.6 and NOT EXECUTED -- neither the build image nor the GPU box
# has a `julia` binary.  The tested host layer with the same surface is hmc.jl_amd/hmc.py; the C ABI
# it shares with this file is what the parity tests exercise.
#
# Wired: estimatemodel, estimatewindows (batched; `devices = [0,1,...]` partitions the windows over several GPUs through
# hmcg_estimate_batch_multi; `window_ids` pins the RNG streams), estimatesignals! (signal Monte-Carlo path incl. signals
# past the end date), saveresults with and without signals -- written by the library's native CSV writer
# (hmcg_save_results_csv: CSV.jl 0.5.16 float text, 250k rows x 5 files in under a second).  Not wired here (available
# through the C ABI and the Python host layer): checkpoint/resume, the smoothed-probability output, the correlation
# workbook writer (calccorr's matrices themselves: estimatewindows(...; corr=true)).  calccdfs / predictive_cdf: the
# predictive CDFs of code/hassan_cdfs/calc_cdfs.jl from the draws, on the device (hmcg_predictive_cdf).  calcbias /
# bias_moments: uncerbias and totalbias of code/hassan_cdfs/bias_calcs.jl likewise (hmcg_bias_moments).  calcmoments /
# mixture_moments: what code/skewness.jl and code/alt_forecasts.jl ask of the summary rows, asked of the draws
# (hmcg_mixture_moments); calcskewness / altforecasts: the two scripts themselves, in closed form.  calcchain /
# chain_density: the binned chain densities and running means plots/mcplots.jl and plots/timeseriesplots.jl draw
# (hmcg_chain_density).  calcess / chain_autocorr: autocovariances, integrated autocorrelation time, effective sample size,
# Monte-Carlo standard error and split-R-hat of the draws (hmcg_chain_autocorr; no reference script).  calcquantiles /
# chain_quantiles: the exact median and credible limits of the draws by selection (hmcg_chain_quantiles).  calcergodic /
# ergodic_moments: the stationary regime law, durations and long-run moments of the draws (hmcg_ergodic_moments).  calcfan /
# predictive_quantiles: the median, forecast bands and value-at-risk levels of the predictive mixture (hmcg_predictive_quantiles).  calcscores /
# predictive_scores: CRPS, probability integral transform and density of the predictive mixture at the realised value
# (hmcg_predictive_scores; no reference script).  runaggregate /
# calcdispersion of the reference work unchanged on the files written here (same names, columns and float text).
#
# Reference lines mirrored: estopt src/Hmc.jl:17-73, accessors :85-107, makedate :573-582,
# forecast :658-667, basicsave/saveresults :707-748, estimatemodel :850-865.
module Hmc

using Dates
using Printf
using LinearAlgebra

export makedate

const LIBHMCG = get(ENV, "HMCG_LIBRARY", joinpath(@__DIR__, "..", "csrc", "libhmcgibbs.so"))
const HMCG_MAXH = 8

# ---- C structs (include/hmcg.h) ------------------------------------------------------------
struct hmcg_config
    struct_size::Int32
    W::Int32
    K::Int32
    ldY::Int32
    max_T::Int32
    burnin::Int32
    nrun::Int32
    H::Int32
    horizons::NTuple{HMCG_MAXH,Int32}
    seed::UInt64
    window_base::UInt32
    device::Int32
    flags::Int32
    threads_per_window::Int32
    sweep_base::Int32
    sweep_count::Int32
    alpha::Float64
    nu::Float64
    kappa::Float64
    n_samples::Int32
    blend_mask::Int32
    min_T::Int32                      # device entry: hint for the length-bucketed dispatch (host entries ignore it)
    reserved3::Int32
end

struct hmcg_extras
    struct_size::Int32
    reserved::Int32
    x_init::Ptr{Int32}
    x_final::Ptr{Int32}
    pif_final::Ptr{Float64}
    xstate::Ptr{UInt8}
    sumacc::Ptr{Float64}
    window_ids::Ptr{UInt32}
    sig_range::Ptr{Int32}
    save_range::Ptr{Int32}
    sigma_signal::Ptr{Float64}
    sigvals::Ptr{Float64}
    nsave_ld::Int32
    reserved2::Int32
    end_pos::Ptr{Int32}
    pi_smooth_mean::Ptr{Float64}
    pi_filter_mean::Ptr{Float64}
    corr::Ptr{Float64}
    pi_smooth_draws::Ptr{Float64}     # [W][K][ldY][nd] = (Nrun, N, D, W): samples.pib of every kept draw (src/Hmc.jl:552,558)
    sample_summary::Ptr{Float64}      # [W][n_samples][3K+K^2+2H]: runaggregate's (date, signalid) rows of a signal run (hmcg.h)
end
const HMCG_MAXTAIL = 256
const HMCG_MAXDEV = 16

struct hmcg_timing                    # include/hmcg.h (ABI 109)
    kernel_ms::Float64
    launches::Int32
    threads_per_window::Int32
    steps_per_thread::Int32
    lds_bytes::Int32
    helper_waves::Int32
    device::Int32
    call_ms::Float64
    windows::Int32
    occupancy::Int32
    buckets::Int32
    streaming::Int32
end

const HMCG_PRED_ROUND5 = Int32(1)
struct hmcg_predictive                # include/hmcg.h: predictive CDFs of the regime mixture (calc_cdfs.jl)
    struct_size::Int32
    W::Int32
    K::Int32
    device::Int32
    nd::Int64
    nd_ld::Int64
    G::Int32
    n_h::Int32
    horizons::NTuple{HMCG_MAXH,Int32}
    flags::Int32
    reserved::Int32
end

const HMCG_BIAS_ROUND5 = Int32(1)
struct hmcg_bias                      # include/hmcg.h: uncertainty-bias moments of the draws (bias_calcs.jl)
    struct_size::Int32
    W::Int32
    K::Int32
    device::Int32
    nd::Int64
    nd_ld::Int64
    horizon::Int32
    H::Int32
    flags::Int32
    reserved::Int32
end
bias_stride(K::Integer) = 2 + 2K + 4K^2     # HMCG_BIAS_STRIDE

const HMCG_MIX_ROUND5 = Int32(1)
const HMCG_MIX_STRIDE = 8
struct hmcg_mixmom                    # include/hmcg.h: predictive mixture moments of the draws (skewness.jl, alt_forecasts.jl)
    struct_size::Int32
    W::Int32
    K::Int32
    device::Int32
    nd::Int64
    nd_ld::Int64
    n_h::Int32
    flags::Int32
    horizons::NTuple{HMCG_MAXH,Int32}
end
const HMCG_DENS_ROUND5 = Int32(1)
struct hmcg_density                   # include/hmcg.h: chain densities and running means of the draws (plots/mcplots.jl)
    struct_size::Int32
    W::Int32
    C::Int32
    device::Int32
    nd::Int64
    nd_ld::Int64
    B::Int32
    n_cuts::Int32
    cuts::NTuple{HMCG_MAXH,Int64}
    trace_len::Int32
    flags::Int32
    trace_stride::Int64
end
const HMCG_ACF_ROUND5 = Int32(1)
const HMCG_ACF_STRIDE = 8
struct hmcg_autocorr                  # include/hmcg.h: autocorrelation, effective sample size and split-R-hat of the draws
    struct_size::Int32
    W::Int32
    C::Int32
    device::Int32
    nd::Int64
    nd_ld::Int64
    L::Int32
    flags::Int32
end
const HMCG_ORD_ROUND5 = Int32(1)
const HMCG_ORD_MAXQ = 16
const HMCG_ORD_STRIDE = 4
struct hmcg_quantiles                 # include/hmcg_order.h (the companion header): exact quantiles of the draws
    struct_size::Int32
    W::Int32
    C::Int32
    device::Int32
    nd::Int64
    nd_ld::Int64
    Q::Int32
    flags::Int32
    probs::NTuple{16,Float64}
end
const HMCG_ERG_ROUND5 = Int32(1)
struct hmcg_ergodic                   # include/hmcg_ergodic.h (a companion header): ergodic law, durations, long-run moments
    struct_size::Int32
    W::Int32
    K::Int32
    device::Int32
    nd::Int64
    nd_ld::Int64
    flags::Int32
    reserved::Int32
end
const HMCG_SCORE_ROUND5 = Int32(1)
const HMCG_SCORE_DRAWS_DEFAULT = 4096
const HMCG_SCORE_STRIDE = 5
struct hmcg_score                     # include/hmcg_score.h (a companion header): proper scores of the predictive regime mixture
    struct_size::Int32
    W::Int32
    K::Int32
    device::Int32
    nd::Int64
    nd_ld::Int64
    n_h::Int32
    flags::Int32
    horizons::NTuple{8,Int32}
    stride::Int64
    reserved::Int64
end
const HMCG_FAN_ROUND5 = Int32(1)
const HMCG_FAN_MAXP = 16
const HMCG_FAN_STRIDE = 5
struct hmcg_fan                       # include/hmcg_fan.h (a companion header): quantiles of the predictive regime mixture
    struct_size::Int32
    W::Int32
    K::Int32
    device::Int32
    nd::Int64
    nd_ld::Int64
    n_h::Int32
    n_p::Int32
    horizons::NTuple{8,Int32}
    rounds::Int32
    flags::Int32
    probs::NTuple{16,Float64}
    reserved::Int64
end

last_error() = unsafe_string(ccall((:hmcg_last_error, LIBHMCG), Cstring, ()))
device_count() = Int(ccall((:hmcg_device_count, LIBHMCG), Cint, ()))

# ---- options (field names and keyword defaults of the reference struct) ---------------------
mutable struct estopt
    rawdata::Vector{Float64}
    dates::Vector{Date}
    sampleRange::AbstractVector{Int}
    signalRange::AbstractVector{Int}
    signalSave::AbstractVector{Int}
    obsRange::AbstractVector{Int}
    endIndex::Int
    horizons::Vector{Int}
    D::Int
    burnin::Int
    Nrun::Int
    signalburnin::Int
    signalNrun::Int
    noise::Float64
    noiseSamples::Int
    σsignal::Float64
    series::String
    seed::Int
    function estopt(rawdata, dates; sampleRange=1:121, signalRange=2:1, signalSave=2:1, endIndex=121,
                    horizons=[12], D=3, burnin=1_000, Nrun=1_000, signalburnin=1_000, signalNrun=1_000,
                    noise=0.0, noiseSamples=1, σsignal=0.0, series="offical", seed=1234)
        issubset(signalRange, sampleRange) || @error "signalRange is not a subset of sampleRange"
        issubset(signalSave, signalRange) || @error "signalSave is not a subset of signalRange"
        new(Vector{Float64}(rawdata), Vector{Date}(dates), sampleRange, signalRange, signalSave,
            setdiff(sampleRange, signalRange), endIndex, collect(Int, horizons), D, burnin, Nrun,
            signalburnin, signalNrun, noise, noiseSamples, σsignal, series, seed)
    end
end

update_itators!(opt::estopt) = (opt.obsRange = setdiff(opt.sampleRange, opt.signalRange); nothing)
makey(x::estopt) = x.rawdata[x.sampleRange]
enddate(x::estopt, extra=0) = x.dates[x.endIndex + extra]
startdate(x::estopt) = x.dates[first(x.sampleRange)]
yobs(x::estopt, index) = x.rawdata[index]
yend(x::estopt, extra=0) = x.rawdata[x.endIndex + extra]

function makedate(x)
    y = Int(x)
    Dates.Date(y ÷ 12 + 1960, mod(y, 12) + 1)
end

function forecast(μ, A, πb, horizon, Yreal)
    f = dot(vec(πb' * A^horizon), μ)
    return f, f - Yreal
end

# ---- the ccall ---------------------------------------------------------------------------
function _check_live(opt::estopt; signals::Bool=false)
    (signals || isempty(opt.signalRange)) || error("this entry takes windows without signals; use estimatesignals!")
    (first(opt.sampleRange) == 1 && collect(opt.sampleRange) == collect(1:last(opt.sampleRange))) ||
        error("sampleRange must be 1:N (src/Hmc.jl indexes window-relative arrays with absolute indices)")
    if !isempty(opt.signalRange)
        sr = collect(opt.signalRange)
        (sr == collect(first(sr):last(sr)) && last(sr) == last(opt.sampleRange)) ||
            error("signalRange must be a contiguous tail of sampleRange")
        0 <= last(sr) - opt.endIndex <= HMCG_MAXTAIL || error("sigLen = last(signalRange) - endIndex must lie in 0..$(HMCG_MAXTAIL)")
    end
end

_yreal(opt::estopt) = [opt.endIndex + h <= length(opt.rawdata) ? opt.rawdata[opt.endIndex + h] : NaN for h in opt.horizons]

"""
    estimatewindows(opts::Vector{estopt}; device=0, devices=nothing, keepdraws=true, window_ids=nothing)

One call for many windows (all must share D, burnin, Nrun, horizons, seed) -- what the reference fans out as
`sbatch --array=120-579`, one Julia process per end date (slurmscripts/base_estimation.sh:5,17).  `devices = [0, 1, ..., 7]`
partitions the windows over those GPUs inside the library (hmcg_estimate_batch_multi: one host thread per device,
results gathered into these arrays; bit-identical to the single-device call).  `window_ids` (UInt32 per window) pins
the RNG streams.  Returns
`(samples::Vector{NamedTuple}, summary::Matrix{Float64}, status::Vector{Int32})`; `summary[:, w]` holds the
means of the 5-digit-rounded draws in the order mu | sigma | pib_end | A(:) | forecasts.  `corr=true` adds a fourth
value, `ρ[:, :, w]`: the correlation matrix calccorr (src/Hmc.jl:1094-1163) computes per end date from the per-draw CSV
files, accumulated on the device (extras.corr; labels: `corrnames`); with `keepdraws=false` no draw leaves the GPU.
"""
function estimatewindows(opts::Vector{estopt}; device::Integer=0, devices=nothing, keepdraws::Bool=true, window_ids=nothing,
                         corr::Bool=false)
    foreach(_check_live, opts)
    o = opts[1]
    W = length(opts); K = o.D; H = length(o.horizons); nrun = o.Nrun
    Ts = Int32[length(x.sampleRange) for x in opts]
    ldY = Int(maximum(Ts))
    Y = zeros(Float64, ldY, W)                       # column w = window w  (C: Y[w][t])
    yreal = zeros(Float64, max(H, 1), W)
    for (w, x) in enumerate(opts)
        Y[1:Ts[w], w] = makey(x)
        H > 0 && (yreal[1:H, w] = _yreal(x))
    end
    hz = ntuple(i -> i <= H ? Int32(o.horizons[i]) : Int32(0), HMCG_MAXH)
    cfg = Ref(hmcg_config(Int32(sizeof(hmcg_config)), W, K, ldY, Int32(maximum(Ts)), o.burnin, nrun, H, hz,
                          UInt64(o.seed), UInt32(0), Int32(device), Int32(0), Int32(0), Int32(0), Int32(0), 0.0, 0.0,
                          0.0, Int32(0), Int32(0), Int32(0), Int32(0)))
    NS = 3K + K * K + 2H
    μ = keepdraws ? Array{Float64}(undef, nrun, K, W) : Float64[]
    σ = keepdraws ? Array{Float64}(undef, nrun, K, W) : Float64[]
    A = keepdraws ? Array{Float64}(undef, nrun, K, K, W) : Float64[]
    πe = keepdraws ? Array{Float64}(undef, nrun, K, W) : Float64[]
    fc = keepdraws ? Array{Float64}(undef, nrun, 2H, W) : Float64[]
    summary = Array{Float64}(undef, NS, W)
    status = zeros(Int32, W)
    NC = 3K + K * K + 1
    ρ = corr ? Array{Float64}(undef, NC, NC, W) : Float64[]      # symmetric: C row-major == Julia column-major
    p(a) = isempty(a) ? Ptr{Float64}(C_NULL) : pointer(a)
    wids = window_ids === nothing ? UInt32[] : Vector{UInt32}(window_ids)
    ex = Ref(hmcg_extras(Int32(sizeof(hmcg_extras)), Int32(0), C_NULL, C_NULL, C_NULL, C_NULL, C_NULL,
                         isempty(wids) ? Ptr{UInt32}(C_NULL) : pointer(wids), C_NULL, C_NULL, C_NULL, C_NULL, Int32(0), Int32(0),
                         C_NULL, C_NULL, C_NULL, corr ? pointer(ρ) : Ptr{Float64}(C_NULL), C_NULL, C_NULL))
    yr = H > 0 ? pointer(yreal) : Ptr{Float64}(C_NULL)
    rc = GC.@preserve Y Ts yreal μ σ A πe fc summary status wids ρ begin
        if devices === nothing
            ccall((:hmcg_estimate_batch, LIBHMCG), Cint,
                  (Ref{hmcg_config}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ref{hmcg_extras}, Ptr{Cvoid}),
                  cfg, Y, Ts, yr, p(μ), p(σ), p(A), p(πe), p(fc), summary, status, ex, C_NULL)
        else
            devs = Vector{Int32}(devices)
            ccall((:hmcg_estimate_batch_multi, LIBHMCG), Cint,
                  (Ref{hmcg_config}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ref{hmcg_extras}, Ptr{Cvoid}),
                  cfg, Int32(length(devs)), devs, Y, Ts, yr, p(μ), p(σ), p(A), p(πe), p(fc), summary, status, ex, C_NULL)
        end
    end
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    samples = NamedTuple[]
    if keepdraws
        for (w, x) in enumerate(opts)
            push!(samples, (μ = μ[:, :, w], σ = σ[:, :, w],
                            πb = reshape(πe[:, :, w], nrun, 1, K),   # only the last time step is produced (src/Hmc.jl:744,861)
                            A = A[:, :, :, w], forecasts = fc[:, :, w], obsdates = fill(enddate(x), nrun)))
        end
    end
    return corr ? (samples, summary, status, ρ) : (samples, summary, status)
end

"""
    corrnames(K, horizons) -> Vector{String}

Row / column labels of the matrices `estimatewindows(...; corr=true)` returns: what calccorr (src/Hmc.jl:1094-1163)
derives from the CSV headers -- μ1..K, σ1..K, π1..K, trans_i_j (i fastest), forecast_<first horizon>.
"""
corrnames(K::Integer, horizons) = vcat(["μ$i" for i in 1:K], ["σ$i" for i in 1:K], ["π$i" for i in 1:K],
                                       vec(["trans_$(i)_$(j)" for i in 1:K, j in 1:K]), ["forecast_$(horizons[1])"])

# ---- predictive CDFs (code/hassan_cdfs/calc_cdfs.jl:31-42) -----------------------------------------------------------
_predictive(W, K, nd, ld, G, horizons, device, round5) =
    hmcg_predictive(Int32(sizeof(hmcg_predictive)), Int32(W), Int32(K), Int32(device), Int64(nd), Int64(ld), Int32(G),
                    Int32(length(horizons)), ntuple(i -> i <= length(horizons) ? Int32(horizons[i]) : Int32(0), HMCG_MAXH),
                    round5 ? HMCG_PRED_ROUND5 : Int32(0), Int32(0))

"""
    predictive_cdf(μ, σ, πe, A, ys; horizons=[0], device=0, round5=true) -> Array (G, n_h, W)

hmcg_predictive_cdf over host draw arrays in the layouts estimatewindows fills -- μ, σ, πe (nrun, K, W), A (nrun, K, K, W),
`nothing` when every horizon is 0: per window and horizon the mean over the draws of
Σ_k ω[k] Φ((y - μ[k]) / sqrt(σ[k])), ω = πe A^h -- `expectationsbar` of calc_cdfs.jl:39-41 at h = 0.
"""
function predictive_cdf(μ::Array{Float64,3}, σ::Array{Float64,3}, πe::Array{Float64,3}, A, ys; horizons=[0], device::Integer=0,
                        round5::Bool=true)
    nrun, K, W = size(μ)
    grid = Vector{Float64}(collect(ys))
    cdf = Array{Float64}(undef, length(grid), length(horizons), W)
    pa = A === nothing ? Ptr{Float64}(C_NULL) : pointer(A)
    rc = GC.@preserve μ σ πe A grid cdf ccall((:hmcg_predictive_cdf, LIBHMCG), Cint,
        (Ref{hmcg_predictive}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
        _predictive(W, K, nrun, nrun, length(grid), horizons, device, round5), μ, σ, πe, pa, grid, cdf, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return cdf
end

"""
    predictive_cdf_device(W, K, nd, ld, dμ, dσ, dπe, dA, dgrid, G, dcdf; horizons=[0], device=0, round5=true, stream=C_NULL)

hmcg_predictive_cdf_device over device pointers (dA = C_NULL when every horizon is 0); enqueued on `stream`
(C_NULL: the library's own) and not waited for.
"""
function predictive_cdf_device(W, K, nd, ld, dμ::Ptr{Float64}, dσ::Ptr{Float64}, dπe::Ptr{Float64}, dA::Ptr{Float64},
                               dgrid::Ptr{Float64}, G, dcdf::Ptr{Float64}; horizons=[0], device::Integer=0, round5::Bool=true,
                               stream::Ptr{Cvoid}=C_NULL)
    rc = ccall((:hmcg_predictive_cdf_device, LIBHMCG), Cint,
               (Ref{hmcg_predictive}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid},
                Ptr{Cvoid}), _predictive(W, K, nd, ld, G, horizons, device, round5), dμ, dσ, dπe, dA, dgrid, dcdf, stream, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return nothing
end

"""
    calccdfs(opts, ys=-5:.25:15; horizons=[0], device=0) -> (dates, ys, expectationsbar (G, n_h, W))

calc_cdfs.jl without the per-draw files and the plots: estimates the windows and takes the predictive CDFs from their draws
on the device.  `quantile.(Normal(), expectationsbar)` (Distributions) gives upstream's `finverse`.
"""
function calccdfs(opts::Vector{estopt}, ys=-5:.25:15; horizons=[0], device::Integer=0)
    samples, _, _ = estimatewindows(opts; device=device)
    W, K = length(opts), opts[1].D
    cat3(f) = cat((f(s) for s in samples)...; dims=3)
    μ, σ, πe = cat3(s -> s.μ), cat3(s -> s.σ), cat3(s -> s.πb[:, 1, :])
    A = any(h -> h > 0, horizons) ? cat((s.A for s in samples)...; dims=4) : nothing
    return [enddate(o) for o in opts], collect(ys), predictive_cdf(μ, σ, πe, A, ys; horizons=horizons, device=device)
end

# ---- uncertainty-bias moments (code/hassan_cdfs/bias_calcs.jl:40-53) ---------------------------------------------------
_bias(W, K, nd, ld, horizon, H, device, round5) =
    hmcg_bias(Int32(sizeof(hmcg_bias)), Int32(W), Int32(K), Int32(device), Int64(nd), Int64(ld), Int32(horizon), Int32(H),
              round5 ? HMCG_BIAS_ROUND5 : Int32(0), Int32(0))

"""
    bias_moments(μ, πe, A, forecasts; horizon=12, device=0, round5=true) -> (uncerbias (W), totalbias (W), mean (2K, W), cov (2K, 2K, W))

hmcg_bias_moments over host draw arrays in the layouts estimatewindows fills -- μ, πe (nrun, K, W), A (nrun, K, K, W)
(`nothing` when horizon is 0), forecasts (nrun, 2H, W) or `nothing`: per window `nab * covv * nab'` with
covv = cov(hcat(futstate, means)), nab = mean(hcat(means, futstate), dims=1), futstate = πe A^horizon per draw (the two column
orders differ upstream, bias_calcs.jl:49-51, and are kept), and the mean of forecasts[:, 2] (`totalbias`; NaN without
forecasts).  mean and cov are those of [futstate | means].
"""
function bias_moments(μ::Array{Float64,3}, πe::Array{Float64,3}, A, forecasts; horizon::Integer=12, device::Integer=0,
                      round5::Bool=true)
    nrun, K, W = size(μ)
    H = forecasts === nothing ? 0 : size(forecasts, 2) ÷ 2
    out = Array{Float64}(undef, bias_stride(K), W)
    pa = A === nothing ? Ptr{Float64}(C_NULL) : pointer(A)
    pf = forecasts === nothing ? Ptr{Float64}(C_NULL) : pointer(forecasts)
    rc = GC.@preserve μ πe A forecasts out ccall((:hmcg_bias_moments, LIBHMCG), Cint,
        (Ref{hmcg_bias}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
        _bias(W, K, nrun, nrun, horizon, H, device, round5), μ, πe, pa, pf, out, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    # the C block holds cov row-major; it is symmetric bit for bit, so the column-major reshape is the same matrix
    return out[1, :], out[2, :], out[3:2+2K, :], reshape(out[3+2K:end, :], 2K, 2K, W)
end

"""
    bias_moments_device(W, K, nd, ld, dμ, dπe, dA, dforecasts, H, dout; horizon=12, device=0, round5=true, stream=C_NULL)

hmcg_bias_moments_device over device pointers (dA = C_NULL when horizon is 0, dforecasts = C_NULL for no totalbias);
dout holds W * bias_stride(K) doubles; enqueued on `stream` (C_NULL: the library's own) and not waited for.
"""
function bias_moments_device(W, K, nd, ld, dμ::Ptr{Float64}, dπe::Ptr{Float64}, dA::Ptr{Float64}, dforecasts::Ptr{Float64}, H,
                             dout::Ptr{Float64}; horizon::Integer=12, device::Integer=0, round5::Bool=true,
                             stream::Ptr{Cvoid}=C_NULL)
    rc = ccall((:hmcg_bias_moments_device, LIBHMCG), Cint,
               (Ref{hmcg_bias}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}),
               _bias(W, K, nd, ld, horizon, H, device, round5), dμ, dπe, dA, dforecasts, dout, stream, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return nothing
end

"""
    calcbias(opts; horizon=12, device=0) -> (dates, uncerbias, totalbias)

bias_calcs.jl without the per-draw files and the plot: estimates the windows and takes both numbers from their draws on
the device.
"""
function calcbias(opts::Vector{estopt}; horizon::Integer=12, device::Integer=0)
    samples, _, _ = estimatewindows(opts; device=device)
    cat3(f) = cat((f(s) for s in samples)...; dims=3)
    μ, πe, fc = cat3(s -> s.μ), cat3(s -> s.πb[:, 1, :]), cat3(s -> s.forecasts)
    A = horizon > 0 ? cat((s.A for s in samples)...; dims=4) : nothing
    unc, tot, _, _ = bias_moments(μ, πe, A, size(fc, 2) > 0 ? fc : nothing; horizon=horizon, device=device)
    return [enddate(o) for o in opts], unc, tot
end

"""
    estimatemodel(opt) -> (μ, σ, πb, A, forecasts, obsdates)      (src/Hmc.jl:850-865)

`πb` has size (Nrun, 1, D): only `πb[:, end, :]` exists, which is all `saveresults` and `forecast` read.
"""
estimatemodel(opt::estopt; device::Integer=0) = estimatewindows([opt]; device=device)[1][1]

# One window on the signal path: n_samples chained noise samples of (burnin + nrun) sweeps (src/Hmc.jl:889-912).
# ---- predictive mixture moments (code/skewness.jl, code/alt_forecasts.jl) ----------------------------------------------
_mixmom(W, K, nd, ld, horizons, device, round5) =
    hmcg_mixmom(Int32(sizeof(hmcg_mixmom)), Int32(W), Int32(K), Int32(device), Int64(nd), Int64(ld), Int32(length(horizons)),
                round5 ? HMCG_MIX_ROUND5 : Int32(0), ntuple(i -> i <= length(horizons) ? Int32(horizons[i]) : Int32(0), HMCG_MAXH))

"""
    mixture_moments(μ, σ, πe, A; horizons=[0], device=0, round5=true) -> Array (8, n_h, W)

hmcg_mixture_moments over host draw arrays in the layouts estimatewindows fills -- μ, σ, πe (nrun, K, W), A (nrun, K, K, W),
`nothing` when every horizon is 0: per window and horizon the moments of the predictive law Σ_k ω[k] N(μ[k], σ[k]), ω = πe A^h,
pooled over the draws in closed form.  Rows: mean, variance, skewness, excess kurtosis, mean within-draw variance, variance
over the draws of the per-draw mean, mean per-draw skewness, mean weight.
"""
function mixture_moments(μ::Array{Float64,3}, σ::Array{Float64,3}, πe::Array{Float64,3}, A; horizons=[0], device::Integer=0,
                         round5::Bool=true)
    nrun, K, W = size(μ)
    out = Array{Float64}(undef, HMCG_MIX_STRIDE, length(horizons), W)
    pa = A === nothing ? Ptr{Float64}(C_NULL) : pointer(A)
    rc = GC.@preserve μ σ πe A out ccall((:hmcg_mixture_moments, LIBHMCG), Cint,
        (Ref{hmcg_mixmom}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
        _mixmom(W, K, nrun, nrun, horizons, device, round5), μ, σ, πe, pa, out, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return out
end

"""
    mixture_moments_device(W, K, nd, ld, dμ, dσ, dπe, dA, dout; horizons=[0], device=0, round5=true, stream=C_NULL)

hmcg_mixture_moments_device over device pointers (dA = C_NULL when every horizon is 0); dout holds W * n_h * 8 doubles;
enqueued on `stream` (C_NULL: the library's own) and not waited for.
"""
function mixture_moments_device(W, K, nd, ld, dμ::Ptr{Float64}, dσ::Ptr{Float64}, dπe::Ptr{Float64}, dA::Ptr{Float64},
                                dout::Ptr{Float64}; horizons=[0], device::Integer=0, round5::Bool=true, stream::Ptr{Cvoid}=C_NULL)
    rc = ccall((:hmcg_mixture_moments_device, LIBHMCG), Cint,
               (Ref{hmcg_mixmom}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}),
               _mixmom(W, K, nd, ld, horizons, device, round5), dμ, dσ, dπe, dA, dout, stream, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return nothing
end

"""
    calcmoments(opts; horizons=[0], device=0) -> (dates, moments (8, n_h, W))

skewness.jl's and alt_forecasts.jl's question asked of the draws: estimates the windows and takes the moments of the predictive
mixture from their draws on the device.
"""
function calcmoments(opts::Vector{estopt}; horizons=[0], device::Integer=0)
    samples, _, _ = estimatewindows(opts; device=device)
    cat3(f) = cat((f(s) for s in samples)...; dims=3)
    μ, σ, πe = cat3(s -> s.μ), cat3(s -> s.σ), cat3(s -> s.πb[:, 1, :])
    A = any(h -> h > 0, horizons) ? cat((s.A for s in samples)...; dims=4) : nothing
    return [enddate(o) for o in opts], mixture_moments(μ, σ, πe, A; horizons=horizons, device=device)
end

# ---- chain densities and running means (plots/mcplots.jl, plots/timeseriesplots.jl up to the drawing) ---------------------
_density(W, C, nd, ld, cuts, bins, trace, device, round5) =
    hmcg_density(Int32(sizeof(hmcg_density)), Int32(W), Int32(C), Int32(device), Int64(nd), Int64(ld), Int32(bins), Int32(length(cuts)),
                 ntuple(i -> i <= length(cuts) ? Int64(cuts[i]) : Int64(0), HMCG_MAXH), Int32(trace[1]),
                 round5 ? HMCG_DENS_ROUND5 : Int32(0), Int64(trace[2]))

"""
    chain_density(x; cuts=[nrun], bins=64, lo_hi=nothing, trace=(0, 1), device=0, round5=true)
        -> (range (2, C, W), counts (bins + 3, n_cuts, C, W), stats (2, n_cuts, C, W), trace (trace_len, C, W))

hmcg_chain_density over ONE host draw array in a layout estimatewindows fills, draw index first and window last -- μ, σ, πe
(nrun, K, W), A (nrun, K, K, W), forecasts (nrun, 2H, W); the axes between count as the C columns: per window and column the
binned counts of the chain prefixes 1:cuts[j] (mcplots.jl plotchain: 100000, 150000, 200000, 250000) on `bins` equal bins between
lo and hi (`lo_hi` (2, C, W), default the range of the finite draws), then the draws below lo, above hi and NaN; mean and variance
of each prefix; the running mean after i * trace[2] draws, i <= trace[1] (plotchainmean: (10000, 1)).
"""
function chain_density(x::Array{Float64}; cuts=nothing, bins::Integer=64, lo_hi=nothing, trace=(0, 1), device::Integer=0,
                       round5::Bool=true)
    nrun, W = size(x, 1), size(x, ndims(x))
    C = div(length(x), nrun * W)
    cuts = cuts === nothing ? [nrun] : cuts
    range = Array{Float64}(undef, 2, C, W)
    counts = Array{Int64}(undef, bins + 3, length(cuts), C, W)
    stats = Array{Float64}(undef, 2, length(cuts), C, W)
    tr = Array{Float64}(undef, trace[1], C, W)
    plh = lo_hi === nothing ? Ptr{Float64}(C_NULL) : pointer(lo_hi)
    ptr = trace[1] > 0 ? pointer(tr) : Ptr{Float64}(C_NULL)
    rc = GC.@preserve x lo_hi range counts stats tr ccall((:hmcg_chain_density, LIBHMCG), Cint,
        (Ref{hmcg_density}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
        _density(W, C, nrun, nrun, cuts, bins, trace, device, round5), x, plh, range, counts, stats, ptr, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return range, counts, stats, tr
end

"""
    chain_density_device(W, C, nd, ld, dx, dlo_hi, drange, dcounts, dstats, dtrace; cuts, bins=64, trace=(0, 1), device=0,
                         round5=true, stream=C_NULL)

hmcg_chain_density_device over device pointers (dlo_hi = C_NULL for the automatic range, dtrace = C_NULL without a running
mean); enqueued on `stream` (C_NULL: the library's own) and not waited for.
"""
function chain_density_device(W, C, nd, ld, dx::Ptr{Float64}, dlo_hi::Ptr{Float64}, drange::Ptr{Float64}, dcounts::Ptr{Int64},
                              dstats::Ptr{Float64}, dtrace::Ptr{Float64}; cuts=[nd], bins::Integer=64, trace=(0, 1),
                              device::Integer=0, round5::Bool=true, stream::Ptr{Cvoid}=C_NULL)
    rc = ccall((:hmcg_chain_density_device, LIBHMCG), Cint,
               (Ref{hmcg_density}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}),
               _density(W, C, nd, ld, cuts, bins, trace, device, round5), dx, dlo_hi, drange, dcounts, dstats, dtrace, stream, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return nothing
end

"""
    calcchain(opts, var=:μ; cuts=nothing, bins=64, trace=(0, 1), device=0) -> (dates, range, counts, stats, trace)

plotchain / plotchainmean / plot_mean / plot_var up to the drawing: estimates the windows and bins the chain of one variable
(:μ, :σ, :πe, :A or :forecasts) on the device.
"""
function calcchain(opts::Vector{estopt}, var::Symbol=:μ; cuts=nothing, bins::Integer=64, trace=(0, 1), device::Integer=0)
    samples, _, _ = estimatewindows(opts; device=device)
    pick(s) = var == :πe ? s.πb[:, 1, :] : getfield(s, var)
    x = cat((pick(s) for s in samples)...; dims=var == :A ? 4 : 3)
    return ([enddate(o) for o in opts], chain_density(x; cuts=cuts, bins=bins, trace=trace, device=device)...)
end

# ---- autocorrelation, effective sample size and split-R-hat of the draws (no reference script) ------------------------------
_autocorr(W, C, nd, ld, lags, device, round5) =
    hmcg_autocorr(Int32(sizeof(hmcg_autocorr)), Int32(W), Int32(C), Int32(device), Int64(nd), Int64(ld), Int32(lags),
                  round5 ? HMCG_ACF_ROUND5 : Int32(0))

"""
    chain_autocorr(x; lags=255, device=0, round5=true) -> (acov (lags + 1, C, W), diag (8, C, W))

hmcg_chain_autocorr over ONE host draw array in a layout estimatewindows fills, draw index first and window last -- μ, σ, πe
(nrun, K, W), A (nrun, K, K, W), forecasts (nrun, 2H, W); the axes between count as the C columns: per window and column the
biased autocovariances at lags 0:lags, and diag = mean, variance, tau (integrated autocorrelation time, Geyer's initial monotone
sequence), ess = nrun / tau, mcse = sqrt(variance * tau / nrun), pairs, truncated (1: `lags` is too short), rhat (split-R-hat of
the chain's two halves).
"""
function chain_autocorr(x::Array{Float64}; lags::Integer=255, device::Integer=0, round5::Bool=true)
    nrun, W = size(x, 1), size(x, ndims(x))
    C = div(length(x), nrun * W)
    acov = Array{Float64}(undef, lags + 1, C, W)
    diag = Array{Float64}(undef, HMCG_ACF_STRIDE, C, W)
    rc = GC.@preserve x acov diag ccall((:hmcg_chain_autocorr, LIBHMCG), Cint,
        (Ref{hmcg_autocorr}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
        _autocorr(W, C, nrun, nrun, lags, device, round5), x, acov, diag, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return acov, diag
end

"""
    chain_autocorr_device(W, C, nd, ld, dx, dacov, ddiag; lags=255, device=0, round5=true, stream=C_NULL)

hmcg_chain_autocorr_device over device pointers; enqueued on `stream` (C_NULL: the library's own) and not waited for.
"""
function chain_autocorr_device(W, C, nd, ld, dx::Ptr{Float64}, dacov::Ptr{Float64}, ddiag::Ptr{Float64}; lags::Integer=255,
                               device::Integer=0, round5::Bool=true, stream::Ptr{Cvoid}=C_NULL)
    rc = ccall((:hmcg_chain_autocorr_device, LIBHMCG), Cint,
               (Ref{hmcg_autocorr}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}),
               _autocorr(W, C, nd, ld, lags, device, round5), dx, dacov, ddiag, stream, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return nothing
end

"""
    calcess(opts, var=:μ; lags=255, device=0) -> (dates, acov, diag)

Estimates the windows and takes the convergence diagnostics of one variable's chain (:μ, :σ, :πe, :A or :forecasts) on the device.
"""
function calcess(opts::Vector{estopt}, var::Symbol=:μ; lags::Integer=255, device::Integer=0)
    samples, _, _ = estimatewindows(opts; device=device)
    pick(s) = var == :πe ? s.πb[:, 1, :] : getfield(s, var)
    x = cat((pick(s) for s in samples)...; dims=var == :A ? 4 : 3)
    return ([enddate(o) for o in opts], chain_autocorr(x; lags=lags, device=device)...)
end

# ---- exact quantiles and credible limits of the draws (include/hmcg_order.h; no reference script; not run) -----------------------
function _quantiles(W, C, nd, ld, probs, device, round5)
    1 <= length(probs) <= HMCG_ORD_MAXQ || error("1..$(HMCG_ORD_MAXQ) probabilities")
    p = ntuple(i -> i <= length(probs) ? Float64(probs[i]) : 0.0, HMCG_ORD_MAXQ)
    return hmcg_quantiles(Int32(sizeof(hmcg_quantiles)), Int32(W), Int32(C), Int32(device), Int64(nd), Int64(ld), Int32(length(probs)),
                          round5 ? HMCG_ORD_ROUND5 : Int32(0), p)
end

"""
    chain_quantiles(x; probs=(0.05, 0.5, 0.95), device=0, round5=true) -> (q (4, Q, C, W), n (2, C, W))

hmcg_chain_quantiles over ONE host draw array in a layout estimatewindows fills, draw index first and window last -- μ, σ, πe
(nrun, K, W), A (nrun, K, K, W), forecasts (nrun, 2H, W); the axes between count as the C columns: per window, column and
probability q = value, lo, hi, g -- the exact quantile (Julia's default definition), the two draws that bracket it and the
weight of hi -- selected on the device; n = the draws ranked and the NaNs left out.
"""
function chain_quantiles(x::Array{Float64}; probs=(0.05, 0.5, 0.95), device::Integer=0, round5::Bool=true)
    nrun, W = size(x, 1), size(x, ndims(x))
    C = div(length(x), nrun * W)
    q = Array{Float64}(undef, HMCG_ORD_STRIDE, length(probs), C, W)
    n = Array{Int64}(undef, 2, C, W)
    rc = GC.@preserve x q n ccall((:hmcg_chain_quantiles, LIBHMCG), Cint,
        (Ref{hmcg_quantiles}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}),
        _quantiles(W, C, nrun, nrun, probs, device, round5), x, q, n, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return q, n
end

"""
    chain_quantiles_device(W, C, nd, ld, dx, dq, dn; probs=(0.05, 0.5, 0.95), device=0, round5=true, stream=C_NULL)

hmcg_chain_quantiles_device over device pointers; enqueued on `stream` (C_NULL: the library's own) and not waited for.
"""
function chain_quantiles_device(W, C, nd, ld, dx::Ptr{Float64}, dq::Ptr{Float64}, dn::Ptr{Int64}; probs=(0.05, 0.5, 0.95),
                                device::Integer=0, round5::Bool=true, stream::Ptr{Cvoid}=C_NULL)
    rc = ccall((:hmcg_chain_quantiles_device, LIBHMCG), Cint,
               (Ref{hmcg_quantiles}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Cvoid}),
               _quantiles(W, C, nd, ld, probs, device, round5), dx, dq, dn, stream, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return nothing
end

"""
    calcquantiles(opts, var=:μ; probs=(0.05, 0.5, 0.95), device=0) -> (dates, q, n)

Estimates the windows and selects the quantiles of one variable's chain (:μ, :σ, :πe, :A or :forecasts) on the device.
"""
function calcquantiles(opts::Vector{estopt}, var::Symbol=:μ; probs=(0.05, 0.5, 0.95), device::Integer=0)
    samples, _, _ = estimatewindows(opts; device=device)
    pick(s) = var == :πe ? s.πb[:, 1, :] : getfield(s, var)
    x = cat((pick(s) for s in samples)...; dims=var == :A ? 4 : 3)
    return ([enddate(o) for o in opts], chain_quantiles(x; probs=probs, device=device)...)
end

# ---- ergodic regime law, durations and long-run moments of the draws (include/hmcg_ergodic.h; no reference script; not run) --------
_ergodic(W, K, nd, ld, device, round5) =
    hmcg_ergodic(Int32(sizeof(hmcg_ergodic)), Int32(W), Int32(K), Int32(device), Int64(nd), Int64(ld), round5 ? HMCG_ERG_ROUND5 : Int32(0), Int32(0))

"""
    ergodic_moments(μ, σ, A; cols=false, device=0, round5=true) -> (out (2, 2K + 2, W), n (2, W), cols (nrun, 2K + 2, W) or nothing)

hmcg_ergodic_moments over host draw arrays in the layouts estimatewindows fills -- μ, σ (nrun, K, W), A (nrun, K, K, W): per
draw the stationary law of the regimes (GTH elimination on the off-diagonal cells; the diagonal of A is never read), the
expected durations and the long-run mean and variance, the limit of πe A^h; out = their mean and variance over the good
draws (every column finite), n = the good draws and the rest; cols = the per-draw columns, in the layout chain_quantiles,
chain_density and chain_autocorr take.
"""
function ergodic_moments(μ::Array{Float64,3}, σ::Array{Float64,3}, A::Array{Float64,4}; cols::Bool=false, device::Integer=0,
                         round5::Bool=true)
    nrun, K, W = size(μ)
    C = 2K + 2
    out = Array{Float64}(undef, 2, C, W)
    n = Array{Int64}(undef, 2, W)
    cl = cols ? Array{Float64}(undef, nrun, C, W) : nothing
    pc = cols ? pointer(cl) : Ptr{Float64}(C_NULL)
    rc = GC.@preserve μ σ A out n cl ccall((:hmcg_ergodic_moments, LIBHMCG), Cint,
        (Ref{hmcg_ergodic}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}),
        _ergodic(W, K, nrun, nrun, device, round5), μ, σ, A, pc, out, n, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return out, n, cl
end

"""
    ergodic_moments_device(W, K, nd, ld, dμ, dσ, dA, dcols, dout, dn; device=0, round5=true, stream=C_NULL)

hmcg_ergodic_moments_device over device pointers (dcols = C_NULL when the per-draw columns are not kept); enqueued on `stream`
(C_NULL: the library's own) and not waited for.
"""
function ergodic_moments_device(W, K, nd, ld, dμ::Ptr{Float64}, dσ::Ptr{Float64}, dA::Ptr{Float64}, dcols::Ptr{Float64},
                                dout::Ptr{Float64}, dn::Ptr{Int64}; device::Integer=0, round5::Bool=true, stream::Ptr{Cvoid}=C_NULL)
    rc = ccall((:hmcg_ergodic_moments_device, LIBHMCG), Cint,
               (Ref{hmcg_ergodic}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Cvoid}),
               _ergodic(W, K, nd, ld, device, round5), dμ, dσ, dA, dcols, dout, dn, stream, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return nothing
end

"""
    calcergodic(opts; cols=false, device=0) -> (dates, out, n, cols)

Estimates the windows and takes the ergodic law, durations and long-run moments of their draws on the device.
"""
function calcergodic(opts::Vector{estopt}; cols::Bool=false, device::Integer=0)
    samples, _, _ = estimatewindows(opts; device=device)
    cat3(f) = cat((f(s) for s in samples)...; dims=3)
    A = cat((s.A for s in samples)...; dims=4)
    return ([enddate(o) for o in opts], ergodic_moments(cat3(s -> s.μ), cat3(s -> s.σ), A; cols=cols, device=device)...)
end

# ---- quantiles of the predictive regime mixture: the fan chart (include/hmcg_fan.h; no reference script; not run) ----------------
function _fan(W, K, nd, ld, probs, horizons, rounds, device, round5)
    length(probs) <= HMCG_FAN_MAXP || error("at most $HMCG_FAN_MAXP probabilities")
    length(horizons) <= 8 || error("at most 8 horizons")
    hz = ntuple(j -> j <= length(horizons) ? Int32(horizons[j]) : Int32(0), 8)
    ps = ntuple(i -> i <= length(probs) ? Float64(probs[i]) : 0.0, 16)
    return hmcg_fan(Int32(sizeof(hmcg_fan)), Int32(W), Int32(K), Int32(device), Int64(nd), Int64(ld), Int32(length(horizons)),
                    Int32(length(probs)), hz, Int32(rounds), round5 ? HMCG_FAN_ROUND5 : Int32(0), ps, Int64(0))
end

"""
    predictive_quantiles(μ, σ, πe, A, probs; horizons=(0,), rounds=0, device=0, round5=true)
        -> (out (5, n_p, n_h, W), range (2, W), flag (n_p, n_h, W))

hmcg_predictive_quantiles over host draw arrays in the layouts estimatewindows fills -- μ, σ, πe (nrun, K, W), A (nrun, K, K, W)
or nothing when every horizon is 0: per window, horizon and probability the quantile of the predictive law, the mixture of
nrun * K normals whose CDF predictive_cdf evaluates (the median, the forecast bands of a fan chart, value-at-risk levels), by
`rounds` rounds of grid refinement (0: the default, 4).  out = quantile, lo, hi, Flo, Fhi; flag 1 = NaN, 2 = p not reached,
4 = a flat last cell.
"""
function predictive_quantiles(μ::Array{Float64,3}, σ::Array{Float64,3}, πe::Array{Float64,3}, A::Union{Array{Float64,4},Nothing}, probs;
                              horizons=(0,), rounds::Integer=0, device::Integer=0, round5::Bool=true)
    nrun, K, W = size(μ)
    out = Array{Float64}(undef, HMCG_FAN_STRIDE, length(probs), length(horizons), W)
    rng = Array{Float64}(undef, 2, W)
    flag = Array{Int32}(undef, length(probs), length(horizons), W)
    pa = A === nothing ? Ptr{Float64}(C_NULL) : pointer(A)
    rc = GC.@preserve μ σ πe A out rng flag ccall((:hmcg_predictive_quantiles, LIBHMCG), Cint,
        (Ref{hmcg_fan}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}),
        _fan(W, K, nrun, nrun, probs, horizons, rounds, device, round5), μ, σ, πe, pa, out, rng, flag, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return out, rng, flag
end

"""
    predictive_quantiles_device(W, K, nd, ld, probs, dμ, dσ, dπe, dA, dout, drange, dflag; horizons=(0,), rounds=0, device=0,
                                round5=true, stream=C_NULL)

hmcg_predictive_quantiles_device over device pointers (dA = C_NULL when every horizon is 0); enqueued on `stream` (C_NULL: the
library's own) and not waited for.
"""
function predictive_quantiles_device(W, K, nd, ld, probs, dμ::Ptr{Float64}, dσ::Ptr{Float64}, dπe::Ptr{Float64}, dA::Ptr{Float64},
                                     dout::Ptr{Float64}, drange::Ptr{Float64}, dflag::Ptr{Int32}; horizons=(0,), rounds::Integer=0,
                                     device::Integer=0, round5::Bool=true, stream::Ptr{Cvoid}=C_NULL)
    rc = ccall((:hmcg_predictive_quantiles_device, LIBHMCG), Cint,
               (Ref{hmcg_fan}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ptr{Cvoid}),
               _fan(W, K, nd, ld, probs, horizons, rounds, device, round5), dμ, dσ, dπe, dA, dout, drange, dflag, stream, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return nothing
end

"""
    calcfan(opts, probs; horizons=(0,), rounds=0, device=0) -> (dates, out, range, flag)

Estimates the windows and takes the quantiles of their predictive law on the device: the fan chart per end date and horizon.
"""
function calcfan(opts::Vector{estopt}, probs; horizons=(0,), rounds::Integer=0, device::Integer=0)
    samples, _, _ = estimatewindows(opts; device=device)
    cat3(f) = cat((f(s) for s in samples)...; dims=3)
    A = any(h -> h > 0, horizons) ? cat((s.A for s in samples)...; dims=4) : nothing
    μ, σ, πe = cat3(s -> s.μ), cat3(s -> s.σ), cat3(s -> s.πb[:, 1, :])
    return ([enddate(o) for o in opts], predictive_quantiles(μ, σ, πe, A, probs; horizons=horizons, rounds=rounds, device=device)...)
end

"""
    write_fan(path, dates, probs, horizons, out, flag)

`date,horizon,p,quantile,lo,hi,flag`: one row per end date, horizon and probability.
"""
function write_fan(path, dates, probs, horizons, out, flag)
    open(path, "w") do io
        println(io, "date,horizon,p,quantile,lo,hi,flag")
        for (w, d) in enumerate(dates), (j, h) in enumerate(horizons), (i, p) in enumerate(probs)
            println(io, join((d, h, p, out[1, i, j, w], out[2, i, j, w], out[3, i, j, w], flag[i, j, w]), ','))
        end
    end
    return path
end

# ---- proper scores of the predictive regime mixture: CRPS, PIT, density (include/hmcg_score.h; no reference script; not run) ----
function _score(W, K, nd, ld, horizons, stride, device, round5)
    length(horizons) <= 8 || error("at most 8 horizons")
    hz = ntuple(j -> j <= length(horizons) ? Int32(horizons[j]) : Int32(0), 8)
    return hmcg_score(Int32(sizeof(hmcg_score)), Int32(W), Int32(K), Int32(device), Int64(nd), Int64(ld), Int32(length(horizons)),
                      round5 ? HMCG_SCORE_ROUND5 : Int32(0), hz, Int64(stride), Int64(0))
end

"(stride, n_u) of a score call over nd draws: stride 0 is the smallest stride that leaves at most 4 096 used draws."
function score_thinning(nd::Integer, stride::Integer=0)
    st = stride > 0 ? stride : max(1, cld(nd, HMCG_SCORE_DRAWS_DEFAULT))
    return st, cld(nd, st)
end

"""
    predictive_scores(μ, σ, πe, A, yreal; horizons=(0,), stride=0, device=0, round5=true) -> out (5, n_h, W)

hmcg_predictive_scores over host draw arrays in the layouts estimatewindows fills -- μ, σ, πe (nrun, K, W), A (nrun, K, K, W) or
nothing when every horizon is 0 -- and the realised values yreal (W, n_h), NaN for unknown: per window and horizon
crps = E|X - y| - E|X - X'| / 2 of the predictive law (the mixture of the used draws' normals), e_abs, e_pair, pit = F(y) and
pdf = F'(y).  stride: every stride-th draw is used (0: thinned to at most 4 096 draws, 1: the exact score).
"""
function predictive_scores(μ::Array{Float64,3}, σ::Array{Float64,3}, πe::Array{Float64,3}, A::Union{Array{Float64,4},Nothing},
                           yreal::Matrix{Float64}; horizons=(0,), stride::Integer=0, device::Integer=0, round5::Bool=true)
    nrun, K, W = size(μ)
    size(yreal) == (W, length(horizons)) || error("yreal must be (W, n_h)")
    out = Array{Float64}(undef, HMCG_SCORE_STRIDE, length(horizons), W)
    pa = A === nothing ? Ptr{Float64}(C_NULL) : pointer(A)
    rc = GC.@preserve μ σ πe A yreal out ccall((:hmcg_predictive_scores, LIBHMCG), Cint,
        (Ref{hmcg_score}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
        _score(W, K, nrun, nrun, horizons, stride, device, round5), μ, σ, πe, pa, yreal, out, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return out
end

"""
    predictive_scores_device(W, K, nd, ld, dμ, dσ, dπe, dA, dyreal, dout; horizons=(0,), stride=0, device=0, round5=true,
                             stream=C_NULL)

hmcg_predictive_scores_device over device pointers (dA = C_NULL when every horizon is 0; dyreal [n_h][W], dout [W][n_h][5]);
enqueued on `stream` (C_NULL: the library's own) and not waited for.
"""
function predictive_scores_device(W, K, nd, ld, dμ::Ptr{Float64}, dσ::Ptr{Float64}, dπe::Ptr{Float64}, dA::Ptr{Float64},
                                  dyreal::Ptr{Float64}, dout::Ptr{Float64}; horizons=(0,), stride::Integer=0, device::Integer=0,
                                  round5::Bool=true, stream::Ptr{Cvoid}=C_NULL)
    rc = ccall((:hmcg_predictive_scores_device, LIBHMCG), Cint,
               (Ref{hmcg_score}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}),
               _score(W, K, nd, ld, horizons, stride, device, round5), dμ, dσ, dπe, dA, dyreal, dout, stream, C_NULL)
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return nothing
end

"""
    calcscores(opts, rawdata; horizons=(0,), stride=0, device=0) -> (dates, yreal (W, n_h), out (5, n_h, W))

Estimates the windows and scores their predictive laws on the device against the series' own values rawdata[endIndex + h]
(NaN past its end).
"""
function calcscores(opts::Vector{estopt}, rawdata::Vector{Float64}; horizons=(0,), stride::Integer=0, device::Integer=0)
    samples, _, _ = estimatewindows(opts; device=device)
    cat3(f) = cat((f(s) for s in samples)...; dims=3)
    A = any(h -> h > 0, horizons) ? cat((s.A for s in samples)...; dims=4) : nothing
    μ, σ, πe = cat3(s -> s.μ), cat3(s -> s.σ), cat3(s -> s.πb[:, 1, :])
    yreal = [o.endIndex + h <= length(rawdata) ? rawdata[o.endIndex + h] : NaN for o in opts, h in horizons]
    return [enddate(o) for o in opts], yreal, predictive_scores(μ, σ, πe, A, yreal; horizons=horizons, stride=stride, device=device)
end

"""
    write_scores(path, dates, horizons, yreal, out)

`date,horizon,yreal,crps,e_abs,e_pair,pit,pdf`: one row per end date and horizon.
"""
function write_scores(path, dates, horizons, yreal, out)
    open(path, "w") do io
        println(io, "date,horizon,yreal,crps,e_abs,e_pair,pit,pdf")
        for (w, d) in enumerate(dates), (j, h) in enumerate(horizons)
            println(io, join((d, h, yreal[w, j], out[1, j, w], out[2, j, w], out[3, j, w], out[4, j, w], out[5, j, w]), ','))
        end
    end
    return path
end

"""
    scoresummary(out; bins=10) -> (mean_crps (n_h), count (n_h), pit_hist (bins, n_h))

Per horizon over the windows with a known realised value (a finite crps): the mean CRPS, their count and the PIT histogram on
equal bins of [0, 1] (a PIT of 1 counts in the last).
"""
function scoresummary(out::Array{Float64,3}; bins::Integer=10)
    n_h = size(out, 2)
    mean_crps, count, hist = fill(NaN, n_h), zeros(Int, n_h), zeros(Int, bins, n_h)
    for j in 1:n_h
        known = [w for w in 1:size(out, 3) if isfinite(out[1, j, w])]
        count[j] = length(known)
        isempty(known) || (mean_crps[j] = sum(out[1, j, w] for w in known) / length(known))
        for w in known
            hist[min(bins, 1 + floor(Int, out[4, j, w] * bins)), j] += 1
        end
    end
    return mean_crps, count, hist
end

function _summary_rows(datadir, stem)
    lines = readlines(joinpath(datadir, stem * "_summary.csv"))
    cells = [split(l, ',') for l in lines[2:end]]
    return split(lines[1], ','), [String(c[1]) for c in cells], [parse(Float64, c[j]) for c in cells, j in 2:length(cells[1])]
end

"""
    calcskewness(datadir; date=nothing) -> (date, mean, std, skewness)

code/skewness.jl:22-43 in closed form: the mixture Σ_k p_k N(μ_k, sqrt(var_k)) of the latest date's row (or `date`'s) of the
three `*_summary.csv` files, p normalised (:33); Σ_k p_k e_k (e_k² + 3 var_k) / std³ with e_k = μ_k - mean is what upstream's
10 000 000 variates estimate.
"""
function calcskewness(datadir; date=nothing)
    _, dates, μ = _summary_rows(datadir, "filtered_means")
    _, dv, v = _summary_rows(datadir, "filtered_variances")
    _, dp, p = _summary_rows(datadir, "filtered_state_probs")
    d = date === nothing ? maximum(dates) : string(date)
    m, vr, pr = μ[findfirst(==(d), dates), :], v[findfirst(==(d), dv), :], p[findfirst(==(d), dp), :]
    pr = pr ./ sum(pr)
    mean = sum(pr .* m)
    e = m .- mean
    var = sum(pr .* (e .^ 2 .+ vr))
    return d, mean, sqrt(var), sum(pr .* e .* (e .^ 2 .+ 3 .* vr)) / (var * sqrt(var))
end

"""
    altforecasts(datadir; horizon=12) -> (dates, forecast_post, forecast_proper)

code/alt_forecasts.jl:23-38: per summary row the plug-in forecast dot(π' * A^12, μ), A = reshape(row, K, K) (column-major,
whatever the header calls the columns), beside the `forecast_12_mean` column of forecasts_summary.csv.
"""
function altforecasts(datadir; horizon::Integer=12)
    _, dates, μ = _summary_rows(datadir, "filtered_means")
    _, _, π = _summary_rows(datadir, "filtered_state_probs")
    _, _, tr = _summary_rows(datadir, "filtered_trans_probs")
    hf, _, fc = _summary_rows(datadir, "forecasts")
    K = size(μ, 2)
    post = map(1:size(μ, 1)) do i
        A = reshape(tr[i, :], K, K)
        w = π[i, :]'
        for _ in 1:horizon
            w = w * A
        end
        sum(w' .* μ[i, :])
    end
    return dates, post, fc[:, findfirst(==("forecast_$(horizon)_mean"), hf) - 1]
end

"""
    write_forecast_comparison(path, dates, forecast_post, forecast_proper)

alt_forecasts.jl:28,39: `date,forecast_post,forecast_proper`, float text as in the other files.
"""
function write_forecast_comparison(path, dates, forecast_post, forecast_proper)
    open(path, "w") do io
        println(io, "date,forecast_post,forecast_proper")
        for (d, a, b) in zip(dates, forecast_post, forecast_proper)
            println(io, d, ",", _fmt(Float64(a)), ",", _fmt(Float64(b)))
        end
    end
    return path
end

function _signal_call(opt::estopt, burnin, nrun, n_samples, σsignal, κ, α, ν, devh::Vector{Int}, blend::Integer, endpos; device::Integer=0)
    Y = makey(opt); T = Int32[length(Y)]; K = opt.D; H = length(opt.horizons); nd = n_samples * nrun
    hz = ntuple(i -> i <= H ? Int32(devh[i]) : Int32(0), HMCG_MAXH)
    cfg = Ref(hmcg_config(Int32(sizeof(hmcg_config)), 1, K, length(Y), length(Y), burnin, nrun, H, hz, UInt64(opt.seed),
                          UInt32(0), Int32(device), Int32(0), Int32(0), Int32(0), Int32(0), Float64(α), Float64(ν), Float64(κ),
                          Int32(n_samples), Int32(blend), Int32(0), Int32(0)))
    sig = Int32[first(opt.signalRange) - 1, last(opt.signalRange)]                 # 0-based [begin, end)
    nsave = length(opt.signalSave)
    sv = nsave > 0 ? Int32[first(opt.signalSave) - 1, last(opt.signalSave)] : Int32[0, 0]
    ssig = Float64[σsignal]
    sigvals = zeros(Float64, max(nsave, 1), n_samples)                             # C: [n_samples][nsave_ld]
    ep = Int32[endpos]
    yreal = _yreal(opt)
    μ = Array{Float64}(undef, nd, K); σ = similar(μ); πe = similar(μ)
    A = Array{Float64}(undef, nd, K, K); fc = Array{Float64}(undef, nd, 2H); st = zeros(Int32, 1)
    rc = GC.@preserve Y T yreal μ σ A πe fc st sig sv ssig sigvals ep begin
        ex = Ref(hmcg_extras(Int32(sizeof(hmcg_extras)), Int32(0), C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL,
                             pointer(sig), pointer(sv), pointer(ssig), pointer(sigvals), Int32(max(nsave, 1)), Int32(0),
                             endpos >= 0 ? pointer(ep) : Ptr{Int32}(C_NULL), C_NULL, C_NULL, C_NULL, C_NULL, C_NULL))
        ccall((:hmcg_estimate_batch, LIBHMCG), Cint,
              (Ref{hmcg_config}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
               Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ref{hmcg_extras}, Ptr{Cvoid}),
              cfg, Y, T, H > 0 ? pointer(yreal) : Ptr{Float64}(C_NULL), μ, σ, A, πe, fc, C_NULL, st, ex, C_NULL)
    end
    rc == 0 || error("libhmcgibbs rc=$rc: $(last_error())")
    return μ, σ, πe, A, fc, sigvals
end

"""
    estimatesignals!(opt) -> (μ, σ, πb, A, forecasts, obsdates, signalvals, signalids)      (src/Hmc.jl:868-914)

Sets `opt.σsignal` from a base run when it is 0 (`:869-872`; upstream runs that one with HyperParams(Y, D): κ = 1,
α = ν = 1).  `πb` is (Ndraws, D) as upstream (`:900`).  Noise comes from the library's counter-based RNG.
"""
function estimatesignals!(opt::estopt; device::Integer=0)
    _check_live(opt; signals=true)
    isempty(opt.signalRange) && error("estimatesignals! needs a signalRange")
    H = length(opt.horizons)
    if isapprox(opt.σsignal, 0)
        _, σb, _, _, _, _ = _signal_call(opt, opt.burnin, opt.Nrun, 1, 0.0, 1.0, 1.0, 1.0, collect(Int, opt.horizons), 0, -1; device=device)
        opt.σsignal = sum(σb) / length(σb) * opt.noise
    end
    sigLen = last(opt.signalRange) - opt.endIndex                                   # :888
    devh = [h > sigLen ? h - sigLen : 0 for h in opt.horizons]                     # :907
    blend = sigLen > 0 ? sum(Int[(1 << (k - 1)) for (k, h) in enumerate(opt.horizons) if h == sigLen]) : 0
    μ, σ, πe, A, fc, sigvals = _signal_call(opt, opt.signalburnin, opt.signalNrun, opt.noiseSamples, opt.σsignal, opt.noise,
                                            2.0, 2.0, devh, blend, sigLen > 0 ? opt.endIndex - 1 : -1; device=device)
    for (k, h) in enumerate(opt.horizons)
        h < sigLen && (fc[:, 2k-1:2k] .= NaN)                                       # never assigned upstream (:906-910)
    end
    n = opt.signalNrun; nd = n * opt.noiseSamples
    nsave = length(opt.signalSave)
    signalvals = Array{Float64}(undef, nd, nsave)
    signalids = Array{Int64}(undef, nd)
    for s in 1:opt.noiseSamples
        r = n*(s-1)+1:n*s
        signalids[r] .= s                                                            # :903
        for j in 1:nsave
            signalvals[r, j] .= sigvals[j, s]                                        # :904
        end
    end
    return (μ = μ, σ = σ, πb = πe, A = A, forecasts = fc, obsdates = fill(enddate(opt), nd),
            signalvals = signalvals, signalids = signalids)
end

# ---- CSV output (layout of src/Hmc.jl:707-748) ---------------------------------------------
# CSV.jl 0.5.16 float text (shortest round-trip digits; integral values without a fraction; |x| < 1e-4 as
# <integer mantissa>e-<n>, e.g. 24e-11), produced by the library so that every host language prints the same bytes
function _fmt(x::Float64)
    buf = Vector{UInt8}(undef, 48)
    n = ccall((:hmcg_format_float, LIBHMCG), Cint, (Float64, Ptr{UInt8}), x, buf)
    return String(buf[1:n])
end

# The five per-window files of saveresults (:741-746) for draw arrays in Julia layout, through the library's writer
# (hmcg_save_results_csv).  μ, σ, πe: (n, K); A: (n, K, K); fc: (n, 2H); sigvals: (nsave, noiseSamples) or nothing.
function _save_native(dir, date, K, horizons, μ, σ, πe, A, fc; sigvals=nothing)
    mkpath(dir)
    H = length(horizons); n = size(μ, 1)
    hz = Vector{Int32}(horizons)
    dates = [string(date)]
    sv = sigvals === nothing ? Ptr{Float64}(C_NULL) : pointer(sigvals)
    nsmp = sigvals === nothing ? 0 : size(sigvals, 2); nsave = sigvals === nothing ? 0 : size(sigvals, 1)
    rc = GC.@preserve μ σ πe A fc hz dates sigvals begin
        ccall((:hmcg_save_results_csv, LIBHMCG), Cint,
              (Cstring, Int32, Ptr{Cstring}, Int32, Int32, Ptr{Int32}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
               Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Int32, Int32, Int32),
              dir, Int32(1), dates, Int32(K), Int32(H), hz, Int64(n), μ, σ, πe, A, H > 0 ? pointer(fc) : Ptr{Float64}(C_NULL),
              sv, Int32(nsmp), Int32(nsave), Int32(nsave), Int32(0), Int32(1))
    end
    rc == 0 || error("hmcg_save_results_csv rc=$rc (directory $dir)")
end

function basicsave(data, dates, fname, dataheader; precision=5, signal=Array{Float64}(undef, 0, 0), signalids=Int64[])
    hassig = size(signal, 2) > 0
    header = vcat(["date"], String.(dataheader))
    hassig && append!(header, ["signal_$i" for i in 1:size(signal, 2)])
    !isempty(signalids) && insert!(header, 2, "signalid")                          # :717
    open(fname, "w") do io
        println(io, join(header, ","))
        for i in 1:size(data, 1)
            cells = [string(dates[i])]
            hassig && push!(cells, string(signalids[i]))                           # only together with signals (:715-717)
            append!(cells, [_fmt(round(Float64(v); digits=precision)) for v in data[i, :]])
            hassig && append!(cells, [_fmt(round(Float64(v); digits=5)) for v in signal[i, :]])
            println(io, join(cells, ","))
        end
    end
end

function _savesignalresults(samples, opt, dir)
    h1 = ["state_$i" for i in 1:opt.D]
    h2 = vec(["trans_$(i)_$(j)" for i in 1:opt.D, j in 1:opt.D])
    h3 = String[]
    for h in opt.horizons
        push!(h3, "forecast_$h"); push!(h3, "forecast_error_$h")
    end
    mkpath(dir)
    kw = (signal = samples.signalvals, signalids = samples.signalids)
    n = size(samples.μ, 1)
    basicsave(samples.μ, samples.obsdates, joinpath(dir, "filtered_means_$(enddate(opt)).csv"), h1; kw...)
    basicsave(samples.σ, samples.obsdates, joinpath(dir, "filtered_variances_$(enddate(opt)).csv"), h1; kw...)
    basicsave(samples.πb, samples.obsdates, joinpath(dir, "filtered_state_probs_$(enddate(opt)).csv"), h1; kw...)
    basicsave(reshape(samples.A, n, :), samples.obsdates, joinpath(dir, "filtered_trans_probs_$(enddate(opt)).csv"), h2; kw...)
    basicsave(samples.forecasts, samples.obsdates, joinpath(dir, "forecasts_$(enddate(opt)).csv"), h3; kw...)
end

function saveresults(samples, opt, dir; hassignals=false)
    hassignals && return _savesignalresults(samples, opt, dir)                     # :735-739 (writes under `dir`)
    odir = "data/output/$(opt.series)/"          # the reference ignores `dir` here (src/Hmc.jl:741)
    _save_native(odir, enddate(opt), opt.D, opt.horizons, samples.μ, samples.σ, samples.πb[:, end, :], samples.A,
                 samples.forecasts)
end

end # module
