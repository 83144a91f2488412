// nmpc_wave.h — arithmetic and wave-level primitives every solve kernel uses, swarm (through nmpc_solve_common.h) and LIDAR alike: the
// v_rcp_f64 reciprocals, the fast division, the mantissa / exponent accumulator of sum log, wave-uniform values and the reductions over the
// wavefronts of an instance.  It knows nothing of a kernel's parameter block.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace nmpc {

// reciprocal: v_rcp_f64 seed + ONE Newton step (seed error e0 = 4.2e-8 measured; after the step <= e0^2 + 2u = 2.0e-15, 1.9e-15 measured: docs/WAVE_PRIMITIVES.md) ...
__device__ __forceinline__ double rcp1(double d)
{
    double r = __builtin_amdgcn_rcp(d);
    return fma(fma(-d, r, 1.0), r, r);
}
// ... + TWO Newton steps: full fp64 accuracy, five dependent operations where the IEEE division chain has eleven (the LIDAR kernel's pivots:
// the Riccati stage of a lone wavefront is one long dependency chain with two pivots in it; the swarm kernels' pivots take rcp_nr of
// nmpc_solve_common.h, one step by default)
__device__ __forceinline__ double rcp2(double d)
{
    double r = rcp1(d);
    return fma(fma(-d, r, 1.0), r, r);
}
// Divisions of the stage-parallel phases (sigma = z / s, mu / s, dz, the step-length quotients): NMPC_FAST_DIV = 1 replaces the IEEE division
// chain (~12 instructions: div_scale x2, rcp, four multiply-adds, div_fmas, div_fixup) by rcp1 and a multiply (4): relative error <= 2.1e-15
// (e0^2 + 3u; 2.0e-15 measured, tests/probes/wave_probe.hip), NaN at a denominator 0, +-inf or below 2^-1024 where the division gives +-inf, +-0
// or a finite value (docs/WAVE_PRIMITIVES.md).  Every site of one quantity goes through the same helper, so the sites stay consistent with each other.  NMPC_FAST_DIV = 0 restores the divisions (A/B; the LIDAR source sets it from its own switch NMPC_LIDAR_FAST_DIV).
// A/B in one session (round 4): six robots B=4096 262 k -> 280 k solves/s, B=16384 388 k -> 410 k, a lone wave +10 %, mean iterations 29.0735 -> 29.0720.
#ifndef NMPC_FAST_DIV
#define NMPC_FAST_DIV 1
#endif
__device__ __forceinline__ double qdiv(double a, double b)
{
#if NMPC_FAST_DIV
    return a * rcp1(b);
#else
    return a / b;
#endif
}

// A value every lane of the wave holds identically (a finished reduction, an LDS word read at a wave-uniform address),
// moved through v_readfirstlane: the compiler then KNOWS it is wave-uniform, so the branches that depend on it (line-search
// acceptance, convergence, pivot failure, barrier update) become scalar branches instead of exec-masked divergent regions.
__device__ __forceinline__ double uniform_f64(double v)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// Sum of log(s_i), s_i > 0, accumulated as (product of the mantissas, sum of the exponents): four instructions per term instead of a
// logarithm (~90), one logarithm per wavefront at the end.  The mantissa product is renormalised after every term (no underflow however
// many terms); a term <= 0 or NaN makes the result NaN, as the logarithm would.
struct LogSum {
    double m = 1.0, lo = INFINITY;
    int e = 0;
    __device__ __forceinline__ void add(double s_)
    {
        const double t = m * __builtin_amdgcn_frexp_mant(s_);
        e += __builtin_amdgcn_frexp_exp(s_) + __builtin_amdgcn_frexp_exp(t);
        m = __builtin_amdgcn_frexp_mant(t);
        lo = fmin(lo, s_);
    }
};

// ---- reductions over the TPB threads of one instance — one, two or four wavefronts; red: [TPB / 64] doubles of LDS, unused for one — with a
// result the compiler knows to be wave-uniform
template <int TPB = 64> __device__ __forceinline__ double wsum(double v, double *red = nullptr)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if constexpr (TPB > 64) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        double t = 0.0;
        for (int w = 0; w < TPB / 64; w++) t += red[w];
        v = t;
    }
    return uniform_f64(v);
}
template <int TPB = 64> __device__ __forceinline__ double wmax(double v, double *red = nullptr)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    if constexpr (TPB > 64) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        double t = red[0];
        for (int w = 1; w < TPB / 64; w++) t = fmax(t, red[w]);
        v = t;
    }
    return uniform_f64(v);
}
template <int TPB = 64> __device__ __forceinline__ double wmin(double v, double *red = nullptr) { return -wmax<TPB>(-v, red); }
template <int TPB = 64> __device__ __forceinline__ double wlogsum(LogSum a, double *red = nullptr)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double t = a.m * __shfl_xor(a.m, o);
        a.e += __shfl_xor(a.e, o) + __builtin_amdgcn_frexp_exp(t);
        a.m = __builtin_amdgcn_frexp_mant(t);
        a.lo = fmin(a.lo, __shfl_xor(a.lo, o));
    }
    double v = (a.lo > 0.0) ? fma((double)a.e, 0.693147180559945309417, log(a.m)) : NAN;
    if constexpr (TPB > 64) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        double t = 0.0;
        for (int w = 0; w < TPB / 64; w++) t += red[w];
        v = t;
    }
    return uniform_f64(v);
}
// wmin<64> and wlogsum<64> in the form the LIDAR kernel was written with: the same values, another instruction sequence (a minimum in place of
// the negated maximum; the logarithm taken before the test of the smallest term, not under it).  That kernel keeps the forms it was tuned
// with, as the swarm kernels keep theirs in the templates above: either side's generated code moves with the other's form (docs/MEMORY_LAYOUT.md).
__device__ __forceinline__ double wave_min(double v) { for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o)); return uniform_f64(v); }
__device__ __forceinline__ double wave_logsum(LogSum a)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double t = a.m * __shfl_xor(a.m, o);
        a.e += __shfl_xor(a.e, o) + __builtin_amdgcn_frexp_exp(t);
        a.m = __builtin_amdgcn_frexp_mant(t);
        a.lo = fmin(a.lo, __shfl_xor(a.lo, o));
    }
    const double r = fma((double)a.e, 0.693147180559945309417, log(a.m));
    return uniform_f64((a.lo > 0.0) ? r : NAN);
}

}  // namespace nmpc
