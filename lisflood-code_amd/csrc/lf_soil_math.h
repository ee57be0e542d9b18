// lf_soil_math.h -- per-layer arithmetic of the soil kernel (lf_soil.hip): builtins min / max, x^y and the
// unsaturated conductivity (soilloop.py:360-383).  In a header of its own so that tests/probes/lf_math_probe.hip runs
// exactly what the soil kernels run.
#pragma once
#include <hip/hip_runtime.h>

#include "lf_math.h"

namespace {

__device__ __forceinline__ double dmin(double a, double b) { return (b < a) ? b : a; } // builtins.min(a, b)
__device__ __forceinline__ double dmax(double a, double b) { return (b > a) ? b : a; } // builtins.max(a, b)

// saturationDegree (soilloop.py:378-383) + unsaturatedConductivity (360-367)
// x^y with x in [0, 1] and y > 0: lf_pow_pos (lf_math.h) or OCML pow (LF_GENERAL_POW=1)
template <bool FASTPOW>
__device__ __forceinline__ double powxy(double x, double y)
{
    return FASTPOW ? lf_pow_pos(x, y) : pow(x, y);
}

template <bool FASTPOW>
__device__ __forceinline__ double unsat_k(double w, bool pore, double wres, double ws, double ksat, double inv_m,
                                          double m)
{
    // evaluated for every lane and selected (a divergent branch here would split the sub-step loop into basic blocks
    // and serialise the three layers' dependent chains); without pore space the quotient is discarded
    const double sc = dmax(dmin((w - wres) / (ws - wres), 1.), 0.);
    const double s = pore ? sc : 0.;
    const double t = 1. - powxy<FASTPOW>(1. - powxy<FASTPOW>(s, inv_m), m);
    return ksat * sqrt(s) * (t * t);
}

// The same with the reciprocal of the layer's (ws - wres) worked out once per column instead of once per sub-step: the
// quotient below is the hardware's own division sequence (v_rcp_f64, two Newton steps on the reciprocal, product, one
// correction of the quotient) with the denominator's part hoisted out of the sub-step loop -- the same operations, so the
// same bits wherever the hardware sequence does not rescale its operands (it does for denormal or wildly different
// exponents only: water contents in mm are neither; (w - wres) == 0 gives 0 either way).  8 instructions fewer per
// sub-step, one of them a quarter-rate v_rcp_f64.
#ifndef LF_SOIL_HOISTED_RCP
#define LF_SOIL_HOISTED_RCP 1
#endif
__device__ __forceinline__ double soil_rcp_refined(double d)
{
    double r = __builtin_amdgcn_rcp(d);
    r = fma(r, fma(-d, r, 1.0), r);
    r = fma(r, fma(-d, r, 1.0), r);
    return r;
}
// What the sub-step loop (layer_loop) divides by, worked out once per column: q = fma(fma(-d, n r0, n), r1, n r0).
// With den != 0 and a finite reciprocal: d = den, r0 = r1 = the refined reciprocal (the sequence above).  Otherwise the
// IEEE quotient's value through the same two fmas: d = 0 and r0 = 0 make the inner fma n, r1 = 1 / den (IEEE) gives
// n * (+-inf) = n / (+-0) -- +-inf, NaN for n == 0 -- for ws == wres (ThetaS == ThetaR with the pore-space flag set, as
// the oracle and unsat_k divide), +-0 for den = +-inf and NaN for NaN.  (A denormal den, less than 2^-1022 mm of pore
// space, comes from no caller: it would take the same path and round twice.)
struct soil_den {
    double d, r0, r1;
};
__device__ __forceinline__ soil_den soil_den_of(double ws, double wres)
{
    const double den = ws - wres, rden = soil_rcp_refined(den);
    const bool hoist = den != 0.0 && __builtin_isfinite(rden);
    return {hoist ? den : 0.0, hoist ? rden : 0.0, hoist ? rden : 1.0 / den};
}
template <bool FASTPOW>
__device__ __forceinline__ double unsat_k_r(double w, bool pore, double wres, const soil_den &D, double ksat, double inv_m,
                                            double m)
{
    const double n = w - wres;
    const double q0 = n * D.r0;
    const double q = fma(fma(-D.d, q0, n), D.r1, q0); // n / d
    const double sc = dmax(dmin(q, 1.), 0.);
    const double s = pore ? sc : 0.;
    const double t = 1. - powxy<FASTPOW>(1. - powxy<FASTPOW>(s, inv_m), m);
    return ksat * sqrt(s) * (t * t);
}

// the three layers of a column at once (lf_pow_pos_n: the dependent chains of the layers interleaved)
template <bool FASTPOW>
__device__ __forceinline__ void unsat_k3(const double (&w)[3], const bool (&pore)[3], const double (&wres)[3],
                                         const double (&ws)[3], const double (&ksat)[3], const double (&inv_m)[3],
                                         const double (&m)[3], double (&k)[3])
{
    if (!FASTPOW) {
#pragma unroll
        for (int l = 0; l < 3; ++l) k[l] = unsat_k<false>(w[l], pore[l], wres[l], ws[l], ksat[l], inv_m[l], m[l]);
        return;
    }
    double s[3], a[3], b[3], t[3];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const double sc = dmax(dmin((w[l] - wres[l]) / (ws[l] - wres[l]), 1.), 0.);
        s[l] = pore[l] ? sc : 0.;
    }
    lf_pow_pos_n<3>(s, inv_m, a);
#pragma unroll
    for (int l = 0; l < 3; ++l) a[l] = 1. - a[l];
    lf_pow_pos_n<3>(a, m, b);
#pragma unroll
    for (int l = 0; l < 3; ++l) t[l] = 1. - b[l];
#pragma unroll
    for (int l = 0; l < 3; ++l) k[l] = ksat[l] * sqrt(s[l]) * (t[l] * t[l]);
}

} // namespace
