// lf_math_probe.hip -- the device math helpers of the product, one value per lane, for tests/test_device_math_gpu.py.
//
// Built by the tests (tests/probes/probe_build.py) with the CXXFLAGS of lisflood-code_amd/Makefile, so every helper inlined
// here computes the bits it computes inside the product's kernels.  One element-wise kernel per family of helpers, the
// form picked by `variant`; the lockstep forms (N arguments side by side) take the value under test in lane slot `slot`
// and neighbouring values of the input in the other slots, so a test that calls every slot sends every value through
// every slot.  Each host entry point copies in, launches once, synchronises, copies back and returns the HIP error code.
#include <hip/hip_runtime.h>

#include "lf_math.h"
#include "lf_sweep.h"
#include "lf_fused.h"
#include "lf_soil_math.h"

namespace {

constexpr int kProbeBlock = 256;

// the value of slot j for lane i when lane i's own value sits in slot `slot` (i + j - slot, modulo n)
__device__ __forceinline__ long long rot(long long i, int j, int slot, long long n)
{
    return ((i + j - slot) % n + n) % n;
}

// fused_args as the router sets it up for its beta (lf_fused.h: F.beta, F.inv_beta, F.b_minus_1 from the router's
// beta, 1 / beta, beta - 1)
fused_args probe_fused_args(double beta)
{
    fused_args F;
    std::memset(&F, 0, sizeof F);
    F.beta = beta;
    F.inv_beta = 1 / beta;
    F.b_minus_1 = beta - 1;
    F.solve35 = beta == 0.6 ? 1 : 0;
    return F;
}

// x^0.6 (fam 0) and x^(1/0.6) (fam 1)
//   0 lf_pow_3_5 / lf_pow_5_3      1..4 lf_pow_3_5_n<variant> (fam 0 only)      5 lf_pow_3_5_hot (fam 0 only)
//   6 cone_pow_*<true>             7 cone_pow_*<false> with is35                8 cone_pow_*_two<true>
//   9 cone_pow_*_two<false>        10 OCML pow
__global__ void k_pow_beta(int fam, int variant, int slot, long long n, const double *__restrict__ x, double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * kProbeBlock + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    const double e = fam == 0 ? 0.6 : 1.0 / 0.6;
    double r = 0.0;
    if (variant == 0) {
        r = fam == 0 ? lf_pow_3_5(v) : lf_pow_5_3(v);
    } else if (variant >= 1 && variant <= 4 && fam == 0) {
        double xs[4], ys[4];
        for (int j = 0; j < 4; ++j) xs[j] = x[rot(i, j, slot, n)];
        if (variant == 1) {
            const double a[1] = {xs[0]};
            double b[1];
            lf_pow_3_5_n<1>(a, b);
            ys[0] = b[0];
        } else if (variant == 2) {
            const double a[2] = {xs[0], xs[1]};
            double b[2];
            lf_pow_3_5_n<2>(a, b);
            ys[0] = b[0], ys[1] = b[1];
        } else if (variant == 3) {
            const double a[3] = {xs[0], xs[1], xs[2]};
            double b[3];
            lf_pow_3_5_n<3>(a, b);
            ys[0] = b[0], ys[1] = b[1], ys[2] = b[2];
        } else {
            const double a[4] = {xs[0], xs[1], xs[2], xs[3]};
            double b[4];
            lf_pow_3_5_n<4>(a, b);
            ys[0] = b[0], ys[1] = b[1], ys[2] = b[2], ys[3] = b[3];
        }
        r = ys[slot];
    } else if (variant == 5 && fam == 0) {
        r = lf_pow_3_5_hot(v);
    } else if (variant == 6) {
        r = fam == 0 ? cone_pow_3_5<true>(v, e, true) : cone_pow_5_3<true>(v, e, true);
    } else if (variant == 7) {
        r = fam == 0 ? cone_pow_3_5<false>(v, e, true) : cone_pow_5_3<false>(v, e, true);
    } else if (variant == 8 || variant == 9) {
        const double x1 = x[rot(i, 0, slot, n)], x2 = x[rot(i, 1, slot, n)];
        double y1, y2;
        if (variant == 8) {
            if (fam == 0) cone_pow_3_5_two<true>(x1, x2, y1, y2);
            else cone_pow_5_3_two<true>(x1, x2, y1, y2);
        } else {
            if (fam == 0) cone_pow_3_5_two<false>(x1, x2, y1, y2);
            else cone_pow_5_3_two<false>(x1, x2, y1, y2);
        }
        r = slot == 0 ? y1 : y2;
    } else if (variant == 10) {
        r = pow(v, e);
    } else {
        r = __builtin_nan("");
    }
    out[i] = r;
}

// root Q of Q + a Q^beta = c
//   0 lf_solve_3_5      1 lf_solve_3_5_pre (af, laf made as the cone kernel makes them)      2 solve_any(b35)
//   3 cone_solve<true>  4 cone_solve<false> with is35      5 cone_solve_two<true>      6 cone_solve_two<false>
//   7 lf_solve_cell     8 lf_solve_cell_cold
// (fused_args with `beta`; variants 0-6 are the beta = 3/5 forms)
__global__ void k_solve(int variant, int slot, long long n, const double *__restrict__ c, const double *__restrict__ a,
                        fused_args F, double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * kProbeBlock + threadIdx.x;
    if (i >= n) return;
    const double cv = c[i], av = a[i];
    double r = 0.0;
    if (variant == 0) {
        r = lf_solve_3_5(cv, av);
    } else if (variant == 1) {
        const float af = (float)av;
        const float laf = __builtin_amdgcn_logf(af);
        r = lf_solve_3_5_pre(cv, av, af, laf);
    } else if (variant == 2) {
        r = solve_any(cv, av, true, F);
    } else if (variant == 3) {
        r = cone_solve<true>(cv, av, true, F);
    } else if (variant == 4) {
        r = cone_solve<false>(cv, av, true, F);
    } else if (variant == 5 || variant == 6) {
        const long long i1 = rot(i, 0, slot, n), i2 = rot(i, 1, slot, n);
        double q1, q2;
        if (variant == 5) cone_solve_two<true>(c[i1], a[i1], c[i2], a[i2], F, q1, q2);
        else cone_solve_two<false>(c[i1], a[i1], c[i2], a[i2], F, q1, q2);
        r = slot == 0 ? q1 : q2;
    } else if (variant == 7) {
        r = lf_solve_cell(cv, av, F.beta * av, F.beta, F.inv_beta, F.b_minus_1);
    } else if (variant == 8) {
        r = lf_solve_cell_cold(cv, av, F.beta * av, F.beta, F.inv_beta, F.b_minus_1);
    } else {
        r = __builtin_nan("");
    }
    out[i] = r;
}

// x^y
//   0 lf_pow_pos      1..3 lf_pow_pos_n<variant>      4 powxy<true>      5 lf_pow_scalar_exponent      6 OCML pow
//   7 powxy<false>
__global__ void k_pow_pos(int variant, int slot, long long n, const double *__restrict__ x, const double *__restrict__ y,
                          double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * kProbeBlock + threadIdx.x;
    if (i >= n) return;
    const double xv = x[i], yv = y[i];
    double r = 0.0;
    if (variant == 0) {
        r = lf_pow_pos(xv, yv);
    } else if (variant >= 1 && variant <= 3) {
        double xs[3], ys[3], os[3];
        for (int j = 0; j < 3; ++j) {
            const long long k = rot(i, j, slot, n);
            xs[j] = x[k];
            ys[j] = y[k];
        }
        if (variant == 1) {
            const double a[1] = {xs[0]}, b[1] = {ys[0]};
            double o[1];
            lf_pow_pos_n<1>(a, b, o);
            os[0] = o[0];
        } else if (variant == 2) {
            const double a[2] = {xs[0], xs[1]}, b[2] = {ys[0], ys[1]};
            double o[2];
            lf_pow_pos_n<2>(a, b, o);
            os[0] = o[0], os[1] = o[1];
        } else {
            lf_pow_pos_n<3>(xs, ys, os);
        }
        r = os[slot];
    } else if (variant == 4) {
        r = powxy<true>(xv, yv);
    } else if (variant == 5) {
        r = lf_pow_scalar_exponent(xv, yv);
    } else if (variant == 6) {
        r = pow(xv, yv);
    } else if (variant == 7) {
        r = powxy<false>(xv, yv);
    } else {
        r = __builtin_nan("");
    }
    out[i] = r;
}

// unsaturated conductivity of one layer
//   0 unsat_k<true>      1 unsat_k<false>
//   2 unsat_k_r<true> as the sub-step loop calls it (soil_den_of once per column)      3 the same <false>
//   4 unsat_k3<true> (the value under test in layer `slot`)      5 unsat_k3<false>
__global__ void k_unsat_k(int variant, int slot, long long n, const double *__restrict__ w, const unsigned char *__restrict__ pore,
                          const double *__restrict__ wres, const double *__restrict__ ws, const double *__restrict__ ksat,
                          const double *__restrict__ inv_m, const double *__restrict__ m, double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * kProbeBlock + threadIdx.x;
    if (i >= n) return;
    const bool p = pore[i] != 0;
    double r = 0.0;
    if (variant == 0) {
        r = unsat_k<true>(w[i], p, wres[i], ws[i], ksat[i], inv_m[i], m[i]);
    } else if (variant == 1) {
        r = unsat_k<false>(w[i], p, wres[i], ws[i], ksat[i], inv_m[i], m[i]);
    } else if (variant == 2 || variant == 3) {
        const soil_den D = soil_den_of(ws[i], wres[i]);
        r = variant == 2 ? unsat_k_r<true>(w[i], p, wres[i], D, ksat[i], inv_m[i], m[i])
                         : unsat_k_r<false>(w[i], p, wres[i], D, ksat[i], inv_m[i], m[i]);
    } else if (variant == 4 || variant == 5) {
        double w3[3], wres3[3], ws3[3], ks3[3], im3[3], m3[3], k3[3];
        bool p3[3];
        for (int l = 0; l < 3; ++l) {
            const long long k = rot(i, l, slot, n);
            w3[l] = w[k], p3[l] = pore[k] != 0, wres3[l] = wres[k], ws3[l] = ws[k];
            ks3[l] = ksat[k], im3[l] = inv_m[k], m3[l] = m[k];
        }
        if (variant == 4) unsat_k3<true>(w3, p3, wres3, ws3, ks3, im3, m3, k3);
        else unsat_k3<false>(w3, p3, wres3, ws3, ks3, im3, m3, k3);
        r = k3[slot];
    } else {
        r = __builtin_nan("");
    }
    out[i] = r;
}

// device buffers of one call, freed on every path
struct probe_bufs {
    void *p[9] = {};
    int k = 0;
    hipError_t put(const void *host, size_t bytes, void **dev)
    {
        hipError_t e = hipMalloc(dev, bytes ? bytes : 1);
        if (e != hipSuccess) return e;
        p[k++] = *dev;
        return host ? hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice) : hipSuccess;
    }
    ~probe_bufs()
    {
        for (int j = 0; j < k; ++j) (void)hipFree(p[j]);
    }
};

#define PROBE_TRY(x)                                                                                                   \
    do {                                                                                                               \
        const hipError_t e_ = (x);                                                                                     \
        if (e_ != hipSuccess) return (int)e_;                                                                          \
    } while (0)

inline unsigned int probe_grid(long long n) { return (unsigned int)((n + kProbeBlock - 1) / kProbeBlock); }

} // namespace

extern "C" {

int probe_pow_beta(int fam, int variant, int slot, long long n, const double *x, double *out)
{
    if (n <= 0) return 0;
    probe_bufs B;
    double *dx, *dout;
    PROBE_TRY(B.put(x, n * sizeof(double), (void **)&dx));
    PROBE_TRY(B.put(nullptr, n * sizeof(double), (void **)&dout));
    hipLaunchKernelGGL(k_pow_beta, dim3(probe_grid(n)), dim3(kProbeBlock), 0, 0, fam, variant, slot, n, dx, dout);
    PROBE_TRY(hipGetLastError());
    PROBE_TRY(hipDeviceSynchronize());
    PROBE_TRY(hipMemcpy(out, dout, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int probe_solve(int variant, int slot, double beta, long long n, const double *c, const double *a, double *out)
{
    if (n <= 0) return 0;
    probe_bufs B;
    double *dc, *da, *dout;
    PROBE_TRY(B.put(c, n * sizeof(double), (void **)&dc));
    PROBE_TRY(B.put(a, n * sizeof(double), (void **)&da));
    PROBE_TRY(B.put(nullptr, n * sizeof(double), (void **)&dout));
    hipLaunchKernelGGL(k_solve, dim3(probe_grid(n)), dim3(kProbeBlock), 0, 0, variant, slot, n, dc, da,
                       probe_fused_args(beta), dout);
    PROBE_TRY(hipGetLastError());
    PROBE_TRY(hipDeviceSynchronize());
    PROBE_TRY(hipMemcpy(out, dout, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int probe_pow_pos(int variant, int slot, long long n, const double *x, const double *y, double *out)
{
    if (n <= 0) return 0;
    probe_bufs B;
    double *dx, *dy, *dout;
    PROBE_TRY(B.put(x, n * sizeof(double), (void **)&dx));
    PROBE_TRY(B.put(y, n * sizeof(double), (void **)&dy));
    PROBE_TRY(B.put(nullptr, n * sizeof(double), (void **)&dout));
    hipLaunchKernelGGL(k_pow_pos, dim3(probe_grid(n)), dim3(kProbeBlock), 0, 0, variant, slot, n, dx, dy, dout);
    PROBE_TRY(hipGetLastError());
    PROBE_TRY(hipDeviceSynchronize());
    PROBE_TRY(hipMemcpy(out, dout, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int probe_unsat_k(int variant, int slot, long long n, const double *w, const unsigned char *pore, const double *wres,
                  const double *ws, const double *ksat, const double *inv_m, const double *m, double *out)
{
    if (n <= 0) return 0;
    probe_bufs B;
    double *dw, *dwres, *dws, *dks, *dim, *dm, *dout;
    unsigned char *dp;
    const size_t b = n * sizeof(double);
    PROBE_TRY(B.put(w, b, (void **)&dw));
    PROBE_TRY(B.put(pore, n, (void **)&dp));
    PROBE_TRY(B.put(wres, b, (void **)&dwres));
    PROBE_TRY(B.put(ws, b, (void **)&dws));
    PROBE_TRY(B.put(ksat, b, (void **)&dks));
    PROBE_TRY(B.put(inv_m, b, (void **)&dim));
    PROBE_TRY(B.put(m, b, (void **)&dm));
    PROBE_TRY(B.put(nullptr, b, (void **)&dout));
    hipLaunchKernelGGL(k_unsat_k, dim3(probe_grid(n)), dim3(kProbeBlock), 0, 0, variant, slot, n, dw, dp, dwres, dws, dks,
                       dim, dm, dout);
    PROBE_TRY(hipGetLastError());
    PROBE_TRY(hipDeviceSynchronize());
    PROBE_TRY(hipMemcpy(out, dout, b, hipMemcpyDeviceToHost));
    return 0;
}

} // extern "C"
