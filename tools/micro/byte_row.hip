// What does the byte row of lf_snow_frost_members_device (isFrozenSoil: one byte per pixel beside 13 double rows) cost, and is
// it cheaper written four pixels per lane (one dword store per lane, the double rows as 32-byte accesses) than one pixel per
// lane (one byte store per lane: 64 B per wavefront, the one store of the kernel narrower than a line)?  The traffic of the
// kernel without its arithmetic: 6 double rows read, 7 double rows and the byte row written, n elements each.
//   one      : one pixel per lane, as the kernel has it
//   one_nob  : the same without the byte row
//   four     : four pixels per lane, double4 loads and stores, uchar4 store (n a multiple of 4, rows 32-byte aligned)
//   four_nob : the same without the byte row
// Alternating, median of `reps` launches each, bytes over time against each other.
//   hipcc -O3 --offload-arch=gfx950 -o byte_row byte_row.hip && ./byte_row
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>
constexpr int IN = 6, OUT = 7, LANES = 256;
struct rows {
    const double *in[IN];
    double *out[OUT];
    unsigned char *flag;
};
template <bool BYTE>
__global__ void __launch_bounds__(LANES) k_one(rows R, long long n)
{
    const long long i = (long long)blockIdx.x * LANES + threadIdx.x;
    if (i >= n) return;
    double x[IN];
#pragma unroll
    for (int k = 0; k < IN; ++k) x[k] = __builtin_nontemporal_load(R.in[k] + i);
    double s = x[0];
#pragma unroll
    for (int k = 0; k < OUT; ++k) {
        s = s + x[(k + 1) % IN];
        R.out[k][i] = s;
    }
    if (BYTE) R.flag[i] = s > 3.0 ? 1 : 0;
}
template <bool BYTE>
__global__ void __launch_bounds__(LANES) k_four(rows R, long long n)
{
    const long long i = ((long long)blockIdx.x * LANES + threadIdx.x) * 4;
    if (i >= n) return;
    double4 x[IN];
#pragma unroll
    for (int k = 0; k < IN; ++k) x[k] = *(const double4 *)(R.in[k] + i);
    double4 s = x[0];
#pragma unroll
    for (int k = 0; k < OUT; ++k) {
        const double4 y = x[(k + 1) % IN];
        s.x = s.x + y.x; s.y = s.y + y.y; s.z = s.z + y.z; s.w = s.w + y.w;
        *(double4 *)(R.out[k] + i) = s;
    }
    if (BYTE) *(uchar4 *)(R.flag + i) = make_uchar4(s.x > 3.0, s.y > 3.0, s.z > 3.0, s.w > 3.0);
}
int main()
{
    const long long n = 64000000; // 16 members of 2000^2 pixels
    const int reps = 11;
    rows R;
    std::vector<double> host(n);
    for (long long i = 0; i < n; ++i) host[i] = (double)(i % 7) * 0.25;
    for (int k = 0; k < IN; ++k) {
        hipMalloc((void **)&R.in[k], n * sizeof(double));
        hipMemcpy((void *)R.in[k], host.data(), n * sizeof(double), hipMemcpyHostToDevice);
    }
    for (int k = 0; k < OUT; ++k) hipMalloc((void **)&R.out[k], n * sizeof(double));
    hipMalloc((void **)&R.flag, n);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    const char *name[4] = {"one", "one_nob", "four", "four_nob"};
    std::vector<float> ms[4];
    const unsigned g1 = (unsigned)((n + LANES - 1) / LANES), g4 = (unsigned)((n / 4 + LANES - 1) / LANES);
    for (int rep = 0; rep <= reps; ++rep)
        for (int v = 0; v < 4; ++v) {
            hipEventRecord(e0);
            if (v == 0) hipLaunchKernelGGL(k_one<true>, dim3(g1), dim3(LANES), 0, 0, R, n);
            if (v == 1) hipLaunchKernelGGL(k_one<false>, dim3(g1), dim3(LANES), 0, 0, R, n);
            if (v == 2) hipLaunchKernelGGL(k_four<true>, dim3(g4), dim3(LANES), 0, 0, R, n);
            if (v == 3) hipLaunchKernelGGL(k_four<false>, dim3(g4), dim3(LANES), 0, 0, R, n);
            hipEventRecord(e1);
            if (hipEventSynchronize(e1) != hipSuccess) {
                printf("launch failed: %s\n", hipGetErrorString(hipGetLastError()));
                return 1;
            }
            float t;
            hipEventElapsedTime(&t, e0, e1);
            if (rep) ms[v].push_back(t); // (the first round warms up)
        }
    for (int v = 0; v < 4; ++v) {
        std::sort(ms[v].begin(), ms[v].end());
        const double bytes = (double)n * ((IN + OUT) * 8 + (v % 2 == 0 ? 1 : 0));
        const float med = ms[v][ms[v].size() / 2];
        printf("%-9s median %.3f ms (min %.3f, max %.3f)  %.2f TB/s\n", name[v], med, ms[v].front(), ms[v].back(), bytes / (med * 1e-3) / 1e12);
    }
    return 0;
}
