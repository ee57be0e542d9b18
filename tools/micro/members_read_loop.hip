// What limits the read loop of k_members_summary (lf_members.hip) at 51 member rows of 4e6 doubles?  One lane per element, the
// sum and the two folds in member order, three outputs: rows in flight (4 / 8 / 16), a pad on the row stride, stores in place
// against stores through a permutation, plain against non-temporal row loads, one block per 256 elements against a grid-stride
// loop.  Prints ms and TB/s of member rows read.  hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 members_read_loop.hip -o members_read_loop
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <numeric>
#include <algorithm>
#include <random>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__device__ __forceinline__ double npmin(double a, double b) { return (a != a) ? a : ((b != b) ? b : (b < a ? b : a)); }
__device__ __forceinline__ double npmax(double a, double b) { return (a != a) ? a : ((b != b) ? b : (b > a ? b : a)); }

template <int U, bool NT, bool GRIDSTRIDE>
__global__ void __launch_bounds__(256) k(const double *rows, long long stride, long long n, int M, const int *idx, double *mean,
                                         double *mn, double *mx)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += GRIDSTRIDE ? (long long)gridDim.x * 256 : n) {
        const double *p = rows + i;
        auto ld = [&](long long m) { return NT ? __builtin_nontemporal_load(p + m * stride) : p[m * stride]; };
        double x = ld(0), sum = x, lo = x, hi = x;
        int m = 1;
        for (; m + U <= M; m += U) {
            double raw[U];
#pragma unroll
            for (int u = 0; u < U; ++u) raw[u] = ld(m + u);
#pragma unroll
            for (int u = 0; u < U; ++u) { sum = sum + raw[u]; lo = npmin(lo, raw[u]); hi = npmax(hi, raw[u]); }
        }
        for (; m < M; ++m) { x = ld(m); sum = sum + x; lo = npmin(lo, x); hi = npmax(hi, x); }
        const long long d = idx ? idx[i] : i;
        mean[d] = sum / (double)M; mn[d] = lo; mx[d] = hi;
    }
}

int main()
{
    const long long n = 4000000;
    const int M = 51;
    const long long maxstride = n + 64;
    double *rows, *o[3];
    int *idx;
    CK(hipMalloc(&rows, sizeof(double) * M * maxstride));      // every variant reads below M * maxstride
    CK(hipMemset(rows, 0, sizeof(double) * M * maxstride));
    for (auto &p : o) CK(hipMalloc(&p, sizeof(double) * n));
    std::vector<int> h(n);
    std::iota(h.begin(), h.end(), 0);
    std::shuffle(h.begin(), h.end(), std::mt19937(1));           // a permutation of 0 .. n - 1: every index is below n
    CK(hipMalloc(&idx, sizeof(int) * n));
    CK(hipMemcpy(idx, h.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    hipEvent_t a, b;
    CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    const int blocks = (int)((n + 255) / 256);
    auto run = [&](const char *name, auto kernel, int grid, long long stride, const int *ix) -> int {
        float best = 1e9f;
        for (int rep = 0; rep < 6; ++rep) {
            CK(hipEventRecord(a));
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, 0, rows, stride, n, M, ix, o[0], o[1], o[2]);
            CK(hipEventRecord(b));
            CK(hipEventSynchronize(b));
            float ms; CK(hipEventElapsedTime(&ms, a, b));
            if (rep) best = std::min(best, ms);
        }
        CK(hipGetLastError());
        printf("%-44s stride n+%-3lld %s  %.4f ms  %.2f TB/s read\n", name, stride - n, ix ? "permuted" : "identity", best,
               M * n * 8.0 / best / 1e9);
        return 0;
    };
    for (long long pad : {0LL, 37LL, 64LL})
        for (const int *ix : {(const int *)nullptr, (const int *)idx}) {
            if (run("U8", k<8, false, false>, blocks, n + pad, ix)) return 1;
        }
    if (run("U16", k<16, false, false>, blocks, n, nullptr)) return 1;
    if (run("U4", k<4, false, false>, blocks, n, nullptr)) return 1;
    if (run("U8 nontemporal", k<8, true, false>, blocks, n, nullptr)) return 1;
    if (run("U8 nontemporal", k<8, true, false>, blocks, n, idx)) return 1;
    if (run("U16 nontemporal", k<16, true, false>, blocks, n, nullptr)) return 1;
    if (run("U8 grid-stride 2048", k<8, false, true>, 2048, n, nullptr)) return 1;
    if (run("U8 grid-stride 4096 nontemporal", k<8, true, true>, 4096, n, nullptr)) return 1;
    return 0;
}
