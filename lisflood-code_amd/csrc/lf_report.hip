// lf_report.hip -- report maps in the form a map writer takes: member rows and product maps as the device holds them ->
// [rows][H * W] rasters, float32 / float64 / int32, the fill outside the land mask, packed into one staging area that a
// single asynchronous copy brings to page-locked host memory (lf_device.cpp: lf_download_*).
//
//   k_pack_rasters<VEC> : blockIdx.y = source, a lane owns VEC consecutive cells of every row of its source
//
// The index table says per raster cell where the value sits in a source row (>= 0), that the cell is not land (-1: fill) or
// that the source's domain leaves the land pixel out (-2: zero).  Stores are full lines in raster order; the loads are
// coalesced where the table is monotone (rows in pixel order) and a gather where it permutes (rows in a sweep order).
#include "lf_common.h"

namespace {

constexpr int kPackLanes = 256;
constexpr int kPackMaxMaps = 16;
constexpr int kPackCellsPerLane = 4; // 4 x float32 / int32 = one 16-byte store, 4 x fp64 = two

struct pack_args {
    const void *src[kPackMaxMaps];
    void *dst[kPackMaxMaps];
    long long stride[kPackMaxMaps];
    double divisor[kPackMaxMaps];
    int rows[kPackMaxMaps];
    int kinds[kPackMaxMaps]; // 0: fp64 -> fp64, 1: fp64 -> float32, 2: int32 -> int32
    const int *idx;
    long long cells;
    double fill;
};

template <typename S, typename D, bool DIV>
__device__ __forceinline__ D pack_value(const S *__restrict__ row, int at, double divisor, D fill)
{
    if (at >= 0) {
        if constexpr (DIV)
            return (D)((double)row[at] / divisor);
        else
            return (D)row[at];
    }
    return at == -1 ? fill : (D)0;
}

template <typename D>
struct alignas(16) quad {
    D v[16 / sizeof(D)];
};

// the rows of one source for the VEC cells of a lane starting at `cell` (VEC == 1, or 4 with all of them inside)
template <typename S, typename D, bool DIV, int VEC>
__device__ __forceinline__ void pack_rows(const pack_args &A, int k, long long cell, const int (&at)[VEC])
{
    const S *src = (const S *)A.src[k];
    D *dst = (D *)A.dst[k] + cell;
    const D fill = (D)A.fill;
    const double divisor = A.divisor[k];
    for (int r = 0; r < A.rows[k]; ++r, src += A.stride[k], dst += A.cells) {
        if constexpr (VEC == 1) {
            dst[0] = pack_value<S, D, DIV>(src, at[0], divisor, fill);
        } else {
            D v[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = pack_value<S, D, DIV>(src, at[j], divisor, fill);
            constexpr int per = 16 / sizeof(D); // elements of one 16-byte store
#pragma unroll
            for (int q = 0; q < VEC / per; ++q) {
                quad<D> out;
#pragma unroll
                for (int j = 0; j < per; ++j) out.v[j] = v[q * per + j];
                *(quad<D> *)(dst + q * per) = out;
            }
        }
    }
}

template <int VEC>
__device__ __forceinline__ void pack_source(const pack_args &A, int k, long long cell, const int (&at)[VEC])
{
    const bool div = A.divisor[k] != 1.0; // (the same for every lane of the workgroup, like the kind)
    switch (A.kinds[k]) {
    case 0:
        if (div)
            pack_rows<double, double, true, VEC>(A, k, cell, at);
        else
            pack_rows<double, double, false, VEC>(A, k, cell, at);
        break;
    case 1:
        if (div)
            pack_rows<double, float, true, VEC>(A, k, cell, at);
        else
            pack_rows<double, float, false, VEC>(A, k, cell, at);
        break;
    default: pack_rows<int, int, false, VEC>(A, k, cell, at); break;
    }
}

template <int VEC>
__global__ void __launch_bounds__(kPackLanes) k_pack_rasters(pack_args A)
{
    const int k = (int)blockIdx.y;
    const long long cell = ((long long)blockIdx.x * kPackLanes + threadIdx.x) * VEC;
    if (cell >= A.cells) return;
    if constexpr (VEC == 1) {
        const int at[1] = {A.idx[cell]};
        pack_source<1>(A, k, cell, at);
    } else {
        if (cell + VEC <= A.cells) {
            const int4 t = *(const int4 *)(A.idx + cell); // (the table is 16-byte aligned: the host checked)
            const int at[4] = {t.x, t.y, t.z, t.w};
            pack_source<4>(A, k, cell, at);
        } else { // the last lane of a raster whose cells are no multiple of four
            for (long long c = cell; c < A.cells; ++c) {
                const int at[1] = {A.idx[c]};
                pack_source<1>(A, k, c, at);
            }
        }
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

} // namespace

int lf_pack_rasters_device(int device, int nmaps, const void *const *src_dev, void *const *dst_dev, const int32_t *rows_host,
                           const int64_t *stride_host, const int32_t *src_kind_host, const int32_t *dst_kind_host,
                           const double *divisor_host, const int32_t *idx_dev, int64_t cells, double fill)
{
    if (nmaps < 1 || nmaps > kPackMaxMaps)
        return lf_set_error(LF_E_INVALID, "pack rasters: nmaps must be 1 to %d (got %d)", kPackMaxMaps, nmaps);
    if (cells < 0 || cells > 0x7fffffffll)
        return lf_set_error(LF_E_INVALID, "pack rasters: cells = %lld outside the 32-bit range of a launch", (long long)cells);
    if (!src_dev || !dst_dev || !rows_host || !stride_host || !src_kind_host || !dst_kind_host || !divisor_host)
        return lf_set_error(LF_E_INVALID, "pack rasters: a host array (src_dev, dst_dev, rows_host, stride_host, src_kind_host, "
                                          "dst_kind_host, divisor_host) is NULL");
    pack_args A = {};
    bool wide = aligned16(idx_dev);
    for (int k = 0; k < nmaps; ++k) {
        if (rows_host[k] < 1) return lf_set_error(LF_E_INVALID, "pack rasters: rows_host[%d] must be at least 1 (got %d)", k, (int)rows_host[k]);
        if (stride_host[k] < 0) return lf_set_error(LF_E_INVALID, "pack rasters: stride_host[%d] = %lld is negative", k, (long long)stride_host[k]);
        const int sk = src_kind_host[k], dk = dst_kind_host[k];
        if (sk != LF_PACK_F64 && sk != LF_PACK_I32)
            return lf_set_error(LF_E_INVALID, "pack rasters: src_kind_host[%d] = %d is neither fp64 (%d) nor int32 (%d)", k, sk, LF_PACK_F64, LF_PACK_I32);
        if (dk != LF_PACK_F64 && dk != LF_PACK_F32 && dk != LF_PACK_I32)
            return lf_set_error(LF_E_INVALID, "pack rasters: dst_kind_host[%d] = %d is none of fp64 (%d), float32 (%d), int32 (%d)", k, dk,
                                LF_PACK_F64, LF_PACK_F32, LF_PACK_I32);
        if ((sk == LF_PACK_I32) != (dk == LF_PACK_I32))
            return lf_set_error(LF_E_INVALID, "pack rasters: source %d: an fp64 source goes to fp64 or float32, an int32 source to int32 "
                                              "(src_kind_host %d, dst_kind_host %d)", k, sk, dk);
        if (sk == LF_PACK_I32 && divisor_host[k] != 1.0)
            return lf_set_error(LF_E_INVALID, "pack rasters: divisor_host[%d] must be 1 for an int32 source (got %g)", k, divisor_host[k]);
        if (cells > 0 && !src_dev[k]) return lf_set_error(LF_E_INVALID, "pack rasters: src_dev[%d] is NULL", k);
        if (cells > 0 && !dst_dev[k]) return lf_set_error(LF_E_INVALID, "pack rasters: dst_dev[%d] is NULL", k);
        A.src[k] = src_dev[k];
        A.dst[k] = dst_dev[k];
        A.stride[k] = (long long)stride_host[k];
        A.divisor[k] = divisor_host[k];
        A.rows[k] = rows_host[k];
        A.kinds[k] = dk;
        // 16-byte stores: every row of the destination starts on a 16-byte boundary
        const size_t row_bytes = (size_t)cells * (dk == LF_PACK_F64 ? 8 : 4);
        wide = wide && aligned16(dst_dev[k]) && (rows_host[k] == 1 || row_bytes % 16 == 0);
    }
    if (cells > 0 && !idx_dev) return lf_set_error(LF_E_INVALID, "pack rasters: idx_dev is NULL");
    if (cells == 0) return LF_OK;
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    A.idx = (const int *)idx_dev;
    A.cells = (long long)cells;
    A.fill = fill;
    static const bool one_cell = [] { // LF_PACK_CELLS=1: one cell per lane whatever the alignment (A/B switch)
        const char *e = std::getenv("LF_PACK_CELLS");
        return e && e[0] == '1';
    }();
    if (wide && !one_cell) {
        const int64_t lanes = (cells + kPackCellsPerLane - 1) / kPackCellsPerLane;
        hipLaunchKernelGGL(k_pack_rasters<kPackCellsPerLane>, dim3((unsigned)((lanes + kPackLanes - 1) / kPackLanes), (unsigned)nmaps),
                           dim3(kPackLanes), 0, c->stream, A);
    } else {
        hipLaunchKernelGGL(k_pack_rasters<1>, dim3((unsigned)((cells + kPackLanes - 1) / kPackLanes), (unsigned)nmaps), dim3(kPackLanes),
                           0, c->stream, A);
    }
    LF_HIP(hipGetLastError());
    return LF_OK;
}
