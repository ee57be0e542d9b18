// lf_members.hip -- products over the members of an ensemble, element by element: what a forecast or a calibration reads
// out of `members` rows of n doubles, `stride` elements apart (hotpath.HotPathEnsemble keeps every member vector that way),
// without the rows ever leaving the device.
//
//   k_members_summary : mean, minimum, maximum and the number of members above up to four threshold maps, one pass
//   k_members_order   : order statistics (the value with exactly r values before it in the stable order), column in LDS
//   k_members_track   : one step folded into run-long accumulators per member -- peak and its step, sum, first step above
//                       and steps above up to four threshold maps -- rows laid out like their source
//   k_members_transform / k_members_resample : the analysis step of an assimilation cycle, the only kernels here that WRITE
//                       the member rows -- x_new[m] = sum_k x[k] W[k][m] with taper and bounds, x_new[m] = x[parents[m]];
//                       in place, the element's column in LDS before the first store (their own section below)
//   k_members_regress : the localised serial analysis -- the increments of up to 256 gauges regressed onto the element's
//                       column in one pass, each weighted by Gaspari-Cohn's function of the element's distance to the gauge
//                       (k_members_regress_reg: the column in registers, up to 16 members)
//   k_members_perturb : the forecast step's counterpart -- the member rows written or rewritten from one base row or their
//                       own values plus / times a sum of `rank` static patterns weighted by a [members][rank] table
//   k_members_zonal   : the one kernel here that sums ACROSS the elements of a row -- runs of up to 256 entries of every
//                       member's row, one wavefront per run, in an order the plan fixes (its own section below)
//
// The value of (m, i) is rows[m * stride + i] / divisor, an IEEE division (divisor 1: the element itself), the result of
// element i goes to dst_index ? dst_index[i] : i.  Everything is in member order: the sum is ((x0 + x1) + x2) + ..., the
// folds keep the earlier member on a tie.  Elements between n and stride are never read.
#include "lf_common.h"
#include "lf_structures.h" // lf_npmin / lf_npmax

namespace {

constexpr int kSummaryLanes = 256; // one lane per element: a row load of a wavefront is 64 x 8 B = 512 B, coalesced
constexpr int kUnroll = 8;         // rows in flight per lane (the arithmetic behind them stays in member order)
constexpr int kMaxThresholds = 4;
constexpr int kMaxRanks = 8;
constexpr int kMaxOrderMembers = 128;
constexpr size_t kOrderTileBytes = 64 * 1024; // of the 160 KiB of a CU: two workgroups

struct members_rows {
    const double *rows;
    long long stride, n, dst_n;
    int members;
    double divisor;
    const int *dst_index;
};

struct summary_out {
    double *mean, *min, *max;
    const double *thresholds;
    long long threshold_stride;
    int *exceed;
};

struct track_out {
    double *peak;
    int *peak_step;
    double *sum;
    const double *thresholds;
    long long threshold_stride;
    int *first_above, *steps_above;
    long long track_stride;
    int step;
};

struct order_out {
    int n_ranks;
    int ranks[kMaxRanks];
    double *out;
};

template <bool DIV>
__device__ __forceinline__ double member_value(double raw, double divisor)
{
    return DIV ? raw / divisor : raw;
}

// a row element is read once and never again: loaded past the caches' keep policy, which leaves L2 to the scattered
// stores of the outputs (a tenth to a fifth faster at 51 rows of 4e6 elements)
__device__ __forceinline__ double row_load(const double *p) { return __builtin_nontemporal_load(p); }

template <int NT, bool DIV>
__global__ void __launch_bounds__(kSummaryLanes) k_members_summary(members_rows R, summary_out O)
{
    const long long i = (long long)blockIdx.x * kSummaryLanes + threadIdx.x;
    if (i >= R.n) return;
    double thr[NT > 0 ? NT : 1];
    int above[NT > 0 ? NT : 1];
#pragma unroll
    for (int t = 0; t < NT; ++t) thr[t] = O.thresholds[(long long)t * O.threshold_stride + i];
    const double *p = R.rows + i;
    double x = member_value<DIV>(row_load(p), R.divisor);
    double sum = x, lo = x, hi = x;
#pragma unroll
    for (int t = 0; t < NT; ++t) above[t] = x > thr[t] ? 1 : 0;
    auto take = [&](double raw) {
        const double v = member_value<DIV>(raw, R.divisor);
        sum = sum + v;
        lo = lf_npmin(lo, v);
        hi = lf_npmax(hi, v);
#pragma unroll
        for (int t = 0; t < NT; ++t) above[t] += v > thr[t] ? 1 : 0;
    };
    int m = 1;
    for (; m + kUnroll <= R.members; m += kUnroll) {
        double raw[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) raw[u] = row_load(p + (long long)(m + u) * R.stride);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) take(raw[u]);
    }
    for (; m < R.members; ++m) take(row_load(p + (long long)m * R.stride));
    const long long dst = R.dst_index ? (long long)R.dst_index[i] : i;
    if (O.mean) O.mean[dst] = sum / (double)R.members;
    if (O.min) O.min[dst] = lo;
    if (O.max) O.max[dst] = hi;
#pragma unroll
    for (int t = 0; t < NT; ++t) O.exceed[(long long)t * R.dst_n + dst] = above[t];
}

// What one (member, element) holds of its accumulators while a group of source rows is in flight: the peak, the sum and, per
// threshold, steps_above -- or first_above where there is no steps_above (its sign then says whether the value was above before).
template <int NT>
struct track_held {
    double peak, sum;
    int had[NT > 0 ? NT : 1];
};

// The streaming update of the run-long accumulators (lf_members_track_device): the summary kernel's shape -- one lane per
// element, its NT thresholds in registers, kUnroll source rows in flight -- with the member's accumulators loaded beside its
// source row.  Every (member, element) has one owner; peak, peak_step and first_above are stored only where they change,
// steps_above only where it counts, peak_step and (with steps_above) first_above are never loaded.  FIRST: nothing is loaded.
template <int NT, bool DIV, bool FIRST>
__global__ void __launch_bounds__(kSummaryLanes) k_members_track(members_rows R, track_out O)
{
    const long long i = (long long)blockIdx.x * kSummaryLanes + threadIdx.x;
    if (i >= R.n) return;
    double thr[NT > 0 ? NT : 1];
#pragma unroll
    for (int t = 0; t < NT; ++t) thr[t] = O.thresholds[(long long)t * O.threshold_stride + i];
    const double *p = R.rows + i;
    auto row_of = [&](int t, int m) { return ((long long)t * R.members + m) * O.track_stride + i; };
    auto load = [&](int m) {
        track_held<NT> h = {};
        if (!FIRST) {
            if (O.peak) h.peak = O.peak[row_of(0, m)];
            if (O.sum) h.sum = O.sum[row_of(0, m)];
#pragma unroll
            for (int t = 0; t < NT; ++t) h.had[t] = O.steps_above ? O.steps_above[row_of(t, m)] : O.first_above[row_of(t, m)];
        }
        return h;
    };
    auto take = [&](int m, double raw, const track_held<NT> &h) {
        const double v = member_value<DIV>(raw, R.divisor);
        const long long at = row_of(0, m);
        if (FIRST) {
            if (O.peak) O.peak[at] = v;
            if (O.peak_step) O.peak_step[at] = O.step;
            if (O.sum) O.sum[at] = v;
        } else {
            if (O.peak && ((v > h.peak) || (v != v && h.peak == h.peak))) {
                O.peak[at] = v;
                if (O.peak_step) O.peak_step[at] = O.step;
            }
            if (O.sum) O.sum[at] = h.sum + v;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bool above = v > thr[t];
            const long long att = row_of(t, m);
            if (FIRST) {
                if (O.first_above) O.first_above[att] = above ? O.step : -1;
                if (O.steps_above) O.steps_above[att] = above ? 1 : 0;
            } else if (above) {
                if (O.first_above && (O.steps_above ? h.had[t] == 0 : h.had[t] < 0)) O.first_above[att] = O.step;
                if (O.steps_above) O.steps_above[att] = h.had[t] + 1;
            }
        }
    };
    int m = 0;
    for (; m + kUnroll <= R.members; m += kUnroll) {
        double raw[kUnroll];
        track_held<NT> held[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) raw[u] = row_load(p + (long long)(m + u) * R.stride);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) held[u] = load(m + u);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) take(m + u, raw[u], held[u]);
    }
    for (; m < R.members; ++m) take(m, row_load(p + (long long)m * R.stride), load(m));
}

// a goes before b whatever their members: a < b, or b is a NaN and a is none (np.sort puts the NaNs last)
__device__ __forceinline__ bool goes_before(double a, double b) { return a < b || (b != b && a == a); }

// The lane's column sits in LDS as tile[m * W + lane]: a lane reads and writes only its own column, so there is no barrier,
// and consecutive lanes hit consecutive banks.  Rank counting: member j has before it every member that goes before it by
// value, and of those that tie with it the ones with a lower index -- np.sort(kind="stable") along the members.
template <int W, bool DIV>
__global__ void __launch_bounds__(W) k_members_order(members_rows R, order_out O)
{
    extern __shared__ double tile[];
    const int lane = threadIdx.x;
    const long long i = (long long)blockIdx.x * W + lane;
    if (i >= R.n) return;
    const double *p = R.rows + i;
    const int M = R.members;
    int m = 0;
    for (; m + kUnroll <= M; m += kUnroll) {
        double raw[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) raw[u] = row_load(p + (long long)(m + u) * R.stride);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) tile[(m + u) * W + lane] = member_value<DIV>(raw[u], R.divisor);
    }
    for (; m < M; ++m) tile[m * W + lane] = member_value<DIV>(row_load(p + (long long)m * R.stride), R.divisor);
    const long long dst = R.dst_index ? (long long)R.dst_index[i] : i;
    for (int j = 0; j < M; ++j) {
        const double xj = tile[j * W + lane];
        int before = 0;
        for (int k = 0; k < j; ++k) before += goes_before(xj, tile[k * W + lane]) ? 0 : 1;
        for (int k = j + 1; k < M; ++k) before += goes_before(tile[k * W + lane], xj) ? 1 : 0;
        for (int r = 0; r < O.n_ranks; ++r)
            if (O.ranks[r] == before) O.out[(long long)r * R.dst_n + dst] = xj;
    }
}

// ---- the analysis step of an ensemble: the members' rows rewritten in place, element by element --------------------------------
constexpr int kMaxTransformMembers = 64;  // the weight table: 64 x 64 doubles = 32 KiB, read through the scalar cache
constexpr int kMaxResampleMembers = 128;
constexpr int kBlock = 8;                 // output members per register block: 8 accumulators with compile-time indices
constexpr int kStage = 16;                // rows in flight per lane while the column goes to LDS

struct transform_args {
    long long stride, n;
    int members;
    double lower, upper;
};

struct resample_plan {
    int n_src, n_dst;
    unsigned char src[kMaxResampleMembers];  // the rows some OTHER row draws from, each once: slot s of the tile holds row src[s]
    unsigned char dst[kMaxResampleMembers];  // the rows with parents[m] != m ...
    unsigned char slot[kMaxResampleMembers]; // ... and the slot their parent sits in
};

// One register block of the transform: output members m0 .. m0 + kBlock - 1 of the lane's column (in LDS, complete) -- the
// sum in ascending k with one multiply and one add each, then taper and bounds, then the store.  The weight addresses are
// uniform across the lanes (k, m0 and M come from kernel arguments): scalar loads.  FULL: the block lies inside the table;
// otherwise the columns past M - 1 read column M - 1 again and store nothing.
template <int W, bool FULL>
__device__ __forceinline__ void transform_block(const double *tile, int lane, double *__restrict__ out, const double *__restrict__ w,
                                                int M, int m0, long long stride, bool tapered, double tp, double lo, double hi)
{
    int col[kBlock];
#pragma unroll
    for (int j = 0; j < kBlock; ++j) col[j] = FULL ? m0 + j : (m0 + j < M ? m0 + j : M - 1);
    double acc[kBlock];
    const double x0 = tile[lane];
#pragma unroll
    for (int j = 0; j < kBlock; ++j) acc[j] = x0 * w[col[j]];
#pragma unroll 4                        // (the weights and column values of four k in flight ahead of their 64 operations)
    for (int k = 1; k < M; ++k) {
        const double xk = tile[k * W + lane];
        const double *wk = w + k * M;
#pragma unroll
        for (int j = 0; j < kBlock; ++j) acc[j] = acc[j] + xk * wk[col[j]];
    }
#pragma unroll
    for (int j = 0; j < kBlock; ++j) {
        if (!FULL && m0 + j >= M) break;
        double v = acc[j];
        if (tapered) {
            const double xm = tile[(m0 + j) * W + lane];
            v = xm + tp * (v - xm);
        }
        v = (lo > v || (lo != lo && v == v)) ? lo : v;
        v = (hi < v || (hi != hi && v == v)) ? hi : v;
        out[(long long)(m0 + j) * stride] = v;
    }
}

// x_new[m] = sum_k x[k] W[k][m] in place (lf_members_transform_device).  A lane owns element i of every member: the column
// goes to LDS as tile[k * W + lane] (k_members_order's layout: no barrier, consecutive lanes on consecutive banks) before
// the first store, and no row is read from global again.  The element's taper and bound values are read once.
template <int W>
__global__ void __launch_bounds__(W)
k_members_transform(double *__restrict__ rows, const double *__restrict__ weights, const double *__restrict__ taper,
                    const double *__restrict__ lower_dev, const double *__restrict__ upper_dev, transform_args A)
{
    extern __shared__ double tile[];
    const int lane = threadIdx.x;
    const long long i = (long long)blockIdx.x * W + lane;
    if (i >= A.n) return;
    double *p = rows + i;
    const int M = A.members;
    int k = 0;
    for (; k + kStage <= M; k += kStage) {
        double raw[kStage];
#pragma unroll
        for (int u = 0; u < kStage; ++u) raw[u] = row_load(p + (long long)(k + u) * A.stride);
#pragma unroll
        for (int u = 0; u < kStage; ++u) tile[(k + u) * W + lane] = raw[u];
    }
    for (; k < M; ++k) tile[k * W + lane] = row_load(p + (long long)k * A.stride);
    const bool tapered = taper != nullptr;
    const double tp = tapered ? taper[i] : 1.0;
    const double lo = lower_dev ? lower_dev[i] : A.lower;
    const double hi = upper_dev ? upper_dev[i] : A.upper;
    int m0 = 0;
    for (; m0 + kBlock <= M; m0 += kBlock) transform_block<W, true>(tile, lane, p, weights, M, m0, A.stride, tapered, tp, lo, hi);
    if (m0 < M) transform_block<W, false>(tile, lane, p, weights, M, m0, A.stride, tapered, tp, lo, hi);
}

// x_new[m] = x[parents[m]] in place (lf_members_resample_device): the rows another row draws from go to LDS, each once, then
// the rows that change are stored.  A row that keeps itself is not stored, and loaded only where another row draws from it.
template <int W>
__global__ void __launch_bounds__(W) k_members_resample(double *__restrict__ rows, long long stride, long long n, resample_plan P)
{
    extern __shared__ double tile[];
    const int lane = threadIdx.x;
    const long long i = (long long)blockIdx.x * W + lane;
    if (i >= n) return;
    double *p = rows + i;
    int s = 0;
    for (; s + kUnroll <= P.n_src; s += kUnroll) {
        double raw[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) raw[u] = row_load(p + (long long)P.src[s + u] * stride);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) tile[(s + u) * W + lane] = raw[u];
    }
    for (; s < P.n_src; ++s) tile[s * W + lane] = row_load(p + (long long)P.src[s] * stride);
    for (int d = 0; d < P.n_dst; ++d) p[(long long)P.dst[d] * stride] = tile[P.slot[d] * W + lane];
}

// ---- the localised serial analysis: the increments of every gauge regressed onto the element's column in one pass ------------
constexpr int kMaxRegressGauges = 256;    // the table: 256 (2 x 64 + 5) doubles = 266 KiB at most, read through the scalar cache

struct regress_args {
    long long stride, n;
    int members, gauges, bounded;
    double lower, upper;
};

// Gaspari-Cohn's fifth-order function of z = distance / half-width in the header's Horner form, 0 <= z < 2
__device__ __forceinline__ double gaspari_cohn(double z)
{
    constexpr double C53 = 5.0 / 3.0, C112 = 1.0 / 12.0, C23 = 2.0 / 3.0;
    if (z <= 1.0) {
        double p = -0.25 * z + 0.5;
        p = p * z + 0.625;
        p = p * z - C53;
        p = p * z;
        return p * z + 1.0;
    }
    double q = C112 * z - 0.5;
    q = q * z + 0.625;
    q = q * z + C53;
    q = q * z - 5.0;
    q = q * z + 4.0;
    return q - C23 / z;
}

// x[k] += rho_j (sum_k x[k] A[j][k]) s[j] D[j][k] for the gauges j in ascending order, in place
// (lf_members_regress_device).  k_members_transform's shape: a lane owns element i of every member, its column sits in LDS
// as tile[k * W + lane] from the load to the store and every gauge works on it there.  Every table address is uniform
// across the lanes (j, k and the section offsets come from kernel arguments and loop counters): scalar loads.  A gauge
// with no lane of the wavefront in range is left before the square root and the divisions by one wave-wide vote; the vote
// only saves work -- each lane's own `in` decides what happens to its column.  A lane whose column no gauge touched stores
// nothing unless the call has bounds.
template <int W>
__global__ void __launch_bounds__(W)
k_members_regress(double *__restrict__ rows, const double *__restrict__ cx, const double *__restrict__ cy,
                  const double *__restrict__ table, const double *__restrict__ lower_dev, const double *__restrict__ upper_dev,
                  regress_args A)
{
    extern __shared__ double tile[];
    const int lane = threadIdx.x;
    const long long i = (long long)blockIdx.x * W + lane;
    if (i >= A.n) return;
    double *p = rows + i;
    const int M = A.members, G = A.gauges;
    int k = 0;
    for (; k + kStage <= M; k += kStage) {
        double raw[kStage];
#pragma unroll
        for (int u = 0; u < kStage; ++u) raw[u] = row_load(p + (long long)(k + u) * A.stride);
#pragma unroll
        for (int u = 0; u < kStage; ++u) tile[(k + u) * W + lane] = raw[u];
    }
    for (; k < M; ++k) tile[k * W + lane] = row_load(p + (long long)k * A.stride);
    const double ex = cx[i], ey = cy[i];
    const double *anomalies = table, *increments = table + G * M, *scale = table + 2 * G * M;
    const double *gx = scale + G, *gy = gx + G, *width = gy + G, *cut2 = width + G;
    bool touched = false;
    for (int j = 0; j < G; ++j) {
        const double dx = ex - gx[j], dy = ey - gy[j];
        const double d2 = dx * dx + dy * dy;
        const bool in = d2 < cut2[j];
        if (!__any(in)) continue;
        if (!in) continue;
        const double rho = gaspari_cohn(sqrt(d2) / width[j]);
        if (!(rho > 0.0)) continue;
        const double *a = anomalies + j * M, *d = increments + j * M;
        double cov = tile[lane] * a[0];
#pragma unroll 4
        for (int m = 1; m < M; ++m) cov = cov + tile[m * W + lane] * a[m];
        const double g = rho * (cov * scale[j]);
#pragma unroll 4
        for (int m = 0; m < M; ++m) tile[m * W + lane] = tile[m * W + lane] + g * d[m];
        touched = true;
    }
    if (!touched && !A.bounded) return;
    const double lo = lower_dev ? lower_dev[i] : A.lower;
    const double hi = upper_dev ? upper_dev[i] : A.upper;
    for (int m = 0; m < M; ++m) {
        double v = tile[m * W + lane];
        v = (lo > v || (lo != lo && v == v)) ? lo : v;
        v = (hi < v || (hi != hi && v == v)) ? hi : v;
        p[(long long)m * A.stride] = v;
    }
}

// The same arithmetic, line for line, with the column in registers for a member count known at compile time (2 to 16): no
// LDS, so the registers set the residency (38 VGPRs at 4 members, 86 at 16), and the member loops are unrolled around
// scalar operands.  Measured against the LDS kernel on the same rows it is never slower beyond the repeat spread and up
// to 28 % faster where many gauges are in range, so up to 16 members it is the one that runs.
constexpr int kMaxRegressRegisterMembers = 16;

template <int M>
__global__ void __launch_bounds__(256)
k_members_regress_reg(double *__restrict__ rows, const double *__restrict__ cx, const double *__restrict__ cy,
                      const double *__restrict__ table, const double *__restrict__ lower_dev, const double *__restrict__ upper_dev,
                      regress_args A)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    double *p = rows + i;
    const int G = A.gauges;
    double x[M];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = row_load(p + (long long)m * A.stride);
    const double ex = cx[i], ey = cy[i];
    const double *anomalies = table, *increments = table + G * M, *scale = table + 2 * G * M;
    const double *gx = scale + G, *gy = gx + G, *width = gy + G, *cut2 = width + G;
    bool touched = false;
    for (int j = 0; j < G; ++j) {
        const double dx = ex - gx[j], dy = ey - gy[j];
        const double d2 = dx * dx + dy * dy;
        const bool in = d2 < cut2[j];
        if (!__any(in)) continue;
        if (!in) continue;
        const double rho = gaspari_cohn(sqrt(d2) / width[j]);
        if (!(rho > 0.0)) continue;
        const double *a = anomalies + j * M, *d = increments + j * M;
        double cov = x[0] * a[0];
#pragma unroll
        for (int m = 1; m < M; ++m) cov = cov + x[m] * a[m];
        const double g = rho * (cov * scale[j]);
#pragma unroll
        for (int m = 0; m < M; ++m) x[m] = x[m] + g * d[m];
        touched = true;
    }
    if (!touched && !A.bounded) return;
    const double lo = lower_dev ? lower_dev[i] : A.lower;
    const double hi = upper_dev ? upper_dev[i] : A.upper;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        double v = x[m];
        v = (lo > v || (lo != lo && v == v)) ? lo : v;
        v = (hi < v || (hi != hi && v == v)) ? hi : v;
        p[(long long)m * A.stride] = v;
    }
}

template <int M>
void launch_regress_reg(hipStream_t s, double *rows, const double *cx, const double *cy, const double *table,
                        const double *lower_dev, const double *upper_dev, const regress_args &A)
{
    const dim3 grid((unsigned)((A.n + 255) / 256)), block(256);
    hipLaunchKernelGGL((k_members_regress_reg<M>), grid, block, 0, s, rows, cx, cy, table, lower_dev, upper_dev, A);
}

template <int W>
void launch_regress(hipStream_t s, double *rows, const double *cx, const double *cy, const double *table, const double *lower_dev,
                    const double *upper_dev, const regress_args &A)
{
    const dim3 grid((unsigned)((A.n + W - 1) / W)), block(W);
    hipLaunchKernelGGL((k_members_regress<W>), grid, block, (size_t)A.members * W * sizeof(double), s, rows, cx, cy, table,
                       lower_dev, upper_dev, A);
}

// ---- the forecast step's counterpart: member rows perturbed from a few static patterns and a [members][rank] table ----------
constexpr int kMaxPerturbMembers = 128;
constexpr int kMaxPerturbRank = 16;   // 128 x 16 coefficients = 16 KiB: lf_device_ctx::kPerturbTableBytes
constexpr int kPerturbLanes = 256;

struct perturb_args {
    long long stride, n, pattern_stride;
    int members, multiplicative;
    double lower, upper;
};

// s = sum_r c[r] P[r] in ascending r with one multiply and one add each, then the base, the mode and the bounds.  c is uniform
// across the lanes (the member comes from a loop counter, the table from a kernel argument): RANK scalar loads.
template <int RANK>
__device__ __forceinline__ double perturb_value(const double (&P)[RANK], const double *__restrict__ c, double b, bool mul, double lo,
                                                double hi)
{
    double s = c[0] * P[0];
#pragma unroll
    for (int r = 1; r < RANK; ++r) s = s + c[r] * P[r];
    double v = mul ? b * (1.0 + s) : b + s;
    v = (lo > v || (lo != lo && v == v)) ? lo : v;
    v = (hi < v || (hi != hi && v == v)) ? hi : v;
    return v;
}

// rows[m][i] = bound(base (+ or * (1 +)) sum_r coeff[m][r] patterns[r][i]) (lf_members_perturb_device).  A lane owns element
// i of every member: its RANK pattern values, its bound values and (OWN = false) the one base value are loaded together and
// stay in registers while it walks the members, every store a full line of consecutive positions.  OWN: every member's row is
// its own base; the rows are loaded kStage at a time ahead of their arithmetic, each element read once and stored once.
// base may be rows (member 0's row): the lane has read base[i] before it stores rows[0 * stride + i] and no other lane
// touches element i, so neither pointer is __restrict__.  No LDS.
template <int RANK, bool OWN>
__global__ void __launch_bounds__(kPerturbLanes)
k_members_perturb(double *rows, const double *base, const double *__restrict__ patterns, const double *__restrict__ coeff,
                  const double *__restrict__ lower_dev, const double *__restrict__ upper_dev, perturb_args A)
{
    const long long i = (long long)blockIdx.x * kPerturbLanes + threadIdx.x;
    if (i >= A.n) return;
    double P[RANK];
#pragma unroll
    for (int r = 0; r < RANK; ++r) P[r] = patterns[(long long)r * A.pattern_stride + i];
    const double lo = lower_dev ? lower_dev[i] : A.lower;
    const double hi = upper_dev ? upper_dev[i] : A.upper;
    const bool mul = A.multiplicative != 0;
    const int M = A.members;
    double *p = rows + i;
    if (!OWN) {
        const double b = base[i];
#pragma unroll 4                        // (the coefficients of four members in flight ahead of their arithmetic)
        for (int m = 0; m < M; ++m) p[(long long)m * A.stride] = perturb_value<RANK>(P, coeff + m * RANK, b, mul, lo, hi);
        return;
    }
    int m = 0;
    for (; m + kStage <= M; m += kStage) {
        double raw[kStage];
#pragma unroll
        for (int u = 0; u < kStage; ++u) raw[u] = row_load(p + (long long)(m + u) * A.stride);
#pragma unroll
        for (int u = 0; u < kStage; ++u)
            p[(long long)(m + u) * A.stride] = perturb_value<RANK>(P, coeff + (m + u) * RANK, raw[u], mul, lo, hi);
    }
    for (; m < M; ++m) {
        double *q = p + (long long)m * A.stride;
        *q = perturb_value<RANK>(P, coeff + m * RANK, row_load(q), mul, lo, hi);
    }
}

template <int RANK>
void launch_perturb(hipStream_t s, double *rows, const double *base, const double *patterns, const double *coeff,
                    const double *lower_dev, const double *upper_dev, const perturb_args &A)
{
    const dim3 grid((unsigned)((A.n + kPerturbLanes - 1) / kPerturbLanes)), block(kPerturbLanes);
    if (base)
        hipLaunchKernelGGL((k_members_perturb<RANK, false>), grid, block, 0, s, rows, base, patterns, coeff, lower_dev, upper_dev, A);
    else
        hipLaunchKernelGGL((k_members_perturb<RANK, true>), grid, block, 0, s, rows, base, patterns, coeff, lower_dev, upper_dev, A);
}

// ---- sums across the elements of a member row: runs of up to 256 entries, one wavefront per run, in a fixed order --------------
constexpr int kZonalRun = 256;          // entries of a run: four per lane of a wavefront
constexpr int kZonalPerLane = kZonalRun / 64;
constexpr int kZonalWaves = 4;          // runs (wavefronts) per workgroup
constexpr int kZonalMembers = 4;        // members whose four loads per lane are in flight before the first fold
constexpr long long kZonalFewBlocks = 1024; // below this many workgroups of runs the members go on the grid as well

struct zonal_args {
    const double *rows;
    long long stride;
    double divisor;
    const int *index;
    const double *weights;
    long long runs;
    const int *run_start;
    double *out;
    long long out_stride;
    int members, members_per_block;
};

// One pass of the zonal reduction (lf_members_zonal_device).  A wavefront owns run r = entries run_start[r] .. run_start[r + 1]
// - 1: lane l holds the row positions and weights of entries l, l + 64, l + 128 and l + 192 of the run in registers and walks
// the members, kZonalMembers at a time -- their 4 x kZonalMembers loads are issued before the first addition.  A lane past the
// end of its run loads nothing and contributes a selected +0.0 (never a product); the lane sum is ((0.0 + v0) + v1) + v2) + v3
// and the fold s[l] = s[l] + s[l + d], d = 32 .. 1, goes through __shfl_down, so every run sum has one order whatever the
// grid: blockIdx.y only says which members this wavefront walks.  Lane 0 stores.  No atomics, no LDS.
template <bool DIV, bool WEIGHTED>
__global__ void __launch_bounds__(64 * kZonalWaves) k_members_zonal(zonal_args A)
{
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * kZonalWaves + (threadIdx.x >> 6);
    if (r >= A.runs) return;
    const int first = A.run_start[r], len = A.run_start[r + 1] - first;
    bool on[kZonalPerLane];
    long long at[kZonalPerLane];
    double w[kZonalPerLane];
#pragma unroll
    for (int k = 0; k < kZonalPerLane; ++k) {
        const int e = lane + 64 * k;
        on[k] = e < len;
        at[k] = on[k] ? (A.index ? (long long)A.index[first + e] : (long long)first + e) : 0;
        w[k] = (WEIGHTED && on[k]) ? A.weights[first + e] : 0.0;
    }
    auto value = [&](int k, double raw) {
        double v = member_value<DIV>(raw, A.divisor);
        if (WEIGHTED) v = v * w[k];
        return on[k] ? v : 0.0;
    };
    auto fold = [&](int m, const double (&raw)[kZonalPerLane]) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < kZonalPerLane; ++k) s = s + value(k, raw[k]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_down(s, d);
        if (lane == 0) A.out[(long long)m * A.out_stride + r] = s;
    };
    auto load = [&](int m, double (&raw)[kZonalPerLane]) {
        const double *p = A.rows + (long long)m * A.stride;
#pragma unroll
        for (int k = 0; k < kZonalPerLane; ++k) raw[k] = on[k] ? row_load(p + at[k]) : 0.0;
    };
    int m = blockIdx.y * A.members_per_block;
    const int end = m + A.members_per_block < A.members ? m + A.members_per_block : A.members;
    for (; m + kZonalMembers <= end; m += kZonalMembers) {
        double raw[kZonalMembers][kZonalPerLane];
#pragma unroll
        for (int u = 0; u < kZonalMembers; ++u) load(m + u, raw[u]);
#pragma unroll
        for (int u = 0; u < kZonalMembers; ++u) fold(m + u, raw[u]);
    }
    for (; m < end; ++m) {
        double raw[kZonalPerLane];
        load(m, raw);
        fold(m, raw);
    }
}

template <bool DIV>
void launch_zonal(hipStream_t s, const zonal_args &A, dim3 grid)
{
    const dim3 block(64 * kZonalWaves);
    if (A.weights)
        hipLaunchKernelGGL((k_members_zonal<DIV, true>), grid, block, 0, s, A);
    else
        hipLaunchKernelGGL((k_members_zonal<DIV, false>), grid, block, 0, s, A);
}

// what the two perturb entry points refuse, in the order the header lists it (no device is touched)
int check_perturb(const double *rows_dev, int members, int64_t stride, int64_t n, int rank, const double *patterns_dev,
                  int64_t pattern_stride, const double *coeff_host, int multiplicative, const double *lower_dev, double lower,
                  const double *upper_dev, double upper)
{
    if (!rows_dev) return lf_set_error(LF_E_INVALID, "rows_dev is NULL");
    if (!patterns_dev) return lf_set_error(LF_E_INVALID, "patterns_dev is NULL");
    if (!coeff_host) return lf_set_error(LF_E_INVALID, "coeff_host is NULL");
    if (members < 1) return lf_set_error(LF_E_INVALID, "members must be at least 1 (got %d)", members);
    if (members > kMaxPerturbMembers)
        return lf_set_error(LF_E_INVALID, "members = %d: a perturbation takes at most %d members", members, kMaxPerturbMembers);
    if (rank < 1 || rank > kMaxPerturbRank) return lf_set_error(LF_E_INVALID, "rank must be 1 to %d (got %d)", kMaxPerturbRank, rank);
    if (n < 0 || n > 0x7fffffffll) return lf_set_error(LF_E_INVALID, "n = %lld outside the 32-bit range of a launch", (long long)n);
    if (members > 1 && stride < n) return lf_set_error(LF_E_INVALID, "stride %lld is less than n = %lld", (long long)stride, (long long)n);
    if (rank > 1 && pattern_stride < n)
        return lf_set_error(LF_E_INVALID, "pattern_stride %lld is less than n = %lld", (long long)pattern_stride, (long long)n);
    if (multiplicative != 0 && multiplicative != 1)
        return lf_set_error(LF_E_INVALID, "multiplicative must be 0 or 1 (got %d)", multiplicative);
    if (!lower_dev && !upper_dev && lower > upper)
        return lf_set_error(LF_E_INVALID, "lower = %g is greater than upper = %g", lower, upper);
    return LF_OK;
}

// The coefficient table goes up through a page-locked slot into the next table of the context's ring, on `s`; the kernel
// behind it on `s`; the event behind the kernel is what the slot's next user makes ITS stream wait for.  The host never waits.
int enqueue_perturb(lf_device_ctx *c, hipStream_t s, double *rows_dev, int members, int64_t stride, int64_t n, const double *base_dev,
                    int rank, const double *patterns_dev, int64_t pattern_stride, const double *coeff_host, int multiplicative,
                    const double *lower_dev, double lower, const double *upper_dev, double upper)
{
    if (!c->perturb_tables) LF_HIP(hipMalloc(&c->perturb_tables, lf_device_ctx::kPerturbSlots * lf_device_ctx::kPerturbTableBytes));
    const int k = c->perturb_next;
    c->perturb_next = (k + 1) % lf_device_ctx::kPerturbSlots;
    if (!c->perturb_read[k]) LF_HIP(hipEventCreateWithFlags(&c->perturb_read[k], hipEventDisableTiming));
    if (c->perturb_read_valid[k]) LF_HIP(hipStreamWaitEvent(s, c->perturb_read[k], 0));
    double *coeff = (double *)((char *)c->perturb_tables + (size_t)k * lf_device_ctx::kPerturbTableBytes);
    LF_TRY(lf_staged_h2d(c, s, coeff, coeff_host, (size_t)members * (size_t)rank * sizeof(double)));
    const perturb_args A = {(long long)stride, (long long)n, (long long)pattern_stride, members, multiplicative, lower, upper};
#define LF_PERTURB_RANK(R) \
    case R: launch_perturb<R>(s, rows_dev, base_dev, patterns_dev, coeff, lower_dev, upper_dev, A); break;
    switch (rank) {
        LF_PERTURB_RANK(1) LF_PERTURB_RANK(2) LF_PERTURB_RANK(3) LF_PERTURB_RANK(4) LF_PERTURB_RANK(5) LF_PERTURB_RANK(6)
        LF_PERTURB_RANK(7) LF_PERTURB_RANK(8) LF_PERTURB_RANK(9) LF_PERTURB_RANK(10) LF_PERTURB_RANK(11) LF_PERTURB_RANK(12)
        LF_PERTURB_RANK(13) LF_PERTURB_RANK(14) LF_PERTURB_RANK(15)
    default: launch_perturb<16>(s, rows_dev, base_dev, patterns_dev, coeff, lower_dev, upper_dev, A); break;
    }
#undef LF_PERTURB_RANK
    LF_HIP(hipGetLastError());
    LF_HIP(hipEventRecord(c->perturb_read[k], s));
    c->perturb_read_valid[k] = true;
    return LF_OK;
}

// what the two in-place calls refuse in common
int check_inplace_rows(const double *rows_dev, int members, int cap, const char *what, int64_t stride, int64_t n)
{
    if (!rows_dev) return lf_set_error(LF_E_INVALID, "rows_dev is NULL");
    if (members < 1) return lf_set_error(LF_E_INVALID, "members must be at least 1 (got %d)", members);
    if (members > cap) return lf_set_error(LF_E_INVALID, "members = %d: %s takes at most %d members", members, what, cap);
    if (n < 0 || n > 0x7fffffffll) return lf_set_error(LF_E_INVALID, "n = %lld outside the 32-bit range of a launch", (long long)n);
    if (members > 1 && stride < n) return lf_set_error(LF_E_INVALID, "stride %lld is less than n = %lld", (long long)stride, (long long)n);
    return LF_OK;
}

template <int W>
void launch_transform(hipStream_t s, double *rows, const double *weights, const double *taper, const double *lower_dev,
                      const double *upper_dev, const transform_args &A)
{
    const dim3 grid((unsigned)((A.n + W - 1) / W)), block(W);
    hipLaunchKernelGGL((k_members_transform<W>), grid, block, (size_t)A.members * W * sizeof(double), s, rows, weights, taper,
                       lower_dev, upper_dev, A);
}

template <int W>
void launch_resample(hipStream_t s, double *rows, long long stride, long long n, const resample_plan &P)
{
    const dim3 grid((unsigned)((n + W - 1) / W)), block(W);
    hipLaunchKernelGGL((k_members_resample<W>), grid, block, (size_t)P.n_src * W * sizeof(double), s, rows, stride, n, P);
}

// what both entry points refuse, in the order the header lists it (no device is touched)
int check_rows(const double *rows_dev, int members, int64_t stride, int64_t n, const int32_t *dst_index_dev, int64_t dst_n)
{
    if (members < 1) return lf_set_error(LF_E_INVALID, "members must be at least 1 (got %d)", members);
    if (n < 0 || n > 0x7fffffffll) return lf_set_error(LF_E_INVALID, "n = %lld outside the 32-bit range of a launch", (long long)n);
    if (stride < n) return lf_set_error(LF_E_INVALID, "stride %lld is less than n = %lld", (long long)stride, (long long)n);
    if (!dst_index_dev && dst_n != n)
        return lf_set_error(LF_E_INVALID, "dst_n %lld must be n = %lld without a dst_index", (long long)dst_n, (long long)n);
    if (dst_n < n) return lf_set_error(LF_E_INVALID, "dst_n %lld is less than n = %lld", (long long)dst_n, (long long)n);
    if (n > 0 && !rows_dev) return lf_set_error(LF_E_INVALID, "rows_dev is NULL");
    return LF_OK;
}

template <int NT>
void launch_summary(hipStream_t s, const members_rows &R, const summary_out &O)
{
    const dim3 grid((unsigned)((R.n + kSummaryLanes - 1) / kSummaryLanes)), block(kSummaryLanes);
    if (R.divisor == 1.0)
        hipLaunchKernelGGL((k_members_summary<NT, false>), grid, block, 0, s, R, O);
    else
        hipLaunchKernelGGL((k_members_summary<NT, true>), grid, block, 0, s, R, O);
}

template <int NT>
void launch_track(hipStream_t s, const members_rows &R, const track_out &O, bool first)
{
    const dim3 grid((unsigned)((R.n + kSummaryLanes - 1) / kSummaryLanes)), block(kSummaryLanes);
    if (R.divisor == 1.0) {
        if (first)
            hipLaunchKernelGGL((k_members_track<NT, false, true>), grid, block, 0, s, R, O);
        else
            hipLaunchKernelGGL((k_members_track<NT, false, false>), grid, block, 0, s, R, O);
    } else {
        if (first)
            hipLaunchKernelGGL((k_members_track<NT, true, true>), grid, block, 0, s, R, O);
        else
            hipLaunchKernelGGL((k_members_track<NT, true, false>), grid, block, 0, s, R, O);
    }
}

template <int W>
void launch_order(hipStream_t s, const members_rows &R, const order_out &O)
{
    const dim3 grid((unsigned)((R.n + W - 1) / W)), block(W);
    const size_t lds = (size_t)R.members * W * sizeof(double);
    if (R.divisor == 1.0)
        hipLaunchKernelGGL((k_members_order<W, false>), grid, block, lds, s, R, O);
    else
        hipLaunchKernelGGL((k_members_order<W, true>), grid, block, lds, s, R, O);
}

} // namespace

int lf_members_summary_device(int device, const double *rows_dev, int members, int64_t stride, int64_t n, double divisor,
                              const int32_t *dst_index_dev, int64_t dst_n, double *mean_dev, double *min_dev, double *max_dev,
                              int n_thresholds, const double *thresholds_dev, int64_t threshold_stride, int32_t *exceed_dev)
{
    LF_TRY(check_rows(rows_dev, members, stride, n, dst_index_dev, dst_n));
    if (n_thresholds < 0 || n_thresholds > kMaxThresholds)
        return lf_set_error(LF_E_INVALID, "n_thresholds must be 0 to %d (got %d)", kMaxThresholds, n_thresholds);
    if (n_thresholds > 0 && !thresholds_dev) return lf_set_error(LF_E_INVALID, "thresholds_dev is NULL with n_thresholds = %d", n_thresholds);
    if (n_thresholds > 0 && !exceed_dev) return lf_set_error(LF_E_INVALID, "exceed_dev is NULL with n_thresholds = %d", n_thresholds);
    if (n_thresholds > 0 && threshold_stride < n)
        return lf_set_error(LF_E_INVALID, "threshold_stride %lld is less than n = %lld", (long long)threshold_stride, (long long)n);
    if (!mean_dev && !min_dev && !max_dev && n_thresholds == 0)
        return lf_set_error(LF_E_INVALID, "no output requested: mean_dev, min_dev and max_dev are NULL and n_thresholds is 0");
    if (n == 0) return LF_OK;
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    const members_rows R = {rows_dev, (long long)stride, (long long)n, (long long)dst_n, members, divisor, (const int *)dst_index_dev};
    const summary_out O = {mean_dev, min_dev, max_dev, thresholds_dev, (long long)threshold_stride, (int *)exceed_dev};
    switch (n_thresholds) {
    case 0: launch_summary<0>(c->stream, R, O); break;
    case 1: launch_summary<1>(c->stream, R, O); break;
    case 2: launch_summary<2>(c->stream, R, O); break;
    case 3: launch_summary<3>(c->stream, R, O); break;
    default: launch_summary<4>(c->stream, R, O); break;
    }
    LF_HIP(hipGetLastError());
    return LF_OK;
}

int lf_members_track_device(int device, const double *rows_dev, int members, int64_t stride, int64_t n, double divisor, int step,
                            int first, int64_t track_stride, double *peak_dev, int32_t *peak_step_dev, double *sum_dev,
                            int n_thresholds, const double *thresholds_dev, int64_t threshold_stride, int32_t *first_above_dev,
                            int32_t *steps_above_dev)
{
    LF_TRY(check_rows(rows_dev, members, stride, n, nullptr, n));
    if (track_stride < n)
        return lf_set_error(LF_E_INVALID, "track_stride %lld is less than n = %lld", (long long)track_stride, (long long)n);
    if (step < 0) return lf_set_error(LF_E_INVALID, "step must be at least 0 (got %d): -1 is the mark of never", step);
    if (n_thresholds < 0 || n_thresholds > kMaxThresholds)
        return lf_set_error(LF_E_INVALID, "n_thresholds must be 0 to %d (got %d)", kMaxThresholds, n_thresholds);
    if (n_thresholds > 0 && !thresholds_dev) return lf_set_error(LF_E_INVALID, "thresholds_dev is NULL with n_thresholds = %d", n_thresholds);
    if (n_thresholds > 0 && threshold_stride < n)
        return lf_set_error(LF_E_INVALID, "threshold_stride %lld is less than n = %lld", (long long)threshold_stride, (long long)n);
    if (n_thresholds > 0 && !first_above_dev && !steps_above_dev)
        return lf_set_error(LF_E_INVALID, "first_above_dev and steps_above_dev are both NULL with n_thresholds = %d", n_thresholds);
    if (peak_step_dev && !peak_dev) return lf_set_error(LF_E_INVALID, "peak_step_dev without peak_dev: the peak decides when it changes");
    if (!peak_dev && !sum_dev && n_thresholds == 0)
        return lf_set_error(LF_E_INVALID, "no output requested: peak_dev and sum_dev are NULL and n_thresholds is 0");
    if (n == 0) return LF_OK;
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    const members_rows R = {rows_dev, (long long)stride, (long long)n, (long long)n, members, divisor, nullptr};
    const track_out O = {peak_dev, (int *)peak_step_dev, sum_dev, thresholds_dev, (long long)threshold_stride,
                         (int *)first_above_dev, (int *)steps_above_dev, (long long)track_stride, step};
    switch (n_thresholds) {
    case 0: launch_track<0>(c->stream, R, O, first != 0); break;
    case 1: launch_track<1>(c->stream, R, O, first != 0); break;
    case 2: launch_track<2>(c->stream, R, O, first != 0); break;
    case 3: launch_track<3>(c->stream, R, O, first != 0); break;
    default: launch_track<4>(c->stream, R, O, first != 0); break;
    }
    LF_HIP(hipGetLastError());
    return LF_OK;
}

int lf_members_order_statistics_device(int device, const double *rows_dev, int members, int64_t stride, int64_t n, double divisor,
                                       const int32_t *dst_index_dev, int64_t dst_n, int n_ranks, const int32_t *ranks_host,
                                       double *out_dev)
{
    LF_TRY(check_rows(rows_dev, members, stride, n, dst_index_dev, dst_n));
    if (n_ranks < 1 || n_ranks > kMaxRanks) return lf_set_error(LF_E_INVALID, "n_ranks must be 1 to %d (got %d)", kMaxRanks, n_ranks);
    if (!ranks_host) return lf_set_error(LF_E_INVALID, "ranks_host is NULL");
    order_out O = {};
    O.n_ranks = n_ranks;
    O.out = out_dev;
    for (int r = 0; r < n_ranks; ++r) {
        if (ranks_host[r] < 0 || ranks_host[r] >= members)
            return lf_set_error(LF_E_INVALID, "rank %d (ranks_host[%d]) outside 0 .. members - 1 = %d", (int)ranks_host[r], r, members - 1);
        O.ranks[r] = ranks_host[r];
    }
    if (members > kMaxOrderMembers)
        return lf_set_error(LF_E_INVALID, "members = %d: order statistics take at most %d members", members, kMaxOrderMembers);
    if (n > 0 && !out_dev) return lf_set_error(LF_E_INVALID, "out_dev is NULL");
    if (n == 0) return LF_OK;
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    const members_rows R = {rows_dev, (long long)stride, (long long)n, (long long)dst_n, members, divisor, (const int *)dst_index_dev};
    // the widest workgroup whose [members][W] tile fits: 256 lanes up to 32 members, 128 up to 64, 64 up to 128
    if ((size_t)members * 256 * sizeof(double) <= kOrderTileBytes)
        launch_order<256>(c->stream, R, O);
    else if ((size_t)members * 128 * sizeof(double) <= kOrderTileBytes)
        launch_order<128>(c->stream, R, O);
    else
        launch_order<64>(c->stream, R, O);
    LF_HIP(hipGetLastError());
    return LF_OK;
}

int lf_members_transform_device(int device, double *rows_dev, int members, int64_t stride, int64_t n, const double *weights_dev,
                                const double *taper_dev, const double *lower_dev, double lower, const double *upper_dev, double upper)
{
    LF_TRY(check_inplace_rows(rows_dev, members, kMaxTransformMembers, "the transform (a 32 KiB weight table)", stride, n));
    if (!weights_dev) return lf_set_error(LF_E_INVALID, "weights_dev is NULL");
    if (!lower_dev && !upper_dev && lower > upper)
        return lf_set_error(LF_E_INVALID, "lower = %g is greater than upper = %g", lower, upper);
    if (n == 0) return LF_OK;
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    const transform_args A = {(long long)stride, (long long)n, members, lower, upper};
    // the widest workgroup whose [members][W] tile fits: 256 lanes up to 32 members, 128 up to 64
    if ((size_t)members * 256 * sizeof(double) <= kOrderTileBytes)
        launch_transform<256>(c->stream, rows_dev, weights_dev, taper_dev, lower_dev, upper_dev, A);
    else
        launch_transform<128>(c->stream, rows_dev, weights_dev, taper_dev, lower_dev, upper_dev, A);
    LF_HIP(hipGetLastError());
    return LF_OK;
}

int lf_members_regress_device(int device, double *rows_dev, int members, int64_t stride, int64_t n, int gauges, const double *cx_dev,
                              const double *cy_dev, const double *table_dev, const double *lower_dev, double lower,
                              const double *upper_dev, double upper)
{
    if (members < 2 || members > kMaxTransformMembers)
        return lf_set_error(LF_E_INVALID, "members must be 2 to %d (got %d): the regression needs a spread and a column in LDS",
                            kMaxTransformMembers, members);
    if (gauges < 1 || gauges > kMaxRegressGauges)
        return lf_set_error(LF_E_INVALID, "gauges must be 1 to %d (got %d)", kMaxRegressGauges, gauges);
    if (n < 0 || n > 0x7fffffffll) return lf_set_error(LF_E_INVALID, "n = %lld outside the 32-bit range of a launch", (long long)n);
    if (stride < n) return lf_set_error(LF_E_INVALID, "stride %lld is less than n = %lld", (long long)stride, (long long)n);
    if (n > 0 && !rows_dev) return lf_set_error(LF_E_INVALID, "rows_dev is NULL");
    if (n > 0 && !cx_dev) return lf_set_error(LF_E_INVALID, "cx_dev is NULL");
    if (n > 0 && !cy_dev) return lf_set_error(LF_E_INVALID, "cy_dev is NULL");
    if (n > 0 && !table_dev) return lf_set_error(LF_E_INVALID, "table_dev is NULL");
    if (!lower_dev && !upper_dev && lower > upper)
        return lf_set_error(LF_E_INVALID, "lower = %g is greater than upper = %g", lower, upper);
    if (n == 0) return LF_OK;
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    // (bounds of -inf / +inf take nothing from any value: such a call stores only the columns a gauge touched)
    const int bounded = lower_dev || upper_dev || !(lower == -HUGE_VAL) || !(upper == HUGE_VAL);
    const regress_args A = {(long long)stride, (long long)n, members, gauges, bounded, lower, upper};
    // up to 16 members the column stays in registers (one kernel per member count); beyond, in LDS at the transform's
    // widths: 256 lanes up to 32 members, 128 up to 64 -- a tile of 64 KiB at most, two workgroups per CU
    if (members <= kMaxRegressRegisterMembers) {
#define LF_REGRESS_REG(M) \
    case M: launch_regress_reg<M>(c->stream, rows_dev, cx_dev, cy_dev, table_dev, lower_dev, upper_dev, A); break;
        switch (members) {
            LF_REGRESS_REG(2) LF_REGRESS_REG(3) LF_REGRESS_REG(4) LF_REGRESS_REG(5) LF_REGRESS_REG(6) LF_REGRESS_REG(7)
            LF_REGRESS_REG(8) LF_REGRESS_REG(9) LF_REGRESS_REG(10) LF_REGRESS_REG(11) LF_REGRESS_REG(12) LF_REGRESS_REG(13)
            LF_REGRESS_REG(14) LF_REGRESS_REG(15) LF_REGRESS_REG(16)
        }
#undef LF_REGRESS_REG
    } else if ((size_t)members * 256 * sizeof(double) <= kOrderTileBytes)
        launch_regress<256>(c->stream, rows_dev, cx_dev, cy_dev, table_dev, lower_dev, upper_dev, A);
    else
        launch_regress<128>(c->stream, rows_dev, cx_dev, cy_dev, table_dev, lower_dev, upper_dev, A);
    LF_HIP(hipGetLastError());
    return LF_OK;
}

int lf_members_zonal_device(int device, const double *rows_dev, int members, int64_t stride, double divisor, int64_t entries,
                            const int32_t *index_dev, const double *weights_dev, int64_t runs, const int32_t *run_start_dev,
                            double *out_dev, int64_t out_stride)
{
    if (members < 1) return lf_set_error(LF_E_INVALID, "members must be at least 1 (got %d)", members);
    if (entries < 0 || entries > 0x7fffffffll)
        return lf_set_error(LF_E_INVALID, "entries = %lld outside the 32-bit range of a launch", (long long)entries);
    if (runs < 0 || runs > 0x7fffffffll)
        return lf_set_error(LF_E_INVALID, "runs = %lld outside the 32-bit range of a launch", (long long)runs);
    if (runs > 0 && !run_start_dev) return lf_set_error(LF_E_INVALID, "run_start_dev is NULL with runs = %lld", (long long)runs);
    if (runs > 0 && !out_dev) return lf_set_error(LF_E_INVALID, "out_dev is NULL with runs = %lld", (long long)runs);
    if (out_stride < runs)
        return lf_set_error(LF_E_INVALID, "out_stride %lld is less than runs = %lld", (long long)out_stride, (long long)runs);
    if (entries > 0 && !rows_dev) return lf_set_error(LF_E_INVALID, "rows_dev is NULL with entries = %lld", (long long)entries);
    if (divisor == 0.0 || divisor != divisor) return lf_set_error(LF_E_INVALID, "divisor must be neither 0 nor a NaN (got %g)", divisor);
    if (runs == 0) return LF_OK;
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    // Few runs leave most of the device idle while each wavefront walks every member: the members then go on the grid's
    // second dimension, kZonalMembers per workgroup (LF_ZONAL_GRID=0 / 1 in the environment: never / always; A/B switch).
    // Which wavefront computes a (member, run) does not enter its arithmetic.
    const long long blocks = (runs + kZonalWaves - 1) / kZonalWaves;
    const char *e = std::getenv("LF_ZONAL_GRID");
    const bool split = e && (e[0] == '0' || e[0] == '1') ? e[0] == '1' : blocks < kZonalFewBlocks;
    int per_block = members;
    if (split && members > kZonalMembers && (members + kZonalMembers - 1) / kZonalMembers <= 65535) per_block = kZonalMembers;
    const zonal_args A = {rows_dev, (long long)stride, divisor, (const int *)index_dev, weights_dev, (long long)runs,
                          (const int *)run_start_dev, out_dev, (long long)out_stride, members, per_block};
    const dim3 grid((unsigned)blocks, (unsigned)((members + per_block - 1) / per_block));
    if (divisor == 1.0)
        launch_zonal<false>(c->stream, A, grid);
    else
        launch_zonal<true>(c->stream, A, grid);
    LF_HIP(hipGetLastError());
    return LF_OK;
}

int lf_members_resample_device(int device, double *rows_dev, int members, int64_t stride, int64_t n, const int32_t *parents_host)
{
    LF_TRY(check_inplace_rows(rows_dev, members, kMaxResampleMembers, "resampling", stride, n));
    if (!parents_host) return lf_set_error(LF_E_INVALID, "parents_host is NULL");
    resample_plan P = {};
    int slot_of[kMaxResampleMembers];
    for (int m = 0; m < members; ++m) slot_of[m] = -1;
    for (int m = 0; m < members; ++m) {
        const int parent = parents_host[m];
        if (parent < 0 || parent >= members)
            return lf_set_error(LF_E_INVALID, "parent %d (parents_host[%d]) outside 0 .. members - 1 = %d", parent, m, members - 1);
        if (parent == m) continue;
        if (slot_of[parent] < 0) {
            slot_of[parent] = P.n_src;
            P.src[P.n_src++] = (unsigned char)parent;
        }
        P.dst[P.n_dst] = (unsigned char)m;
        P.slot[P.n_dst++] = (unsigned char)slot_of[parent];
    }
    if (n == 0 || P.n_dst == 0) return LF_OK;      // (the identity: nothing is launched)
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    if ((size_t)P.n_src * 256 * sizeof(double) <= kOrderTileBytes)
        launch_resample<256>(c->stream, rows_dev, (long long)stride, (long long)n, P);
    else if ((size_t)P.n_src * 128 * sizeof(double) <= kOrderTileBytes)
        launch_resample<128>(c->stream, rows_dev, (long long)stride, (long long)n, P);
    else
        launch_resample<64>(c->stream, rows_dev, (long long)stride, (long long)n, P);
    LF_HIP(hipGetLastError());
    return LF_OK;
}

int lf_members_perturb_device(int device, double *rows_dev, int members, int64_t stride, int64_t n, const double *base_dev, int rank,
                              const double *patterns_dev, int64_t pattern_stride, const double *coeff_host, int multiplicative,
                              const double *lower_dev, double lower, const double *upper_dev, double upper)
{
    LF_TRY(check_perturb(rows_dev, members, stride, n, rank, patterns_dev, pattern_stride, coeff_host, multiplicative, lower_dev,
                         lower, upper_dev, upper));
    if (n == 0) return LF_OK;
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    return enqueue_perturb(c, c->stream, rows_dev, members, stride, n, base_dev, rank, patterns_dev, pattern_stride, coeff_host,
                           multiplicative, lower_dev, lower, upper_dev, upper);
}

int lf_upload_perturb_rows(int device, double *rows_dev, int members, int64_t stride, int64_t n, const double *base_dev, int rank,
                           const double *patterns_dev, int64_t pattern_stride, const double *coeff_host, int multiplicative,
                           const double *lower_dev, double lower, const double *upper_dev, double upper)
{
    LF_TRY(check_perturb(rows_dev, members, stride, n, rank, patterns_dev, pattern_stride, coeff_host, multiplicative, lower_dev,
                         lower, upper_dev, upper));
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    if (c->upload_open < 0 || !c->copy_stream)
        return lf_set_error(LF_E_INVALID, "lf_upload_perturb_rows outside lf_upload_begin(set) .. lf_upload_end(set)");
    if (n == 0) return LF_OK;
    return enqueue_perturb(c, c->copy_stream, rows_dev, members, stride, n, base_dev, rank, patterns_dev, pattern_stride, coeff_host,
                           multiplicative, lower_dev, lower, upper_dev, upper);
}
