// lf_meteo.hip -- the front of the model step: snow.dynamic followed by frost.dynamic (three elevation zones), which turn
// what a forecast delivers -- precipitation and average temperature -- into the Rain, SnowMelt and isFrozenSoil the land
// surface starts from, and carry the snow pack of the zones (SnowCoverS) and the frost index from one step to the next.
//
//   k_snow_frost<SNOW, FROST> : one kernel for a single run and an ensemble, both halves or either one
//
// A lane owns a pixel and walks the members of its slice (blockIdx.y: up to kMemberSlice members, as k_upload_rows and
// k_members_track have it): the three statics of the pixel and the scalars are read once per lane and serve every member,
// a member's six loads go out together, and the next member's go out before this member's stores.  Every double store is a
// full line of consecutive pixels; the byte row of isFrozenSoil is the one store narrower than that (64 B per wavefront).
// No LDS, no atomics.  The arithmetic is include/lisflood_amd.h's text, one IEEE operation per sign in the order written
// (-ffp-contract=off); exp is OCML's.
#include <cmath>

#include "lf_common.h"
#include "lf_structures.h" // lf_npmin / lf_npmax

namespace {

constexpr int kLanes = 256;
constexpr int kMemberSlice = 8;
constexpr int kMaxGridY = 65535;
static_assert(sizeof(lf_snow_frost_args) == 22 * 8, "12 pointers, 9 doubles, N: lisflood_amd.snow_frost._SnowFrostArgs mirrors it");

struct meteo_members {
    long long zone_stride, row_stride, forcing_stride;
    int members;
};

// what one (member, pixel) reads: SNOW: precipitation and the three zones; FROST: the frost index and, without the snow
// half, the snow cover; both: the temperature
struct meteo_in {
    double precipitation, tavg, zone[3], frost, cover;
};

template <bool SNOW, bool FROST>
__device__ __forceinline__ meteo_in meteo_load(const lf_snow_frost_args &A, const meteo_members &M, long long m, long long i)
{
    meteo_in x = {};
    x.tavg = A.Tavg[m * M.forcing_stride + i];
    if (SNOW) {
        x.precipitation = A.Precipitation[m * M.forcing_stride + i];
        const double *z = A.SnowCoverS + m * M.zone_stride + i;
#pragma unroll
        for (int k = 0; k < 3; ++k) x.zone[k] = z[(long long)k * A.N];
    }
    if (FROST) {
        x.frost = A.FrostIndex[m * M.row_stride + i];
        if (!SNOW) x.cover = A.SnowCover[m * M.row_stride + i];
    }
    return x;
}

template <bool SNOW, bool FROST>
__global__ void __launch_bounds__(kLanes) k_snow_frost(lf_snow_frost_args A, meteo_members M)
{
    const long long i = (long long)blockIdx.x * kLanes + threadIdx.x;
    if (i >= A.N) return;
    const long long m0 = (long long)blockIdx.y * kMemberSlice;
    const int count = min(M.members - (int)m0, kMemberSlice); // (the same for every lane of the slice)
    double delta = 0., seas = 0., factor = 0.;
    if (SNOW) {
        delta = A.DeltaTSnow[i];
        seas = A.SnowSeasonTerm + A.SnowMeltCoef[i];
        factor = A.SnowFactor[i];
    }
    meteo_in x = meteo_load<SNOW, FROST>(A, M, m0, i);
    for (int k = 0; k < count; ++k) {
        const long long m = m0 + k;
        meteo_in next = {};
        if (k + 1 < count) next = meteo_load<SNOW, FROST>(A, M, m + 1, i);
        const long long row = m * M.row_stride + i;
        double cover = x.cover;
        if (SNOW) {
            double snow = 0., rain = 0., melt = 0.;
            double *z = A.SnowCoverS + m * M.zone_stride + i;
            cover = 0.;
#pragma unroll
            for (int zone = 0; zone < 3; ++zone) { // 0: the highest
                const double tavg_s = x.tavg + delta * (double)(zone - 1);
                const double snow_s = tavg_s < A.TempSnow ? factor * x.precipitation : 0.;
                const double rain_s = tavg_s >= A.TempSnow ? x.precipitation : 0.;
                double melt_s = lf_npmax((tavg_s - A.TempMelt) * seas * (1. + 0.01 * rain_s) * A.DtDay, 0.);
                const double ice_s = lf_npmax((zone < 2 ? x.tavg : tavg_s) * A.IceMeltCoef * A.DtDay * A.SummerSeason, 0.);
                melt_s = lf_npmax(lf_npmin(melt_s + ice_s, x.zone[zone]), 0.);
                const double pack = x.zone[zone] + snow_s - melt_s;
                z[(long long)zone * A.N] = pack;
                snow = snow + snow_s;
                rain = rain + rain_s;
                melt = melt + melt_s;
                cover = cover + pack;
            }
            cover = cover / 3.;
            A.Rain[row] = rain / 3.;
            A.SnowMelt[row] = melt / 3.;
            if (A.Snow) A.Snow[row] = snow / 3.;
            A.SnowCover[row] = cover;
        }
        if (FROST) {
            const double kfrost = x.tavg < 0. ? 0.08 : 0.5;
            const double rate = -(1. - A.Afrost) * x.frost - x.tavg * exp(-0.04 * kfrost * cover / A.SnowWaterEquivalent);
            const double frost = lf_npmax(x.frost + rate * A.DtDay, 0.);
            A.FrostIndex[row] = frost;
            A.isFrozenSoil[row] = frost > A.FrostIndexThreshold ? 1 : 0; // (row_stride counts bytes here)
        }
        x = next;
    }
}

// rows of `len` elements `stride` apart, `members` of them: [p, p + span)
struct span {
    const char *lo, *hi;
};
span span_of(const void *p, int members, int64_t stride, int64_t len, size_t elem)
{
    const char *b = (const char *)p;
    return {b, b + ((int64_t)(members - 1) * stride + len) * (int64_t)elem};
}
bool overlap(const span &a, const span &b) { return a.lo < b.hi && b.lo < a.hi; }

} // namespace

int lf_snow_frost_members_device(int device, const lf_snow_frost_args *a, int members, int64_t zone_stride, int64_t row_stride,
                                 int64_t forcing_stride)
{
    if (!a) return lf_set_error(LF_E_INVALID, "snow / frost: null argument");
    const int64_t N = a->N;
    if (N < 0 || N > 0x7fffffffll)
        return lf_set_error(LF_E_INVALID, "snow / frost: N = %lld outside the 32-bit range of a launch", (long long)N);
    if (members < 1) return lf_set_error(LF_E_INVALID, "snow / frost: members must be at least 1 (got %d)", members);
    const bool snow = a->SnowCoverS != nullptr, frost = a->FrostIndex != nullptr;
    if (!snow && !frost) return lf_set_error(LF_E_INVALID, "snow / frost: SnowCoverS and FrostIndex are both NULL: nothing to do");
    if (!a->Tavg) return lf_set_error(LF_E_INVALID, "snow / frost: Tavg is NULL");
    if (!a->SnowCover) return lf_set_error(LF_E_INVALID, "snow / frost: SnowCover is NULL (the snow half's output, the frost half's input)");
    if (snow && (!a->Precipitation || !a->Rain || !a->SnowMelt || !a->DeltaTSnow || !a->SnowMeltCoef || !a->SnowFactor))
        return lf_set_error(LF_E_INVALID, "snow / frost: the snow half needs Precipitation, Rain, SnowMelt, DeltaTSnow, SnowMeltCoef "
                                          "and SnowFactor");
    if (!snow && (a->Precipitation || a->Rain || a->SnowMelt || a->Snow))
        return lf_set_error(LF_E_INVALID, "snow / frost: SnowCoverS is NULL (frost only) but Precipitation or a snow output is not");
    if (frost && !a->isFrozenSoil) return lf_set_error(LF_E_INVALID, "snow / frost: isFrozenSoil is NULL with a FrostIndex");
    if (!frost && a->isFrozenSoil) return lf_set_error(LF_E_INVALID, "snow / frost: FrostIndex is NULL (snow only) but isFrozenSoil is not");
    if (snow && zone_stride < 3 * N)
        return lf_set_error(LF_E_INVALID, "snow / frost: zone_stride %lld is less than 3 * N = %lld", (long long)zone_stride, (long long)(3 * N));
    if (row_stride < N)
        return lf_set_error(LF_E_INVALID, "snow / frost: row_stride %lld is less than N = %lld", (long long)row_stride, (long long)N);
    if (forcing_stride != 0 && forcing_stride < N)
        return lf_set_error(LF_E_INVALID, "snow / frost: forcing_stride %lld is neither 0 (one row for all) nor at least N = %lld",
                            (long long)forcing_stride, (long long)N);
    {
        // no two vectors of the call may share an element: inputs against outputs and outputs against each other
        struct named {
            const char *name;
            span s;
            bool out;
        } v[16];
        int nv = 0;
        auto add = [&](const char *name, const void *p, int rows, int64_t stride, int64_t len, size_t elem, bool out) {
            if (p) v[nv++] = {name, span_of(p, rows, stride, len, elem), out};
        };
        const int frows = forcing_stride ? members : 1;
        add("Precipitation", a->Precipitation, frows, forcing_stride, N, 8, false);
        add("Tavg", a->Tavg, frows, forcing_stride, N, 8, false);
        add("DeltaTSnow", a->DeltaTSnow, 1, 0, N, 8, false);
        add("SnowMeltCoef", a->SnowMeltCoef, 1, 0, N, 8, false);
        add("SnowFactor", a->SnowFactor, 1, 0, N, 8, false);
        add("SnowCoverS", a->SnowCoverS, members, zone_stride, 3 * N, 8, true);
        add("FrostIndex", a->FrostIndex, members, row_stride, N, 8, true);
        add("Rain", a->Rain, members, row_stride, N, 8, true);
        add("SnowMelt", a->SnowMelt, members, row_stride, N, 8, true);
        add("Snow", a->Snow, members, row_stride, N, 8, true);
        add("SnowCover", a->SnowCover, members, row_stride, N, 8, snow);
        add("isFrozenSoil", a->isFrozenSoil, members, row_stride, N, 1, true);
        for (int p = 0; p < nv; ++p)
            for (int q = p + 1; q < nv; ++q)
                if ((v[p].out || v[q].out) && N > 0 && overlap(v[p].s, v[q].s))
                    return lf_set_error(LF_E_INVALID, "snow / frost: %s and %s overlap", v[p].name, v[q].name);
    }
    if (N == 0) return LF_OK;
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    const int slices = (members + kMemberSlice - 1) / kMemberSlice;
    for (int s0 = 0; s0 < slices; s0 += kMaxGridY) { // (one launch unless there are more slices than a grid has)
        const int m0 = s0 * kMemberSlice, mm = std::min(members - m0, kMaxGridY * kMemberSlice);
        lf_snow_frost_args A = *a;
        if (A.Precipitation) A.Precipitation += (int64_t)m0 * forcing_stride;
        A.Tavg += (int64_t)m0 * forcing_stride;
        if (A.SnowCoverS) A.SnowCoverS += (int64_t)m0 * zone_stride;
        if (A.FrostIndex) A.FrostIndex += (int64_t)m0 * row_stride;
        if (A.Rain) A.Rain += (int64_t)m0 * row_stride;
        if (A.SnowMelt) A.SnowMelt += (int64_t)m0 * row_stride;
        if (A.Snow) A.Snow += (int64_t)m0 * row_stride;
        A.SnowCover += (int64_t)m0 * row_stride;
        if (A.isFrozenSoil) A.isFrozenSoil += (int64_t)m0 * row_stride;
        const meteo_members M = {(long long)zone_stride, (long long)row_stride, (long long)forcing_stride, mm};
        const dim3 grid((unsigned)((N + kLanes - 1) / kLanes), (unsigned)std::min(slices - s0, kMaxGridY)), block(kLanes);
        if (snow && frost)
            hipLaunchKernelGGL((k_snow_frost<true, true>), grid, block, 0, c->stream, A, M);
        else if (snow)
            hipLaunchKernelGGL((k_snow_frost<true, false>), grid, block, 0, c->stream, A, M);
        else
            hipLaunchKernelGGL((k_snow_frost<false, true>), grid, block, 0, c->stream, A, M);
    }
    LF_HIP(hipGetLastError());
    return LF_OK;
}
