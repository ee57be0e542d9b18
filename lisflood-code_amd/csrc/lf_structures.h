// lf_structures.h -- lakes and reservoirs of the routing loop, one lane per site; shared by the sub-step-by-sub-step
// path (lf_modules.hip: k_inloop_sites) and the fused sub-step wavefront (lf_fused.h: k_sites_wave, k_sites_blocks and the
// site lanes of k_fused_level_steps).
#pragma once
#include "lf_common.h"

// np.minimum / np.maximum: NaN propagates, first argument first
__device__ __forceinline__ double lf_npmin(double a, double b) { return (a != a) ? a : ((b != b) ? b : (b < a ? b : a)); }
__device__ __forceinline__ double lf_npmax(double a, double b) { return (a != a) ? a : ((b != b) ? b : (b > a ? b : a)); }

// lakes.dynamic_inloop (lakes.py:215-258) for lake i (i < n_lakes) or reservoir.dynamic_inloop (reservoir.py:190-296)
// for reservoir i - n_lakes: inflow = np.bincount(downstruct, weights=ChanQ)[site] in ascending source id, then the
// site's storage / outflow update; the outflow volume goes to the dense QLakeOutM3Dt / QResOutM3Dt at the site cell.
// The gather (lf_site_inflow) and the update (lf_site_body) are apart because the time-major fused form
// (lf_fused.h: k_fused_level_steps<.., 2>) takes the inflow from its feed buffer instead of ChanQ.
__device__ __forceinline__ double lf_site_inflow(const lf_inloop_args &A, long long i)
{
    double inflow = 0.0; // np.bincount(downstruct, weights=ChanQ)[LakeIndex / ReservoirIndex]: ascending source id
    if (i < A.n_lakes) {
        for (int e = A.lake_ups_ptr[i]; e < A.lake_ups_ptr[i + 1]; ++e) inflow += A.ChanQ[A.lake_ups_idx[e]];
    } else if (i - A.n_lakes < A.n_res) {
        const long long r = i - A.n_lakes;
        for (int e = A.res_ups_ptr[r]; e < A.res_ups_ptr[r + 1]; ++e) inflow += A.ChanQ[A.res_ups_idx[e]];
    }
    return inflow;
}

__device__ __forceinline__ void lf_site_body(const lf_inloop_args &A, long long i, const double inflow)
{
    if (i < A.n_lakes) {
        A.LakeInflowCC[i] = inflow;
        const double lake_in = (inflow + A.LakeInflowOldCC[i]) * 0.5;
        A.LakeInflowOldCC[i] = inflow;
        const double si = A.LakeStorageM3CC[i] / A.DtRouting - 0.5 * A.LakeOutflowCC[i] + lake_in;
        const double y = -A.LakeFactor[i] + sqrt(A.LakeFactorSqr[i] + 2 * si);
        const double out = y * y; // np.square
        A.LakeOutflowCC[i] = out;
        const double out_m3 = out * A.DtRouting;
        double st = (si - out * 0.5) * A.DtRouting;
        if (st < 0 || st != st) st = 0; // lakes.py:250-255
        A.LakeStorageM3CC[i] = st;
        A.LakeStorageM3BalanceCC[i] += lake_in * A.DtRouting - out_m3;
        A.LakeLevelCC[i] = st / A.LakeAreaCC[i];
        A.QLakeOutM3Dt[A.lake_cell[i]] = out_m3;
    }
    const long long r = i - A.n_lakes;
    if (r >= 0 && r < A.n_res) {
        const double inv_day = 1 / 86400.0; // 1 / float(86400)
        A.ReservoirInflowCC[r] = inflow;
        const double tot = A.TotalReservoirStorageM3CC[r];
        double st = A.ReservoirStorageM3CC[r] + inflow * A.DtRouting;
        const double fill = st / tot;
        const double qmin = A.MinReservoirOutflowCC[r], qnorm = A.NormalReservoirOutflowCC[r],
                     qnd = A.NonDamagingReservoirOutflowCC[r];
        const double lc2 = 2 * A.ConservativeStorageLimitCC[r], ln = A.NormalStorageLimitCC[r],
                     lf = A.FloodStorageLimitCC[r], lnf = A.Normal_FloodStorageLimitCC[r];
        const double o1 = lf_npmin(qmin, st * inv_day);
        const double o2 = qmin + A.DeltaO[r] * (fill - lc2) / A.DeltaLN[r];
        const double o3b = qnorm + ((fill - lnf) / A.DeltaNFL[r]) * (qnd - qnorm);
        const double tmp = lf_npmin(qnd, lf_npmax(inflow * 1.2, qnorm));
        const double o4 = lf_npmax((fill - lf - 0.01) * tot * inv_day, tmp);
        double o = o1;
        if (fill > lc2) o = o2;
        if (fill > ln) o = qnorm;
        if (fill > lnf) o = o3b;
        if (fill > lf) o = o4;
        const double tmp2 = lf_npmin(o, lf_npmax(inflow, qnorm));
        if ((o > 1.2 * inflow) && (o > qnorm) && (fill < lf)) o = tmp2;
        double out_m3 = o * A.DtRouting;
        out_m3 = lf_npmin(out_m3, st);
        out_m3 = lf_npmax(out_m3, st - tot);
        st -= out_m3;
        double f2 = st / tot;
        if (f2 != f2 || f2 < 0) f2 = 0;
        A.ReservoirStorageM3CC[r] = st;
        A.ReservoirFillCC[r] = f2;
        A.QResOutM3Dt[A.res_cell[r]] = out_m3;
    }
}

__device__ __forceinline__ void lf_site_update(const lf_inloop_args &A, long long i) { lf_site_body(A, i, lf_site_inflow(A, i)); }

// ---- host side ----
// The lake and reservoir lists of the fused calls with structures in the loop (lf_router.hip: fused_impl), as the router
// keeps them between calls: the levels of the site cells and the site plan of the time-major form (lf_common.h:
// lf_site_plan_t), on the host where the schedules read them (lf_fused.h: fused_wavefront) and on the device.  A set of
// lists is checked and planned once, by ensure(), and known by its four device pointers and two counts: a caller that
// rewrites its lists at the same addresses says so with reset().  ensure() forgets the key before anything else and stamps
// it last: whatever fails in between -- refused lists, an allocation, a copy -- leaves a cache that matches nothing.
struct fused_site_cache {
    const void *key[4] = {nullptr, nullptr, nullptr, nullptr}; // lake_cell, lake_ups_idx, res_cell, res_ups_idx
    int64_t cnt[2] = {-1, -1};                                 // n_lakes, n_res
    bool applies = false;                                      // the plan applies (and every feeder is a link of the graph)
    int64_t nfeed = 0;
    std::vector<int32_t> site_level_sorted; // levels of the site cells, ascending (the sites callback of the skewed schedules)
    std::vector<int32_t> level_ptr;         // sites per level: host copy of site_ptr (empty: no site)
    lf_dbuf<int> site_level;                // fused_args::site_level
    lf_dbuf<uint8_t> flags;                 // [N] 1: link, 2: site cell -- fused_args::linked of the time-major form
    lf_dbuf<int32_t> slot, site_ptr, site;  // fused_args::tm_slot / tm_site_ptr / tm_site
    // [nsteps + 1][nfeed] ChanQ of the cells feeding a site ([slice] of them, one per member, in an ensemble call): working
    // storage, grown on demand
    mutable lf_dbuf<double> feed;

    bool matches(const lf_inloop_args &I) const
    {
        const void *k[4] = {I.lake_cell, I.lake_ups_idx, I.res_cell, I.res_ups_idx};
        return I.n_lakes + I.n_res > 0 && cnt[0] == I.n_lakes && cnt[1] == I.n_res && std::equal(k, k + 4, key);
    }
    void reset() // matches nothing: the rest is read only behind a key that matched or was stamped
    {
        std::fill(key, key + 4, nullptr);
        cnt[0] = cnt[1] = -1;
    }
    // The lists of I (counts >= 0) checked, planned and resident; nothing to do for those of the last build, or for none.
    // level_start: the router's level table over its n cells (host); linked: the graph's structure links (device, null: none).
    int ensure(int64_t n, const std::vector<int64_t> &level_start, const uint8_t *linked, const lf_inloop_args &I, hipStream_t s)
    {
        const int64_t nsites = I.n_lakes + I.n_res;
        if (nsites == 0 || matches(I)) return LF_OK;
        reset();
        std::vector<int32_t> cell[2], ptr[2], idx[2]; // host copies of the lists: lakes, reservoirs
        const int64_t count[2] = {I.n_lakes, I.n_res};
        const int32_t *const dev[2][3] = {{I.lake_cell, I.lake_ups_ptr, I.lake_ups_idx}, {I.res_cell, I.res_ups_ptr, I.res_ups_idx}};
        for (int li = 0; li < 2; ++li) {
            if (count[li] == 0) continue;
            if (!dev[li][0] || !dev[li][1] || !dev[li][2])
                return lf_set_error(LF_E_INVALID, "%s site lists missing", li ? "reservoir" : "lake");
            cell[li].resize(count[li]);
            ptr[li].resize(count[li] + 1);
            LF_HIP(hipMemcpy(cell[li].data(), dev[li][0], sizeof(int32_t) * count[li], hipMemcpyDeviceToHost));
            LF_HIP(hipMemcpy(ptr[li].data(), dev[li][1], sizeof(int32_t) * (count[li] + 1), hipMemcpyDeviceToHost));
            const int32_t entries = std::max<int32_t>(ptr[li].back(), 0); // (a pointer out of range: the plan refuses it)
            idx[li].resize(std::max<int32_t>(entries, 1));
            if (entries > 0) LF_HIP(hipMemcpy(idx[li].data(), dev[li][2], sizeof(int32_t) * entries, hipMemcpyDeviceToHost));
        }
        lf_site_plan_t P;
        LF_TRY(lf_site_plan_build(n, (int64_t)level_start.size() - 1, level_start.data(), I.n_lakes, cell[0].data(), ptr[0].data(),
                                  idx[0].data(), I.n_res, cell[1].data(), ptr[1].data(), idx[1].data(), P));
        if (const int64_t i = P.off_level_site; i >= 0)
            return lf_set_error(LF_E_INVALID, "%s %lld: a cell draining into it is not on its level -- build the router's graph "
                                "with lf_graph_create_ex(virtual_down)", i < I.n_lakes ? "lake" : "reservoir",
                                (long long)(i < I.n_lakes ? i : i - I.n_lakes));
        std::vector<uint8_t> fl((size_t)n, 0);
        if (linked) {
            LF_HIP(hipMemcpyAsync(fl.data(), linked, (size_t)n, hipMemcpyDeviceToHost, s));
            LF_HIP(hipStreamSynchronize(s));
        }
        for (int64_t p = 0; p < n && P.applies; ++p) // a feeder that is no link of the graph would never be written
            if (P.slot_of[p] >= 0 && !fl[p]) P.applies = false;
        if (P.applies) {
            for (int li = 0; li < 2; ++li)
                for (int32_t c : cell[li]) fl[c] |= 2;
            LF_TRY(flags.upload(fl.data(), fl.size(), s));
            LF_TRY(slot.upload(P.slot_of.data(), P.slot_of.size(), s));
            LF_TRY(site_ptr.upload(P.level_ptr.data(), P.level_ptr.size(), s));
            LF_TRY(site.upload(P.level_site.data(), P.level_site.size(), s));
        }
        LF_TRY(site_level.upload(P.site_level.data(), (size_t)nsites, s));
        site_level_sorted = std::move(P.site_level_sorted);
        level_ptr = std::move(P.level_ptr);
        nfeed = P.nfeed;
        applies = P.applies;
        const void *k[4] = {I.lake_cell, I.lake_ups_idx, I.res_cell, I.res_ups_idx};
        std::copy(k, k + 4, key);
        cnt[0] = I.n_lakes;
        cnt[1] = I.n_res;
        return LF_OK;
    }
};
