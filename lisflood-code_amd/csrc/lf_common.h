// lf_common.h -- internal declarations shared by the translation units of liblisflood_amd.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdlib>
#include <cstdint>
#include <cstdio>
#include <string>
#include <map>
#include <utility>
#include <vector>

#include "../../include/lisflood_amd.h"

#define LF_NEWTON_TOL 1e-12 /* kinematic_wave_parallel_tools.py:26 */
#define LF_MAX_ITERS 3000   /* kinematic_wave_parallel_tools.py:27 */

int lf_set_error(int code, const char *fmt, ...);

#define LF_HIP(call)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return lf_set_error(LF_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                                __LINE__);                                                                \
    } while (0)

#define LF_TRY(call)          \
    do {                      \
        int rc_ = (call);     \
        if (rc_ != LF_OK) return rc_; \
    } while (0)

// Per-device context: one compute stream, a stopwatch event pair.
struct lf_device_ctx {
    bool ready = false;
    hipStream_t stream = nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    // staging arena of the *_host entry points (lf_soil.hip): one grow-only device allocation carved up per call
    // instead of ~70 hipMalloc / hipFree pairs; a call that needs more gets overflow buffers and the arena grows
    // before the next one
    void *stage_base = nullptr;
    size_t stage_bytes = 0, stage_need = 0;
    void *soil_ws = nullptr; // lists and straggler records of the soil call (lf_soil.hip: soil_ws_layout)
    size_t soil_ws_bytes = 0, soil_ntiles = 0;
    int soil_last_form = 0; // of the last soil / land-surface call: lf_soil_last_form
    int module_last_form[2] = {0, 0}; // of the last pixel-aggregates / surface-step call: lf_module_last_form
    // upload stream for double-buffered inputs (lf_upload_*): copies of the NEXT step's forcing overlap the kernels of
    // the current one; per buffer set an event "copy finished" and an event "last kernel reading the set finished"
    hipStream_t copy_stream = nullptr;
    // lf_upload_copy_f32, lf_upload_rows: staging buffer (device pointer, bytes) of the raw host image per destination vector
    std::map<void *, std::pair<void *, size_t>> upload_stage;
    hipEvent_t copied[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
    bool consumed_valid[2] = {false, false}, copied_valid[2] = {false, false};
    // download stream for double-buffered results (lf_report_acquire, lf_download_*): the copy of a step's report maps runs
    // beside the kernels of the step after it; per set an event "copy finished", and two events that carry what the main
    // and the side stream held at lf_download_begin over to the download stream.  All five are made and released together
    bool down_ready = false;
    hipStream_t down_stream = nullptr;
    hipEvent_t downloaded[2] = {nullptr, nullptr}, down_after[2] = {nullptr, nullptr};
    bool downloaded_valid[2] = {false, false};
    int down_open = -1; // the set between lf_download_begin and lf_download_end, -1: none
    // page-locked staging ring of lf_memcpy_h2d_staged: small per-step uploads that must not stall the host
    struct staged_slot {
        void *host = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr;
        bool in_flight = false;
    };
    staged_slot staged[8];
    int staged_next = 0;
    int upload_open = -1; // the set between lf_upload_begin and lf_upload_end, -1: none (lf_upload_perturb_rows asks)
    // coefficient tables of lf_members_perturb_device / lf_upload_perturb_rows on the device: a ring of kPerturbSlots
    // tables of 128 x 16 doubles in one allocation made on first use (lf_device_trim frees it).  A table is filled through
    // the page-locked ring above on the call's stream; the event behind the call's kernel lets the next user of the
    // slot -- possibly on another stream -- wait for it on the device, never on the host
    static constexpr int kPerturbSlots = 4;
    static constexpr size_t kPerturbTableBytes = 128 * 16 * sizeof(double);
    void *perturb_tables = nullptr;
    hipEvent_t perturb_read[kPerturbSlots] = {nullptr, nullptr, nullptr, nullptr};
    bool perturb_read_valid[kPerturbSlots] = {false, false, false, false};
    int perturb_next = 0;
    // side stream (lf_side_stream_*): a part of a step that the NEXT step's first kernels do not depend on -- the channel
    // wavefront of a model step beside the canopy / soil / overland kernels of the step after it (hotpath.py)
    hipStream_t side_stream = nullptr, main_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_side_done = nullptr;
    bool side_active = false, side_pending = false;
    // lanes (lf_lane_*): streams for independent work items of one device (loopback blocks of the partition)
    std::vector<hipStream_t> lanes;
    std::vector<hipEvent_t> lane_done;
    std::vector<bool> lane_used;
    hipEvent_t lane_fork = nullptr;
    hipStream_t lane_main = nullptr;
    int lane_current = 0;
    bool lane_forked = false;
};
int lf_ctx(int device, lf_device_ctx **out); // makes `device` current, creates the context on first use
// lf_memcpy_h2d_staged on a stream of the caller's choice: `bytes` of host memory through a page-locked slot of the context's
// ring (the source is free again on return) to dst_dev by DMA on `s`; the slot's event is recorded on `s`
int lf_staged_h2d(lf_device_ctx *c, hipStream_t s, void *dst_dev, const void *src_host, size_t bytes);

// Host-side graph.  Positions ("sweep order") are the engine's internal cell numbering: levels
// ascending (level = max distance to outlet - distance, as kinematic_wave_parallel.py:148-149),
// breadth-first from the outlets inside a level, which makes the upstream cells of position p the
// contiguous positions [ups_ptr[p], ups_ptr[p+1]) in ascending pixel id.
struct lf_graph {
    int H = 0, W = 0;
    int64_t N = 0, NL = 0;
    int K = 1;
    std::vector<int32_t> down;        // [N] downstream pixel id, -1 = none
    std::vector<int32_t> perm;        // [N] position -> pixel
    std::vector<int32_t> ups_ptr;     // [N+1]
    std::vector<int64_t> level_start; // [NL+1]
    // zero-length structure links (lf_graph_create_ex): flag per POSITION, 1 = this pit hangs on a structure cell of
    // its own level.  Such cells sit at the end of their level outside every upstream range, so the LAST cell of
    // the next level finds them behind its own children: only sweeps that write a separate router-output buffer
    // (the fused sub-step wavefront, which stores 0 for them) may run on such a graph.
    std::vector<uint8_t> linked;
    bool has_links = false;
    uint64_t serial = 0; // identity of this graph object (unique per process): routers swept together must share it
    lf_graph() = default;
    lf_graph(const lf_graph &) = delete;
    lf_graph &operator=(const lf_graph &) = delete;
};

template <typename T>
struct lf_dbuf { // owning device buffer
    T *p = nullptr;
    size_t n = 0;
    int alloc(size_t count)
    {
        release();
        n = count;
        if (count == 0) return LF_OK;
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return lf_set_error(LF_E_HIP, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
        }
        return LF_OK;
    }
    // A buffer of `count` elements in place of this one (contents not kept), for buffers that grow on demand: the new one
    // is taken first, so when it does not fit this one is still whole -- p and n as they were -- and the caller can refuse
    // its call and serve the next one.
    int grow(size_t count)
    {
        lf_dbuf<T> next;
        if (int rc = next.alloc(count)) {
            (void)hipGetLastError(); // (the refused hipMalloc is reported here, not by the next call's launch check)
            return rc;
        }
        std::swap(p, next.p);
        std::swap(n, next.n);
        return LF_OK;
    }
    // `stream`: the stream the kernels that read the buffer run on.  The library's compute stream is non-blocking, i.e. it
    // does not synchronise with the legacy stream a plain hipMemcpy uses, and a pageable H2D copy may return once the
    // source is staged: the copy is therefore enqueued on the consumer's own stream and waited for there.
    int upload(const T *src, size_t count, hipStream_t stream = nullptr)
    {
        LF_TRY(alloc(count));
        if (count) {
            LF_HIP(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, stream));
            LF_HIP(hipStreamSynchronize(stream));
        }
        return LF_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~lf_dbuf() { release(); }
    lf_dbuf() = default;
    lf_dbuf(const lf_dbuf &) = delete;
    lf_dbuf &operator=(const lf_dbuf &) = delete;
};

// The [nsteps][N] history of the time-major fused form (k_fused_level_steps) is OPTIONAL working storage: without it the
// skewed wavefront runs.  It can be tens of GB (10000^2, 24 split sub-steps: 2 x 19 GB), so it is taken only inside a
// budget -- LF_FUSED_TIME_MAJOR_MAX_BYTES if set, otherwise half of what hipMemGetInfo reports free (counting what the
// two buffers already hold) -- and a refused size is remembered, so a router that does not fit never pays a multi-GB
// hipMalloc / failed hipMalloc / synchronising hipFree per call.  -> true: both buffers hold `count` doubles (h2 only
// if `two`).
// The budget itself (bytes; counting what the two buffers already hold) -> false: the device did not tell.
inline bool lf_history_budget(const lf_dbuf<double> &h1, const lf_dbuf<double> &h2, size_t &budget)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const size_t held = (h1.p ? h1.n : 0) * sizeof(double) + (h2.p ? h2.n : 0) * sizeof(double);
    budget = (free_b + held) / 2;
    static const long long cap = [] {
        const char *e = std::getenv("LF_FUSED_TIME_MAJOR_MAX_BYTES");
        return e ? std::atoll(e) : -1ll;
    }();
    if (cap >= 0) budget = std::min((size_t)cap, free_b + held);
    return true;
}
inline bool lf_history_ensure(lf_dbuf<double> &h1, lf_dbuf<double> &h2, size_t &refused_bytes, size_t count, bool two)
{
    const bool ok1 = h1.p && h1.n >= count, ok2 = !two || (h2.p && h2.n >= count);
    if (ok1 && ok2) return true;
    const size_t total = count * sizeof(double) * (two ? 2 : 1);
    if (total >= refused_bytes) return false;
    size_t budget = 0;
    if (!lf_history_budget(h1, h2, budget)) {
        refused_bytes = total;
        return false;
    }
    if (total > budget) {
        refused_bytes = total;
        return false;
    }
    bool ok = true;
    if (!ok1) ok = h1.alloc(count) == LF_OK;
    if (ok && !ok2) ok = h2.alloc(count) == LF_OK;
    if (!ok) {
        (void)hipGetLastError();
        h1.release();
        h2.release();
        refused_bytes = total;
    }
    return ok;
}

// Site plan of the time-major fused form with lakes and reservoirs in the loop (lf_fused.h: k_fused_level_steps<.., STRUCT>),
// a pure function of the level table and the six site lists (engine positions):
//  * feed slots: entry e of lake_ups_idx has slot e, entry e of res_ups_idx slot lake_ups_ptr[n_lakes] + e; slot_of[N] is the
//    inverse map (cell position -> slot, -1: the cell feeds no site);
//  * the sites of every level: level_site[level_ptr[k] .. level_ptr[k + 1]) are the sites (lakes 0 .. n_lakes - 1, then the
//    reservoirs) whose cell is on level k, ascending;
//  * applies: no site cell feeds another site (chained sites), no two sites share a cell, no cell feeds two sites and every
//    feeder is on its site's level -- otherwise the skewed wavefront runs.  The arrays are complete only if it applies;
//  * whether or not it applies: site_level[i], the level of site i's cell, site_level_sorted, the same ascending, and
//    off_level_site, the first site with a feeder off its own level (-1: none) -- no schedule runs that (fused_site_cache).
// A cell, a pointer or a level table out of range is an error (LF_E_INVALID), not a plan that does not apply.
struct lf_site_plan_t {
    bool applies = false;
    int64_t nfeed = 0, off_level_site = -1;
    std::vector<int32_t> slot_of, level_ptr, level_site, site_level, site_level_sorted;
};
inline int lf_site_plan_build(int64_t n, int64_t nlevels, const int64_t *level_start, int64_t n_lakes, const int32_t *lake_cell,
                              const int32_t *lake_ups_ptr, const int32_t *lake_ups_idx, int64_t n_res, const int32_t *res_cell,
                              const int32_t *res_ups_ptr, const int32_t *res_ups_idx, lf_site_plan_t &P)
{
    if (n < 0 || n >= ((int64_t)1 << 31) || nlevels < 0 || !level_start || n_lakes < 0 || n_res < 0 ||
        n_lakes + n_res >= ((int64_t)1 << 31))
        return lf_set_error(LF_E_INVALID, "site plan: bad argument");
    if (level_start[0] != 0 || level_start[nlevels] != n) return lf_set_error(LF_E_INVALID, "site plan: the levels do not cover the cells");
    for (int64_t k = 0; k < nlevels; ++k)
        if (level_start[k] > level_start[k + 1]) return lf_set_error(LF_E_INVALID, "site plan: level table not ascending");
    if ((n_lakes > 0 && (!lake_cell || !lake_ups_ptr)) || (n_res > 0 && (!res_cell || !res_ups_ptr)))
        return lf_set_error(LF_E_INVALID, "site plan: site lists missing");
    const int64_t nsites = n_lakes + n_res;
    const int64_t lake_entries = n_lakes > 0 ? lake_ups_ptr[n_lakes] : 0, res_entries = n_res > 0 ? res_ups_ptr[n_res] : 0;
    auto check_list = [&](int64_t cnt, const int32_t *cell, const int32_t *ptr, const int32_t *idx, const char *what) -> int {
        if (cnt == 0) return LF_OK;
        if (ptr[0] != 0) return lf_set_error(LF_E_INVALID, "site plan: %s_ups_ptr does not start at 0", what);
        for (int64_t i = 0; i < cnt; ++i) {
            if (cell[i] < 0 || cell[i] >= n) return lf_set_error(LF_E_INVALID, "site plan: %s cell out of range", what);
            if (ptr[i + 1] < ptr[i]) return lf_set_error(LF_E_INVALID, "site plan: %s_ups_ptr not ascending", what);
        }
        if (ptr[cnt] > 0 && !idx) return lf_set_error(LF_E_INVALID, "site plan: %s_ups_idx missing", what);
        for (int32_t e = 0; e < ptr[cnt]; ++e)
            if (idx[e] < 0 || idx[e] >= n) return lf_set_error(LF_E_INVALID, "site plan: a cell draining into a %s is out of range", what);
        return LF_OK;
    };
    LF_TRY(check_list(n_lakes, lake_cell, lake_ups_ptr, lake_ups_idx, "lake"));
    LF_TRY(check_list(n_res, res_cell, res_ups_ptr, res_ups_idx, "reservoir"));
    if (lake_entries + res_entries >= ((int64_t)1 << 31)) return lf_set_error(LF_E_INVALID, "site plan: too many feeders");
    auto level_of = [&](int64_t pos) { return (int32_t)(std::upper_bound(level_start, level_start + nlevels + 1, pos) - level_start) - 1; };
    P.applies = true;
    P.nfeed = lake_entries + res_entries;
    P.off_level_site = -1;
    P.slot_of.assign((size_t)n, -1);
    P.site_level.assign((size_t)nsites, 0);
    P.level_ptr.assign((size_t)nlevels + 1, 0);
    P.level_site.assign((size_t)nsites, 0);
    std::vector<uint8_t> is_site((size_t)n, 0);
    auto cell_of = [&](int64_t i) { return i < n_lakes ? lake_cell[i] : res_cell[i - n_lakes]; };
    for (int64_t i = 0; i < nsites; ++i) {
        const int32_t c = cell_of(i);
        if (is_site[c]) P.applies = false; // two sites share a cell
        is_site[c] = 1;
        P.site_level[i] = level_of(c);
        ++P.level_ptr[P.site_level[i] + 1];
    }
    for (int64_t k = 0; k < nlevels; ++k) P.level_ptr[k + 1] += P.level_ptr[k];
    {
        std::vector<int32_t> next(P.level_ptr.begin(), P.level_ptr.end() - 1);
        for (int64_t i = 0; i < nsites; ++i) P.level_site[next[P.site_level[i]]++] = (int32_t)i;
    }
    P.site_level_sorted = P.site_level;
    std::sort(P.site_level_sorted.begin(), P.site_level_sorted.end());
    auto feeders = [&](int64_t cnt, const int32_t *ptr, const int32_t *idx, int64_t site0, int64_t slot0) {
        for (int64_t i = 0; i < cnt; ++i)
            for (int32_t e = ptr[i]; e < ptr[i + 1]; ++e) {
                const int32_t c = idx[e];
                if (P.slot_of[c] >= 0) // a cell feeds two sites (or is listed twice)
                    P.applies = false;
                else
                    P.slot_of[c] = (int32_t)(slot0 + e);
                const bool off_level = level_of(c) != P.site_level[site0 + i];
                if (is_site[c] || off_level) P.applies = false; // chained sites; not on the site's level
                if (off_level && P.off_level_site < 0) P.off_level_site = site0 + i;
            }
    };
    feeders(n_lakes, lake_ups_ptr, lake_ups_idx, 0, 0);
    feeders(n_res, res_ups_ptr, res_ups_idx, n_lakes, lake_entries);
    return LF_OK;
}
