// lf_router.hip -- kinematic-wave routing on gfx950: level-ordered implicit sweep with a per-cell
// Newton-Raphson solve.  Replaces kinematicWave.kinematicWaveRouting + kinematicRouting + solve1Pixel
// (kinematic_wave_parallel.py:160-184, kinematic_wave_parallel_tools.py:34-92).
//
// Data layout (HBM, all fp64 unless noted), N = land pixels, positions = sweep order (lf_graph):
//   perm[N]      int32  position -> pixel (gather/scatter to the caller's pixel-order vectors)
//   ups_ptr[N+1] int32  upstream cells of position p are the CONTIGUOUS positions [ups_ptr[p], ups_ptr[p+1])
//   a1[N], a2[N]        alpha*dx/dt for main channel / floodplains, sweep order
//   dx[N]               space delta (only when it is per-pixel), sweep order
//   constant[N]         a*Qold^beta + q*dx, sweep order (written by the prep kernel)
//   qord[N]             new discharge, sweep order (read by the downstream level)
// Because a level is a contiguous range of positions and the upstream cells of consecutive positions
// are consecutive too, every global access of the sweep except the perm-indexed gather/scatter of the
// caller's vectors is a coalesced stream.
//
// Launch structure per call: 1 prep launch over all cells, then one launch per "wide" level
// (> kNarrowMax cells, one cell per lane) and one single-workgroup launch per run of consecutive
// "narrow" levels (the workgroup walks the levels with a barrier between them).  A dependent kernel
// boundary costs ~1.5 us on MI355X, less than any software grid barrier (4-7 us), so wide levels
// are separated by launches, not by in-kernel synchronisation.
#include <algorithm>
#include <cmath>

#include <cstdlib>
#include <cstring>

#include "lf_blocks.h"
#include "lf_structures.h"
#include "lf_sweep.h"

namespace {

// out[pixel(p)] = sum of w over the upstream cells of p, ascending pixel id (np.bincount order)
// (`linked`: zero-length structure links of lf_graph_create_ex sit behind the last range of a level -- skipped)
__global__ void __launch_bounds__(kBlock) k_upstream_sum(int n, const int *__restrict__ perm,
                                                         const int *__restrict__ ups_ptr, const double *__restrict__ w_pix,
                                                         double *__restrict__ out_pix, const uint8_t *__restrict__ linked)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    double s = 0.0;
    for (int e = ups_ptr[p]; e < ups_ptr[p + 1]; ++e)
        if (!linked || !linked[e]) s += w_pix[perm[e]];
    out_pix[perm[p]] = s;
}

// accuflux: acc[p] = x[p] + sum over upstream acc (upstream first, ascending pixel id, then the cell itself); up to
// kMaxAccu vectors share a sweep (the catchment totals of routing.py:645-691 come four at a time)
constexpr int kMaxAccu = 4;
struct accu_multi {
    const double *x[kMaxAccu];
    double *acc[kMaxAccu];
};

template <int NV>
__global__ void __launch_bounds__(kBlock) k_accu_level(int first, int count, const int *__restrict__ ups_ptr, accu_multi M)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const int p = first + i;
    const int u0 = ups_ptr[p], u1 = ups_ptr[p + 1];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double s = 0.0;
        for (int e = u0; e < u1; ++e) s += M.acc[v][e];
        M.acc[v][p] = s + M.x[v][p];
    }
}

template <int NV>
__global__ void __launch_bounds__(kNarrowBlock) k_accu_narrow(int k0, int k1, const long long *__restrict__ level_start,
                                                              const int *__restrict__ ups_ptr, accu_multi M)
{
    for (int k = k0; k < k1; ++k) {
        const int first = (int)level_start[k], last = (int)level_start[k + 1];
        for (int p = first + (int)threadIdx.x; p < last; p += kNarrowBlock) {
            const int u0 = ups_ptr[p], u1 = ups_ptr[p + 1];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                double s = 0.0;
                for (int e = u0; e < u1; ++e) s += M.acc[v][e];
                M.acc[v][p] = s + M.x[v][p];
            }
        }
        __threadfence_block();
        __syncthreads();
    }
}

// One block of consecutive levels of the router's plan (build_level_blocks, the plan of k_sweep_cones), cone by cone.
// An accumulation level is a handful of additions, far shorter than a trip to memory, so the cone is worked through in
// CHUNKS of LC levels: all operands of a chunk (upstream ranges, x) are requested at once and parked in LDS -- one memory
// latency per chunk instead of one per level --, the levels of the chunk are then added up from LDS alone (the sums
// replace x in place and are the next level's inflow), and the chunk's sums leave with one burst of stores that nothing
// waits for.  CW = cells per level of a cone = threads (64: one wavefront, whose LDS operations complete in order -- no
// barrier).  Same additions in the same order as k_accu_level.
template <int NV, int CW>
__global__ void __launch_bounds__(CW) k_accu_cones(cone_plan_args C, const int *__restrict__ ups_ptr, accu_multi M)
{
    constexpr int LC0 = 49152 / (CW * (8 + 8 * NV)), LC = LC0 < 2 ? 2 : (LC0 > 64 ? 64 : LC0);
    __shared__ int U0[LC][CW], U1[LC][CW];
    __shared__ double X[NV][LC][CW], PREV[NV][CW];
    const int tid = threadIdx.x, nl = C.nl;
    const int *c0 = C.cone + (size_t)blockIdx.x * nl, *c1 = c0 + nl;
    int first_up = 0;
    for (int j0 = 0; j0 < nl; j0 += LC) {
        const int L = nl - j0 < LC ? nl - j0 : LC;
        // ---- every operand of the chunk: independent loads, all in flight together ----
#pragma unroll 8
        for (int jj = 0; jj < L; ++jj) {
            const int p = ld_table(c0, j0 + jj) + tid;
            const bool act = p < ld_table(c1, j0 + jj);
            const int pc = act ? p : 0;
            const int u0 = ups_ptr[pc], u1 = ups_ptr[pc + 1];
            U0[jj][tid] = u0;
            U1[jj][tid] = act ? u1 : u0; // a lane beyond the cone's range: no upstream cells, its sum is never stored
#pragma unroll
            for (int v = 0; v < NV; ++v) X[v][jj][tid] = M.x[v][pc];
        }
        cone_sync<CW>();
        // ---- the levels of the chunk, from LDS ----
        for (int jj = 0; jj < L; ++jj) {
            const int first = ld_table(c0, j0 + jj);
            const int u0 = U0[jj][tid], u1 = U1[jj][tid];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                double t[8];
                if (j0 + jj == 0) { // from the block before (previous launch)
#pragma unroll
                    for (int k = 0; k < 8; ++k) t[k] = (u0 + k < u1) ? M.acc[v][u0 + k] : 0.0;
                } else {
                    const double *z = jj == 0 ? &PREV[v][0] : &X[v][jj - 1][0];
                    const int base = u0 - first_up;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const bool have = u0 + k < u1;
                        const double w = z[have ? base + k : 0];
                        t[k] = have ? w : 0.0;
                    }
                }
                double sum = 0.0;
#pragma unroll
                for (int k = 0; k < 8; ++k) sum += t[k];
                const double a = sum + X[v][jj][tid];
                X[v][jj][tid] = a;
            }
            cone_sync<CW>();
            first_up = first;
        }
        // ---- the chunk's sums: one burst of stores; the last level stays behind for the next chunk ----
        for (int jj = 0; jj < L; ++jj) {
            const int p = ld_table(c0, j0 + jj) + tid;
            if (p < ld_table(c1, j0 + jj)) {
#pragma unroll
                for (int v = 0; v < NV; ++v) M.acc[v][p] = X[v][jj][tid];
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) PREV[v][tid] = X[v][L - 1][tid];
        cone_sync<CW>();
    }
}

__global__ void __launch_bounds__(kBlock) k_count_nonfinite(long long n, const double *__restrict__ x,
                                                            unsigned long long *count)
{
    long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long local = 0;
    for (; i < n; i += (long long)gridDim.x * kBlock) local += !isfinite(x[i]);
    for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(count, local);
}

} // namespace

struct lf_router : lf_router_core {
    int64_t NL = 0;
    lf_dbuf<double> qord, io_q, io_lat, tmp_ord;
    lf_dbuf<double> members_pix, members_ord; // lf_router_route_members_host: [2][members][N] discharge, lateral inflow
    lf_dbuf<unsigned long long> counter;
    lf_dbuf<uint8_t> linked; // zero-length structure links (lf_graph_create_ex); null without them
    lf_dbuf<int> level_nlinked; // ... and how many of them are parked at the end of every level (k_fused_cones_split)
    lf_dbuf<int32_t> parent; // [N] downstream position of every position, -1 = outlet (lf_ldd.hip builds it on demand)
    lf_dbuf<int32_t> root;   // [N] position of the outlet every position drains to (lf_ldd.hip, on demand: catchment totals)
    lf_dbuf<double> totals_scratch; // catchment totals: engine-order copies of the weights and their accuflux
    std::vector<level_segment> schedule; // launches of a call without level blocks (level_segments)
    uint64_t graph_serial = 0; // lf_graph::serial of the graph the router was built on: same object <=> same plan
    // (the fused plan of lf_router_core, fplan, is build_level_blocks' and carries lvl2blk for the sites of the structures
    // variant; rplan feeds k_sweep_cones)
    lf_dbuf<double2> adx1, adx2; // the (a, dx) records of k_level<.., STATICS = 1> per section (level_statics)
    // the upstream ranges of k_level<.., STATICS = 2>, the graph's and so both sections' (level_counts): a count byte per
    // cell, and ups_ptr at every 64th cell of every level -- level k's entries from wave_off[k] on
    lf_dbuf<unsigned char> upcnt;
    lf_dbuf<int> wave_start, wave_off_dev;
    std::vector<int> wave_off;
    int64_t last_stats[4] = {0, 0, 0, 0};
    fused_site_cache sites; // the lake and reservoir lists of the last fused call with structures in the loop
    // profiling
    bool profile = false;
    std::vector<hipEvent_t> ev_pool;
    struct rec {
        int cls;
        size_t e0, e1;
        int64_t cells;
    };
    std::vector<rec> recs;
    size_t ev_used = 0;
    double prof_acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    ~lf_router()
    {
        for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    }
    int ev_get(size_t *idx)
    {
        if (ev_used == ev_pool.size()) {
            hipEvent_t e;
            LF_HIP(hipEventCreate(&e));
            ev_pool.push_back(e);
        }
        *idx = ev_used++;
        return LF_OK;
    }
    int prof_begin(int cls, int64_t cells)
    {
        if (!profile) return LF_OK;
        rec r{cls, 0, 0, cells};
        LF_TRY(ev_get(&r.e0));
        LF_TRY(ev_get(&r.e1));
        LF_HIP(hipEventRecord(ev_pool[r.e0], ctx->stream));
        recs.push_back(r);
        return LF_OK;
    }
    int prof_end()
    {
        if (!profile) return LF_OK;
        LF_HIP(hipEventRecord(ev_pool[recs.back().e1], ctx->stream));
        return LF_OK;
    }
    int prof_collect()
    {
        if (recs.empty()) return LF_OK;
        LF_HIP(hipStreamSynchronize(ctx->stream));
        for (const rec &r : recs) {
            float ms = 0.f;
            LF_HIP(hipEventElapsedTime(&ms, ev_pool[r.e0], ev_pool[r.e1]));
            prof_acc[3 * r.cls + 0] += 1.0;
            prof_acc[3 * r.cls + 1] += (double)ms;
            prof_acc[3 * r.cls + 2] += (double)r.cells;
        }
        recs.clear();
        ev_used = 0;
        return LF_OK;
    }
};

namespace {

// The (a, dx) records of A's section for the wide levels of an ordered beta = 3/5 call, or nullptr: dx is a scalar (the
// sweep then has one static load anyway), LF_LEVEL_STATICS=0 or no memory for them (16 bytes per cell and section).
const double2 *level_statics(lf_router *r, const sweep_args &A)
{
    if (!level_records_wanted(*r)) return nullptr;
    lf_dbuf<double2> &buf = (A.a == r->a1.p) ? r->adx1 : r->adx2;
    if (!buf.p) {
        if (!level_records_alloc(*r, buf)) return nullptr;
        hipLaunchKernelGGL(k_static_records, dim3((unsigned)((r->N + kLevelBlock - 1) / kLevelBlock)), dim3(kLevelBlock), 0, r->ctx->stream,
                           (long long)r->N, A.a, (const double *)r->dx.p, buf.p);
    }
    return buf.p;
}

// The count bytes and wavefront starts of r's graph for the wide levels that read the records, built on first use -> true;
// LF_LEVEL_COUNTS=0 or no memory for them (1 byte per cell, 4 bytes per 64 cells of a level; a refusal is the records'
// refusal: the separate streams stay for good) -> false
bool level_counts(lf_router *r)
{
    if (!level_counts_enabled() || r->statics_refused) return false;
    if (r->wave_start.p) return true;
    const size_t nl = r->h_level_start.size() - 1;
    r->wave_off.assign(nl + 1, 0);
    for (size_t k = 0; k < nl; ++k)
        r->wave_off[k + 1] = r->wave_off[k] + (int)((r->h_level_start[k + 1] - r->h_level_start[k] + 63) / 64);
    if (!level_records_alloc(*r, r->upcnt)) return false;
    lf_dbuf<int> table;
    if (!level_records_alloc(*r, table, true, (size_t)r->wave_off[nl]) || r->wave_off_dev.upload(r->wave_off.data(), nl + 1, r->ctx->stream) != LF_OK) {
        r->statics_refused = true;
        (void)hipGetLastError();
        r->upcnt.release();
        return false;
    }
    hipLaunchKernelGGL(k_static_counts, dim3((unsigned)((r->N + kLevelBlock - 1) / kLevelBlock)), dim3(kLevelBlock), 0, r->ctx->stream,
                       (long long)r->N, (const int *)r->ups_ptr.p, r->upcnt.p);
    hipLaunchKernelGGL(k_wave_starts, dim3((unsigned)std::min<size_t>(nl, 4096), 64), dim3(kLevelBlock), 0, r->ctx->stream, (long long)nl,
                       (const long long *)r->level_start.p, (const int *)r->wave_off_dev.p, (const int *)r->ups_ptr.p, table.p);
    std::swap(r->wave_start.p, table.p);
    std::swap(r->wave_start.n, table.n);
    return true;
}

// one wide level of an ORDERED beta = 3/5 call
void launch_level_ordered_fused(lf_router *r, hipStream_t s, int first, int cells, sweep_args A)
{
    const dim3 grid(level_blocks_for(cells)), block(kLevelBlock);
    A.adx = level_statics(r, A);
    if (A.adx && level_counts(r)) {
        // the level that starts at `first` (the last of them: the ones before it are empty)
        const size_t k = (size_t)(std::upper_bound(r->h_level_start.begin(), r->h_level_start.end() - 1, (int64_t)first) - r->h_level_start.begin()) - 1;
        A.upcnt = r->upcnt.p;
        A.wave_start = r->wave_start.p + r->wave_off[k];
        hipLaunchKernelGGL((k_level<true, true, false, 2>), grid, block, 0, s, first, cells, A);
    } else if (A.adx)
        hipLaunchKernelGGL((k_level<true, true, false, 1>), grid, block, 0, s, first, cells, A);
    else
        hipLaunchKernelGGL((k_level<true, true>), grid, block, 0, s, first, cells, A);
}

bool cone_split_enabled() // LF_ROUTE_SPLIT=0: one wavefront per cone does everything (the round-3 kernel; A/B switch)
{
    const char *e = std::getenv("LF_ROUTE_SPLIT");
    return !(e && e[0] == '0');
}
// One block of levels cone by cone, for NR routers of one graph.  k_sweep_cones_split comes in two shapes for a single
// router.  FEW cones per launch (at most kFewCones: about one per CU, the chain-bound networks) -> chunks of 8 levels and
// four supply wavefronts, 72 KB of LDS per cone; MANY cones (several per CU: their wavefronts share the SIMDs, the launch
// is throughput-bound) -> chunks of 4 levels and two supply wavefronts, 37 KB.  Several routers on one graph: chunks of 4
// levels, two supply wavefronts.
constexpr int kFewCones = 256;
template <bool FUSED, bool ORDERED, int NR, int KC, int NS>
void launch_split(dim3 grid, hipStream_t s, const cone_plan_args &C, const sweep_args_multi &M)
{
    hipLaunchKernelGGL((k_sweep_cones_split<FUSED, ORDERED, NR, KC, NS>), grid, dim3(64 * (1 + NS)), 0, s, C, M);
}
template <int NR>
void launch_sweep_cones(int cw, bool fused, bool ordered, dim3 grid, hipStream_t s, const cone_plan_args &C,
                        const sweep_args_multi &M)
{
    const bool split = cw == 64 && cone_split_enabled() && C.n_cells < (1 << 29); // (byte offsets of the buffer stores: 32 bits)
    pick_flags(fused, ordered, [&](auto f, auto o) {
        if (split && NR == 1 && (int)grid.x <= kFewCones)
            launch_split<f, o, 1, LF_CONE_KC, LF_CONE_NS>(grid, s, C, M);
        else if (split)
            launch_split<f, o, NR, 4, 2>(grid, s, C, M);
        else if (cw == 64)
            hipLaunchKernelGGL((k_sweep_cones<f, o, NR, 64>), grid, dim3(64), 0, s, C, M);
        else
            hipLaunchKernelGGL((k_sweep_cones<f, o, NR, kBlock>), grid, dim3(kBlock), 0, s, C, M);
    });
}

// Do rs[0 .. count) sweep the level blocks of rs[0]'s route plan together?  Only on one graph object with one plan; else
// the segment schedule, which routers swept together share (swept_together)
bool same_plan(int count, lf_router *const *rs)
{
    const lf_router *r = rs[0];
    bool same = !r->rplan.empty();
    for (int i = 1; i < count; ++i)
        same = same && rs[i]->graph_serial == r->graph_serial && r->graph_serial != 0 && rs[i]->rplan.lmax == r->rplan.lmax &&
               rs[i]->rplan.cw == r->rplan.cw;
    return same;
}

// the launch counts of a call that swept rs[0 .. count) (lf_router_last_launches)
void set_last_stats(int count, lf_router *const *rs, const launch_counts &c)
{
    for (int i = 0; i < count; ++i) {
        rs[i]->last_stats[0] = c.launches;
        rs[i]->last_stats[1] = c.wide;
        rs[i]->last_stats[2] = c.narrow;
        rs[i]->last_stats[3] = rs[i]->NL;
    }
}

// `count` (1 to 4) routers built on the same graph (same level schedule) swept together: one launch per level block, wide
// level or run of narrow levels for all of them.  One router: k_level / k_levels_narrow / k_sweep_cones<.., 1, ..>;
// several: k_level_multi / k_levels_narrow_multi (blockIdx.y / blockIdx.x picks the router) and, on one graph object with
// one plan, k_sweep_cones<.., count, ..>.
int enqueue_route(int count, lf_router **rs, double **q_dev, const double **lat_dev, int section, bool ordered)
{
    lf_router *r = rs[0];
    hipStream_t s = r->ctx->stream;
    const int n = (int)r->N;
    sweep_args_multi M;
    for (int i = 0; i < kMaxMulti; ++i) {
        lf_router *ri = rs[i < count ? i : 0];
        double *q = q_dev[i < count ? i : 0];
        M.r[i] = sweep_args_of(*ri, section, ordered ? q : ri->qord.p, ordered ? nullptr : q, lat_dev[i < count ? i : 0]);
    }
    launch_counts c;
    if (n > 0 && !r->fused)
        for (int i = 0; i < count; ++i) {
            LF_TRY(r->prof_begin(0, n));
            hipLaunchKernelGGL(k_prep, dim3(blocks_for(n)), dim3(kBlock), 0, s, n, ordered ? nullptr : rs[i]->perm.p, q_dev[i],
                               lat_dev[i], M.r[i].a, M.r[i].dx, rs[i]->dx_scalar, rs[i]->beta, rs[i]->constant.p);
            LF_TRY(r->prof_end());
            ++c.launches;
        }
    const bool blocks = same_plan(count, rs);
    LF_TRY(pick_count(count, [&](auto nr) {
        constexpr int NR = nr;
        auto cones = [&](dim3 grid, const cone_plan_args &C, int64_t cells) {
            LF_TRY(r->prof_begin(2, cells));
            launch_sweep_cones<NR>(r->rplan.cw, r->fused, ordered, grid, s, C, M);
            return r->prof_end();
        };
        auto level = [&](int first, int cells) {
            LF_TRY(r->prof_begin(1, cells));
            pick_flags(r->fused, ordered, [&](auto f, auto o) {
                if constexpr (NR > 1)
                    hipLaunchKernelGGL((k_level_multi<f, o>), dim3(blocks_for(cells), NR), dim3(kBlock), 0, s, first, cells, M);
                else if constexpr (f && o)
                    launch_level_ordered_fused(r, s, first, cells, M.r[0]);
                else
                    hipLaunchKernelGGL((k_level<f, o>), dim3(level_blocks_for(cells)), dim3(kLevelBlock), 0, s, first, cells, M.r[0]);
            });
            return r->prof_end();
        };
        auto narrow = [&](int k0, int k1) {
            LF_TRY(r->prof_begin(2, r->h_level_start[k1] - r->h_level_start[k0]));
            pick_flags(r->fused, ordered, [&](auto f, auto o) {
                if constexpr (NR > 1)
                    hipLaunchKernelGGL((k_levels_narrow_multi<f, o>), dim3(NR), dim3(kNarrowBlock), 0, s, k0, k1, r->level_start.p, M);
                else
                    hipLaunchKernelGGL((k_levels_narrow<f, o>), dim3(1), dim3(kNarrowBlock), 0, s, k0, k1, r->level_start.p, M.r[0]);
            });
            return r->prof_end();
        };
        return route_schedule(*r, 0, r->rplan.nblocks(), r->schedule, blocks, c, cones, level, narrow);
    }));
    set_last_stats(count, rs, c);
    return LF_OK;
}

// the section exists and the graph has no structure links: what every plain router call asks of r
int check_plain_call(const lf_router *r, int section)
{
    LF_TRY(check_section(*r, section));
    if (r->linked.p)
        return lf_set_error(LF_E_INVALID, "a router on a graph with structure links (lf_graph_create_ex) runs only the "
                            "fused sub-step path (lf_routing_substeps_fused*)");
    return LF_OK;
}

// May routers[0 .. count) be swept together, one launch for all of them?  Several routers without structure links, on one
// device and stream, with the same cells, solver and level schedule, none of them profiling.
bool swept_together(int count, lf_router *const *routers)
{
    const lf_router *r0 = routers[0];
    bool together = count > 1;
    for (int i = 0; i < count && together; ++i) {
        const lf_router *r = routers[i];
        together = !r->linked.p && r->device == r0->device && r->ctx == r0->ctx && r->N == r0->N && r->fused == r0->fused &&
                   r->h_level_start == r0->h_level_start && !r->profile;
    }
    return together;
}

int route_device(lf_router *r, double *q_dev, const double *lat_dev, int section, bool ordered = false)
{
    LF_TRY(check_plain_call(r, section));
    LF_HIP(hipSetDevice(r->device));
    LF_TRY(enqueue_route(1, &r, &q_dev, &lat_dev, section, ordered));
    LF_HIP(hipGetLastError());
    if (r->profile) LF_TRY(r->prof_collect());
    return LF_OK;
}

// ---- an ensemble on one or several routers of one graph (lf_sweep.h: member_rows) ---------------------------------------
// Members per lane of k_level_members, chosen by measurement on the shallow 10 000^2 graph: 4
// members per lane sweep 4 and 8 members in 0.77 of the time of as many single calls, 2 per lane in 0.86, 1 per lane in
// 0.98; two members are one short group either way (0.87).  LF_MEMBERS_MB = 1, 2 or 4, read at every call, is the A/B
// switch of that measurement (tools/bench_route_members.py --mb).
constexpr int kMembersPerLane = 4;
int members_per_lane()
{
    if (const char *e = std::getenv("LF_MEMBERS_MB")) {
        const int v = std::atoi(e);
        if (v == 1 || v == 2 || v == 4) return v;
    }
    return kMembersPerLane;
}
constexpr int kMaxGridY = 65535; // blockIdx.y picks the unit (cones) or the member group (wide levels)

template <bool FUSED, int STATICS, bool MULTI>
void launch_level_members(int mb, unsigned blocks, int count, int members, hipStream_t s, int first, int cells,
                          const member_block<MULTI> &B, const member_rows &R)
{
    const dim3 grid(blocks, (unsigned)(count * ((members + mb - 1) / mb))), block(kLevelBlock);
    if (mb == 1)
        hipLaunchKernelGGL((k_level_members<FUSED, true, STATICS, 1, MULTI>), grid, block, 0, s, first, cells, B, R);
    else if (mb == 2)
        hipLaunchKernelGGL((k_level_members<FUSED, true, STATICS, 2, MULTI>), grid, block, 0, s, first, cells, B, R);
    else
        hipLaunchKernelGGL((k_level_members<FUSED, true, STATICS, 4, MULTI>), grid, block, 0, s, first, cells, B, R);
}

// `count` routers, one or several that may be swept together (swept_together: the caller's check), each with its `members`
// rows of q_dev[i] / lat_dev[i] (sweep order, `stride` elements apart), swept on rs[0]'s schedule: the plan, the
// LF_ROUTE_CONES switch and the profile hooks of enqueue_route (routers swept together do not profile), every launch once
// for all count * members units (more than kMaxGridY of them: in slices of members).  The chain / supply cone kernel stays
// a single call's: here the members fill the machine.
int enqueue_route_members(int count, lf_router **rs, double *const *q_dev, const double *const *lat_dev, int members,
                          int64_t stride, int section)
{
    lf_router *r = rs[0];
    hipStream_t s = r->ctx->stream;
    const int n = (int)r->N;
    if (!r->fused) {
        bool grow = false;
        for (int i = 0; i < count; ++i) grow = grow || rs[i]->constant.n < (size_t)members * (size_t)n;
        if (grow) LF_HIP(hipStreamSynchronize(s)); // (earlier calls read the buffers that go)
        for (int i = 0; i < count; ++i) // (refused: a router keeps the buffer it had, for fewer members)
            if (rs[i]->constant.n < (size_t)members * (size_t)n) LF_TRY(rs[i]->constant.grow((size_t)members * (size_t)n));
    }
    const bool blocks = same_plan(count, rs);
    const int mb = members_per_lane(), slice = kMaxGridY / count;
    launch_counts c;
    LF_TRY(pick_flags(r->fused, count > 1, [&](auto fused, auto multi) {
        constexpr bool FUSED = fused, MULTI = multi;
        // what a kernel is handed of the routers' blocks: all of them, or the one router's
        auto block_of = [](const sweep_args_multi &M) -> const member_block<MULTI> & {
            if constexpr (MULTI)
                return M;
            else
                return M.r[0];
        };
        for (int m0 = 0; m0 < members; m0 += slice) {
            const int mm = std::min(members - m0, slice), units = count * mm;
            sweep_args_multi M;
            for (int i = 0; i < kMaxMulti; ++i) {
                const int j = i < count ? i : 0;
                M.r[i] = sweep_args_of(*rs[j], section, q_dev[j] + (int64_t)m0 * stride, nullptr, lat_dev[j] + (int64_t)m0 * stride);
                if (!FUSED) M.r[i].constant = rs[j]->constant.p + (int64_t)m0 * n;
            }
            const member_rows R{(long long)stride, (long long)n, mm};
            if (!FUSED) {
                LF_TRY(r->prof_begin(0, (int64_t)n * mm));
                hipLaunchKernelGGL(k_prep_members<MULTI>, dim3(blocks_for(n), units), dim3(kBlock), 0, s, n, block_of(M), R);
                LF_TRY(r->prof_end());
                ++c.launches;
            }
            auto cones = [&](dim3 grid, const cone_plan_args &C, int64_t cells) {
                LF_TRY(r->prof_begin(2, cells * mm));
                grid.y = (unsigned)units;
                if (r->rplan.cw == 64)
                    hipLaunchKernelGGL((k_sweep_cones_members<FUSED, true, 64, MULTI>), grid, dim3(64), 0, s, C, block_of(M), R);
                else
                    hipLaunchKernelGGL((k_sweep_cones_members<FUSED, true, kBlock, MULTI>), grid, dim3(kBlock), 0, s, C, block_of(M), R);
                return r->prof_end();
            };
            auto level = [&](int first, int cells) {
                LF_TRY(r->prof_begin(1, (int64_t)cells * mm));
                const unsigned nb = (unsigned)level_blocks_for(cells);
                sweep_args_multi B = M;
                bool records = FUSED; // the (a, dx) records: for every router or for none
                for (int i = 0; i < count && records; ++i) records = (B.r[i].adx = level_statics(rs[i], M.r[i])) != nullptr;
                for (int i = count; i < kMaxMulti; ++i) B.r[i].adx = B.r[0].adx;
                if (records)
                    launch_level_members<true, 1, MULTI>(mb, nb, count, mm, s, first, cells, block_of(B), R);
                else
                    launch_level_members<FUSED, 0, MULTI>(mb, nb, count, mm, s, first, cells, block_of(B), R);
                return r->prof_end();
            };
            auto narrow = [&](int k0, int k1) {
                LF_TRY(r->prof_begin(2, (r->h_level_start[k1] - r->h_level_start[k0]) * mm));
                hipLaunchKernelGGL((k_levels_narrow_members<FUSED, true, MULTI>), dim3(units), dim3(kNarrowBlock), 0, s, k0, k1,
                                   r->level_start.p, block_of(M), R);
                return r->prof_end();
            };
            LF_TRY(route_schedule(*r, 0, r->rplan.nblocks(), r->schedule, blocks, c, cones, level, narrow));
        }
        return (int)LF_OK;
    }));
    set_last_stats(count, rs, c);
    return LF_OK;
}

// (the arguments are checked by the caller: lf_router_route_ordered_members)
int route_members(lf_router *r, double *q_dev, const double *lat_dev, int members, int64_t stride, int section)
{
    if (members == 1) return route_device(r, q_dev, lat_dev, section, true);
    LF_TRY(check_plain_call(r, section));
    if (r->N == 0) return LF_OK;
    LF_HIP(hipSetDevice(r->device));
    LF_TRY(enqueue_route_members(1, &r, &q_dev, &lat_dev, members, stride, section));
    LF_HIP(hipGetLastError());
    if (r->profile) LF_TRY(r->prof_collect());
    return LF_OK;
}

} // namespace

// Level blocks for the fused sub-step wavefront (k_fused_cones): runs of consecutive levels of at most `wide` cells are
// cut into blocks of up to lmax levels (fused wavefront: LF_FUSED_LEVELS, default 16; plain router calls, k_sweep_cones:
// LF_ROUTE_LEVELS, default 256; 1 = off); a wider level is a block of its own.  A
// block is cut into cones: chunks of its last level, as long as possible with no level of the cone wider than cw
// cells; a block whose thinnest possible cone (one cell of the last level) is still too wide somewhere loses levels
// until it fits (one level always does).  Nothing is built, and the router's plan stays as it is, when no block holds
// more than one level.
static int build_level_blocks(lf_router *r, const lf_graph *g, bool for_route, int lmax_override = 0)
{
    int lmax = for_route ? 256 : 16; // LF_ROUTE_LEVELS / LF_FUSED_LEVELS (measured: §4.1c / §4.3b of DESIGN.md)
    if (!for_route && !g->has_links) {
        // graphs whose launches all stay chain-bound (the chain / supply cone kernel, k_fused_cones_split, runs them): blocks
        // of 32 levels halve the pipeline fill of that kernel (deep 2000^2: 8.5 -> 7.7 ms per model step); k_fused_cones,
        // which takes the launches of wider graphs, is slower on them (44 vs 31 ms at 5000^2) and keeps 16
        int64_t widest = 0;
        for (int64_t k = 0; k < g->NL; ++k) widest = std::max(widest, g->level_start[k + 1] - g->level_start[k]);
        if (widest <= 3000) lmax = 32;
    }
    // a catchment of a few thousand cells (LF_ETRS89: 2 847 cells, 113 levels): every launch is its own latency, a cone's chain
    // of levels is what it costs, and 8 levels per block balance chain against launch count (model step with structures, ms:
    // 2.29 / 1.96 / 1.96 / 2.20 / 2.96 for 2 / 4 / 8 / 16 / 32 levels per block)
    if (!for_route && g->N <= 65536) lmax = 8;
    const lf_block_knobs knobs = lf_read_block_knobs(for_route, lmax, lmax_override);
    // (the fused cone kernels address a cell by a 32-bit byte offset into its arrays: below 2^29 cells; a larger graph keeps
    // the level-by-level wavefront)
    if (knobs.lmax <= 1 || g->NL < 2 || g->N >= ((int64_t)1 << (for_route ? 31 : 29))) return LF_OK;
    // one wavefront per cone.  Plain calls: no barrier between the levels (deep 10 000^2: 11.3 -> 10.1 ms per call); fused
    // wavefront: the chain / supply kernel needs it (k_fused_cones itself measured the same at 64 and 256: DESIGN.md
    // section 8b)
    int cw = 64;
    if (const char *e = std::getenv(for_route ? "LF_ROUTE_CONE_WIDTH" : "LF_FUSED_CONE_WIDTH"))
        cw = std::atoi(e) == 64 ? 64 : kBlock;
    lf_block_plan plan;
    LF_TRY(lf_build_blocks_guarded([&] {
        // every cell below the last level drains into the next level, so the upstream ranges tile the level before:
        // the first position draining at or behind `pos` is the first upstream position of `pos`
        lf_build_level_blocks(g->level_start, 0, g->NL, knobs.lmax, knobs.wide, cw,
                              [&](int64_t pos) { return (int64_t)g->ups_ptr[pos]; }, plan);
        plan.finish(g->NL);
        if (!for_route && !plan.empty()) plan.index_levels();
    }));
    if (plan.empty()) return LF_OK;
    LF_TRY((for_route ? r->rplan_dev : r->fplan_dev).upload(plan, !for_route, r->ctx->stream));
    (for_route ? r->rplan : r->fplan) = std::move(plan);
    return LF_OK;
}

// ---- levels per block of plain router calls, chosen per graph ------------------------------------------------------------
// Blocks of 256 levels are right for graphs whose cone launches are CHAIN-bound (deep 10 000^2: 157 cones per launch, every
// launch costs its fill + 256 level times whatever the block length, so fewer launches win).  A graph of many short trees --
// the overland graph of a domain with few channel pixels: 4 223 cones of ~100 levels whose ranges are 64 cells wide at one
// level and ~10 on average -- is THROUGHPUT-bound on lanes that idle: a cone must fit its widest level, so the longer the
// block, the thinner the rest of the cone.  Shorter blocks re-cut the cones where the graph narrows (overland 4000^2, 4 %
// channel pixels: 1.43 ms with 256 levels per block, 1.08 / 0.90 / 0.86 / 0.90 / 1.06 with 128 / 64 / 32 / 16 / 8).  Which
// length is best depends on the width profile, so it is MEASURED: when the default plan fills less than 40 % of its lanes
// and has more cones in a launch than the chip holds at once, the candidates are built and timed on scratch vectors (three
// router calls each, hipEvents) and the fastest stays.  Routers of one graph share the result (they must: swept together
// they use one plan).  The plan does not change a single bit of the results (every routing test runs on whatever it picks).
// LF_ROUTE_LEVELS=n fixes the length, LF_ROUTE_TUNE=0 keeps the default.
__global__ void __launch_bounds__(kBlock) k_fill_f64(long long n, double *x, double v)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) x[i] = v;
}

static int tune_route_blocks(lf_router *r, const lf_graph *g)
{
    static std::map<uint64_t, int> tuned; // graph serial -> levels per block (one thread per device context drives this)
    if (std::getenv("LF_ROUTE_LEVELS")) return LF_OK;
    if (const char *e = std::getenv("LF_ROUTE_TUNE"))
        if (e[0] == '0') return LF_OK;
    if (r->rplan.empty() || r->N < 1000000) return LF_OK;
    int64_t st[6];
    LF_TRY(lf_router_route_plan_stats(r, st));
    const double lane_use = st[3] > 0 ? (double)st[4] / ((double)r->rplan.cw * (double)st[3]) : 1.0;
    if (lane_use >= 0.4 || st[5] <= 1024) return LF_OK; // lanes busy, or few enough cones per launch to be chain-bound
    auto it = tuned.find(g->serial);
    if (g->serial != 0 && it != tuned.end()) return it->second == r->rplan.lmax ? LF_OK : build_level_blocks(r, g, true, it->second);
    lf_dbuf<double> Q, q;
    LF_TRY(Q.alloc((size_t)r->N));
    LF_TRY(q.alloc((size_t)r->N));
    hipStream_t s = r->ctx->stream;
    hipEvent_t e0, e1;
    LF_HIP(hipEventCreate(&e0));
    LF_HIP(hipEventCreate(&e1));
    int best = r->rplan.lmax, rc = LF_OK;
    float best_ms = 1e30f;
    for (int lmax : {256, 128, 64, 32, 16}) {
        if (lmax != r->rplan.lmax) rc = build_level_blocks(r, g, true, lmax);
        if (rc != LF_OK || r->rplan.lmax != lmax) break; // (no multi-level block at this length: nothing shorter will have one)
        hipLaunchKernelGGL(k_fill_f64, dim3(blocks_for(r->N)), dim3(kBlock), 0, s, (long long)r->N, Q.p, 1.0);
        hipLaunchKernelGGL(k_fill_f64, dim3(blocks_for(r->N)), dim3(kBlock), 0, s, (long long)r->N, q.p, 1.0e-4);
        rc = route_device(r, Q.p, q.p, 0, true); // warm
        if (rc != LF_OK) break;
        (void)hipEventRecord(e0, s);
        for (int k = 0; k < 3 && rc == LF_OK; ++k) rc = route_device(r, Q.p, q.p, 0, true);
        (void)hipEventRecord(e1, s);
        if (rc != LF_OK || hipEventSynchronize(e1) != hipSuccess) break;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (ms < best_ms) {
            best_ms = ms;
            best = lmax;
        } else if (ms > 1.15f * best_ms)
            break; // past the minimum
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc == LF_OK && r->rplan.lmax != best) rc = build_level_blocks(r, g, true, best);
    if (rc == LF_OK && g->serial != 0) tuned[g->serial] = best;
    return rc;
}

extern "C" {

int lf_router_create(const lf_graph *g, const double *alpha, double beta, const double *dx, double dx_scalar, double dt,
                     const double *alpha_floodplains, int device, lf_router **out)
{
    if (!g || !alpha || !out) return lf_set_error(LF_E_INVALID, "null argument");
    lf_device_ctx *ctx;
    LF_TRY(lf_ctx(device, &ctx));
    lf_router *r = new lf_router();
    r->NL = g->NL;
    r->graph_serial = g->serial; // routers swept together (cone plan and upstream ranges of router 0) must share the graph
    const int64_t n = g->N;
    const std::vector<int32_t> &g_perm = g->perm;
    int rc = router_core_init(*r, device, ctx, n, g->K, beta, dx_scalar, dt, g_perm, g->ups_ptr, alpha, alpha_floodplains, dx,
                              ctx->stream);
    if (rc == LF_OK && g->has_links) rc = r->linked.upload(g->linked.data(), n, ctx->stream);
    if (rc == LF_OK && g->has_links) {
        std::vector<int> parked((size_t)g->NL, 0);
        for (int64_t k = 0; k < g->NL; ++k)
            for (int64_t p = g->level_start[k]; p < g->level_start[k + 1]; ++p) parked[k] += g->linked[p] ? 1 : 0;
        rc = r->level_nlinked.upload(parked.data(), parked.size(), ctx->stream);
    }
    if (rc == LF_OK && n > 0) {
        std::vector<uint8_t> has_up(n, 0), iso(n, 0);
        for (int64_t p = 0; p < n; ++p)
            if (g->down[p] >= 0) has_up[g->down[p]] = 1;
        for (int64_t p = 0; p < n; ++p) {
            const int32_t pix = g_perm[p];
            iso[p] = (g->down[pix] < 0 && !has_up[pix] && !(g->has_links && g->linked[p])) ? 1 : 0;
            r->n_isolated += iso[p];
        }
        if (r->n_isolated > 0) rc = r->isolated.upload(iso.data(), n, ctx->stream);
    }
    if (rc == LF_OK) rc = router_core_init_levels(*r, g->level_start, ctx->stream);
    if (rc == LF_OK) rc = r->qord.alloc(n);
    if (rc == LF_OK) rc = r->counter.alloc(1);
    if (rc != LF_OK) {
        delete r;
        return rc;
    }
    r->schedule = level_segments(g->level_start, 0, g->NL);
    // (zero-length structure links need nothing special: such cells sit at the end of their level, inside the upstream
    // range of the LAST cell of the next level -- which adds their 0.0 -- and so inside the last cone of a block)
    rc = build_level_blocks(r, g, false);
    if (rc == LF_OK && !g->has_links) rc = build_level_blocks(r, g, true);
    if (rc == LF_OK && !g->has_links) rc = tune_route_blocks(r, g);
    if (rc != LF_OK) {
        delete r;
        return rc;
    }
    *out = r;
    return LF_OK;
}

void lf_router_destroy(lf_router *r)
{
    if (!r) return;
    (void)hipSetDevice(r->device);
    (void)hipStreamSynchronize(r->ctx->stream);
    delete r;
}

int lf_router_route_device(lf_router *r, double *discharge_dev, const double *lateral_dev, int section)
{
    if (!r || !discharge_dev || !lateral_dev) return lf_set_error(LF_E_INVALID, "null argument");
    return route_device(r, discharge_dev, lateral_dev, section);
}

// Several routers with the same level schedule (built on one lf_graph: e.g. the three overland routers of
// surface_routing.py:108-113, which differ in alpha only) swept together, one launch per level for all of them.  Routers
// whose schedules differ are swept one after the other.  engine_order != 0: the vectors
// are resident in the routers' sweep order (lf_router_route_ordered), else in pixel order (lf_router_route_device).
int lf_router_route_device_multi(int count, lf_router **routers, double **discharge_dev, const double **lateral_dev,
                                 int section, int engine_order)
{
    if (count < 1 || !routers || !discharge_dev || !lateral_dev) return lf_set_error(LF_E_INVALID, "null argument");
    for (int i = 0; i < count; ++i)
        if (!routers[i] || !discharge_dev[i] || !lateral_dev[i]) return lf_set_error(LF_E_INVALID, "null argument");
    LF_TRY(check_section(*routers[0], section)); // (the other routers are checked where they are not swept together)
    bool together = count <= kMaxMulti && swept_together(count, routers);
    for (int i = 0; i < count && together; ++i) together = section == LF_SECTION_MAIN || routers[i]->has_floodplains;
    if (!together) {
        for (int i = 0; i < count; ++i)
            LF_TRY(route_device(routers[i], discharge_dev[i], lateral_dev[i], section, engine_order != 0));
        return LF_OK;
    }
    LF_HIP(hipSetDevice(routers[0]->device));
    LF_TRY(enqueue_route(count, routers, discharge_dev, lateral_dev, section, engine_order != 0));
    LF_HIP(hipGetLastError());
    return LF_OK;
}

int lf_router_route_ordered(lf_router *r, double *discharge_ord_dev, const double *lateral_ord_dev, int section)
{
    if (!r || !discharge_ord_dev || !lateral_ord_dev) return lf_set_error(LF_E_INVALID, "null argument");
    return route_device(r, discharge_ord_dev, lateral_ord_dev, section, true);
}

// An ensemble on one router: `members` discharge / lateral-inflow rows that share r's static vectors and schedule, one
// launch per wide level, narrow run or level block for all of them (enqueue_route_members).  The arguments are checked
// before r or a device is touched as far as they can be.
int lf_router_route_ordered_members(lf_router *r, double *discharge_ord_dev, const double *lateral_ord_dev, int members,
                                    int64_t stride, int section)
{
    if (members < 1) return lf_set_error(LF_E_INVALID, "members must be at least 1 (got %d)", members);
    if (stride < 0) return lf_set_error(LF_E_INVALID, "stride %lld is less than the router's number of cells", (long long)stride);
    if (!r || !discharge_ord_dev || !lateral_ord_dev) return lf_set_error(LF_E_INVALID, "null argument");
    if (stride < r->N)
        return lf_set_error(LF_E_INVALID, "stride %lld is less than the router's number of cells (%lld)", (long long)stride,
                            (long long)r->N);
    return route_members(r, discharge_ord_dev, lateral_ord_dev, members, stride, section);
}

// An ensemble on `count` routers: router i sweeps its own `members` rows of discharge_ord_dev[i] / lateral_ord_dev[i].
// Routers that may be swept together (swept_together) get one launch per wide level, narrow run or level block
// for all count * members units (enqueue_route_members); others one member call each.  The arguments are checked
// before a router or a device is touched.
int lf_router_route_ordered_members_multi(int count, lf_router **routers, double **discharge_ord_dev,
                                          const double **lateral_ord_dev, int members, int64_t stride, int section)
{
    if (count < 1 || count > kMaxMulti) return lf_set_error(LF_E_INVALID, "count must be 1 to %d (got %d)", kMaxMulti, count);
    if (members < 1) return lf_set_error(LF_E_INVALID, "members must be at least 1 (got %d)", members);
    if (stride < 0) return lf_set_error(LF_E_INVALID, "stride %lld is less than the router's number of cells", (long long)stride);
    if (!routers || !discharge_ord_dev || !lateral_ord_dev) return lf_set_error(LF_E_INVALID, "null argument");
    for (int i = 0; i < count; ++i)
        if (!routers[i] || !discharge_ord_dev[i] || !lateral_ord_dev[i]) return lf_set_error(LF_E_INVALID, "null argument");
    for (int i = 0; i < count; ++i) {
        if (stride < routers[i]->N)
            return lf_set_error(LF_E_INVALID, "stride %lld is less than the number of cells of router %d (%lld)", (long long)stride, i,
                                (long long)routers[i]->N);
    }
    for (int i = 0; i < count; ++i) LF_TRY(check_plain_call(routers[i], section));
    if (!swept_together(count, routers)) {
        for (int i = 0; i < count; ++i)
            LF_TRY(route_members(routers[i], discharge_ord_dev[i], lateral_ord_dev[i], members, stride, section));
        return LF_OK;
    }
    if (members == 1) return lf_router_route_device_multi(count, routers, discharge_ord_dev, lateral_ord_dev, section, 1);
    if (routers[0]->N == 0) return LF_OK;
    LF_HIP(hipSetDevice(routers[0]->device));
    LF_TRY(enqueue_route_members(count, routers, discharge_ord_dev, lateral_ord_dev, members, stride, section));
    LF_HIP(hipGetLastError());
    return LF_OK;
}

// ... from host arrays in pixel order: up, every row into sweep order, the member call, back (staging kept with r)
int lf_router_route_members_host(lf_router *r, double *discharge_host, const double *lateral_host, int members, int section)
{
    if (members < 1) return lf_set_error(LF_E_INVALID, "members must be at least 1 (got %d)", members);
    if (!r || !discharge_host || !lateral_host) return lf_set_error(LF_E_INVALID, "null argument");
    LF_TRY(check_plain_call(r, section));
    if (r->N == 0) return LF_OK;
    LF_HIP(hipSetDevice(r->device));
    hipStream_t s = r->ctx->stream;
    const size_t n = (size_t)r->N, total = n * (size_t)members, bytes = sizeof(double) * total;
    if (r->members_pix.n < 2 * total || r->members_ord.n < 2 * total) { // (each is whole whether or not the other grew)
        LF_HIP(hipStreamSynchronize(s));
        if (r->members_pix.n < 2 * total) LF_TRY(r->members_pix.grow(2 * total));
        if (r->members_ord.n < 2 * total) LF_TRY(r->members_ord.grow(2 * total));
    }
    double *q_pix = r->members_pix.p, *lat_pix = q_pix + total, *q_ord = r->members_ord.p, *lat_ord = q_ord + total;
    LF_HIP(hipMemcpyAsync(q_pix, discharge_host, bytes, hipMemcpyHostToDevice, s));
    LF_HIP(hipMemcpyAsync(lat_pix, lateral_host, bytes, hipMemcpyHostToDevice, s));
    for (size_t m = 0; m < (size_t)members; ++m) {
        LF_TRY(core_to_engine_order(*r, q_pix + m * n, q_ord + m * n));
        LF_TRY(core_to_engine_order(*r, lat_pix + m * n, lat_ord + m * n));
    }
    LF_TRY(route_members(r, q_ord, lat_ord, members, (int64_t)n, section));
    for (size_t m = 0; m < (size_t)members; ++m) LF_TRY(core_from_engine_order(*r, q_ord + m * n, q_pix + m * n));
    LF_HIP(hipMemcpyAsync(discharge_host, q_pix, bytes, hipMemcpyDeviceToHost, s));
    LF_HIP(hipStreamSynchronize(s));
    return LF_OK;
}

// dst[i] = src[index[i]] for i < n (device vectors; index is int32): the permutation between two domains, e.g. a
// full-raster pixel vector into the engine order of a router that covers only a subset of the pixels
int lf_gather_device(int device, int64_t n, const int32_t *index_dev, const double *src_dev, double *dst_dev)
{
    if (n < 0 || (n > 0 && (!index_dev || !src_dev || !dst_dev))) return lf_set_error(LF_E_INVALID, "bad argument");
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    if (n > 0)
        hipLaunchKernelGGL(k_gather, dim3(blocks_for(n)), dim3(kBlock), 0, c->stream, (int)n, (const int *)index_dev, src_dev,
                           dst_dev);
    LF_HIP(hipGetLastError());
    return LF_OK;
}

int lf_gather_rows_device(int device, int64_t n, const int32_t *index_dev, const double *src_dev, int64_t src_stride,
                          double *dst_dev, int64_t dst_stride, int rows)
{
    if (rows < 1) return lf_set_error(LF_E_INVALID, "rows must be at least 1 (got %d)", rows);
    if (n < 0 || n > 0x7fffffffll) return lf_set_error(LF_E_INVALID, "n = %lld outside the 32-bit range of a launch", (long long)n);
    if (dst_stride < n) return lf_set_error(LF_E_INVALID, "dst_stride %lld is less than n = %lld", (long long)dst_stride, (long long)n);
    if (src_stride < 0) return lf_set_error(LF_E_INVALID, "src_stride %lld is negative", (long long)src_stride);
    if (n > 0 && (!index_dev || !src_dev || !dst_dev)) return lf_set_error(LF_E_INVALID, "null argument");
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    for (int r0 = 0; r0 < rows && n > 0; r0 += kMaxGridY) // (one launch unless there are more rows than a grid has)
        hipLaunchKernelGGL(k_gather_rows, dim3(blocks_for(n), (unsigned)std::min(rows - r0, kMaxGridY)), dim3(kBlock), 0, c->stream, (int)n,
                           (const int *)index_dev, src_dev + (int64_t)r0 * src_stride, src_stride, dst_dev + (int64_t)r0 * dst_stride,
                           dst_stride);
    LF_HIP(hipGetLastError());
    return LF_OK;
}

int lf_router_to_engine_order(lf_router *r, const double *src_pix_dev, double *dst_ord_dev)
{
    if (!r || !src_pix_dev || !dst_ord_dev) return lf_set_error(LF_E_INVALID, "null argument");
    return core_to_engine_order(*r, src_pix_dev, dst_ord_dev);
}

int lf_router_from_engine_order(lf_router *r, const double *src_ord_dev, double *dst_pix_dev)
{
    if (!r || !src_ord_dev || !dst_pix_dev) return lf_set_error(LF_E_INVALID, "null argument");
    return core_from_engine_order(*r, src_ord_dev, dst_pix_dev);
}

int lf_router_route_host(lf_router *r, double *discharge_host, const double *lateral_host, int section)
{
    if (!r || !discharge_host || !lateral_host) return lf_set_error(LF_E_INVALID, "null argument");
    LF_TRY(check_section(*r, section));
    LF_HIP(hipSetDevice(r->device));
    const size_t bytes = sizeof(double) * (size_t)r->N;
    if (!r->io_q.p) LF_TRY(r->io_q.alloc(r->N));
    if (!r->io_lat.p) LF_TRY(r->io_lat.alloc(r->N));
    hipStream_t s = r->ctx->stream;
    if (bytes) {
        LF_HIP(hipMemcpyAsync(r->io_q.p, discharge_host, bytes, hipMemcpyHostToDevice, s));
        LF_HIP(hipMemcpyAsync(r->io_lat.p, lateral_host, bytes, hipMemcpyHostToDevice, s));
    }
    LF_TRY(route_device(r, r->io_q.p, r->io_lat.p, section));
    if (bytes) LF_HIP(hipMemcpyAsync(discharge_host, r->io_q.p, bytes, hipMemcpyDeviceToHost, s));
    LF_HIP(hipStreamSynchronize(s));
    return LF_OK;
}

int lf_count_nonfinite(int device, const double *x_dev, int64_t n, int64_t *count)
{
    if (!x_dev || !count) return lf_set_error(LF_E_INVALID, "null argument");
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    lf_dbuf<unsigned long long> ctr;
    LF_TRY(ctr.alloc(1));
    LF_HIP(hipMemsetAsync(ctr.p, 0, sizeof(unsigned long long), c->stream));
    if (n > 0) {
        const int grid = (int)std::min<int64_t>((n + kBlock - 1) / kBlock, 2048);
        hipLaunchKernelGGL(k_count_nonfinite, dim3(grid), dim3(kBlock), 0, c->stream, (long long)n, x_dev, ctr.p);
    }
    unsigned long long h = 0;
    LF_HIP(hipMemcpyAsync(&h, ctr.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    LF_HIP(hipStreamSynchronize(c->stream));
    *count = (int64_t)h;
    return LF_OK;
}

int lf_router_device(const lf_router *r) { return r ? r->device : -1; }
int64_t lf_router_num_pixels(const lf_router *r) { return r ? r->N : -1; }

int lf_router_last_fused_form(const lf_router *r) { return r ? r->last_fused_form : -1; }

int lf_router_last_launches(const lf_router *r, int64_t stats[4])
{
    if (!r || !stats) return lf_set_error(LF_E_INVALID, "null argument");
    for (int i = 0; i < 4; ++i) stats[i] = r->last_stats[i];
    return LF_OK;
}

// Shape of the block plan of single router calls (build_level_blocks): how full the cone wavefronts are.
int lf_router_route_plan_stats(const lf_router *r, int64_t out[6])
{
    if (!r || !out) return lf_set_error(LF_E_INVALID, "null argument");
    r->rplan.stats(r->h_level_start, out);
    return LF_OK;
}

// The fused-with-structures call checks and plans the site lists once per set of device pointers (fused_site_cache); a
// caller that rebuilds its site lists (possibly at the same addresses) drops that cache here.
int lf_router_reset_site_cache(lf_router *r)
{
    if (!r) return lf_set_error(LF_E_INVALID, "null argument");
    r->sites.reset();
    return LF_OK;
}

int lf_router_profile_enable(lf_router *r, int on)
{
    if (!r) return lf_set_error(LF_E_INVALID, "null argument");
    r->profile = on != 0;
    return LF_OK;
}

int lf_router_profile_read(lf_router *r, double out[9], int reset)
{
    if (!r || !out) return lf_set_error(LF_E_INVALID, "null argument");
    for (int i = 0; i < 9; ++i) out[i] = r->prof_acc[i];
    if (reset)
        for (int i = 0; i < 9; ++i) r->prof_acc[i] = 0;
    return LF_OK;
}

int lf_upstream_sum_device(lf_router *r, const double *w_dev, double *out_dev)
{
    if (!r || !w_dev || !out_dev) return lf_set_error(LF_E_INVALID, "null argument");
    LF_HIP(hipSetDevice(r->device));
    const int n = (int)r->N;
    if (n > 0)
        hipLaunchKernelGGL(k_upstream_sum, dim3(blocks_for(n)), dim3(kBlock), 0, r->ctx->stream, n, r->perm.p,
                           r->ups_ptr.p, w_dev, out_dev, (const uint8_t *)r->linked.p);
    LF_HIP(hipGetLastError());
    return LF_OK;
}

int lf_upstream_sum_host(lf_router *r, const double *w_host, double *out_host)
{
    if (!r || !w_host || !out_host) return lf_set_error(LF_E_INVALID, "null argument");
    LF_HIP(hipSetDevice(r->device));
    const size_t bytes = sizeof(double) * (size_t)r->N;
    if (!r->io_q.p) LF_TRY(r->io_q.alloc(r->N));
    if (!r->io_lat.p) LF_TRY(r->io_lat.alloc(r->N));
    hipStream_t s = r->ctx->stream;
    if (bytes) LF_HIP(hipMemcpyAsync(r->io_lat.p, w_host, bytes, hipMemcpyHostToDevice, s));
    LF_TRY(lf_upstream_sum_device(r, r->io_lat.p, r->io_q.p));
    if (bytes) LF_HIP(hipMemcpyAsync(out_host, r->io_q.p, bytes, hipMemcpyDeviceToHost, s));
    LF_HIP(hipStreamSynchronize(s));
    return LF_OK;
}

// accuflux over engine-order device vectors: acc[p] = x[p] + sum of acc over the upstream cells; nv (<= 4) vectors in
// one sweep.  On the level layout it runs on the router's block plan (blocks of up to 64 levels cone by cone through
// LDS, single wide levels one launch each), like a router call.
int lf_accuflux_ordered_multi_device(lf_router *r, int nv, const double *const *x_ord_dev, double *const *acc_ord_dev)
{
    if (!r || !x_ord_dev || !acc_ord_dev || nv < 1 || nv > kMaxAccu) return lf_set_error(LF_E_INVALID, "bad argument");
    for (int v = 0; v < nv; ++v)
        if (!x_ord_dev[v] || !acc_ord_dev[v]) return lf_set_error(LF_E_INVALID, "null argument");
    if (r->linked.p) return lf_set_error(LF_E_INVALID, "accuflux is not defined on a graph with structure links");
    LF_HIP(hipSetDevice(r->device));
    hipStream_t s = r->ctx->stream;
    if (r->N == 0) return LF_OK;
    accu_multi M;
    for (int v = 0; v < kMaxAccu; ++v) {
        M.x[v] = x_ord_dev[v < nv ? v : 0];
        M.acc[v] = acc_ord_dev[v < nv ? v : 0];
    }
    launch_counts c;
    LF_TRY(pick_count(nv, [&](auto nvc) {
        constexpr int NV = nvc;
        auto cones = [&](dim3 grid, const cone_plan_args &C, int64_t) {
            if (r->rplan.cw == 64)
                hipLaunchKernelGGL((k_accu_cones<NV, 64>), grid, dim3(64), 0, s, C, r->ups_ptr.p, M);
            else
                hipLaunchKernelGGL((k_accu_cones<NV, kBlock>), grid, dim3(kBlock), 0, s, C, r->ups_ptr.p, M);
            return LF_OK;
        };
        auto level = [&](int first, int cells) {
            hipLaunchKernelGGL(k_accu_level<NV>, dim3(blocks_for(cells)), dim3(kBlock), 0, s, first, cells, r->ups_ptr.p, M);
            return LF_OK;
        };
        auto narrow = [&](int k0, int k1) {
            hipLaunchKernelGGL(k_accu_narrow<NV>, dim3(1), dim3(kNarrowBlock), 0, s, k0, k1, r->level_start.p, r->ups_ptr.p, M);
            return LF_OK;
        };
        return route_schedule(*r, 0, r->rplan.nblocks(), r->schedule, !r->rplan.empty(), c, cones, level, narrow);
    }));
    r->last_stats[0] = c.launches;
    r->last_stats[1] = r->last_stats[2] = 0;
    r->last_stats[3] = r->NL;
    LF_HIP(hipGetLastError());
    return LF_OK;
}

int lf_accuflux_ordered_device(lf_router *r, const double *x_ord_dev, double *acc_ord_dev)
{
    const double *x[1] = {x_ord_dev};
    double *acc[1] = {acc_ord_dev};
    return lf_accuflux_ordered_multi_device(r, 1, x, acc);
}

int lf_accuflux_host(lf_router *r, const double *x_host, double *out_host)
{
    if (!r || !x_host || !out_host) return lf_set_error(LF_E_INVALID, "null argument");
    if (r->linked.p) return lf_set_error(LF_E_INVALID, "accuflux is not defined on a graph with structure links");
    LF_HIP(hipSetDevice(r->device));
    const int n = (int)r->N;
    const size_t bytes = sizeof(double) * (size_t)r->N;
    if (!r->io_q.p) LF_TRY(r->io_q.alloc(r->N));
    if (!r->io_lat.p) LF_TRY(r->io_lat.alloc(r->N));
    if (!r->tmp_ord.p) LF_TRY(r->tmp_ord.alloc(r->N));
    hipStream_t s = r->ctx->stream;
    if (n == 0) return LF_OK;
    LF_HIP(hipMemcpyAsync(r->io_lat.p, x_host, bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_gather, dim3(blocks_for(n)), dim3(kBlock), 0, s, n, r->perm.p, r->io_lat.p, r->tmp_ord.p);
    LF_TRY(lf_accuflux_ordered_device(r, r->tmp_ord.p, r->qord.p));
    hipLaunchKernelGGL(k_scatter, dim3(blocks_for(n)), dim3(kBlock), 0, s, n, r->perm.p, r->qord.p, r->io_q.p);
    LF_HIP(hipGetLastError());
    LF_HIP(hipMemcpyAsync(out_host, r->io_q.p, bytes, hipMemcpyDeviceToHost, s));
    LF_HIP(hipStreamSynchronize(s));
    return LF_OK;
}

} // extern "C"

// accessors for lf_ldd.hip (the router struct is private to this file)
struct lf_router_view {
    int device;
    lf_device_ctx *ctx;
    int64_t N;
    const int32_t *perm, *ups_ptr;
    const uint8_t *linked;
    int32_t **parent_slot;
    int32_t **root_slot;
};

int lf_router_view_of(lf_router *r, lf_router_view *v)
{
    if (!r || !v) return lf_set_error(LF_E_INVALID, "null argument");
    LF_HIP(hipSetDevice(r->device));
    v->device = r->device;
    v->ctx = r->ctx;
    v->N = r->N;
    v->perm = r->perm.p;
    v->ups_ptr = r->ups_ptr.p;
    v->linked = r->linked.p;
    v->parent_slot = &r->parent.p;
    v->root_slot = &r->root.p;
    return LF_OK;
}

int lf_router_alloc_root(lf_router *r)
{
    if (!r) return lf_set_error(LF_E_INVALID, "null argument");
    return r->root.p ? LF_OK : r->root.alloc((size_t)r->N);
}

// (a root table whose contents never arrived must not be trusted by later calls)
int lf_router_drop_root(lf_router *r)
{
    if (!r) return lf_set_error(LF_E_INVALID, "null argument");
    r->root.release();
    return LF_OK;
}

// grow-only scratch of the catchment totals (count doubles)
int lf_router_totals_scratch(lf_router *r, size_t count, double **p)
{
    if (!r || !p) return lf_set_error(LF_E_INVALID, "null argument");
    if (r->totals_scratch.n < count) {
        LF_HIP(hipStreamSynchronize(r->ctx->stream));
        LF_TRY(r->totals_scratch.alloc(count));
    }
    *p = r->totals_scratch.p;
    return LF_OK;
}

int lf_router_alloc_parent(lf_router *r)
{
    if (!r) return lf_set_error(LF_E_INVALID, "null argument");
    return r->parent.p ? LF_OK : r->parent.alloc((size_t)r->N);
}

// ================================================================================================
// routing.dynamic() sub-step: element-wise arithmetic around the router calls (routing.py:512-603,
// 693-703), fused into three kernels so that a model step's NoRoutSteps x (1..2) router calls never
// leave the device.
// ================================================================================================
namespace {

// routing.py:512 (+524 in the single branch) and, for split routing, 549-567
__global__ void __launch_bounds__(kBlock) k_substep_sideflow(int n, lf_substep_args A)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    double side = A.IsChannelKinematic[p] ? A.SideflowChanM3[p] * A.InvChanLength[p] * A.InvDtRouting : 0.0;
    if (!A.split) {
        if (isnan(side)) side = 0.0; // :524
        A.scratch0[p] = side;
        return;
    }
    const double m3 = A.ChanM3Kin[p], m3_2 = A.Chan2M3Kin[p];
    const double tot = m3 + m3_2;
    const double ratio = (tot > 0) ? m3 / tot : 0.0;                                  // :549
    double s1 = ((tot - A.Chan2M3Start[p]) > A.M3Limit[p]) ? ratio * side : side;     // :557-558
    if (fabs(side) < 1e-7) s1 = side;                                                 // :563
    A.Sideflow1Chan[p] = s1;
    A.scratch0[p] = s1;
    A.scratch1[p] = (side - s1) + A.Chan2QStart[p] * A.InvChanLength[p];              // :565-567
}

__device__ __forceinline__ void velocity(const lf_substep_args &A, int p, double m3, double q)
{
    double area = m3 * A.InvChanLength[p]; // :693
    if (area < 0.01) area = 0.01;
    const double v1 = q / area, v2 = 0.36 * pow(q, 0.24);
    double v = (v2 < v1) ? v2 : v1; // np.minimum, NaN propagates
    if (isnan(v2)) v = v2;
    double sinu = sqrt(A.PixelArea[p]) * A.InvChanLength[p];
    if (sinu > 1) sinu = 1;
    v *= sinu;
    A.FlowVelocity[p] = v;
    A.TravelDistance[p] = v * A.DtSec;
}

// routing.py:527-538 (single) / 574-578 (split, main channel)
__global__ void __launch_bounds__(kBlock) k_substep_main(int n, lf_substep_args A)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const bool b35 = A.Beta == 0.6;
    double v = A.ChanLength[p] * A.ChannelAlpha[p] * (b35 ? lf_pow_3_5(A.ChanQKin[p]) : pow(A.ChanQKin[p], A.Beta));
    if (v < 0.0) v = 0.0;
    const double x = v * A.InvChanLength[p] * A.InvChannelAlpha[p];
    const double q = b35 ? lf_pow_5_3(x) : pow(x, A.InvBeta);
    A.ChanM3Kin[p] = v;
    A.ChanQKin[p] = q;
    if (!A.split) {
        A.ChanQ[p] = q;
        A.sumDisDay[p] += q;
        velocity(A, p, v, q);
    }
}

// routing.py:584-603 + 693-703
__global__ void __launch_bounds__(kBlock) k_substep_floodplain(int n, lf_substep_args A)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const double start = A.Chan2M3Start[p];
    const bool b35 = A.Beta == 0.6;
    double v = A.ChanLength[p] * A.ChannelAlpha2[p] * (b35 ? lf_pow_3_5(A.Chan2QKin[p]) : pow(A.Chan2QKin[p], A.Beta));
    if ((v - start) < 0.0) v = start;
    A.Chan2M3Kin[p] = v;
    A.CrossSection2Area[p] = (v - start) * A.InvChanLength[p];
    const double x2 = v * A.InvChanLength[p] * A.InvChannelAlpha2[p];
    const double q2 = b35 ? lf_pow_5_3(x2) : pow(x2, A.InvBeta);
    A.Chan2QKin[p] = q2;
    const double q1 = A.ChanQKin[p];
    double q = q1 + q2 - A.QLimit[p];
    if (q < 0.0) q = 0.0; // np.maximum(q, 0.0), NaN propagates
    A.ChanQ[p] = q;
    A.sumDisDay[p] += q;
    velocity(A, p, A.ChanM3Kin[p], q1);
}

} // namespace

// The three element-wise stages of a sub-step on their own (stage 0: sideflow assembly, 1: main-channel fix-up and
// discharge sums, 2: floodplain fix-up), for callers that run the router calls in between themselves -- the row-block
// partition (lf_dist_routing_substep) does, with halo exchanges inside each router call.
extern "C" int lf_substep_stage(int device, int stage, int64_t n, const lf_substep_args *a)
{
    if (!a || stage < 0 || stage > 2 || n < 0) return lf_set_error(LF_E_INVALID, "bad argument");
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    if (n == 0) return LF_OK;
    const dim3 grid(blocks_for(n)), block(kBlock);
    if (stage == 0)
        hipLaunchKernelGGL(k_substep_sideflow, grid, block, 0, c->stream, (int)n, *a);
    else if (stage == 1)
        hipLaunchKernelGGL(k_substep_main, grid, block, 0, c->stream, (int)n, *a);
    else
        hipLaunchKernelGGL(k_substep_floodplain, grid, block, 0, c->stream, (int)n, *a);
    LF_HIP(hipGetLastError());
    return LF_OK;
}

extern "C" int lf_routing_substep(lf_router *r, const lf_substep_args *a)
{
    if (!r || !a) return lf_set_error(LF_E_INVALID, "null argument");
    if (a->split && !r->has_floodplains)
        return lf_set_error(LF_E_SECTION, "split routing requested but the router has no floodplain alpha");
    if (r->linked.p)
        return lf_set_error(LF_E_INVALID, "a router on a graph with structure links runs only lf_routing_substeps_fused*");
    LF_HIP(hipSetDevice(r->device));
    hipStream_t s = r->ctx->stream;
    const int n = (int)r->N;
    if (n == 0) return LF_OK;
    const dim3 grid(blocks_for(n)), block(kBlock);
    hipLaunchKernelGGL(k_substep_sideflow, grid, block, 0, s, n, *a);
    const bool ordered = a->engine_order != 0;
    LF_TRY(route_device(r, a->ChanQKin, a->scratch0, LF_SECTION_MAIN, ordered));
    hipLaunchKernelGGL(k_substep_main, grid, block, 0, s, n, *a);
    if (a->split) {
        LF_TRY(route_device(r, a->Chan2QKin, a->scratch1, LF_SECTION_FLOODPLAINS, ordered));
        hipLaunchKernelGGL(k_substep_floodplain, grid, block, 0, s, n, *a);
    }
    LF_HIP(hipGetLastError());
    return LF_OK;
}

// ================================================================================================
// Fused multi-sub-step routing: the NoRoutSteps sub-steps of a model step (Lisflood_dynamic.py:179-180) as ONE
// skewed wavefront.  Sub-step s+1 of a cell needs only the cell's own state after sub-step s and the
// sub-step-(s+1) router output of its upstream cells (one level up), so launch t processes every (level k,
// sub-step s) with k + s = t: NL + S - 1 launches instead of S x (1..2) x NL, each S times wider.  Router
// outputs live in two parity buffers per section (sub-step s writes buffer s&1, which sub-step s+2 may only
// overwrite one launch after its last reader).  Arithmetic per cell is exactly that of lf_routing_substep, so
// the result is bit-identical to S sequential sub-steps.  Valid when the sideflow of every sub-step is known
// up front (stride 0: the same vector for all sub-steps, as in the model when no lake / reservoir sits in the
// loop; stride N: one vector per sub-step).
// ================================================================================================
#include "lf_fused.h"

namespace {

void fused_set_stats(lf_router *r, int64_t launches) // what lf_router_last_launches tells of a fused call
{
    r->last_stats[0] = r->last_stats[1] = launches;
    r->last_stats[2] = 0;
    r->last_stats[3] = r->NL;
}

// Structures in the loop: I = the caller's block `in` (an ensemble's: member 0's) as the kernels read it, its site lists
// checked and planned once per set of lists (r->sites).  sc: the site cache of the call -- r->sites, or an empty one for a
// call without structures (in null, I untouched) or without a site: the schedules as with sites, none of them found.
int fused_inloop_of(lf_router *r, const lf_substep_args &a, const lf_inloop_args *in, lf_inloop_args &I, hipStream_t s,
                    const fused_site_cache *&sc)
{
    static const fused_site_cache no_sites;
    sc = &no_sites;
    if (!in) return LF_OK;
    I = *in;
    if (I.n_lakes <= 0) {
        I.n_lakes = 0;
        I.QLakeOutM3Dt = nullptr;
    }
    if (I.n_res <= 0) {
        I.n_res = 0;
        I.QResOutM3Dt = nullptr;
    }
    if (!I.ToChanM3RunoffDt || !I.SideflowChanM3 || I.N != r->N)
        return lf_set_error(LF_E_INVALID, "lf_inloop_args: ToChanM3RunoffDt, SideflowChanM3 and N = num_pixels are needed");
    I.ChanQ = a.ChanQ;
    LF_TRY(r->sites.ensure(r->N, r->h_level_start, r->linked.p, I, s));
    if (I.n_lakes + I.n_res > 0) sc = &r->sites;
    return LF_OK;
}

// A fused call on the single domain: check, sites, flags, pick the schedule, run.
// flags_ready: see fused_statics_flags (fused_ensemble_impl)
int fused_impl(lf_router *r, const lf_substep_args *a, int nsteps, int64_t sideflow_stride, const lf_inloop_args *in,
               int msteps = 0, int64_t side_mstride = 0, bool flags_ready = false)
{
    if (!r || !a || nsteps < 1) return lf_set_error(LF_E_INVALID, "bad argument");
    LF_TRY(fused_check_call(*r, *a, sideflow_stride, "fused sub-step wavefront needs"));
    if (msteps <= 0) msteps = nsteps; // one model step
    if (nsteps % msteps != 0) return lf_set_error(LF_E_INVALID, "the sub-step count must be a multiple of the sub-steps per model step");
    if (msteps != nsteps && (in || sideflow_stride != 0 || (side_mstride != 0 && side_mstride < r->N)))
        return lf_set_error(LF_E_INVALID, "several model steps per call: no structures, one sideflow vector per model step "
                                          "(stride 0 or >= N)");
    LF_HIP(hipSetDevice(r->device));
    const int64_t n = r->N;
    if (n == 0) return LF_OK;
    LF_TRY(fused_parity_ensure(*r, a->split != 0, (size_t)n));
    fused_args F = fused_args_of(*r, *a, nsteps, msteps, sideflow_stride, side_mstride);
    F.linked = r->linked.p;
    F.level_nlinked = r->level_nlinked.p;
    F.fb_lvl2blk = r->fplan_dev.lvl2blk.p;
    hipStream_t s = r->ctx->stream;
    const fused_site_cache *sites_of = nullptr;
    LF_TRY(fused_inloop_of(r, *a, in, F.I, s, sites_of));
    const fused_site_cache &sc = *sites_of;
    const int64_t nsites = F.I.n_lakes + F.I.n_res;
    F.site_level = sc.site_level.p;
    // time-major: without structures on a graph without links; with them when the site plan applies (no site: nothing to plan)
    const bool time_major = in ? nsites == 0 || sc.applies : !F.linked;
    int64_t launches = 0;
    const bool tm_struct = in && time_major && fused_time_major_ready(*r, 0, (int)r->NL, nsteps, a->split != 0);
    LF_TRY(fused_statics_flags(*r, F, in != nullptr, tm_struct, flags_ready, s, launches));
    const bool all35 = r->fused && a->Beta == 0.6; // otherwise: run-time flags and inlined OCML pow, as fused_cell
    auto cones = [&](int64_t ncones) {
        const dim3 grid((unsigned)ncones);
        // The chain / supply form (lf_fused.h: k_fused_cones_split) where it applies and where the launch is chain-bound: up
        // to ~1100 cones in flight (24 sub-steps x 2900 cells per level) it is 1.1 - 1.7 x faster, beyond that the launch is
        // bound by throughput (three wavefronts and 31 KB of LDS per cone) and the one-wavefront kernel wins (DESIGN.md
        // section 4.3b; deep 2000^2, ~860 cones: 7.7 vs 8.7 ms per model step, 3000^2, ~1220: 15.9 vs 14.5).
        // LF_FUSED_SPLIT=0 / 1: never / always (A/B switch).
        static const int64_t split_max = [] {
            const char *e = std::getenv("LF_FUSED_SPLIT_MAX");
            return e ? std::atoll(e) : (long long)1100;
        }();
        // (with structures in the loop the supply wavefronts also carry the sideflow assembly and, on reaches with
        // transmission loss, two OCML pow calls per cell: the crossover is lower -- 3000^2 with 256 sites: 5.5 vs 8.2 ms
        // at 1000^2, 16.1 vs 15.2 at 2000^2)
        static const int64_t split_max_struct = [] {
            const char *e = std::getenv("LF_FUSED_SPLIT_MAX_STRUCT");
            return e ? std::atoll(e) : (long long)600;
        }();
        const char *es = std::getenv("LF_FUSED_SPLIT");
        // (with structures in the loop: on a graph with their links; without them: on a graph without links)
        const bool split_form = all35 && !F.inert && (in ? F.linked != nullptr : F.linked == nullptr) && r->fplan.cw == 64 &&
                                n < ((int64_t)1 << 29) && (es ? es[0] != '0' : ncones <= (in ? split_max_struct : split_max));
        if (split_form)
            pick_flags(a->split, in, [&](auto sp, auto st) {
                hipLaunchKernelGGL((k_fused_cones_split<sp, st>), grid, dim3(64 * (1 + kFusedKC)), 0, s, F);
            });
        else
            pick_flags(a->split, all35, [&](auto sp, auto a35) {
                pick_flags(in, r->fplan.cw == 64, [&](auto st, auto cw64) {
                    constexpr int CW = decltype(cw64)::value ? 64 : kBlock;
                    hipLaunchKernelGGL((k_fused_cones<sp, a35, st, false, CW>), grid, dim3(CW), 0, s, F);
                });
            });
    };
    auto levels = [&](dim3 grid) {
        pick_flags(a->split, in, [&](auto sp, auto st) {
            hipLaunchKernelGGL((k_fused_substeps<sp, st>), grid, dim3(kBlock), 0, s, F);
        });
    };
    // lakes and reservoirs of the blocks / levels [lo, hi]: sub-step t - block / level, before the cells of that block / level
    std::vector<int> site_blocks; // sorted blocks of the lakes and reservoirs
    if (!r->fplan.empty())
        for (int lv : sc.site_level_sorted) site_blocks.push_back(r->fplan.lvl2blk[lv]);
    auto sites = [&](bool blocks, int lo, int hi) {
        const std::vector<int> &units = blocks ? site_blocks : sc.site_level_sorted;
        auto it = std::lower_bound(units.begin(), units.end(), lo);
        if (it == units.end() || *it > hi) return;
        if (blocks)
            hipLaunchKernelGGL(k_sites_blocks, dim3(blocks_for(nsites)), dim3(kBlock), 0, s, F);
        else
            hipLaunchKernelGGL(k_sites_wave, dim3(blocks_for(nsites)), dim3(kBlock), 0, s, F);
        ++launches;
    };
    const int NB = r->fplan.empty() ? -1 : r->fplan.nblocks();
    LF_TRY(fused_wavefront<false>(*r, F, 0, (int)r->NL, 0, NB, time_major, s, launches, cones, levels, sites, in ? &sc : nullptr));
    fused_set_stats(r, launches);
    return LF_OK;
}

} // namespace

extern "C" int lf_routing_substeps_fused(lf_router *r, const lf_substep_args *a, int nsteps, int64_t sideflow_stride)
{
    return fused_impl(r, a, nsteps, sideflow_stride, nullptr);
}

// Several MODEL steps as one wavefront: the skew runs on across the model-step boundary, so the pipeline fill (one launch per
// level block) is paid once per call instead of once per model step -- what a deep network needs (deep 5000^2: 313 blocks +
// 23 launches per model step on its own, 24 per model step in steady state).
extern "C" int lf_routing_model_steps_fused(lf_router *r, const lf_substep_args *a, int steps_per_model_step, int n_model_steps,
                                            int64_t sideflow_model_stride)
{
    if (steps_per_model_step < 1 || n_model_steps < 1) return lf_set_error(LF_E_INVALID, "bad argument");
    return fused_impl(r, a, steps_per_model_step * n_model_steps, 0, nullptr, steps_per_model_step, sideflow_model_stride);
}

extern "C" int lf_routing_substeps_fused_structures(lf_router *r, const lf_substep_args *a, const lf_inloop_args *in,
                                                    int nsteps)
{
    if (!in) return lf_set_error(LF_E_INVALID, "null argument");
    return fused_impl(r, a, nsteps, 0, in);
}

// ================================================================================================
// An ensemble through the sub-step loop: `members` state rows on ONE router, sharing its statics and its launch schedule.
// Where the time-major form applies the members are a second grid dimension of its level kernel
// (k_fused_level_steps_members), slice by slice: a slice is as many members as the history [slice][nsteps][N] has room
// for inside its budget.  Otherwise the members run one after the other through the single-member schedule -- correct and
// bit-identical, with no gain but the flag passes, which run once.  Both calls, plain and with structures in the loop, are
// one implementation (fused_ensemble_impl) behind one set of refusals (fused_members_check).
// ================================================================================================
extern "C" int64_t lf_fused_members_slice(int members, int64_t n, int nsteps, int split, int64_t budget_bytes, int cap)
{
    if (members < 1 || n < 0 || nsteps < 1 || budget_bytes < 0) return 0;
    int64_t s = std::min<int64_t>(members, 65535); // blockIdx.y
    if (cap > 0) s = std::min<int64_t>(s, cap);
    const __int128 per = (__int128)nsteps * n * 8 * (split ? 2 : 1); // bytes of one member's history
    if (per > 0) s = (int64_t)std::min<__int128>(s, (__int128)budget_bytes / per);
    return s;
}

namespace {

// `a` with every per-member row moved m members on
lf_substep_args member_args(const lf_substep_args &a, int64_t m, int64_t member_stride, int64_t side_member_stride)
{
    lf_substep_args b = a;
    auto move = [&](double *&x) {
        if (x) x += m * member_stride;
    };
    b.SideflowChanM3 += m * side_member_stride;
    move(b.ChanQKin);
    move(b.ChanM3Kin);
    move(b.Chan2QKin);
    move(b.Chan2M3Kin);
    move(b.CrossSection2Area);
    move(b.Sideflow1Chan);
    move(b.ChanQ);
    move(b.sumDisDay);
    move(b.FlowVelocity);
    move(b.TravelDistance);
    return b;
}

// `in` with every per-member row moved m members on: the dense [N] rows by member_stride, the site-state rows by the site
// strides, the forcing rows by forcing_stride (0: member 0's for all); site lists, site parameters, UpTrans and the scalars
// are shared, and a null pointer (an option switched off) stays null -- as k_fused_level_steps_members<.., STRUCT> moves them
lf_inloop_args member_inloop(const lf_inloop_args &in, int64_t m, int64_t member_stride, int64_t lake_stride, int64_t res_stride,
                             int64_t forcing_stride)
{
    lf_inloop_args b = in;
    auto move = [m](auto *&x, int64_t stride) {
        if (x) x += m * stride;
    };
    for (auto x : {&b.QLakeOutM3Dt, &b.QResOutM3Dt, &b.QInDt, &b.QinADDEDM3, &b.TransLossM3Dt, &b.TransCum, &b.SideflowChanM3})
        move(*x, member_stride);
    move(b.ChanQ, member_stride);
    for (auto x : {&b.LakeStorageM3CC, &b.LakeInflowOldCC, &b.LakeOutflowCC, &b.LakeStorageM3BalanceCC, &b.LakeLevelCC, &b.LakeInflowCC})
        move(*x, lake_stride);
    for (auto x : {&b.ReservoirStorageM3CC, &b.ReservoirFillCC, &b.ReservoirInflowCC}) move(*x, res_stride);
    for (auto x : {&b.ToChanM3RunoffDt, &b.EvaAddM3Dt, &b.WUseAddM3Dt, &b.ChannelToPolderM3Dt, &b.QInM3Old, &b.QDelta})
        move(*x, forcing_stride);
    return b;
}

// What both ensemble calls refuse, in this order; structures: the call with lakes, reservoirs, inflow hydrographs and
// transmission loss in the loop (needs `in`, has no sideflow strides), otherwise the plain one (no site and forcing strides)
int fused_members_check(const lf_router *r, const lf_substep_args *a, const lf_inloop_args *in, bool structures, int nsteps,
                        int64_t sideflow_stride, const fused_member_strides &M)
{
    // ---- what needs no router, and so no device ----
    if (M.members < 1) return lf_set_error(LF_E_INVALID, "members must be at least 1 (got %d)", M.members);
    if (M.member < 0)
        return lf_set_error(LF_E_INVALID, "member_stride %lld is less than the router's number of cells", (long long)M.member);
    if (M.side < 0)
        return lf_set_error(LF_E_INVALID, "sideflow_member_stride %lld is neither 0 nor a whole member's sideflow rows",
                            (long long)M.side);
    if (M.lake < 0)
        return lf_set_error(LF_E_INVALID, "lake_member_stride %lld is less than the number of lakes", (long long)M.lake);
    if (M.res < 0)
        return lf_set_error(LF_E_INVALID, "res_member_stride %lld is less than the number of reservoirs", (long long)M.res);
    if (M.forcing < 0)
        return lf_set_error(LF_E_INVALID, "forcing_member_stride %lld is neither 0 nor at least the router's number of cells",
                            (long long)M.forcing);
    if (!r || !a || (structures && !in)) return lf_set_error(LF_E_INVALID, "null argument");
    if (nsteps < 1)
        return structures ? lf_set_error(LF_E_INVALID, "nsteps must be at least 1 (got %d)", nsteps)
                          : lf_set_error(LF_E_INVALID, "bad argument");
    // ---- against the router's and the lists' sizes: host fields, still no device ----
    if (M.member < r->N)
        return lf_set_error(LF_E_INVALID, "member_stride %lld is less than the router's number of cells (%lld)",
                            (long long)M.member, (long long)r->N);
    if (in && in->n_lakes > 0 && M.lake < in->n_lakes)
        return lf_set_error(LF_E_INVALID, "lake_member_stride %lld is less than the number of lakes (%lld)", (long long)M.lake,
                            (long long)in->n_lakes);
    if (in && in->n_res > 0 && M.res < in->n_res)
        return lf_set_error(LF_E_INVALID, "res_member_stride %lld is less than the number of reservoirs (%lld)", (long long)M.res,
                            (long long)in->n_res);
    if (M.forcing != 0 && M.forcing < r->N)
        return lf_set_error(LF_E_INVALID, "forcing_member_stride %lld is neither 0 nor at least the router's number of cells (%lld)",
                            (long long)M.forcing, (long long)r->N);
    LF_TRY(fused_check_call(*r, *a, sideflow_stride, "fused sub-step wavefront needs"));
    const int64_t side_rows = sideflow_stride == 0 ? r->N : (int64_t)nsteps * r->N;
    if (M.side != 0 && M.side < side_rows)
        return lf_set_error(LF_E_INVALID, "sideflow_member_stride %lld is neither 0 nor a whole member's sideflow rows (%lld)",
                            (long long)M.side, (long long)side_rows);
    if (!structures && r->linked.p)
        return lf_set_error(LF_E_INVALID, "a router on a graph with structure links runs no ensemble through the sub-step loop "
                                          "(lf_routing_substeps_fused_members)");
    return LF_OK;
}

// An ensemble call of M.members > 1 members on a router with cells, its arguments checked (fused_members_check); in: the
// in-loop block of the call with structures (member 0's; the site lists are shared by the members: checked and planned once
// per call), null: the plain call.  Where the time-major form applies to the ensemble -- more than one sub-step, the single
// call's width rule with the lanes of a launch counted over the members (members * N), room for a slice's history and, with
// structures, a site plan that applies (or no site) and room for a slice's feed buffers -- the members of a slice are the
// second grid dimension of the level kernel (fused_time_major_levels).  Otherwise member after member through fused_impl.
int fused_ensemble_impl(lf_router *r, const lf_substep_args *a, const lf_inloop_args *in, int nsteps, int64_t sideflow_stride,
                        const fused_member_strides &M)
{
    LF_HIP(hipSetDevice(r->device));
    const int64_t n = r->N;
    const int NL = (int)r->NL;
    const bool split = a->split != 0;
    hipStream_t s = r->ctx->stream;
    lf_inloop_args I = {};
    const fused_site_cache *sc = nullptr;
    LF_TRY(fused_inloop_of(r, *a, in, I, s, sc));
    // ---- does the member form of the time-major schedule apply, and on slices of how many members? -------------------
    int64_t slice = 0;
    size_t budget = 0;
    if (fused_time_major_wanted(NL, (int64_t)M.members * n) && nsteps > 1 && (I.n_lakes + I.n_res == 0 || sc->applies) &&
        lf_history_budget(r->fused_hist1, r->fused_hist2, budget)) {
        const char *c = std::getenv("LF_FUSED_MEMBERS_SLICE"); // A/B switch, read per call
        slice = lf_fused_members_slice(M.members, n, nsteps, split, (int64_t)std::min<size_t>(budget, INT64_MAX), c ? std::atoi(c) : 0);
        // (the size was cut to the budget first, so nothing is refused for its size -- and a history or a feed buffer that
        // still does not come is not remembered in r->fused_hist_refused, which belongs to the single call's own, smaller,
        // request: the members then run one after the other, each with that request)
        size_t refused = SIZE_MAX;
        if (slice > 0 && !lf_history_ensure(r->fused_hist1, r->fused_hist2, refused, (size_t)slice * nsteps * (size_t)n, split))
            slice = 0;
        const size_t feed = (size_t)slice * (size_t)(nsteps + 1) * (size_t)sc->nfeed;
        if (in && slice > 0 && sc->feed.n < feed && sc->feed.grow(feed) != LF_OK) slice = 0;
    }
    int64_t launches = 0;
    if (slice == 0) {
        // Member after member through the single call's schedule.  What runs once: the site checks and the plan (above; every
        // member's call finds the cache by the shared list pointers) and the flag passes over the statics (flags_ready from
        // the second member on).  With structures in the loop no pass of the call reads member state -- the inert flags, the
        // one candidate, are never taken then --, so nothing is repeated per member but the wavefront itself.
        for (int m = 0; m < M.members; ++m) {
            const lf_substep_args b = member_args(*a, m, M.member, M.side);
            const lf_inloop_args bi = in ? member_inloop(*in, m, M.member, M.lake, M.res, M.forcing) : I;
            LF_TRY(fused_impl(r, &b, nsteps, sideflow_stride, in ? &bi : nullptr, 0, 0, m > 0));
            launches += r->last_stats[0];
        }
    } else {
        LF_TRY(fused_parity_ensure(*r, split, (size_t)n)); // (as fused_impl leaves a router: other forms find them)
        fused_args F = fused_args_of(*r, *a, nsteps, nsteps, sideflow_stride, 0);
        if (in) {
            F.linked = r->linked.p; // (fused_time_major_levels: the site plan's cell flags in its place)
            F.level_nlinked = r->level_nlinked.p;
            F.fb_lvl2blk = r->fplan_dev.lvl2blk.p;
            F.site_level = sc->site_level.p;
            F.I = I;
        }
        // once for all members -- plain: both flags; time-major with structures: neither is taken
        LF_TRY(fused_statics_flags(*r, F, in != nullptr, in != nullptr, false, s, launches));
        fused_member_strides Ms = M;
        for (int64_t m0 = 0; m0 < M.members; m0 += slice) {
            Ms.members = (int)std::min<int64_t>(slice, M.members - m0);
            F.S = member_args(*a, m0, M.member, M.side);
            if (in) F.I = member_inloop(I, m0, M.member, M.lake, M.res, M.forcing);
            fused_time_major_levels<false>(*r, F, 0, NL, in ? sc : nullptr, &Ms, s, launches);
        }
        r->last_fused_form = 1;
        LF_HIP(hipGetLastError());
    }
    fused_set_stats(r, launches);
    return LF_OK;
}

} // namespace

extern "C" int lf_routing_substeps_fused_structures_members(lf_router *r, const lf_substep_args *a, const lf_inloop_args *in,
                                                            int nsteps, int members, int64_t member_stride,
                                                            int64_t lake_member_stride, int64_t res_member_stride,
                                                            int64_t forcing_member_stride)
{
    const fused_member_strides M = {members, member_stride, 0, lake_member_stride, res_member_stride, forcing_member_stride};
    LF_TRY(fused_members_check(r, a, in, true, nsteps, 0, M));
    if (members == 1) return fused_impl(r, a, nsteps, 0, in);
    if (r->N == 0) return LF_OK;
    return fused_ensemble_impl(r, a, in, nsteps, 0, M);
}

extern "C" int lf_routing_substeps_fused_members(lf_router *r, const lf_substep_args *a, int nsteps, int64_t sideflow_stride,
                                                 int members, int64_t member_stride, int64_t sideflow_member_stride)
{
    const fused_member_strides M = {members, member_stride, sideflow_member_stride, 0, 0, 0};
    LF_TRY(fused_members_check(r, a, nullptr, false, nsteps, sideflow_stride, M));
    if (members == 1) return fused_impl(r, a, nsteps, sideflow_stride, nullptr);
    if (r->N == 0) return LF_OK;
    return fused_ensemble_impl(r, a, nullptr, nsteps, sideflow_stride, M);
}

// ================================================================================================
// PMC calibration: a stream copy with exactly known HBM traffic (n*8 B read + n*8 B written) in this
// engine's access widths, so that rocprofv3's FETCH_SIZE / WRITE_SIZE can be calibrated on gfx950
// (MI355X_MICROARCH.md, HBM section) before they are compared with byte counts.
// ================================================================================================
namespace {
__global__ void __launch_bounds__(kBlock) k_calib_copy8(long long n, const double *__restrict__ src, double *__restrict__ dst)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
__global__ void __launch_bounds__(kBlock) k_calib_copy16(long long n2, const double2 *__restrict__ src,
                                                         double2 *__restrict__ dst)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < n2) dst[i] = src[i];
}
} // namespace

namespace {
struct calib_streams {
    const double *src[8];
};
template <int NS>
__global__ void __launch_bounds__(kBlock) k_calib_streams(long long n, calib_streams S, double *__restrict__ dst)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double v[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = S.src[k][i];
    double acc = v[0];
#pragma unroll
    for (int k = 1; k < NS; ++k) acc += v[k];
    dst[i] = acc;
}
} // namespace

// nread (1..8) read streams and one write stream of n doubles, one element per lane: the byte mix of the level sweep
// without its arithmetic and without its gather -- what the memory system gives a kernel of that many 8-byte streams
extern "C" int lf_calibration_streams(int device, int nread, const double *const *src_dev, double *dst_dev, int64_t n)
{
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    if (!src_dev || !dst_dev || n <= 0 || nread < 1 || nread > 8) return lf_set_error(LF_E_INVALID, "bad argument");
    calib_streams S;
    for (int k = 0; k < 8; ++k) S.src[k] = src_dev[k < nread ? k : 0];
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    switch (nread) {
    case 1: hipLaunchKernelGGL(k_calib_streams<1>, grid, block, 0, c->stream, (long long)n, S, dst_dev); break;
    case 2: hipLaunchKernelGGL(k_calib_streams<2>, grid, block, 0, c->stream, (long long)n, S, dst_dev); break;
    case 3: hipLaunchKernelGGL(k_calib_streams<3>, grid, block, 0, c->stream, (long long)n, S, dst_dev); break;
    case 4: hipLaunchKernelGGL(k_calib_streams<4>, grid, block, 0, c->stream, (long long)n, S, dst_dev); break;
    case 5: hipLaunchKernelGGL(k_calib_streams<5>, grid, block, 0, c->stream, (long long)n, S, dst_dev); break;
    case 6: hipLaunchKernelGGL(k_calib_streams<6>, grid, block, 0, c->stream, (long long)n, S, dst_dev); break;
    case 7: hipLaunchKernelGGL(k_calib_streams<7>, grid, block, 0, c->stream, (long long)n, S, dst_dev); break;
    default: hipLaunchKernelGGL(k_calib_streams<8>, grid, block, 0, c->stream, (long long)n, S, dst_dev); break;
    }
    LF_HIP(hipGetLastError());
    return LF_OK;
}

extern "C" int lf_calibration_copy(int device, const double *src_dev, double *dst_dev, int64_t n, int bytes_per_lane)
{
    lf_device_ctx *c;
    LF_TRY(lf_ctx(device, &c));
    if (!src_dev || !dst_dev || n <= 0) return lf_set_error(LF_E_INVALID, "bad argument");
    if (bytes_per_lane == 16) {
        const long long n2 = n / 2;
        hipLaunchKernelGGL(k_calib_copy16, dim3((unsigned)((n2 + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, n2,
                           (const double2 *)src_dev, (double2 *)dst_dev);
    } else {
        hipLaunchKernelGGL(k_calib_copy8, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                           (long long)n, src_dev, dst_dev);
    }
    LF_HIP(hipGetLastError());
    return LF_OK;
}
