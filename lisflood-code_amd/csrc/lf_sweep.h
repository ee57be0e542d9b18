// lf_sweep.h -- the level sweep, shared by the single-GPU router (lf_router.hip) and the row-block distributed router
// (lf_dist.hip): device code, then the host schedule of a router call.  See lf_router.hip for the data layout.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "lf_blocks.h"
#include "lf_common.h"
#include "lf_math.h"

namespace {


constexpr int kBlock = 256;
constexpr int kNarrowBlock = 1024;
constexpr int kNarrowMax = 1024; // levels up to this many cells are swept by the single-workgroup kernel

inline int blocks_for(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }

// One launch of a router call without level blocks: a wide level, or a run of consecutive narrow levels
struct level_segment {
    int k0, k1; // levels [k0, k1); wide segments have k1 == k0 + 1
    bool wide;
};

// Levels [k_lo, k_hi) of `level_start` as segments: a level of more than kNarrowMax cells is one wide segment, a run of
// levels of at most kNarrowMax cells one narrow segment
inline std::vector<level_segment> level_segments(const std::vector<int64_t> &level_start, int64_t k_lo, int64_t k_hi)
{
    auto narrow = [&](int64_t k) { return level_start[k + 1] - level_start[k] <= kNarrowMax; };
    std::vector<level_segment> out;
    for (int64_t k = k_lo; k < k_hi;) {
        int64_t e = k + 1;
        if (narrow(k))
            while (e < k_hi && narrow(e)) ++e;
        out.push_back({(int)k, (int)e, !narrow(k)});
        k = e;
    }
    return out;
}

// solve1Pixel, kinematic_wave_parallel_tools.py:59-82 (c = const_plus_ups_infl)
__device__ __forceinline__ double lf_solve_cell(double c, double a, double ba, double beta, double inv_beta,
                                                double b_minus_1)
{
    if (c <= LF_NEWTON_TOL) return 0.0;
    const double t = ba * pow(c, b_minus_1);
    double secant;
    if (t <= 1.0)
        secant = c / (1.0 + t);
    else
        secant = c / (1.0 + pow(t, inv_beta));
    const double other = pow((c - secant) / a, inv_beta);
    double q = (secant + other) / 2.0;
    double err = q + a * pow(q, beta) - c; // closureError, :89-92
    double prev = -1.0;
    int count = 0;
    while (fabs(err) > LF_NEWTON_TOL && q != prev && count < LF_MAX_ITERS) {
        prev = q;
        q -= err / (1.0 + ba * pow(q, b_minus_1));
        q = (LF_NEWTON_TOL > q) ? LF_NEWTON_TOL : q; // builtins.max(q, NEWTON_TOL)
        err = q + a * pow(q, beta) - c;
        ++count;
    }
    if (q == LF_NEWTON_TOL) q = 0.0;
    return q;
}

// The same out of line: inside the cone kernel's level loop the general path is taken by single lanes with extreme
// arguments or not at all when beta = 3/5 -- one copy to jump to instead of ~1500 instructions to jump over per level
__device__ __attribute__((noinline)) double lf_solve_cell_cold(double c, double a, double ba, double beta, double inv_beta,
                                                               double b_minus_1)
{
    return lf_solve_cell(c, a, ba, beta, inv_beta, b_minus_1);
}
__device__ __attribute__((noinline)) double lf_pow_cold(double x, double y) { return pow(x, y); }
// lf_pow_3_5 with the OCML fallback (arguments beyond the fast range) out of line
__device__ __forceinline__ double lf_pow_3_5_hot(double x)
{
    if (x == 0.0) return 0.0;
    if (lf_fast_range(x)) {
        const double r = lf_root5(x);
        return r * r * r;
    }
    return lf_pow_cold(x, 0.6);
}

// constant = a*Qold^beta + q*dx (kinematic_wave_parallel.py:163,175), gathered into sweep order
__global__ void __launch_bounds__(kBlock) k_prep(int n, const int *__restrict__ perm, const double *__restrict__ q_pix,
                                                 const double *__restrict__ lat_pix, const double *__restrict__ a,
                                                 const double *__restrict__ dx, double dx_scalar, double beta,
                                                 double *__restrict__ constant)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int pix = perm ? perm[p] : p; // perm == nullptr: vectors already in sweep order
    const double lateral = lat_pix[pix] * (dx ? dx[p] : dx_scalar);
    constant[p] = a[p] * pow(q_pix[pix], beta) + lateral;
}

// everything one sweep launch needs (passed by value)
struct sweep_args {
    const int *__restrict__ ups_ptr;
    const int *__restrict__ ups_idx;     // INDEXED only: upstream positions (may point into the ghost slots)
    const int *__restrict__ ups_base;    // INDEXED only: first upstream position if they are consecutive, else -1
    const int *__restrict__ perm;        // pixel-order I/O only
    const double *__restrict__ a;        // alpha*dx/dt, sweep order
    const double *__restrict__ constant; // general path: written by k_prep
    const double *__restrict__ lat;      // fused path: specific lateral inflow (pixel order, or sweep order if ORDERED)
    const double *__restrict__ dx;       // fused path: per-pixel dx (sweep order) or nullptr
    double dx_scalar;
    double beta, inv_beta, b_minus_1;
    int kmax;     // max in-degree of the graph (<= 8)
    double *qord; // discharge in sweep order: upstream values are read from it, the new value is written to it
    double *q_pix; // pixel-order I/O: caller's discharge vector (old value in, new value out); unused if ORDERED
    // INDEXED only (row-block partition, pipelined calls): the old discharge is read from here instead of qord when not
    // null -- successive calls ping-pong between two state vectors so that a call may start before the one before it has
    // finished its later phases (lf_dist_router_route_many)
    const double *qold_src;
    // STATICS kernels only (wide levels of an ordered beta = 3/5 call): what a cell reads of the router's static vectors as
    // ONE record instead of separate loads -- the level sweep is sensitive to the number of its memory instructions at the
    // same bytes.  STATICS = 1: (a, dx), 16 bytes, ups_ptr read as before.
    const double2 *__restrict__ adx;
    // STATICS = 3 (INDEXED: the row-block partition's level kernel, which reads four static streams -- a, dx, ups_ptr,
    // ups_base): (a, dx, first list entry | count << 28, ups_base), 24 bytes
    const struct lf_rec24 *__restrict__ rec24;
    // STATICS = 2 (wide levels of an ordered beta = 3/5 call): the (a, dx) records of STATICS = 1, and the upstream range
    // from one count byte per cell instead of two ups_ptr entries -- upcnt[p] = ups_ptr[p + 1] - ups_ptr[p], and ups_ptr at
    // the first cell of every group of 64 cells of the level being swept (wave_start points at the level's first group)
    const unsigned char *__restrict__ upcnt;
    const int *__restrict__ wave_start;
};
struct lf_rec24 {
    double a, dx;
    unsigned int up; // first entry of the cell's upstream list (28 bits) | number of upstream cells << 28
    int base;        // ups_base: first upstream position if they are consecutive, else -1
};

// One cell of the implicit sweep.
//   FUSED (beta == 3/5): the old-discharge term is computed here (kinematic_wave_parallel.py:163,175 folded
//     into the sweep) and the closure is solved as a quintic in Q^(1/5) (lf_math.h); otherwise `constant`
//     comes from k_prep and the reference's own Newton iteration runs.
//   ORDERED: discharge and lateral inflow are resident in sweep order (engine layout): qord[p] holds the old
//     discharge on entry and the new one on exit, every access is a coalesced stream.  Otherwise they are
//     gathered from / scattered to the caller's pixel-order vectors through perm.
//   INDEXED: upstream positions come from the index list ups_idx[ups_ptr[p] .. ups_ptr[p+1]) instead of being the
//     contiguous positions themselves (row-block partitions: upstream cells may sit in other phases or in the
//     ghost slots filled by the halo exchange).
// What a cell reads of the router's static vectors -- the same for every member of an ensemble swept on one router: a, dx
// (STATICS = 3, the partition's record with the upstream range in it: sweep_cell_range)
template <bool FUSED, int STATICS>
__device__ __forceinline__ void sweep_cell_statics(int p, const sweep_args &A, double &ap, double &dxp)
{
    if (STATICS == 1 || STATICS == 2) {
        const double2 sd = A.adx[p];
        ap = sd.x;
        dxp = sd.y;
    } else {
        ap = A.a[p];
        dxp = (FUSED && A.dx) ? A.dx[p] : A.dx_scalar;
    }
}
// two consecutive discharges as one 16-byte load from an address that is only 8-byte aligned (double2 itself asks for 16)
__device__ __forceinline__ double2 lf_load_pair(const double *p)
{
    double2 t;
    __builtin_memcpy(&t, p, sizeof t);
    return t;
}
// ... and everything else of the cell: the state vectors of A (one member's), the solve, the store
template <bool FUSED, bool ORDERED, bool INDEXED = false, int STATICS = 0>
__device__ __forceinline__ void sweep_cell_state(int p, int pix, double ap, double dxp, int u0, int u1, int rec_base, const sweep_args &A)
{
    // the cell's own two values first: requested with the statics above, before anything waits for the upstream range
    double lat_q = 0.0, qold = 0.0;
    if (FUSED) {
        lat_q = A.lat[pix];
        qold = ORDERED ? ((INDEXED && A.qold_src) ? A.qold_src[p] : A.qord[p]) : A.q_pix[pix];
    }
    // Upstream inflow, summed in ascending pixel id (kinematic_wave_parallel_tools.py:57-58).  A D8 cell has
    // at most 8 upstream neighbours: all candidate loads are issued at once (predicated) instead of a
    // dependent load per loop trip; missing ones contribute +0.0, which leaves the sum bit-identical.
    // The requests go out as soon as the upstream range is known, BEFORE the old-discharge term is worked out (its power
    // runs while they travel), and nothing may use a value before all of them are out: the empty asm behind the power is
    // where they are first needed (without it the compiler sinks `0.0 + v[0]` into the first load's branch and waits for
    // that load before it requests the others).
    double v[8];
    const int base = INDEXED ? (STATICS == 3 ? rec_base : A.ups_base[p]) : u0;
    // (the upstream loads sit behind branches -- a wavefront none of whose lanes has a fourth pair skips that request -- so
    // the compiler cannot count them and waits for ALL loads wherever it needs one: the cell's own values are therefore
    // taken in here, before the upstream requests go out, and the power below then runs with only those in flight)
    // (pixel-order vectors: the cell's own values are themselves a second trip, behind perm -- the upstream requests go out
    // with them and one wait takes all of it in)
    if (FUSED && ORDERED) asm volatile("" : "+v"(qold), "+v"(lat_q));
    if (!INDEXED) {
        // the contiguous upstream run two values per load: four 16-byte loads instead of eight 8-byte ones (the sweep is
        // sensitive to the number of its memory instructions).  The second value of a pair may lie one position behind the
        // run -- still inside the vector (a cell's upstream positions all precede its own) -- and is then discarded.
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double2 t = make_double2(0.0, 0.0);
            if (2 * j < A.kmax && u0 + 2 * j < u1) t = lf_load_pair(A.qord + u0 + 2 * j);
            v[2 * j] = t.x;
            v[2 * j + 1] = t.y;
        }
    } else if (base >= 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (k < A.kmax && u0 + k < u1) ? A.qord[base + k] : 0.0;
    } else { // ghost or cross-phase inflow: positions from the list (a second, dependent load)
        // (all list entries first, then all discharges: entry by entry the compiler waits for every load in flight before each
        // dependent one -- sixteen round trips in a row for a wavefront with one such lane)
        int e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = (k < A.kmax && u0 + k < u1) ? A.ups_idx[u0 + k] : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(e[k]));
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (k < A.kmax && u0 + k < u1) ? A.qord[e[k]] : 0.0;
    }
    double cst;
    if (FUSED) {
        const double lateral = lat_q * dxp;
        cst = ap * lf_pow_3_5(qold) + lateral;
    } else {
        cst = A.constant[p];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(v[k]));
    if (!INDEXED) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[2 * j + 1] = (u0 + 2 * j + 1 < u1) ? v[2 * j + 1] : 0.0;
    }
    double ups = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) ups += v[k];
    const double c = ups + cst;
    double q;
    if (FUSED && lf_fast_range(c) && lf_fast_range(ap)) {
        q = (c <= LF_NEWTON_TOL) ? 0.0 : lf_solve_3_5(c, ap);
    } else {
        q = lf_solve_cell(c, ap, A.beta * ap, A.beta, A.inv_beta, A.b_minus_1); // incl. alpha == 0 / NaN semantics
    }
    A.qord[p] = q;
    if (!ORDERED) A.q_pix[pix] = q;
}
template <bool FUSED, bool ORDERED, bool INDEXED = false, int STATICS = 0>
__device__ __forceinline__ void sweep_cell_range(int p, int u0, int u1, const sweep_args &A)
{
    static_assert(STATICS == 0 || (FUSED && ORDERED && INDEXED == (STATICS == 3)), "the records are the ordered beta = 3/5 router's");
    const int pix = ORDERED ? p : A.perm[p];
    double ap, dxp;
    int rec_base = 0;
    if (STATICS == 3) {
        const lf_rec24 R = A.rec24[p];
        ap = R.a;
        dxp = R.dx;
        u0 = (int)(R.up & 0x0fffffffu);
        u1 = u0 + (int)(R.up >> 28);
        rec_base = R.base;
    } else {
        sweep_cell_statics<FUSED, STATICS>(p, A, ap, dxp);
    }
    sweep_cell_state<FUSED, ORDERED, INDEXED, STATICS>(p, pix, ap, dxp, u0, u1, rec_base, A);
}
template <bool FUSED, bool ORDERED, bool INDEXED = false, int STATICS = 0>
__device__ __forceinline__ void sweep_cell(int p, const sweep_args &A)
{
    if (STATICS == 3)
        sweep_cell_range<FUSED, ORDERED, INDEXED, STATICS>(p, 0, 0, A); // (the upstream range comes with the record)
    else
        sweep_cell_range<FUSED, ORDERED, INDEXED, STATICS>(p, A.ups_ptr[p], A.ups_ptr[p + 1], A);
}

// Read of a table that no kernel of this library ever writes (the cone plans of the level blocks) through the
// constant address space: with a wavefront-uniform index it becomes a scalar load (s_load) instead of a vector load that
// the compiler, fearing an alias with the discharge stores, would wait for together with every store in flight.
__device__ __forceinline__ int ld_table(const int *p, int i)
{
    typedef const int __attribute__((address_space(4))) *const_int_ptr;
    return ((const_int_ptr)(unsigned long long)p)[i];
}

// STATICS = 2: the cell at position p, number i of its level.  The upstream runs of consecutive cells are consecutive
// (ups_ptr is their running sum), so a cell's run starts at the start of its wavefront's first run plus the counts of the
// lanes below it: one byte per cell and one scalar load per wavefront instead of two 4-byte loads per lane.  A count is at
// most 8: the prefix is the number of lanes below with bit b of the count set, weighted 1, 2, 4, 8 -- four ballots and
// mbcnt, no data moves between lanes, and a lane that has left (beyond the level's end) is in no ballot.
template <bool FUSED, bool ORDERED>
__device__ __forceinline__ void sweep_cell_counted(int p, int i, const sweep_args &A)
{
    const unsigned cnt = A.upcnt[p];
    double ap, dxp;
    sweep_cell_statics<FUSED, 2>(p, A, ap, dxp);
    const int start = ld_table(A.wave_start, __builtin_amdgcn_readfirstlane(i >> 6));
    unsigned below[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64((cnt >> b) & 1u);
        below[b] = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    }
    const int u0 = start + (int)(below[0] + 2u * below[1] + 4u * below[2] + 8u * below[3]);
    sweep_cell_state<FUSED, ORDERED, false, 2>(p, p, ap, dxp, u0, u0 + (int)cnt, 0, A);
}

// one wide level: one cell per lane
#ifndef LF_LEVEL_WAVES
#define LF_LEVEL_WAVES 8 /* <= 80 SGPRs / 64 VGPRs: 8 wavefronts per SIMD instead of the 7 that 96 SGPRs allow (+2.3 %) */
#endif
#ifndef LF_LEVEL_BLOCK
#define LF_LEVEL_BLOCK 256
#endif
constexpr int kLevelBlock = LF_LEVEL_BLOCK; // workgroup of the wide-level kernel
inline int level_blocks_for(int64_t n) { return (int)((n + kLevelBlock - 1) / kLevelBlock); }
#if LF_LEVEL_WAVES
#define LF_LEVEL_ATTR __attribute__((amdgpu_waves_per_eu(LF_LEVEL_WAVES)))
#else
#define LF_LEVEL_ATTR
#endif
template <bool FUSED, bool ORDERED, bool INDEXED = false, int STATICS = 0>
__global__ void __launch_bounds__(kLevelBlock) LF_LEVEL_ATTR k_level(int first, int count, sweep_args A)
{
    const int i = blockIdx.x * kLevelBlock + threadIdx.x;
    if (i >= count) return;
    if constexpr (STATICS == 2) {
        static_assert(FUSED && ORDERED && !INDEXED && kLevelBlock % 64 == 0, "a wavefront is one group of 64 cells of the level");
        sweep_cell_counted<FUSED, ORDERED>(first + i, i, A);
    } else {
        sweep_cell<FUSED, ORDERED, INDEXED, STATICS>(first + i, A);
    }
}

// the count bytes of k_level<.., STATICS = 2> (once per router)
__global__ void __launch_bounds__(kLevelBlock) k_static_counts(long long n, const int *__restrict__ ups_ptr, unsigned char *__restrict__ upcnt)
{
    const long long i = (long long)blockIdx.x * kLevelBlock + threadIdx.x;
    if (i < n) upcnt[i] = (unsigned char)(ups_ptr[i + 1] - ups_ptr[i]);
}
// ... and its table of wavefront starts: for every level k, from entry wave_off[k] on, ups_ptr at every 64th cell of the
// level counted from its first one (blockIdx.x strides the levels, blockIdx.y and the threads the groups of a level)
__global__ void __launch_bounds__(kLevelBlock) k_wave_starts(long long nl, const long long *__restrict__ level_start,
                                                             const int *__restrict__ wave_off, const int *__restrict__ ups_ptr,
                                                             int *__restrict__ wave_start)
{
    for (long long k = blockIdx.x; k < nl; k += gridDim.x) {
        const long long first = level_start[k], groups = (level_start[k + 1] - first + 63) / 64;
        for (long long w = (long long)blockIdx.y * kLevelBlock + threadIdx.x; w < groups; w += (long long)gridDim.y * kLevelBlock)
            wave_start[wave_off[k] + w] = ups_ptr[first + 64 * w];
    }
}

// the 24-byte records of k_level<.., INDEXED, STATICS = 3> (row-block partition; once per router and section)
__global__ void __launch_bounds__(kLevelBlock) k_static_records_indexed(long long n, const double *__restrict__ a,
                                                                        const double *__restrict__ dx, const int *__restrict__ ups_ptr,
                                                                        const int *__restrict__ ups_base, lf_rec24 *__restrict__ rec)
{
    const long long i = (long long)blockIdx.x * kLevelBlock + threadIdx.x;
    if (i >= n) return;
    lf_rec24 r;
    r.a = a[i];
    r.dx = dx[i];
    r.up = (unsigned)ups_ptr[i] | ((unsigned)(ups_ptr[i + 1] - ups_ptr[i]) << 28);
    r.base = ups_base[i];
    rec[i] = r;
}

// the (a, dx) records of k_level<.., STATICS = 1> from the router's static vectors (once per router and section)
__global__ void __launch_bounds__(kLevelBlock) k_static_records(long long n, const double *__restrict__ a, const double *__restrict__ dx,
                                                                double2 *__restrict__ adx)
{
    const long long i = (long long)blockIdx.x * kLevelBlock + threadIdx.x;
    if (i < n) adx[i] = make_double2(a[i], dx[i]);
}

// Several routers on ONE graph (surface_routing.py:151-153: the direct / other / forest overland routers differ only in
// alpha and in their vectors) swept together: blockIdx.y (wide levels) or blockIdx.x (narrow runs) picks the router, so a
// level costs one launch for all of them.
constexpr int kMaxMulti = 4;
struct sweep_args_multi {
    sweep_args r[kMaxMulti];
};

template <bool FUSED, bool ORDERED>
__global__ void __launch_bounds__(kBlock) LF_LEVEL_ATTR k_level_multi(int first, int count, sweep_args_multi M)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    sweep_cell<FUSED, ORDERED, false>(first + i, M.r[blockIdx.y]);
}

template <bool FUSED, bool ORDERED>
__global__ void __launch_bounds__(kNarrowBlock) k_levels_narrow_multi(int k0, int k1, const long long *__restrict__ level_start,
                                                                      sweep_args_multi M)
{
    const sweep_args &A = M.r[blockIdx.x];
    for (int k = k0; k < k1; ++k) {
        const int first = (int)level_start[k], last = (int)level_start[k + 1];
        for (int p = first + (int)threadIdx.x; p < last; p += kNarrowBlock) sweep_cell<FUSED, ORDERED, false>(p, A);
        __threadfence_block();
        __syncthreads();
    }
}

// One BLOCK of consecutive levels of a router call, cone by cone (the plan of lf_router.hip: build_level_blocks).  A
// workgroup owns a chunk of the block's last level and the whole upstream cone above it -- level by level one contiguous
// range of at most CW cells, the cones tile every level -- so the levels of a block need no synchronisation between
// workgroups: the new discharges travel to the next level through LDS (two buffers by level parity; they are also
// stored, the block after this one and later calls read them).  One level of a cone is a dependent chain about as long
// as one trip to memory and nothing else runs on its SIMD, so the operands of a level are requested TWO levels ahead
// (three rotating register sets), the request holds loaded values only and sits behind no branch, the stores of a level
// leave one level later, and the rarely taken general-exponent paths live out of line.  NR
// routers of one graph (the overland routers of surface_routing.py:151-153) share the cone.  Arithmetic per cell =
// sweep_cell: bit-identical to the level sweep.
struct cone_plan_args {
    const int *__restrict__ cone; // starts of this block's cones, nl per cone, then the closing row (ends of the levels)
    int nl;                       // levels of the block
    int n_cells;                  // cells of the graph (k_sweep_cones_split: extent of the state vectors, < 2^29)
};

template <int CW>
__device__ __forceinline__ void cone_sync() // between the levels of a cone: workgroup barrier, or nothing for one wavefront
{
    if (CW > 64)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else
        asm volatile("" ::: "memory"); // its LDS operations complete in order
}

// CW: cells per level of a cone = threads of the workgroup (64: one wavefront, no barrier between the levels)
// (the kernel's body: cone `cone` of the block for the NR routers of M -- k_sweep_cones_members runs it on one member's
// state vectors)
template <bool FUSED, bool ORDERED, int NR, int CW>
__device__ __forceinline__ void sweep_cone(unsigned cone, const cone_plan_args &C, const sweep_args_multi &M)
{
    __shared__ double x[NR][2][CW];
    const int tid = threadIdx.x, nl = C.nl;
    const int *c0 = C.cone + (size_t)cone * nl, *c1 = c0 + nl;
    struct cell { // the operands of one cell as loaded: no arithmetic before the level that solves it (a product here
                  // would make the loads wait where they are issued)
        int u0, u1, pix;
        double ap[NR], lat[NR], dx[NR], qold[NR];
        bool active;
    };
    auto load = [&](int p, bool active, cell &R) {
        R.active = active;
        const int pc = active ? p : 0; // lanes beyond the cone's range load cell 0: no branch around the loads
        R.u0 = M.r[0].ups_ptr[pc];
        R.u1 = M.r[0].ups_ptr[pc + 1];
        R.pix = ORDERED ? pc : M.r[0].perm[pc];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const sweep_args &A = M.r[r];
            R.ap[r] = A.a[pc];
            if (FUSED) {
                R.lat[r] = A.lat[R.pix];
                R.dx[r] = A.dx ? A.dx[pc] : A.dx_scalar;
                R.qold[r] = ORDERED ? A.qord[pc] : A.q_pix[R.pix];
            } else {
                R.lat[r] = A.constant[pc];
                R.dx[r] = 1.0;
                R.qold[r] = 0.0;
            }
        }
    };
    int first_up = 0;
    // the stores of a level are issued one level later, right behind the barrier (with the next loads): then everything
    // outstanding at the end of a level was issued before its arithmetic, and the wait there is short
    double pend_q[NR];
    int pend_p = 0, pend_pix = 0;
    bool pend = false;
    auto flush = [&]() {
        if (!pend) return;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            M.r[r].qord[pend_p] = pend_q[r];
            if (!ORDERED) M.r[r].q_pix[pend_pix] = pend_q[r];
        }
        pend = false;
    };
    // Software pipeline of depth 2: level j is solved from operands loaded while level j - 2 was solved, so a load has two
    // level times to arrive (one level of a cone takes about as long as one trip to memory: with depth 1 every level
    // waited for its own loads).  Three operand sets rotate; the waits are the compiler's (vmcnt counts the loads and
    // stores issued since, nothing is waited for that is not needed).
    auto level = [&](int j, const cell &cur, cell &nn, int first, int last, int fn2, int ln2) {
        const int p = first + tid;
        flush();
        load(fn2 + tid, fn2 + tid < ln2, nn); // nothing of them depends on this launch; beyond the block: bounds 0, 0
        if (j > 0) { // level j-1 of this cone is in LDS
            if (CW > 64)
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            else
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // one wavefront: its LDS operations complete in order
        }
        // every lane runs the level's arithmetic (a lane beyond the cone's range: on cell 0, nothing of it is kept), the
        // quintic path without a branch on sanitised arguments -- the loop over the levels is straight code but for the
        // block's first level and the out-of-line general path (single lanes with extreme arguments, or beta != 3/5)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const sweep_args &A = M.r[r];
            double v[8];
            if (j == 0) { // from the block before (previous launch)
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = (k < A.kmax && cur.u0 + k < cur.u1) ? A.qord[cur.u0 + k] : 0.0;
            } else {
                const double *y = &x[r][(j - 1) & 1][0];
                const int base = cur.u0 - first_up;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const bool have = k < A.kmax && cur.u0 + k < cur.u1;
                    const double t = y[have ? base + k : 0];
                    v[k] = have ? t : 0.0;
                }
            }
            double ups = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) ups += v[k];
            const double ap = cur.ap[r];
            double q;
            if (FUSED) {
                const double qo = cur.qold[r];
                const bool fq = lf_fast_range(qo);
                const double rt = lf_root5(fq ? qo : 1.0);
                double pw = fq ? rt * rt * rt : 0.0;                  // lf_pow_3_5: +-0 -> +0
                if (!fq && qo != 0.0) pw = lf_pow_cold(qo, 0.6);      // beyond the fast range, NaN
                const double c = ups + (ap * pw + cur.lat[r] * cur.dx[r]);
                const bool fc = lf_fast_range(c) && lf_fast_range(ap);
                const bool solve = fc && !(c <= LF_NEWTON_TOL);
                q = lf_solve_3_5(solve ? c : 1.0, solve ? ap : 1.0);
                q = solve ? q : 0.0;                                   // fast range and c <= NEWTON_TOL: 0
                if (!fc) q = lf_solve_cell_cold(c, ap, A.beta * ap, A.beta, A.inv_beta, A.b_minus_1);
            } else {
                const double c = ups + cur.lat[r];
                q = lf_solve_cell(c, ap, A.beta * ap, A.beta, A.inv_beta, A.b_minus_1);
            }
            pend_q[r] = q;
            if (j + 1 < nl) x[r][j & 1][tid] = q;
        }
        pend = cur.active;
        pend_p = p;
        pend_pix = cur.pix;
        first_up = first;
        (void)last;
    };
    auto bound = [&](const int *t, int k) { return k < nl ? ld_table(t, k) : 0; };
    cell r0, r1, r2;
    int f0 = ld_table(c0, 0), f1 = bound(c0, 1), f2 = bound(c0, 2), l0 = ld_table(c1, 0), l1 = bound(c1, 1), l2 = bound(c1, 2);
    load(f0 + tid, f0 + tid < l0, r0);
    load(f1 + tid, f1 + tid < l1, r1);
    // three levels per trip, no branch around a level or its loads (the wait counts stay exact): a level beyond the block
    // has the bounds 0, 0 -- no active cell, only its barrier
    for (int j = 0; j < nl; j += 3) {
        // bounds of the levels whose operands this round of three requests
        const int f3 = bound(c0, j + 3), l3 = bound(c1, j + 3), f4 = bound(c0, j + 4), l4 = bound(c1, j + 4);
        const int f5 = bound(c0, j + 5), l5 = bound(c1, j + 5);
        level(j, r0, r2, f0, l0, f2, l2);
        level(j + 1, r1, r0, f1, l1, f3, l3);
        level(j + 2, r2, r1, f2, l2, f4, l4);
        f0 = f3;
        f1 = f4;
        f2 = f5;
        l0 = l3;
        l1 = l4;
        l2 = l5;
    }
    flush();
}
template <bool FUSED, bool ORDERED, int NR, int CW = kBlock>
__global__ void __launch_bounds__(CW) k_sweep_cones(cone_plan_args C, sweep_args_multi M)
{
    sweep_cone<FUSED, ORDERED, NR, CW>(blockIdx.x, C, M);
}

// The cone sweep with the work split between TWO wavefronts of a 128-thread workgroup (round 4).  One level of a cone is
// a dependent chain that a single wavefront issues in order; on chain-bound networks three quarters of the SIMDs idle while
// that wavefront also works out everything that does NOT depend on the level above (operand addresses and loads, the
// old-discharge term a*Qold^0.6 + q*dx, the stores).  Here
//   * the SUPPLY wavefront (threads 64..127) runs a chunk of KC levels ahead: it requests every operand of the chunk at
//     once, works out the constant term of every cell (kinematic_wave_parallel.py:163,175) and parks it in LDS together
//     with a and the cell's upstream range as (first slot, count) in the level above; one chunk later it takes the chunk's
//     new discharges out of LDS and stores them;
//   * the CHAIN wavefront (threads 0..63) touches LDS and registers only: gather the level above -> sum in ascending
//     pixel id (kinematic_wave_parallel_tools.py:57-58) -> closure solve -> LDS.
// The two meet at one workgroup barrier per chunk; operand and result buffers alternate by chunk parity.  The upstream
// discharges of the block's first level are final in memory (the block before): the supply wavefront adds them up and
// hands the chain wavefront c = ups + constant with an empty range (0.0 + c == c for every c that is solved; c == -0.0
// gives 0 either way).  Arithmetic per cell = sweep_cell: bit-identical to the level sweep.
#ifndef LF_CONE_KC
#define LF_CONE_KC 8 /* levels per chunk and supply wavefronts of the few-cones shape (lf_router.hip: launch_sweep_cones) */
#endif
#ifndef LF_CONE_NS
#define LF_CONE_NS 4
#endif
constexpr int kConeSlots = 65;           // a level's 64 discharges + one slot holding 0.0 ("no such upstream cell" reads it)
constexpr int kConeRow = kConeSlots * 8; // bytes of a row

// What the supply wavefronts park for a chunk of KC levels, per lane in 16-byte records (one ds_read_b128 each).
struct cone_rec_ca {
    double cst; // a*Qold^beta + q*dx (first level of the block: + the inflow from the block before)
    double ap;  // a, 1.0 where a is outside the fast range (the cold path reads the true value from memory)
};
struct cone_rec_fl {
    float af, laf; // (float)a and log2 of it: the part of lf_solve_3_5's seed that does not depend on c
    int fast_a;    // a in the fast range
    int pos;       // the position the lane's operands were read from (cell 0 for a lane beyond the cone's range)
};
struct cone_rec_ad {
    int ad[4]; // byte offsets (in the result rows) of four reads of the level above: slot first + k, or the 0.0 in slot 64
};
template <int NR, int KC>
struct cone_chunk_ops {
    cone_rec_ca ca[KC][NR][64];
    cone_rec_fl fl[KC][NR][64];
    cone_rec_ad ad[KC][2][64]; // reads 0..3 and 4..7 of router 0 (router r: + r rows)
};
template <int NR, int KC>
struct cone_lds {
    double xr[2 * KC * NR][kConeSlots]; // row (chunk parity * KC + level of the chunk) * NR + router; first: small offsets
    cone_chunk_ops<NR, KC> ops[2];
};

// The chain wavefront's loop over the chunks, for a graph of at most KM upstream cells per cell: LDS and registers only.
template <bool FUSED, int NR, int KC, int KM>
__device__ __forceinline__ void cone_chain(cone_lds<NR, KC> &S, int tid, int nl, const int *c0, const sweep_args_multi &M)
{
    const int nch = (nl + KC - 1) / KC;
    const char *xb = (const char *)&S.xr[0][0];
    struct operands {
        cone_rec_ca ca[NR];
        cone_rec_fl fl[NR];
        cone_rec_ad a0, a1;
    };
    auto request = [&](const cone_chunk_ops<NR, KC> &O, int jj, operands &P) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            P.ca[r] = O.ca[jj][r][tid];
            P.fl[r] = O.fl[jj][r][tid];
        }
        P.a0 = O.ad[jj][0][tid];
        if (KM > 4) P.a1 = O.ad[jj][1][tid];
    };
    for (int ch = 0; ch < nch; ++ch) {
        const int ob = ch & 1, L = nl - ch * KC < KC ? nl - ch * KC : KC;
        const cone_chunk_ops<NR, KC> &O = S.ops[ob];
        // one level: `cur` holds its operands, those of the next level are requested into `nxt` behind the gather
        auto level = [&](int jj, const operands &cur, operands &nxt) {
            // the level above, all reads in flight together
            double t[NR][KM];
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int k = 0; k < KM; ++k) // (router r: r rows on; slot 64 of EVERY row holds 0.0)
                    t[r][k] = *(const double *)(xb + (k < 4 ? cur.a0.ad[k & 3] : cur.a1.ad[k & 3]) + r * kConeRow);
            request(O, jj + 1 < L ? jj + 1 : jj, nxt); // (the chunk's last level: its own again)
            const int row = (ob * KC + jj) * NR;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                // ascending pixel id (kinematic_wave_parallel_tools.py:57-58); the reference starts from 0.0, and 0.0 + x
                // is x bit for bit unless x is -0.0, which no discharge written to LDS is (0.0, a positive root, or NaN)
                double ups = t[r][0];
#pragma unroll
                for (int k = 1; k < KM; ++k) ups += t[r][k];
                const double c = ups + cur.ca[r].cst;
                double q;
                if (FUSED) {
                    // c <= NEWTON_TOL: 0 on every path; else the quintic when c and a are in its range, else the general
                    // path (c beyond 1e30, NaN, a outside the fast range: kinematic_wave_parallel_tools.py:59-82)
                    const bool le = c <= LF_NEWTON_TOL;
                    const bool quintic = c <= LF_FAST_MAX && cur.fl[r].fast_a != 0;
#ifdef LF_EXP_NOSOLVE /* timing experiments only (tools/build_variant.sh): WRONG results, bounded values */
                    q = c * 1e-3 + 0.5 * cur.ca[r].cst;
#else
                    q = lf_solve_3_5_pre(c, cur.ca[r].ap, cur.fl[r].af, cur.fl[r].laf); // (lanes not selected: garbage)
#endif
                    q = (le || !quintic) ? 0.0 : q;
                    if (!le && !quintic) {
                        const sweep_args &A = M.r[r];
                        const double at = A.a[cur.fl[r].pos]; // (a lane beyond the cone's range: cell 0, like its other operands)
                        q = lf_solve_cell_cold(c, at, A.beta * at, A.beta, A.inv_beta, A.b_minus_1);
                    }
                } else {
                    const sweep_args &A = M.r[r];
                    q = lf_solve_cell(c, cur.ca[r].ap, A.beta * cur.ca[r].ap, A.beta, A.inv_beta, A.b_minus_1);
                }
                S.xr[row + r][tid] = q;
            }
        };
        operands pa, pb; // two sets, swapping roles level by level (no copies)
        request(O, 0, pa); // the chunk's first level; inside the chunk the operands are requested one level ahead
#ifdef LF_EXP_NOCHAIN /* timing experiments only: the supply side alone, WRONG results */
        for (int jj = 0; jj < L; ++jj) S.xr[(ob * KC + jj) * NR][tid] = 1.0;
        for (int jj = 0; jj < 0; jj += 2) {
#else
        for (int jj = 0; jj < L; jj += 2) {
#endif
            level(jj, pa, pb);
            if (jj + 1 >= L) break;
            level(jj + 1, pb, pa);
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
}

// NS supply wavefronts share a chunk level by level (wavefront s: levels s, s + NS, ... of every chunk); each keeps the
// operands of its levels of the NEXT chunk in flight while it works out the current one (two register sets).
template <bool FUSED, bool ORDERED, int NR, int KC, int NS>
__global__ void __launch_bounds__(64 * (1 + NS)) k_sweep_cones_split(cone_plan_args C, sweep_args_multi M)
{
    __shared__ cone_lds<NR, KC> S;
    static_assert(2 * KC * NR <= 64, "one lane per row");
    static_assert(KC % NS == 0, "every supply wavefront takes KC / NS levels of a chunk");
    constexpr int KS = KC / NS;
    const int tid = threadIdx.x & 63, nl = C.nl;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // 0 = chain, 1.. = supply (uniform: scalar table reads)
    const int nch = (nl + KC - 1) / KC;
    const int *c0 = C.cone + (size_t)blockIdx.x * nl, *c1 = c0 + nl;
    if (wave == 0) {
        if (tid < 2 * KC * NR) S.xr[tid][64] = 0.0; // the zero slot of every row
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); // chunk 0 is in LDS
        switch (M.r[0].kmax) {
        case 0:
        case 1: cone_chain<FUSED, NR, KC, 1>(S, tid, nl, c0, M); break;
        case 2: cone_chain<FUSED, NR, KC, 2>(S, tid, nl, c0, M); break;
        case 3: cone_chain<FUSED, NR, KC, 3>(S, tid, nl, c0, M); break;
        case 4: cone_chain<FUSED, NR, KC, 4>(S, tid, nl, c0, M); break;
        case 5: cone_chain<FUSED, NR, KC, 5>(S, tid, nl, c0, M); break;
        case 6: cone_chain<FUSED, NR, KC, 6>(S, tid, nl, c0, M); break;
        case 7: cone_chain<FUSED, NR, KC, 7>(S, tid, nl, c0, M); break;
        default: cone_chain<FUSED, NR, KC, 8>(S, tid, nl, c0, M); break;
        }
        return;
    }
    // ---- a supply wavefront ----
    // Its loop over the chunks is straight code but for the out-of-line pow of an extreme old discharge: no branch around
    // a load or a store (lanes beyond the cone's range load cell 0 and store beyond the end of a buffer resource, which the
    // hardware drops; phases beyond the block work on empty levels), so the compiler's wait counts stay exact and the
    // operands requested during one phase are not waited for before the next.
    const int sw = wave - 1;
    typedef int v2i __attribute__((ext_vector_type(2)));
    __amdgpu_buffer_rsrc_t q_rsrc[NR], qpix_rsrc[NR];
    const double *dxp[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        q_rsrc[r] = __builtin_amdgcn_make_buffer_rsrc(M.r[r].qord, 0, (int)((unsigned)C.n_cells * 8u), 0x00020000);
        qpix_rsrc[r] = __builtin_amdgcn_make_buffer_rsrc(ORDERED ? M.r[r].qord : M.r[r].q_pix, 0, (int)((unsigned)C.n_cells * 8u), 0x00020000);
        dxp[r] = M.r[r].dx ? M.r[r].dx : M.r[r].a; // (no per-pixel dx: any valid stream, the scalar is selected)
    }
    auto lbound = [&](const int *t, int k) { // entry k of a cone's row of the plan, 0 outside the block: an unconditional
        const bool in = (unsigned)k < (unsigned)nl; // scalar load and a select, no branch in the load step
        const int v = ld_table(t, in ? k : 0);
        return in ? v : 0;
    };
    struct opset { // the operands of this wavefront's KS levels of a chunk, as loaded
        int u0[KS], u1[KS], pix[KS];
        double ap[KS][NR], lat[KS][NR], dx[KS][NR], qo[KS][NR];
        bool act[KS];
    };
    auto issue = [&](int ph, opset &P) { // independent loads, all in flight together
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            const int j = ph * KC + sw + i * NS;
            const int p = lbound(c0, j) + tid;
            P.act[i] = p < lbound(c1, j);    // a level beyond the block: bounds 0, 0
            const int pc = P.act[i] ? p : 0; // lanes beyond the cone's range load cell 0: no branch around the loads
            P.u0[i] = M.r[0].ups_ptr[pc];
            P.u1[i] = M.r[0].ups_ptr[pc + 1];
            P.pix[i] = ORDERED ? pc : M.r[0].perm[pc];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const sweep_args &A = M.r[r];
                P.ap[i][r] = A.a[pc];
                if (FUSED) {
                    P.lat[i][r] = A.lat[P.pix[i]];
                    P.dx[i][r] = dxp[r][pc];
                    P.qo[i][r] = ORDERED ? A.qord[pc] : A.q_pix[P.pix[i]];
                } else {
                    P.lat[i][r] = A.constant[pc];
                    P.dx[i][r] = 1.0;
                    P.qo[i][r] = 0.0;
                }
            }
        }
    };
    auto store = [&](int ph) { // results of chunk ph - 2: out of LDS, into the state vector
        const int ob = ph & 1;
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            const int jj = sw + i * NS, j = (ph - 2) * KC + jj;
            const int p = lbound(c0, j) + tid;
            const bool act = p < lbound(c1, j);
            const unsigned off = act ? (unsigned)p * 8u : 0xffffffffu; // beyond the buffer: dropped
            unsigned off_pix = off;
            if (!ORDERED) {
                const int pix = M.r[0].perm[act ? p : 0];
                off_pix = act ? (unsigned)pix * 8u : 0xffffffffu;
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const double q = S.xr[(ob * KC + jj) * NR + r][tid];
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i, q), q_rsrc[r], off, 0, 0);
                if (!ORDERED) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i, q), qpix_rsrc[r], off_pix, 0, 0);
            }
        }
    };
    auto finish = [&](int ph, const opset &P, auto first_chunk) { // constant terms of chunk ph
        const int ob = ph & 1;
        cone_chunk_ops<NR, KC> &O = S.ops[ob];
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            const int jj = sw + i * NS, j = ph * KC + jj;
            const bool block_top = decltype(first_chunk)::value && i == 0 && sw == 0; // the block's first level
            // the reads of the level above: its rows are those of level jj - 1 of this chunk or the last of the chunk before
            const int above = jj > 0 ? (ob * KC + jj - 1) * NR : ((ob ^ 1) * KC + KC - 1) * NR;
            int cnt = P.act[i] ? P.u1[i] - P.u0[i] : 0;
            const int ab = above * kConeRow + (((P.u0[i] - lbound(c0, j - 1)) & 0xff) << 3);
            cone_rec_ad a0, a1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a0.ad[k] = (k < cnt && !block_top) ? ab + 8 * k : 64 * 8;
                a1.ad[k] = (k + 4 < cnt && !block_top) ? ab + 8 * (k + 4) : 64 * 8;
            }
            O.ad[jj][0][tid] = a0;
            O.ad[jj][1][tid] = a1;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const sweep_args &A = M.r[r];
                double cst;
                if (FUSED) {
                    const double q = P.qo[i][r];
                    const bool fq = lf_fast_range(q);
                    const double rt = lf_root5(fq ? q : 1.0);
                    double pw = fq ? rt * rt * rt : 0.0;           // lf_pow_3_5: +-0 -> +0
                    if (!fq && q != 0.0) pw = lf_pow_cold(q, 0.6); // beyond the fast range, NaN
                    cst = P.ap[i][r] * pw + P.lat[i][r] * (A.dx ? P.dx[i][r] : A.dx_scalar);
                } else {
                    cst = P.lat[i][r];
                }
                if (decltype(first_chunk)::value && i == 0) {
                    if (block_top) { // its upstream cells are final in memory (the block before)
                        double v[8];
#pragma unroll
                        for (int k = 0; k < 8; ++k) v[k] = (k < A.kmax && k < cnt) ? A.qord[P.u0[i] + k] : 0.0;
                        double ups = 0.0;
#pragma unroll
                        for (int k = 0; k < 8; ++k) ups += v[k];
                        cst = ups + cst;
                    }
                }
                const bool fast_a = lf_fast_range(P.ap[i][r]);
                cone_rec_ca ca;
                ca.cst = cst;
                ca.ap = (fast_a || !FUSED) ? P.ap[i][r] : 1.0;
                cone_rec_fl fl;
                fl.af = (float)ca.ap;
                fl.laf = __builtin_amdgcn_logf(fl.af);
                fl.fast_a = fast_a;
                fl.pos = P.act[i] ? lbound(c0, j) + tid : 0;
                O.ca[jj][r][tid] = ca;
                O.fl[jj][r][tid] = fl;
            }
        }
    };
    // phase ph: request chunk ph + 1, store chunk ph - 2, work out chunk ph; barriers behind the phases 0 .. nch
    opset SA, SB;
    issue(0, SA);
    issue(1, SB);
    finish(0, SA, std::true_type());
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int ph = 1; ph <= nch; ph += 2) {
        issue(ph + 1, SA);
        store(ph);
        finish(ph, SB, std::false_type());
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (ph + 1 > nch) break;
        issue(ph + 2, SB);
        store(ph + 1);
        finish(ph + 1, SA, std::false_type());
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    store(nch + 1);
}

// The same on the row-block partition (lf_dist.hip; one router, sweep-order vectors, one wavefront per cone).  A cell's
// upstream cells are the consecutive run starting at ups_base or come from the list ups_idx; those in the unit above of
// this cone are new this launch and come from LDS, all others -- ghost slots, earlier phases, the block before -- are
// final in the state vector.  Reading those inside the level would cost two dependent trips to memory on every level that
// has one such cell, so the prefetch has THREE stages over five rotating register sets:
//   A  four units ahead: upstream range, run start and the operands;
//   B  two units ahead:  the upstream positions (run start + k, or the list entries -- needs A);
//   C  one unit ahead:   the discharges of the positions that are not in the unit above (needs B; usually L2 hits);
// the level itself touches LDS and registers only.  qold_src: the old discharge from a second state vector (pipelined calls).
template <bool FUSED>
__global__ void __launch_bounds__(64) k_sweep_cones_dist(cone_plan_args C, sweep_args A)
{
    __shared__ double x[2][64];
    const int tid = threadIdx.x, nl = C.nl;
    const int *c0 = C.cone + (size_t)blockIdx.x * nl, *c1 = c0 + nl;
    const double *qold_from = A.qold_src ? A.qold_src : A.qord;
    const int kmax = A.kmax;
    struct cell {
        int u0, u1, base, p;
        double ap, lat, dx, qold;
        int e[8];
        double gq[8];
        bool active;
    };
    auto stage_a = [&](int first, int last, cell &R) {
        const int p = first + tid;
        R.active = p < last;
        const int pc = R.active ? p : 0; // a lane beyond the cone's range: cell 0, nothing of it is kept
        R.p = p;
        R.u0 = A.ups_ptr[pc];
        R.u1 = A.ups_ptr[pc + 1];
        R.base = A.ups_base[pc];
        R.ap = A.a[pc];
        if (FUSED) {
            R.lat = A.lat[pc];
            R.dx = A.dx ? A.dx[pc] : A.dx_scalar;
            R.qold = qold_from[pc];
        } else {
            R.lat = A.constant[pc];
            R.dx = 1.0;
            R.qold = 0.0;
        }
    };
    auto stage_b = [&](cell &R) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool have = k < kmax && R.u0 + k < R.u1;
            int e = R.base + k;
            if (R.base < 0) e = have ? A.ups_idx[R.u0 + k] : 0; // ghost or cross-phase inflow: from the list
            R.e[k] = have ? e : -1;
        }
    };
    // [fa, la): the cone's range in the unit above (empty for the block's first unit: everything comes from memory)
    auto stage_c = [&](cell &R, int fa, int la) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = R.e[k];
            const bool ext = e >= 0 && !(e >= fa && e < la);
            R.gq[k] = 0.0;
            if (ext) R.gq[k] = A.qord[e];
        }
    };
    double pend_q = 0.0;
    int pend_p = 0;
    bool pend = false;
    auto level = [&](int j, const cell &cur, cell &n1, cell &n2, cell &n4, int first, int last, int fa, int la, int f4,
                     int l4) {
        if (pend) A.qord[pend_p] = pend_q;
        stage_a(f4, l4, n4);
        stage_b(n2);
        stage_c(n1, first, last);
        if (j > 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // one wavefront: its LDS operations complete in order
        const double *y = &x[(j - 1) & 1][0];
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = cur.e[k];
            const bool above = e >= fa && e < la;
            const double t = y[above ? e - fa : 0];
            v[k] = above ? t : cur.gq[k]; // (no upstream cell k: gq = 0)
        }
        double ups = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) ups += v[k];
        const double ap = cur.ap;
        double q;
        if (FUSED) {
            const double qo = cur.qold;
            const bool fq = lf_fast_range(qo);
            const double rt = lf_root5(fq ? qo : 1.0);
            double pw = fq ? rt * rt * rt : 0.0;
            if (!fq && qo != 0.0) pw = lf_pow_cold(qo, 0.6);
            const double c = ups + (ap * pw + cur.lat * cur.dx);
            const bool fc = lf_fast_range(c) && lf_fast_range(ap);
            const bool solve = fc && !(c <= LF_NEWTON_TOL);
            q = lf_solve_3_5(solve ? c : 1.0, solve ? ap : 1.0);
            q = solve ? q : 0.0;
            if (!fc) q = lf_solve_cell_cold(c, ap, A.beta * ap, A.beta, A.inv_beta, A.b_minus_1);
        } else {
            q = lf_solve_cell(ups + cur.lat, ap, A.beta * ap, A.beta, A.inv_beta, A.b_minus_1);
        }
        x[j & 1][tid] = q;
        pend = cur.active;
        pend_p = cur.p;
        pend_q = q;
    };
    auto bound = [&](const int *t, int k) { return k < nl ? ld_table(t, k) : 0; };
    cell s0, s1, s2, s3, s4;
    int f[5], l[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        f[i] = bound(c0, i);
        l[i] = bound(c1, i);
    }
    stage_a(f[0], l[0], s0);
    stage_a(f[1], l[1], s1);
    stage_a(f[2], l[2], s2);
    stage_a(f[3], l[3], s3);
    stage_b(s0);
    stage_b(s1);
    stage_c(s0, 0, 0);
    int fa = 0, la = 0; // the cone's range in the unit above the current one
    for (int j = 0; j < nl; j += 5) {
        int fn[5], ln[5]; // bounds of the units j + 5 .. j + 9
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            fn[i] = bound(c0, j + 5 + i);
            ln[i] = bound(c1, j + 5 + i);
        }
        // (the exits leave the trip straight code: a stage of three units -- the tail phases -- does not pay for five)
        level(j, s0, s1, s2, s4, f[0], l[0], fa, la, f[4], l[4]);
        if (j + 1 >= nl) break;
        level(j + 1, s1, s2, s3, s0, f[1], l[1], f[0], l[0], fn[0], ln[0]);
        if (j + 2 >= nl) break;
        level(j + 2, s2, s3, s4, s1, f[2], l[2], f[1], l[1], fn[1], ln[1]);
        if (j + 3 >= nl) break;
        level(j + 3, s3, s4, s0, s2, f[3], l[3], f[2], l[2], fn[2], ln[2]);
        if (j + 4 >= nl) break;
        level(j + 4, s4, s0, s1, s3, f[4], l[4], f[3], l[3], fn[3], ln[3]);
        fa = f[4];
        la = l[4];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            f[i] = fn[i];
            l[i] = ln[i];
        }
    }
    if (pend) A.qord[pend_p] = pend_q;
}

// a run of narrow levels [k0, k1): one workgroup, barrier between levels
template <bool FUSED, bool ORDERED, bool INDEXED = false>
__global__ void __launch_bounds__(kNarrowBlock) k_levels_narrow(int k0, int k1, const long long *__restrict__ level_start,
                                                                sweep_args A)
{
    for (int k = k0; k < k1; ++k) {
        const int first = (int)level_start[k], last = (int)level_start[k + 1];
        for (int p = first + (int)threadIdx.x; p < last; p += kNarrowBlock) sweep_cell<FUSED, ORDERED, INDEXED>(p, A);
        __threadfence_block();
        __syncthreads();
    }
}

// ---- an ensemble on one or several routers (lf_router_route_ordered_members, .._members_multi) ---------------------------
// `members` state vectors that share a router's static vectors and so its whole launch schedule: member m's discharge
// and lateral inflow are rows m of two [members][stride] arrays in sweep order.  Every launch of the schedule covers all
// members; the argument block is one sweep_args (row 0) and member_rows, whatever the count.  Several routers of one graph
// (the overland routers of an ensemble; MULTI) hand over one such block each, M.r[i], with the same rows R.  The unit of
// work is (router, member), router-major: a unit picks its router's block (unit_block; one router: the block, the unit is
// the member) and then runs sweep_cell_state / sweep_cone on the member's view of it -- per cell and member bit-identical to
// the member swept alone.
struct member_rows {
    long long stride;  // elements between the rows of the state vectors (>= N)
    long long cstride; // ... and of `constant` (general exponent: N)
    int members;
};
__device__ __forceinline__ sweep_args member_view(sweep_args A, const member_rows &R, int m)
{
    A.qord += (long long)m * R.stride;
    A.lat += (long long)m * R.stride;
    if (A.constant) A.constant += (long long)m * R.cstride;
    return A;
}
template <bool MULTI>
using member_block = std::conditional_t<MULTI, sweep_args_multi, sweep_args>;
// the argument block of `unit`, of per_router units to a router, and the unit's number within its router
__device__ __forceinline__ const sweep_args &unit_block(const sweep_args &A, int &, int) { return A; }
__device__ __forceinline__ const sweep_args &unit_block(const sweep_args_multi &M, int &unit, int per_router)
{
    const int router = unit / per_router;
    unit -= router * per_router;
    return M.r[router];
}

// k_prep for all units: blockIdx.y = unit, vectors in sweep order
template <bool MULTI>
__global__ void __launch_bounds__(kBlock) k_prep_members(int n, member_block<MULTI> B, member_rows R)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    int m = (int)blockIdx.y;
    const sweep_args &A = unit_block(B, m, R.members);
    double *__restrict__ constant = const_cast<double *>(A.constant);
    const long long row = (long long)m * R.stride;
    const double lateral = A.lat[row + p] * (A.dx ? A.dx[p] : A.dx_scalar); // (k_prep's expression, sweep order)
    constant[(long long)m * R.cstride + p] = A.a[p] * pow(A.qord[row + p], A.beta) + lateral;
}

// One wide level for all units: a lane owns one cell for a group of MB members (blockIdx.y = router * groups + group; a
// router's last group may be short, so a group stays within one router, whose (a, dx) the lane holds across it).  The
// cell's static operands -- the (a, dx) record or a and dx, and the ups_ptr pair -- are loaded once and stay in registers;
// per member the requests then go out in sweep_cell_state's order.  (Sharing them through L2 instead would depend on which
// XCD a workgroup lands on.)  The members one after the other, each behind its own uniform branch (in a loop the compiler
// hoists the solve's constants out of it and runs out of registers).
// One member per lane is k_level's code at k_level's 8 wavefronts per SIMD; with the statics held across two or four
// members the kernel needs 77 VGPRs (75 for several routers), and forced into 64 it spills: 6 wavefronts per SIMD (80 VGPRs), no scratch.
#define LF_MEMBERS_ATTR(MB) __attribute__((amdgpu_waves_per_eu((MB) == 1 ? 8 : 6)))
template <bool FUSED, bool ORDERED, int STATICS, int MB, bool MULTI>
__global__ void __launch_bounds__(kLevelBlock) LF_MEMBERS_ATTR(MB) k_level_members(int first, int count, member_block<MULTI> B, member_rows R)
{
    static_assert(ORDERED && (STATICS == 0 || (STATICS == 1 && FUSED)), "members lie in sweep order; records: (a, dx)");
    const int i = blockIdx.x * kLevelBlock + threadIdx.x;
    if (i >= count) return;
    int group = (int)blockIdx.y;
    const sweep_args &A = unit_block(B, group, (R.members + MB - 1) / MB);
    const int m0 = group * MB;
    const int p = first + i;
    const int u0 = A.ups_ptr[p], u1 = A.ups_ptr[p + 1];
    double ap, dxp;
    sweep_cell_statics<FUSED, STATICS>(p, A, ap, dxp);
#pragma unroll
    for (int j = 0; j < MB; ++j)
        if (m0 + j < R.members) sweep_cell_state<FUSED, ORDERED, false, STATICS>(p, p, ap, dxp, u0, u1, 0, member_view(A, R, m0 + j));
}

// A run of narrow levels: k_levels_narrow's walk, one workgroup per unit (blockIdx.x)
template <bool FUSED, bool ORDERED, bool MULTI>
__global__ void __launch_bounds__(kNarrowBlock) k_levels_narrow_members(int k0, int k1, const long long *__restrict__ level_start,
                                                                        member_block<MULTI> B, member_rows R)
{
    int m = (int)blockIdx.x;
    const sweep_args &A = unit_block(B, m, R.members);
    const sweep_args V = member_view(A, R, m);
    for (int k = k0; k < k1; ++k) {
        const int first = (int)level_start[k], last = (int)level_start[k + 1];
        for (int p = first + (int)threadIdx.x; p < last; p += kNarrowBlock) sweep_cell<FUSED, ORDERED, false>(p, V);
        __threadfence_block();
        __syncthreads();
    }
}

// A level block: k_sweep_cones' cone (one router), blockIdx.y = unit
template <bool FUSED, bool ORDERED, int CW, bool MULTI>
__global__ void __launch_bounds__(CW) k_sweep_cones_members(cone_plan_args C, member_block<MULTI> B, member_rows R)
{
    int m = (int)blockIdx.y;
    const sweep_args &A = unit_block(B, m, R.members);
    sweep_args_multi U;
    U.r[0] = member_view(A, R, m);
    sweep_cone<FUSED, ORDERED, 1, CW>(blockIdx.x, C, U);
}

// ================================================================================================
// Host side: what the single domain's router (lf_router.hip: lf_router) and the row-block partition's (lf_dist.hip:
// lf_dist_router) have in common -- lf_router_core, its setup and the launch schedule of a plain router call.
// ================================================================================================

// The part of a router that both kinds share; lf_router and lf_dist_router derive from it and add what is theirs.
struct lf_router_core {
    int device = 0;
    lf_device_ctx *ctx = nullptr;
    int64_t N = 0;
    int kmax = 8;
    double beta = 0, inv_beta = 0, b_minus_1 = 0, dx_scalar = 0, dt = 0;
    bool has_floodplains = false, dx_per_pixel = false;
    bool fused = false; // beta == 3/5: prep fused into the sweep, polynomial closure solve (lf_math.h)
    lf_dbuf<unsigned int> derived_ok; // fused sub-steps: flags of k_check_derived (fused_args::recompute)
    lf_dbuf<uint8_t> isolated; // [N] by position: 1 = no upstream and no downstream cell (lf_router; n_isolated of them)
    lf_dbuf<uint8_t> inert;    // [N] per fused call: isolated, not a channel, zero split-routing thresholds (k_inert_flags)
    int64_t n_isolated = 0;
    lf_dbuf<int32_t> perm, ups_ptr;
    lf_dbuf<long long> level_start;
    lf_dbuf<double> a1, a2, dx, constant;
    lf_dbuf<double> fused_qr1, fused_qr2;     // fused sub-steps: router outputs by sub-step parity (fused_args::qr1 / qr2)
    lf_dbuf<double> fused_hist1, fused_hist2; // [nsteps][N] router outputs of every sub-step (k_fused_level_steps)
    size_t fused_hist_refused = SIZE_MAX;     // smallest history size that did not fit its budget (lf_history_ensure)
    int last_fused_form = 0; // schedule of the last fused_wavefront: 1 time-major, 2 level blocks, 3 levels (0: none yet)
    std::vector<int64_t> h_level_start;
    // level blocks and cones (lf_blocks.h) of the fused sub-step wavefront; empty: the level-by-level wavefront
    lf_block_plan fplan;
    lf_block_plan_dev fplan_dev;
    // the same for plain router calls (longer blocks: no sub-step dimension to fill the machine with, so fewer, longer
    // launches pay); empty: the segment schedule
    lf_block_plan rplan;
    lf_block_plan_dev rplan_dev;
    // the static vectors of a cell as one record per section for the wide levels of ordered beta = 3/5 calls (k_level<..,
    // STATICS>) are built on the first such call; statics_refused: the allocation failed once, the separate streams stay
    bool statics_refused = false;
};

// position <-> pixel order of a vector through perm (dst_ord[p] = src_pix[perm[p]] and back)
__global__ void __launch_bounds__(kBlock) k_gather(int n, const int *__restrict__ perm, const double *__restrict__ src_pix,
                                                   double *__restrict__ dst_ord)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p < n) dst_ord[p] = src_pix[perm[p]];
}

// k_gather for several rows with one index table: blockIdx.y = row (lf_gather_rows_device)
__global__ void __launch_bounds__(kBlock) k_gather_rows(int n, const int *__restrict__ index, const double *__restrict__ src,
                                                        long long src_stride, double *__restrict__ dst, long long dst_stride)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p < n) dst[(long long)blockIdx.y * dst_stride + p] = src[(long long)blockIdx.y * src_stride + index[p]];
}

__global__ void __launch_bounds__(kBlock) k_scatter(int n, const int *__restrict__ perm, const double *__restrict__ src_ord,
                                                    double *__restrict__ dst_pix)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p < n) dst_pix[perm[p]] = src_ord[p];
}

// a vector of r's N cells from pixel order into engine (sweep) order and back, on r's stream
inline int core_to_engine_order(lf_router_core &r, const double *src_pix_dev, double *dst_ord_dev)
{
    LF_HIP(hipSetDevice(r.device));
    const int n = (int)r.N;
    if (n > 0)
        hipLaunchKernelGGL(k_gather, dim3(blocks_for(n)), dim3(kBlock), 0, r.ctx->stream, n, r.perm.p, src_pix_dev, dst_ord_dev);
    LF_HIP(hipGetLastError());
    return LF_OK;
}
inline int core_from_engine_order(lf_router_core &r, const double *src_ord_dev, double *dst_pix_dev)
{
    LF_HIP(hipSetDevice(r.device));
    const int n = (int)r.N;
    if (n > 0)
        hipLaunchKernelGGL(k_scatter, dim3(blocks_for(n)), dim3(kBlock), 0, r.ctx->stream, n, r.perm.p, src_ord_dev, dst_pix_dev);
    LF_HIP(hipGetLastError());
    return LF_OK;
}

// The instantiation of a kernel for two run-time flags: fn(std::bool_constant<a>, std::bool_constant<b>), its result
template <class Fn>
decltype(auto) pick_flags(bool a, bool b, Fn &&fn)
{
    if (a && b) return fn(std::true_type(), std::true_type());
    if (a) return fn(std::true_type(), std::false_type());
    if (b) return fn(std::false_type(), std::true_type());
    return fn(std::false_type(), std::false_type());
}

// ... for a count of 1 to 4 (routers swept together, accuflux vectors): fn(std::integral_constant<int, n>), its result
template <class Fn>
decltype(auto) pick_count(int n, Fn &&fn)
{
    if (n == 1) return fn(std::integral_constant<int, 1>());
    if (n == 2) return fn(std::integral_constant<int, 2>());
    if (n == 3) return fn(std::integral_constant<int, 3>());
    return fn(std::integral_constant<int, 4>());
}

// beta == 3/5 (every LISFLOOD setting): prep fused into the sweep, polynomial closure solve (lf_math.h).  LF_GENERAL_POW=1
// forces the general path (the reference's own Newton iteration with pow) for A/B parity and timing.
inline bool router_fused(double beta)
{
    const char *e = std::getenv("LF_GENERAL_POW");
    return beta == 0.6 && !(e && e[0] == '1');
}

// LF_LEVEL_STATICS=0: the wide levels read their static vectors as separate streams, not as one record per cell (A/B
// switch, read at every call)
inline bool level_statics_enabled()
{
    const char *e = std::getenv("LF_LEVEL_STATICS");
    return !(e && e[0] == '0');
}

// LF_DIST_OVERLAP=0: the row-block partition runs its halo rounds on the compute stream, not beside the bulk of a phase
// (A/B switch, read at every call)
inline bool dist_overlap_enabled()
{
    const char *e = std::getenv("LF_DIST_OVERLAP");
    return !(e && e[0] == '0');
}

// LF_LEVEL_COUNTS=0: the wide levels that read the records take the upstream range from ups_ptr, not from the count
// bytes (A/B switch, read at every call)
inline bool level_counts_enabled()
{
    const char *e = std::getenv("LF_LEVEL_COUNTS");
    return !(e && e[0] == '0');
}

// Do the wide levels of r's ordered calls read one record per cell (lf_router_core::statics_refused)?  Not with a scalar
// dx (the sweep then has one static load anyway), off the beta = 3/5 path, after a refusal or with LF_LEVEL_STATICS=0.
inline bool level_records_wanted(const lf_router_core &r)
{
    return r.fused && r.dx_per_pixel && !r.statics_refused && r.N > 0 && level_statics_enabled();
}

// The records of one section on their first use: `buf` for r's N cells (or `count` elements), which the caller then
// fills -> true; no memory for them (or !fits, the caller's own limit) -> refused for good, the HIP error cleared
template <class T>
bool level_records_alloc(lf_router_core &r, lf_dbuf<T> &buf, bool fits = true, size_t count = 0)
{
    if (fits && buf.alloc(count ? count : (size_t)r.N) == LF_OK) return true;
    r.statics_refused = true;
    (void)hipGetLastError();
    return false;
}

inline int check_section(const lf_router_core &r, int section)
{
    if (section != LF_SECTION_MAIN && section != LF_SECTION_FLOODPLAINS)
        return lf_set_error(LF_E_SECTION, "The section parameter must be either 'main_channel' or 'floodplain'!");
    if (section == LF_SECTION_FLOODPLAINS && !r.has_floodplains)
        return lf_set_error(LF_E_SECTION, "floodplains routing requested but alpha_floodplains was not given");
    return LF_OK;
}

// a_dx_div_dt = alpha * dx / dt, evaluated left to right (kinematic_wave_parallel.py:127), for the main channel (a1) and
// the floodplains (a2, if given), and the per-pixel dx (if given), permuted into sweep order and uploaded on stream s
inline int upload_sweep_statics(lf_router_core &r, const std::vector<int32_t> &perm, const double *alpha, const double *alpha_floodplains,
                                const double *dx, hipStream_t s)
{
    const int64_t n = r.N;
    std::vector<double> h(n);
    auto fill = [&](const double *al) {
        for (int64_t p = 0; p < n; ++p) {
            const int32_t pix = perm[p];
            h[p] = al[pix] * (dx ? dx[pix] : r.dx_scalar) / r.dt;
        }
    };
    fill(alpha);
    LF_TRY(r.a1.upload(h.data(), n, s));
    if (alpha_floodplains) {
        fill(alpha_floodplains);
        LF_TRY(r.a2.upload(h.data(), n, s));
    }
    if (dx) {
        for (int64_t p = 0; p < n; ++p) h[p] = dx[perm[p]];
        LF_TRY(r.dx.upload(h.data(), n, s));
    }
    return LF_OK;
}

// What lf_router_create and lf_dist_router_create have in common, in two steps so that a create function keeps the order
// of its device allocations (its own upstream tables go between the two).  First the scalars, the beta = 3/5 switch and,
// on stream s, the sweep statics, perm and ups_ptr.  kmax: the largest in-degree a sweep has to look at.
inline int router_core_init(lf_router_core &r, int device, lf_device_ctx *ctx, int64_t n, int kmax, double beta, double dx_scalar,
                            double dt, const std::vector<int32_t> &perm, const std::vector<int32_t> &ups_ptr, const double *alpha,
                            const double *alpha_floodplains, const double *dx, hipStream_t s)
{
    r.device = device;
    r.ctx = ctx;
    r.N = n;
    r.kmax = kmax;
    r.beta = beta;
    r.inv_beta = 1 / beta;  // kinematic_wave_parallel.py:125
    r.b_minus_1 = beta - 1; // :126
    r.dx_scalar = dx_scalar;
    r.dt = dt;
    r.dx_per_pixel = dx != nullptr;
    r.has_floodplains = alpha_floodplains != nullptr;
    r.fused = router_fused(beta);
    LF_TRY(upload_sweep_statics(r, perm, alpha, alpha_floodplains, dx, s));
    LF_TRY(r.perm.upload(perm.data(), n, s));
    return r.ups_ptr.upload(ups_ptr.data(), n + 1, s);
}

// ... then the levels: level_start on stream s and on the host, and `constant` off the beta = 3/5 path
inline int router_core_init_levels(lf_router_core &r, const std::vector<int64_t> &level_start, hipStream_t s)
{
    const std::vector<long long> ls(level_start.begin(), level_start.end());
    LF_TRY(r.level_start.upload(ls.data(), ls.size(), s));
    if (!r.fused) LF_TRY(r.constant.alloc(r.N));
    r.h_level_start = level_start;
    return LF_OK;
}

// sweep_args of a call on r's section: the new discharge goes to qord (sweep order) and, unless null, to q_pix (pixel
// order); the INDEXED and STATICS fields stay null for the caller
inline sweep_args sweep_args_of(const lf_router_core &r, int section, double *qord, double *q_pix, const double *lat)
{
    sweep_args A;
    A.ups_ptr = r.ups_ptr.p;
    A.ups_idx = nullptr;
    A.ups_base = nullptr;
    A.perm = r.perm.p;
    A.a = (section == LF_SECTION_MAIN) ? r.a1.p : r.a2.p;
    A.constant = r.constant.p;
    A.lat = lat;
    A.dx = r.dx_per_pixel ? r.dx.p : nullptr;
    A.dx_scalar = r.dx_scalar;
    A.beta = r.beta;
    A.inv_beta = r.inv_beta;
    A.b_minus_1 = r.b_minus_1;
    A.kmax = r.kmax;
    A.qord = qord;
    A.q_pix = q_pix;
    A.qold_src = nullptr;
    A.adx = nullptr;
    A.rec24 = nullptr;
    A.upcnt = nullptr;
    A.wave_start = nullptr;
    return A;
}

struct launch_counts {
    int64_t launches = 0, wide = 0, narrow = 0; // every launch; of them, the one-level ones; the cone and narrow-run ones
};

// The launch schedule of a router call.  With level blocks -- use_blocks, the caller's condition,
// and LF_ROUTE_CONES not 0 (read at every call: bench.py switches it for its A/B legs) -- the blocks [b0, b0 + nblocks) of
// r's route plan (r.rplan, its cone table in r.rplan_dev), each one launch:
//   several levels  cones(grid, C, cells): one workgroup per cone of the block;
//   one level       level(first, cells), none for an empty level;
// otherwise the segments `segs`:
//   a wide level    level(first, cells);
//   narrow levels   narrow(k0, k1): one workgroup walks the run.
// The callbacks return an LF_ status; n counts the launches.
template <class Cones, class Level, class Narrow>
int route_schedule(const lf_router_core &r, int b0, int nblocks, const std::vector<level_segment> &segs, bool use_blocks,
                   launch_counts &n, Cones &&cones, Level &&level, Narrow &&narrow)
{
    const char *e = std::getenv("LF_ROUTE_CONES");
    auto cells = [&](int k0, int k1) { return r.h_level_start[k1] - r.h_level_start[k0]; };
    if (use_blocks && !(e && e[0] == '0')) {
        for (int b = b0; b < b0 + nblocks; ++b) {
            const int k0 = r.rplan.level[b], nl = r.rplan.nlevels(b);
            if (nl > 1) {
                cone_plan_args C;
                C.cone = r.rplan_dev.cone.p + r.rplan.off[b];
                C.nl = nl;
                C.n_cells = (int)r.N;
                LF_TRY(cones(dim3((unsigned)r.rplan.ncones(b)), C, cells(k0, k0 + nl)));
                ++n.narrow;
            } else {
                if (cells(k0, k0 + 1) <= 0) continue;
                LF_TRY(level((int)r.h_level_start[k0], (int)cells(k0, k0 + 1)));
                ++n.wide;
            }
            ++n.launches;
        }
        return LF_OK;
    }
    for (const level_segment &g : segs) {
        if (g.wide) {
            LF_TRY(level((int)r.h_level_start[g.k0], (int)cells(g.k0, g.k1)));
            ++n.wide;
        } else {
            LF_TRY(narrow(g.k0, g.k1));
            ++n.narrow;
        }
        ++n.launches;
    }
    return LF_OK;
}

} // namespace
