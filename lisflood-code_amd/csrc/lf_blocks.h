// lf_blocks.h -- host side: level blocks and their cones for the LDS sweeps (k_sweep_cones, k_fused_cones), shared by the
// single-domain router (lf_router.hip) and the row-block partition (lf_dist.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <vector>

#include "lf_common.h"

// Workgroups go to the eight XCDs round robin by their linear id.  Neighbouring cones of a block share the 128-byte lines
// their level segments begin and end in (a segment of 64 cells = 4 lines + on average one shared): with the cones of a
// (block, sub-step) dealt out in launch order the two halves of such a line are fetched into two L2s.  This gives the
// workgroups of one XCD CONSECUTIVE cones of the range [0, n) instead: i = position in launch order, linear_id = of this
// workgroup (so position 0 has linear id linear_id - i); a bijection of [0, n), positions beyond n map to themselves.
// Device code (k_fused_cones) and host (lf_xcd_contiguous_order: the tests look at the whole order).
__host__ __device__ inline int lf_xcd_contiguous(int i, int n, unsigned linear_id)
{
    if (i >= n) return i;
    const unsigned start = linear_id - (unsigned)i; // linear id of position 0
    const int cls = (int)(linear_id & 7u);
    int before = 0, r_mine = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int r = (int)(((unsigned)c - start) & 7u); // first position of class c
        const int cnt = r < n ? (n - r + 7) >> 3 : 0;
        before += c < cls ? cnt : 0;
        r_mine = c == cls ? r : r_mine;
    }
    return before + ((i - r_mine) >> 3);
}

// The ensemble launches whose unit of work is (tile of 256 columns or pixels, member) -- the land surface (lf_soil.hip) and
// the element-wise member kernels (lf_modules.hip) -- order their units tile-major, u = tile * members + member, and deal
// them to the workgroups with lf_xcd_contiguous: the members of a tile run next to each other on one XCD.
// -> (tile, member) of the workgroup at `position` of the launch whose linear id is `linear_id`
#ifndef LF_LAND_MEMBERS_XCD
#define LF_LAND_MEMBERS_XCD 1
#endif
__host__ __device__ inline void land_members_unit(unsigned int units, unsigned int members, unsigned int position,
                                                  unsigned int linear_id, unsigned int &tile, unsigned int &member)
{
    const unsigned int u = LF_LAND_MEMBERS_XCD ? (unsigned int)lf_xcd_contiguous((int)position, (int)units, linear_id) : position;
    tile = u / members;
    member = u - tile * members;
}

// Runs of consecutive levels [k_lo, k_hi) of at most `wide` cells are cut into blocks of up to lmax levels; a wider level
// is a block of its own.  A block is cut into CONES: chunks of its last level, as long as possible with no level of the
// cone wider than `max_cone` cells, each with the range of every earlier level that drains into it (`child(pos)` = first
// position of the level before whose downstream cell is at or behind `pos`; the ranges tile every level of the block).
// A block whose thinnest possible cone (one cell of the last level) is still too wide somewhere loses levels until it
// fits (one level always does).
//   level[b]      first level of block b (absolute), level[B] = k_hi once closed
//   row[b]        first cone row of block b; block b has row[b+1] - row[b] - 1 cones and one closing row
//   off[b]        first entry of block b in `cone`; a row holds one start per level of the block
//   part[i]       first block of phase / stage i of the partition, which builds one plan from several level ranges
//                 (part[n] = B once closed); empty for the single domain
// A plan is built by lf_build_level_blocks, once per level range, and then closed (close / finish).  The empty plan is
// "no plan": its owner sweeps level by level.
struct lf_block_plan {
    std::vector<int> level, row, off, cone, part;
    std::vector<int> lvl2blk; // block of every level (index_levels: the single domain's structure sites)
    int lmax = 0, cw = 0;     // levels per block and cells per level of a cone the plan was built with
    bool any_multi = false;   // some block holds more than one level

    bool empty() const { return level.empty(); }
    int nblocks() const { return empty() ? 0 : (int)level.size() - 1; }
    int nlevels(int b) const { return level[b + 1] - level[b]; }
    int ncones(int b) const { return row[b + 1] - row[b] - 1; }
    bool multi(int b) const { return nlevels(b) > 1; }
    void begin_part() { part.push_back((int)level.size()); } // before the level range of every phase / stage
    // the closing level and, for a plan in parts, the closing part entry
    void close(int64_t k_hi)
    {
        if (!part.empty()) part.push_back((int)level.size());
        level.push_back((int)k_hi);
    }
    // close; a plan with nothing to gain (no block of several levels) or a cone table beyond 32-bit offsets is dropped
    void finish(int64_t k_hi)
    {
        close(k_hi);
        if (!any_multi || cone.size() >= ((size_t)1 << 31)) *this = lf_block_plan();
    }
    void index_levels()
    {
        lvl2blk.assign((size_t)level.back(), 0);
        for (int b = 0; b < nblocks(); ++b)
            for (int k = level[b]; k < level[b + 1]; ++k) lvl2blk[k] = b;
    }
    // how full the cone wavefronts are: out = {blocks, blocks of several levels, their cones, cone rows (cones x levels),
    // their cells, most cones in one block}
    void stats(const std::vector<int64_t> &level_start, int64_t out[6]) const
    {
        for (int i = 0; i < 6; ++i) out[i] = 0;
        out[0] = nblocks();
        for (int b = 0; b < nblocks(); ++b) {
            if (!multi(b)) continue;
            const int64_t cones = ncones(b);
            out[1] += 1;
            out[2] += cones;
            out[3] += cones * nlevels(b);
            out[4] += level_start[level[b + 1]] - level_start[level[b]];
            out[5] = std::max(out[5], cones);
        }
    }
};

// Levels per block and the width above which a level is a block of its own: LF_ROUTE_LEVELS (plain router calls) or
// LF_FUSED_LEVELS (fused wavefront) replaces `lmax`, the caller's default for its graph, and lmax_override (> 0: the
// tuner of the single domain) replaces both; clamped to 1..512 / 1..64.  LF_FUSED_WIDE replaces the 262144 cells.
struct lf_block_knobs {
    int lmax;
    int64_t wide;
};
inline lf_block_knobs lf_read_block_knobs(bool for_route, int lmax, int lmax_override = 0)
{
    if (const char *e = for_route ? std::getenv("LF_ROUTE_LEVELS") : std::getenv("LF_FUSED_LEVELS")) lmax = std::atoi(e);
    if (lmax_override > 0) lmax = lmax_override;
    lf_block_knobs k{std::min(std::max(lmax, 1), for_route ? 512 : 64), 262144};
    if (const char *e = std::getenv("LF_FUSED_WIDE")) k.wide = std::atoll(e);
    return k;
}

// build(): calls of lf_build_level_blocks and what they need; running out of host memory there is an LF_ error
template <class BUILD>
inline int lf_build_blocks_guarded(BUILD &&build)
{
    try {
        build();
    } catch (const std::bad_alloc &) {
        return lf_set_error(LF_E_INVALID, "out of host memory while building the level blocks");
    }
    return LF_OK;
}

// The device side of a plan: always the cone table (all that k_sweep_cones takes: cone_plan_args); with `tables` also
// level / row / off (the fused kernels find their block themselves: fused_args::fb_*); lvl2blk where the plan has it.
struct lf_block_plan_dev {
    lf_dbuf<int> level, row, off, cone, lvl2blk;
    int upload(const lf_block_plan &p, bool tables, hipStream_t stream = nullptr)
    {
        if (tables) {
            LF_TRY(level.upload(p.level.data(), p.level.size(), stream));
            LF_TRY(row.upload(p.row.data(), p.row.size(), stream));
            LF_TRY(off.upload(p.off.data(), p.off.size(), stream));
        }
        LF_TRY(cone.upload(p.cone.data(), p.cone.size(), stream));
        return tables ? lvl2blk.upload(p.lvl2blk.data(), p.lvl2blk.size(), stream) : LF_OK;
    }
};

// Appends the blocks of the levels [k_lo, k_hi) to `out`.
template <class CHILD>
inline void lf_build_level_blocks(const std::vector<int64_t> &ls, int64_t k_lo, int64_t k_hi, int lmax, int64_t wide,
                                  int max_cone, CHILD child, lf_block_plan &out)
{
    auto width = [&](int64_t k) { return ls[k + 1] - ls[k]; };
    if (out.row.empty()) out.row.push_back(0);
    out.lmax = lmax;
    out.cw = max_cone;
    std::vector<int64_t> st((size_t)std::max(lmax, 1)), en((size_t)std::max(lmax, 1));
    // starts of the cone above last-level position `pos` of the block [k0, k0 + nl): st[nl-1] = pos, st[j] = first
    // position of level j draining at or behind st[j+1] (the end of level j when st[j+1] is the end of level j+1, the
    // start of level j when it is the start)
    auto chain = [&](int64_t k0, int nl, int64_t pos, std::vector<int64_t> &o) {
        o[nl - 1] = pos;
        for (int j = nl - 2; j >= 0; --j) {
            if (pos >= ls[k0 + j + 2])
                pos = ls[k0 + j + 1];
            else if (pos <= ls[k0 + j + 1])
                pos = ls[k0 + j];
            else
                pos = child(pos);
            o[j] = pos;
        }
    };
    for (int64_t k = k_lo; k < k_hi;) {
        int nl = 1;
        if (width(k) <= wide)
            while (k + nl < k_hi && nl < lmax && width(k + nl) <= wide) ++nl;
        std::vector<int> rows; // starts, nl per cone, then the closing row
        for (;; --nl) {        // shrink until every cone fits a workgroup
            rows.clear();
            const int64_t lo = ls[k + nl - 1], hi = ls[k + nl];
            bool fits = true;
            for (int64_t a = lo; a < hi && fits;) {
                chain(k, nl, a, st);
                auto ok = [&](int64_t e) { // cone [a, e) of the last level: every level's range <= max_cone?
                    chain(k, nl, e, en);
                    for (int j = 0; j < nl; ++j)
                        if (en[j] - st[j] > max_cone) return false;
                    return true;
                };
                int64_t e = std::min<int64_t>(a + max_cone, hi);
                if (!ok(e)) { // largest e in (a, a + max_cone) that fits: the widths grow with e
                    int64_t good = a, bad = e;
                    while (bad - good > 1) {
                        const int64_t mid = good + (bad - good) / 2;
                        if (ok(mid)) good = mid; else bad = mid;
                    }
                    e = good;
                }
                if (e == a) { // even one cell of the last level has too wide a cone
                    fits = false;
                    break;
                }
                for (int j = 0; j < nl; ++j) rows.push_back((int)st[j]);
                a = e;
            }
            if (fits || nl == 1) break;
        }
        for (int j = 0; j < nl; ++j) rows.push_back((int)ls[k + j + 1]); // closing row: the end of every level
        out.level.push_back((int)k);
        out.off.push_back((int)out.cone.size());
        out.row.push_back(out.row.back() + (int)(rows.size() / nl));
        out.cone.insert(out.cone.end(), rows.begin(), rows.end());
        out.any_multi = out.any_multi || nl > 1;
        k += nl;
    }
}
