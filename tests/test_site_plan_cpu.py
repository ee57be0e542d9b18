"""The site plan of the time-major fused form with lakes and reservoirs in the loop (lf_site_plan, include/lisflood_amd.h):
a pure host function over the level table and the six site lists, run here through the C ABI on graphs built with
Graph(cut, mask, virtual_down=...) and checked against a numpy restatement -- feed slots that are the inverse of the two
feeder lists, the sites of every level, and whether the form applies (no chained sites, no shared cell, no cell feeding
two sites).  No device is needed."""
import ctypes as C

import numpy as np
import pytest

import module_edges as E
from lisflood_amd import _lib, synthetic as syn
from lisflood_amd.kinematic_wave_parallel import Graph


def _site_lists(cut, mask, downstruct, lake, res):
    """-> (Graph with the sites' links, level_start, the six site lists in engine positions as routing.attach_structures
    builds them: feeders grouped by site, ascending pixel id)"""
    N = int(np.asarray(mask).sum())
    ds = np.asarray(downstruct).astype(np.int64)
    site = np.zeros(N + 1, bool)
    site[lake] = True
    site[res] = True
    dsc = np.minimum(ds, N)
    vd = np.where(site[dsc] & (dsc < N), dsc, -1)
    g = Graph(cut, mask, virtual_down=vd)
    perm, _, level_start = g.layout()
    pos = np.empty(N, np.int64)
    pos[perm.astype(np.int64)] = np.arange(N)
    order = np.argsort(ds, kind="stable")
    starts = np.searchsorted(ds[order], np.arange(N + 1))

    def csr(cells):
        ptr = np.zeros(len(cells) + 1, np.int32)
        idx = [order[starts[c]:starts[c + 1]] for c in cells]
        ptr[1:] = np.cumsum([u.size for u in idx])
        idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
        return ptr, pos[idx].astype(np.int32)
    lake_ptr, lake_idx = csr(lake)
    res_ptr, res_idx = csr(res)
    return g, level_start, (pos[lake].astype(np.int32), lake_ptr, lake_idx, pos[res].astype(np.int32), res_ptr, res_idx)


def _plan(N, level_start, lists):
    lake_cell, lake_ptr, lake_idx, res_cell, res_ptr, res_idx = [np.ascontiguousarray(x, np.int32) for x in lists]
    nl = level_start.size - 1
    applies = C.c_int32(-1)
    slot = np.full(N, -7, np.int32)
    ptr = np.full(nl + 1, -7, np.int32)
    sites = np.full(lake_cell.size + res_cell.size, -7, np.int32)
    pad = lambda a: a if a.size else np.zeros(1, np.int32)
    rc = _lib.lib().lf_site_plan(N, nl, _lib.ptr(np.ascontiguousarray(level_start, np.int64)), lake_cell.size,
                                 _lib.ptr(pad(lake_cell)), _lib.ptr(lake_ptr), _lib.ptr(pad(lake_idx)), res_cell.size,
                                 _lib.ptr(pad(res_cell)), _lib.ptr(res_ptr), _lib.ptr(pad(res_idx)), C.byref(applies),
                                 _lib.ptr(slot), _lib.ptr(ptr), _lib.ptr(pad(sites)))
    return rc, applies.value, slot, ptr, sites


def _level_of(level_start, p):
    return np.searchsorted(level_start, p, side="right") - 1


def _loop_case(family):
    r, s, cut, mask = E.loop_inputs(family)
    return _site_lists(cut, mask, s["downstruct"], s["LakeIndex"], s["ReservoirIndex"])


def _chained_case():
    H, W = 60, 80
    codes = syn.make_ldd("shallow", H, W, 8).reshape(-1).astype(np.float64)
    p = syn.router_params(H * W, seed=4)
    d, cut = syn.structures_scenario(codes, (H, W), p["Q0"], 3600.0, n_lakes=40, n_res=60)
    return _site_lists(cut, np.ones((H, W), bool), d["downstruct"], d["LakeIndex"], d["ReservoirIndex"])


@pytest.mark.parametrize("family", ["shallow", "deep"])
def test_plan_of_the_loop_inputs(family):
    """module_edges.loop_inputs: 130 lakes + 190 reservoirs, no site just downstream of another.  shallow: 8 levels, 4 of
    them wider than 256 cells, sites on 4 of them (up to 240 on one), 1 to 5 feeders per site; deep: 118 levels, 110 with
    sites.  The plan applies, the slots invert the two feeder lists (lakes first, list order) and the per-level site lists
    partition the sites by the level of their cell."""
    g, level_start, lists = _loop_case(family)
    lake_cell, lake_ptr, lake_idx, res_cell, res_ptr, res_idx = lists
    N, nl = g.num_pixels, g.num_levels
    widths = np.diff(level_start)
    cells = np.concatenate([lake_cell, res_cell])
    lv = _level_of(level_start, cells)
    per_level = np.bincount(lv, minlength=nl)
    nfeed = np.concatenate([np.diff(lake_ptr), np.diff(res_ptr)])
    if family == "shallow":
        assert nl == 8 and (widths > 256).sum() == 4 and (per_level > 0).sum() == 4 and per_level.max() == 240
        assert nfeed.min() == 1 and nfeed.max() == 5
    else:
        assert nl == 118 and (per_level > 0).sum() == 110
        assert nfeed.min() == 1 and nfeed.max() > 1
    rc, applies, slot, ptr, sites = _plan(N, level_start, lists)
    assert rc == 0 and applies == 1
    # the slots: the inverse of the two feeder lists, numbered in list order, lakes first
    feeders = np.concatenate([lake_idx, res_idx])
    assert np.unique(feeders).size == feeders.size
    want = np.full(N, -1, np.int32)
    want[feeders] = np.arange(feeders.size)
    assert np.array_equal(slot, want)
    assert np.array_equal(slot[lake_idx], np.arange(lake_idx.size))
    assert np.array_equal(slot[res_idx], lake_idx.size + np.arange(res_idx.size))
    assert g.links()[feeders].all()                       # every feeder is a link of the graph, on its site's level
    # the sites of every level: a partition of all sites by the level of their cell, ascending inside a level
    assert ptr[0] == 0 and ptr[-1] == cells.size and np.array_equal(np.diff(ptr), per_level)
    assert np.array_equal(np.sort(sites), np.arange(cells.size))
    for k in range(nl):
        here = sites[ptr[k]:ptr[k + 1]]
        assert np.array_equal(here, np.nonzero(lv == k)[0])
    g.close()


def test_chained_sites_do_not_apply():
    """structures_scenario on make_ldd("shallow", 60, 80, 8) with 40 lakes + 60 reservoirs draws its sites without looking
    at their neighbours: 6 levels, and 6 site cells drain straight into another site.  The plan says so; the fused call
    then keeps the skewed wavefront."""
    g, level_start, lists = _chained_case()
    lake_cell, lake_ptr, lake_idx, res_cell, res_ptr, res_idx = lists
    cells, feeders = np.concatenate([lake_cell, res_cell]), np.concatenate([lake_idx, res_idx])
    assert g.num_levels == 6 and np.isin(cells, feeders).sum() == 6
    rc, applies, _, _, _ = _plan(g.num_pixels, level_start, lists)
    assert rc == 0 and applies == 0
    g.close()


def test_shared_cell_and_double_feeder_do_not_apply():
    level_start = np.array([0, 4, 8], np.int64)
    one = np.array([0, 1], np.int32)
    # a lake and a reservoir on the same cell
    rc, applies, *_ = _plan(8, level_start, (np.array([5]), one, np.array([6]), np.array([5]), one, np.array([7])))
    assert rc == 0 and applies == 0
    # a cell listed as feeder of two sites
    rc, applies, *_ = _plan(8, level_start, (np.array([4]), one, np.array([6]), np.array([5]), one, np.array([6])))
    assert rc == 0 and applies == 0
    # the same lists apart: applies, reservoirs numbered behind the lakes
    rc, applies, slot, ptr, sites = _plan(8, level_start, (np.array([4]), one, np.array([6]), np.array([5]), one, np.array([7])))
    assert rc == 0 and applies == 1
    assert slot.tolist() == [-1, -1, -1, -1, -1, -1, 0, 1] and ptr.tolist() == [0, 0, 2] and sites.tolist() == [0, 1]
    # no site at all: nothing to plan, applies
    none = np.zeros(0, np.int32)
    rc, applies, slot, ptr, _ = _plan(8, level_start, (none, np.zeros(1, np.int32), none, none, np.zeros(1, np.int32), none))
    assert rc == 0 and applies == 1 and (slot == -1).all() and (ptr == 0).all()


def test_feeder_off_its_level_is_no_error():
    """levels [0, 4) and [4, 8), one lake on cell 5: a feeder on the other level (cell 2) is a plan that does not apply
    -- rc 0, not an error: refusing such lists is the fused call's business, not the plan's --, a feeder on the lake's
    own level (cell 6) one that does"""
    level_start = np.array([0, 4, 8], np.int64)
    one, none = np.array([0, 1], np.int32), np.zeros(0, np.int32)
    for feeder, want in ((2, 0), (6, 1)):
        rc, applies, *_ = _plan(8, level_start, (np.array([5]), one, np.array([feeder]), none, np.zeros(1, np.int32), none))
        assert rc == 0 and applies == want, feeder


@pytest.mark.parametrize("bad", ["site cell", "negative site cell", "feeder", "pointer"])
def test_out_of_range_is_refused(bad):
    """a cell or a pointer out of range is an error with a message, not a crash and not a plan"""
    g, level_start, lists = _loop_case("shallow")
    lists = [np.array(x, copy=True) for x in lists]
    N = g.num_pixels
    if bad == "site cell":
        lists[3][7] = N
    elif bad == "negative site cell":
        lists[0][0] = -1
    elif bad == "feeder":
        lists[2][-1] = N + 5
    else:
        lists[1][3] = lists[1][2] - 1
    rc, *_ = _plan(N, level_start, lists)
    assert rc == _lib.LF_E_INVALID
    assert b"site plan" in _lib.lib().lf_last_error()
    g.close()
