"""The inputs of tests/test_ldd_edges_gpu.py are what tests/ldd_edges.py says they are, shown without a GPU: the restated
accuflux lies within the derived bound of recursive summation of math.fsum over every cell's upstream tree and the exact
ordered-sum claims hold in it; the engine's layout has the two properties the restatement relies on; the host helpers of
lisflood_amd.ldd equal the restatements; every (configuration, NV) a GPU case names has the chunk shapes, in-degrees and
NaN levels it claims in the schedule worked out from the layout; the point deals put the lane mix of k_jump_init into one
wavefront; and the rasters of the element-wise and tile kernels hold every plant.  No case here or on the GPU is skipped
for lack of a suitable cell: what a graph cannot supply is not asked of it, and that is asserted here."""
import numpy as np
import pytest

import ldd_edges as D
import route_edges as E

FINITE = ("random", "random_b", "ordered")


# ---- the restatement against the exact reference ---------------------------------------------------------------------
@pytest.mark.parametrize("name", E.GRAPHS + ["chains_half"])
def test_restated_accuflux_lies_within_the_summation_bound_of_fsum(name):
    """|restated - fsum| <= gamma(n - 1) sum|x| over the tree of n cells, gamma(k) = k u / (1 - k u), u = 2^-53: the bound of n - 1
    additions in any order (a cell with j upstream cells adds j times: the first term joins 0.0 exactly), no factor added"""
    g = D.graph(name)
    for kind in FINITE + ("signed_zero",):
        x = D.deal(name, kind)["x"]
        with np.errstate(all="ignore"):
            got = D.restated(name, "accuflux", kind)
            total, err, mass, size = D.exact_accuflux(g, x, got)
            finite = np.isfinite(mass)
            assert finite.all() or kind == "signed_zero"
            bound = np.array([D.gamma(int(n) - 1) for n in size]) * mass
        assert (err[finite] <= bound[finite]).all(), (name, kind, np.flatnonzero(finite & ~(err <= bound))[:5])
        assert size.max() >= 3 and (err[finite] > 0).any() or name.startswith("chains") or kind == "signed_zero"
        # a cell nothing drains into returns 0.0 + x: its own value, but never a negative zero
        src = g["indeg"] == 0
        assert E.bits_equal(got[src], np.where(x[src] == 0, 0.0, x[src])).all()


@pytest.mark.parametrize("name", E.GRAPHS)
def test_the_exact_ordered_sum_claims_hold_in_the_restatement(name):
    g, d = D.graph(name), D.deal(name, "ordered")
    got = D.restated(name, "accuflux", "ordered")
    kmax = int(name[3:]) if name.startswith("fan") else 8
    seen = {}
    for centre, ups, what in d["fans"]:
        k = len(ups)
        seen.setdefault(what, set()).add(k)
        vals = [D.BIG] + [1.0] * (k - 1)
        assert np.array_equal(got[ups], vals[::-1] if what == "mirror" else vals)
        if what == "asc":
            assert got[centre] == D.BIG
        elif what == "mirror":
            e = k - 1                                            # 2^53 + (k - 1), rounded to even: the spacing there is 2
            assert got[centre] == D.BIG + (e if e % 2 == 0 else (e + 1 if (e + 1) % 4 == 0 else e - 1))
            assert (got[centre] != D.BIG) == (k >= 3)            # from three terms on the other order gives other bits
        else:
            assert got[centre] == D.BIG + 2.0                    # upstream first, the cell last
            other = 2.0
            for v in vals:
                other = other + v
            assert (other != got[centre]) == (k >= 2) and (k < 2 or other == D.BIG + 4.0)   # a sum started from x
    # every kind at every in-degree a confluence of the graph can have (`many` has no one-star trees: a top star has 1..7)
    degs = set(range(1, (min(kmax, 7) if name == "many" else kmax) + 1))
    for what in D.ORDERED:
        assert seen[what] >= degs, (name, what, sorted(seen[what]))


@pytest.mark.parametrize("name", E.GRAPHS)
def test_signed_zeros_and_infinities_do_what_the_restatement_says(name):
    g, d = D.graph(name), D.deal(name, "signed_zero")
    x, got = d["x"], D.restated(name, "accuflux", "signed_zero")
    down = E.topology(g)[0]
    kinds = {}
    for what, cell in d["plants"]:
        kinds.setdefault(what, []).append(cell)
    plus_zero = lambda v: (np.ascontiguousarray(v).view(np.uint64) == 0).all()
    assert len(kinds["negzero_pit"]) >= 8 and np.signbit(x[kinds["negzero_pit"]]).all() and plus_zero(got[kinds["negzero_pit"]])
    if name != "many":                                            # (no one-star trees there)
        assert len(kinds["negzero_star"]) >= 2
        for what in ("negzero_star", "negzero_source"):
            assert np.signbit(x[kinds[what]]).all() and plus_zero(got[kinds[what]])
    # downstream copies the bits: the sources of a -0.0 star read -0.0, and so does the pit itself
    ds = D.restated_downstream(g, x)
    cells = kinds["negzero_pit"] + kinds.get("negzero_source", [])
    assert (ds[cells] == 0).all() and np.signbit(ds[cells]).all()
    # +inf and -inf on two sources of one confluence: NaN there and on its whole path downstream, nowhere else
    want = np.zeros(g["N"], bool)
    assert len(kinds.get("inf_confluence", [])) >= (name != "fan1")      # (fan1 has no cell with two upstream cells)
    for c in kinds.get("inf_confluence", []):
        while c >= 0:
            want[c] = True
            c = down[c]
    assert np.array_equal(np.isnan(got), want)
    if name != "fan1":
        assert want.sum() > len(kinds["inf_confluence"])          # a top star: cells below it


# ---- what the restatement relies on in the layout --------------------------------------------------------------------
@pytest.mark.parametrize("name", E.GRAPHS + list(D.CHAINS))
def test_upstream_ranges_are_ascending_pixel_ids_one_level_above(name):
    g = D.graph(name)
    perm, ups_ptr, ls, _ = E.layout_of(name)
    down, ups, dist = E.topology(g)
    lvl = E.level_of(ls, np.arange(perm.size))
    for p in range(perm.size):
        rng = np.arange(ups_ptr[p], ups_ptr[p + 1])
        assert np.array_equal(perm[rng], ups[perm[p]]), p         # the upstream cells, in ascending pixel id
        assert (lvl[rng] == lvl[p] - 1).all(), p                  # exactly one level above
    assert np.array_equal(lvl, (len(ls) - 2) - dist[perm])


def test_structure_links_sit_inside_upstream_ranges_and_send_nothing():
    g = D.linked_graph()
    perm, ups_ptr, ls, _ = g["layout"]
    linked, down = g["linked"], g["down"]
    assert g["structures"] >= 3 and linked.sum() == 2 * g["structures"] == (g["vd"] >= 0).sum()
    inside = 0
    for p in range(perm.size):
        rng = np.arange(ups_ptr[p], ups_ptr[p + 1])
        inside += int(linked[rng].sum())
        assert np.array_equal(perm[rng[~linked[rng]]], g["ups"][perm[p]]), p
    assert inside >= 1                                            # k_upstream_sum meets links in its ranges
    assert (down[g["vd"] >= 0] < 0).all()


# ---- the host helpers against the restatements ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.CHAINS) + ["main_shallow_masked", "fan8"])
def test_host_walks_equal_the_restatements(name):
    from lisflood_amd import ldd as L
    g = D.graph(name)
    codes, mask = g["codes"][g["mask"]].astype(np.float64), g["mask"]
    assert np.array_equal(L.downstream_index(codes, mask), E.topology(g)[0])
    assert np.array_equal(L.pit(codes), D.restated_pit(codes))
    x = D.deal(name, "signed_zero")["x"].copy()
    x[D.spots(3, g["N"])] = np.nan
    assert E.bits_equal(L.downstream(codes, mask, x), D.restated_downstream(g, x)).all()
    for kind in (D.POINT_DEALS if name in D.CHAINS else ()) + ("scatter",):
        pts = D.points(name, kind)
        assert np.array_equal(L.subcatchment(codes, mask, pts), D.restated_subcatchment(g, pts)), kind
        assert np.array_equal(L.catchment(codes, mask, pts), D.restated_catchment(g, pts)), kind


@pytest.mark.parametrize("shape", D.REPAIR_SHAPES)
def test_host_lddrepair_and_lddmask_equal_the_restatements(shape):
    """the host forms work on compressed vectors: a land pixel with an unknown code stays in the vector, as a pit after
    lddrepair and as it was after lddmask; everything else is the raster restatement's"""
    from lisflood_amd import ldd as L
    mask = np.ones(shape, bool)
    for r, keep in D.repair_rasters(shape):
        want = D.restated_lddrepair(r).reshape(-1)
        got = L.lddrepair(r.reshape(-1).astype(np.float64), mask)
        assert np.array_equal(got, np.where(want == 0, 5, want)), (shape, r)
        k = keep.reshape(-1) != 0
        want = D.restated_lddmask(r, keep).reshape(-1)
        got, sub = L.lddmask(r.reshape(-1).astype(np.float64), mask, k)
        assert np.array_equal(np.where(np.isin(got, range(1, 10)), got, 0), want[k]) and np.array_equal(sub.reshape(-1), k), (shape, r)


@pytest.mark.parametrize("shape", D.REPAIR_SHAPES)
def test_repair_rasters_hold_every_plant(shape):
    ras = D.repair_rasters(shape)
    cen = D.repair_census(ras)
    if shape == (1, 1):
        assert sorted(int(r[0, 0]) for r, _ in ras) == list(range(11)) + [255] and cen["into"]["off"] == 8
        return
    assert cen["corners"] >= {(a, b, k) for a in (False, True) for b in (False, True) for k in range(1, 10)
                              if (shape[0] > 1 or not a) and (shape[1] > 1 or not b)}
    for t in (0, 10, 255, 5, "off", "flows"):
        assert cen["into"].get(t, 0) >= (1 if shape[0] * shape[1] == 9 else 2), (shape, t, cen["into"])
    if shape[0] * shape[1] >= 255:
        assert cen["kept_pits"] >= 1 and all(cen["pairs"].get((a, b), 0) >= 1 for a in (False, True) for b in (False, True)), cen["pairs"]
    # the restatements differ from their input and from each other: the plants bite
    assert any((D.restated_lddrepair(r) != D.restated_lddmask(r, k)).any() for r, k in ras)


@pytest.mark.parametrize("shape", D.UPSTREAM_SHAPES)
def test_upstream_rasters_hold_every_plant(shape):
    H, W = shape
    for variant in D.VARIANTS:
        ldd, w, centres = D.upstream_raster(shape, variant)
        want = D.restated_upstream_raster(ldd, w)
        assert not np.isnan(want).any() and np.isnan(w).sum() >= (H * W >= 63)      # NaN weights reach nobody
        for r, c, k in centres:
            n = sum(1 for dr, dc, _ in E.NBRS if 0 <= r + dr < H and 0 <= c + dc < W)
            assert k == n
            if variant.startswith("asc"):
                assert want[r, c] == (D.BIG if k else 0.0)
            elif variant.startswith("mirror"):
                assert want[r, c] == ((float(k - 1) + D.BIG) if k else 0.0)
            elif k == 8:
                assert want[r, c] == 5.0
        assert (0, 0) in [x[:2] for x in centres] and any(max(H - 1 - x[0], W - 1 - x[1]) <= 2 for x in centres)
        seam, off = D.upstream_raster_census(ldd)
        if H > D.TILE_H and W > D.TILE_W:
            at = (D.TILE_H - 1, D.TILE_W - 1) if variant.startswith("mirror") else (D.TILE_H, D.TILE_W)
            assert at in [x[:2] for x in centres]
            assert seam == set(E._SHIFT)                         # every direction across a tile seam
        if H > D.TILE_H + 1 and W > D.TILE_W + 1:
            assert (at + (8,)) in centres                        # in-degree 8, its sources in four tiles
        if H >= 15 and W >= 63:                                  # off each edge, in every direction on the largest raster
            full = dict(N={7, 8, 9}, S={1, 2, 3}, W={1, 4, 7}, E={3, 6, 9})
            assert all(off[e] <= full[e] and len(off[e]) >= 2 for e in full) and (off == full or (H, W) != (33, 129)), off


# ---- the schedule every GPU case names -------------------------------------------------------------------------------
def test_every_configuration_and_nv_has_the_chunk_shapes_and_nan_levels_it_claims():
    """on the 87 levels of main_deep and its masked variant: blocks of exactly one full chunk, of a full chunk and a ragged
    one of one level, and of several chunks, for every NV at both cone widths; the NaN levels on all three inflow paths"""
    have = {}
    for name in D.DEEP:
        ls = E.layout_of(name)[2]
        assert len(ls) - 1 == 87
        for config, cfg in D.CONFIGS.items():
            for nv in D.NVS:
                shapes = D.chunk_shapes(name, config, nv)
                for s in D.claimed_shapes(config, nv):
                    assert shapes[s] >= 1, (name, config, nv, s, shapes)
                    have.setdefault((cfg["cw"], nv), set()).add(s)
                if "plus1" in D.claimed_shapes(config, nv):
                    assert shapes["ragged1"] >= 1
                paths = D.nan_levels(name, config, nv)
                if cfg["lmax"] == 0:
                    assert paths == {}
                    continue
                lc = D.LC[cfg["cw"]][nv]
                want = {"mid"} | ({"chunk"} if min(cfg["lmax"], 87) > lc else set()) | ({"block"} if cfg["lmax"] < 87 else set())
                # (LF_FUSED_WIDE=100 cuts the blocks at the levels above 100 cells, wherever those are)
                assert set(paths) == want or (config == "wide100" and "mid" in paths), (name, config, nv, paths)
                b = D.blocks(name, config)
                for path, k in paths.items():                     # the level after k is where the case says it is
                    k0, nl = [(k0, nl) for k0, nl in b if k0 <= k + 1 < k0 + nl][0]
                    j = k + 1 - k0
                    assert nl > 1 and (j == 0, j > 0 and j % lc == 0) == (path == "block", path == "chunk"), (name, config, nv, path, k)
                    assert 0 <= k < 86 and ls[k + 1] > ls[k]
                    have.setdefault((cfg["cw"], nv, "nan"), set()).add(path)
    for cw in (64, 256):
        for nv in D.NVS:
            assert have[cw, nv] == {"eq", "plus1", "gt"} and have[cw, nv, "nan"] == {"mid", "chunk", "block"}, (cw, nv, have)


@pytest.mark.parametrize("name", D.CONE_GRAPHS)
def test_the_plans_are_the_schedules_worked_out_from_the_layout(name):
    """lf_graph_block_plan_stats (host only) builds the plan a router would: as many blocks, and as many of several levels,
    as route_edges.regions counts; every in-degree 1..8 inside a block and 0..7 on a block's first level"""
    import ctypes as C
    from lisflood_amd import _lib
    from lisflood_amd.kinematic_wave_parallel import Graph
    g = E.graph(name)
    G = Graph(ldd_raster=g["codes"], land_mask=None if g["mask"].all() else g["mask"])
    k = int(name[3:]) if name.startswith("fan") else 8
    inside, top = {}, {}
    for config, cfg in D.CONFIGS.items():
        if cfg["lmax"] == 0:
            continue
        st = (C.c_int64 * 6)()
        _lib.check(_lib.lib().lf_graph_block_plan_stats(G._h, cfg["lmax"], cfg["wide"], cfg["cw"], st))
        b = D.blocks(name, config)
        assert (st[0], st[1]) == (len(b), sum(nl > 1 for _, nl in b)), (name, config, list(st))
        assert D.launches(name, config)[0] == (len(b) if st[1] else D.launches(name, "segments")[0])
        i, t = D.indegree_census(name, config)
        if config == "wide100":                                   # (its blocks end where a level is wider than 100 cells)
            continue
        assert set(i) >= set(range(1, (k if cfg["lmax"] >= 26 else min(k, 7)) + 1)), (name, config, i)
        for j, n in i.items():
            inside[j] = inside.get(j, 0) + n
        for j, n in t.items():
            top[j] = top.get(j, 0) + n
    G.close()
    assert set(inside) >= set(range(1, k + 1))
    if name != "many":
        assert set(top) >= set(range(0, min(k, 7) + 1)), (name, top)
    # one launch per level: k_accu_level on the levels above 1024 cells (not on the fans), k_accu_narrow on the others
    total, wide = D.launches(name, "segments")
    assert (wide >= 1) == (not name.startswith("fan")) and (total > wide or name == "many")


@pytest.mark.parametrize("name", D.CONE_GRAPHS)
def test_every_deal_has_its_plants_in_the_regions(name):
    """the census of every deal: planted kind -> launch region -> cells.  Ordered sums lie inside blocks in every block
    configuration and on first levels under the short blocks; the NaN of every named level is the first cell of its level"""
    perm, _, ls, _ = E.layout_of(name)
    for kind in ("ordered", "signed_zero"):
        d = D.deal(name, kind)
        rarest = {}
        for config, cfg in D.CONFIGS.items():
            cen = D.deal_census(name, d, config)
            for what, by_region in cen.items():
                for r, n in by_region.items():
                    rarest[what, r] = min(rarest.get((what, r), n), n)
            if kind == "ordered" and cfg["lmax"] >= 2 and config != "wide100":
                assert min(cen[w].get("inside", 0) for w in D.ORDERED) >= 2, (name, config, cen)
        print(name, kind, {"%s/%s" % k: v for k, v in sorted(rarest.items())})
    tops = sum(D.deal_census(name, D.deal(name, "ordered"), c)[w].get("top", 0) for c in ("levels4", "levels7", "cones256_levels4") for w in D.ORDERED)
    assert tops >= 1 or name == "many", name                      # (many: the top stars' centres lie on level 1)
    for config in D.CONFIGS:
        for nv in D.NVS:
            for path, k in D.nan_levels(name, config, nv).items():
                d = D.deal(name, "nan_at_first", k)
                (what, cell), = d["plants"]
                assert D.positions(name)[cell] == ls[k] and np.isnan(d["x"]).sum() == 1
    # the NaN positions of the restatement are exactly the planted cell's downstream path
    down = E.topology(E.graph(name))[0]
    for k in sorted({k for c in D.CONFIGS for nv in D.NVS for k in D.nan_levels(name, c, nv).values()})[:6]:
        want, c = np.zeros(perm.size, bool), int(perm[ls[k]])
        while c >= 0:
            want[c] = True
            c = down[c]
        assert np.array_equal(np.isnan(D.restated(name, "accuflux", "nan_at_first", k)), want) and want.sum() >= 2


# ---- pointer jumping -------------------------------------------------------------------------------------------------
def test_chains_and_point_deals_are_what_they_claim():
    full = D.graph("chains_full")
    assert len(full["lengths"]) == 29 and full["H"] * full["W"] < 35000 and max(full["lengths"]) == 1025
    assert set(full["lengths"]) >= {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025}
    rounds = {}
    for name in D.CHAINS:
        g = D.graph(name)
        dist = E.topology(g)[2]
        assert sorted(np.bincount(dist)[0:1]) == [len(g["lengths"])] and dist.max() == max(g["lengths"]) - 1
        for kind in D.POINT_DEALS:
            pts = D.points(name, kind)
            assert np.abs(pts).max() < 2 ** 31
            rounds[name, kind] = D.jump_rounds(g, pts)
            mix = D.lane_mix(name, pts)
            if kind == "none" or (name == "chains_tiny" and kind == "nested"):
                assert not pts.any()
                continue
            # every wavefront with a lane that stops at a point also has lanes that keep their parent; and the wavefronts of
            # the last levels hold all three kinds of lane at once (pits lie on the last level only, so nowhere else)
            assert mix["point"] >= 1 and (mix["bare"] == 0 or name == "chains_tiny"), (name, kind, mix)
            assert mix["mixed"] >= 1 or name == "chains_tiny", (name, kind, mix)
        assert (D.points(name, "too_big") == 2 ** 31).sum() == 1
    # no round changes anything on chains of one and two cells; both parities of the number of rounds, so both buffers
    assert rounds["chains_tiny", "none"] == 1
    assert {r % 2 for (name, _), r in rounds.items() if name != "chains_tiny"} == {0, 1}, rounds
    assert rounds["chains_full", "none"] == 11 and rounds["chains_half", "none"] == 10
    ext = D.points("chains_full", "extreme")
    assert (ext == 2 ** 31 - 1).sum() >= 3 and (ext == -1).sum() >= 3
    g = D.graph("chains_full")
    assert set(np.unique(D.restated_subcatchment(g, ext))) >= {-1, 2 ** 31 - 1, 0, 5, 7}
    nested = D.points("chains_full", "nested")
    assert (D.restated_subcatchment(g, nested) != D.restated_catchment(g, nested)).sum() > 1000
