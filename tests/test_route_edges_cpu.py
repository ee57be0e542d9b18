"""The inputs of tests/test_route_edges_gpu.py are what tests/route_edges.py says they are, shown without a GPU: the graphs
hold the in-degrees and level shapes per launch region (from Graph.layout(), lf_graph_max_upstream and the host-only plan
functions), the C oracle equals the numpy restatement of solve1Pixel and the sweep bit for bit on them, every planted row
takes the branch it is planted for, the exact claims (zeros, both sides of the 1e-12 tie, ordered upstream sums) hold in the
oracle, and no unplanted cell lies where the last ulp of a pow could move it across a branch."""
import ctypes as C

import numpy as np
import pytest

import route_edges as E


def plan_stats(name, lmax, wide, cw):
    """(lf_graph_block_plan_stats, lf_graph_block_plan_check) of a graph: host only"""
    from lisflood_amd import _lib
    from lisflood_amd.kinematic_wave_parallel import Graph
    g = E.graph(name)
    G = Graph(ldd_raster=g["codes"], land_mask=None if g["mask"].all() else g["mask"])
    st, ck = (C.c_int64 * 6)(), (C.c_int64 * 4)()
    _lib.check(_lib.lib().lf_graph_block_plan_stats(G._h, lmax, wide, cw, st))
    _lib.check(_lib.lib().lf_graph_block_plan_check(G._h, lmax, wide, cw, ck))
    G.close()
    return list(st), list(ck)


@pytest.mark.parametrize("name", E.GRAPHS)
def test_graphs_hold_the_in_degrees_and_the_plans_they_are_built_for(name):
    g = E.graph(name)
    perm, ups_ptr, ls, kmax = E.layout_of(name)
    cnt = np.diff(ups_ptr)
    NL = len(ls) - 1
    assert np.array_equal(np.sort(perm), np.arange(g["N"]))
    if name.endswith("_masked") or name.startswith("fan"):
        assert not g["mask"].all()                           # pixel order is not raster order
    k = int(name[3:]) if name.startswith("fan") else 8
    assert kmax == k and cnt.max() == k                      # lf_graph_max_upstream: the chain kernel runs cone_chain<KM = k>
    assert set(np.unique(cnt)) == set(range(k + 1))          # cells of every in-degree 0..k
    # in-degree 8: a pit (nothing left to drain to), so on the last level; in-degree 7 drains through the eighth neighbour
    assert (E.level_of(ls, np.flatnonzero(cnt == 8)) == NL - 1).all()
    if k >= 7:
        assert (E.level_of(ls, np.flatnonzero(cnt == 7)) < NL - 1).any()
    for config, cfg in E.CONFIGS.items():
        if cfg["lmax"] == 0:
            continue
        st, ck = plan_stats(name, cfg["lmax"], cfg["wide"], cfg["cw"])
        reg, blocks = E.regions(ls, cfg["lmax"], cfg["wide"])
        assert blocks == st[0], (config, blocks, st)         # the regions below are the plan's
        assert ck[0] == 0 and ck[1] <= cfg["cw"] and ck[2] <= k, (config, ck)
        if name == "many" and config in ("default", "levels7"):
            # more than 256 cones in one launch: k_sweep_cones_split<.., 1, 4, 2>; two chunks of four levels, the last ragged
            assert st[5] > 256 and np.diff(ls).max() > 16384 and g["N"] < 100000 and NL == 5, (st, NL)
        elif name != "many":
            assert st[5] <= 256, (config, st)                # the few-cones shape (KC, NS) = (8, 4)
    if name.startswith("fan") or name.startswith("main_deep"):
        # one block of all levels by default: more than one chunk of 8 levels and a ragged last one
        st, _ = plan_stats(name, 256, E.DEFAULT_WIDE, 64)
        assert st[:2] == [1, 1] and NL >= 10 and NL > 8 and NL % 8 != 0, (st, NL)


@pytest.mark.parametrize("name", E.GRAPHS)
def test_every_in_degree_lies_in_every_launch_region(name):
    """per graph and launch configuration: which in-degrees lie in wide levels, in narrow runs, inside a level block and on
    a block's first level"""
    k = int(name[3:]) if name.startswith("fan") else 8
    perm, ups_ptr, ls, _ = E.layout_of(name)
    census = {config: E.region_census(name, config)[0] for config in E.CONFIGS}
    print(name, {c: {r: sorted(d) for r, d in v.items() if d} for c, v in census.items()})
    # inside a block (inflow through LDS): every in-degree 0..k, in every block configuration
    # (a pit of in-degree 8 lies on the last level, which short blocks may leave as a block of its own: a wide level)
    for config in ("default", "levels4", "levels7", "cones256"):
        kk = k if config in ("default", "cones256") else min(k, 7)
        assert set(census[config]["inside"]) >= set(range(1, kk + 1)), (config, census[config])
        assert 0 in census[config]["inside"] or 0 in census[config]["top"]
    # a block's first level (inflow from memory): every in-degree 0..min(k, 7) under LF_ROUTE_LEVELS = 4 or 7
    if name != "many":
        tops = set(census["levels4"]["top"]) | set(census["levels7"]["top"])
        assert tops >= set(range(0, min(k, 7) + 1)), (name, tops)
        for j in range(1, min(k, 7) + 1):                    # the in-degree-k cells themselves: at least 1 each, both places
            assert census["levels4"]["top"].get(j, 0) + census["levels7"]["top"].get(j, 0) >= 1
            assert min(census["levels4"]["inside"].get(j, 0), census["levels7"]["inside"].get(j, 0)) >= 1
    # one launch per level: the fans run narrow (their last level too: in-degree 8 in a narrow run), the others have wide levels
    if name.startswith("fan"):
        assert not census["segments"]["wide"] and set(census["segments"]["narrow"]) == set(range(k + 1))
    else:
        assert set(census["segments"]["wide"]) == set(range(9)), census["segments"]["wide"]
    if name.startswith("main"):
        assert set(census["segments"]["narrow"]) >= set(range(8))
        # LF_FUSED_WIDE = 100: single-level blocks among the level blocks, every in-degree in them
        assert set(census["wide100"]["wide"]) == set(range(9)) and census["wide100"]["inside"], census["wide100"]


@pytest.mark.parametrize("name", ["main_deep", "main_shallow", "main_shallow_masked"])
def test_wide_levels_of_main_have_the_shapes_where_the_range_arithmetic_can_go_wrong(name):
    perm, ups_ptr, ls, _ = E.layout_of(name)
    for config in ("wide100", "segments"):
        reg, _ = E.regions(ls, E.CONFIGS[config]["lmax"], E.CONFIGS[config]["wide"])
        have = E.wide_shapes(ups_ptr, ls, reg == "wide")
        print(name, config, have)
        for shape, count in have.items():
            # (one launch per level on main_deep: the wide levels are the last two, whose partial last wavefronts hold only
            # cells that nothing drains into -- sources and isolated pits come last in a level)
            assert count >= 1 or (config, name, shape) == ("segments", "main_deep", "tail"), (name, config, shape, have)
    # cones of the 256-wide plan with more than 64 cells in a level: fewer cones than the widest level has 64-cell chunks
    st, _ = plan_stats(name, 256, E.DEFAULT_WIDE, 256)
    assert st[2] * 64 < np.diff(ls).max(), st


_runs = {}


def oracle_and_restatement(oracle, name, beta):
    """three calls through the oracle and through the restatement (computed once)"""
    if (name, beta) not in _runs:
        g, inp = E.graph(name), E.inputs(name, beta=beta)
        cpu = oracle.kinematicWave(g["codes"][g["mask"]].astype(np.float64), g["mask"], inp["alpha"], beta, inp["dx"], inp["dt"])
        Qo, Qr = inp["Q0"].copy(), inp["Q0"].copy()
        calls = []
        for s in range(E.CALLS):
            before = Qr.copy()
            with np.errstate(all="ignore"):
                cpu.kinematicWaveRouting(Qo, inp["lat"][s])
            info = E.restated_call(g, inp, Qr, inp["lat"][s])
            calls.append(dict(before=before, oracle=Qo.copy(), restated=Qr.copy(), info=info))
        _runs[name, beta] = (inp, calls)
    return _runs[name, beta]


CASES = [(n, 0.6) for n in E.GRAPHS] + [(n, 0.72) for n in ("fan5", "fan8", "main_deep", "main_shallow")]


@pytest.mark.parametrize("name,beta", CASES)
def test_oracle_equals_the_restatement_and_no_unplanted_cell_is_near_a_branch(oracle, name, beta):
    inp, calls = oracle_and_restatement(oracle, name, beta)
    for s, c in enumerate(calls):
        assert np.array_equal(np.isnan(c["oracle"]), np.isnan(c["restated"])), s
        assert E.bits_equal(c["oracle"], c["restated"]).all(), (s, np.flatnonzero(~E.bits_equal(c["oracle"], c["restated"]))[:5])
        near = E.near_a_branch(inp, c["info"], c["before"])
        assert near.size == 0, (s, near[:5])
    # NaN and beyond-1e30 results stay on pits and one cell above a pit
    down, _, dist = E.topology(E.graph(name))
    last = calls[-1]["oracle"]
    with np.errstate(invalid="ignore"):
        wild = np.isnan(last) | (np.abs(last) > 1e29)
    assert wild.sum() >= 10 and (dist[wild] <= 1).all()


@pytest.mark.parametrize("name", E.GRAPHS)
def test_every_census_row_is_hit_at_each_in_degree_it_is_planted_for(oracle, name):
    inp, calls = oracle_and_restatement(oracle, name, 0.6)
    cen = E.census(inp, calls[0]["info"], calls[0]["restated"])
    k = int(name[3:]) if name.startswith("fan") else 8
    for kind in E.OWN:
        assert kind in cen and kind in E.EXPECT, kind        # every row of its own is planted, and its branch is stated
    for kind, want in E.EXPECT.items():
        got = sorted(set(x for v in cen.get(kind, {}).values() for x in v))
        if kind == "conf_tie_above" and name == "many":      # (no one-star trees there: its pits have no exact-zero inflow)
            continue
        assert got == [want], (kind, got, want)
    # the confluence rows at every in-degree: the tie 1..k (one side on any cell, the NaN side on pits), the ordered sums 1..k
    degs = set(range(1, k + 1))
    top = set(range(1, min(k, 7) + 1))
    for kind in ("fan_asc", "fan_mirror", "fan_asc_lat", "conf_tie_on", "conf_tie_on_fast"):
        assert set(cen[kind]) >= (top if name == "many" else degs), (kind, sorted(cen[kind]))
    if name != "many":
        assert set(cen["conf_tie_above"]) >= degs
    # both arms of t <= 1 beyond the fast range (the fused forms run lf_solve_cell there), the floor, the closed first guess
    info = calls[0]["info"]
    with np.errstate(invalid="ignore"):
        out = ~((info["a"] >= E.FAST_MIN) & (info["a"] <= E.FAST_MAX) & (info["c"] >= E.FAST_MIN) & (info["c"] <= E.FAST_MAX))
    out &= info["branch"] != "le_tol"
    assert (info["branch"][out] == "t<=1").sum() >= 3 and (info["branch"][out] == "t>1").sum() >= 3
    assert (info["floored"] & out).sum() >= 1
    # ... and of the general-exponent forms on the random fill
    assert (info["branch"][~inp["planted"]] == "t<=1").sum() >= 50 and (info["branch"][~inp["planted"]] == "t>1").sum() >= 50


@pytest.mark.parametrize("name,beta", CASES)
def test_the_exact_claims_hold_in_the_oracle(oracle, name, beta):
    inp, calls = oracle_and_restatement(oracle, name, beta)
    kinds = {}
    for kind, cell, indeg, role in inp["rows"]:
        kinds.setdefault(kind, []).append(cell)
    plus_zero = lambda x: (np.ascontiguousarray(x).view(np.uint64) == 0).all()
    for s, c in enumerate(calls):
        Q = c["oracle"]
        # exactly +0.0: c on the tie, c of 0, -0.0 and below 0, c at the lower end of the fast range, the floor
        for kind in ("tie_on", "tie_on_fast", "conf_tie_on", "conf_tie_on_fast", "c_zero", "c_negzero", "c_negative", "c_1e-30", "c_below_1e-30", "c_above_1e-30", "floor"):
            assert plus_zero(Q[kinds[kind]]), (s, kind)
        # one ulp above the tie with alpha = 0: NaN
        for kind in ("tie_above", "conf_tie_above"):
            if kind in kinds:
                assert np.isnan(Q[kinds[kind]]).all(), (s, kind)
        # the first guess closes: a positive value below 1e-12, where the exact root is of the order 1e-19
        if s == 0:
            assert ((Q[kinds["first_guess"]] > 0) & (Q[kinds["first_guess"]] < 1e-12)).all()
        # the ordered sums: the sources return their inflow, the confluence the sum in ascending pixel id, bit for bit
        differs = 0
        for centre, ups, what in inp["fans"]:
            vals = [E.BIG] + [1.0] * (len(ups) - 1)
            vals = vals[::-1] if what == "fan_mirror" else vals
            assert np.array_equal(Q[ups], vals), (s, what, len(ups))
            acc = np.float64(0.0)
            for v in vals:
                acc = acc + v
            if what == "fan_asc_lat":                        # its own inflow of 2 comes last: 2^53 + 2, where a sum started
                assert Q[centre] == acc + 2.0 == E.BIG + 2.0  # from it gives 2^53 + 4 from two terms on
                other = np.float64(2.0)
                for v in vals:
                    other = other + v
                assert (other != Q[centre]) == (len(ups) >= 2)
                continue
            assert Q[centre] == acc, (s, what, len(ups), Q[centre], acc)
            rev = np.float64(0.0)
            for v in vals[::-1]:
                rev = rev + v
            differs += int(rev != acc)
            assert (rev != acc) == (len(ups) >= 3)           # from three terms on the other order gives other bits
        assert differs == sum(len(ups) >= 3 and what != "fan_asc_lat" for _, ups, what in inp["fans"])
    assert calls[0]["oracle"][inp["fans"][0][0]] in (9007199254740992.0, 9007199254741000.0)


def test_ordered_sums_lie_in_every_region_and_beside_a_large_neighbour(oracle):
    """the ordered-sum confluences per launch region and in-degree; and those of odd in-degree whose last pair load takes
    in, as its second value, a discharge of 2^52 or more from the position behind the run (discarded by sweep_cell_state)"""
    union = {}
    for name in E.GRAPHS:
        inp, calls = oracle_and_restatement(oracle, name, 0.6)
        perm, ups_ptr, ls, _ = E.layout_of(name)
        found = {}
        for config in E.CONFIGS:
            for region, d in E.region_census(name, config, inp)[1].items():
                found.setdefault(region, set()).update(d)
                union.setdefault(region, set()).update(d)
        print(name, {r: sorted(v) for r, v in found.items()})
        if name.startswith("main"):
            assert found["wide"] >= set(range(2, 9)) and found["inside"] >= set(range(2, 9)), (name, found)
        if name == "many":
            assert found["inside"] >= set(range(2, 8)), found
        if name.startswith("fan"):
            assert found["narrow"] >= set(range(2, int(name[3:]) + 1)), (name, found)
        pos = np.empty(perm.size, np.int64)
        pos[perm] = np.arange(perm.size)
        Q = calls[0]["oracle"]
        beside = 0
        for centre, ups, what in inp["fans"]:
            p = pos[centre]
            behind = ups_ptr[p + 1]
            if len(ups) % 2 == 1 and E.level_of(ls, behind) == E.level_of(ls, p) - 1:
                beside += int(Q[perm[behind]] >= 2.0 ** 52)
        if not name.startswith("fan") or int(name[3:]) >= 3:
            assert beside >= 1, (name, beside)
    # every in-degree 2..8 (a block's first level: 2..7) in every region, over the graphs
    assert union["wide"] >= set(range(2, 9)) and union["narrow"] >= set(range(2, 9)) and union["inside"] >= set(range(2, 9))
    assert union["top"] >= set(range(2, 8)), union
