"""-m gpu: the cell of a plain router call -- the upstream sum in ascending pixel id, a Qold^beta + q dx, the dispatch between
the quintic and lf_solve_cell -- is written out by hand in sweep_cell_state / sweep_cell_counted, sweep_cone, the supply
wavefront and cone_chain of k_sweep_cones_split, k_sweep_cones_dist and k_prep (csrc/lf_sweep.h).  The inputs of
tests/route_edges.py (corner values on both sides and on the tie of every comparison, ordered upstream sums whose bits tell
the order, on graphs with every in-degree 0..8 in every launch region; tests/test_route_edges_cpu.py shows that they are
what they claim) go through every one of them, three consecutive calls each:

  * the REFERENCE FORM, one launch per level in pixel order (LF_ROUTE_CONES=0, route_device), is held to the oracle at the
    routing tolerance of test_gpu_parity.py (rtol 1e-9 / atol 1e-12) with NaN positions exact, exactly +0.0 wherever the
    oracle has exactly 0 on a planted cell, and the ordered sums and their sources bit for bit;
  * every other form is held to the reference form of the same solver class bit for bit, NaN equal to NaN, after each call,
    and asserts from last_launches() / route_plan_stats() / lf_graph_max_upstream that it ran the kernels it names.

Solver classes: beta = 3/5 fused, LF_GENERAL_POW=1 at beta = 3/5, beta = 0.72.  639 cases, 15.6 s in all on MI355X, the
slowest 0.24 s; the mutations the suite was run against are listed in DESIGN.md section 4.1.1."""
import numpy as np
import pytest

import route_edges as E

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12
SOLVERS = {"fused": (0.6, {}), "general_pow": (0.6, {"LF_GENERAL_POW": "1"}), "beta_0.72": (0.72, {})}
SWITCHES = ("LF_GENERAL_POW LF_ROUTE_CONES LF_ROUTE_LEVELS LF_ROUTE_SPLIT LF_ROUTE_CONE_WIDTH LF_ROUTE_TUNE LF_FUSED_WIDE "
            "LF_LEVEL_STATICS LF_LEVEL_COUNTS LF_MEMBERS_MB").split()
MAINS = ["main_deep", "main_shallow"]
PAD, SENTINEL = 37, -777.25


@pytest.fixture(scope="module")
def amd():
    import types
    from lisflood_amd import _lib, kinematic_wave_parallel
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return types.SimpleNamespace(kw=kinematic_wave_parallel, lib=_lib)


def set_env(monkeypatch, solver, *envs):
    """the switches of one case and nothing else; -> beta"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    beta, env = SOLVERS[solver]
    for e in (env,) + envs:
        for k, v in e.items():
            monkeypatch.setenv(k, v)
    return beta


_inputs = {}


def inputs(name, beta, statics=0, state=0, scalar_dx=False):
    """E.inputs with the static vectors (alpha, dx) of deal `statics` and the state (Q0, lateral inflow) of deal `state`;
    scalar_dx: every channel 1024 m long.  Built once, read-only."""
    key = (name, beta, statics, state, scalar_dx)
    if key not in _inputs:
        a = E.inputs(name, beta=beta, shift=statics)
        b = a if state == statics else E.inputs(name, beta=beta, shift=state)
        d = dict(a, Q0=b["Q0"], lat=b["lat"])
        if scalar_dx:
            d["dx"] = np.full_like(a["dx"], E.DX)
        for k in ("alpha", "dx", "Q0", "lat"):
            d[k] = np.ascontiguousarray(d[k])
            d[k].setflags(write=False)
        _inputs[key] = d
    return _inputs[key]


def make_graph(amd, name):
    g = E.graph(name)
    return amd.kw.Graph(ldd_raster=g["codes"], land_mask=None if g["mask"].all() else g["mask"])


def make_router(amd, graph, inp, scalar_dx=False):
    return amd.kw.kinematicWave(None, None, inp["alpha"], inp["beta"], E.DX if scalar_dx else inp["dx"], inp["dt"], graph=graph)


def run_pixel(amd, kw, inp):
    """three route_device calls -> [CALLS, N] pixel order"""
    DA = amd.lib.DeviceArray
    Q, out = DA.from_host(inp["Q0"]), []
    for s in range(E.CALLS):
        q = DA.from_host(inp["lat"][s])
        kw.route_device(Q, q)
        out.append(Q.download().copy())
        q.free()
    Q.free()
    return np.stack(out)


def run_ordered(amd, kw, inp):
    """three route_ordered calls on vectors resident in engine order -> [CALLS, N] pixel order"""
    DA = amd.lib.DeviceArray
    perm = kw.graph.layout()[0]
    Q, out = DA.from_host(np.ascontiguousarray(inp["Q0"][perm])), []
    for s in range(E.CALLS):
        q = DA.from_host(np.ascontiguousarray(inp["lat"][s][perm]))
        kw.route_ordered(Q, q)
        pix = np.empty(perm.size)
        pix[perm] = Q.download()
        out.append(pix)
        q.free()
    Q.free()
    return np.stack(out)


_reference = {}


def reference(amd, monkeypatch, name, solver, statics=0, state=0):
    """the reference form: one launch per level in pixel order (computed once per input set) -> [CALLS, N], launches"""
    key = (name, solver, statics, state)
    if key not in _reference:
        beta = set_env(monkeypatch, solver, E.CONFIGS["segments"]["env"])
        inp = inputs(name, beta, statics, state)
        kw = make_router(amd, make_graph(amd, name), inp)
        got = run_pixel(amd, kw, inp)
        got.setflags(write=False)
        _reference[key] = (got, kw.last_launches(), kw.route_plan_stats())
        kw.close()
    return _reference[key]


def expected_launches(name, config):
    """(wide, narrow or cone launches) of a call under a configuration, from the layout"""
    ls = E.layout_of(name)[2]
    cfg = E.CONFIGS[config]
    reg, _ = E.regions(ls, cfg["lmax"], cfg["wide"])
    wide = int((reg == "wide").sum())
    if cfg["lmax"] == 0:
        narrow = int(((reg == "narrow") & np.r_[True, reg[:-1] != "narrow"]).sum())
    else:
        narrow = int((reg == "top").sum())
    return wide, narrow


def ran_as_planned(kw, name, config, solver, routers=1):
    """last_launches() and route_plan_stats() of the case are those of the configuration it names"""
    st, plan = kw.last_launches(), kw.route_plan_stats()
    wide, narrow = expected_launches(name, config)
    assert (st["wide"], st["narrow"]) == (wide, narrow), (name, config, st, wide, narrow)
    assert st["launches"] - wide - narrow == (0 if solver == "fused" else routers), st      # k_prep, general exponent
    cfg = E.CONFIGS[config]
    if cfg["lmax"] and narrow:                                # (no block of several levels: no plan, the levels one by one)
        assert plan["blocks"] == E.regions(E.layout_of(name)[2], cfg["lmax"], cfg["wide"])[1] and plan["cone_blocks"] == narrow, plan
        if name == "many" and config in ("default", "levels7"):
            assert plan["max_cones_per_launch"] > 256, plan      # k_sweep_cones_split<.., 1, 4, 2>
        elif name != "many":
            assert 1 <= plan["max_cones_per_launch"] <= 256, plan  # k_sweep_cones_split<.., 1, 8, 4>
    return st


def same_bits(got, want, what):
    for s in range(E.CALLS):
        eq = E.bits_equal(got[s], want[s])
        assert eq.all(), (what, "call", s, "cells", np.flatnonzero(~eq)[:8], got[s][~eq][:8], want[s][~eq][:8])


_oracle = {}


def oracle_calls(oracle, name, beta):
    if (name, beta) not in _oracle:
        g, inp = E.graph(name), inputs(name, beta)
        cpu = oracle.kinematicWave(g["codes"][g["mask"]].astype(np.float64), g["mask"], inp["alpha"], beta, inp["dx"], inp["dt"])
        Q, out = inp["Q0"].copy(), []
        for s in range(E.CALLS):
            with np.errstate(all="ignore"):
                cpu.kinematicWaveRouting(Q, inp["lat"][s])
            out.append(Q.copy())
        _oracle[name, beta] = np.stack(out)
    return _oracle[name, beta]


# ---- the reference form against the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("name", E.GRAPHS)
def test_reference_form_against_the_oracle(amd, oracle, monkeypatch, name, solver):
    got, st, _ = reference(amd, monkeypatch, name, solver)
    beta = SOLVERS[solver][0]
    inp, want = inputs(name, beta), oracle_calls(oracle, name, beta)
    wide, narrow = expected_launches(name, "segments")
    assert (st["wide"], st["narrow"]) == (wide, narrow) and st["launches"] - wide - narrow == (solver != "fused"), st
    planted = inp["planted"]
    for s in range(E.CALLS):
        assert np.array_equal(np.isnan(got[s]), np.isnan(want[s])), (s, np.flatnonzero(np.isnan(got[s]) != np.isnan(want[s]))[:8])
        np.testing.assert_allclose(got[s], want[s], rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=str((name, solver, s)))
        zero = planted & (want[s] == 0)
        assert zero.sum() >= 20 and (got[s][zero].view(np.uint64) == 0).all(), (s, np.flatnonzero(zero & (got[s].view(np.uint64) != 0))[:8])
        for centre, ups, what in inp["fans"]:
            assert got[s][centre] == want[s][centre] and np.array_equal(got[s][ups], want[s][ups]), (s, what, len(ups), got[s][centre], want[s][centre])
    assert np.isnan(want[0]).sum() >= 10 and len(inp["fans"]) >= 4


# ---- engine order, and the wide levels' records and count bytes -----------------------------------------------------
@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("config", ["segments", "default"])
@pytest.mark.parametrize("name", E.GRAPHS)
def test_engine_order(amd, monkeypatch, name, config, solver):
    want, _, _ = reference(amd, monkeypatch, name, solver)
    beta = set_env(monkeypatch, solver, E.CONFIGS[config]["env"])
    inp = inputs(name, beta)
    kw = make_router(amd, make_graph(amd, name), inp)
    same_bits(run_ordered(amd, kw, inp), want, (name, config, solver))
    ran_as_planned(kw, name, config, solver)
    kw.close()


@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("statics,counts", [("1", "1"), ("1", "0"), ("0", "1")])
@pytest.mark.parametrize("config", ["segments", "wide100"])
@pytest.mark.parametrize("name", MAINS)
def test_wide_levels_with_records_and_count_bytes(amd, monkeypatch, name, config, statics, counts, solver):
    """k_level<.., STATICS = 2> (records and count bytes: sweep_cell_counted), STATICS = 1 (records, ups_ptr) and 0 (separate
    streams) on the wide levels of one launch per level and of LF_FUSED_WIDE=100"""
    want, _, _ = reference(amd, monkeypatch, name, solver)
    beta = set_env(monkeypatch, solver, E.CONFIGS[config]["env"], {"LF_LEVEL_STATICS": statics, "LF_LEVEL_COUNTS": counts})
    inp = inputs(name, beta)
    kw = make_router(amd, make_graph(amd, name), inp)
    same_bits(run_ordered(amd, kw, inp), want, (name, config, statics, counts, solver))
    st = ran_as_planned(kw, name, config, solver)
    assert st["wide"] >= 1, st
    kw.close()


# ---- the cone kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("width", ["64", "256"])
@pytest.mark.parametrize("name", E.GRAPHS)
def test_one_wavefront_cones(amd, monkeypatch, name, width, solver):
    """k_sweep_cones<.., 1, 64> (LF_ROUTE_SPLIT=0) and <.., 1, 256> (LF_ROUTE_CONE_WIDTH=256): sweep_cone, in both orders"""
    want, _, _ = reference(amd, monkeypatch, name, solver)
    config = "default" if width == "64" else "cones256"
    beta = set_env(monkeypatch, solver, E.CONFIGS[config]["env"], {"LF_ROUTE_SPLIT": "0"} if width == "64" else {})
    inp = inputs(name, beta)
    kw = make_router(amd, make_graph(amd, name), inp)
    same_bits(run_pixel(amd, kw, inp), want, (name, width, solver, "pixel order"))
    ran_as_planned(kw, name, config, solver)
    same_bits(run_ordered(amd, kw, inp), want, (name, width, solver, "engine order"))
    st = ran_as_planned(kw, name, config, solver)
    assert st["narrow"] >= 1 and kw.route_plan_stats()["cones"] >= 1
    kw.close()


@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("config", ["default", "levels4", "levels7"])
@pytest.mark.parametrize("name", E.GRAPHS)
def test_chain_and_supply_wavefronts(amd, monkeypatch, name, config, solver):
    """k_sweep_cones_split: the supply wavefronts' constant term and block-top sum, cone_chain<KM> with KM the graph's largest
    in-degree (fan1..fan8: every instantiation), in the few-cones shape (8, 4) and, on `many`, the many-cones shape (4, 2);
    blocks of 256, 4 and 7 levels, both orders"""
    want, _, _ = reference(amd, monkeypatch, name, solver)
    beta = set_env(monkeypatch, solver, E.CONFIGS[config]["env"])
    inp = inputs(name, beta)
    kw = make_router(amd, make_graph(amd, name), inp)
    assert kw.graph.max_upstream == (int(name[3:]) if name.startswith("fan") else 8)     # cone_chain<KM>
    same_bits(run_pixel(amd, kw, inp), want, (name, config, solver, "pixel order"))
    st = ran_as_planned(kw, name, config, solver)
    assert st["narrow"] >= 1
    same_bits(run_ordered(amd, kw, inp), want, (name, config, solver, "engine order"))
    ran_as_planned(kw, name, config, solver)
    kw.close()


# ---- several routers of one graph swept together -----------------------------------------------------------------------
@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("nr", [2, 3, 4])
@pytest.mark.parametrize("config", ["default", "default-split0", "cones256", "segments", "wide100"])
@pytest.mark.parametrize("name", MAINS + ["main_deep_masked"])
def test_routers_swept_together(amd, monkeypatch, name, config, nr, solver):
    """route_together in pixel and in engine order: on the block schedule k_sweep_cones_split<.., NR, 4, 2> and, with
    LF_ROUTE_SPLIT=0 / LF_ROUTE_CONE_WIDTH=256, sweep_cone<NR, 64 / 256> in k_sweep_cones<.., NR, ..>; k_level_multi (wide
    levels) and k_levels_narrow_multi (narrow runs).  Router r has the planted rows dealt out r places on: its alpha, its
    old discharge and its inflow differ from its neighbours' on every planted cell."""
    DA = amd.lib.DeviceArray
    wants = [reference(amd, monkeypatch, name, solver, r, r)[0] for r in range(nr)]
    split0 = config.endswith("-split0")
    config = config.split("-")[0]
    beta = set_env(monkeypatch, solver, E.CONFIGS[config]["env"], {"LF_ROUTE_SPLIT": "0"} if split0 else {})
    inps = [inputs(name, beta, r, r) for r in range(nr)]
    graph = make_graph(amd, name)
    routers = [make_router(amd, graph, inp) for inp in inps]
    perm = graph.layout()[0]
    for ordered in (False, True):
        to_dev = (lambda x: np.ascontiguousarray(x[perm])) if ordered else (lambda x: x)
        Qs = [DA.from_host(to_dev(inp["Q0"])) for inp in inps]
        for s in range(E.CALLS):
            lats = [DA.from_host(to_dev(inp["lat"][s])) for inp in inps]
            amd.kw.kinematicWave.route_together(routers, Qs, lats, engine_order=ordered)
            for r in range(nr):
                got = Qs[r].download()
                if ordered:
                    pix = np.empty(perm.size)
                    pix[perm] = got
                    got = pix
                eq = E.bits_equal(got, wants[r][s])
                assert eq.all(), (name, config, nr, solver, ordered, "router", r, "call", s, np.flatnonzero(~eq)[:8])
            for q in lats:
                q.free()
        for Q in Qs:
            Q.free()
        ran_as_planned(routers[0], name, config, solver, routers=nr)
    for kw in routers:
        kw.close()


# ---- an ensemble on one router -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("mb", ["1", "2", "4"])
@pytest.mark.parametrize("config", ["default", "segments", "wide100", "cones256"])
@pytest.mark.parametrize("name", MAINS)
def test_five_members(amd, monkeypatch, name, config, mb, solver):
    """route_ordered_members, 5 members, stride N + 37: k_level_members<MB = 1, 2, 4>, k_levels_narrow_members,
    k_sweep_cones_members at 64 and 256 (and k_prep_members).  Member 0 has the planted values, member m the planted old
    discharges and inflows dealt out m places on (the statics are the router's)."""
    M = 5
    DA = amd.lib.DeviceArray
    wants = [reference(amd, monkeypatch, name, solver, 0, m)[0] for m in range(M)]
    beta = set_env(monkeypatch, solver, E.CONFIGS[config]["env"], {"LF_MEMBERS_MB": mb})
    inps = [inputs(name, beta, 0, m) for m in range(M)]
    kw = make_router(amd, make_graph(amd, name), inps[0])
    perm = kw.graph.layout()[0]
    N, stride = perm.size, perm.size + PAD

    def rows(vectors):
        out = np.full((M, stride), SENTINEL)
        for m, v in enumerate(vectors):
            out[m, :N] = v[perm]
        return out
    Q = DA.from_host(rows([inp["Q0"] for inp in inps]))
    for s in range(E.CALLS):
        q = DA.from_host(rows([inp["lat"][s] for inp in inps]))
        kw.route_ordered_members(Q, q, M, stride)
        got = Q.download()
        q.free()
        assert (got[:, N:] == SENTINEL).all()
        for m in range(M):
            eq = E.bits_equal(got[m, :N], wants[m][s][perm])
            assert eq.all(), (name, config, mb, solver, "member", m, "call", s, perm[np.flatnonzero(~eq)[:8]])
    Q.free()
    st = ran_as_planned(kw, name, config, solver)
    if config in ("segments", "wide100"):
        assert st["wide"] >= 1                                # k_level_members<.., MB>
    kw.close()


# ---- scalar dx, and the row-block partition ----------------------------------------------------------------------------
@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("config", ["segments", "default", "wide100"])
@pytest.mark.parametrize("name", MAINS + ["fan8", "many"])
def test_scalar_dx_on_the_single_domain(amd, monkeypatch, name, config, solver):
    """every channel 1024 m long: a router built with the scalar (no dx stream, no (a, dx) records) against the reference
    form built with the vector of the same value, in both orders"""
    beta = set_env(monkeypatch, solver, E.CONFIGS["segments"]["env"])
    inp = inputs(name, beta, scalar_dx=True)
    ref = make_router(amd, make_graph(amd, name), inp)
    want = run_pixel(amd, ref, inp)
    ref.close()
    set_env(monkeypatch, solver, E.CONFIGS[config]["env"])
    kw = make_router(amd, make_graph(amd, name), inp, scalar_dx=True)
    same_bits(run_pixel(amd, kw, inp), want, (name, config, solver, "pixel order"))
    same_bits(run_ordered(amd, kw, inp), want, (name, config, solver, "engine order"))
    ran_as_planned(kw, name, config, solver)
    assert np.isnan(want[0]).sum() >= 10
    kw.close()


def partition_launches(graph, cones_on, general):
    """What one loopback call launches on one block of the partition, from its DistGraph alone (csrc/lf_dist.hip:
    dist_compute_phase, dist_pack): dict(prep, packs, cones, levels, wide, narrow, total).  With level blocks (the graph has a
    route plan and LF_ROUTE_CONES is not 0) every block of the plan is one launch -- k_sweep_cones_dist for a block of several
    launch units (`cones`), the level kernel for a block of one (`levels`); otherwise every stage (phase, part) goes segment
    by segment: a unit of more than 1024 cells is one launch of the level kernel (`wide`), a run of smaller ones one launch
    of k_levels_narrow (`narrow`).  k_prep once for the general exponent, one pack per halo round with anything to send."""
    import ctypes as C
    from lisflood_amd import _lib
    sizes = (C.c_int64 * 5)()
    _lib.check(_lib.lib().lf_dist_graph_get_route_plan(graph._h, sizes, None, None, None, None, None, None))
    ls = np.empty(int(sizes[4]), np.int64)
    _lib.check(_lib.lib().lf_dist_graph_get_route_plan(graph._h, sizes, None, None, None, None, None, _lib.ptr(ls)))
    assert ls.size - 1 == graph.num_launch_units and (np.diff(ls) > 0).all()      # no empty unit: positions name units
    nph = graph.num_phases
    stages = [tuple(int(np.searchsorted(ls, x)) for x in graph.part_range(j, pt)) for j in range(nph) for pt in (0, 1)]
    assert stages[0][0] == 0 and stages[-1][1] == ls.size - 1 and all(a[1] == b[0] for a, b in zip(stages, stages[1:]))
    out = dict(prep=int(general and graph.num_pixels > 0), cones=0, levels=0, wide=0, narrow=0,
               packs=sum(1 for j in range(nph - 1) if sum(graph.round_counts(j)["send"]) > 0))
    plan = graph.route_plan()
    if plan is not None and cones_on:
        first = plan["level"]
        assert [int(first[b]) for b in plan["stage_block"]] == [k0 for k0, _ in stages] + [ls.size - 1]  # the plan's stages
        units = np.diff(first)
        out["cones"], out["levels"] = int((units > 1).sum()), int((units == 1).sum())
    else:
        for k0, k1 in stages:
            wide = np.diff(ls[k0:k1 + 1]) > E.SEGMENT_WIDE
            out["wide"] += int(wide.sum())
            out["narrow"] += int((~wide & np.r_[True, wide[:-1]]).sum())
    out["total"] = sum(out.values())
    return out


def cuts_through_fans(name, nblocks):
    """row blocks whose cuts run between the centre of a planted ordered sum and its northern neighbours: the confluence
    reads them from ghost slots"""
    g, inp = E.graph(name), inputs(name, 0.6)
    assert g["mask"].all()
    rows = sorted(set(c // g["W"] for c, ups, _ in inp["fans"] if len(ups) >= 3 and min(ups) // g["W"] < c // g["W"]))
    want = [g["H"] * (i + 1) // nblocks for i in range(nblocks - 1)]
    cut = [min(rows, key=lambda r: abs(r - w)) for w in want]
    assert len(set(cut)) == nblocks - 1 and 0 < cut[0] and cut[-1] < g["H"]
    straddle = sum(1 for c, ups, _ in inp["fans"] if c // g["W"] in cut and min(ups) // g["W"] < c // g["W"])
    assert straddle >= nblocks - 1
    edges = [0] + cut + [g["H"]]
    return list(zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("cones", ["0", None])
@pytest.mark.parametrize("scalar_dx", [False, True])
@pytest.mark.parametrize("nblocks", [2, 3])
@pytest.mark.parametrize("name", MAINS)
def test_row_block_partition_in_loopback(amd, monkeypatch, name, nblocks, scalar_dx, cones, solver):
    """dist.loopback_route: the partition's level kernel (24-byte records with per-pixel dx, separate streams with a scalar
    dx), its narrow runs and k_sweep_cones_dist, with planted ordered sums reading ghost slots"""
    from lisflood_amd import dist as D
    beta = set_env(monkeypatch, solver, E.CONFIGS["segments"]["env"])
    inp = inputs(name, beta, scalar_dx=scalar_dx)
    if scalar_dx:
        ref = make_router(amd, make_graph(amd, name), inp)
        want = run_pixel(amd, ref, inp)
        ref.close()
    else:
        want = reference(amd, monkeypatch, name, solver)[0]
    set_env(monkeypatch, solver, {} if cones is None else {"LF_ROUTE_CONES": cones})
    g = E.graph(name)
    codes, W = g["codes"], g["W"]
    blocks = cuts_through_fans(name, nblocks)
    graphs = [D.DistGraph(codes[r0:r1], None, codes[r0 - 1] if r0 > 0 else None, None, codes[r1] if r1 < g["H"] else None, None)
              for (r0, r1) in blocks]
    D.settle_phases_local(graphs)
    sl = [slice(r0 * W, r1 * W) for (r0, r1) in blocks]
    routers = [D.DistRouter(gr, inp["alpha"][s], beta, E.DX if scalar_dx else inp["dx"][s], inp["dt"]) for gr, s in zip(graphs, sl)]
    Qs = [r.new_state(inp["Q0"][s]) for r, s in zip(routers, sl)]
    plans = [partition_launches(gr, cones is None, solver != "fused") for gr in graphs]
    for step in range(E.CALLS):
        lats = [r.new_state(inp["lat"][step][s]) for r, s in zip(routers, sl)]
        before = [r.last_launches() for r in routers]
        D.loopback_route(routers, Qs, lats)
        # every block launched what its graph and LF_ROUTE_CONES say (the count runs on from call to call)
        for k, r in enumerate(routers):
            assert r.last_launches() - before[k] == plans[k]["total"], (name, nblocks, cones, solver, "block", k, "call", step, plans[k])
        got = np.concatenate([r.download_pix(Q) for r, Q in zip(routers, Qs)])
        eq = E.bits_equal(got, want[step])
        assert eq.all(), (name, nblocks, scalar_dx, cones, solver, "call", step, np.flatnonzero(~eq)[:8])
        for d in lats:
            d.free()
    if cones is None:
        # k_sweep_cones_dist ran: a block of the partition has a route plan with blocks of several units, and the other
        # schedule would have taken another number of launches on it
        assert any(gr.route_plan() is not None for gr in graphs) and sum(p["cones"] for p in plans) >= 1, plans
        other = [partition_launches(gr, False, solver != "fused") for gr in graphs]
        assert any(p["cones"] and p["total"] != o["total"] for p, o in zip(plans, other)), (plans, other)
    else:
        assert sum(p["cones"] + p["levels"] for p in plans) == 0 and sum(p["narrow"] for p in plans) >= 1, plans
        if name == "main_shallow":
            assert sum(p["wide"] for p in plans) >= 1, plans      # the level kernel: 24-byte records, or separate streams
    for Q in Qs:
        Q.free()
    for r in routers:
        r.close()
