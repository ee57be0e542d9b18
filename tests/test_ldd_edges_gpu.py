"""-m gpu: the LDD reductions and labellings -- k_accu_level, k_accu_narrow, k_accu_cones<NV = 1..4, CW = 64 / 256>, k_upstream_sum
(csrc/lf_router.hip), k_upstream_sum_raster (csrc/lf_modules.hip), k_lddrepair, k_lddmask, k_parents, k_downstream,
k_jump_init, k_jump_step, k_labels, k_totals_gather, k_totals_take (csrc/lf_ldd.hip) -- held to the plain restatements of
tests/ldd_edges.py bit for bit: NaN equals NaN, the sign of a zero counts, integer labels are equal.  There is no tolerance
anywhere, and no case is held to another device run.  tests/test_ldd_edges_cpu.py shows that the restatements are right
(within the derived summation bound of math.fsum) and that the inputs are what they claim; each accuflux case asserts from
last_launches() and route_plan_stats() that it ran the schedule it names.

215 cases, 3.4 s in all on MI355X, the slowest 0.54 s; the mutations the suite was run against are listed in DESIGN.md
section 4.1.2."""
import ctypes as C

import numpy as np
import pytest

import ldd_edges as D
import route_edges as E

pytestmark = pytest.mark.gpu

SWITCHES = ("LF_GENERAL_POW LF_ROUTE_CONES LF_ROUTE_LEVELS LF_ROUTE_SPLIT LF_ROUTE_CONE_WIDTH LF_ROUTE_TUNE LF_FUSED_WIDE "
            "LF_LEVEL_STATICS LF_LEVEL_COUNTS LF_MEMBERS_MB").split()
SENTINEL = -777.25


@pytest.fixture(scope="module")
def amd():
    import types
    from lisflood_amd import _lib, kinematic_wave_parallel, ldd
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return types.SimpleNamespace(kw=kinematic_wave_parallel, lib=_lib, ldd=ldd)


def set_env(monkeypatch, config):
    """the switches of one configuration and nothing else"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in D.CONFIGS[config]["env"].items():
        monkeypatch.setenv(k, v)


def make_router(amd, name):
    g = D.graph(name)
    graph = amd.kw.Graph(ldd_raster=g["codes"], land_mask=None if g["mask"].all() else g["mask"])
    return amd.kw.kinematicWave(None, None, np.ones(g["N"]), 0.6, 1.0, 1.0, graph=graph)


def ldd_device(amd, name):
    g = D.graph(name)
    return amd.ldd.LddDevice(g["codes"][g["mask"]].astype(np.float64), g["mask"])


def same_bits(got, want, what):
    eq = E.bits_equal(got, want)
    assert eq.all(), (what, "cells", np.flatnonzero(~eq)[:8], np.asarray(got)[~eq][:8], np.asarray(want)[~eq][:8])


def sweep(amd, kw, xs):
    """lf_accuflux_ordered_multi_device on engine-order device vectors: xs, pixel order -> the sums, pixel order; the input
    vectors come back unchanged"""
    DA = amd.lib.DeviceArray
    perm = kw.graph.layout()[0]
    nv = len(xs)
    ordered = [np.ascontiguousarray(x[perm]) for x in xs]
    X = [DA.from_host(o) for o in ordered]
    A = [DA.from_host(np.full(perm.size, SENTINEL)) for _ in xs]
    px, pa = (C.c_void_p * nv)(*[d.ptr for d in X]), (C.c_void_p * nv)(*[d.ptr for d in A])
    amd.lib.check(amd.lib.lib().lf_accuflux_ordered_multi_device(kw._h, nv, px, pa))
    out = []
    for v in range(nv):
        pix = np.empty(perm.size)
        pix[perm] = A[v].download()
        out.append(pix)
        same_bits(X[v].download(), ordered[v], ("input vector", v))
    for d in X + A:
        d.free()
    return out


def ran_as_planned(kw, name, config):
    """the launches and the plan are those of the schedule worked out from the layout: k_accu_cones for a block of several
    levels, k_accu_level for a block of one (or a level above 1024 cells), k_accu_narrow for a run of narrower levels"""
    st, plan = kw.last_launches(), kw.route_plan_stats()
    total, single = D.launches(name, config)
    assert st["launches"] == total, (name, config, st, total)
    b = D.blocks(name, config if config != "segments" else "default")
    if any(nl > 1 for _, nl in b):
        assert (plan["blocks"], plan["cone_blocks"]) == (len(b), sum(nl > 1 for _, nl in b)), (name, config, plan)
    else:
        assert plan["cone_blocks"] == 0, plan
    return total, single


# ---- accuflux: the reference form ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.GRAPHS)
def test_accuflux_one_launch_per_level(amd, monkeypatch, name):
    """LF_ROUTE_CONES=0: k_accu_level<NV> on the levels above 1024 cells, k_accu_narrow<NV> on the runs of the others; through
    kinematicWave.accuflux in pixel order and through lf_accuflux_ordered_multi_device with NV = 1..4, vector v the deal v"""
    set_env(monkeypatch, "segments")
    kw = make_router(amd, name)
    for kind in D.VECTOR_DEALS:
        same_bits(kw.accuflux(D.deal(name, kind)["x"]), D.restated(name, "accuflux", kind), (name, kind, "pixel order"))
        total, wide = ran_as_planned(kw, name, "segments")
    assert (wide >= 1) == (not name.startswith("fan")) and (total > wide or name == "many")   # both kernels (fans: narrow)
    for nv in D.NVS:
        got = sweep(amd, kw, [D.deal(name, kind)["x"] for kind in D.VECTOR_DEALS[:nv]])
        for v in range(nv):
            same_bits(got[v], D.restated(name, "accuflux", D.VECTOR_DEALS[v]), (name, "nv", nv, "vector", v))
        ran_as_planned(kw, name, "segments")
    kw.close()


# ---- accuflux: every other form --------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [c for c in D.CONFIGS if c != "segments"])
@pytest.mark.parametrize("name", D.CONE_GRAPHS)
def test_accuflux_on_level_blocks(amd, monkeypatch, name, config):
    """k_accu_cones<NV, 64 / 256> (k_accu_level for a block of one level) with NV = 1..4 under every block length: blocks of
    one full chunk, of a chunk and a ragged one of one level, of several chunks; and the NaN at the first cell of the level
    before a mid-chunk level, before a chunk's first level (PREV) and before a block's first level (memory) -- where the
    schedule of this graph has such a level (tests/test_ldd_edges_cpu.py: main_deep has them all, for every NV and width)"""
    set_env(monkeypatch, config)
    kw = make_router(amd, name)
    for nv in D.NVS:
        kinds = D.VECTOR_DEALS[:nv]
        got = sweep(amd, kw, [D.deal(name, kind)["x"] for kind in kinds])
        for v in range(nv):
            same_bits(got[v], D.restated(name, "accuflux", kinds[v]), (name, config, "nv", nv, "vector", v))
        ran_as_planned(kw, name, config)
        for path, k in D.nan_levels(name, config, nv).items():
            v = k % nv                                            # the vector that carries the NaN
            xs = [D.deal(name, kind)["x"] for kind in kinds]
            xs[v] = D.deal(name, "nan_at_first", k)["x"]
            got = sweep(amd, kw, xs)
            for u in range(nv):
                want = D.restated(name, "accuflux", "nan_at_first", k) if u == v else D.restated(name, "accuflux", kinds[u])
                same_bits(got[u], want, (name, config, "nv", nv, path, "level", k, "vector", u))
    for kind in D.VECTOR_DEALS:                                   # pixel order: gather, sweep, scatter
        same_bits(kw.accuflux(D.deal(name, kind)["x"]), D.restated(name, "accuflux", kind), (name, config, kind, "pixel order"))
    ran_as_planned(kw, name, config)
    kw.close()


# ---- catchment totals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chains_full", "main_deep", "many"])
def test_catchment_totals_of_one_to_nine_vectors(amd, monkeypatch, name):
    """LddDevice.catchment_totals_multi: k_totals_gather, the sweep, k_totals_take with NV = 1..4 and the Python chunking by
    four with a ragged last chunk; the cached outlet table; the parent array shared with catchment and downstream"""
    set_env(monkeypatch, "default")
    g = D.graph(name)
    base = [D.deal(name, kind)["x"] for kind in D.VECTOR_DEALS]
    wants = [D.restated(name, "totals", kind) for kind in D.VECTOR_DEALS]
    scaled = lambda i: base[i % 4] if i < 4 else np.ldexp(base[i % 4], i // 4)     # distinct vectors: exact powers of two
    scaled_want = lambda i: wants[i % 4] if i < 4 else np.ldexp(wants[i % 4], i // 4)
    dev = ldd_device(amd, name)
    for n in (1, 2, 3, 4, 5, 6, 9):
        got = dev.catchment_totals_multi([scaled(i) for i in range(n)])
        assert len(got) == n
        for i in range(n):
            same_bits(got[i], scaled_want(i), (name, n, "vector", i))
    dev.close()
    # a device of its own: the labellings first (they build the parent array), then the totals, twice (the outlet table)
    dev = ldd_device(amd, name)
    pts = D.points(name, "pits" if name in D.CHAINS else "scatter")
    assert np.array_equal(dev.catchment(pts), D.restated_catchment(g, pts))
    same_bits(dev.downstream(base[2]), D.restated_downstream(g, base[2]), (name, "downstream"))
    for call in range(2):
        got = dev.catchment_totals_multi(base[:3])
        for i in range(3):
            same_bits(got[i], wants[i], (name, "after the labellings, call", call, "vector", i))
    dev.close()


# ---- the one-hop upstream sum ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.GRAPHS)
def test_upstream_sum(amd, monkeypatch, name):
    set_env(monkeypatch, "default")
    kw = make_router(amd, name)
    for kind in ("ordered", "random", "signed_zero"):
        same_bits(kw.upstream_sum(D.deal(name, kind)["x"]), D.restated(name, "upstream", kind), (name, kind))
    kw.close()


def test_upstream_sum_skips_structure_links_and_accuflux_refuses_them(amd, monkeypatch):
    set_env(monkeypatch, "default")
    g = D.linked_graph()
    graph = amd.kw.Graph(g["codes"][g["mask"]].astype(np.float64), g["mask"], virtual_down=g["vd"])
    kw = amd.kw.kinematicWave(None, None, np.ones(g["N"]), 0.6, 1.0, 1.0, graph=graph)
    for seed in (1, 2):
        x = np.random.default_rng(seed).uniform(-1.0, 3.0, g["N"])
        x[np.flatnonzero(g["vd"] >= 0)[::3]] = np.nan            # NaN on linked feeders: it must reach nobody
        want = D.restated_upstream(g, x)
        assert not np.isnan(want[g["vd"][g["vd"] >= 0]]).any()
        same_bits(kw.upstream_sum(x), want, ("linked", seed))
    with pytest.raises(amd.lib.LisfloodAmdError) as e:
        kw.accuflux(np.ones(g["N"]))
    assert e.value.code == amd.lib.LF_E_INVALID
    kw.close()


# ---- pointer jumping -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.CHAINS))
def test_labellings_and_downstream_on_chains(amd, monkeypatch, name):
    """k_parents, k_jump_init, k_jump_step (both buffers as the result: tests/test_ldd_edges_cpu.py), k_labels, k_downstream"""
    set_env(monkeypatch, "default")
    g = D.graph(name)
    dev = ldd_device(amd, name)
    for kind in D.POINT_DEALS:
        pts = D.points(name, kind)
        assert np.array_equal(dev.subcatchment(pts), D.restated_subcatchment(g, pts)), (name, kind)
        assert np.array_equal(dev.catchment(pts), D.restated_catchment(g, pts)), (name, kind)
    with pytest.raises(amd.lib.LisfloodAmdError) as e:
        dev.subcatchment(D.points(name, "too_big"))
    assert e.value.code == amd.lib.LF_E_INVALID
    x = D.deal(name, "signed_zero")["x"].copy()
    x[D.spots(3, g["N"])] = np.nan
    x[D.spots(5, g["N"])] = -0.0
    same_bits(dev.downstream(x), D.restated_downstream(g, x), (name, "downstream"))
    dev.close()


@pytest.mark.parametrize("name", ["fan8", "main_shallow_masked", "many"])
def test_labellings_on_trees(amd, monkeypatch, name):
    set_env(monkeypatch, "default")
    g = D.graph(name)
    dev = ldd_device(amd, name)
    pts = D.points(name, "scatter")
    assert np.array_equal(dev.subcatchment(pts), D.restated_subcatchment(g, pts))
    assert np.array_equal(dev.catchment(pts), D.restated_catchment(g, pts))
    x = D.deal(name, "signed_zero")["x"]
    same_bits(dev.downstream(x), D.restated_downstream(g, x), (name, "downstream"))
    dev.close()


# ---- the element-wise and tile kernels ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.REPAIR_SHAPES)
def test_lddrepair_and_lddmask_on_whole_rasters(amd, shape):
    for r, keep in D.repair_rasters(shape):
        assert np.array_equal(amd.ldd._raster_op(r, None, 0), D.restated_lddrepair(r)), (shape, r)
        assert np.array_equal(amd.ldd._raster_op(r, keep, 0), D.restated_lddmask(r, keep)), (shape, r, keep)


@pytest.mark.parametrize("shape", D.UPSTREAM_SHAPES)
def test_upstream_sum_raster(amd, shape):
    for variant in D.VARIANTS:
        ldd, w, _ = D.upstream_raster(shape, variant)
        same_bits(amd.ldd.upstream_raster(ldd, w), D.restated_upstream_raster(ldd, w), (shape, variant))


# ---- argument checks that need a device context ----------------------------------------------------------------------
def test_argument_checks(amd, monkeypatch):
    set_env(monkeypatch, "default")
    lib, DA = amd.lib.lib(), amd.lib.DeviceArray
    invalid = lambda rc: rc == amd.lib.LF_E_INVALID
    kw = make_router(amd, "fan3")
    N = kw.num_pixels
    host, out = np.ones((4, N)), np.empty((4, N))
    X = [DA.from_host(np.ones(N)) for _ in range(2)]
    px, pa = (C.c_void_p * 4)(*[X[0].ptr] * 4), (C.c_void_p * 4)(*[X[1].ptr] * 4)
    for nv in (0, 5):
        assert invalid(lib.lf_catchment_totals_multi_host(kw._h, nv, amd.lib.ptr(host), amd.lib.ptr(out))), nv
        assert invalid(lib.lf_accuflux_ordered_multi_device(kw._h, nv, px, pa)), nv
    with pytest.raises(amd.lib.LisfloodAmdError):
        amd.lib.check(lib.lf_accuflux_ordered_multi_device(kw._h, 5, px, pa))
    kw.close()
    for d in X:
        d.free()
    r = np.full((4, 4), 5, np.uint8)
    o = np.empty_like(r)
    d_l, d_w, d_o = DA.from_host(r), DA.from_host(np.ones((4, 4))), DA((4, 4), np.float64)
    for H, W in ((0, 4), (4, 0)):
        assert invalid(lib.lf_ldd_raster_host(0, amd.lib.ptr(r), None, amd.lib.ptr(o), H, W))
        assert invalid(lib.lf_upstream_sum_raster_device(0, d_l.ptr, d_w.ptr, d_o.ptr, H, W))
    assert invalid(lib.lf_lddrepair_raster_device(0, d_l.ptr, d_l.ptr, 4, 4))       # the output aliases the input
    for d in (d_l, d_w, d_o):
        d.free()
