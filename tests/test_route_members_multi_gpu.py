"""An ensemble on several routers of one graph (lf_router_route_ordered_members_multi): the three overland routers of an
ensemble -- one Graph, three alpha vectors, M members each -- swept with ONE launch per wide level, narrow run or level
block for all (router, member) units.  Every (router, member) row must be bit-identical to route_ordered on that router with
that row alone, in every launch kind and with 1, 2 and 4 members per lane; the shapes, members and configurations are those
of test_members_gpu.py."""
import numpy as np
import pytest

from test_members_gpu import (CALLS, CONFIGS, H, M, N, PAD, REACHES, SENTINEL, W, ZERO_MEMBER, amd, case, make_router, member_calls,
                              rows, single_calls, solver)  # noqa: F401  (amd, case, solver: fixtures)

pytestmark = pytest.mark.gpu

SCALE = (1.0, 1.3, 0.7)            # the three routers' alpha, and their members' starting discharge, relative to the case's


def three_routers(amd, codes, p, graphs=1):
    """three routers with different alpha vectors on one Graph (graphs=2: the last one on a Graph object of its own)"""
    gs = [amd.kw.Graph(ldd_raster=codes) for _ in range(graphs)]
    return [amd.kw.kinematicWave(None, None, p["alpha"] * f, p["beta"], p["dx"], p["dt"], graph=gs[-1 if i == 2 else 0])
            for i, f in enumerate(SCALE)]


def inputs(Q0, lat):
    """-> per router: Q0[M, N], lat[CALLS, M, N] (router i's members start from SCALE[i] * Q0 and get lat shifted by i members)"""
    return [(Q0 * f, np.roll(lat, i, axis=1)) for i, f in enumerate(SCALE)]


def multi_calls(amd, rs, perm, ins, stride, members=None):
    """all routers and members in one call per step -> per router [calls, M, stride] discharge and lateral rows afterwards"""
    members = ins[0][0].shape[0] if members is None else members
    Q = [amd.lib.DeviceArray.from_host(rows(q0, perm, stride)) for q0, _ in ins]
    got, lat_after = [[] for _ in rs], [[] for _ in rs]
    for s in range(ins[0][1].shape[0]):
        q = [amd.lib.DeviceArray.from_host(rows(lat[s], perm, stride)) for _, lat in ins]
        amd.kw.kinematicWave.route_ordered_members_multi(rs, Q, q, members, stride)
        for i in range(len(rs)):
            got[i].append(Q[i].download())
            lat_after[i].append(q[i].download())
            q[i].free()
    for d in Q:
        d.free()
    return [np.stack(g) for g in got], [np.stack(x) for x in lat_after]


def every_unit_as_alone(amd, case, monkeypatch, family, config, graphs=1):
    for k, v in CONFIGS[config].items():
        monkeypatch.setenv(k, v)                  # before the routers exist: LF_FUSED_WIDE is read when they are created
    codes, p, Q0, lat, _ = case(family)
    rs = three_routers(amd, codes, p, graphs)
    perm = rs[0].graph.layout()[0]
    stride = N + PAD
    ins = inputs(Q0, lat)
    alone = [single_calls(amd, r, perm, q0, x) for r, (q0, x) in zip(rs, ins)]
    got, lat_after = multi_calls(amd, rs, perm, ins, stride)
    wide, narrow = REACHES[family, config]
    for r in rs:
        st = r.last_launches()
        assert (st["wide"] > 0) == wide and (st["narrow"] > 0) == narrow, st
    assert not np.array_equal(alone[0], alone[1]) and not np.array_equal(alone[0], alone[2])     # the routers do differ
    for i in range(3):
        zero = (ZERO_MEMBER + i) % M              # (the lateral rows were rolled by i members; Q0's zero row was not)
        for s in range(CALLS):
            for m in range(M):
                assert np.array_equal(got[i][s, m, :N], alone[i][s, m]), (i, s, m)
            assert (got[i][s, :, N:] == SENTINEL).all() and (lat_after[i][s][:, N:] == SENTINEL).all(), (i, s)
            assert np.array_equal(lat_after[i][s][:, :N], ins[i][1][s][:, perm]), (i, s)
        if i == 0:
            assert (got[0][:, zero, :N] == 0.0).all()
    for r in rs:
        r.close()


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("family", ["shallow", "deep"])
def test_units_through_every_launch_kind(amd, case, solver, monkeypatch, family, config):
    monkeypatch.delenv("LF_MEMBERS_MB", raising=False)
    every_unit_as_alone(amd, case, monkeypatch, family, config)


@pytest.mark.parametrize("mb", ["1", "2", "4"])
@pytest.mark.parametrize("config", ["segments", "blocks_wide"])
def test_wide_levels_with_1_2_4_members_per_lane(amd, case, solver, monkeypatch, config, mb):
    """every instantiation of k_level_members<.., MULTI = true>: the groups of 5 members stay within one router"""
    monkeypatch.setenv("LF_MEMBERS_MB", mb)
    every_unit_as_alone(amd, case, monkeypatch, "shallow", config)


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("family", ["shallow", "deep"])
def test_one_launch_for_all_units(amd, case, solver, monkeypatch, family, config):
    """the call for 3 routers x 5 members costs the launches of one single-router call, k_prep of the general exponent
    included as ONE launch"""
    for k, v in CONFIGS[config].items():
        monkeypatch.setenv(k, v)
    codes, p, Q0, lat, _ = case(family)
    rs = three_routers(amd, codes, p)
    perm = rs[0].graph.layout()[0]
    single_calls(amd, rs[0], perm, Q0[:1], lat[:1, :1])
    one = rs[0].last_launches()
    multi_calls(amd, rs, perm, [(q0, x[:1]) for q0, x in inputs(Q0, lat)], N)
    assert one["launches"] >= 1
    for r in rs:
        assert r.last_launches() == one, (one, r.last_launches())
    assert (one["launches"] - one["wide"] - one["narrow"]) == (1 if solver == "general_pow" else 0)
    for r in rs:
        r.close()


def test_one_router_is_the_member_call(amd, case, solver):
    codes, p, Q0, lat, _ = case("shallow")
    kw = make_router(amd, codes, p)
    perm = kw.graph.layout()[0]
    want, want_lat, st = member_calls(amd, kw, perm, Q0, lat, N + PAD)
    got, lat_after = multi_calls(amd, [kw], perm, [(Q0, lat)], N + PAD)
    assert np.array_equal(got[0], want) and np.array_equal(lat_after[0], want_lat) and kw.last_launches() == st
    kw.close()


def test_routers_on_two_graphs_are_swept_one_after_the_other(amd, case, solver, monkeypatch):
    """two Graph objects of the same raster have the same level schedule and so share the level and narrow launches, but
    not one level-block plan: the segments schedule, the same bits"""
    monkeypatch.delenv("LF_MEMBERS_MB", raising=False)
    codes, p, Q0, lat, _ = case("deep")
    rs = three_routers(amd, codes, p, graphs=2)
    perm = rs[0].graph.layout()[0]
    assert np.array_equal(perm, rs[2].graph.layout()[0])
    ins = inputs(Q0, lat)
    alone = [single_calls(amd, r, perm, q0, x) for r, (q0, x) in zip(rs, ins)]
    got, _ = multi_calls(amd, rs, perm, ins, N + PAD)
    for i in range(3):
        assert np.array_equal(got[i][:, :, :N], alone[i]), i
    # ... and routers whose schedules differ (another raster): one member call per router
    other = make_router(amd, case("shallow")[0], p)
    perm2 = other.graph.layout()[0]
    alone2 = single_calls(amd, other, perm2, Q0, lat)
    Q = [amd.lib.DeviceArray.from_host(rows(ins[0][0], perm, N)), amd.lib.DeviceArray.from_host(rows(Q0, perm2, N))]
    for s in range(CALLS):
        q = [amd.lib.DeviceArray.from_host(rows(ins[0][1][s], perm, N)), amd.lib.DeviceArray.from_host(rows(lat[s], perm2, N))]
        amd.kw.kinematicWave.route_ordered_members_multi([rs[0], other], Q, q, M, N)
        assert np.array_equal(Q[0].download(), alone[0][s]) and np.array_equal(Q[1].download(), alone2[s]), s
        for d in q:
            d.free()
    for d in Q:
        d.free()
    for r in rs + [other]:
        r.close()


def test_bad_arguments_leave_the_routers_usable(amd, case, solver):
    codes, p, Q0, lat, _ = case("shallow")
    rs = three_routers(amd, codes, p)
    perm = rs[0].graph.layout()[0]
    ins = [(q0[:2], x[:1, :2]) for q0, x in inputs(Q0, lat)]
    Q = [amd.lib.DeviceArray.from_host(rows(q0, perm, N)) for q0, _ in ins]
    q = [amd.lib.DeviceArray.from_host(rows(x[0], perm, N)) for _, x in ins]
    before = [d.download() for d in Q]
    route = amd.kw.kinematicWave.route_ordered_members_multi
    with pytest.raises(amd.lib.LisfloodAmdError, match="stride %d is less than the number of cells of router 0" % (N - 1)):
        route(rs, Q, q, 2, N - 1)
    with pytest.raises(amd.lib.LisfloodAmdError, match="members must be at least 1"):
        route(rs, Q, q, 0)
    with pytest.raises(amd.lib.LisfloodAmdError, match="count must be 1 to 4"):
        route(rs + rs[:2], Q + Q[:2], q + q[:2], 2)
    with pytest.raises(ValueError, match="member rows"):
        route(rs, Q, q, 3)
    with pytest.raises(Exception, match="The section parameter must be either 'main_channel' or 'floodplain'!"):
        route(rs, Q, q, 2, section="overland")
    with pytest.raises(amd.lib.LisfloodAmdError, match="alpha_floodplains was not given"):
        route(rs, Q, q, 2, section="floodplains")
    for d, b in zip(Q, before):
        assert np.array_equal(d.download(), b)
    alone = [single_calls(amd, r, perm, q0, x) for r, (q0, x) in zip(rs, ins)]
    route(rs, Q, q, 2)
    for i in range(3):
        assert np.array_equal(Q[i].download(), alone[i][0]), i
    for d in Q + q:
        d.free()
    for r in rs:
        r.close()
