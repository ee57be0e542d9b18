"""-m gpu: the time-major form of the routing sub-step loop with lakes, reservoirs, inflow hydrographs and transmission
loss in the loop (k_fused_level_steps<.., STRUCT>, lf_fused.h) against the sub-step-by-sub-step engine bit for bit, against
the oracle loop at the tolerances of test_module_edges_gpu.test_sites_inside_the_loop_for_each_option_set, and against the
skewed wavefront of the same build.  The inputs are those of tests/module_edges.py (120 x 160, 130 lakes + 190 reservoirs
that visit every regime of the site arithmetic); the chained scenario is the one of tests/test_site_plan_cpu.py, where
the plan does not apply and the call must keep the skew."""
import types

import numpy as np
import pytest

import module_edges as E
from test_module_edges_gpu import RTOL, _loop_keys

pytestmark = pytest.mark.gpu

SWITCH = "LF_FUSED_TIME_MAJOR"
_inputs = {}
_stepwise = {}


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def _loop_inputs(family):
    if family not in _inputs:
        _inputs[family] = E.loop_inputs(family)
    return _inputs[family]


def _module(r, s, cut, mask, switches):
    from lisflood_amd import routing as R
    v = E.loop_var(r, s)
    m = R.routing(v, options=dict(SplitRouting=True, InitLisflood=False, **switches), engine_order=True)
    m.attach_router(cut, mask)
    m.attach_structures()
    return v, m


def _snapshot(v, keys):
    return {k: np.array(getattr(v, k), copy=True) for k in keys}


def _same(got, want, what):
    for k in want:
        assert E.same_bits(got[k], want[k]), "%s %s: %s" % (what, k, E.first_difference(got[k], want[k]))


def _site_levels(m):
    """number of levels that hold a lake or reservoir cell of routing module m"""
    level_start = m.river_router.graph.layout()[2]
    cells = [np.asarray(getattr(m.var, k)) for k, o in (("LakeIndex", "simulateLakes"), ("ReservoirIndex", "simulateReservoirs"))
             if m.options.get(o)]
    if not cells:
        return 0
    pos = m._pos[np.concatenate(cells).astype(np.int64)]
    return np.unique(np.searchsorted(level_start, pos, side="right") - 1).size


def _reference(family, name):
    """24 x dynamic(s), once per (family, option set): the state after the first model step"""
    key = (family, name)
    if key not in _stepwise:
        r, s, cut, mask = _loop_inputs(family)
        va, ma = _module(r, s, cut, mask, E.LOOP_OPTION_SETS[name])
        for sub in range(int(r["NoRoutSteps"])):
            ma.dynamic(sub)
        _stepwise[key] = _snapshot(va, _loop_keys(E.LOOP_OPTION_SETS[name]))
    return _stepwise[key]


@pytest.mark.parametrize("name", list(E.LOOP_OPTION_SETS))
@pytest.mark.parametrize("family", ["shallow", "deep"])
def test_time_major_with_each_option_set(amd, oracle, monkeypatch, family, name):
    """dynamic_fused() under LF_FUSED_TIME_MAJOR=1 reports the time-major form (the skew on the parent commit), in at most
    num_levels + 2 x (levels holding a site) launches, and leaves the bits of 24 x dynamic(s) in every vector of
    _loop_keys -- NaN sites included --; against the oracle loop it holds the tolerances of
    test_sites_inside_the_loop_for_each_option_set.  The same inputs under LF_FUSED_TIME_MAJOR=0 take a skewed form
    and leave the same bits.  shallow: 8 levels, up to 240 site lanes in one launch; deep: 118 levels, 110 with sites."""
    r, s, cut, mask = _loop_inputs(family)
    switches = E.LOOP_OPTION_SETS[name]
    nsteps = int(r["NoRoutSteps"])
    keys = _loop_keys(switches)
    want = _reference(family, name)
    monkeypatch.setenv(SWITCH, "1")
    vb, mb = _module(r, s, cut, mask, switches)
    mb.dynamic_fused()
    form, launches = mb.river_router.last_fused_form(), mb.river_router.last_launches()["launches"]
    nl, site_levels = mb.river_router.graph.num_levels, _site_levels(mb)
    print("%s %s: form %s, %d launches, %d levels, %d with sites" % (family, name, form, launches, nl, site_levels))
    assert form == "time-major"
    assert launches <= nl + 2 * site_levels
    _same(_snapshot(vb, keys), want, (family, name, "time-major"))
    vc, _ = E.loop_oracle_run(oracle, family, name)
    cancel = 256 * np.finfo(float).eps * float(np.nanmax(vc.ChanQ)) * r["DtRouting"]
    for k in keys:
        atol = cancel * (nsteps if k == "TransCum" else 1) if k in ("TransLossM3Dt", "TransCum") else 1e-6
        np.testing.assert_allclose(getattr(vb, k), getattr(vc, k), rtol=RTOL, atol=atol, err_msg=str((family, name, k)))
    assert np.isfinite(vb.ChanQ).mean() >= 0.9 and np.nanmax(vb.ChanQ) > 0
    monkeypatch.setenv(SWITCH, "0")
    vs, ms = _module(r, s, cut, mask, switches)
    ms.dynamic_fused()
    assert ms.river_router.last_fused_form() in ("level blocks", "levels")
    _same(_snapshot(vs, keys), want, (family, name, "skewed"))


@pytest.mark.parametrize("family", ["shallow", "deep"])
def test_second_model_step_continues(amd, monkeypatch, family):
    """Two model steps, the second continuing from the first on both sides (nothing reset in between): the lake and
    reservoir state, TransCum, QinADDEDM3 and sumDisDay carry over, and every vector stays bit-identical."""
    r, s, cut, mask = _loop_inputs(family)
    switches = E.LOOP_OPTION_SETS["everything"]
    keys = _loop_keys(switches) + ["CrossSection2Area", "Sideflow1Chan", "LakeStorageM3", "ReservoirStorageM3"]
    monkeypatch.setenv(SWITCH, "1")
    (va, ma), (vb, mb) = _module(r, s, cut, mask, switches), _module(r, s, cut, mask, switches)
    for step in range(2):
        for sub in range(int(r["NoRoutSteps"])):
            ma.dynamic(sub)
        mb.dynamic_fused()
        assert mb.river_router.last_fused_form() == "time-major"
        _same(_snapshot(vb, keys), _snapshot(va, keys), (family, "model step %d" % step))
    first = _reference(family, "everything")
    assert not E.same_bits(va.sumDisDay, first["sumDisDay"]) and not E.same_bits(va.TransCum, first["TransCum"])


def test_chained_sites_keep_the_skew(amd, monkeypatch):
    """structures_scenario on a 60 x 80 shallow raster with 40 lakes + 60 reservoirs has site cells that drain straight
    into another site (tests/test_site_plan_cpu.py): the plan does not apply, so under LF_FUSED_TIME_MAJOR=1 the call
    succeeds on a skewed form and equals the sub-step-by-sub-step engine bit for bit (split routing, 24 sub-steps)."""
    from lisflood_amd import synthetic as syn
    H, W = 60, 80
    N = H * W
    mask = np.ones((H, W), bool)
    codes = syn.make_ldd("shallow", H, W, 8).reshape(-1).astype(np.float64)
    p = syn.router_params(N, seed=4)
    rng = np.random.default_rng(29)
    beta, dt, nsteps = p["beta"], 3600.0, 24
    alpha, length = p["alpha"], p["dx"]
    alpha2 = alpha * rng.uniform(1.2, 2.0, N)
    qlimit = 2.0 * p["Q0"] * rng.uniform(0.3, 1.2, N)
    switches = dict(E.ALL_OPTIONS)

    def module():
        from lisflood_amd import routing as R
        v = types.SimpleNamespace(
            ChanLength=length, InvChanLength=1 / length, ChannelAlpha=alpha, InvChannelAlpha=1 / alpha,
            ChannelAlpha2=alpha2, InvChannelAlpha2=1 / alpha2, QLimit=qlimit, M3Limit=alpha * length * qlimit ** beta,
            Chan2M3Start=alpha2 * length * qlimit ** beta, Chan2QStart=qlimit * 0.1, PixelArea=np.full(N, 2.5e7),
            IsChannelKinematic=np.ones(N, bool), Beta=beta, InvBeta=1 / beta, DtRouting=dt, InvDtRouting=1 / dt,
            NoRoutSteps=nsteps, InvNoRoutSteps=1 / nsteps, DtSec=dt * nsteps,
            ToChanM3RunoffDt=syn.lateral_inflow(N, 0) * length * dt)
        v.Chan2M3Kin = v.Chan2M3Start.copy()
        v.ChanM3Kin = alpha * length * p["Q0"] ** beta
        v.ChanQKin = p["Q0"].copy()
        v.Chan2QKin = (v.Chan2M3Kin / length / alpha2) ** (1 / beta)
        v.ChanQ = v.ChanQKin.copy()
        v.CrossSection2Area, v.Sideflow1Chan, v.sumDisDay = np.zeros(N), np.zeros(N), np.zeros(N)
        d, cut = syn.structures_scenario(codes, (H, W), v.ChanQ, dt, n_lakes=40, n_res=60)
        for k, x in d.items():
            setattr(v, k, np.array(x, copy=True) if isinstance(x, np.ndarray) else x)
        m = R.routing(v, options=dict(SplitRouting=True, InitLisflood=False, **switches), engine_order=True)
        m.attach_router(cut, mask)
        m.attach_structures()
        return v, m

    keys = _loop_keys(switches)
    monkeypatch.setenv(SWITCH, "1")
    (va, ma), (vb, mb) = module(), module()
    for sub in range(nsteps):
        ma.dynamic(sub)
    mb.dynamic_fused()
    assert mb.river_router.last_fused_form() in ("level blocks", "levels")
    _same(_snapshot(vb, keys), _snapshot(va, keys), "chained sites")
    assert np.nanmax(vb.QLakeOutM3Dt) > 0 and np.nanmax(vb.QResOutM3Dt) > 0


def test_one_sub_step_takes_the_skew(amd, monkeypatch):
    """NoRoutSteps = 1 on the shallow inputs: more than one sub-step is a precondition of the time-major form, so the call
    takes the skewed path even under LF_FUSED_TIME_MAJOR=1, and equals dynamic(0)."""
    r, s, cut, mask = _loop_inputs("shallow")
    r = dict(r, NoRoutSteps=1, InvNoRoutSteps=1.0, DtSec=r["DtRouting"])
    switches = E.LOOP_OPTION_SETS["everything"]
    keys = _loop_keys(switches)
    monkeypatch.setenv(SWITCH, "1")
    (va, ma), (vb, mb) = _module(r, s, cut, mask, switches), _module(r, s, cut, mask, switches)
    ma.dynamic(0)
    mb.dynamic_fused()
    assert mb.river_router.last_fused_form() in ("level blocks", "levels")
    _same(_snapshot(vb, keys), _snapshot(va, keys), "one sub-step")


def _off_level_position(m):
    """the first position of a non-empty level other than the one that holds the cell of lake 0"""
    level_start = np.asarray(m.river_router.graph.layout()[2])
    cell = int(m._st["dev"]["lake_cell"].download()[0])
    own = int(np.searchsorted(level_start, cell, side="right")) - 1
    k = next(k for k in range(level_start.size - 1) if k != own and level_start[k + 1] > level_start[k])
    return int(level_start[k])


@pytest.mark.parametrize("bad, message", [("feeder off its level", "not on its level"), ("site cell out of range", "out of range")])
def test_refused_lists_leave_the_router_usable(amd, monkeypatch, bad, message):
    """Entry 0 of the device lake_ups_idx set to a position on another level than lake 0's, or lake_cell[0] = N, and the
    site cache reset: dynamic_fused() refuses the lists with a message.  The list restored under the same pointer, without
    a reset: the next call takes the time-major form and leaves the bits of 24 x dynamic(s) in every vector of _loop_keys
    -- the refused call left nothing behind that passes for checked lists."""
    r, s, cut, mask = _loop_inputs("shallow")
    switches = E.LOOP_OPTION_SETS["everything"]
    want = _reference("shallow", "everything")
    monkeypatch.setenv(SWITCH, "1")
    vb, mb = _module(r, s, cut, mask, switches)
    dev = mb._st["dev"]["lake_ups_idx" if bad == "feeder off its level" else "lake_cell"]
    good = dev.download()
    wrong = good.copy()
    wrong[0] = _off_level_position(mb) if bad == "feeder off its level" else mb.river_router.num_pixels
    assert wrong[0] != good[0]
    dev.upload(wrong)
    amd.check(amd.lib().lf_router_reset_site_cache(mb.river_router._h))
    with pytest.raises(amd.LisfloodAmdError, match=message):
        mb.dynamic_fused()
    dev.upload(good)
    mb.dynamic_fused()
    assert mb.river_router.last_fused_form() == "time-major"
    _same(_snapshot(vb, _loop_keys(switches)), want, (bad, "after the refused call"))


def test_a_miss_between_two_hits_rebuilds_both_ways(amd, monkeypatch):
    """A good call, a call whose lake_ups_idx points at a second device array with a feeder off its level (refused), and a
    call with the pointer back at the first array, no reset in between: the third call takes the time-major form, and the
    state equals 2 x 24 x dynamic(s) on a second module bit for bit -- the refused call neither advanced nor damaged it."""
    r, s, cut, mask = _loop_inputs("shallow")
    switches = E.LOOP_OPTION_SETS["everything"]
    keys = _loop_keys(switches) + ["CrossSection2Area", "Sideflow1Chan", "LakeStorageM3", "ReservoirStorageM3"]
    monkeypatch.setenv(SWITCH, "1")
    (va, ma), (vb, mb) = _module(r, s, cut, mask, switches), _module(r, s, cut, mask, switches)
    for step in range(2):
        for sub in range(int(r["NoRoutSteps"])):
            ma.dynamic(sub)
    mb.dynamic_fused()
    assert mb.river_router.last_fused_form() == "time-major"
    good = mb._inloop.lake_ups_idx
    wrong = mb._st["dev"]["lake_ups_idx"].download()
    wrong[0] = _off_level_position(mb)
    other = amd.DeviceArray.from_host(wrong, mb.device)
    mb._inloop.lake_ups_idx = other.ptr.value
    with pytest.raises(amd.LisfloodAmdError, match="not on its level"):
        mb.dynamic_fused()
    mb._inloop.lake_ups_idx = good
    mb.dynamic_fused()
    assert mb.river_router.last_fused_form() == "time-major"
    _same(_snapshot(vb, keys), _snapshot(va, keys), "a miss between two hits")
    other.free()
