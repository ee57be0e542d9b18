"""-m gpu: an ensemble through the routing sub-step loop with lakes, reservoirs, inflow hydrographs and transmission loss in
the loop (lf_routing_substeps_fused_structures_members, k_fused_level_steps_members<.., STRUCT>).  The reference of a member is
always lf_routing_substeps_fused_structures on that member alone, bit for bit: every member is a routing module of its own
(tests/module_edges.py: loop_inputs, 120 x 160, 130 lakes + 190 reservoirs), whose device vectors -- as its own
dynamic_fused() would hand them to the library -- are copied into the member rows of the ensemble call before either runs.
Member 0 carries the unscaled inputs and also holds the oracle loop's tolerances (test_time_major_with_each_option_set)."""
import ctypes as C
import types

import numpy as np
import pytest

import module_edges as E
from test_module_edges_gpu import RTOL, _loop_keys

pytestmark = pytest.mark.gpu

SWITCH, SLICE = "LF_FUSED_TIME_MAJOR", "LF_FUSED_MEMBERS_SLICE"
SENTINEL = -1.2345678e300              # what the padding between member rows holds before and after a call
PAD = dict(dense=37, lake=3, res=5, forcing=11)
SKEWED = ("level blocks", "levels")
_inputs = {}
_oracle_runs = {}


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


def member_inputs(r, s, m):
    """member m's inputs: member 0 as they are; the others with channel state, lake / reservoir storage and forcing scaled
    (by a few per cent per member, so that every member stays in the regime of the unscaled run)"""
    if m == 0:
        return r, s
    f, g, h = 1.0 + 0.06 * m, 1.0 - 0.05 * m, 1.0 + 0.08 * m
    r, s = dict(r), dict(s)
    r["ChanQKin"] = r["ChanQKin"] * f
    r["ChanQ"] = r["ChanQKin"].copy()
    r["ChanM3Kin"] = r["ChannelAlpha"] * r["ChanLength"] * r["ChanQKin"] ** r["Beta"]
    r["ToChanM3RunoffDt"] = r["ToChanM3RunoffDt"] * h
    for k in ("LakeStorageM3", "ReservoirStorageM3"):
        s[k] = s[k] * g
    for k in ("EvaAddM3Dt", "withdrawal_CH_actual_M3_routStep", "returnflow_GwAbs2Channel_M3_routStep", "ChannelToPolderM3Dt",
              "QInM3Old"):
        s[k] = s[k] * h
    return r, s


def loop_module(r, s, cut, mask, switches, split=True):
    from lisflood_amd import routing as R
    v = E.loop_var(r, s)
    m = R.routing(v, options=dict(SplitRouting=split, InitLisflood=False, **switches), engine_order=True)
    m.attach_router(cut, mask)
    m.attach_structures()
    return m


def chained_module(state_scale=1.0):
    """the 60 x 80 scenario of test_time_major_structures_gpu.test_chained_sites_keep_the_skew: site cells that drain
    straight into another site, so the site plan does not apply"""
    from lisflood_amd import routing as R
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
    v = types.SimpleNamespace(
        ChanLength=length, InvChanLength=1 / length, ChannelAlpha=alpha, InvChannelAlpha=1 / alpha,
        ChannelAlpha2=alpha2, InvChannelAlpha2=1 / alpha2, QLimit=qlimit, M3Limit=alpha * length * qlimit ** beta,
        Chan2M3Start=alpha2 * length * qlimit ** beta, Chan2QStart=qlimit * 0.1, PixelArea=np.full(N, 2.5e7),
        IsChannelKinematic=np.ones(N, bool), Beta=beta, InvBeta=1 / beta, DtRouting=dt, InvDtRouting=1 / dt,
        NoRoutSteps=nsteps, InvNoRoutSteps=1 / nsteps, DtSec=dt * nsteps,
        ToChanM3RunoffDt=syn.lateral_inflow(N, 0) * length * dt * state_scale)
    v.Chan2M3Kin = v.Chan2M3Start.copy()
    v.ChanQKin = p["Q0"] * state_scale
    v.ChanM3Kin = alpha * length * v.ChanQKin ** beta
    v.Chan2QKin = (v.Chan2M3Kin / length / alpha2) ** (1 / beta)
    v.ChanQ = v.ChanQKin.copy()
    v.CrossSection2Area, v.Sideflow1Chan, v.sumDisDay = np.zeros(N), np.zeros(N), np.zeros(N)
    d, cut = syn.structures_scenario(codes, (H, W), p["Q0"], dt, n_lakes=40, n_res=60)
    for k, x in d.items():
        setattr(v, k, np.array(x, copy=True) if isinstance(x, np.ndarray) else x)
    for k in ("LakeStorageM3", "ReservoirStorageM3"):
        setattr(v, k, getattr(v, k) * state_scale)
    m = R.routing(v, options=dict(SplitRouting=True, InitLisflood=False, **E.ALL_OPTIONS), engine_order=True)
    m.attach_router(cut, mask)
    m.attach_structures()
    return m


def ready(m):
    """the device vectors of module m as its dynamic_fused() hands them to the library (routing._fused_with_structures)"""
    m._ensure_device()
    m._upload_state()
    m._structures_substep(0, launch=False)
    m._args.split = 1 if m._split() else 0
    return m


def single_call(amd, m):
    """lf_routing_substeps_fused_structures on module m's own device vectors"""
    amd.check(amd.lib().lf_routing_substeps_fused_structures(m.river_router._h, C.byref(m._args), C.byref(m._inloop),
                                                             int(m.var.NoRoutSteps)))
    return m.river_router.last_fused_form(), m.river_router.last_launches()["launches"]


def member_vectors(m):
    """name -> (kind, entries, the module's device array) of every per-member vector of the two argument blocks"""
    from lisflood_amd import routing as R
    st, N = m._st, m.river_router.num_pixels
    out = {k: ("dense", N, m._dev[k]) for k in R._STATE + R._OUT + ["SideflowChanM3"]}
    for k in R._INLOOP_DENSE[:-1]:
        if k in st["dev"]:
            out[k] = ("dense", N, st["dev"][k])
    for kind, names, count in (("lake", R._LAKE_STATE, st["lakes"]), ("res", R._RES_STATE, st["res"])):
        for k in names if count else ():
            out[k] = (kind, count, st["dev"][k])
    for k in ("ToChanM3RunoffDt", "EvaAddM3Dt", "WUseAddM3Dt", "ChannelToPolderM3Dt", "QInM3Old", "QDelta"):
        if getattr(m._inloop, k):
            out[k] = ("forcing", N, st["dev"][k])
    return out


class Packed:
    """The member rows of an ensemble call, filled from the member modules' device vectors (after ready()), with padding
    between the rows that holds SENTINEL; the call runs on the router, statics and site lists of mods[0]."""

    def __init__(self, amd, mods, shared_forcing=False):
        from lisflood_amd import routing as R
        self.amd, self.mods, self.M = amd, mods, len(mods)
        self.names = member_vectors(mods[0])
        st = mods[0]._st
        self.count = dict(dense=mods[0].river_router.num_pixels, lake=st["lakes"], res=st["res"])
        self.count["forcing"] = self.count["dense"]
        self.stride = {k: n + PAD[k] for k, n in self.count.items()}
        self.dev, self.before = {}, {}
        for k, (kind, n, _) in self.names.items():
            rows = np.full((self.M, self.stride[kind]), SENTINEL)
            for i, m in enumerate(mods):
                rows[i, :n] = member_vectors(m)[k][2].download()[:n]
            if kind == "forcing" and shared_forcing:
                rows[1:, :n] = np.nan                  # never read: every member takes member 0's rows
            self.before[k] = rows
            self.dev[k] = amd.DeviceArray.from_host(rows.reshape(-1), mods[0].device)
        self.args = R._SubstepArgs.from_buffer_copy(mods[0]._args)
        self.inloop = R._InloopArgs.from_buffer_copy(mods[0]._inloop)
        for k, (kind, _, _) in self.names.items():
            block = self.args if k in R._STATE + R._OUT else self.inloop
            setattr(block, k, self.dev[k].ptr.value)
        self.args.SideflowChanM3 = self.inloop.SideflowChanM3
        self.inloop.ChanQ = self.args.ChanQ
        self.forcing_stride = 0 if shared_forcing else self.stride["forcing"]

    def call(self, members=None, **strides):
        kw = dict(member_stride=self.stride["dense"], lake_member_stride=self.stride["lake"],
                  res_member_stride=self.stride["res"], forcing_member_stride=self.forcing_stride)
        kw.update(strides)
        r = self.mods[0].river_router
        r.routing_substeps_structures_members(self.args, self.inloop, int(self.mods[0].var.NoRoutSteps),
                                              self.M if members is None else members, **kw)
        return r.last_fused_form(), r.last_launches()["launches"]

    def rows(self, k):
        kind, n, _ = self.names[k]
        return self.dev[k].download().reshape(self.M, self.stride[kind])

    def check(self, what, members=None):
        """every per-member vector of member m equals module m's own (after its single call), the forcing rows and all
        padding are as they were"""
        for k, (kind, n, _) in self.names.items():
            rows = self.rows(k)
            assert E.same_bits(rows[:, n:], self.before[k][:, n:]), "%s %s: the padding changed" % (what, k)
            for i in range(self.M) if members is None else members:
                want = self.before[k][i, :n] if kind == "forcing" else member_vectors(self.mods[i])[k][2].download()[:n]
                assert E.same_bits(rows[i, :n], want), "%s member %d %s: %s" % (what, i, k, E.first_difference(rows[i, :n], want))

    def free(self):
        for d in self.dev.values():
            d.free()


def members_of(family, switches, M, split=True, same_forcing=False):
    r, s, cut, mask = _loop_inputs(family)
    mods = []
    for i in range(M):
        ri, si = member_inputs(r, s, i)
        if same_forcing:
            ri, si = dict(ri, ToChanM3RunoffDt=r["ToChanM3RunoffDt"]), dict(si, **{k: s[k] for k in (
                "EvaAddM3Dt", "withdrawal_CH_actual_M3_routStep", "returnflow_GwAbs2Channel_M3_routStep",
                "ChannelToPolderM3Dt", "QInM3Old")})
        mods.append(ready(loop_module(ri, si, cut, mask, switches, split)))
    return mods


def stays_finite(m):
    """the condition on a member's own single call: at least nine cells in ten finite"""
    q = m._dev["ChanQ"].download()[:m.river_router.num_pixels]
    return np.isfinite(q).mean() >= 0.9 and np.nanmax(q) > 0


def oracle_run(orc, name, split):
    """the shallow model step by the oracle alone (module_edges.loop_oracle_run; single routing: the same loop, unsplit)"""
    if split:
        return E.loop_oracle_run(orc, "shallow", name)[0]
    if name not in _oracle_runs:
        r, s, cut, mask = _loop_inputs("shallow")
        v = E.loop_var(r, s)
        kw = orc.kinematicWave(cut, mask, r["ChannelAlpha"], r["Beta"], r["ChanLength"], r["DtRouting"])
        st, sub = orc.InloopStructures(v, E.LOOP_OPTION_SETS[name]), orc.RoutingSubstep(kw, v)
        for step in range(int(v.NoRoutSteps)):
            st.dynamic_inloop(step)
            sub.dynamic(split=False, sideflow_m3=v.SideflowChanM3)
        _oracle_runs[name] = v
    return _oracle_runs[name]


@pytest.mark.parametrize("solver", ["quintic", "general_pow"])
@pytest.mark.parametrize("split", [True, False], ids=["split", "single"])
@pytest.mark.parametrize("name", list(E.LOOP_OPTION_SETS))
def test_every_row_as_alone(amd, oracle, monkeypatch, name, split, solver):
    """shallow under LF_FUSED_TIME_MAJOR=1: five members, member_stride = N + 37, site strides n_lakes + 3 / n_res + 5, the
    padding filled with a sentinel; the members differ in channel state, lake / reservoir storage and forcing.  The call
    takes the time-major form in no more launches than one single call; every per-member vector of both argument blocks
    (a superset of _loop_keys plus the site state) equals the member's own single call bit for bit and the padding keeps
    its sentinel; `everything` runs a second model step on top.  Member 0 also holds the oracle tolerances."""
    if solver == "general_pow":
        monkeypatch.setenv("LF_GENERAL_POW", "1")
    else:
        monkeypatch.delenv("LF_GENERAL_POW", raising=False)
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.delenv(SLICE, raising=False)
    switches = E.LOOP_OPTION_SETS[name]
    mods = members_of("shallow", switches, 5, split)
    P = Packed(amd, mods)
    for step in range(2 if name == "everything" else 1):
        form, launches = P.call()
        singles = [single_call(amd, m) for m in mods]
        print("%s %s %s step %d: %s in %d launches, a single call: %s in %d" % ((name, split, solver, step, form, launches) + singles[0]))
        assert form == "time-major" and all(f == "time-major" for f, _ in singles)
        assert launches <= singles[0][1]
        assert all(stays_finite(m) for m in mods)
        P.check((name, split, solver, "model step %d" % step))
        if step == 0:
            r = _loop_inputs("shallow")[0]
            vc = oracle_run(oracle, name, split)
            cancel = 256 * np.finfo(float).eps * float(np.nanmax(vc.ChanQ)) * r["DtRouting"]
            for k in _loop_keys(switches):
                got = P.rows(k)[0, :P.names[k][1]]
                if P.names[k][0] == "dense":
                    got = mods[0]._down(got)
                atol = cancel * (int(r["NoRoutSteps"]) if k == "TransCum" else 1) if k in ("TransLossM3Dt", "TransCum") else 1e-6
                np.testing.assert_allclose(got, getattr(vc, k), rtol=RTOL, atol=atol, err_msg=str((name, split, solver, k)))
    P.free()


def test_slices(amd, monkeypatch):
    """LF_FUSED_MEMBERS_SLICE=2 on five members: three slices, so three times the level and site launches of the unsliced
    call, and the same bits"""
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.delenv(SLICE, raising=False)
    switches = E.LOOP_OPTION_SETS["everything"]
    whole = Packed(amd, members_of("shallow", switches, 5))
    form, launches = whole.call()
    assert form == "time-major"
    monkeypatch.setenv(SLICE, "2")
    mods = members_of("shallow", switches, 5)
    P = Packed(amd, mods)
    form2, launches2 = P.call()
    assert form2 == "time-major" and launches2 == 3 * launches
    for m in mods:
        single_call(amd, m)
    P.check("slices of two")
    for k in P.names:
        assert E.same_bits(P.rows(k), whole.rows(k)), k
    whole.free()
    P.free()


def _site_levels(m):
    level_start = m.river_router.graph.layout()[2]
    cells = np.concatenate([np.asarray(m.var.LakeIndex), np.asarray(m.var.ReservoirIndex)]).astype(np.int64)
    return np.unique(np.searchsorted(level_start, m._pos[cells], side="right") - 1).size


def test_deep_graph_when_forced(amd, monkeypatch):
    """deep (118 levels, 110 of them with sites) under LF_FUSED_TIME_MAJOR=1: the member form, one launch per level and one
    more on every level that holds a site, and the bits of the single calls"""
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.delenv(SLICE, raising=False)
    mods = members_of("deep", E.LOOP_OPTION_SETS["everything"], 3)
    P = Packed(amd, mods)
    form, launches = P.call()
    nl, site_levels = mods[0].river_router.graph.num_levels, _site_levels(mods[0])
    assert form == "time-major" and site_levels == 110 and launches == nl + site_levels
    for m in mods:
        single_call(amd, m)
    P.check("deep, forced")
    P.free()


@pytest.mark.parametrize("case", ["deep_by_default", "shallow_switched_off", "chained_sites"])
def test_fallbacks_run_member_after_member(amd, monkeypatch, case):
    """deep with the switch unset, shallow with LF_FUSED_TIME_MAJOR=0, and the chained-site scenario under =1: the members
    run one after the other on a skewed form -- as many launches as the single calls together, less the flag passes that
    run once -- and leave the bits of their single calls"""
    monkeypatch.delenv(SLICE, raising=False)
    if case == "deep_by_default":
        monkeypatch.delenv(SWITCH, raising=False)
        mods = members_of("deep", E.LOOP_OPTION_SETS["everything"], 3)
    elif case == "shallow_switched_off":
        monkeypatch.setenv(SWITCH, "0")
        mods = members_of("shallow", E.LOOP_OPTION_SETS["everything"], 3)
    else:
        monkeypatch.setenv(SWITCH, "1")
        mods = [ready(chained_module(1.0 + 0.05 * i)) for i in range(3)]
    P = Packed(amd, mods)
    form, launches = P.call()
    singles = [single_call(amd, m) for m in mods]
    print(case, form, launches, singles)
    assert form in SKEWED and all(f in SKEWED for f, _ in singles)
    assert launches <= sum(n for _, n in singles) and launches >= sum(n for _, n in singles) - 2 * (len(mods) - 1)
    P.check(case)
    q = P.rows("QLakeOutM3Dt")
    assert np.nanmax(q[:, :P.count["dense"]]) > 0
    P.free()


def test_members_do_not_see_each_other(amd, monkeypatch):
    """Member 1's runoff is NaN at the cells that feed lake 0: its lake turns NaN; members 0 and 2 equal their single calls
    and are finite wherever those are -- every member has a feed buffer of its own."""
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.delenv(SLICE, raising=False)
    r, s, cut, mask = _loop_inputs("shallow")
    lake = 2                                                        # (lakes 0 / 1 may be the planted NaN sites)
    feeders = np.nonzero(s["downstruct"] == s["LakeIndex"][lake])[0]
    assert feeders.size > 0
    mods = []
    for i in range(3):
        ri, si = member_inputs(r, s, i)
        if i == 1:
            ri = dict(ri, ToChanM3RunoffDt=ri["ToChanM3RunoffDt"].copy())
            ri["ToChanM3RunoffDt"][feeders] = np.nan
        mods.append(ready(loop_module(ri, si, cut, mask, E.LOOP_OPTION_SETS["everything"])))
    P = Packed(amd, mods)
    form, _ = P.call()
    assert form == "time-major"
    for m in mods:
        single_call(amd, m)
    P.check("isolation")
    storage = P.rows("LakeStorageM3CC")
    inflow = P.rows("LakeInflowCC")
    assert np.isnan(inflow[1, lake]) and np.isfinite(inflow[[0, 2], lake]).all() and np.isfinite(storage[[0, 2], lake]).all()
    for k in ("ChanQ", "LakeInflowCC", "LakeStorageM3CC"):
        for i in (0, 2):
            n = P.names[k][1]
            alone = member_vectors(mods[i])[k][2].download()[:n]
            assert (np.isfinite(P.rows(k)[i, :n]) == np.isfinite(alone)).all()
    P.free()


def test_shared_forcing_rows(amd, monkeypatch):
    """forcing_member_stride = 0: every member reads member 0's forcing rows; the rows of the other members hold NaN and
    are never read"""
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.delenv(SLICE, raising=False)
    mods = members_of("shallow", E.LOOP_OPTION_SETS["everything"], 3, same_forcing=True)
    P = Packed(amd, mods, shared_forcing=True)
    form, _ = P.call()
    assert form == "time-major"
    for m in mods:
        single_call(amd, m)
    assert all(stays_finite(m) for m in mods)
    P.check("shared forcing")
    P.free()


def test_one_member_is_the_single_call(amd, monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    mods = members_of("shallow", E.LOOP_OPTION_SETS["everything"], 1)
    P = Packed(amd, mods)
    got = P.call(members=1)
    assert got == single_call(amd, mods[0]) and got[0] == "time-major"
    P.check("one member")
    P.free()


def test_refusals_leave_the_router_usable(amd, monkeypatch):
    """strides below a row's length, and a forcing stride strictly between 0 and N, are refused with a message naming the
    argument; nothing has advanced, and the next good call takes the time-major form and leaves the right bits"""
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.delenv(SLICE, raising=False)
    mods = members_of("shallow", E.LOOP_OPTION_SETS["everything"], 3)
    P = Packed(amd, mods)
    N, nl, nr = P.count["dense"], P.count["lake"], P.count["res"]
    for bad, message in ((dict(member_stride=N - 1), "member_stride"), (dict(lake_member_stride=nl - 1), "lake_member_stride"),
                         (dict(res_member_stride=nr - 1), "res_member_stride"), (dict(forcing_member_stride=N - 1), "forcing_member_stride"),
                         (dict(forcing_member_stride=1), "forcing_member_stride")):
        with pytest.raises(amd.LisfloodAmdError, match=message):
            P.call(**bad)
    for k in P.names:
        assert E.same_bits(P.rows(k), P.before[k]), k
    form, _ = P.call()
    assert form == "time-major"
    for m in mods:
        single_call(amd, m)
    P.check("after the refused calls")
    P.free()


def test_ensemble_of_a_module(amd, monkeypatch):
    """routing.ensemble(3) after attach_structures: members set through set_state and a forcing dict of mixed shapes, two
    model steps; every member equals a fresh module's dynamic_fused() on its inputs, site state carried over."""
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.delenv(SLICE, raising=False)
    r, s, cut, mask = _loop_inputs("shallow")
    switches = E.LOOP_OPTION_SETS["everything"]
    M = 3
    inputs = [member_inputs(r, s, i) for i in range(M)]
    base = loop_module(r, s, cut, mask, switches)
    ens = base.ensemble(M)
    for k in ("ChanQKin", "ChanQ", "ChanM3Kin"):
        ens.set_state(k, np.stack([ri[k] for ri, _ in inputs]))
    ens.set_state("LakeStorageM3CC", np.stack([si["LakeStorageM3"][s["LakeIndex"]] for _, si in inputs]))
    ens.set_state("ReservoirStorageM3CC", np.stack([si["ReservoirStorageM3"][s["ReservoirIndex"]] for _, si in inputs]))
    wuse = lambda si: si["withdrawal_CH_actual_M3_routStep"] - si["returnflow_GwAbs2Channel_M3_routStep"]
    forcing = dict(ToChanM3RunoffDt=np.stack([ri["ToChanM3RunoffDt"] for ri, _ in inputs]),
                   EvaAddM3Dt=np.stack([si["EvaAddM3Dt"] for _, si in inputs]), WUseAddM3Dt=np.stack([wuse(si) for _, si in inputs]),
                   ChannelToPolderM3Dt=np.stack([si["ChannelToPolderM3Dt"] for _, si in inputs]),
                   QInM3Old=np.stack([si["QInM3Old"] for _, si in inputs]), QDelta=s["QDelta"])      # QDelta: one row for all
    alone = [loop_module(ri, si, cut, mask, switches) for ri, si in inputs]
    keys = _loop_keys(switches) + ["CrossSection2Area", "Sideflow1Chan", "FlowVelocity", "TravelDistance", "SideflowChanM3"]
    for step in range(2):
        ens.dynamic_fused(forcing)
        assert ens.last_fused_form() == "time-major"
        for i, m in enumerate(alone):
            m.var.sumDisDay = np.zeros(m._nfull)           # the ensemble zeroes it at the start of a model step
            m.dynamic_fused()
            for k in keys:
                got, want = ens.state(k)[i], np.asarray(getattr(m.var, k))
                assert E.same_bits(got, want), "model step %d member %d %s: %s" % (step, i, k, E.first_difference(got, want))
    with pytest.raises(ValueError, match="no state or output vector"):
        ens.state("Discharge")
    with pytest.raises(ValueError, match=r"float64 \[3, 130\] array"):
        ens.set_state("LakeOutflowCC", np.zeros((3, 131)))
    ens.free()
