"""An ensemble through the sub-step loop of a model step (lf_routing_substeps_fused_members / routingEnsemble): M members
that share the LDD and every static vector go through the time-major level kernel as a second grid dimension
(k_fused_level_steps_members), slice by slice; where that form does not apply they run one after the other through the
single call's schedule.  Either way every member must be bit-identical to lf_routing_substeps_fused on that member alone,
on the same router (bench_support.RoutingStepDevice: the single call is itself pinned to the reference's fixtures)."""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12
SENTINEL = -777.25      # padding between the member rows: neither read nor written
H = W = 160
N = H * W
M, PAD, NSTEPS, ZERO_MEMBER = 5, 37, 9, 3


@pytest.fixture(scope="module")
def amd():
    import types
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    from lisflood_amd import kinematic_wave_parallel, routing
    return types.SimpleNamespace(kw=kinematic_wave_parallel, routing=routing, lib=_lib)


@pytest.fixture(params=["fused_beta_3_5", "general_pow"])
def solver(request, monkeypatch):
    """both arithmetic paths, chosen when the router is created: ALL35 (beta = 3/5 known on the host) and the run-time
    path with OCML pow (LF_GENERAL_POW=1)"""
    if request.param == "general_pow":
        monkeypatch.setenv("LF_GENERAL_POW", "1")
    else:
        monkeypatch.delenv("LF_GENERAL_POW", raising=False)
    return request.param


# ---- the 160 x 160 graphs, their statics and the members' states ------------------------------------------------------
_cases = {}


def case(family):
    """family -> (ldd raster, router parameters, model-step values, dt); worked out once and left unchanged"""
    from lisflood_amd import synthetic as syn
    if family not in _cases:
        codes = syn.make_ldd(family, H, W, 5)
        p = syn.router_params(N)
        vals, dt = syn.model_step_values(N, p)
        for a in vals.values():
            a.setflags(write=False)
        _cases[family] = (codes, p, vals, dt)
    return _cases[family]


def make_router(amd, codes, p, vals, dt):
    g = amd.kw.Graph(ldd_raster=codes)
    return amd.kw.kinematicWave(None, None, p["alpha"], p["beta"], p["dx"], dt, graph=g, alpha_floodplains=vals["ChannelAlpha2"])


def member_states(vals, beta, members, zero_member=None, chan=None):
    """member m: the discharge of the model-step values times 1 + 0.25 m with the volume that goes with it, ChanQ equal to
    the discharge and m in its discharge sum; `zero_member`: every state vector zero; chan: pixels outside it hold no water"""
    from lisflood_amd.routing import _STATE
    out = []
    for m in range(members):
        q = vals["ChanQKin"] * (1 + 0.25 * m)
        if chan is not None:
            q = np.where(chan, q, 0.0)
        st = dict(ChanQKin=q, ChanM3Kin=vals["ChannelAlpha"] * vals["ChanLength"] * q ** beta, Chan2QKin=vals["Chan2QKin"].copy(),
                  Chan2M3Kin=vals["Chan2M3Kin"].copy(), CrossSection2Area=np.zeros(N), Sideflow1Chan=np.zeros(N), ChanQ=q.copy(),
                  sumDisDay=np.full(N, float(m)))
        if m == zero_member:
            st = {k: np.zeros(N) for k in _STATE}
        out.append(st)
    return out


def member_sideflows(vals, dt, members, nsteps, per_substep, zero_member=None):
    """[M, N] (one vector per member) or [M, nsteps, N] sideflow volumes in pixel order"""
    from lisflood_amd import synthetic as syn
    if per_substep:
        side = np.stack([[syn.lateral_inflow(N, 300 + 10 * m + s) * vals["ChanLength"] * dt for s in range(nsteps)]
                         for m in range(members)])
    else:
        side = np.stack([vals["SideflowChanM3"] * (1 + 0.1 * m) for m in range(members)])
    if zero_member is not None:
        side[zero_member] = 0.0
    return side


def alone(kw, vals, state, side, split, beta, dt, nsteps, model_steps=1):
    """one member through lf_routing_substeps_fused on `kw` -> (name -> [N] in engine order, launch statistics, form)"""
    from bench_support import RoutingStepDevice
    from lisflood_amd.routing import _OUT, _STATE
    v = dict(vals)
    v.update(state)
    if side.ndim == 1:
        v["SideflowChanM3"] = side
    r = RoutingStepDevice(kw, v, split, beta, 1.0 / dt, dt * nsteps)
    for _ in range(model_steps):
        if side.ndim == 1:
            r.run_fused(nsteps)
        else:
            r.run_fused_sideflow_per_substep(list(side))
    out = {k: r.dev[k].download() for k in _STATE + _OUT}
    st, form = kw.last_launches(), kw.last_fused_form()
    r.free()
    return out, st, form


def together(amd, kw, vals, states, side, split, beta, dt, nsteps, stride, model_steps=1, side_member_stride=None):
    """all members in one lf_routing_substeps_fused_members call per model step -> (name -> [M, stride] rows as the device
    holds them afterwards, the sideflow rows afterwards, launch statistics, form).  side: [M, N] or [M, nsteps, N]; rows
    and sideflow rows are padded with the sentinel.  side_member_stride = 0: the call is told to share member 0's."""
    from lisflood_amd.routing import _OUT, _STATE, _STATIC, SubstepVectors, substep_host_vectors
    members = len(states)
    perm = kw.graph.layout()[0].astype(np.int64)
    per_member = side[0].size                      # N, or nsteps * N
    srows = np.full((members, per_member + PAD), SENTINEL)
    srows[:, :per_member] = side[..., perm].reshape(members, per_member)
    host = substep_host_vectors(vals, N, perm, _STATIC)
    sv = SubstepVectors(host, N, beta, 1.0 / dt, dt * nsteps, split, True, sideflow=srows,
                        lengths={k: members * stride for k in _STATE + _OUT})
    for k in _STATE + _OUT:
        rows = np.full((members, stride), SENTINEL)
        rows[:, :N] = np.stack([s[k][perm] if k in s else np.zeros(N) for s in states])
        sv.upload(k, rows.reshape(-1))
    sms = per_member + PAD if side_member_stride is None else side_member_stride
    for _ in range(model_steps):
        kw.routing_substeps_members(sv.args, nsteps, members, stride, N if side.ndim == 3 else 0, sms)
    out = {k: sv.download(k).reshape(members, stride) for k in _STATE + _OUT}
    side_after = sv.download("SideflowChanM3").reshape(members, per_member + PAD)
    st, form = kw.last_launches(), kw.last_fused_form()
    assert np.array_equal(side_after, srows, equal_nan=True)                           # sideflow rows and their padding: untouched
    sv.free()
    return out, st, form


def assert_rows_as_alone(got, want, stride, members=None):
    """every state and output row equals the member's own call, bit for bit, and the padding keeps its sentinel"""
    for k, rows in got.items():
        for m in range(rows.shape[0]) if members is None else members:
            assert np.array_equal(rows[m, :N], want[m][k], equal_nan=True), (k, m)
        assert (rows[:, N:] == SENTINEL).all(), k


@pytest.mark.parametrize("per_substep", [False, True], ids=["sideflow_stride_0", "sideflow_stride_N"])
@pytest.mark.parametrize("split", [True, False], ids=["split", "single"])
def test_every_row_as_alone(amd, solver, monkeypatch, split, per_substep):
    """shallow, M = 5, member_stride = N + 37, nsteps = 9, two consecutive model steps, one all-zero member: every state and
    output vector of every member equals the member's own single call, the padding of every row keeps its sentinel, and the
    member kernel ran.  The zero member stays exactly zero in single routing; under split routing its main channel does
    (the shared statics give every member's floodplain its threshold volume Chan2M3Start and the inflow Chan2QStart, so
    those vectors are its single call's, not zero)."""
    monkeypatch.setenv("LF_FUSED_TIME_MAJOR", "1")
    codes, p, vals, dt = case("shallow")
    kw = make_router(amd, codes, p, vals, dt)
    states = member_states(vals, p["beta"], M, ZERO_MEMBER)
    side = member_sideflows(vals, dt, M, NSTEPS, per_substep, ZERO_MEMBER)
    want = [alone(kw, vals, states[m], side[m], split, p["beta"], dt, NSTEPS, model_steps=2)[0] for m in range(M)]
    assert kw.last_fused_form() == "time-major"
    got, st, form = together(amd, kw, vals, states, side, split, p["beta"], dt, NSTEPS, N + PAD, model_steps=2)
    assert form == "time-major"
    assert_rows_as_alone(got, want, N + PAD)
    moved = sum(not np.array_equal(got[k][0, :N], states[0][k][kw.graph.layout()[0]]) for k in ("ChanQKin", "ChanM3Kin", "sumDisDay"))
    assert moved == 3                                                      # (the call did something)
    zero_names = ["ChanQKin", "ChanM3Kin", "Sideflow1Chan"] if split else list(got)
    for k in zero_names:
        assert (got[k][ZERO_MEMBER, :N] == 0.0).all(), k
    kw.close()


def test_slices(amd, solver, monkeypatch):
    """LF_FUSED_MEMBERS_SLICE=2: slices of 2, 2 and 1 members, the same bits; the level launches are three times those of
    the unsliced call, the flag passes counted once"""
    monkeypatch.setenv("LF_FUSED_TIME_MAJOR", "1")
    monkeypatch.delenv("LF_FUSED_MEMBERS_SLICE", raising=False)
    codes, p, vals, dt = case("shallow")
    kw = make_router(amd, codes, p, vals, dt)
    states = member_states(vals, p["beta"], M, ZERO_MEMBER)
    side = member_sideflows(vals, dt, M, NSTEPS, False, ZERO_MEMBER)
    want, one = [], None
    for m in range(M):
        w, one, _ = alone(kw, vals, states[m], side[m], True, p["beta"], dt, NSTEPS)
        want.append(w)
    levels = kw.graph.num_levels
    flags = one["launches"] - levels                                       # the single call: flag passes + one launch per level
    assert 0 <= flags <= 2
    got, whole, form = together(amd, kw, vals, states, side, True, p["beta"], dt, NSTEPS, N + PAD)
    assert form == "time-major" and whole["launches"] == one["launches"]
    assert_rows_as_alone(got, want, N + PAD)
    monkeypatch.setenv("LF_FUSED_MEMBERS_SLICE", "2")
    got, sliced, form = together(amd, kw, vals, states, side, True, p["beta"], dt, NSTEPS, N + PAD)
    assert form == "time-major"
    assert_rows_as_alone(got, want, N + PAD)
    assert sliced["launches"] - flags == 3 * (whole["launches"] - flags), (one, whole, sliced)
    kw.close()


def test_shared_sideflow(amd, solver, monkeypatch):
    """sideflow_member_stride = 0: every member reads member 0's sideflow (the other rows hold NaN and are never read)"""
    monkeypatch.setenv("LF_FUSED_TIME_MAJOR", "1")
    codes, p, vals, dt = case("shallow")
    kw = make_router(amd, codes, p, vals, dt)
    states = member_states(vals, p["beta"], 3)
    for per_substep in (False, True):
        side = member_sideflows(vals, dt, 3, NSTEPS, per_substep)
        want = [alone(kw, vals, states[m], side[0], True, p["beta"], dt, NSTEPS)[0] for m in range(3)]
        side[1:] = np.nan
        got, _, form = together(amd, kw, vals, states, side, True, p["beta"], dt, NSTEPS, N + PAD, side_member_stride=0)
        assert form == "time-major"
        assert_rows_as_alone(got, want, N + PAD)
        assert all(np.isfinite(rows[:, :N]).all() for rows in got.values())
    kw.close()


def test_inert_pixels(amd, solver, monkeypatch):
    """the 80 %-channel lddmask domain of test_inert_pixels_leave_the_same_sums_in_both_fused_forms at 160 x 160, one model
    step per call (the entry point carries no msteps): the non-channel pixels are isolated and hold no water, so the kernel
    jumps them to the last sub-step.  The sums are preloaded with -0.0 and positive values; every member's sums -- and
    everything else -- must have the bits of its single call."""
    from lisflood_amd import ldd as L
    from lisflood_amd.kinematic_wave_parallel import kinematicWave
    monkeypatch.setenv("LF_FUSED_TIME_MAJOR", "1")
    codes, p, vals, dt = case("shallow")
    mask = np.ones((H, W), bool)
    rng = np.random.default_rng(23)
    is_chan = rng.random(N) < 0.8
    kin, _ = L.lddmask(codes.reshape(-1).astype(np.float64), mask, is_chan)
    ldd_kin = np.zeros(N)
    ldd_kin[is_chan] = kin
    # (a non-channel pixel is inert only with zero thresholds: they follow the masked discharge, as in that test)
    beta, alpha, alpha2, length = p["beta"], vals["ChannelAlpha"], vals["ChannelAlpha2"], vals["ChanLength"]
    qlimit = np.where(is_chan, vals["QLimit"], 0.0)
    v = dict(vals, IsChannelKinematic=is_chan, QLimit=qlimit, M3Limit=alpha * length * qlimit ** beta,
             Chan2M3Start=alpha2 * length * qlimit ** beta, Chan2QStart=qlimit * 0.1)
    v["Chan2M3Kin"] = v["Chan2M3Start"].copy()
    v["Chan2QKin"] = (v["Chan2M3Kin"] / length / alpha2) ** (1 / beta)
    kw = kinematicWave(ldd_kin, mask, p["alpha"], p["beta"], p["dx"], dt, alpha_floodplains=vals["ChannelAlpha2"])
    states = member_states(v, p["beta"], 3, chan=is_chan)
    for m, st in enumerate(states):
        sums = np.zeros(N)
        sums[m::3] = -0.0
        sums[(m + 1) % 3::3] = rng.uniform(1.0, 9.0, sums[(m + 1) % 3::3].size)
        st["sumDisDay"] = sums
    side = member_sideflows(v, dt, 3, NSTEPS, False)
    want = [alone(kw, v, states[m], side[m], True, p["beta"], dt, NSTEPS)[0] for m in range(3)]
    got, _, form = together(amd, kw, v, states, side, True, p["beta"], dt, NSTEPS, N + PAD)
    assert form == "time-major"
    perm = kw.graph.layout()[0]
    inert = ~is_chan[perm]
    assert inert.sum() > N // 10
    for m in range(3):
        for k in got:
            same = got[k][m, :N].view(np.int64) == want[m][k].view(np.int64)            # bits: +0.0 and -0.0 differ
            assert same.all(), (k, m, np.argwhere(~same)[:5])
        sums = got["sumDisDay"][m, :N][inert]
        assert (sums == states[m]["sumDisDay"][perm][inert]).all() and not np.signbit(sums).any()   # -0.0 + 0.0 = +0.0
    kw.close()


def test_members_do_not_leak_into_each_other(amd, solver, monkeypatch):
    """member 1's sideflow is NaN at twenty source cells: members 0 and 2 equal their single calls and are finite, member 1
    is NaN exactly where its single call is"""
    monkeypatch.setenv("LF_FUSED_TIME_MAJOR", "1")
    codes, p, vals, dt = case("shallow")
    kw = make_router(amd, codes, p, vals, dt)
    perm, ups_ptr, _ = kw.graph.layout()
    sources = np.flatnonzero(np.diff(ups_ptr) == 0)
    assert sources.size >= 20
    states = member_states(vals, p["beta"], 3)
    side = member_sideflows(vals, dt, 3, NSTEPS, False)
    side[1, perm[sources[:: sources.size // 20][:20]]] = np.nan
    want = [alone(kw, vals, states[m], side[m], True, p["beta"], dt, NSTEPS)[0] for m in range(3)]
    got, _, form = together(amd, kw, vals, states, side, True, p["beta"], dt, NSTEPS, N + PAD)
    assert form == "time-major"
    assert_rows_as_alone(got, want, N + PAD)
    for k, rows in got.items():
        assert np.isfinite(rows[0, :N]).all() and np.isfinite(rows[2, :N]).all(), k
        assert np.array_equal(np.isnan(rows[1, :N]), np.isnan(want[1][k])), k
    assert np.isnan(want[1]["ChanQKin"]).sum() >= 20
    kw.close()


@pytest.mark.parametrize("family, env", [("deep", None), ("shallow", "0")], ids=["deep_env_unset", "shallow_time_major_0"])
def test_fallback_runs_the_members_one_after_the_other(amd, solver, monkeypatch, family, env):
    """where the time-major form does not apply the members go through the single call's schedule one by one: the same
    bits, and M times the single call's launches, the flag passes aside (they run once)"""
    codes, p, vals, dt = case(family)
    kw = make_router(amd, codes, p, vals, dt)
    states = member_states(vals, p["beta"], 3)
    side = member_sideflows(vals, dt, 3, NSTEPS, False)
    # the flag passes of a call on this router: what a forced time-major call launches beyond one launch per level
    monkeypatch.setenv("LF_FUSED_TIME_MAJOR", "1")
    _, tm, form = alone(kw, vals, states[0], side[0], True, p["beta"], dt, NSTEPS)
    assert form == "time-major"
    flags = tm["launches"] - kw.graph.num_levels
    assert 0 <= flags <= 2
    if env is None:
        monkeypatch.delenv("LF_FUSED_TIME_MAJOR")
    else:
        monkeypatch.setenv("LF_FUSED_TIME_MAJOR", env)
    want, one = [], None
    for m in range(3):
        w, one, form = alone(kw, vals, states[m], side[m], True, p["beta"], dt, NSTEPS)
        assert form in ("level blocks", "levels")
        want.append(w)
    got, many, form = together(amd, kw, vals, states, side, True, p["beta"], dt, NSTEPS, N + PAD)
    assert form in ("level blocks", "levels")
    assert_rows_as_alone(got, want, N + PAD)
    assert many["launches"] - flags == 3 * (one["launches"] - flags), (flags, one, many)
    kw.close()


def test_one_member_is_the_single_call(amd, solver, monkeypatch):
    monkeypatch.setenv("LF_FUSED_TIME_MAJOR", "1")
    codes, p, vals, dt = case("shallow")
    kw = make_router(amd, codes, p, vals, dt)
    states = member_states(vals, p["beta"], 1)
    side = member_sideflows(vals, dt, 1, NSTEPS, True)
    want, one, _ = alone(kw, vals, states[0], side[0], True, p["beta"], dt, NSTEPS)
    got, st, form = together(amd, kw, vals, states, side, True, p["beta"], dt, NSTEPS, N + PAD)
    assert form == "time-major" and st == one
    assert_rows_as_alone(got, [want], N + PAD)
    kw.close()


@pytest.mark.parametrize("mode", ["split", "single"])
def test_ensemble_against_the_references_own_numbers(amd, solver, mode):
    """the substep_split / substep_single fixtures through routingEnsemble: member 0 carries the fixture's state, members 1
    and 2 carry it scaled by 0.5 and 2, the fixture's sideflows go to every member.  Member 0 must reproduce the
    reference-captured end state (the tolerances of test_routing_substeps_fused_wavefront), members 1 and 2 their own
    routing.dynamic_fused bit for bit."""
    g = golden("substep_" + mode)
    split = mode == "split"
    n = int(g["NoRoutSteps"])
    scales = (1.0, 0.5, 2.0)
    state_names = ("ChanQKin", "ChanM3Kin", "Chan2QKin", "Chan2M3Kin", "CrossSection2Area", "Sideflow1Chan", "ChanQ")

    def scaled(scale):
        v = amd.routing.var_from_fixture(g)
        for k in state_names:
            setattr(v, k, getattr(v, k) * scale)
        return v
    v0 = scaled(1.0)
    mod = amd.routing.routing(v0, split_routing=split)
    mod.attach_router(g["codes"], g["mask"])
    ens = amd.routing.routingEnsemble(v0, mod.river_router, 3, split_routing=split)
    for k in state_names:
        ens.set_state(k, np.stack([getattr(scaled(s), k) for s in scales]))
        assert np.array_equal(ens.state(k), np.stack([getattr(scaled(s), k) for s in scales]))
    ens.dynamic_fused(np.ascontiguousarray(np.broadcast_to(g["ToChanM3RunoffDt"], (3,) + g["ToChanM3RunoffDt"].shape)))
    assert ens.last_fused_form() in ("time-major", "level blocks", "levels")
    keys = ["ChanQKin", "ChanM3Kin", "ChanQ", "sumDisDay", "FlowVelocity", "TravelDistance"]
    if split:
        keys += ["Chan2QKin", "Chan2M3Kin", "CrossSection2Area", "Sideflow1Chan"]
    got = {k: ens.state(k) for k in keys}
    last = g["sampled"].tolist().index(n - 1)
    for k in keys:
        if k == "CrossSection2Area":
            scale = float(np.max(np.abs(g["Chan2M3Start"] / g["ChanLength"])))
            np.testing.assert_allclose(got[k][0], g["out_" + k][last], rtol=RTOL, atol=RTOL * scale)
        else:
            np.testing.assert_allclose(got[k][0], g["out_" + k][last], rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=k)
    for m in (1, 2):
        vm = scaled(scales[m])
        mm = amd.routing.routing(vm, split_routing=split)
        mm.attach_router(g["codes"], g["mask"])
        mm.dynamic_fused(g["ToChanM3RunoffDt"])
        for k in keys:
            assert np.array_equal(got[k][m], getattr(vm, k), equal_nan=True), (m, k)
        mm.river_router.close()
    ens.free()
    mod.river_router.close()


def test_refusals_on_a_real_router(amd, solver):
    from lisflood_amd import ldd as L
    from lisflood_amd.routing import _STATE, _OUT, _STATIC, SubstepVectors, substep_host_vectors
    codes, p, vals, dt = case("shallow")
    kw = make_router(amd, codes, p, vals, dt)
    perm = kw.graph.layout()[0].astype(np.int64)
    sv = SubstepVectors(substep_host_vectors(vals, N, perm, _STATIC), N, p["beta"], 1.0 / dt, dt * NSTEPS, True, True,
                        lengths={k: 2 * N for k in _STATE + _OUT}, sideflow=np.zeros((2, N)))
    before = sv.download("ChanQKin")
    with pytest.raises(amd.lib.LisfloodAmdError, match=r"member_stride %d is less than the router's number of cells \(%d\)" % (N - 1, N)):
        kw.routing_substeps_members(sv.args, NSTEPS, 2, N - 1)
    with pytest.raises(amd.lib.LisfloodAmdError, match="member_stride 0 is less than"):
        kw.routing_substeps_members(sv.args, NSTEPS, 2, 0)
    with pytest.raises(amd.lib.LisfloodAmdError, match="sideflow_member_stride %d" % (N - 1)):
        kw.routing_substeps_members(sv.args, NSTEPS, 2, N, 0, N - 1)
    with pytest.raises(amd.lib.LisfloodAmdError, match="sideflow_member_stride %d" % N):
        kw.routing_substeps_members(sv.args, NSTEPS, 2, N, N, N)             # one vector per sub-step: nsteps * N at least
    pixel_order = sv.with_overrides(engine_order=0)
    with pytest.raises(amd.lib.LisfloodAmdError, match="engine-order"):
        kw.routing_substeps_members(pixel_order, NSTEPS, 2)
    # a graph with structure links: cut the LDD at a few cells, their inflow cells come back as zero-length links
    flat = codes.reshape(-1).astype(np.float64)
    allm = np.ones((H, W), bool)
    down = L.downstream_index(flat, allm)
    sites = np.random.default_rng(2).choice(np.nonzero(down >= 0)[0], 12, replace=False)
    is_site = np.zeros(N, bool)
    is_site[sites] = True
    feeds = (down >= 0) & is_site[np.maximum(down, 0)]
    cut = flat.copy()
    cut[feeds] = L.PIT
    gl = amd.kw.Graph(cut, allm, virtual_down=np.where(feeds, down, -1))
    linked = amd.kw.kinematicWave(None, None, p["alpha"], p["beta"], p["dx"], dt, graph=gl, alpha_floodplains=vals["ChannelAlpha2"])
    for members in (1, 2):
        with pytest.raises(amd.lib.LisfloodAmdError, match="structure links"):
            linked.routing_substeps_members(sv.args, NSTEPS, members)
    assert np.array_equal(sv.download("ChanQKin"), before)
    sv.free()
    linked.close()
    kw.close()
