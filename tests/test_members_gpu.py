"""An ensemble on one router (lf_router_route_ordered_members / kinematicWaveRoutingEnsemble): M members that share the
LDD and the channel geometry are swept with ONE launch per wide level, narrow run or level block.  Every member must be
bit-identical to its own route_ordered call on the same router, and agree with the oracle within the project's routing
tolerance."""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12
SENTINEL = -777.25      # padding between the rows of the state vectors: neither read nor written


def close(a, b, msg=""):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=str(msg))


@pytest.fixture(scope="module")
def amd():
    import types
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    from lisflood_amd import kinematic_wave_parallel
    return types.SimpleNamespace(kw=kinematic_wave_parallel, lib=_lib)


@pytest.fixture(params=["fused_beta_3_5", "general_pow"])
def solver(request, monkeypatch):
    """both arithmetic paths of the router, chosen when it is created: the beta = 3/5 polynomial solve and the
    reference's own iteration with pow (LF_GENERAL_POW=1: k_prep for all members, `constant` of members * N)"""
    if request.param == "general_pow":
        monkeypatch.setenv("LF_GENERAL_POW", "1")
    else:
        monkeypatch.delenv("LF_GENERAL_POW", raising=False)
    return request.param


# ---- the 160 x 160 graphs and their members ---------------------------------------------------------------------------
H = W = 160
N = H * W
M, PAD, CALLS, ZERO_MEMBER = 5, 37, 3, 3


def member_inputs(n, members, calls, zero_member=None):
    """member m starts from Q0 * (1 + 0.25 m) and gets lateral_inflow(n, 300 + 10 m + s) in call s"""
    from lisflood_amd import synthetic as syn
    p = syn.router_params(n)
    Q0 = np.stack([p["Q0"] * (1 + 0.25 * m) for m in range(members)])
    lat = np.stack([[syn.lateral_inflow(n, 300 + 10 * m + s) for m in range(members)] for s in range(calls)])
    if zero_member is not None:
        Q0[zero_member] = 0.0
        lat[:, zero_member] = 0.0
    return p, Q0, lat


_cases = {}


@pytest.fixture(scope="module")
def case(oracle):
    """family -> (ldd raster, parameters, Q0[M, N], lat[CALLS, M, N], oracle's Q[CALLS, M, N]); worked out once"""
    from lisflood_amd import synthetic as syn

    def get(family):
        if family not in _cases:
            codes = syn.make_ldd(family, H, W, 5)
            p, Q0, lat = member_inputs(N, M, CALLS, ZERO_MEMBER)
            cpu = oracle.kinematicWave(codes.reshape(-1).astype(np.float64), np.ones((H, W), bool), p["alpha"], p["beta"],
                                       p["dx"], p["dt"])
            want = np.empty((CALLS, M, N))
            for m in range(M):
                Q = Q0[m].copy()
                for s in range(CALLS):
                    cpu.kinematicWaveRouting(Q, lat[s, m])
                    want[s, m] = Q
            for a in (Q0, lat, want):
                a.setflags(write=False)
            _cases[family] = (codes, p, Q0, lat, want)
        return _cases[family]
    return get


def make_router(amd, codes, p, **kw):
    g = amd.kw.Graph(ldd_raster=codes)
    return amd.kw.kinematicWave(None, None, p["alpha"], p["beta"], p["dx"], p["dt"], graph=g, **kw)


def rows(pix, perm, stride):
    """[M, n] pixel order -> [M, stride] sweep order, the padding filled with the sentinel"""
    out = np.full((pix.shape[0], stride), SENTINEL)
    out[:, :perm.size] = pix[:, perm]
    return out


def single_calls(amd, kw, perm, Q0, lat, section="main_channel"):
    """every member alone through route_ordered on the same router -> [calls, M, n] in sweep order"""
    calls, members, n = lat.shape
    out = np.empty((calls, members, n))
    for m in range(members):
        Q = amd.lib.DeviceArray.from_host(np.ascontiguousarray(Q0[m][perm]))
        for s in range(calls):
            q = amd.lib.DeviceArray.from_host(np.ascontiguousarray(lat[s, m][perm]))
            kw.route_ordered(Q, q, section)
            out[s, m] = Q.download()
            q.free()
        Q.free()
    return out


def member_calls(amd, kw, perm, Q0, lat, stride, section="main_channel"):
    """all members in one call per step -> [calls, M, stride] discharge rows and [calls, M, stride] lateral rows as the
    device holds them afterwards, and the launch statistics of the last call"""
    calls, members, n = lat.shape
    Q = amd.lib.DeviceArray.from_host(rows(Q0, perm, stride))
    got, lat_after = [], []
    for s in range(calls):
        q = amd.lib.DeviceArray.from_host(rows(lat[s], perm, stride))
        kw.route_ordered_members(Q, q, members, stride, section)
        got.append(Q.download())
        lat_after.append(q.download())
        q.free()
    Q.free()
    return np.stack(got), np.stack(lat_after), kw.last_launches()


# what each configuration is there to reach, per graph: (wide-level launches, narrow-run or cone launches).  The deep
# graph has no level of more than 217 cells: its launches are cone launches (level blocks) or narrow runs (segments).
CONFIGS = {
    "default": {},                             # level blocks -> k_sweep_cones_members
    "segments": {"LF_ROUTE_CONES": "0"},       # k_level_members for levels > 1024 cells, k_levels_narrow_members
    "blocks_wide": {"LF_FUSED_WIDE": "2000"},  # block schedule whose levels > 2000 cells are single-level blocks
    "cones_256": {"LF_ROUTE_CONE_WIDTH": "256"},  # level blocks planned for 256-wide cones: the member cone kernel with barriers
}
REACHES = {("shallow", "default"): (False, True), ("shallow", "segments"): (True, True), ("shallow", "blocks_wide"): (True, True),
           ("shallow", "cones_256"): (False, True), ("deep", "cones_256"): (False, True),
           ("deep", "default"): (False, True), ("deep", "segments"): (False, True), ("deep", "blocks_wide"): (False, True)}


def every_row_as_alone(amd, case, monkeypatch, family, config):
    """M = 5, stride = N + 37, three consecutive calls in `config`: every row equals the member routed alone bit for bit,
    agrees with the oracle, the all-zero member stays exactly zero and the padding keeps its sentinel in both vectors"""
    for k, v in CONFIGS[config].items():
        monkeypatch.setenv(k, v)                  # before the router exists: LF_FUSED_WIDE is read when it is created
    codes, p, Q0, lat, want = case(family)
    kw = make_router(amd, codes, p)
    perm = kw.graph.layout()[0]
    stride = N + PAD
    alone = single_calls(amd, kw, perm, Q0, lat)
    got, lat_after, st = member_calls(amd, kw, perm, Q0, lat, stride)
    wide, narrow = REACHES[family, config]
    assert (st["wide"] > 0) == wide and (st["narrow"] > 0) == narrow, st
    if config != "segments":
        assert kw.route_plan_stats()["cone_blocks"] > 0      # "narrow" counted cone launches
    for s in range(CALLS):
        for m in range(M):
            assert np.array_equal(got[s, m, :N], alone[s, m]), (s, m)
            pix = np.empty(N)
            pix[perm] = got[s, m, :N]
            close(pix, want[s, m], (family, config, s, m))
        assert (got[s, ZERO_MEMBER, :N] == 0.0).all()
        assert (got[s, :, N:] == SENTINEL).all() and (lat_after[s][:, N:] == SENTINEL).all()
        assert np.array_equal(lat_after[s][:, :N], lat[s][:, perm])
    kw.close()


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("family", ["shallow", "deep"])
def test_members_through_every_launch_kind(amd, case, solver, monkeypatch, family, config):
    """M = 5 (a short last member group for 2 and 4 members per lane), stride = N + 37, three consecutive calls, with the
    library's own number of members per lane"""
    monkeypatch.delenv("LF_MEMBERS_MB", raising=False)
    every_row_as_alone(amd, case, monkeypatch, family, config)


@pytest.mark.parametrize("mb", ["1", "2", "4"])
@pytest.mark.parametrize("config", ["segments", "blocks_wide"])
def test_wide_levels_with_1_2_4_members_per_lane(amd, case, solver, monkeypatch, config, mb):
    """every instantiation of k_level_members (LF_MEMBERS_MB, read per call), on the graph and in the configurations that
    have wide levels: 5 members are five groups of one, two groups and a single one, one group of four and a single one"""
    monkeypatch.setenv("LF_MEMBERS_MB", mb)
    every_row_as_alone(amd, case, monkeypatch, "shallow", config)


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("family", ["shallow", "deep"])
def test_one_launch_for_all_members(amd, case, solver, monkeypatch, family, config):
    """a member call costs the launches of a single call, k_prep of the general exponent included"""
    for k, v in CONFIGS[config].items():
        monkeypatch.setenv(k, v)
    codes, p, Q0, lat, _ = case(family)
    kw = make_router(amd, codes, p)
    perm = kw.graph.layout()[0]
    single_calls(amd, kw, perm, Q0[:1], lat[:1, :1])
    one = kw.last_launches()
    _, _, many = member_calls(amd, kw, perm, Q0, lat[:1], N)
    assert one["launches"] >= 1 and many == one, (one, many)
    assert (one["launches"] - one["wide"] - one["narrow"]) == (1 if solver == "general_pow" else 0)
    kw.close()


def test_members_do_not_leak_into_each_other(amd, case, solver):
    """member 1's lateral inflow is NaN at twenty source cells: members 0 and 2 do not see it, member 1 is NaN where its
    own single call is"""
    codes, p, Q0, lat, _ = case("deep")
    kw = make_router(amd, codes, p)
    perm, ups_ptr, _ = kw.graph.layout()
    sources = np.flatnonzero(np.diff(ups_ptr) == 0)
    assert sources.size >= 20
    Q0, lat = Q0[:3].copy(), lat[:2, :3].copy()
    lat[:, 1, perm[sources[:: sources.size // 20][:20]]] = np.nan
    alone = single_calls(amd, kw, perm, Q0, lat)
    got, _, _ = member_calls(amd, kw, perm, Q0, lat, N + PAD)
    for s in range(lat.shape[0]):
        for m in (0, 2):
            assert np.array_equal(got[s, m, :N], alone[s, m]) and np.isfinite(got[s, m, :N]).all(), (s, m)
        assert np.isnan(alone[s, 1]).sum() >= 20
        assert np.array_equal(np.isnan(got[s, 1, :N]), np.isnan(alone[s, 1]))
        assert np.array_equal(got[s, 1, :N], alone[s, 1], equal_nan=True)
    kw.close()


def test_sections_and_scalar_dx_through_the_host_form(amd, oracle, solver):
    from lisflood_amd import synthetic as syn
    g = golden("route_etrs89")
    args = (g["codes"], g["mask"], g["alpha"], float(g["beta"]), g["dx"], float(g["dt"]))
    kw = amd.kw.kinematicWave(*args, alpha_floodplains=g["alpha2"])
    scale = np.array([1.0, 0.5, 2.0, 3.5])[:, None]
    E1, E2 = scale * g["Q0"], scale * g["Q0_2"]
    S1, S2 = E1.copy(), E2.copy()
    for s in range(g["q"].shape[0]):
        q1, q2 = scale * g["q"][s], scale * (0.25 * g["q"][s])
        assert kw.kinematicWaveRoutingEnsemble(E1, q1, "main_channel") is None
        kw.kinematicWaveRoutingEnsemble(E2, q2, "floodplains")
        close(E1[0], g["Q"][s], s)
        close(E2[0], g["Q_2"][s], s)
        for m in range(scale.size):
            kw.kinematicWaveRouting(S1[m], q1[m], "main_channel")
            kw.kinematicWaveRouting(S2[m], q2[m], "floodplains")
        assert np.array_equal(E1, S1) and np.array_equal(E2, S2), s
    with pytest.raises(Exception, match="The section parameter must be either 'main_channel' or 'floodplain'!"):
        kw.kinematicWaveRoutingEnsemble(E1, g["q"][0], "floodplain")
    single = amd.kw.kinematicWave(*args)
    before = E1.copy()
    with pytest.raises(amd.lib.LisfloodAmdError, match="alpha_floodplains was not given"):
        single.kinematicWaveRoutingEnsemble(E1, g["q"][0], "floodplains")
    assert np.array_equal(E1, before)
    kw.close(); single.close()
    # a scalar dx (no (a, dx) records) on a masked raster, the lateral inflow broadcast from one row
    Hs, Ws = 120, 90
    codes = syn.make_ldd("deep", Hs, Ws, 2)
    mask = np.ones((Hs, Ws), bool); mask[:9, :11] = False
    c = codes[mask].astype(np.float64)
    n = int(mask.sum())
    p, Q0, lat = member_inputs(n, 4, 3)
    gpu = amd.kw.kinematicWave(c, mask, p["alpha"], 0.6, 5000.0, 86400.0)
    cpu = oracle.kinematicWave(c, mask, p["alpha"], 0.6, 5000.0, 86400.0)
    E, want = Q0.copy(), Q0.copy()
    for s in range(3):
        q = lat[s] if s < 2 else lat[s, 0]           # the last call: one row for all members
        gpu.kinematicWaveRoutingEnsemble(E, q)
        for m in range(4):
            cpu.kinematicWaveRouting(want[m], lat[s, m] if s < 2 else lat[s, 0])
        close(E, want, s)
    gpu.close()


def test_ragged_rasters_vs_oracle(amd, oracle, solver):
    """eight of the random rasters of test_route_random_rasters_vs_oracle (its recipe): 1 x 1, 1 x 17, 23 x 1, 2 x 2 and
    four random shapes, random land masks, extra pits, non-channel cells, beta 0.6 and 0.72, zero and large discharge,
    partly negative lateral inflow; three members, three calls, each member against the oracle"""
    from lisflood_amd import synthetic as syn
    rng = np.random.default_rng(77)
    shapes = [(1, 1), (1, 17), (23, 1), (2, 2)] + [(int(rng.integers(3, 41)), int(rng.integers(3, 41))) for _ in range(4)]
    betas = set()
    for i, (Hr, Wr) in enumerate(shapes):
        mask = rng.random((Hr, Wr)) < rng.uniform(0.5, 1.0)
        if not mask.any():
            mask[0, 0] = True
        raster = syn.make_ldd("shallow" if i % 2 else "deep", Hr, Wr, 100 + i, land_mask=mask)
        codes = raster[mask].astype(np.float64)
        r = rng.random(codes.size)
        codes[r < 0.08] = 5.0            # extra pits
        codes[(r >= 0.08) & (r < 0.16)] = 0.0   # non-channel cells of a channel LDD
        n = codes.size
        beta = 0.6 if i % 3 else 0.72
        betas.add(beta)
        p = syn.router_params(n, seed=200 + i, beta=beta)
        Q0 = p["Q0"].copy()
        Q0[rng.random(n) < 0.2] = 0.0
        Q0[rng.random(n) < 0.05] *= 1e4
        dx = p["dx"] if i % 4 else 2500.0
        gpu = amd.kw.kinematicWave(codes, mask, p["alpha"], beta, dx, p["dt"])
        cpu = oracle.kinematicWave(codes, mask, p["alpha"], beta, dx, p["dt"])
        E = np.stack([Q0 * (1 + 0.25 * m) for m in range(3)])
        want = E.copy()
        for s in range(3):
            q = np.stack([syn.lateral_inflow(n, 300 + 10 * m + s) - (1e-4 if s == 1 else 0.0) for m in range(3)])
            gpu.kinematicWaveRoutingEnsemble(E, q)
            for m in range(3):
                cpu.kinematicWaveRouting(want[m], q[m])
            close(E, want, (i, Hr, Wr, beta, s))
        assert (E >= 0).all()
        gpu.close()
    assert betas == {0.6, 0.72}


def test_edge_arguments(amd, case, solver):
    codes, p, Q0, lat, _ = case("shallow")
    kw = make_router(amd, codes, p)
    perm = kw.graph.layout()[0]
    alone = single_calls(amd, kw, perm, Q0[:2], lat[:1, :2])
    # one member, stride = N: the single call
    got, _, _ = member_calls(amd, kw, perm, Q0[:1], lat[:1, :1], N)
    assert np.array_equal(got[0, 0], alone[0, 0])
    # two members far apart
    got, lat_after, _ = member_calls(amd, kw, perm, Q0[:2], lat[:1, :2], N + 100000)
    assert np.array_equal(got[0, :, :N], alone[0]) and (got[0, :, N:] == SENTINEL).all() and (lat_after[0][:, N:] == SENTINEL).all()
    # the row-by-row permutations, and the default stride
    Qp = amd.lib.DeviceArray.from_host(np.ascontiguousarray(Q0[:2]))
    qp = amd.lib.DeviceArray.from_host(np.ascontiguousarray(lat[0, :2]))
    Qo, qo = kw.to_engine_order_members(Qp, 2), kw.to_engine_order_members(qp, 2)
    assert np.array_equal(Qo.download(), Q0[:2][:, perm])
    kw.route_ordered_members(Qo, qo, 2)
    assert np.array_equal(Qo.download(), alone[0])
    assert np.array_equal(kw.from_engine_order_members(Qo, 2, Qp).download()[:, perm], alone[0])
    # refused on the host, before any launch: a stride below N, no member
    before = Qo.download()
    with pytest.raises(amd.lib.LisfloodAmdError, match="stride %d is less than the router's number of cells" % (N - 1)):
        kw.route_ordered_members(Qo, qo, 2, N - 1)
    with pytest.raises(amd.lib.LisfloodAmdError, match="members must be at least 1"):
        kw.route_ordered_members(Qo, qo, 0)
    # ... and a vector too short for the rows asked for, by the wrapper
    for call in (lambda: kw.route_ordered_members(Qo, qo, 3), lambda: kw.route_ordered_members(Qo, qo, 2, N + 1),
                 lambda: kw.to_engine_order_members(Qp, 3), lambda: kw.from_engine_order_members(Qo, 3),
                 lambda: kw.from_engine_order_members(Qo, 2, amd.lib.DeviceArray(N))):
        with pytest.raises(ValueError, match="member rows"):
            call()
    assert np.array_equal(Qo.download(), before)
    kw.close()
