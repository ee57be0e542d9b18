"""The ensemble forms of the stages between the land surface and the channel loop, on the device: the per-pixel aggregates
(lf_pixel_aggregates_members_device), the overland step (lf_surface_step_members) and the row gather
(lf_gather_rows_device).  Every member's rows are compared bit for bit (module_edges.same_bits) with the single call on that
member's own copy, over three consecutive calls, with padded strides and sentinels between the rows."""
import numpy as np
import pytest

import hotpath_members as HM
from module_edges import first_difference, same_bits

pytestmark = pytest.mark.gpu

SIZES = {2880: (48, 60), 120: (10, 12)}      # 11 full blocks of 256 pixels and a ragged one; one ragged block
CALLS = 3
REPORT = {"TaPixel", "ThetaAll", "LZAvInflow", "GwLossCUM", "InterSealed", "Theta1bPixel"}    # a subset: k_pixel_aggregates<false>


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def assert_rows(got, alone, what):
    """got: per call name -> [M, ...]; alone: per member, per call name -> [...]"""
    for s, out in enumerate(got):
        assert out, what
        for k, rows in out.items():
            for m in range(rows.shape[0]):
                assert same_bits(rows[m], alone[m][s][k]), (what, s, k, m, first_difference(rows[m], alone[m][s][k]))


@pytest.mark.parametrize("forcing_per_member", [False, True], ids=["forcing_shared", "forcing_per_member"])
@pytest.mark.parametrize("report", [None, REPORT], ids=["all_maps", "report_subset"])
@pytest.mark.parametrize("N", list(SIZES))
def test_pixel_aggregates_of_every_member_as_alone(amd, monkeypatch, N, report, forcing_per_member):
    M = 3
    monkeypatch.delenv("LF_PIXEL_MEMBERS", raising=False)
    monkeypatch.delenv("LF_AGG_ALL", raising=False)
    shared, members = HM.pixel_inputs(N, M, 40 + N, forcing_per_member)
    alone = []
    for m in range(M):
        got, form = HM.run_pixel_single(shared, members[m], report, CALLS, N)
        assert form == 1
        alone.append(got)
    assert not same_bits(alone[0][0]["LZ"], alone[1][0]["LZ"])                 # the members do differ
    assert not same_bits(alone[0][0]["TaCUM"] if report is None else alone[0][0]["GwLossCUM"],
                         alone[0][2]["TaCUM"] if report is None else alone[0][2]["GwLossCUM"])     # the sums accumulate
    got, untouched, form = HM.run_pixel_members(shared, members, report, CALLS, N, forcing_per_member)
    assert form == 2 and untouched
    assert_rows(got, alone, "one launch")
    monkeypatch.setenv("LF_PIXEL_MEMBERS", "0")
    got, untouched, form = HM.run_pixel_members(shared, members, report, CALLS, N, forcing_per_member)
    assert form == 3 and untouched
    assert_rows(got, alone, "member after member")
    monkeypatch.delenv("LF_PIXEL_MEMBERS")
    got, untouched, form = HM.run_pixel_members(shared, members[:1], report, CALLS, N, forcing_per_member)
    assert form == 1 and untouched
    assert_rows(got, alone[:1], "members = 1")


@pytest.fixture(scope="module")
def overland(amd):
    """N -> (the three overland routers of hotpath_scenario's graph: direct, other, forest; values; scalars)"""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.kinematic_wave_parallel import Graph, kinematicWave
    made = {}

    def get(N):
        if N not in made:
            values, sc, mask, ldd_to_chan, _ = syn.hotpath_scenario(*SIZES[N])
            g = Graph(ldd_to_chan, mask)
            mk = lambda row: kinematicWave(None, None, np.asarray(values["OFAlpha"], float)[row], sc["Beta"], sc["PixelLength"],
                                           sc["DtSec"], graph=g)
            other, forest, direct = mk(0), mk(1), mk(2)
            made[N] = ((direct, other, forest), values, sc)
        return made[N]
    yield get
    for routers, _, _ in made.values():
        for r in routers:
            r.close()


@pytest.mark.parametrize("M", [3, 5])
@pytest.mark.parametrize("N", list(SIZES))
def test_surface_step_of_every_member_as_alone(amd, overland, monkeypatch, N, M):
    monkeypatch.delenv("LF_SURFACE_MEMBERS", raising=False)
    monkeypatch.delenv("LF_MEMBERS_MB", raising=False)
    routers, values, sc = overland(N)
    shared, members = HM.surface_inputs(N, M, 70 + N + M, values)
    alone = []
    for m in range(M):
        got, form = HM.run_surface_single(routers, shared, members[m], sc, CALLS, N)
        assert form == 1
        alone.append(got)
    assert not same_bits(alone[0][0]["OFQOther"], alone[1][0]["OFQOther"]) and not same_bits(alone[0][0]["OFQOther"], alone[0][2]["OFQOther"])
    single_launches = routers[0].last_launches()
    got, untouched, form = HM.run_surface_members(routers, shared, members, sc, CALLS, N)
    assert form == 2 and untouched
    assert_rows(got, alone, "one launch")
    for r in routers:                    # ONE member sweep of the three routers: the launches of one single sweep
        assert r.last_launches() == single_launches, (r.last_launches(), single_launches)
    monkeypatch.setenv("LF_SURFACE_MEMBERS", "0")
    got, untouched, form = HM.run_surface_members(routers, shared, members, sc, CALLS, N)
    assert form == 3 and untouched
    assert_rows(got, alone, "member after member")
    monkeypatch.delenv("LF_SURFACE_MEMBERS")
    got, untouched, form = HM.run_surface_members(routers, shared, members[:1], sc, CALLS, N)
    assert form == 1 and untouched
    assert_rows(got, alone[:1], "members = 1")


def test_gather_rows_is_gather_row_by_row(amd):
    """5 rows of 700 entries gathered out of rows of 1000 through one index table, both strides padded: lf_gather_device of
    every row, nothing written between the rows; and one row is lf_gather_device"""
    import ctypes as C
    L = amd.lib()
    rng = np.random.default_rng(5)
    n_src, n, rows, sstride, dstride = 1000, 700, 5, 1000 + 11, 700 + 13
    index = rng.integers(0, n_src, n).astype(np.int32)
    src = rng.standard_normal((rows, sstride))
    d_idx, d_src = amd.DeviceArray.from_host(index), amd.DeviceArray.from_host(src.reshape(-1))
    d_dst = amd.DeviceArray.from_host(np.full(rows * dstride, HM.SENTINEL))
    amd.check(L.lf_gather_rows_device(0, n, d_idx.ptr, d_src.ptr, sstride, d_dst.ptr, dstride, rows))
    got = d_dst.download().reshape(rows, dstride)
    one = amd.DeviceArray(n)
    for r in range(rows):
        amd.check(L.lf_gather_device(0, n, d_idx.ptr, d_src.ptr.value + 8 * r * sstride, one.ptr))
        assert np.array_equal(got[r, :n], one.download()) and np.array_equal(got[r, :n], src[r, index]), r
    assert (got[:, n:] == HM.SENTINEL).all()
    d_dst.upload(np.full(rows * dstride, HM.SENTINEL))
    amd.check(L.lf_gather_rows_device(0, n, d_idx.ptr, d_src.ptr, 0, d_dst.ptr, dstride, 2))      # src_stride 0: one source row
    got = d_dst.download().reshape(rows, dstride)
    assert np.array_equal(got[0, :n], src[0, index]) and np.array_equal(got[1, :n], src[0, index]) and (got[2:] == HM.SENTINEL).all()
    for d in (d_idx, d_src, d_dst, one):
        d.free()


# ---- the chain: HotPathEnsemble beside one HotPathDevice per member ------------------------------------------------------
CH, CW_, CM, STEPS, PAD = 48, 60, 3, 3, 5
CN = CH * CW_
NOT_IN_THE_ENSEMBLE = {"scratch", "scratch0", "scratch1", "ESMax"}     # work space, and the soil kernel's copy of ESMax
CHAIN_REPORT = {"TaPixel", "ThetaAll", "LZAvInflow", "Theta1bPixel", "Sat1", "GwLossCUM"}
# structures_scenario(n_lakes=3, n_res=5) by seed: with the default one (23) a site cell feeds another site, so the site plan
# of the time-major form does not apply (lf_site_plan) and the loop with structures keeps the skewed wavefront whatever the
# switch says; with seed 24 it applies, and LF_FUSED_TIME_MAJOR=1 reaches the structures member kernel
CHAINED, PLANNED = 23, 24
VARIANTS = {          # structures (False or the seed), split, report, environment
    "plain": (False, True, None, {}),
    "structures": (CHAINED, True, None, {}),
    "no_split": (False, False, None, {}),
    "structures_no_split": (CHAINED, False, None, {}),
    "report_subset": (False, True, CHAIN_REPORT, {}),
    "time_major": (False, True, None, {"LF_FUSED_TIME_MAJOR": "1"}),
    "time_major_structures": (PLANNED, True, None, {"LF_FUSED_TIME_MAJOR": "1"}),
    "time_major_chained_sites": (CHAINED, True, None, {"LF_FUSED_TIME_MAJOR": "1"}),
    "skewed": (False, True, None, {"LF_FUSED_TIME_MAJOR": "0"}),
    "skewed_structures": (PLANNED, True, None, {"LF_FUSED_TIME_MAJOR": "0"}),
}


def cp(d):
    return {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}


@pytest.fixture(scope="module")
def scenario():
    from lisflood_amd import synthetic as syn
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(CH, CW_)
    st, cut = {}, {}
    for seed in (CHAINED, PLANNED):
        st[seed], cut[seed] = syn.structures_scenario(ldd_kin, (CH, CW_), values["ChanQ"], sc["DtRouting"], n_lakes=3, n_res=5,
                                                      seed=seed)
    return values, sc, mask, ldd_to_chan, ldd_kin, st, cut


def member_forcing(m, s):
    from lisflood_amd import synthetic as syn
    return syn.hotpath_forcing(CN, s + 10 * m)


def member_inflow(st, m, s):
    return st["QInM3Old"] * (1.0 + 0.1 * s + 0.05 * m)


def build(scenario, cls, structures, split, report, **kw):
    values, sc, mask, ldd_to_chan, ldd_kin, st, cut = scenario
    return cls(cp(values), sc, mask, ldd_to_chan, cut[structures] if structures else ldd_kin, split=split,
               structures=cp(st[structures]) if structures else None, report=report, **kw)


def site_plan_applies(ens):
    """lf_site_plan on the site lists and the level schedule of the ensemble's channel part: does the time-major form with
    structures apply?"""
    import ctypes as C
    from lisflood_amd import _lib
    dev = ens.rmod._st["dev"]
    lists = [np.ascontiguousarray(dev[k].download(), np.int32) for k in ("lake_cell", "lake_ups_ptr", "lake_ups_idx", "res_cell",
                                                                         "res_ups_ptr", "res_ups_idx")]
    level_start = np.ascontiguousarray(ens.river.graph.layout()[2], np.int64)
    nl, applies = level_start.size - 1, C.c_int32(-1)
    slot, ptr, sites = np.zeros(ens.Nk, np.int32), np.zeros(nl + 1, np.int32), np.zeros(lists[0].size + lists[3].size, np.int32)
    _lib.check(_lib.lib().lf_site_plan(ens.Nk, nl, _lib.ptr(level_start), lists[0].size, *[_lib.ptr(x) for x in lists[:3]],
                                       lists[3].size, *[_lib.ptr(x) for x in lists[3:]], C.byref(applies), _lib.ptr(slot),
                                       _lib.ptr(ptr), _lib.ptr(sites)))
    return bool(applies.value)


def snapshot(hp):
    """every vector of a HotPathDevice: name -> array (download / download_site / chan_q_avg)"""
    out = {k: hp.download(k) for k in hp.d if k not in NOT_IN_THE_ENSEMBLE}
    if hp.rmod is not None:
        out.update({"site:" + k: hp.download_site(k) for k in hp.rmod._st["dev"]})
    out["chan_q_avg"] = hp.chan_q_avg()
    return out


_reference = {}


def reference(scenario, variant, forcing=member_forcing, steps=STEPS, members=CM):
    """per step, per member: snapshot of that member's own HotPathDevice; worked out once per variant and forcing"""
    key = (variant, forcing.__name__, steps, members)
    if key not in _reference:
        structures, split, report, _ = VARIANTS[variant]
        out = [[None] * members for _ in range(steps)]
        for m in range(members):
            hp = build(scenario, __import__("lisflood_amd.hotpath", fromlist=["x"]).HotPathDevice, structures, split, report)
            for s in range(steps):
                hp.step(forcing(m, s), time_since_start=s + 1, QInM3=member_inflow(scenario[5][structures], m, s) if structures else None)
                out[s][m] = snapshot(hp)
            hp.free()
        _reference[key] = out
    return _reference[key]


def assert_members_equal(ens, want, step, members=None, at_least=60):
    """every vector of the ensemble, member by member, against the members' own snapshots (at_least: how many of them must
    have been member vectors)"""
    members = range(ens.members) if members is None else members
    seen = 0
    for k in want[0]:
        if k.startswith("site:"):
            got = ens.download_site(k[5:])
        elif k == "chan_q_avg":
            got = ens.chan_q_avg()
        else:
            got = ens.download(k)
        per_member = np.ndim(got) == np.ndim(want[0][k]) + 1
        for m in members:
            g = got[m] if per_member else got
            assert same_bits(g, want[m][k]), (step, k, m, first_difference(g, want[m][k]))
        seen += per_member
    assert seen >= at_least or ens.report is not None, seen    # (the member vectors were really there)


def assert_gaps(ens, sentinel):
    from lisflood_amd.soilloop import GAP_BYTE
    for k in ens.gap_names():
        g = ens.gaps(k)
        assert g.shape == (ens.members, PAD), (k, g.shape)
        if g.dtype == np.uint8:
            assert (g == GAP_BYTE).all(), k
        else:
            ok = (g == sentinel) | np.isnan(g)
            assert ok.all() and not np.isnan(g[:-1]).any(), (k, g)


def run_ensemble(scenario, variant, forcing=member_forcing, steps=STEPS, members=CM, after_step=None, **kw):
    from lisflood_amd.hotpath import HotPathEnsemble
    structures, split, report, _ = VARIANTS[variant]
    ens = build(scenario, HotPathEnsemble, structures, split, report, members=members, pad=PAD, **kw)
    ens.set_gaps(HM.SENTINEL)
    for s in range(steps):
        f = [forcing(m, s) for m in range(members)]
        q = np.stack([member_inflow(scenario[5][structures], m, s) for m in range(members)]) if structures else None
        ens.step({k: np.stack([x[k] for x in f]) for k in f[0]}, time_since_start=s + 1, QInM3=q)
        if after_step is not None:
            after_step(ens, s)
    return ens


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_member_of_the_chain_as_its_own_hot_path(amd, scenario, monkeypatch, variant):
    for k in ("LF_FUSED_TIME_MAJOR", "LF_LAND_MEMBERS", "LF_PIXEL_MEMBERS", "LF_SURFACE_MEMBERS", "LF_MEMBERS_MB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in VARIANTS[variant][3].items():
        monkeypatch.setenv(k, v)
    want = reference(scenario, variant)
    forms = []

    def check(ens, s):
        assert_members_equal(ens, want[s], s)
        assert_gaps(ens, HM.SENTINEL)
        forms.append(ens.last_forms())
    ens = run_ensemble(scenario, variant, after_step=check)
    assert not same_bits(want[2][0]["ChanQ"], want[2][1]["ChanQ"]) and not same_bits(want[2][0]["LZ"], want[2][1]["LZ"])
    for f in forms:
        assert (f["land"], f["pixel_aggregates"], f["overland"]) == (2, 2, 2), f
        if variant in ("time_major", "time_major_structures"):      # the member kernel, with and without structures
            assert f["channel"] == "time-major", f
        if variant.startswith("skewed") or variant == "time_major_chained_sites":
            assert f["channel"] != "time-major", f
    if VARIANTS[variant][0]:
        assert ens.Nk < ens.N                      # the compact channel domain, with the structures on it
        assert site_plan_applies(ens) == (VARIANTS[variant][0] == PLANNED)      # (what the variants' names say)
    ens.free()


def test_shared_forcing_gives_identical_members(amd, scenario, monkeypatch):
    monkeypatch.delenv("LF_FUSED_TIME_MAJOR", raising=False)
    from lisflood_amd.hotpath import HotPathEnsemble
    ens = build(scenario, HotPathEnsemble, False, True, None, members=CM, pad=PAD)
    want = reference(scenario, "plain")
    for s in range(2):
        ens.step(member_forcing(0, s), time_since_start=s + 1)            # [N] vectors: every member reads them
        assert ens.land.forcing_member_stride() == 0
        assert_members_equal(ens, [want[s][0]] * CM, s)
    ens.free()


def test_one_member_is_the_hot_path(amd, scenario, monkeypatch):
    monkeypatch.delenv("LF_FUSED_TIME_MAJOR", raising=False)
    want = reference(scenario, "structures")

    def check(ens, s):
        assert_members_equal(ens, want[s][:1], s)
        f = ens.last_forms()
        assert (f["land"], f["pixel_aggregates"], f["overland"]) == (1, 1, 1), f
    run_ensemble(scenario, "structures", members=1, after_step=check).free()


def test_member_after_member_switches_give_the_same_bits(amd, scenario, monkeypatch):
    monkeypatch.delenv("LF_FUSED_TIME_MAJOR", raising=False)
    for k in ("LF_LAND_MEMBERS", "LF_PIXEL_MEMBERS", "LF_SURFACE_MEMBERS"):
        monkeypatch.setenv(k, "0")
    want = reference(scenario, "plain")

    def check(ens, s):
        assert_members_equal(ens, want[s], s)
        assert_gaps(ens, HM.SENTINEL)
        f = ens.last_forms()
        assert (f["land"], f["pixel_aggregates"], f["overland"]) == (3, 3, 3), f
    run_ensemble(scenario, "plain", after_step=check).free()


def nan_rain(m, s):
    f = member_forcing(m, s)
    if m == 1:
        f["Rain"][::137] = np.nan
    return f


def test_a_member_with_nan_rain_stays_alone(amd, scenario, monkeypatch):
    monkeypatch.delenv("LF_FUSED_TIME_MAJOR", raising=False)
    want = reference(scenario, "plain")
    poisoned = reference(scenario, "plain", forcing=nan_rain)
    assert np.isnan(poisoned[2][1]["ChanQ"]).any() and np.isnan(poisoned[2][1]["DirectRunoff"]).any()

    def check(ens, s):
        assert_members_equal(ens, want[s], s, members=(0, 2))
        assert_members_equal(ens, poisoned[s], s, members=(1,))
        assert_gaps(ens, HM.SENTINEL)
    run_ensemble(scenario, "plain", forcing=nan_rain, after_step=check).free()


@pytest.mark.parametrize("variant", ["plain", "structures"])
def test_state_file_continues_the_run(amd, scenario, monkeypatch, tmp_path, variant):
    monkeypatch.delenv("LF_FUSED_TIME_MAJOR", raising=False)
    from lisflood_amd.hotpath import HotPathEnsemble
    structures, split, report, _ = VARIANTS[variant]
    want = reference(scenario, variant)
    path = str(tmp_path / "state.npz")
    first = run_ensemble(scenario, variant, steps=2)
    first.save_state(path)
    saved = np.load(path)
    assert saved["ChanQ"].shape == (CM, CN) and saved["W1a"].shape == (CM, 3, CN) and int(saved["steps_done"]) == 2
    first.free()
    fresh = build(scenario, HotPathEnsemble, structures, split, report, members=CM, pad=PAD)
    fresh.load_state(path)
    f = [member_forcing(m, 2) for m in range(CM)]
    q = np.stack([member_inflow(scenario[5][structures], m, 2) for m in range(CM)]) if structures else None
    fresh.step({k: np.stack([x[k] for x in f]) for k in f[0]}, time_since_start=3, QInM3=q)
    state = fresh.state_names() + (["site:LakeStorageM3CC", "site:ReservoirStorageM3CC"] if structures else []) + ["chan_q_avg"]
    assert_members_equal(fresh, [{k: w[k] for k in state} for w in want[2]], 2, at_least=40)
    # water on a pixel outside the compact channel domain is refused, as HotPathDevice.load_state refuses it
    if fresh.Nk < fresh.N:
        rows = np.zeros((CM, CN))
        rows[1, np.setdiff1d(np.arange(CN), fresh.ids)[0]] = 1.0
        with pytest.raises(ValueError, match="compact=False"):
            fresh.set_member_state("ChanQ", rows)
    with pytest.raises(ValueError, match="no state vector"):
        fresh.set_member_state("DirectRunoff", np.zeros((CM, CN)))
    fresh.free()


def test_member_0_against_the_oracle_chain(amd, scenario, oracle, monkeypatch):
    """member 0 of a structure-free run against the same chain assembled from the C oracle, within the tolerance of
    test_gpu_parity.test_resident_hot_path_vs_oracle_chain: the new chain pinned to something that is not the code under test"""
    import types
    monkeypatch.delenv("LF_FUSED_TIME_MAJOR", raising=False)
    values, sc, mask, ldd_to_chan, ldd_kin, _, _ = scenario
    v = types.SimpleNamespace()
    for k, a in list(cp(values).items()) + list(sc.items()):
        setattr(v, k, np.ascontiguousarray(a, dtype=np.float64) if isinstance(a, np.ndarray) and a.dtype.kind == "f" else a)
    v.InvBeta, v.InvPixelLength, v.InvDtSec = 1 / v.Beta, 1 / v.PixelLength, 1 / v.DtSec
    v.InvDtRouting, v.InvNoRoutSteps, v.NoRoutSteps = 1 / v.DtRouting, 1 / v.NoRoutSteps, int(v.NoRoutSteps)
    idx = np.arange(3)
    surf = oracle.SurfaceRouting(v, ldd_to_chan, mask)
    kw = oracle.kinematicWave(ldd_kin, mask, v.ChannelAlpha, v.Beta, v.ChanLength, v.DtRouting, alpha_floodplains=v.ChannelAlpha2)
    sub = oracle.RoutingSubstep(kw, v)

    def check(ens, step):
        for k, a in member_forcing(0, step).items():
            setattr(v, k, a)
        oracle.canopy(v, idx)
        d = dict(vars(v))
        d["ESMax"] = np.ascontiguousarray(v.ESRef * v.LAITerm)
        d.update(index_landuse_all=idx, is_irrigated=np.array([False, False, True]), is_paddy_irrig=np.zeros(3, bool),
                 paddy_inactive=np.zeros((1, CN), bool))
        oracle.soil_columns(d)
        v.TimeSinceStart = float(step + 1)
        oracle.pixel_aggregates(v)
        surf.dynamic()
        v.sumDisDay = np.zeros(CN)
        for s in range(v.NoRoutSteps):
            sub.dynamic(split=True, sideflow_m3=v.ToChanM3RunoffDt)
        for k in ("W1a", "W1b", "W2", "UZ", "Infiltration", "CumInterception", "LZ", "DirectRunoff", "OFQOther",
                  "OFQDirect", "ToChanM3RunoffDt", "ChanQKin", "Chan2QKin", "ChanM3Kin", "ChanQ", "sumDisDay"):
            got, want = ens.download(k)[0], np.asarray(getattr(v, k))
            np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-9 * max(1.0, float(np.abs(want).max())), err_msg=(step, k))
    ens = run_ensemble(scenario, "plain", steps=2, after_step=check)
    assert np.isfinite(v.ChanQ).all() and v.ChanQ.max() > 0
    ens.free()


def test_a_step_on_the_forcing_the_device_holds(amd, scenario, monkeypatch):
    """step(None) is a step with the forcing rows of the step before"""
    monkeypatch.delenv("LF_FUSED_TIME_MAJOR", raising=False)
    from lisflood_amd.hotpath import HotPathEnsemble
    f = [member_forcing(m, 0) for m in range(2)]
    rows = {k: np.stack([x[k] for x in f]) for k in f[0]}
    a, b = (build(scenario, HotPathEnsemble, False, True, None, members=2, pad=PAD) for _ in range(2))
    for ens, second in ((a, rows), (b, None)):
        ens.step(rows)
        ens.step(second)
    for k in a.state_names() + ["ToChanM3RunoffDt"]:
        assert same_bits(a.download(k), b.download(k)), k
    assert same_bits(a.chan_q_avg(), b.chan_q_avg()) and a.steps_done == b.steps_done == 2
    a.free(); b.free()
