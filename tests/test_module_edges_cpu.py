"""The CPU oracle against numpy restatements of the reference lines, bit for bit, on inputs that take both sides and the
ties of every comparison in dynamic_canopy, the pixel aggregates, the arithmetic before the overland routers and the
lake / reservoir / inflow / transmission-loss step of the routing loop -- and the census that shows the inputs do
(tests/module_edges.py).  No GPU: this is what makes the expected values of tests/test_module_edges_gpu.py trustworthy."""
import ctypes as C

import numpy as np
import pytest

import module_edges as E


def _same(got, want, what):
    assert E.same_bits(got, want), "%s: %s" % (what, E.first_difference(got, want))


def _no_zero_entry(title, census, allowed_zero=()):
    print("\n" + E.counts_table(title, census))
    empty = [k for k, n in census.items() if n < 1 and k not in allowed_zero]
    assert not empty, (title, empty)


def _add(total, census):
    for k, n in census.items():
        total[k] = total.get(k, 0) + n


def test_canopy_oracle_is_the_reference_lines_and_the_inputs_take_every_branch(oracle):
    """oracle.canopy on [3, 777], two consecutive calls: every output the bits of the restated soilloop.py:519-627."""
    d = E.canopy_inputs(777)
    v = E.canopy_var(d)
    total = {}
    for step in range(2):
        E.canopy_forcing(v, d, step)
        state = {k: getattr(v, k).copy() for k in E.CANOPY_STATE}
        want, mid = E.canopy_reference(d, state, step)
        oracle.canopy(v, [0, 1, 2])
        for k in E.CANOPY_IO:
            _same(getattr(v, k), want[k], (step, k))
            assert np.isfinite(getattr(v, k)).all(), (step, k)
        # what the GPU test asserts exactly is there to assert
        assert ((want["RWS"] == 0) | (want["RWS"] == 1)).sum() > 10 and (want["Ta"][:, d["isFrozenSoil"]] == 0).all()
        assert ((want["SoilMoistureStressDays"] == d["DtDay"]) == (v.RWS < 1)).all()
        _add(total, E.canopy_census(mid))
        if step == 0:          # (by the second call W1 is W1a + W1b and the planted columns have given what they had)
            _no_zero_entry("canopy, first call", E.canopy_census(mid))
    _no_zero_entry("canopy, both calls", total)


def test_pixel_aggregates_oracle_is_the_reference_lines_and_the_inputs_take_every_branch(oracle):
    d = E.pixel_inputs(1000)
    v = None
    total = {}
    for step in range(2):
        v = E.pixel_var(d, step, v)
        state = {k: np.array(getattr(v, k), copy=True) for k in E.PIX_STATE}
        want, mid = E.pixel_reference(d, state, step)
        oracle.pixel_aggregates(v)
        for k in E.PIX_OUT + E.PIX_STATE:
            _same(getattr(v, k), want[k], (step, k))
        planted = E.spots(6, 1000)                       # no soil fraction: Theta NaN, ThetaAll exactly +0
        assert np.isnan(v.Theta[:, planted]).all() and (v.ThetaAll[planted] == 0).all() and not np.signbit(v.ThetaAll[planted]).any()
        assert np.isfinite(v.ThetaAll).all()
        _add(total, E.pixel_census(mid))
        if step == 0:
            _no_zero_entry("pixel aggregates, first step", E.pixel_census(mid))
    _no_zero_entry("pixel aggregates, both steps", total)


def test_surface_pre_oracle_is_the_reference_lines_and_the_inputs_take_every_branch(oracle):
    d = E.surface_inputs(0.6)
    N = d["IsChannel"].size
    p = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p)
    for step in range(2):
        want = E.surface_pre_reference(d, step)
        got = dict(SurfaceRunSoil=np.empty((3, N)), SurfaceRunoff=np.empty(N), TotalRunoff=np.empty(N), side=np.empty((3, N)))
        keep = [np.ascontiguousarray(d[k][step] if isinstance(d[k], list) else d[k], np.float64) for k in
                ("SoilFraction", "AvailableWaterForInfiltration", "Infiltration", "DirectRunoff", "UZOutflowPixel",
                 "LZOutflowToChannelPixel")]
        oracle.lib().lfo_surface_pre(*[p(a) for a in keep], C.c_double(d["MMtoM3"]), C.c_double(1 / d["PixelLength"]),
                                     C.c_double(1 / d["DtSec"]), C.c_int64(N), p(got["SurfaceRunSoil"]), p(got["SurfaceRunoff"]),
                                     p(got["TotalRunoff"]), p(got["side"]))
        for k in got:
            _same(got[k], want[k], (step, k))
        _no_zero_entry("surface routing, step %d" % step, E.surface_census(d, step))


@pytest.mark.parametrize("beta", [0.6, 0.5])
def test_surface_volumes_of_the_oracle_run_are_above_what_the_newton_tolerance_leaves_open(oracle, beta):
    """The routed part of the surface case is compared at rtol 1e-9: that is decidable only for volumes of at least
    NEWTON_TOL * DtSec / 1e-9 = 86.4 m3 (module_edges.surface_inputs).  The oracle's own run has no smaller one, and it
    does have exact zeros."""
    d = E.surface_inputs(beta)
    v = E.surface_var(d)
    cpu = oracle.SurfaceRouting(v, d["ldd_to_chan"], d["mask"])
    for step in range(2):
        E.surface_forcing(v, d, step)
        cpu.dynamic()
        ok, smallest = E.surface_volumes_are_comparable(v)
        print("beta %.1f step %d: smallest overland volume > 0: %.1f m3" % (beta, step, smallest))
        assert ok, (step, smallest)
        assert min((getattr(v, k) == 0).sum() for k in ("OFM3Direct", "OFM3Other", "OFM3Forest")) >= 1


def _expected_vectors(options, nl, nr):
    keys = ["SideflowChanM3"]
    if options.get("simulateLakes") and nl:
        keys += E.LAKE_STATE + ["QLakeOutM3Dt"]
    if options.get("simulateReservoirs") and nr:
        keys += E.RES_STATE + ["QResOutM3Dt"]
    if options.get("inflow"):
        keys += ["QInDt", "QinADDEDM3"]
    if options.get("TransLoss"):
        keys += ["TransLossM3Dt", "TransCum"]
    return keys


@pytest.mark.parametrize("sites", [(130, 190), (0, 70), (70, 0), (1, 1)])
@pytest.mark.parametrize("name", list(E.LOOP_OPTION_SETS))
def test_inloop_structures_oracle_is_the_reference_lines(oracle, sites, name):
    """oracle.InloopStructures(v, options), sub-steps 0 and 1, against the np.where cascade of reservoir.py, the lines of
    lakes.py, np.bincount for the site inflow and the dense lines of inflow.py / transmission.py / routing.py:462-478 --
    every vector it writes, bit for bit, for each option set (site lists empty, QInM3Old / UpTrans NULL, the three
    optional sideflow terms)."""
    options = E.LOOP_OPTION_SETS[name]
    d = E.site_inputs(*sites)
    v = E.site_var(d)
    st = oracle.InloopStructures(v, options)
    v.QinADDEDM3 = d["QinADDEDM3"].copy()
    for step in range(2):
        v.ChanQ = d["ChanQ"][step].copy()
        want, _ = E.inloop_reference(d, v, step, options)
        st.dynamic_inloop(step)
        keys = _expected_vectors(options, *sites)
        assert set(keys) == set(want), (sorted(keys), sorted(want))
        for k in keys:
            _same(getattr(v, k), want[k], (name, sites, step, k))


def test_default_options_of_the_oracle_wrapper_are_the_four_switches(oracle):
    d = E.site_inputs(130, 190)
    va, vb = E.site_var(d), E.site_var(d)
    a, b = oracle.InloopStructures(va), oracle.InloopStructures(vb, E.ALL_OPTIONS)
    for step in range(2):
        a.dynamic_inloop(step); b.dynamic_inloop(step)
    for k in E.LAKE_STATE + E.RES_STATE + E.DENSE_OUT:
        _same(getattr(va, k), getattr(vb, k), k)


def test_site_inputs_take_every_rule_tie_and_clamp(oracle):
    """the census of the value-by-value case (130 lakes + 190 reservoirs), from the inputs and the restated lines"""
    d = E.site_inputs(130, 190)
    v = E.site_var(d)
    st = oracle.InloopStructures(v, E.ALL_OPTIONS)
    res, lake = {}, {}
    for step in range(2):
        v.ChanQ = d["ChanQ"][step].copy()
        _, mid = E.inloop_reference(d, v, step, E.ALL_OPTIONS)
        st.dynamic_inloop(step)
        if step == 0:
            first = E.reservoir_census(mid["res"])
        _add(res, E.reservoir_census(mid["res"]))
        _add(lake, E.lake_census(mid["lake"]))
    _no_zero_entry("reservoirs, sub-step 0", first)
    for k in ("fill == 2 Conservative", "fill == Normal", "fill == Normal_Flood", "fill == Flood"):
        assert first[k] >= 2, (k, first[k])               # planted at both ends of the reservoir list
    assert 1 <= first["total == 0: fill inf"] + first["total == 0: fill NaN"] <= 4
    _no_zero_entry("reservoirs, both sub-steps", res)
    _no_zero_entry("lakes, both sub-steps", lake)
    layout = E.layout_census(d)
    _no_zero_entry("site layout", layout)
    assert layout["sites"] > 256 and layout["workgroups of the site kernels"] == 2
    # the ascending-source order shows: (1e16 + 1) + 1 is 1e16, 1e16 + (1 + 1) is not
    big = E.spots(14, 190)[0]
    assert v.ReservoirInflowCC[big] == 1e16 and (1.0 + 1.0) + 1e16 != 1e16
    dense = {"UpTrans set": int(d["UpTrans"].sum()), "UpTrans not set": int((~d["UpTrans"]).sum()),
             "inflow points": int((d["QInM3Old"] != 0).sum()), "EvaAddM3Dt != 0": int((d["EvaAddM3Dt"] != 0).sum()),
             "WUseAddM3Dt != 0": int((d["withdrawal_CH_actual_M3_routStep"] != d["returnflow_GwAbs2Channel_M3_routStep"]).sum()),
             "ChannelToPolderM3Dt != 0": int((d["ChannelToPolderM3Dt"] != 0).sum())}
    _no_zero_entry("dense part", dense)


@pytest.mark.parametrize("family", ["deep", "shallow"])
def test_sites_inside_the_loop_visit_every_regime(oracle, family):
    """the conditions of the in-loop case, on the oracle's run alone: over the 24 sub-steps every reservoir regime, both
    clamps and the damping rule are visited; at the end at least 90 % of the sites and of the cells are finite and at
    most four sites are NaN; no site is the downstream neighbour of another."""
    v, census = E.loop_oracle_run(oracle, family, "everything")
    _no_zero_entry("sites inside the loop (%s), 24 sub-steps" % family, census,
                   allowed_zero=("fill == 2 Conservative", "fill == Normal", "fill == Normal_Flood", "fill == Flood"))
    sites = np.concatenate([v.LakeStorageM3CC, v.ReservoirStorageM3CC])
    nan_sites = int(np.isnan(v.LakeStorageM3CC + v.LakeOutflowCC).sum() + np.isnan(v.ReservoirStorageM3CC).sum())
    print("NaN sites: %d of %d; finite cells: %d of %d" % (nan_sites, sites.size, int(np.isfinite(v.ChanQ).sum()), v.ChanQ.size))
    assert nan_sites <= 4
    assert np.isfinite(v.LakeOutflowCC).mean() >= 0.9 and np.isfinite(v.ReservoirStorageM3CC).mean() >= 0.9
    for k in ("ChanQ", "ChanQKin", "Chan2QKin", "SideflowChanM3"):
        assert np.isfinite(getattr(v, k)).mean() >= 0.9, k
    is_site = np.zeros(v.ChanQ.size + 1, bool)
    is_site[v.LakeIndex] = True; is_site[v.ReservoirIndex] = True
    assert not is_site[v.downstruct[np.concatenate([v.LakeIndex, v.ReservoirIndex])]].any()
