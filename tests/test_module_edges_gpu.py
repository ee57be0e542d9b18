"""-m gpu: the element-wise module kernels and the lake / reservoir sites on both sides and on the ties of every
comparison they make.  The inputs, the census that shows which branches they take and the numpy restatement of the
reference lines are in tests/module_edges.py; tests/test_module_edges_cpu.py pins the CPU oracle to the restatement bit
for bit without a GPU.  Here the HIP kernels run the same inputs:

  k_canopy and the land-surface form of the soil kernel (lf_canopy.h)  against oracle.canopy
  k_pixel_aggregates<true> / <false>                                    against oracle.pixel_aggregates, bit for bit
  k_surface_pre / k_surface_post                                        against oracle.SurfaceRouting
  k_inloop_sites + k_inloop_dense, value by value                       against oracle.InloopStructures, bit for bit
  k_sites_wave / k_sites_blocks / fused_cell<STRUCT> inside the loop    against the sub-step-by-sub-step engine bit for bit
                                                                        and the oracle loop, for four option sets

The library is built with -ffp-contract=off -fno-fast-math, so a body that holds only + - * / sqrt and comparisons gives
the oracle's bits; where a pow or an exp is involved the bar is the one of the existing module tests."""
import ctypes as C
import types

import numpy as np
import pytest

import module_edges as E

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12          # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def _model_var(N):
    """The slice of LisfloodModel_ini (Lisflood_initial.py:108-113, 272-345) the module classes read."""
    from collections import OrderedDict
    uses = ["Rainfed", "Forest", "Irrigated"]
    pres = [u + "_prescribed" for u in uses]
    v = types.SimpleNamespace()
    v.SOIL_USES, v.PRESCRIBED_VEGETATION, v.vegetation, v.prescribed_vegetation = uses, pres, pres[:], pres[:]
    v.VEGETATION_LANDUSE = OrderedDict(zip(pres, uses))
    v.LANDUSE_VEGETATION = OrderedDict([(u, [p]) for p, u in zip(pres, uses)])
    v.dim_pixel, v.dim_landuse = ("pixel", np.arange(N)), ("landuse", uses)
    v.dim_runoff = ("runoff", ["Other", "Forest", "Direct"])
    return v


def _same(got, want, what):
    assert E.same_bits(got, want), "%s: %s" % (what, E.first_difference(got, want))


# ----------------------------------------------------------------------------------------------------------------------
# a. canopy
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [None, {"repStressDays": True, "wateruse": True}], ids=["plain", "stress_days_wateruse"])
@pytest.mark.parametrize("N", [1, 255, 257, 777])
def test_canopy_on_both_sides_of_every_branch(amd, oracle, N, options):
    """soilloop(v).dynamic_canopy(), two consecutive calls so the state carries over, against oracle.canopy at the bar of
    test_soilloop_module_golden (the catch holds an exp) -- and wherever the oracle gives exactly 0, exactly 1 for RWS, or
    NaN, the device gives exactly that: Ta on frozen pixels, Interception where SMax = 0, TaInterception and
    LeafDrainage where cum <= 0, RWS in {0, 1}.  With the option switches on, SoilMoistureStressDays is DtDay exactly
    where the oracle's RWS < 1 and 0 elsewhere; WFilla / WFillb against the restated lines at rtol 1e-12."""
    from lisflood_amd.soilloop import soilloop
    d = E.canopy_inputs(N)
    vg, vc = E.canopy_var(d, base=_model_var(N)), E.canopy_var(d)
    if options:
        vg.SoilMoistureStressDays = np.full((3, N), -1.0)
    m = soilloop(vg, options=options)
    m.initial()
    assert list(m.index_landuse_prescr) == [0, 1, 2]
    for step in range(2):
        E.canopy_forcing(vg, d, step); E.canopy_forcing(vc, d, step)
        lines, _ = E.canopy_reference(d, {k: getattr(vc, k).copy() for k in E.CANOPY_STATE}, step)
        oracle.canopy(vc, [0, 1, 2])
        m.dynamic_canopy()
        for k in E.CANOPY_IO:
            got, want = getattr(vg, k), getattr(vc, k)
            np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-11, err_msg=str((step, k)))
            exact = (want == 0) | np.isnan(want) | ((want == 1) if k == "RWS" else False)
            _same(got[exact], want[exact], (step, k, "where the oracle gives exactly 0, 1 or NaN"))
        assert (vg.Ta[:, d["isFrozenSoil"]] == 0).all()
        if options:
            assert np.array_equal(vg.SoilMoistureStressDays, np.where(vc.RWS < 1, d["DtDay"], 0.0)), step
            np.testing.assert_allclose(vg.WFilla, lines["WFilla"], rtol=1e-12, atol=0, err_msg=str(step))
            np.testing.assert_allclose(vg.WFillb, lines["WFillb"], rtol=1e-12, atol=0, err_msg=str(step))
        else:
            assert not hasattr(vg, "WFilla")


def test_canopy_edges_in_the_land_surface_kernel_equal_the_three_launches(amd):
    """The same edge columns through HotPathDevice: land_fused=True (canopy, ESMax and the soil columns in one pass,
    k_soil_fused<.., CANOPY>) against land_fused=False (k_canopy, then the soil kernel) -- every state vector and every
    canopy / soil output bit for bit over two model steps.  The canopy maps, the layer-1 soil moisture and limits and
    the frozen flags of a 70 x 90 synthetic scenario are the builder's."""
    from lisflood_amd import soilloop as SL
    from lisflood_amd import synthetic as syn
    from lisflood_amd.hotpath import HotPathDevice
    H, W = 70, 90
    N = H * W
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    d = E.canopy_inputs(N)
    for k in ("LAI", "LAITerm", "CropGroupNumber", "WFC1", "WFC1a", "WFC1b", "WWP1", "WWP1a", "WWP1b", "W1", "W1a", "W1b",
              "CumInterception", "isFrozenSoil"):
        assert values[k].shape == d[k].shape, k
        values[k] = d[k].copy()
    sc = dict(sc, DtDay=d["DtDay"], InvDtDay=d["InvDtDay"])
    cp = lambda x: {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in x.items()}
    a = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True, land_fused=False)
    b = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True, land_fused=True)
    assert b.land_fused and not a.land_fused
    names = list(dict.fromkeys(a.state_names() + SL._CANOPY_IO + list(SL._V_IO)))
    for s in range(2):
        f = dict(syn.hotpath_forcing(N, s), Rain=d["Rain"][s].copy(), EWRef=d["EWRef"][s].copy(), ETRef=d["ETRef"][s].copy())
        a.step(f, s + 1)
        b.step(f, s + 1)
        for k in names:
            assert np.array_equal(a.download(k), b.download(k), equal_nan=True), (s, k)
        for k in ("RWS", "Ta", "Interception"):
            assert np.isfinite(b.download(k)).all(), (s, k)
    a.free(); b.free()


# ----------------------------------------------------------------------------------------------------------------------
# b. pixel aggregates
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agg_all", [None, "0"], ids=["all_loads_up_front", "block_by_block"])
@pytest.mark.parametrize("N", [1, 255, 257, 1000])
def test_pixel_aggregates_bit_for_bit(amd, oracle, monkeypatch, N, agg_all):
    """pixel_aggregates.dynamic(v), two steps, both template instances of the kernel (LF_AGG_ALL unset: k_pixel_aggregates
    <true>; = 0: <false>): every state and output vector the oracle's bits -- the body has no transcendental."""
    from lisflood_amd import pixel_aggregates as PA
    if agg_all is None:
        monkeypatch.delenv("LF_AGG_ALL", raising=False)
    else:
        monkeypatch.setenv("LF_AGG_ALL", agg_all)
    d = E.pixel_inputs(N)
    vg = vc = None
    for step in range(2):
        vg, vc = E.pixel_var(d, step, vg), E.pixel_var(d, step, vc)
        oracle.pixel_aggregates(vc)
        PA.dynamic(vg)
        for k in E.PIX_STATE + E.PIX_OUT:
            _same(getattr(vg, k), getattr(vc, k), (step, k))
    planted = E.spots(6, N)                                  # no soil fraction: Theta NaN, ThetaAll exactly 0
    assert (vg.ThetaAll[planted] == 0).all() and np.isfinite(vg.ThetaAll).all()


# ----------------------------------------------------------------------------------------------------------------------
# c. surface routing
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.6, 0.5])
def test_surface_routing_with_runoff_on_both_sides_of_zero(amd, oracle, beta):
    """surface_routing(v).dynamic() against oracle.SurfaceRouting on a 24 x 31 raster with about 30 % channel pixels, two
    steps, Beta = 0.6 (the fused 3/5 power) and 0.5 (pow): SurfaceRunSoil, SurfaceRunoff and TotalRunoff bit for bit
    (products, sums and a maximum), the routed vectors at the tolerance of test_gpu_parity.py.  The builder keeps runoff
    at 0 or well above it: a volume under 86.4 m3 is left open by the reference's own Newton tolerance at rtol 1e-9
    (module_edges.surface_inputs; first run here: one cell of 0.12 m3, fed 1.4e-6 m3/s, 1.1e-7 apart)."""
    from lisflood_amd.surface_routing import surface_routing
    d = E.surface_inputs(beta)
    N = d["IsChannel"].size
    vg, vc = E.surface_var(d, base=_model_var(N)), E.surface_var(d)
    m = surface_routing(vg)
    m.initialSecond(d["ldd_to_chan"], d["mask"])
    cpu = oracle.SurfaceRouting(vc, d["ldd_to_chan"], d["mask"])
    routed = ("OFQDirect", "OFQOther", "OFQForest", "OFM3Direct", "OFM3Other", "OFM3Forest", "OFToChanM3", "WaterDepth",
              "ToChanM3Runoff", "ToChanM3RunoffDt")
    for step in range(2):
        E.surface_forcing(vg, d, step); E.surface_forcing(vc, d, step)
        cpu.dynamic()
        m.dynamic()
        for k in ("SurfaceRunSoil", "SurfaceRunoff", "TotalRunoff"):
            _same(np.asarray(getattr(vg, k)), getattr(vc, k), (step, k))
        for k in routed:
            np.testing.assert_allclose(getattr(vg, k), getattr(vc, k), rtol=RTOL, atol=ATOL, err_msg=str((step, k)))
        assert (vc.OFToChanM3[~d["IsChannel"]] == 0).all() and (vg.OFToChanM3[~d["IsChannel"]] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# d. the sites, value by value
# ----------------------------------------------------------------------------------------------------------------------
def _device_inloop_args(amd, d, st, options):
    """routing._InloopArgs on DeviceArrays for lf_inloop_structures, pixel order; st: the oracle's InloopStructures of the
    same inputs (its CSR lists are the upstream lists).  Every index is checked against the vector it addresses here."""
    from lisflood_amd import routing as R
    N = d["ChanQ"][0].size
    a, dev = R._InloopArgs(), {}

    def put(name, arr):
        arr = np.ascontiguousarray(arr)
        dev[name] = amd.DeviceArray.from_host(arr)
        setattr(a, name, dev[name].ptr.value)
    put("ChanQ", d["ChanQ"][0]); put("ToChanM3RunoffDt", d["ToChanM3RunoffDt"]); put("SideflowChanM3", np.zeros(N))
    for which, cells, (ptr, idx), param, state in (("lake", st.lake_cell, st.lake_csr, E.LAKE_PARAM, E.LAKE_STATE),
                                                   ("res", st.res_cell, st.res_csr, E.RES_PARAM, E.RES_STATE)):
        n = cells.size
        if not n:
            continue
        assert cells.dtype == np.int32 and ptr.dtype == np.int32 and idx.dtype == np.int32
        assert 0 <= cells.min() and cells.max() < N and ptr[0] == 0 and (np.diff(ptr) >= 0).all() and ptr.size == n + 1
        assert ptr[-1] <= idx.size and 0 <= idx.min() and idx.max() < N
        setattr(a, "n_lakes" if which == "lake" else "n_res", n)
        put(which + "_cell", cells); put(which + "_ups_ptr", ptr); put(which + "_ups_idx", idx)
        for k in param:
            put(k, np.asarray(d[k], np.float64))
        dense = "LakeStorageM3" if which == "lake" else "ReservoirStorageM3"
        for k in state:
            put(k, d[dense][cells] if k == dense + "CC" else np.asarray(d.get(k, np.zeros(n)), np.float64))
        put("QLakeOutM3Dt" if which == "lake" else "QResOutM3Dt", np.zeros(N))
    if options.get("inflow"):
        put("QInM3Old", d["QInM3Old"]); put("QDelta", d["QDelta"]); put("QInDt", np.zeros(N)); put("QinADDEDM3", d["QinADDEDM3"])
    if options.get("TransLoss"):
        put("UpTrans", d["UpTrans"].astype(np.uint8)); put("TransLossM3Dt", np.zeros(N)); put("TransCum", d["TransCum"])
        a.TransPower1, a.TransPower2, a.TransSub = d["TransPower1"], d["TransPower2"], d["TransSub"]
    if options.get("openwaterevapo"):
        put("EvaAddM3Dt", d["EvaAddM3Dt"])
    if options.get("wateruse"):
        put("WUseAddM3Dt", d["withdrawal_CH_actual_M3_routStep"] - d["returnflow_GwAbs2Channel_M3_routStep"])
    if options.get("simulatePolders"):
        put("ChannelToPolderM3Dt", d["ChannelToPolderM3Dt"])
    a.DtRouting, a.InvNoRoutSteps, a.N = d["DtRouting"], d["InvNoRoutSteps"], N
    for name in ["ChanQ", "ToChanM3RunoffDt", "UpTrans", "EvaAddM3Dt", "WUseAddM3Dt", "ChannelToPolderM3Dt"] + E.DENSE_OUT:
        assert name not in dev or dev[name].shape == (N,), (name, dev[name].shape)       # indexed by cell: N entries each
    for names, n in ((E.LAKE_PARAM + E.LAKE_STATE, a.n_lakes), (E.RES_PARAM + E.RES_STATE, a.n_res)):
        assert all(dev[k].shape == (n,) for k in names if k in dev)
    return a, dev


@pytest.mark.parametrize("sites", [(130, 190), (0, 70), (70, 0), (1, 1)])
def test_sites_value_by_value(amd, oracle, sites):
    """lf_inloop_structures (k_inloop_sites, k_inloop_dense) called directly, step = 0 then step = 1, on the planted
    lakes and reservoirs: the four exact ties of the fill, every regime, the damping rule, both clamps, total = 0 (fill
    inf and NaN), lake storage < 0 and NaN, sites with none / one / eight sources and the sum 1e16 + 1 + 1 in ascending
    source order; 320 sites are two workgroups with the lake / reservoir boundary inside a wavefront, (0, 70) and (70, 0)
    are the i - n_lakes arithmetic.  Every site vector and both dense outflow vectors: the oracle's bits.  The dense
    vectors too, except the transmission loss, its sum and the sideflow where UpTrans is set: loss = (Q - pow(pow(Q, p2)
    - sub, p1)) * dt is a difference of nearly equal numbers, a few ulp of Q * dt off whatever its size (the `cancel`
    scale of test_structures_mid_size_vs_oracle, here with the largest Q of a flagged reach)."""
    options = E.LOOP_OPTION_SETS["everything"]
    d = E.site_inputs(*sites)
    vc = E.site_var(d)
    st = oracle.InloopStructures(vc, options)
    vc.QinADDEDM3 = d["QinADDEDM3"].copy()
    a, dev = _device_inloop_args(amd, d, st, options)
    flagged = d["UpTrans"]
    cancel = 256 * np.finfo(float).eps * max(float(q[flagged].max()) for q in d["ChanQ"]) * d["DtRouting"]
    site_keys = (E.LAKE_STATE + ["QLakeOutM3Dt"] if sites[0] else []) + (E.RES_STATE + ["QResOutM3Dt"] if sites[1] else [])
    for step in range(2):
        vc.ChanQ = d["ChanQ"][step].copy()
        st.dynamic_inloop(step)
        dev["ChanQ"].upload(d["ChanQ"][step])
        a.step = step
        amd.check(amd.lib().lf_inloop_structures(0, C.byref(a)))
        for k in site_keys + ["QInDt", "QinADDEDM3"]:
            _same(dev[k].download(), getattr(vc, k), (sites, step, k))
        for k in ("TransLossM3Dt", "TransCum", "SideflowChanM3"):
            got, want = dev[k].download(), getattr(vc, k)
            _same(got[~flagged], want[~flagged], (sites, step, k, "where UpTrans is not set"))
            np.testing.assert_allclose(got[flagged], want[flagged], rtol=0, atol=cancel * (step + 1 if k == "TransCum" else 1),
                                       err_msg=str((sites, step, k)))
    if sites == (130, 190):
        big = E.spots(14, 190)[0]
        assert dev["ReservoirInflowCC"].download()[big] == 1e16          # (1e16 + 1) + 1, not 1e16 + (1 + 1)
    for x in dev.values():
        x.free()


# ----------------------------------------------------------------------------------------------------------------------
# e. the sites inside the loop, option subsets
# ----------------------------------------------------------------------------------------------------------------------
_ROUTED = ["ChanQKin", "ChanM3Kin", "Chan2QKin", "Chan2M3Kin", "ChanQ", "sumDisDay"]


def _loop_keys(options):
    keys = list(_ROUTED)
    if options.get("simulateLakes"):
        keys += ["QLakeOutM3Dt", "LakeStorageM3CC", "LakeOutflowCC", "LakeInflowOldCC", "LakeStorageM3BalanceCC", "LakeLevelCC"]
    if options.get("simulateReservoirs"):
        keys += ["QResOutM3Dt", "ReservoirStorageM3CC", "ReservoirFillCC"]
    if options.get("inflow"):
        keys += ["QInDt", "QinADDEDM3"]
    if options.get("TransLoss"):
        keys += ["TransLossM3Dt", "TransCum"]
    return keys


_loop_inputs = {}


@pytest.mark.parametrize("name", list(E.LOOP_OPTION_SETS))
@pytest.mark.parametrize("family", ["deep", "shallow"])
def test_sites_inside_the_loop_for_each_option_set(amd, oracle, family, name):
    """The routing module (engine_order=True, attach_router on the cut LDD, attach_structures) on a 120 x 160 raster with
    130 lakes + 190 reservoirs: all four in-loop modules with the three optional sideflow terms (EvaAddM3Dt,
    WUseAddM3Dt, ChannelToPolderM3Dt) non-zero; lakes only; reservoirs only; inflow + transmission loss without sites --
    the NULL-pointer branches of k_inloop_dense and fused_cell<STRUCT>.  dynamic_fused() (k_sites_wave / k_sites_blocks
    inside the wavefront) against 24 x dynamic(s) (k_inloop_sites) bit for bit, and both against the oracle loop at the
    tolerances of test_structures_mid_size_vs_oracle.  What the oracle's run visits (every regime, both clamps, the
    damping rule; at most four NaN sites) is asserted in tests/test_module_edges_cpu.py."""
    from lisflood_amd import routing as R
    if family not in _loop_inputs:
        _loop_inputs[family] = E.loop_inputs(family)
    r, s, cut, mask = _loop_inputs[family]
    switches = E.LOOP_OPTION_SETS[name]
    nsteps = int(r["NoRoutSteps"])

    def module():
        v = E.loop_var(r, s)
        m = R.routing(v, options=dict(SplitRouting=True, InitLisflood=False, **switches), engine_order=True)
        m.attach_router(cut, mask)
        m.attach_structures()
        return v, m
    (va, ma), (vb, mb) = module(), module()
    for sub in range(nsteps):
        ma.dynamic(sub)
    mb.dynamic_fused()
    keys = _loop_keys(switches)
    for k in keys:
        assert np.array_equal(getattr(va, k), getattr(vb, k), equal_nan=True), (family, name, k)
    vc, _ = E.loop_oracle_run(oracle, family, name)
    cancel = 256 * np.finfo(float).eps * float(np.nanmax(vc.ChanQ)) * r["DtRouting"]
    for k in keys:
        atol = cancel * (nsteps if k == "TransCum" else 1) if k in ("TransLossM3Dt", "TransCum") else 1e-6
        np.testing.assert_allclose(getattr(vb, k), getattr(vc, k), rtol=RTOL, atol=atol, err_msg=str((family, name, k)))
    assert np.isfinite(vb.ChanQ).mean() >= 0.9 and np.nanmax(vb.ChanQ) > 0
