"""-m gpu: parity of the HIP path (through the C ABI) against the CPU oracle and the committed golden
vectors.  Tolerances: fp64, rtol 1e-9 / atol 1e-12 for routing (north-star bar: 1e-6 relative) -- OCML
pow differs from glibc pow in the last ulp and the Newton iteration damps it; soil rtol 1e-9."""
import os
import types

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12


def close(a, b, msg=""):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=str(msg))


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    from lisflood_amd import kinematic_wave_parallel, soilloop, routing
    return types.SimpleNamespace(kw=kinematic_wave_parallel, soil=soilloop, routing=routing, lib=_lib)


@pytest.fixture(params=["fused_beta_3_5", "general_pow"])
def solver(request, monkeypatch):
    """Both arithmetic paths of the engine: the default one (routing: fused beta = 3/5 polynomial solve,
    csrc/lf_math.h; soil: lf_pow_pos) and the general one that follows the reference's own iteration with OCML
    pow (LF_GENERAL_POW=1)."""
    if request.param == "general_pow":
        monkeypatch.setenv("LF_GENERAL_POW", "1")
    else:
        monkeypatch.delenv("LF_GENERAL_POW", raising=False)
    return request.param


@pytest.mark.parametrize("name", ["syn64_shallow", "syn64_deep", "syn48_masked"])
def test_route_golden(amd, solver, name):
    g = golden("route_" + name)
    kw = amd.kw.kinematicWave(g["codes"], g["mask"], g["alpha"], float(g["beta"]), g["dx"], float(g["dt"]))
    Q = g["Q0"].copy()
    for s in range(g["q"].shape[0]):
        assert kw.kinematicWaveRouting(Q, g["q"][s]) is None
        close(Q, g["Q"][s], (name, s))


def test_route_etrs89_two_sections_golden(amd, solver):
    g = golden("route_etrs89")
    kw = amd.kw.kinematicWave(g["codes"], g["mask"], g["alpha"], float(g["beta"]), g["dx"], float(g["dt"]),
                              alpha_floodplains=g["alpha2"])
    Q1, Q2 = g["Q0"].copy(), g["Q0_2"].copy()
    for s in range(g["q"].shape[0]):
        kw.kinematicWaveRouting(Q1, g["q"][s], "main_channel")
        kw.kinematicWaveRouting(Q2, 0.25 * g["q"][s], "floodplains")
        close(Q1, g["Q"][s], s)
        close(Q2, g["Q_2"][s], s)
    with pytest.raises(Exception):
        kw.kinematicWaveRouting(Q1, g["q"][0], "floodplain")
    single = amd.kw.kinematicWave(g["codes"], g["mask"], g["alpha"], float(g["beta"]), g["dx"], float(g["dt"]))
    with pytest.raises(amd.lib.LisfloodAmdError):
        single.kinematicWaveRouting(Q1, g["q"][0], "floodplains")


def test_route_edge_cases_golden(amd, solver):
    g = golden("route_edge")
    kw = amd.kw.kinematicWave(g["codes"], g["mask"], g["alpha"], float(g["beta"]), g["dx"], float(g["dt"]))
    for k in ("zero", "tiny", "branches", "negative"):
        Q = g["Q0_" + k].copy()
        for s in range(3):
            kw.kinematicWaveRouting(Q, g["q_" + k])
            close(Q, g["Q_" + k][s], (k, s))
    # exact zeros stay exact zeros (early exit / 1e-12 floor, kinematic_wave_parallel_tools.py:61-63, 81-82)
    Q = g["Q0_zero"].copy(); kw.kinematicWaveRouting(Q, g["q_zero"]); assert (Q == 0).all()
    kw0 = amd.kw.kinematicWave(g["codes"], g["mask"], g["alpha_zero"], float(g["beta"]), g["dx"], float(g["dt"]),
                               flagnancheck=True)
    Q = g["Q0_branches"].copy()
    with pytest.warns(Warning):
        kw0.kinematicWaveRouting(Q, g["q_branches"])
    assert np.array_equal(np.isnan(Q), np.isnan(g["Q_alpha_zero"]))
    close(Q, g["Q_alpha_zero"])


def test_route_random_rasters_vs_oracle(amd, oracle):
    """Ragged inputs: 24 random rasters (1 x 1 up to 40 x 40, random land masks, extra pits, non-channel cells,
    single rows / columns), beta = 3/5 and a general beta, zero and large discharge, negative lateral inflow --
    graph attributes and three consecutive router calls against the oracle."""
    from lisflood_amd import synthetic as syn
    rng = np.random.default_rng(77)
    shapes = [(1, 1), (1, 17), (23, 1), (2, 2)] + [(int(rng.integers(3, 41)), int(rng.integers(3, 41))) for _ in range(20)]
    for i, (H, W) in enumerate(shapes):
        mask = rng.random((H, W)) < rng.uniform(0.5, 1.0)
        if not mask.any():
            mask[0, 0] = True
        raster = syn.make_ldd("shallow" if i % 2 else "deep", H, W, 100 + i, land_mask=mask)
        codes = raster[mask].astype(np.float64)
        r = rng.random(codes.size)
        codes[r < 0.08] = 5.0            # extra pits
        codes[(r >= 0.08) & (r < 0.16)] = 0.0   # non-channel cells of a channel LDD
        N = codes.size
        beta = 0.6 if i % 3 else 0.72
        p = syn.router_params(N, seed=200 + i, beta=beta)
        Q0 = p["Q0"].copy()
        Q0[rng.random(N) < 0.2] = 0.0
        Q0[rng.random(N) < 0.05] *= 1e4
        dx = p["dx"] if i % 4 else 2500.0
        gpu = amd.kw.kinematicWave(codes, mask, p["alpha"], beta, dx, p["dt"])
        cpu = oracle.kinematicWave(codes, mask, p["alpha"], beta, dx, p["dt"])
        assert np.array_equal(gpu.downstream_lookup, cpu.downstream_lookup)
        assert np.array_equal(gpu.pixels_ordered, cpu.pixels_ordered) and np.array_equal(gpu.order_start_stop, cpu.order_start_stop)
        Qg, Qc = Q0.copy(), Q0.copy()
        for s in range(3):
            q = syn.lateral_inflow(N, 300 + s) - (1e-4 if s == 1 else 0.0)     # partly negative in the second call
            gpu.kinematicWaveRouting(Qg, q); cpu.kinematicWaveRouting(Qc, q)
            close(Qg, Qc, (i, H, W, beta, s))
        assert (Qg >= 0).all()
        gpu.close()


def test_route_scalar_dx_and_device_form_vs_oracle(amd, oracle):
    from lisflood_amd import synthetic as syn
    H, W = 120, 90
    codes = syn.make_ldd("deep", H, W, 2)
    mask = np.ones((H, W), bool); mask[:9, :11] = False
    c = codes[mask].astype(np.float64)
    N = int(mask.sum())
    p = syn.router_params(N, seed=8)
    gpu = amd.kw.kinematicWave(c, mask, p["alpha"], 0.6, 5000.0, 86400.0)
    cpu = oracle.kinematicWave(c, mask, p["alpha"], 0.6, 5000.0, 86400.0)
    Qc = p["Q0"].copy()
    Qd = amd.lib.DeviceArray.from_host(p["Q0"])
    qd = amd.lib.DeviceArray(N)
    for s in range(5):
        q = syn.lateral_inflow(N, s)
        cpu.kinematicWaveRouting(Qc, q)
        qd.upload(q)
        gpu.route_device(Qd, qd)
        close(Qd.download(), Qc, s)
    st = gpu.last_launches()
    assert st["levels"] == cpu.order_start_stop.shape[0] and st["launches"] >= 1
    # engine-order resident form: same numbers, vectors permuted into sweep order once
    Qc2 = p["Q0"].copy()
    Qo = gpu.to_engine_order(amd.lib.DeviceArray.from_host(p["Q0"]))
    qo = amd.lib.DeviceArray(N)
    for s in range(5):
        q = syn.lateral_inflow(N, s)
        cpu.kinematicWaveRouting(Qc2, q)
        qd.upload(q)
        gpu.to_engine_order(qd, qo)
        gpu.route_ordered(Qo, qo)
    close(gpu.from_engine_order(Qo).download(), Qc2, "ordered")
    perm = gpu.graph.layout()[0]
    assert np.array_equal(Qo.download(), gpu.from_engine_order(Qo).download()[perm])


@pytest.mark.parametrize("family,seed", [("shallow", 1), ("deep", 2)])
def test_route_mid_size_vs_oracle(amd, oracle, solver, family, seed):
    """1200 x 1000 cells: exercises wide-level launches (levels > 1024 cells) next to narrow runs,
    in both the pixel-order and the engine-order form."""
    from lisflood_amd import synthetic as syn
    H, W = 1200, 1000
    codes = syn.make_ldd(family, H, W, seed)
    mask = np.ones((H, W), bool)
    c = codes.reshape(-1).astype(np.float64)
    N = H * W
    p = syn.router_params(N)
    gpu = amd.kw.kinematicWave(c, mask, p["alpha"], p["beta"], p["dx"], p["dt"])
    cpu = oracle.kinematicWave(c, mask, p["alpha"], p["beta"], p["dx"], p["dt"])
    Qg, Qc = p["Q0"].copy(), p["Q0"].copy()
    for s in range(2):
        q = syn.lateral_inflow(N, s)
        gpu.kinematicWaveRouting(Qg, q)
        cpu.kinematicWaveRouting(Qc, q)
        close(Qg, Qc, (family, s))
    st = gpu.last_launches()
    # launches: single wide levels ("wide") + blocks of up to 64 narrower levels swept cone by cone ("narrow")
    # (+ one k_prep launch on the general-exponent path)
    assert 1 <= st["wide"] + st["narrow"] <= st["launches"] <= st["wide"] + st["narrow"] + 1
    assert family != "shallow" or st["wide"] > 0
    assert np.array_equal(gpu.pixels_ordered, cpu.pixels_ordered)
    Qo = gpu.to_engine_order(amd.lib.DeviceArray.from_host(p["Q0"]))
    for s in range(2):
        qo = gpu.to_engine_order(amd.lib.DeviceArray.from_host(syn.lateral_inflow(N, s)))
        gpu.route_ordered(Qo, qo)
    close(gpu.from_engine_order(Qo).download(), Qc, (family, "ordered"))


def test_route_full_size_closure_property(amd):
    """Size-independent property at 4000 x 4000 (1.6e7 cells, beyond what the oracle does in seconds):
    every cell satisfies the discretised kinematic-wave equation
        Qnew + a*Qnew^beta = a*Qold^beta + q*dx + sum(upstream Qnew)      (kinematic_wave_parallel_tools.py:89-92)
    to the Newton tolerance, with the upstream sum taken by the device's own LDD reduction."""
    from lisflood_amd import synthetic as syn
    H = W = 4000
    N = H * W
    codes = syn.make_ldd("shallow", H, W, 1)
    p = syn.router_params(N)
    from lisflood_amd.kinematic_wave_parallel import Graph
    gpu = amd.kw.kinematicWave(None, None, p["alpha"], p["beta"], p["dx"], p["dt"], graph=Graph(ldd_raster=codes))
    Qold = p["Q0"].copy()
    Q = Qold.copy()
    q = syn.lateral_inflow(N, 0)
    gpu.kinematicWaveRouting(Q, q)
    assert np.isfinite(Q).all() and (Q >= 0).all()
    a = p["alpha"] * p["dx"] / p["dt"]
    rhs = a * Qold ** p["beta"] + q * p["dx"] + gpu.upstream_sum(Q)
    lhs = Q + a * Q ** p["beta"]
    resid = np.abs(lhs - rhs)
    assert (resid <= 1e-9 * np.maximum(rhs, 1.0) + 2e-12).all(), float(resid.max())
    # idempotence of the fixed point: routing again with q' chosen so that Qold' = Q is stationary is not
    # available in closed form, but mass is conserved exactly by construction of rhs; check a checksum
    assert abs(lhs.sum() - rhs.sum()) <= 1e-9 * rhs.sum()


def test_route_other_beta_vs_oracle(amd, oracle):
    """beta != 3/5 always takes the general path."""
    from lisflood_amd import synthetic as syn
    H, W = 100, 130
    codes = syn.make_ldd("deep", H, W, 4)
    mask = np.ones((H, W), bool)
    c = codes.reshape(-1).astype(np.float64)
    N = H * W
    p = syn.router_params(N, seed=12, beta=0.7)
    gpu = amd.kw.kinematicWave(c, mask, p["alpha"], 0.7, p["dx"], p["dt"])
    cpu = oracle.kinematicWave(c, mask, p["alpha"], 0.7, p["dx"], p["dt"])
    Qg, Qc = p["Q0"].copy(), p["Q0"].copy()
    for s in range(4):
        q = syn.lateral_inflow(N, s)
        gpu.kinematicWaveRouting(Qg, q)
        cpu.kinematicWaveRouting(Qc, q)
        close(Qg, Qc, s)


@pytest.mark.parametrize("name", ["syn48_masked", "etrs89"])
def test_upstream_sum_golden(amd, name):
    g = golden("upstream_sum")
    N = g["w_" + name].size
    kw = amd.kw.kinematicWave(g["codes_" + name], g["mask_" + name], np.ones(N), 0.6, 1000.0, 3600.0)
    out = kw.upstream_sum(g["w_" + name])
    assert np.array_equal(out, g["sum_" + name])          # same summation order -> bit-exact


@pytest.mark.parametrize("shape", [(57, 80), (259, 1003)])
def test_upstream_sum_raster_lds_tiles(amd, shape):
    """The raster-space one-hop reduction (LDS-staged 3 x 3 LDD neighbourhoods) equals np.bincount over the graph's
    downstream ids bit for bit, including ragged tile edges and non-land cells."""
    from lisflood_amd import ldd as L
    from lisflood_amd import synthetic as syn
    H, W = shape
    rng = np.random.default_rng(4)
    if shape == (57, 80):
        z = golden("etrs89_static")
        mask = z["ldd"] != -1
        raster = np.where(mask, z["ldd"], 0).astype(np.uint8)
    else:
        mask = rng.random((H, W)) > 0.05
        raster = syn.make_ldd("shallow", H, W, 3, land_mask=mask)
    w = rng.uniform(0, 10, (H, W))
    got = L.upstream_raster(raster, w)
    down = L.downstream_index(raster[mask].astype(float), mask)
    N = int(mask.sum())
    want = np.zeros((H, W))
    want[mask] = np.bincount(np.where(down >= 0, down, N), weights=w[mask], minlength=N + 1)[:N]
    assert np.array_equal(got[mask], want[mask])


def test_accuflux_matches_reference_uparea(amd):
    """ec_upArea.nc of the reference's test catchment = accuflux(ldd, pixarea) (routing.py:98)."""
    z = golden("etrs89_static")
    mask = z["ldd"] != -1
    N = int(mask.sum())
    kw = amd.kw.kinematicWave(z["ldd"][mask].astype(np.float64), mask, np.ones(N), 0.6, 1000.0, 3600.0)
    area = z["pixarea"][mask].astype(np.float64)
    acc = kw.accuflux(area)
    # host restatement: accumulate along the sweep order (upstream first, ascending id, then the cell)
    down = kw.downstream_lookup.astype(np.int64)
    want = np.zeros(N)
    for pix in kw.pixels_ordered:
        want[pix] += area[pix]
        if down[pix] >= 0:
            want[down[pix]] += want[pix]
    np.testing.assert_allclose(acc, want, rtol=1e-13)
    # the reference's map was cut out of a larger (pan-European) domain: cells fed from outside the test
    # mask carry more area there, every other cell must agree
    ref = z["uparea"][mask]
    assert (acc <= ref * (1 + 1e-6)).all()
    assert np.isclose(acc, ref, rtol=1e-6).mean() > 0.95


@pytest.mark.parametrize("engine_order", [False, True])
@pytest.mark.parametrize("mode", ["split", "single"])
def test_routing_substeps_golden(amd, solver, mode, engine_order):
    """routing.dynamic() sub-steps (routing.py:435-706) through the HydroModule-shaped wrapper; engine_order=True
    keeps the device vectors in sweep order and runs a sub-step as one level sweep over both routers."""
    g = golden("substep_" + mode)
    v = amd.routing.var_from_fixture(g)
    mod = amd.routing.routing(v, split_routing=(mode == "split"), engine_order=engine_order)
    mod.attach_router(g["codes"], g["mask"])
    sampled = g["sampled"].tolist()
    keys = ["ChanQKin", "ChanM3Kin", "ChanQ", "sumDisDay", "FlowVelocity", "TravelDistance"]
    if mode == "split":
        keys += ["Chan2QKin", "Chan2M3Kin", "CrossSection2Area", "Sideflow1Chan"]
    for s in range(int(g["NoRoutSteps"])):
        v.ToChanM3RunoffDt = g["ToChanM3RunoffDt"][s]
        mod.dynamic(s)
        if s in sampled:
            i = sampled.index(s)
            for k in keys:
                if k == "CrossSection2Area":
                    # (Chan2M3Kin - Chan2M3Start) / ChanLength: a difference of two large volumes, so the
                    # 1e-9 relative bar applies at the scale of the volumes, not of their difference
                    scale = float(np.max(np.abs(g["Chan2M3Start"] / g["ChanLength"])))
                    np.testing.assert_allclose(getattr(v, k), g["out_" + k][i], rtol=RTOL, atol=RTOL * scale)
                else:
                    close(getattr(v, k), g["out_" + k][i], (mode, s, k))


@pytest.mark.parametrize("mode", ["split", "single"])
def test_routing_substeps_fused_wavefront(amd, solver, mode):
    """The 24 sub-steps of a model step as ONE skewed wavefront (lf_routing_substeps_fused): must reproduce the
    reference-captured end state and be bit-identical to 24 sequential sub-steps of the same engine."""
    g = golden("substep_" + mode)
    n = int(g["NoRoutSteps"])
    split = mode == "split"
    # sequential
    v1 = amd.routing.var_from_fixture(g)
    m1 = amd.routing.routing(v1, split_routing=split)
    m1.attach_router(g["codes"], g["mask"])
    for s in range(n):
        v1.ToChanM3RunoffDt = g["ToChanM3RunoffDt"][s]
        m1.dynamic(s)
    # fused, one sideflow vector per sub-step
    v2 = amd.routing.var_from_fixture(g)
    m2 = amd.routing.routing(v2, split_routing=split)
    m2.attach_router(g["codes"], g["mask"])
    m2.dynamic_fused(g["ToChanM3RunoffDt"])
    st = m2.river_router.last_launches()
    assert n <= st["launches"] <= st["levels"] + n     # one launch per level block (up to 16 levels) and sub-step offset, + the flag pass
    keys = ["ChanQKin", "ChanM3Kin", "ChanQ", "sumDisDay", "FlowVelocity", "TravelDistance"]
    if split:
        keys += ["Chan2QKin", "Chan2M3Kin", "CrossSection2Area", "Sideflow1Chan"]
    last = g["sampled"].tolist().index(n - 1)
    for k in keys:
        assert np.array_equal(getattr(v1, k), getattr(v2, k), equal_nan=True), k
        if k == "CrossSection2Area":
            scale = float(np.max(np.abs(g["Chan2M3Start"] / g["ChanLength"])))
            np.testing.assert_allclose(getattr(v2, k), g["out_" + k][last], rtol=RTOL, atol=RTOL * scale)
        else:
            close(getattr(v2, k), g["out_" + k][last], (mode, k))
    # one sideflow vector shared by all sub-steps (the model's case) == sequential with that vector
    v3 = amd.routing.var_from_fixture(g); v4 = amd.routing.var_from_fixture(g)
    m3 = amd.routing.routing(v3, split_routing=split); m3.attach_router(g["codes"], g["mask"])
    m4 = amd.routing.routing(v4, split_routing=split); m4.attach_router(g["codes"], g["mask"])
    v3.ToChanM3RunoffDt = v4.ToChanM3RunoffDt = g["ToChanM3RunoffDt"][3]
    for s in range(n):
        m3.dynamic(s)
    m4.dynamic_fused()
    for k in keys:
        assert np.array_equal(getattr(v3, k), getattr(v4, k), equal_nan=True), k


def test_routing_module_initial_to_step_end_on_etrs89(amd, oracle):
    """routing.initial -> initialSecond -> 24 x dynamic -> step_end on the LF_ETRS89 static maps (the reference's
    own test catchment), checked against the reference-formula parameters of the golden fixture and against the
    oracle driven with the same parameters."""
    z = golden("etrs89_static")
    gold = golden("route_etrs89")
    mask = z["ldd"] != -1
    f = lambda k: z[k][mask].astype(np.float64)
    v = types.SimpleNamespace(DtSec=86400.0, DtSecChannel=3600.0)
    m = amd.routing.routing(v, split_routing=False)
    m.initial(dict(beta=0.6, ChanLength=f("chanlength"), Ldd=f("ldd"), Channels=f("chan"), ChanGrad=f("changrad"),
                   ChanGradMin=0.0001, CalChanMan=f("calchanman1"), ChanMan=f("chanman"), ChanBottomWidth=f("chanbw"),
                   ChanDepthThreshold=f("chanbnkf"), ChanSdXdY=f("chans"), PixelArea=f("pixarea")), mask)
    assert v.NoRoutSteps == 24 and v.DtRouting == 3600.0
    np.testing.assert_allclose(v.ChannelAlpha, gold["alpha"], rtol=1e-12)
    np.testing.assert_allclose(v.ChanQKin, gold["Q0"], rtol=1e-12)
    assert v.IsChannel.all() and (v.LddToChan == 5).all()        # every land pixel of LF_ETRS89 is a channel pixel
    assert np.isclose(v.UpArea, z["uparea"][mask], rtol=1e-6).mean() > 0.95
    assert v.Catchments.max() == 149 and (v.Ldd == 5).sum() == 149   # 34 pits + 115 cells cut at the mask edge (lddmask)
    m.initialSecond()
    cpu = oracle.kinematicWave(f("ldd"), mask, v.ChannelAlpha, 0.6, v.ChanLength, v.DtRouting)
    v.sumDisDay = np.zeros(v.ChanQKin.size)
    v.ToChanM3RunoffDt = np.random.default_rng(3).uniform(0, 3000, v.ChanQKin.size)
    sub = oracle.RoutingSubstep(cpu, types.SimpleNamespace(**{k: (a.copy() if isinstance(a, np.ndarray) else a)
                                                                 for k, a in vars(v).items()}))
    sub.v.InvChannelAlpha2 = sub.v.ChannelAlpha2 = None
    for s in range(v.NoRoutSteps):
        m.dynamic(s)
        sub.dynamic(split=False)
    m.step_end()
    close(v.ChanQKin, sub.v.ChanQKin)
    close(v.ChanQAvg, sub.v.sumDisDay / v.NoRoutSteps)
    close(v.TotalCrossSectionArea, sub.v.ChanM3Kin * v.InvChanLength)


def _structures_module(amd, g, engine_order):
    v = amd.routing.var_from_fixture(g)
    v.ChanQ = g["init_ChanQ"].copy()
    v.InvNoRoutSteps = 1 / v.NoRoutSteps
    for k in ("downstruct", "LakeIndex", "LakeAreaCC", "LakeFactor", "LakeFactorSqr", "ReservoirIndex", "QInM3Old",
              "QDelta", "UpTrans", "TotalReservoirStorageM3CC", "ConservativeStorageLimitCC", "NormalStorageLimitCC",
              "FloodStorageLimitCC", "Normal_FloodStorageLimitCC", "MinReservoirOutflowCC", "NormalReservoirOutflowCC",
              "NonDamagingReservoirOutflowCC", "DeltaO", "DeltaLN", "DeltaNFL"):
        setattr(v, k, g[k])
    for k in ("LakeStorageM3", "LakeInflowOldCC", "LakeOutflowCC", "LakeStorageM3BalanceCC", "LakeLevelCC",
              "ReservoirStorageM3", "TransCum"):
        setattr(v, k, g["init_" + k].copy())
    v.TransPower1, v.TransPower2, v.TransSub = float(g["TransPower1"]), float(g["TransPower2"]), float(g["TransSub"])
    m = amd.routing.routing(v, options=dict(SplitRouting=True, InitLisflood=False, simulateLakes=True,
                                            simulateReservoirs=True, inflow=True, TransLoss=True),
                            engine_order=engine_order)
    m.attach_router(g["codes_cut"], g["mask"])
    m.attach_structures()
    return v, m


_STRUCT_KEYS = ("ChanQKin", "ChanM3Kin", "Chan2QKin", "Chan2M3Kin", "ChanQ", "sumDisDay", "QLakeOutM3Dt", "QResOutM3Dt",
                "LakeStorageM3CC", "LakeOutflowCC", "LakeInflowOldCC", "LakeStorageM3BalanceCC", "LakeLevelCC",
                "ReservoirStorageM3CC", "ReservoirFillCC", "QInDt", "QinADDEDM3", "TransLossM3Dt", "TransCum")


@pytest.mark.parametrize("engine_order", [False, True])
def test_routing_with_inloop_structures_golden(amd, solver, engine_order):
    """routing.dynamic with lakes, reservoirs, inflow hydrographs and transmission loss inside the loop
    (routing.py:441-478), all on the device, against vectors captured from the reference's own modules
    (lakes.py, reservoir.py, inflow.py, transmission.py driven by routing.dynamic) on LF_ETRS89's 5 lake and
    64 reservoir sites.  engine_order=True also puts the structures' uncut links into the graph."""
    g = golden("inloop_structures")
    v, m = _structures_module(amd, g, engine_order)
    sampled = g["sampled"].tolist()
    for s in range(v.NoRoutSteps):
        v.ToChanM3RunoffDt = g["ToChanM3RunoffDt"][s]
        m.dynamic(s)
        if s in sampled:
            i = sampled.index(s)
            for k in _STRUCT_KEYS:
                # volumes of 1e6..1e8 m3: the 1e-9 relative bar, with the Newton tolerance scaled by DtRouting as atol
                np.testing.assert_allclose(getattr(v, k), g["out_" + k][i], rtol=RTOL, atol=1e-8, err_msg=str((s, k)))
    assert (v.LakeStorageM3[g["LakeIndex"]] == v.LakeStorageM3CC).all()


def test_fused_wavefront_skips_only_true_fixed_points(amd, monkeypatch):
    """Non-channel land pixels are isolated nodes of the channel router; the wavefront leaves them untouched while
    their state is +0.0 and their parameters are regular.  Against the sub-step-by-sub-step engine (which skips
    nothing) on a 30 %-channel scenario where some non-channel pixels still hold water, some have alpha = 0
    (1/alpha = inf: the reference's arithmetic turns their zero state into NaN) and some a split-routing threshold."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.kinematic_wave_parallel import kinematicWave
    from lisflood_amd.routing import _OUT, _STATE
    from bench_support import RoutingStepDevice
    H, W = 60, 70
    N = H * W
    values, sc, mask, _, ldd_kin = syn.hotpath_scenario(H, W)
    rng = np.random.default_rng(3)
    non = np.nonzero(~values["IsChannelKinematic"])[0]
    wet, odd, thr = non[:20], non[20:30], non[30:40]
    values["ChanQKin"][wet] = rng.uniform(1, 9, wet.size)
    values["ChanM3Kin"][wet] = values["ChannelAlpha"][wet] * values["ChanLength"][wet] * values["ChanQKin"][wet] ** sc["Beta"]
    values["ChannelAlpha"][odd] = 0.0
    with np.errstate(divide="ignore"):
        values["InvChannelAlpha"] = 1 / values["ChannelAlpha"]
    values["QLimit"][thr] = 3.0
    values["SideflowChanM3"] = syn.lateral_inflow(N, 0) * values["ChanLength"] * sc["DtRouting"]
    kw = kinematicWave(ldd_kin, mask, values["ChannelAlpha"], sc["Beta"], values["ChanLength"], sc["DtRouting"],
                       alpha_floodplains=values["ChannelAlpha2"])
    nsteps = int(sc["NoRoutSteps"])
    res = {}
    for mode in ("fused", "sequential", "fused_noskip"):
        if mode == "fused_noskip":
            monkeypatch.setenv("LF_NO_INERT_SKIP", "1")
        st = RoutingStepDevice(kw, values, True, sc["Beta"], 1 / sc["DtRouting"], sc["DtSec"])
        for _ in range(2):
            (st.run_sequential if mode == "sequential" else st.run_fused)(nsteps)
        res[mode] = {k: st.download(k) for k in _STATE + _OUT}
        st.free()
    for k in _STATE + _OUT:
        assert np.array_equal(res["fused"][k], res["sequential"][k], equal_nan=True), k
        assert np.array_equal(res["fused"][k], res["fused_noskip"][k], equal_nan=True), k
    assert np.isnan(res["fused"]["ChanQKin"][odd]).all() and (res["fused"]["ChanQKin"][wet] > 0).all()
    assert (res["fused"]["ChanQKin"][non[40:]] == 0).all()
    kw.close()


@pytest.mark.parametrize("family,shape", [("shallow", (1500, 1500)), ("deep", (500, 1100))])
def test_fused_wavefront_equals_sequential_mid_size(amd, family, shape):
    """2.25e6 / 5.5e5 cells, 20 % non-channel pixels (isolated, partly inert), 12 split-routing sub-steps: the wavefront
    (packed or 2-D grid, inert pixels skipped) against 12 x lf_routing_substep -- every state and output vector
    bit for bit, and the discharge sum grows by exactly the ChanQ of every sub-step."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd import ldd as L
    from lisflood_amd.kinematic_wave_parallel import kinematicWave
    from lisflood_amd.routing import _OUT, _STATE
    from bench_support import RoutingStepDevice
    H, W = shape
    N = H * W
    mask = np.ones((H, W), bool)
    codes = syn.make_ldd(family, H, W, 5).reshape(-1).astype(np.float64)
    rng = np.random.default_rng(23)
    is_chan = rng.random(N) < 0.8
    kin, _ = L.lddmask(codes, mask, is_chan)
    ldd_kin = np.zeros(N); ldd_kin[is_chan] = kin
    p = syn.router_params(N, seed=12)
    beta, dt, nsteps = p["beta"], 3600.0, 12
    alpha, length = p["alpha"], p["dx"]
    alpha2 = alpha * rng.uniform(1.2, 2.0, N)
    q0 = np.where(is_chan, p["Q0"], 0.0)
    qlimit = 2.0 * q0 * rng.uniform(0.3, 1.2, N)
    vals = dict(ChanLength=length, InvChanLength=1 / length, ChannelAlpha=alpha, InvChannelAlpha=1 / alpha,
                ChannelAlpha2=alpha2, InvChannelAlpha2=1 / alpha2, QLimit=qlimit, M3Limit=alpha * length * qlimit ** beta,
                Chan2M3Start=alpha2 * length * qlimit ** beta, Chan2QStart=qlimit * 0.1, PixelArea=np.full(N, 2.5e7),
                IsChannelKinematic=is_chan, SideflowChanM3=syn.lateral_inflow(N, 0) * length * dt)
    vals["Chan2M3Kin"] = vals["Chan2M3Start"].copy()
    vals["ChanM3Kin"] = alpha * length * q0 ** beta
    vals["ChanQKin"] = q0.copy()
    vals["Chan2QKin"] = (vals["Chan2M3Kin"] / length / alpha2) ** (1 / beta)
    kw = kinematicWave(ldd_kin, mask, alpha, beta, length, dt, alpha_floodplains=alpha2)
    a = RoutingStepDevice(kw, vals, True, beta, 1 / dt, dt * nsteps); a.run_fused(nsteps)
    b = RoutingStepDevice(kw, vals, True, beta, 1 / dt, dt * nsteps); b.run_sequential(nsteps)
    for k in _STATE + _OUT:
        assert np.array_equal(a.download(k), b.download(k), equal_nan=True), (family, k)
    q = a.download("ChanQ")
    assert np.isfinite(q).all() and (q >= 0).all() and (q[~is_chan] == 0).all() and q[is_chan].max() > 0
    assert (a.download("sumDisDay") >= q).all()          # the sum holds the last sub-step's ChanQ plus 11 non-negative ones
    a.free(); b.free(); kw.close()


def test_structures_inside_the_fused_wavefront(amd, solver):
    """lf_routing_substeps_fused_structures: the whole loop `for s: lakes/reservoirs/inflow/transmission
    .dynamic_inloop(s); routing.dynamic(s)` as ONE wavefront (sites run between two launches, on a graph that puts
    the cells draining into a structure on the structure's level).  With the same runoff in every sub-step (the
    model's case) it must be bit-identical to the sub-step-by-sub-step engine, for every state and output vector,
    and use ~NoRoutSteps x fewer launches."""
    g = golden("inloop_structures")
    va, ma = _structures_module(amd, g, True)
    vb, mb = _structures_module(amd, g, True)
    runoff = g["ToChanM3RunoffDt"][0]
    va.ToChanM3RunoffDt = runoff
    vb.ToChanM3RunoffDt = runoff
    for s in range(va.NoRoutSteps):
        ma.dynamic(s)
    seq_launches = ma.river_router.last_launches()["launches"]
    mb.dynamic_fused()
    for k in _STRUCT_KEYS + ("CrossSection2Area", "Sideflow1Chan", "FlowVelocity", "TravelDistance", "LakeStorageM3",
                             "ReservoirStorageM3", "LakeInflowCC", "ReservoirInflowCC"):
        assert np.array_equal(getattr(va, k), getattr(vb, k)), k
    fused = mb.river_router.last_launches()["launches"]
    # (both paths run on level blocks: ~NL / 16 + NoRoutSteps launches for the whole model step, ~NL / 16 per sub-step)
    assert fused < 2 * (mb.river_router.graph.num_levels + va.NoRoutSteps) and seq_launches * va.NoRoutSteps > 2 * fused
    # a second model step continues from the state of the first
    for s in range(va.NoRoutSteps):
        ma.dynamic(s)
    mb.dynamic_fused()
    for k in ("ChanQ", "sumDisDay", "LakeStorageM3CC", "ReservoirStorageM3CC", "TransCum"):
        assert np.array_equal(getattr(va, k), getattr(vb, k)), k
    # the plain sweeps refuse a graph with structure links
    with pytest.raises(amd.lib.LisfloodAmdError):
        mb.river_router.kinematicWaveRouting(np.zeros(mb.river_router.num_pixels), np.zeros(mb.river_router.num_pixels))


@pytest.mark.parametrize("family,time_major", [("deep", "0"), ("shallow", "0"), ("shallow", "1")])
def test_fused_wavefront_with_a_sideflow_vector_per_substep(amd, monkeypatch, family, time_major):
    """lf_routing_substeps_fused(sideflow_stride = N): every sub-step of the model step reads its own sideflow vector,
    against the sub-steps one by one with that vector uploaded before each -- bit for bit (cones, level kernel, time-major)."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.kinematic_wave_parallel import kinematicWave
    from lisflood_amd.routing import _STATE, _OUT
    from bench_support import RoutingStepDevice
    monkeypatch.setenv("LF_FUSED_TIME_MAJOR", time_major)
    H, W = (200, 240) if family == "deep" else (500, 600)
    N = H * W
    nsteps = 9
    codes = syn.make_ldd(family, H, W, 4)
    mask = np.ones((H, W), bool)
    p = syn.router_params(N, seed=22)
    vals, dt = syn.model_step_values(N, p)
    kw = kinematicWave(codes[mask].astype(np.float64), mask, p["alpha"], p["beta"], p["dx"], dt,
                       alpha_floodplains=vals["ChannelAlpha2"])
    sides = [syn.lateral_inflow(N, 70 + s) * p["dx"] * dt for s in range(nsteps)]
    a = RoutingStepDevice(kw, dict(vals, SideflowChanM3=sides[0]), True, p["beta"], 1.0 / dt, dt * nsteps)
    b = RoutingStepDevice(kw, dict(vals, SideflowChanM3=sides[0]), True, p["beta"], 1.0 / dt, dt * nsteps)
    for s in range(nsteps):
        a.dev["SideflowChanM3"].upload(np.ascontiguousarray(sides[s][a.perm]))
        a.run_sequential(1)
    b.run_fused_sideflow_per_substep(sides)
    # (the fused call keeps ChanQ / Sideflow1Chan / CrossSection2Area of the last sub-step only -- what the sequence leaves)
    for k in _STATE + [x for x in _OUT if x not in ("scratch0", "scratch1")]:
        assert np.array_equal(a.download(k), b.download(k), equal_nan=True), (family, k)
    a.free(); b.free(); kw.close()


@pytest.mark.parametrize("family,time_major", [("deep", "0"), ("shallow", "0"), ("shallow", "1")])
def test_several_model_steps_in_one_wavefront(amd, monkeypatch, family, time_major):
    """lf_routing_model_steps_fused: four model steps of 24 split-routing sub-steps, each with its own sideflow vector, as
    ONE wavefront (the skew runs on across the model-step boundaries) against four calls of the one-model-step wavefront
    with the discharge sum zeroed in between -- every state vector and every model step's sum bit for bit; on the cones
    (deep), the level kernel (shallow) and the time-major form."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.kinematic_wave_parallel import kinematicWave
    from lisflood_amd.routing import _STATE, _OUT
    from bench_support import RoutingStepDevice
    monkeypatch.setenv("LF_FUSED_TIME_MAJOR", time_major)
    H, W = (260, 300) if family == "deep" else (600, 700)
    N = H * W
    nsteps, M = 24, 4
    codes = syn.make_ldd(family, H, W, 3)
    mask = np.ones((H, W), bool)
    p = syn.router_params(N, seed=21)
    vals, dt = syn.model_step_values(N, p)
    kw = kinematicWave(codes[mask].astype(np.float64), mask, p["alpha"], p["beta"], p["dx"], dt,
                       alpha_floodplains=vals["ChannelAlpha2"])
    sides = [syn.lateral_inflow(N, 40 + m) * p["dx"] * dt for m in range(M)]
    a = RoutingStepDevice(kw, dict(vals, SideflowChanM3=sides[0]), True, p["beta"], 1.0 / dt, dt * nsteps)
    b = RoutingStepDevice(kw, dict(vals, SideflowChanM3=sides[0]), True, p["beta"], 1.0 / dt, dt * nsteps)
    want = []
    for m in range(M):                                        # model step by model step
        a.dev["SideflowChanM3"].upload(np.ascontiguousarray(sides[m][a.perm]))
        a.dev["sumDisDay"].zero()
        a.run_fused(nsteps)
        want.append(a.download("sumDisDay"))
    got = b.run_model_steps(nsteps, sides)                    # the four of them in one wavefront
    for m in range(M):
        assert np.array_equal(got[m], want[m]), (family, m)
    for k in [x for x in _STATE + _OUT if x != "sumDisDay"]:
        assert np.array_equal(a.download(k), b.download(k), equal_nan=True), (family, k)
    assert np.isfinite(got).all() and got.max() > 0
    a.free(); b.free(); kw.close()


def test_inert_pixels_leave_the_same_sums_in_both_fused_forms(amd, monkeypatch):
    """Several model steps in one call on a domain with inert pixels (isolated non-channel pixels whose state is all
    +0.0): the time-major form (k_fused_level_steps) jumps such a pixel to the last sub-step of the call, the skewed form
    (fused_cell) runs the last sub-step of EVERY model step on it -- both must leave `sum + 0.0` in the sums of every
    model step, also when the caller did not zero them: -0.0 becomes +0.0, any other value stays (bit for bit, signs of
    zero included)."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd import ldd as L
    from lisflood_amd.kinematic_wave_parallel import kinematicWave
    from bench_support import RoutingStepDevice
    H, W = 600, 700
    N = H * W
    mask = np.ones((H, W), bool)
    codes = syn.make_ldd("shallow", H, W, 5).reshape(-1).astype(np.float64)
    rng = np.random.default_rng(23)
    is_chan = rng.random(N) < 0.8
    kin, _ = L.lddmask(codes, mask, is_chan)
    ldd_kin = np.zeros(N); ldd_kin[is_chan] = kin
    p = syn.router_params(N, seed=12)
    beta, dt, nsteps, M = p["beta"], 3600.0, 6, 3
    alpha, length = p["alpha"], p["dx"]
    alpha2 = alpha * rng.uniform(1.2, 2.0, N)
    q0 = np.where(is_chan, p["Q0"], 0.0)
    qlimit = 2.0 * q0 * rng.uniform(0.3, 1.2, N)
    vals = dict(ChanLength=length, InvChanLength=1 / length, ChannelAlpha=alpha, InvChannelAlpha=1 / alpha,
                ChannelAlpha2=alpha2, InvChannelAlpha2=1 / alpha2, QLimit=qlimit, M3Limit=alpha * length * qlimit ** beta,
                Chan2M3Start=alpha2 * length * qlimit ** beta, Chan2QStart=qlimit * 0.1, PixelArea=np.full(N, 2.5e7),
                IsChannelKinematic=is_chan, SideflowChanM3=syn.lateral_inflow(N, 0) * length * dt)
    vals["Chan2M3Kin"] = vals["Chan2M3Start"].copy()
    vals["ChanM3Kin"] = alpha * length * q0 ** beta
    vals["ChanQKin"] = q0.copy()
    vals["Chan2QKin"] = (vals["Chan2M3Kin"] / length / alpha2) ** (1 / beta)
    kw = kinematicWave(ldd_kin, mask, alpha, beta, length, dt, alpha_floodplains=alpha2)
    sums0 = np.zeros((M, N))
    sums0[:, ::3] = -0.0
    sums0[:, 1::3] = rng.uniform(1.0, 9.0, (M, sums0[:, 1::3].shape[1]))
    got = {}
    for tm in ("0", "1"):
        monkeypatch.setenv("LF_FUSED_TIME_MAJOR", tm)
        r = RoutingStepDevice(kw, vals, True, beta, 1 / dt, dt * nsteps)
        got[tm] = r.run_model_steps(nsteps, nmodel=M, sums0=sums0)
        r.free()
    same = got["0"].view(np.int64) == got["1"].view(np.int64)                  # bits: +0.0 and -0.0 differ
    assert same.all(), np.argwhere(~same)[:5]
    inert = ~is_chan                                                           # isolated, zero state, no sideflow
    assert inert.sum() > N // 10
    assert (got["1"][:, inert] == sums0[:, inert]).all() and not np.signbit(got["1"][:, inert]).any()
    kw.close()


@pytest.mark.parametrize("family", ["deep", "shallow"])
def test_structures_wavefront_mid_size_synthetic(amd, family):
    """2e5 cells, 16 lakes + 48 reservoirs + 32 inflow points + transmission loss, 24 split-routing sub-steps, two model
    steps: the wavefront with the structures inside against the sub-step-by-sub-step engine (itself pinned to the
    reference's modules by the LF_ETRS89 fixture) -- every vector bit for bit."""
    from lisflood_amd import synthetic as syn
    H, W = 400, 500
    N = H * W
    mask = np.ones((H, W), bool)
    codes = syn.make_ldd(family, H, W, 8).reshape(-1).astype(np.float64)
    p = syn.router_params(N, seed=4)
    rng = np.random.default_rng(31)
    beta, dt, nsteps = p["beta"], 3600.0, 24
    alpha, length = p["alpha"], p["dx"]
    alpha2 = alpha * rng.uniform(1.2, 2.0, N)
    qlimit = 2.0 * p["Q0"] * rng.uniform(0.3, 1.2, N)

    def module():
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
        d, cut = syn.structures_scenario(codes, (H, W), v.ChanQ, dt, n_lakes=16, n_res=48)
        for k, x in d.items():
            setattr(v, k, np.array(x, copy=True) if isinstance(x, np.ndarray) else x)
        m = amd.routing.routing(v, options=dict(SplitRouting=True, InitLisflood=False, simulateLakes=True,
                                                simulateReservoirs=True, inflow=True, TransLoss=True), engine_order=True)
        m.attach_router(cut, mask)
        m.attach_structures()
        return v, m

    (va, ma), (vb, mb) = module(), module()
    for step in range(2):
        va.sumDisDay = np.zeros(N); vb.sumDisDay = np.zeros(N)
        for s in range(nsteps):
            ma.dynamic(s)
        mb.dynamic_fused()
        for k in _STRUCT_KEYS + ("CrossSection2Area", "Sideflow1Chan", "LakeStorageM3", "ReservoirStorageM3"):
            assert np.array_equal(getattr(va, k), getattr(vb, k), equal_nan=True), (family, step, k)
    assert np.isfinite(va.ChanQ).all() and va.QLakeOutM3Dt.max() > 0 and va.QResOutM3Dt.max() > 0 and va.TransCum.max() > 0


@pytest.mark.parametrize("trans", ["scenario", "settings_defaults"])
def test_structures_mid_size_vs_oracle(amd, oracle, trans):
    """`settings_defaults`: TransPower1 = 2, TransSub = 0.3 (transmission.py:58-59 with the settings' default maps) on
    reaches some of which carry less than 0.09 m3/s, so (Q^0.5 - 0.3) is NEGATIVE there and its square is what the
    reference (numpy ** = C pow) computes -- the fast pow of the loss must not turn that into NaN.  ONE sub-step there, by
    the wavefront and by the sub-step-by-sub-step engine: the loss 0.6 sqrt(Q) - 0.09 has an unbounded derivative at Q = 0,
    so from the second sub-step on the 1e-11 rounding noise of a reach that has run dry (ChanQ = max(kin + kin2 - QLimit,
    0)) is a 1e-2 m3 difference of its loss -- in the reference's arithmetic as much as in any other.
    The device's structures + routing sub-step loop against the C oracle (itself 0 ulp from the reference's modules
    on the LF_ETRS89 fixture) on a 1.2e5-cell synthetic network with 12 lakes, 36 reservoirs, inflow points and
    transmission loss: 24 sub-steps, every state vector within the parity tolerance."""
    from lisflood_amd import synthetic as syn
    H, W = 300, 400
    N = H * W
    mask = np.ones((H, W), bool)
    codes = syn.make_ldd("deep", H, W, 11).reshape(-1).astype(np.float64)
    p = syn.router_params(N, seed=7)
    rng = np.random.default_rng(37)
    beta, dt, nsteps = p["beta"], 3600.0, (24 if trans == "scenario" else 1)
    alpha, length = p["alpha"], p["dx"]
    alpha2 = alpha * rng.uniform(1.2, 2.0, N)
    qlimit = 2.0 * p["Q0"] * rng.uniform(0.3, 1.2, N)

    def var():
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
        d, cut = syn.structures_scenario(codes, (H, W), v.ChanQ, dt, n_lakes=12, n_res=36)
        for k, x in d.items():
            setattr(v, k, np.array(x, copy=True) if isinstance(x, np.ndarray) else x)
        if trans == "settings_defaults":
            v.TransPower1, v.TransPower2, v.TransSub = 2.0, 0.5, 0.3
            dry = np.random.default_rng(41).choice(N, 4000, replace=False)
            v.UpTrans = v.UpTrans.copy(); v.UpTrans[dry] = True
            for k in ("ChanQ", "ChanQKin"):
                x = getattr(v, k).copy(); x[dry] = np.linspace(0.0, 0.09, dry.size, endpoint=False); setattr(v, k, x)
            v.ChanM3Kin = alpha * length * v.ChanQKin ** beta
        return v, cut

    vg, cut = var()
    m = amd.routing.routing(vg, options=dict(SplitRouting=True, InitLisflood=False, simulateLakes=True,
                                             simulateReservoirs=True, inflow=True, TransLoss=True), engine_order=True)
    m.attach_router(cut, mask)
    m.attach_structures()
    m.dynamic_fused()
    vc, _ = var()
    kw = oracle.kinematicWave(cut, mask, alpha, beta, length, dt, alpha_floodplains=alpha2)
    st, sub = oracle.InloopStructures(vc), oracle.RoutingSubstep(kw, vc)
    for s in range(nsteps):
        st.dynamic_inloop(s)
        sub.dynamic(split=True, sideflow_m3=vc.SideflowChanM3)
    # transmission loss = (Q - (Q^p2 - sub)^p1) * dt is a difference of nearly equal numbers: its absolute error is a few
    # ulp of Q * dt whatever the loss itself is, so that is the scale of its tolerance
    cancel = 256 * np.finfo(float).eps * float(np.max(vc.ChanQ)) * dt
    for k in _STRUCT_KEYS:
        atol = cancel * (nsteps if k == "TransCum" else 1) if k in ("TransLossM3Dt", "TransCum") else 1e-6
        np.testing.assert_allclose(getattr(vg, k), getattr(vc, k), rtol=RTOL, atol=atol, err_msg=k)
    assert vc.QLakeOutM3Dt.max() > 0 and vc.QResOutM3Dt.max() > 0 and vc.TransCum.max() > 0
    assert np.isfinite(vg.TransCum).all() and np.isfinite(vg.ChanQ).all()
    if trans == "settings_defaults":
        assert vc.TransCum.min() < 0          # the negative-base branch was taken (loss below zero on the dry reaches)
        v2, _ = var()                         # the same sub-step by lf_inloop_structures + lf_routing_substep
        m2 = amd.routing.routing(v2, options=dict(SplitRouting=True, InitLisflood=False, simulateLakes=True,
                                                  simulateReservoirs=True, inflow=True, TransLoss=True), engine_order=True)
        m2.attach_router(cut, mask)
        m2.attach_structures()
        m2.dynamic(0)
        for k in _STRUCT_KEYS:
            assert np.array_equal(getattr(v2, k), getattr(vg, k), equal_nan=True), k


@pytest.mark.parametrize("with_structures", [False, True])
def test_routing_module_compact_domain(amd, with_structures):
    """routing(..., engine_order=True, compact=True): the 70 % of the land pixels that are not channel pixels (isolated,
    zero state) are left out of the router's domain.  Every vector must equal the full-domain module's, for the
    sub-step-by-sub-step calls and for the wavefront, with and without lakes / reservoirs / inflow / transmission loss."""
    from lisflood_amd import synthetic as syn
    H, W = 60, 80
    N = H * W
    values, sc, mask, _, ldd_kin = syn.hotpath_scenario(H, W)
    st, cut = syn.structures_scenario(ldd_kin, (H, W), values["ChanQ"], sc["DtRouting"], n_lakes=3, n_res=6)
    codes = cut if with_structures else ldd_kin
    runoff = syn.lateral_inflow(N, 3) * values["ChanLength"] * sc["DtRouting"]

    def module(compact):
        v = types.SimpleNamespace(**{k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in values.items()
                                     if k in amd.routing._STATIC + amd.routing._STATE})
        v.Beta, v.InvBeta, v.DtRouting, v.InvDtRouting = sc["Beta"], 1 / sc["Beta"], sc["DtRouting"], 1 / sc["DtRouting"]
        v.DtSec, v.NoRoutSteps, v.InvNoRoutSteps = sc["DtSec"], int(sc["NoRoutSteps"]), 1 / sc["NoRoutSteps"]
        v.ToChanM3RunoffDt = runoff
        opts = dict(SplitRouting=True, InitLisflood=False)
        if with_structures:
            for k, a in st.items():
                setattr(v, k, np.array(a, copy=True) if isinstance(a, np.ndarray) else a)
            opts.update(simulateLakes=True, simulateReservoirs=True, inflow=True, TransLoss=True)
        m = amd.routing.routing(v, options=opts, engine_order=True, compact=compact)
        m.attach_router(codes, mask)
        if with_structures:
            m.attach_structures()
        return v, m

    keys = amd.routing._STATE + amd.routing._OUT + (list(_STRUCT_KEYS[6:]) if with_structures else [])
    for fused in (False, True):
        (va, ma), (vb, mb) = module(False), module(True)
        assert mb.river_router.num_pixels < 0.5 * ma.river_router.num_pixels
        for step in range(2):
            va.sumDisDay = np.zeros(N); vb.sumDisDay = np.zeros(N)
            for v, m in ((va, ma), (vb, mb)):
                if fused:
                    m.dynamic_fused()
                else:
                    for s in range(v.NoRoutSteps):
                        m.dynamic(s)
            for k in keys:
                assert np.array_equal(getattr(va, k), getattr(vb, k), equal_nan=True), (fused, step, k)
        assert np.isfinite(va.ChanQ).all() and va.ChanQ.max() > 0


def test_pixel_aggregates_golden(amd):
    """opensealed.dynamic -> soil.dynamic_perpixel -> groundwater.dynamic as one device pass, against vectors
    captured from the reference's own module methods (two consecutive steps)."""
    from lisflood_amd import pixel_aggregates as PA
    g = golden("pixel_aggregates")
    v = types.SimpleNamespace(SoilFraction=g["SoilFraction"], SoilDepthTotal=g["SoilDepthTotal"],
                              InvDtDay=float(g["InvDtDay"]))
    for k in g.files:
        if k.startswith("static_"):
            setattr(v, k[7:], g[k])
        elif k.startswith("init_"):
            setattr(v, k[5:], g[k].copy())
    for s in range(2):
        v.TimeSinceStart = float(s + 3)
        for k in g.files:
            if k.startswith("in%d_" % s):
                setattr(v, k[4:], g[k])
        PA.dynamic(v)
        for k in g.files:
            if k.startswith("out%d_" % s):
                np.testing.assert_allclose(getattr(v, k[5:]), g[k], rtol=1e-12, atol=1e-13, err_msg=k)


def test_resident_hot_path_equals_the_module_classes(amd):
    """HotPathDevice (every stage of a model step chained on device buffers) against the same stages run through
    the module classes on host `var` arrays (each of which is pinned to the reference by its own golden test).
    Same kernels, same order: the results must be bit-identical."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd import pixel_aggregates as PA
    from lisflood_amd.hotpath import HotPathDevice
    from lisflood_amd.soilloop import soilloop
    from lisflood_amd.surface_routing import surface_routing
    H, W = 40, 50
    N = H * W
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    hp = HotPathDevice({k: np.array(a, copy=True) for k, a in values.items()}, sc, mask, ldd_to_chan, ldd_kin, split=True)
    # the same scenario through the module classes
    v = _model_var(N)
    for k, a in values.items():
        setattr(v, k, np.array(a, copy=True))
    for k, a in sc.items():
        setattr(v, k, a)
    v.InvBeta, v.InvPixelLength, v.InvDtSec = 1 / v.Beta, 1 / v.PixelLength, 1 / v.DtSec
    v.InvDtRouting, v.InvNoRoutSteps = 1 / v.DtRouting, 1 / v.NoRoutSteps
    m_soil = soilloop(v); m_soil.initial()
    m_surf = surface_routing(v); m_surf.initialSecond(ldd_to_chan, mask)
    m_rout = amd.routing.routing(v, split_routing=True); m_rout.attach_router(ldd_kin, mask)
    fs = [syn.hotpath_forcing(N, step) for step in range(3)]
    for step in range(3):
        f = fs[step]
        hp.step(f, time_since_start=step + 1)
        if step == 0:
            hp.prefetch(fs[1])          # uploaded on the copy stream while step 0 runs; step 2 uploads inside step()
        for k, a in f.items():
            setattr(v, k, a)
        v.TimeSinceStart = float(step + 1)
        m_soil.dynamic_canopy(); m_soil.dynamic_soil()
        PA.dynamic(v)
        m_surf.dynamic()
        v.sumDisDay = np.zeros(N)
        m_rout.dynamic_fused()
        m_rout.step_end()
        for k in ("W1a", "W2", "UZ", "Infiltration", "LZ", "DirectRunoff", "UZOutflowPixel", "OFQOther", "ToChanM3RunoffDt",
                  "ChanQKin", "Chan2QKin", "ChanM3Kin", "ChanQ"):
            assert np.array_equal(hp.download(k), np.asarray(getattr(v, k)), equal_nan=True), (step, k)
        assert np.array_equal(hp.chan_q_avg(), v.ChanQAvg)
        assert np.isfinite(v.ChanQAvg).all() and v.ChanQAvg.max() > 0
    hp.free()


def test_resident_hot_path_with_structures(amd):
    """The resident chain with lakes, reservoirs, inflow points and transmission loss inside the channel wavefront
    against the module classes stepping the same loop sub-step by sub-step (lf_inloop_structures + one sweep)."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd import pixel_aggregates as PA
    from lisflood_amd.hotpath import HotPathDevice
    from lisflood_amd.soilloop import soilloop
    from lisflood_amd.surface_routing import surface_routing
    H, W = 48, 60
    N = H * W
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    st, cut = syn.structures_scenario(ldd_kin, (H, W), values["ChanQ"], sc["DtRouting"], n_lakes=3, n_res=5)
    st["QInM3Old"][:] = 0; st["QDelta"][:] = 0
    pts = np.nonzero(values["IsChannelKinematic"])[0][::37]
    st["QInM3Old"][pts] = 5e3; st["QDelta"][pts] = 40.0
    cp = lambda d: {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}
    hp = HotPathDevice(cp(values), sc, mask, ldd_to_chan, cut, split=True, structures=cp(st))
    v = _model_var(N)
    for k, a in list(cp(values).items()) + list(sc.items()) + list(cp(st).items()):
        setattr(v, k, a)
    v.InvBeta, v.InvPixelLength, v.InvDtSec = 1 / v.Beta, 1 / v.PixelLength, 1 / v.DtSec
    v.InvDtRouting, v.InvNoRoutSteps = 1 / v.DtRouting, 1 / v.NoRoutSteps
    m_soil = soilloop(v); m_soil.initial()
    m_surf = surface_routing(v); m_surf.initialSecond(ldd_to_chan, mask)
    m_rout = amd.routing.routing(v, options=dict(SplitRouting=True, InitLisflood=False, simulateLakes=True,
                                                 simulateReservoirs=True, inflow=True, TransLoss=True), engine_order=True)
    m_rout.attach_router(cut, mask)
    m_rout.attach_structures()
    for step in range(2):
        f = syn.hotpath_forcing(N, step)
        hp.step(f, time_since_start=step + 1)
        for k, a in f.items():
            setattr(v, k, a)
        v.TimeSinceStart = float(step + 1)
        m_soil.dynamic_canopy(); m_soil.dynamic_soil()
        PA.dynamic(v)
        m_surf.dynamic()
        v.sumDisDay = np.zeros(N)
        for s in range(int(v.NoRoutSteps)):
            m_rout.dynamic(s)
        for k in ("ToChanM3RunoffDt", "ChanQKin", "Chan2QKin", "ChanM3Kin", "ChanQ", "sumDisDay"):
            assert np.array_equal(hp.download(k), np.asarray(getattr(v, k)), equal_nan=True), (step, k)
        for k in ("LakeStorageM3CC", "LakeOutflowCC", "ReservoirStorageM3CC", "ReservoirFillCC", "QLakeOutM3Dt",
                  "QResOutM3Dt", "TransCum", "QinADDEDM3"):
            assert np.array_equal(hp.download_site(k), np.asarray(getattr(v, k))), (step, k)
        assert np.isfinite(v.ChanQ).all() and v.ReservoirStorageM3CC.min() >= 0
    hp.free()


def test_resident_hot_path_vs_oracle_chain(amd, oracle):
    """The whole resident model step -- canopy, soil columns, per-pixel aggregates, overland routing, 24 split-routing
    sub-steps with lakes / reservoirs / inflow / transmission loss in the wavefront, compact channel domain -- against
    the same chain assembled from the C oracle (independent code, each piece 0-2 ulp from the reference's own methods):
    two model steps, every state vector within the parity tolerance."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.hotpath import HotPathDevice
    H, W = 48, 60
    N = H * W
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    st, cut = syn.structures_scenario(ldd_kin, (H, W), values["ChanQ"], sc["DtRouting"], n_lakes=3, n_res=5)
    cp = lambda d: {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}
    hp = HotPathDevice(cp(values), sc, mask, ldd_to_chan, cut, split=True, structures=cp(st))
    v = types.SimpleNamespace()
    for k, a in list(cp(values).items()) + list(sc.items()) + list(cp(st).items()):
        setattr(v, k, np.ascontiguousarray(a, dtype=np.float64) if isinstance(a, np.ndarray) and a.dtype.kind == "f" else a)
    v.InvBeta, v.InvPixelLength, v.InvDtSec = 1 / v.Beta, 1 / v.PixelLength, 1 / v.DtSec
    v.InvDtRouting, v.InvNoRoutSteps, v.NoRoutSteps = 1 / v.DtRouting, 1 / v.NoRoutSteps, int(v.NoRoutSteps)
    idx = np.arange(3)
    surf = oracle.SurfaceRouting(v, ldd_to_chan, mask)
    kw = oracle.kinematicWave(cut, mask, v.ChannelAlpha, v.Beta, v.ChanLength, v.DtRouting, alpha_floodplains=v.ChannelAlpha2)
    stru, sub = oracle.InloopStructures(v), oracle.RoutingSubstep(kw, v)
    for step in range(2):
        f = syn.hotpath_forcing(N, step)
        hp.step(f, time_since_start=step + 1)
        for k, a in f.items():
            setattr(v, k, a)
        oracle.canopy(v, idx)                                                      # Lisflood_dynamic.py:114
        d = dict(vars(v))
        d["ESMax"] = np.ascontiguousarray(v.ESRef * v.LAITerm)
        d.update(index_landuse_all=idx, is_irrigated=np.array([False, False, True]), is_paddy_irrig=np.zeros(3, bool),
                 paddy_inactive=np.zeros((1, N), bool))
        oracle.soil_columns(d)                                                     # :123
        v.TimeSinceStart = float(step + 1)
        oracle.pixel_aggregates(v)                                                 # :129-149
        surf.dynamic()                                                             # :165
        v.sumDisDay = np.zeros(N)
        for s in range(v.NoRoutSteps):                                             # :179-180
            stru.dynamic_inloop(s)
            sub.dynamic(split=True, sideflow_m3=v.SideflowChanM3)
        for k in ("W1a", "W1b", "W2", "UZ", "Infiltration", "CumInterception", "LZ", "DirectRunoff", "OFQOther",
                  "OFQDirect", "ToChanM3RunoffDt", "ChanQKin", "Chan2QKin", "ChanM3Kin", "ChanQ", "sumDisDay"):
            got, want = hp.download(k), np.asarray(getattr(v, k))
            np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-9 * max(1.0, float(np.abs(want).max())), err_msg=(step, k))
        for k in ("LakeStorageM3CC", "ReservoirStorageM3CC", "LakeOutflowCC"):
            np.testing.assert_allclose(hp.download_site(k), getattr(v, k), rtol=1e-8, err_msg=(step, k))
    assert np.isfinite(v.ChanQ).all() and v.ChanQ.max() > 0
    hp.free()


def test_hot_path_in_surface_order_equals_pixel_order(amd):
    """HotPathDevice(surface_order=True) keeps the non-channel vectors in the sweep order of the overland routers' graph (the
    routers then stream them); every downloaded vector and the state file equal the pixel-order object's bit for bit, with
    forcing passed in pixel order and, already permuted, with ordered=True."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.hotpath import HotPathDevice
    H, W = 44, 52
    N = H * W
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    cp = lambda d: {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}
    a = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True, surface_order=False)
    b = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True, surface_order=True)
    c = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True, surface_order=True)
    assert a.pixel_of_position is None and sorted(b.pixel_of_position.tolist()) == list(range(N))
    for s in range(3):
        f = syn.hotpath_forcing(N, s)
        a.step(f, s + 1)
        b.step(f, s + 1)
        c.step({k: np.ascontiguousarray(x[c.pixel_of_position]) for k, x in f.items()}, s + 1, ordered=True)
    for k in a.state_names() + ["sumDisDay", "Infiltration", "ToChanM3RunoffDt", "Theta1a", "OFM3Other", "TotalRunoff"]:
        want = a.download(k)
        assert np.array_equal(want, b.download(k), equal_nan=True), k
        assert np.array_equal(want, c.download(k), equal_nan=True), k
    assert np.abs(a.download("OFQOther")).max() > 0
    a.free(); b.free(); c.free()


@pytest.mark.parametrize("family,env", [("shallow", {"LF_FUSED_WIDE": "2000"}), ("river", {"LF_ROUTE_CONES": "0"})])
def test_static_records_of_the_wide_levels_leave_the_bits_alone(amd, oracle, monkeypatch, family, env):
    """The wide levels of an ordered beta = 3/5 call read (a, dx) of a cell as one 16-byte record instead of two loads
    (k_level<.., STATICS>, csrc/lf_sweep.h) and the contiguous upstream run two values per load: a layout of the router's
    own copies and an access pattern, not arithmetic.  Both sections of a router with floodplains, per-pixel channel
    lengths, four calls: with and without the records (LF_LEVEL_STATICS=1 / 0) bit for bit, and the oracle."""
    from lisflood_amd import _lib
    from lisflood_amd import synthetic as syn
    from lisflood_amd.kinematic_wave_parallel import Graph, kinematicWave
    H, W = 420, 380
    N = H * W
    codes = syn.make_ldd(family, H, W, 5)
    p = syn.router_params(N, seed=8)
    rng = np.random.default_rng(3)
    alpha2 = p["alpha"] * rng.uniform(1.2, 2.0, N)
    lat = [syn.lateral_inflow(N, i) for i in range(4)]
    for k, v in env.items():     # what makes levels of this small raster wide levels (k_level): above 2000 cells among the
        monkeypatch.setenv(k, v)  # level blocks, or above 1024 with one launch per level

    def run(statics):
        monkeypatch.setenv("LF_LEVEL_STATICS", statics)
        g = Graph(ldd_raster=codes)
        kw = kinematicWave(None, None, p["alpha"], p["beta"], p["dx"], p["dt"], alpha_floodplains=alpha2, graph=g)
        tmp = _lib.DeviceArray(N)
        out, wide = [], 0
        for section in ("main_channel", "floodplains"):
            Q = _lib.DeviceArray.from_host(p["Q0"])
            kw.to_engine_order(Q, tmp); Q.copy_from(tmp)
            for i in range(4):
                q = _lib.DeviceArray.from_host(lat[i])
                kw.to_engine_order(q, tmp); q.copy_from(tmp)
                kw.route_ordered(Q, q, section)
                q.free()
            wide = kw.last_launches()["wide"]
            kw.from_engine_order(Q, tmp)
            out.append(tmp.download().copy())
            Q.free()
        tmp.free(); kw.close()
        return out, wide
    (m1, f1), wide = run("1")
    assert wide >= 1, wide                                # the case is about the wide levels
    (m0, f0), _ = run("0")
    assert np.array_equal(m1, m0) and np.array_equal(f1, f0)
    mask = np.ones((H, W), bool)
    cpu = oracle.kinematicWave(codes.reshape(-1).astype(np.float64), mask, p["alpha"], p["beta"], p["dx"], p["dt"],
                               alpha_floodplains=alpha2)
    for got, section in ((m0, "main_channel"), (f0, "floodplains")):
        Q = p["Q0"].copy()
        for i in range(4):
            cpu.kinematicWaveRouting(Q, lat[i], section)
        close(got, Q, (family, section))


def test_block_length_chosen_per_graph_leaves_the_bits_alone(amd, monkeypatch):
    """lf_router_create times shorter level blocks for a graph whose default cone plan (blocks of 256 levels) fills less than
    40 % of its lanes -- the overland graph of a domain with few channel pixels: many short trees -- and keeps the fastest
    (tune_route_blocks, csrc/lf_router.hip).  The plan is a schedule, not arithmetic: the three overland routers swept
    together on the tuned plan, on the default plan (LF_ROUTE_TUNE=0) and one launch per level (LF_ROUTE_CONES=0) give the
    same bits; routers of one graph share the tuned length (they are swept together on one plan)."""
    from lisflood_amd import _lib
    from lisflood_amd import synthetic as syn
    from lisflood_amd.kinematic_wave_parallel import Graph, kinematicWave
    H = W = 1300
    N = H * W
    rng = np.random.default_rng(43)
    codes = syn.make_ldd("deep", H, W, 2)
    raster = np.where(rng.random((H, W)) < 0.04, np.uint8(5), codes)     # ifthenelse(IsChannel, 5, Ldd)
    p = syn.router_params(N, seed=12)
    q0 = [np.minimum(p["Q0"], 50.0) * rng.uniform(0, 1, N) for _ in range(3)]
    lat = [syn.lateral_inflow(N, i, hi=2e-5) for i in range(3)]

    def run(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g = Graph(ldd_raster=raster)
        kws = [kinematicWave(None, None, p["alpha"] * f, p["beta"], 5000.0, 86400.0, graph=g) for f in (1.0, 2.5, 0.4)]
        plans = [kw.route_plan_stats() for kw in kws]
        tmp = _lib.DeviceArray(N)
        qs, ls = [], []
        for kw, a, b in zip(kws, q0, lat):
            for host, dst in ((a, qs), (b, ls)):
                d = _lib.DeviceArray.from_host(host)
                kw.to_engine_order(d, tmp)
                d.copy_from(tmp)
                dst.append(d)
        for _ in range(2):
            kinematicWave.route_together(kws, qs, ls, engine_order=True)
        out = [d.download() for d in qs]
        launches = kws[0].last_launches()["launches"]
        for d in qs + ls + [tmp]:
            d.free()
        for kw in kws:
            kw.close()
        for k in env:
            monkeypatch.delenv(k)
        return out, plans, launches
    tuned, plans_t, launches_t = run({})
    default, plans_d, launches_d = run({"LF_ROUTE_TUNE": "0"})
    levels, _, launches_l = run({"LF_ROUTE_CONES": "0"})
    for a, b, c in zip(tuned, default, levels):
        assert np.array_equal(a, b) and np.array_equal(a, c) and np.isfinite(a).all()
    assert plans_d[0]["lane_use"] < 0.4                                    # the case the tuning is for
    assert plans_t[0]["blocks"] > plans_d[0]["blocks"] and plans_t[0]["lane_use"] > plans_d[0]["lane_use"]
    assert plans_t[0] == plans_t[1] == plans_t[2]                          # one graph, one plan
    assert launches_d <= launches_t < launches_l


def test_land_surface_in_one_pass_equals_the_three_launches(amd, solver):
    """lf_land_columns_device (canopy, ESMax = ESRef * LAITerm and the soil columns in ONE pass: the lane that runs a
    column's canopy carries LeafDrainage, Interception, W1a / W1b / W1 and ESMax into the column's soil water balance in
    registers) against lf_canopy_device + lf_scale_rows_device + lf_soil_columns_device, the launches of rounds 1-5: four
    model steps of the resident chain, every state vector and every canopy / soil output bit for bit -- both `pow` paths
    (the `solver` fixture), trip caps that send columns to the straggler kernel and keep them in the tile."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.hotpath import HotPathDevice
    from lisflood_amd import soilloop as SL
    H, W = 70, 90
    N = H * W
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    cp = lambda d: {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}
    a = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True, land_fused=False)
    b = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True, land_fused=True)
    assert b.land_fused and not a.land_fused and "land_surface" in b.stage_bytes() and "canopy" in a.stage_bytes()
    assert b.stage_bytes()["land_surface"] < a.stage_bytes()["canopy"] + a.stage_bytes()["soil_columns"]
    names = list(dict.fromkeys(a.state_names() + SL._CANOPY_IO + list(SL._V_IO) + ["sumDisDay", "Infiltration", "ToChanM3RunoffDt"]))
    for s in range(4):
        f = syn.hotpath_forcing(N, s)
        a.step(f, s + 1)
        if s == 2:
            ms = b.step_profile(f, s + 1)                     # the timed form takes the same path
            assert "land_surface" in ms and "canopy" not in ms
        else:
            b.step(f, s + 1)
        for k in names:
            assert np.array_equal(a.download(k), b.download(k), equal_nan=True), (s, k)
    import ctypes as C
    multi = C.c_int64(0)
    amd.lib.check(amd.lib.lib().lf_soil_last_deferred(C.c_int(0), C.byref(multi)))
    assert multi.value > 0                                    # some columns did take several Courant sub-steps
    a.free(); b.free()


def test_hot_path_with_unreported_maps_left_out(amd):
    """HotPathDevice(report=[...]): the optional maps (soil diagnostics, per-pixel diagnostics, cumulative sums of the
    mass-balance report) that are not asked for get no device vector, are not computed and their inputs are not streamed
    -- NULL pointers in lf_soil_args / lf_pixel_args.  Everything that exists must be the bits of the object that computes
    all of them: `dis`, every state vector, the reported maps; an unreported map cannot be downloaded."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.hotpath import HotPathDevice, OPTIONAL_MAPS
    H, W = 60, 70
    N = H * W
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    cp = lambda d: {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}
    full = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True)
    lean = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True, report=())
    some = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True, report=("Theta1aPixel", "ThetaAll", "TaCUM", "LZAvInflow"))
    with pytest.raises(ValueError):
        HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True, report=("ChanQ",))
    bytes_full, bytes_lean = full.stage_bytes(), lean.stage_bytes()
    assert bytes_lean["pixel_aggregates"] < 0.5 * bytes_full["pixel_aggregates"]
    land = lambda b: b["land_surface"] if "land_surface" in b else b["canopy"] + b["soil_columns"]     # (LF_LAND_FUSED=0)
    assert land(bytes_lean) < land(bytes_full)
    for s in range(3):
        f = syn.hotpath_forcing(N, s)
        for hp in (full, lean, some):
            hp.step(f, s + 1)
        assert np.array_equal(full.chan_q_avg(), lean.chan_q_avg()) and np.array_equal(full.chan_q_avg(), some.chan_q_avg())
        for hp in (lean, some):
            for k in hp.state_names() + ["sumDisDay", "Infiltration", "ToChanM3RunoffDt", "DirectRunoff", "UZOutflowPixel",
                                         "LZOutflowToChannelPixel", "TaInterception", "Ta"]:
                assert np.array_equal(full.download(k), hp.download(k), equal_nan=True), (s, k)
        for k in ("Theta1aPixel", "ThetaAll", "TaCUM", "LZAvInflow", "Theta1a", "LZInflowCUM"):
            assert np.array_equal(full.download(k), some.download(k), equal_nan=True), (s, k)
    gone = [k for k in OPTIONAL_MAPS if k not in lean.d]
    assert set(gone) == set(OPTIONAL_MAPS)
    assert "Sat1a" not in some.d and "Theta1b" not in some.d and "Theta1a" in some.d
    with pytest.raises(KeyError):
        lean.download("Sat1a")
    for hp in (full, lean, some):
        hp.free()


def test_hot_path_forcing_from_page_locked_buffers(amd):
    """HotPathDevice.pinned_forcing(): forcing vectors filled in place in page-locked host memory and prefetched (an
    asynchronous DMA) give the bits of the same vectors passed as ordinary arrays."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.hotpath import HotPathDevice
    H, W = 40, 50
    N = H * W
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    cp = lambda d: {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}
    a = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True)
    b = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True)
    bufs = [b.pinned_forcing() for _ in range(2)]
    for s in range(3):
        f = syn.hotpath_forcing(N, s)
        a.step(f, s + 1)
        for k, x in f.items():
            bufs[s % 2][k][:] = x
        b.prefetch(bufs[s % 2])
        b.step(bufs[s % 2], s + 1)
    for k in a.state_names() + ["sumDisDay", "Infiltration", "ToChanM3RunoffDt"]:
        assert np.array_equal(a.download(k), b.download(k), equal_nan=True), k
    # ONE page-locked set refilled in place for every step: upload_wait() (lf_upload_wait) is what makes the refill safe --
    # the DMA out of the arrays runs after prefetch() has returned
    one = bufs[0]
    for s in range(3, 7):
        f = syn.hotpath_forcing(N, s)
        a.step(f, s + 1)
        b.upload_wait()
        for k, x in f.items():
            one[k][:] = x
        b.prefetch(one)
        b.step(one, s + 1)
    for k in a.state_names() + ["sumDisDay", "Infiltration", "ToChanM3RunoffDt"]:
        assert np.array_equal(a.download(k), b.download(k), equal_nan=True), k
    a.free(); b.free()


def test_hot_path_float32_forcing_is_widened_on_the_device(amd):
    """Forcing vectors held as float32 (the reference's meteo files are float32) go over PCIe as float32 and are widened on
    the device: the bits of the same values widened on the host first."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.hotpath import HotPathDevice
    H, W = 40, 50
    N = H * W
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    cp = lambda d: {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}
    a = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True)
    b = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin, split=True)
    bufs = [b.pinned_forcing(np.float32) for _ in range(2)]
    for s in range(3):
        f32 = {k: x.astype(np.float32) for k, x in syn.hotpath_forcing(N, s).items()}
        a.step({k: x.astype(np.float64) for k, x in f32.items()}, s + 1)
        for k, x in f32.items():
            bufs[s % 2][k][:] = x
        b.prefetch(bufs[s % 2])
        b.step(bufs[s % 2], s + 1)
    for k in a.state_names() + ["sumDisDay", "Infiltration", "ToChanM3RunoffDt"]:
        assert np.array_equal(a.download(k), b.download(k), equal_nan=True), k
    a.free(); b.free()


def test_hot_path_warm_start(amd, tmp_path):
    """save_state after step 1 -> a fresh HotPathDevice + load_state must continue exactly like the original run
    (with lakes / reservoirs in the loop, so the site vectors travel too)."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.hotpath import HotPathDevice
    H, W = 48, 60
    N = H * W
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    st, cut = syn.structures_scenario(ldd_kin, (H, W), values["ChanQ"], sc["DtRouting"], n_lakes=3, n_res=5)
    cp = lambda d: {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}
    f = [syn.hotpath_forcing(N, s) for s in range(3)]
    a = HotPathDevice(cp(values), sc, mask, ldd_to_chan, cut, split=True, structures=cp(st))
    a.step(f[0], 1)
    a.save_state(str(tmp_path / "state.npz"))
    a.step(f[1], 2); a.step(f[2], 3)
    b = HotPathDevice(cp(values), sc, mask, ldd_to_chan, cut, split=True, structures=cp(st))
    b.load_state(str(tmp_path / "state.npz"))
    b.step(f[1], 2); b.step(f[2], 3)
    for k in a.state_names() + ["sumDisDay", "Infiltration", "ToChanM3RunoffDt"]:
        assert np.array_equal(a.download(k), b.download(k), equal_nan=True), k
    for k in ("LakeStorageM3CC", "ReservoirStorageM3CC", "LakeOutflowCC", "TransCum"):
        assert np.array_equal(a.download_site(k), b.download_site(k)), k
    # a state file carries what the object that wrote it reports: one written without the optional maps warm-starts an
    # object that reports them (they are recomputed every step; the cumulative sums restart), and the other way round
    lean = HotPathDevice(cp(values), sc, mask, ldd_to_chan, cut, split=True, structures=cp(st), report=())
    lean.load_state(str(tmp_path / "state.npz"))
    lean.step(f[1], 2)
    lean.save_state(str(tmp_path / "lean.npz"))
    lean.step(f[2], 3)
    c = HotPathDevice(cp(values), sc, mask, ldd_to_chan, cut, split=True, structures=cp(st))
    c.load_state(str(tmp_path / "lean.npz"))
    c.step(f[2], 3)
    for hp in (lean, c):
        assert np.array_equal(a.chan_q_avg(), hp.chan_q_avg())
        for k in ("W1a", "W1b", "W2", "UZ", "LZ", "ChanQKin", "Chan2QKin", "CumInterception", "DSLR", "CumInterSealed"):
            assert np.array_equal(a.download(k), hp.download(k), equal_nan=True), k
    a.free(); b.free(); lean.free(); c.free()


def test_interception_golden(amd):
    g = golden("interception")
    st = {k: g["in_" + k].copy() for k in ("Interception", "TaInterception", "LeafDrainage", "CumInterception")}
    for s in range(2):
        r = amd.soil.interception_water_balance(st["Interception"], st["TaInterception"], st["LeafDrainage"],
                                                st["CumInterception"], g["in_LAI"], g["in_Rain"],
                                                g["in_TaInterceptionMax"], float(g["in_drainageK"]))
        assert r is None
        for k in st:
            np.testing.assert_allclose(st[k], g["out%d_%s" % (s, k)], rtol=1e-12, atol=1e-14, err_msg=k)


def test_soil_columns_golden(amd, solver):
    from lisflood_amd import synthetic as syn
    g = golden("soil_columns")
    d = {k: (g["in_" + k].copy() if g["in_" + k].ndim else g["in_" + k][()]) for k in syn.SOIL_ARG_ORDER}
    for s in range(3):
        d["Rain"] = g["rains"][s].copy()
        assert amd.soil.soilColumnsWaterBalance(*[d[k] for k in syn.SOIL_ARG_ORDER]) is None
        for k in syn.SOIL_WRITTEN:
            np.testing.assert_allclose(d[k], g["out%d_%s" % (s, k)], rtol=1e-9, atol=1e-11, err_msg=(s, k))


def test_soil_columns_device_resident_vs_oracle(amd, oracle, solver):
    """Bigger ragged N (not a multiple of the block), paddy rows, 4 consecutive resident steps."""
    from lisflood_amd import synthetic as syn
    N = 100003
    d = syn.soil_params(N, seed=5)
    d["is_paddy_irrig"] = np.array([False, False, True])
    d["is_irrigated"] = np.array([False, True, True])
    inactive = np.random.default_rng(1).random((1, N)) < 0.5
    d["paddy_inactive"] = inactive
    ref = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in d.items()}
    dev = amd.soil.SoilColumnsDevice(d)
    for s in range(4):
        rain = np.random.default_rng(100 + s).uniform(0, 25, N)
        dev.set("Rain", rain)
        ref["Rain"] = rain
        dev.step()
        oracle.soil_columns(ref)
    for k in syn.SOIL_WRITTEN:
        np.testing.assert_allclose(dev.get(k), ref[k], rtol=1e-9, atol=1e-11, err_msg=k)
    # all-active paddy (no inactive pixel) -> the fraction is skipped entirely (soilloop.py:109-110)
    d2 = syn.soil_params(4096, seed=6)
    d2["is_paddy_irrig"] = np.array([False, True, False])
    d2["paddy_inactive"] = np.zeros((1, 4096), bool)
    r2 = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in d2.items()}
    amd.soil.soilColumnsWaterBalance(*[d2[k] for k in syn.SOIL_ARG_ORDER])
    oracle.soil_columns(r2)
    for k in syn.SOIL_WRITTEN:
        np.testing.assert_allclose(d2[k], r2[k], rtol=1e-9, atol=1e-11, err_msg=k)
    assert (d2["Theta1a"][1] == 0).all()


def test_soil_derived_parameters_recomputed_give_the_same_bits(amd, monkeypatch):
    """lf_soil_columns_device_derived (GenuInvM, WS1, WRes1, WFC1, WWP1 and the pore-space flags recomputed from the arrays
    soil.py:180-228 makes them of) against the streamed form on the same inputs, bit for bit; an array that does not
    follow the relation switches the object back to the streamed form."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.soilloop import derived_parameters_hold
    N = 20003
    d = syn.soil_params(N, seed=31)
    assert derived_parameters_hold(d)
    outs = []
    for no_derived in ("0", "1"):
        monkeypatch.setenv("LF_SOIL_NO_DERIVED", no_derived)
        dev = amd.soil.SoilColumnsDevice({k: (v.copy() if hasattr(v, "copy") else v) for k, v in d.items()})
        assert dev.derived
        for s in range(2):
            dev.step()
        outs.append({k: dev.get(k) for k in syn.SOIL_WRITTEN})
        for a in dev.dev.values():
            a.free()
    for k in syn.SOIL_WRITTEN:
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k
    d2 = dict(d)
    d2["WS1"] = d["WS1"] * (1 + 1e-15)
    assert not derived_parameters_hold(d2)
    dev = amd.soil.SoilColumnsDevice(d2)
    assert not dev.derived
    for a in dev.dev.values():
        a.free()


@pytest.mark.parametrize("N,V,L", [(1, 3, 3), (63, 1, 1), (255, 5, 2), (257, 4, 3), (777, 5, 2)])
def test_soil_columns_small_and_ragged_shapes(amd, oracle, N, V, L):
    """Tiles that are mostly empty, one column, vegetation fractions that share land-use rows (index_landuse_all with
    repeats), V != L: against the oracle, two steps (device-resident and through the 73-argument drop-in call)."""
    from lisflood_amd import synthetic as syn
    d = syn.soil_params(N, V=V, L=L, seed=41)
    ref = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in d.items()}
    host = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in d.items()}
    dev = amd.soil.SoilColumnsDevice(d)
    for s in range(2):
        dev.step()
        oracle.soil_columns(ref)
        amd.soil.soilColumnsWaterBalance(*[host[k] for k in syn.SOIL_ARG_ORDER])
    for k in syn.SOIL_WRITTEN:
        np.testing.assert_allclose(dev.get(k), ref[k], rtol=1e-9, atol=1e-11, err_msg=k)
        assert np.array_equal(dev.get(k), host[k], equal_nan=True), k          # derived / streamed parameters, device / host form
    for a in dev.dev.values():
        a.free()


def _soil_with_empty_pore_space(N, seed):
    """syn.soil_params with ThetaS == ThetaR (WS == WRes, pore-space flag set) in layers of a third of the columns: in 1b,
    2 or both, the water content above (by >= 1 mm), at and below WRes and KSat raised so that the columns need several
    Courant sub-steps (no soil evaporation or infiltration there: either can leave a layer a hair above WRes, at a huge
    Courant number); in
    1a (every fourth such column), which phase 1 clamps to WS1a == WRes1a: NaN, as in the oracle.  The derived parameter
    arrays are kept consistent (derived_parameters_hold)."""
    from lisflood_amd import synthetic as syn
    d = syn.soil_params(N, seed=seed)
    rng = np.random.default_rng(seed)
    lu = np.asarray(d["index_landuse_all"])
    cols = np.flatnonzero(rng.random(N) < 0.35)
    d["ESMax"][:, cols] = 0.0
    d["Rain"][cols] = d["SnowMelt"][cols] = d["LeafDrainage"][:, cols] = 0.0
    for j, col in enumerate(cols):
        layers = (("1b",), ("2",), ("1b", "2"), ("1a",))[j % 4]
        for name in layers:
            if d["SoilDepth" + name][0, col] == 0:
                continue
            d["WS" + name][:, col] = d["WRes" + name][:, col]
            d["KSat" + name][:, col] = rng.uniform(20.0, 60.0)
            delta = (rng.uniform(1.0, 5.0), 0.0, -rng.uniform(1.0, 5.0))[(j // 4) % 3]
            d["W" + name][:, col] = d["WRes" + name][lu, col] + delta
    for k in ("WS", "WRes", "WFC", "WWP"):
        d[k + "1"] = d[k + "1a"] + d[k + "1b"]
    for name in ("1a", "1b", "2"):
        d["PoreSpaceNotZero" + name] = (d["SoilDepth" + name] != 0) & (d["WS" + name] != 0)
    d["W1"] = d["W1a"] + d["W1b"]
    return d, cols


@pytest.mark.parametrize("no_derived", ["0", "1"])
@pytest.mark.parametrize("trip_cap", ["0", None])
def test_soil_columns_with_empty_pore_space(amd, oracle, monkeypatch, no_derived, trip_cap):
    """Layers with WS == WRes and the pore-space flag set (ThetaS == ThetaR != 0) in columns of several sub-steps: the
    saturation degree is the IEEE quotient (w - WRes) / 0 (+inf -> 1 above WRes, -inf -> 0 below, NaN at WRes) in every
    sub-step, as the oracle divides -- in the derived and the streamed parameter form, in the tile (LF_SOIL_TRIP_CAP=0)
    and in k_soil_stragglers (the default cap).  NaN exactly where the oracle has NaN."""
    import ctypes as C
    from lisflood_amd import synthetic as syn
    from lisflood_amd.soilloop import derived_parameters_hold
    N = 6007
    d, cols = _soil_with_empty_pore_space(N, seed=73)
    assert derived_parameters_hold(d)
    ref = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in d.items()}
    stats = np.zeros(4, np.int64)
    oracle.soil_columns(ref)
    oracle.lib().lfo_soil_stats(stats.ctypes.data_as(C.POINTER(C.c_int64)))
    assert 0 < stats[1] and stats[3] < 400, stats        # multi-sub-step columns, no runaway trip count
    assert np.isnan(ref["W1a"]).any() and np.isfinite(ref["W1a"][:, cols]).any()
    monkeypatch.setenv("LF_SOIL_NO_DERIVED", no_derived)
    if trip_cap is None:
        monkeypatch.delenv("LF_SOIL_TRIP_CAP", raising=False)
    else:
        monkeypatch.setenv("LF_SOIL_TRIP_CAP", trip_cap)
    dev = amd.soil.SoilColumnsDevice({k: (v.copy() if hasattr(v, "copy") else v) for k, v in d.items()})
    dev.step()       # one step: the sub-steps move water into layers below WRes, a second step would start a hair above it
    for k in syn.SOIL_WRITTEN:
        got, w = dev.get(k), ref[k]
        assert np.array_equal(np.isnan(got), np.isnan(w)), (k, np.flatnonzero(np.isnan(got) != np.isnan(w))[:5])
        np.testing.assert_allclose(got, w, rtol=1e-9, atol=1e-11, equal_nan=True, err_msg=k)
    for a in dev.dev.values():
        a.free()


def test_soil_pf_with_empty_pore_space(amd, oracle):
    """soilloop.soil_pf (lf_soil_pf_device) against the oracle on the columns of test_soil_columns_with_empty_pore_space
    (WS == WRes with the pore-space flag set: saturation 1, 0 or NaN) and ordinary ones."""
    from lisflood_amd.soilloop import soilloop
    N = 2003
    d, cols = _soil_with_empty_pore_space(N, seed=79)
    rng = np.random.default_rng(79)
    for name in ("1a", "1b", "2"):
        d["GenuInvAlpha" + name] = rng.uniform(20.0, 200.0, d["WS1a"].shape)
        d["GenuInvN" + name] = rng.uniform(0.71, 0.91, d["WS1a"].shape)
    d["HeadMax"] = 1e7
    want = oracle.soil_pf(d, d["index_landuse_all"], d["HeadMax"])
    v = _model_var(N)
    for k in ("W1a", "W1b", "W2") + tuple(k + n for k in ("WRes", "WS", "PoreSpaceNotZero", "GenuInvAlpha", "GenuInvM",
                                                               "GenuInvN") for n in ("1a", "1b", "2")):
        setattr(v, k, np.array(d[k], copy=True))
    v.HeadMax = d["HeadMax"]
    m = soilloop(v, options={"simulatePF": True}); m.initial()
    m.soil_pf()
    for k, w in zip(("pF0", "pF1", "pF2"), want):
        got = getattr(v, k)
        assert np.array_equal(np.isnan(got), np.isnan(w)), k
        np.testing.assert_allclose(got, w, rtol=1e-12, atol=1e-13, equal_nan=True, err_msg=k)
    assert np.isnan(want[0][:, cols]).any() or (want[0][:, cols] == 7.0).any()


@pytest.mark.parametrize("trip_cap", ["0", "1", "3", "6", "200"])
def test_soil_columns_same_bits_whatever_the_trip_cap(amd, monkeypatch, trip_cap):
    """Which columns leave their tile for k_soil_stragglers (LF_SOIL_TRIP_CAP: none, every multi-sub-step one -- more than
    a tile's 48 record slots hold, so the rest stay in the tile --, the default 6, the round-5 default 16, hardly any) must not
    change a single bit of any output: in-lane, in-tile and straggler columns run the same arithmetic.  The device context's
    workspace (lists, straggler records) is released in between (lf_device_trim) and rebuilt by the next call."""
    from lisflood_amd import synthetic as syn
    N = 30011
    d = syn.soil_params(N, seed=21)
    d["is_irrigated"] = np.array([False, True, True])
    outs = {}
    for cap in ("16", trip_cap):
        monkeypatch.setenv("LF_SOIL_TRIP_CAP", cap)
        dev = amd.soil.SoilColumnsDevice({k: (v.copy() if hasattr(v, "copy") else v) for k, v in d.items()})
        for s in range(3):
            dev.set("Rain", np.random.default_rng(50 + s).uniform(0, 30, N))
            dev.step()
        outs[cap] = {k: dev.get(k) for k in syn.SOIL_WRITTEN}
        for a in dev.dev.values():
            a.free()
        import ctypes as C
        amd.lib.check(amd.lib.lib().lf_device_trim(C.c_int(0)))
    for k in syn.SOIL_WRITTEN:
        assert np.array_equal(outs["16"][k], outs[trip_cap][k], equal_nan=True), k


def test_soil_columns_more_multi_substep_columns_than_a_round_holds(amd, oracle, solver):
    """Nearly saturated soil: most columns of every 256-column tile need several Courant sub-steps, more than the 128 the
    sub-step phase of k_soil_fused takes per round, so the later rounds (records rebuilt from the lanes' registers) run;
    frozen pixels and a skipped paddy fraction in the same tiles."""
    import ctypes as C
    from lisflood_amd import synthetic as syn
    N = 20011
    d = syn.soil_params(N, seed=11)
    lu = np.asarray(d["index_landuse_all"])
    rng = np.random.default_rng(12)
    for name in ("1a", "1b", "2"):                        # nearly saturated + 8 x KSat: ~99 % need several sub-steps, up to ~550
        d["W" + name] = d["WRes" + name][lu] + rng.uniform(0.985, 1.0, (3, N)) * (d["WS" + name][lu] - d["WRes" + name][lu])
        d["KSat" + name] = d["KSat" + name] * 8.0
    d["W1"] = d["W1a"] + d["W1b"]
    d["is_paddy_irrig"] = np.array([False, False, True])
    d["is_irrigated"] = np.array([False, True, True])
    d["paddy_inactive"] = np.random.default_rng(2).random((1, N)) < 0.7
    ref = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in d.items()}
    dev = amd.soil.SoilColumnsDevice(d)
    for s in range(2):
        dev.step()
        oracle.soil_columns(ref)
        if s == 0:
            nd = C.c_int64(0)
            amd.lib.check(amd.lib.lib().lf_soil_last_deferred(C.c_int(0), C.byref(nd)))
            assert nd.value > 0.6 * 2 * N, nd.value      # > 128 of 256 columns per tile on the two full fractions
    for k in syn.SOIL_WRITTEN:
        np.testing.assert_allclose(dev.get(k), ref[k], rtol=1e-9, atol=1e-11, err_msg=k)
    for a in dev.dev.values():
        a.free()


def test_soil_full_size_water_balance_property(amd):
    """Size-independent property at 2e6 pixels x 3 fractions (6e6 columns, beyond what the oracle does in seconds):
    every column closes its water balance over a step,
        d(W1a + W1b + W2 + UZ) = Infiltration - ESAct + PrefFlow - UZOutflow - GwPercUZLZ      (soilloop.py:131-354),
    storages stay inside [residual, saturated], fluxes are non-negative, frozen columns neither infiltrate nor seep,
    and columns that needed several Courant sub-steps (the second pass of the kernel) close as well as the others."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.soilloop import SoilColumnsDevice
    N = 2_000_000
    d = syn.soil_params(N, seed=9)
    dev = SoilColumnsDevice(d)
    store = lambda: sum(dev.get(k) for k in ("W1a", "W1b", "W2", "UZ"))
    for step in range(2):
        before = store()
        dev.step()
        after = store()
        flux = (dev.get("Infiltration") - dev.get("ESAct") + dev.get("PrefFlow") - dev.get("UZOutflow") - dev.get("GwPercUZLZ"))
        err = np.abs((after - before) - flux)
        assert err.max() < 1e-9, (step, float(err.max()))                 # storages are O(100) mm: ~1e-13 relative
        # (seepage between the layers may be negative: the reference limits it by the remaining capacity, which is
        #  below zero after an infiltration overflow into 1b -- soilloop.py:208-211, 280-285)
        for k in ("Infiltration", "ESAct", "PrefFlow", "UZOutflow", "GwPercUZLZ", "SeepSubToGW", "UZ"):
            assert (dev.get(k) >= 0).all(), k
        lu = np.asarray(d["index_landuse_all"])
        for w, lo in (("W1a", "WRes1a"), ("W1b", "WRes1b"), ("W2", "WRes2")):
            assert (dev.get(w) >= d[lo][lu] - 1e-9).all(), w
        assert (dev.get("W1a") <= d["WS1a"][lu] + 1e-9).all()
        frozen = np.asarray(d["isFrozenSoil"], bool)
        assert (dev.get("Infiltration")[:, frozen] == 0).all() and (dev.get("SeepSubToGW")[:, frozen] == 0).all()
    nd = __import__("ctypes").c_int64(0)
    amd.lib.check(amd.lib.lib().lf_soil_last_deferred(__import__("ctypes").c_int(0), __import__("ctypes").byref(nd)))
    assert nd.value > 0.05 * 3 * N          # the multi-sub-step pass really ran on a sizeable share of the columns
    hist = dev.substep_histogram()
    assert hist.sum() == nd.value and hist[0] == 0 and hist[1] == 0 and hist[2] > 0   # deferred = 2 or more sub-steps
    for a in dev.dev.values():
        a.free()


@pytest.mark.parametrize("family,seed,nblocks", [("shallow", 1, 3), ("deep", 2, 4), ("saddle", 6, 2)])
def test_row_block_partition_loopback(amd, oracle, solver, family, seed, nblocks):
    """The multi-GPU path on ONE GPU: nblocks row-block routers in this process, halo exchange by device copy
    instead of RCCL.  Same kernels (indexed sweep, pack), same plan; must match the single-domain oracle."""
    from lisflood_amd import dist as D
    from lisflood_amd import synthetic as syn
    H, W = 300, 260
    codes = syn.make_ldd(family, H, W, seed)
    mask = np.ones((H, W), bool)
    N = H * W
    p = syn.router_params(N, seed=5)
    cpu = oracle.kinematicWave(codes.reshape(-1).astype(np.float64), mask, p["alpha"], p["beta"], p["dx"], p["dt"])
    blocks = D.row_blocks(H, nblocks)
    graphs = [D.DistGraph(codes[r0:r1], None, codes[r0 - 1] if r0 > 0 else None, None,
                          codes[r1] if r1 < H else None, None) for (r0, r1) in blocks]
    nph = D.settle_phases_local(graphs)
    sl = [slice(r0 * W, r1 * W) for (r0, r1) in blocks]
    routers = [D.DistRouter(g, p["alpha"][s], p["beta"], p["dx"][s], p["dt"]) for g, s in zip(graphs, sl)]
    Qs = [r.new_state(p["Q0"][s]) for r, s in zip(routers, sl)]
    Qc = p["Q0"].copy()
    for step in range(3):
        q = syn.lateral_inflow(N, step)
        cpu.kinematicWaveRouting(Qc, q)
        lats = [r.new_state(q[s]) for r, s in zip(routers, sl)]
        D.loopback_route(routers, Qs, lats)
        got = np.concatenate([r.download_pix(Q) for r, Q in zip(routers, Qs)])
        close(got, Qc, (family, step))
    assert nph >= (nblocks if family == "deep" else 2)


@pytest.mark.parametrize("family,nblocks", [("deep", 3), ("shallow", 4)])
def test_row_block_routing_substep_loopback(amd, family, nblocks):
    """A whole routing.dynamic() sub-step (sideflow assembly, two router calls with their halo exchanges, fix-ups, sums)
    on the row-block partition -- nblocks routers on one GPU, exchange by device copy -- against lf_routing_substep on
    the whole raster: bit-identical state after 4 split-routing sub-steps."""
    from lisflood_amd import dist as D
    from lisflood_amd import synthetic as syn
    from lisflood_amd.kinematic_wave_parallel import Graph, kinematicWave
    from lisflood_amd.routing import _OUT, _STATE
    from bench_support import RoutingStepDevice
    H, W = 150, 130
    N = H * W
    codes = syn.make_ldd(family, H, W, 2 if family == "deep" else 1)
    p = syn.router_params(N, seed=6)
    rng = np.random.default_rng(19)
    beta, dt, nsteps = p["beta"], 3600.0, 4
    alpha, length = p["alpha"], p["dx"]
    alpha2 = alpha * rng.uniform(1.2, 2.0, N)
    qlimit = 2.0 * p["Q0"] * rng.uniform(0.3, 1.2, N)
    vals = dict(ChanLength=length, InvChanLength=1 / length, ChannelAlpha=alpha, InvChannelAlpha=1 / alpha,
                ChannelAlpha2=alpha2, InvChannelAlpha2=1 / alpha2, QLimit=qlimit, M3Limit=alpha * length * qlimit ** beta,
                Chan2M3Start=alpha2 * length * qlimit ** beta, Chan2QStart=qlimit * 0.1, PixelArea=np.full(N, 2.5e7),
                IsChannelKinematic=rng.random(N) < 0.9, SideflowChanM3=syn.lateral_inflow(N, 0) * length * dt)
    vals["Chan2M3Kin"] = vals["Chan2M3Start"].copy()
    vals["ChanM3Kin"] = alpha * length * p["Q0"] ** beta
    vals["ChanQKin"] = p["Q0"].copy()
    vals["Chan2QKin"] = (vals["Chan2M3Kin"] / length / alpha2) ** (1 / beta)
    # whole raster
    kw = kinematicWave(None, None, alpha, beta, length, dt, alpha_floodplains=alpha2, graph=Graph(ldd_raster=codes))
    ref = RoutingStepDevice(kw, vals, True, beta, 1 / dt, dt * nsteps)
    ref.run_sequential(nsteps)
    # row blocks
    blocks = D.row_blocks(H, nblocks)
    graphs = [D.DistGraph(codes[r0:r1], None, codes[r0 - 1] if r0 > 0 else None, None,
                          codes[r1] if r1 < H else None, None) for (r0, r1) in blocks]
    D.settle_phases_local(graphs)
    sl = [slice(r0 * W, r1 * W) for (r0, r1) in blocks]
    routers = [D.DistRouter(g, alpha[s], beta, length[s], dt, alpha_floodplains=alpha2[s]) for g, s in zip(graphs, sl)]
    steps = [D.DistRoutingStep(r, {k: (a[s] if isinstance(a, np.ndarray) else a) for k, a in vals.items()}, True, beta,
                               1 / dt, dt * nsteps) for r, s in zip(routers, sl)]
    for _ in range(nsteps):
        D.loopback_substep(steps)
    for k in _STATE + _OUT:
        got = np.concatenate([st.download(k) for st in steps])
        assert np.array_equal(got, ref.download(k), equal_nan=True), (family, k)
    # one block holding everything: the composite C entry point (no exchange needed, no communicator)
    g1 = D.DistGraph(codes, None, None, None, None, None)
    D.settle_phases_local([g1])
    one = D.DistRoutingStep(D.DistRouter(g1, alpha, beta, length, dt, alpha_floodplains=alpha2), vals, True, beta, 1 / dt,
                            dt * nsteps)
    for _ in range(nsteps):
        one.substep()
    for k in _STATE + _OUT:
        assert np.array_equal(one.download(k), ref.download(k), equal_nan=True), ("one block", k)
    for st in steps + [one]:
        st.free()
    ref.free()


@pytest.mark.parametrize("family,nparts", [("shallow", 3), ("deep", 4)])
def test_catchment_partition_routes_like_the_whole_domain(amd, family, nparts):
    """Ranks that own whole catchments need no exchange: nparts independent routers on compressed sub-domains give,
    pixel by pixel, exactly the discharge of the router on the whole raster (3 calls)."""
    from lisflood_amd import partition as P
    from lisflood_amd import synthetic as syn
    H, W = 240, 260
    N = H * W
    mask = np.ones((H, W), bool)
    codes = syn.make_ldd(family, H, W, 4).reshape(-1).astype(np.float64)
    p = syn.router_params(N, seed=2)
    whole = amd.kw.kinematicWave(codes, mask, p["alpha"], p["beta"], p["dx"], p["dt"])
    parts, counts = P.catchment_partition(codes, mask, nparts)
    assert counts.sum() == N and counts.min() > 0
    subs = [amd.kw.kinematicWave(c, m, p["alpha"][ids], p["beta"], p["dx"][ids], p["dt"]) for c, m, ids in parts]
    Qw = p["Q0"].copy()
    Qs = [p["Q0"][ids].copy() for _, _, ids in parts]
    for s in range(3):
        q = syn.lateral_inflow(N, s)
        whole.kinematicWaveRouting(Qw, q)
        got = np.empty(N)
        for kw, Q, (_, _, ids) in zip(subs, Qs, parts):
            kw.kinematicWaveRouting(Q, q[ids])
            got[ids] = Q
        assert np.array_equal(got, Qw), (family, s)


def test_fused_cones_random_cases(amd):
    """tools/stress_fused_cones.py: the wavefront on level blocks (cones, LDS exchange, deferred stores) against the
    per-level wavefront on random rasters / sub-step counts / block lengths (incl. blocks that have to shrink): every
    state vector bit-identical."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "stress_fused_cones.py"), "16", "11"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "different 0" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("family,seed", [("deep", 2), ("river", 7), ("shallow", 1)])
def test_cone_shapes_of_the_block_plan_agree(amd, monkeypatch, family, seed):
    """The switches of the level-block plan -- cells per level of a cone (one wavefront / a workgroup of four), levels per
    block (default, 7, one launch per level), for router calls, accuflux and the fused model step -- change the schedule,
    never a bit of the result.  (The defaults run everywhere else; this is where the other shapes run.)"""
    from lisflood_amd import synthetic as syn
    from lisflood_amd._lib import DeviceArray
    from lisflood_amd.kinematic_wave_parallel import Graph, kinematicWave
    from bench_support import RoutingStepDevice
    H, W = 330, 290
    N = H * W
    codes = syn.make_ldd(family, H, W, seed)
    p = syn.router_params(N, seed=3)
    vals, dt = syn.model_step_values(N, p, seed=11)
    x = np.random.default_rng(4).uniform(0, 2, N)

    def run(env):
        for k in ("LF_ROUTE_CONE_WIDTH", "LF_ROUTE_LEVELS", "LF_FUSED_CONE_WIDTH", "LF_FUSED_LEVELS", "LF_ROUTE_CONES"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g = Graph(ldd_raster=codes)
        kw = kinematicWave(None, None, p["alpha"], p["beta"], p["dx"], p["dt"], graph=g)
        perm = g.layout()[0].astype(np.int64)
        q = DeviceArray.from_host(np.ascontiguousarray(p["Q0"][perm]))
        for s in range(3):
            lat = DeviceArray.from_host(np.ascontiguousarray(syn.lateral_inflow(N, s)[perm]))
            kw.route_ordered(q, lat)
            lat.free()
        out = {"Q": q.download(), "launches": kw.last_launches()["launches"], "accu": kw.accuflux(x)}
        q.free()
        kw2 = kinematicWave(None, None, p["alpha"], p["beta"], p["dx"], dt, alpha_floodplains=vals["ChannelAlpha2"], graph=g)
        st = RoutingStepDevice(kw2, vals, True, p["beta"], 1 / dt, dt * 5)
        st.run_fused(5)
        out.update({k: st.download(k) for k in ("ChanQ", "ChanQKin", "Chan2QKin", "ChanM3Kin", "sumDisDay")})
        st.free(); kw2.close(); kw.close()
        return out

    ref = run({})
    for env in ({"LF_ROUTE_CONE_WIDTH": "256", "LF_FUSED_CONE_WIDTH": "64"}, {"LF_ROUTE_LEVELS": "7", "LF_FUSED_LEVELS": "5"},
                {"LF_ROUTE_CONES": "0", "LF_FUSED_LEVELS": "1"}):
        got = run(env)
        for k, a in ref.items():
            if k != "launches":
                assert np.array_equal(a, got[k], equal_nan=True), (family, env, k)
    monkeypatch.delenv("LF_ROUTE_CONES", raising=False)


@pytest.mark.parametrize("family", ["shallow", "deep", "river"])
def test_routers_on_one_graph_swept_together(amd, solver, family):
    """lf_router_route_device_multi: three routers on the same graph (different alpha, own vectors), one launch per level
    for all of them -- bit-identical to three separate sweeps, in pixel order and in engine order, over 3 calls."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd._lib import DeviceArray
    from lisflood_amd.kinematic_wave_parallel import Graph, kinematicWave
    H, W = 180, 140
    N = H * W
    codes = syn.make_ldd(family, H, W, 5)
    p = syn.router_params(N, seed=3)
    g = Graph(ldd_raster=codes)
    rng = np.random.default_rng(9)
    alphas = [p["alpha"] * f for f in (1.0, 0.6, 1.7)]
    kws = [kinematicWave(None, None, a, p["beta"], p["dx"], p["dt"], graph=g) for a in alphas]
    Q0 = [p["Q0"] * rng.uniform(0.5, 1.5, N) for _ in kws]
    for ordered in (False, True):
        qa = [DeviceArray.from_host(q) for q in Q0]
        qb = [DeviceArray.from_host(q) for q in Q0]
        for s in range(3):
            lat = [DeviceArray.from_host(syn.lateral_inflow(N, s) * f) for f in (1.0, 2.0, 0.5)]
            for kw, q, x in zip(kws, qa, lat):
                (kw.route_ordered if ordered else kw.route_device)(q, x)
            kinematicWave.route_together(kws, qb, lat, engine_order=ordered)
            for i in range(3):
                assert np.array_equal(qa[i].download(), qb[i].download()), (family, ordered, s, i)
            for x in lat:
                x.free()
        assert kws[0].last_launches()["launches"] <= g.num_levels + 1
        for d in qa + qb:
            d.free()
    for kw in kws:
        kw.close()


def test_overland_routers_where_they_route_sparse_channels(amd, oracle, solver):
    """surface_routing.py:104-113,151-153 on a domain where overland flow actually travels: 4 % of the pixels of a `deep`
    land LDD are channel pixels, LddToChan = lddrepair(ifthenelse(IsChannel, 5, Ldd)) -- a graph hundreds of levels deep
    instead of LF_ETRS89's all-pits one.  The three overland routers (direct / other / forest: own alpha, own discharge
    and inflow) are swept TOGETHER (lf_router_route_device_multi, three routers per cone) and compared with the oracle's
    three separate routers over three calls."""
    from lisflood_amd import ldd as L
    from lisflood_amd import synthetic as syn
    from lisflood_amd._lib import DeviceArray
    from lisflood_amd.kinematic_wave_parallel import Graph, kinematicWave
    H, W = 260, 200
    N = H * W
    mask = np.ones((H, W), bool)
    rng = np.random.default_rng(41)
    codes = syn.make_ldd("deep", H, W, 8)[mask].astype(np.float64)
    is_chan = rng.random(N) < 0.04
    ldd_to_chan = L.lddrepair(np.where(is_chan, float(L.PIT), codes), mask)
    g = Graph(ldd_to_chan, mask)
    assert g.num_levels > 40                                   # overland paths of dozens of cells, not all-pits
    p = syn.router_params(N, seed=12)
    alphas = [p["alpha"] * f for f in (1.0, 2.5, 0.4)]         # other / forest / direct differ in Manning's n only
    dt = 86400.0
    kws = [kinematicWave(None, None, a, p["beta"], 5000.0, dt, graph=g) for a in alphas]
    cpu = [oracle.kinematicWave(ldd_to_chan, mask, a, p["beta"], 5000.0, dt) for a in alphas]
    Q0 = [np.minimum(p["Q0"], 50.0) * rng.uniform(0.0, 1.0, N) for _ in kws]
    qd = [DeviceArray.from_host(q) for q in Q0]
    qc = [q.copy() for q in Q0]
    for s in range(3):
        lats = [syn.lateral_inflow(N, s, hi=2e-5) * f for f in (1.0, 2.0, 0.5)]
        ld = [DeviceArray.from_host(x) for x in lats]
        kinematicWave.route_together(kws, qd, ld)
        for c, q, x in zip(cpu, qc, lats):
            c.kinematicWaveRouting(q, x)
        for x in ld:
            x.free()
    for i in range(3):
        got = qd[i].download()
        np.testing.assert_allclose(got, qc[i], rtol=RTOL, atol=ATOL, err_msg="router %d" % i)
        assert (got[is_chan] >= 0).all()
    assert kws[0].last_launches()["launches"] < g.num_levels   # blocks of levels, three routers per launch
    for d in qd:
        d.free()
    for kw in kws:
        kw.close()


@pytest.mark.parametrize("nr", [2, 4])
def test_two_and_four_routers_per_cone(amd, solver, nr):
    """the cone kernels are instantiated for 1..4 routers on one graph (chunks of 4 levels, two supply wavefronts for more
    than one): 2 and 4 routers swept together on a `deep` graph equal their separate sweeps bit for bit, engine order and
    pixel order, two calls"""
    from lisflood_amd import synthetic as syn
    from lisflood_amd._lib import DeviceArray
    from lisflood_amd.kinematic_wave_parallel import Graph, kinematicWave
    H, W = 150, 120
    N = H * W
    g = Graph(ldd_raster=syn.make_ldd("deep", H, W, 6))
    p = syn.router_params(N, seed=4)
    rng = np.random.default_rng(10)
    factors = (1.0, 0.5, 2.2, 1.4)[:nr]
    kws = [kinematicWave(None, None, p["alpha"] * f, p["beta"], p["dx"], p["dt"], graph=g) for f in factors]
    Q0 = [p["Q0"] * rng.uniform(0.5, 1.5, N) for _ in kws]
    for ordered in (True, False):
        qa = [DeviceArray.from_host(q) for q in Q0]
        qb = [DeviceArray.from_host(q) for q in Q0]
        for s in range(2):
            lat = [DeviceArray.from_host(syn.lateral_inflow(N, s) * f) for f in factors]
            for kw, q, x in zip(kws, qa, lat):
                (kw.route_ordered if ordered else kw.route_device)(q, x)
            kinematicWave.route_together(kws, qb, lat, engine_order=ordered)
            for i in range(nr):
                assert np.array_equal(qa[i].download(), qb[i].download()), (nr, ordered, s, i)
            for x in lat:
                x.free()
        for d in qa + qb:
            d.free()
    for kw in kws:
        kw.close()


@pytest.mark.parametrize("family,nparts", [("deep", 3), ("river", 2)])      # (this river raster has two catchments)
def test_catchment_partition_model_step_fused(amd, family, nparts):
    """configs[4]'s workload shape on a partition: every part runs the FUSED wavefront (24 split-routing sub-steps, level
    blocks + cones) on its own whole catchments, no exchange -- state and outputs equal the whole-domain model step bit
    for bit, two model steps in a row."""
    from lisflood_amd import partition as P
    from lisflood_amd import synthetic as syn
    from lisflood_amd.kinematic_wave_parallel import kinematicWave
    from bench_support import RoutingStepDevice
    from test_full_size import model_step_values
    H, W = 300, 280
    N = H * W
    nsteps = 24
    mask = np.ones((H, W), bool)
    codes = syn.make_ldd(family, H, W, 9).reshape(-1).astype(np.float64)
    p = syn.router_params(N, seed=4)
    vals, dt = model_step_values(N, p, np.random.default_rng(23))
    side = [syn.lateral_inflow(N, s) * p["dx"] * dt for s in range(2)]
    keys = ("ChanQ", "ChanQKin", "Chan2QKin", "ChanM3Kin", "Chan2M3Kin", "sumDisDay", "CrossSection2Area")

    def run(c, m, ids):
        kw = kinematicWave(c, m, p["alpha"][ids], p["beta"], p["dx"][ids], dt, alpha_floodplains=vals["ChannelAlpha2"][ids])
        v = {k: (np.ascontiguousarray(x[ids]) if isinstance(x, np.ndarray) else x) for k, x in vals.items()}
        v["SideflowChanM3"] = np.ascontiguousarray(side[0][ids])
        st = RoutingStepDevice(kw, v, True, p["beta"], 1.0 / dt, dt * nsteps)
        st.run_fused(nsteps)
        st.dev["SideflowChanM3"].upload(np.ascontiguousarray(side[1][ids][st.perm]))
        st.dev["sumDisDay"].zero()
        st.run_fused(nsteps)
        out = {k: st.download(k) for k in keys}
        st.free(); kw.close()
        return out

    whole = run(codes, mask, np.arange(N))
    parts, counts = P.catchment_partition(codes, mask, nparts)
    assert counts.sum() == N and counts.min() > 0
    got = {k: np.empty(N) for k in keys}
    for c, m, ids in parts:
        o = run(c, m, ids)
        for k in keys:
            got[k][ids] = o[k]
    for k in keys:
        assert np.array_equal(got[k], whole[k]), (family, k)


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


def test_surface_routing_module_golden(amd, solver):
    """surface_routing.dynamic() (surface_routing.py:115-212) against vectors captured from the reference's own
    module method on an 18 x 24 LDD with 30 % channel pixels (overland routing between cells is exercised)."""
    from lisflood_amd.surface_routing import surface_routing
    g = golden("surface_step")
    N = int(g["mask"].sum())
    v = _model_var(N)
    v.Beta = float(g["Beta"]); v.InvBeta = 1 / v.Beta
    v.PixelLength, v.DtSec = float(g["PixelLength"]), float(g["DtSec"])
    v.InvPixelLength, v.InvDtSec = 1 / v.PixelLength, 1 / v.DtSec
    v.MMtoM3 = 0.001 * float(g["PixelArea"]); v.M3toMM = 1 / v.MMtoM3
    v.InvNoRoutSteps = 1 / float(g["NoRoutSteps"])
    v.IsChannel, v.OFAlpha, v.SoilFraction = g["IsChannel"], g["OFAlpha"], g["SoilFraction"]
    for k in ("OFQDirect", "OFQOther", "OFQForest"):
        setattr(v, k, g["init_" + k].copy())
    m = surface_routing(v)
    m.initialSecond(g["ldd_to_chan"], g["mask"])
    keys = ("OFQDirect", "OFQOther", "OFQForest", "OFM3Direct", "OFM3Other", "OFM3Forest", "SurfaceRunoff",
            "TotalRunoff", "OFToChanM3", "WaterDepth", "ToChanM3Runoff", "ToChanM3RunoffDt")
    for s in range(2):
        for k in ("AvailableWaterForInfiltration", "Infiltration", "DirectRunoff", "UZOutflowPixel",
                  "LZOutflowToChannelPixel"):
            setattr(v, k, g["in%d_%s" % (s, k)])
        m.dynamic()
        for k in keys:
            close(getattr(v, k), g["out%d_%s" % (s, k)], (s, k))


def test_soilloop_module_golden(amd, solver):
    """soilloop.dynamic_canopy() + dynamic_soil() (soilloop.py:519-704) against vectors captured from the
    reference's own class methods, two consecutive steps."""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.soilloop import soilloop
    g = golden("canopy_soil_step")
    N = g["init_W1a"].shape[1]
    v = _model_var(N)
    for k in g.files:
        if k.startswith("static_"):
            setattr(v, k[7:], g[k].copy())
        elif k.startswith("init_"):
            setattr(v, k[5:], g[k].copy())
    v.LeafDrainageK, v.DtDay = float(g["LeafDrainageK"]), float(g["DtDay"])
    v.InvDtDay = 1 / v.DtDay
    v.AvWaterThreshold, v.CourantCrit, v.DrainedFraction = (float(g["AvWaterThreshold"]), float(g["CourantCrit"]),
                                                           float(g["DrainedFraction"]))
    m = soilloop(v)
    m.initial()
    for s in range(2):
        for k in ("Rain", "EWRef", "ETRef", "ESRef"):
            setattr(v, k, g["forc%d_%s" % (s, k)])
        m.dynamic_canopy()
        for k in ("Interception", "TaInterception", "LeafDrainage", "CumInterception", "potential_transpiration",
                  "RWS", "Ta", "W1a", "W1b", "W1"):
            np.testing.assert_allclose(getattr(v, k), g["canopy%d_%s" % (s, k)], rtol=1e-9, atol=1e-11, err_msg=(s, k))
        m.dynamic_soil()
        for k in syn.SOIL_WRITTEN:
            np.testing.assert_allclose(getattr(v, k), g["soil%d_%s" % (s, k)], rtol=1e-9, atol=1e-11, err_msg=(s, k))


def test_soilloop_option_branches_golden(amd):
    """dynamic_canopy's option branches against the reference's own method with the options switched on
    (tests/golden/make_golden.py canopy_options): `wateruse` -> WFilla / WFillb of the irrigated fraction
    (soilloop.py:582-587), `repStressDays` -> SoilMoistureStressDays (:597-598); same inputs as canopy_soil_step's
    first step"""
    from lisflood_amd.soilloop import soilloop
    g, o = golden("canopy_soil_step"), golden("canopy_options")
    N = g["init_W1a"].shape[1]
    v = _model_var(N)
    for k in g.files:
        if k.startswith("static_"):
            setattr(v, k[7:], g[k].copy())
        elif k.startswith("init_"):
            setattr(v, k[5:], g[k].copy())
    v.LeafDrainageK, v.DtDay = float(g["LeafDrainageK"]), float(g["DtDay"])
    v.InvDtDay = 1 / v.DtDay
    v.SoilMoistureStressDays = np.full((3, N), -1.0)
    for k in ("Rain", "EWRef", "ETRef", "ESRef"):
        setattr(v, k, g["forc0_" + k])
    m = soilloop(v, options={"wateruse": True, "repStressDays": True})
    m.initial()
    m.dynamic_canopy()
    np.testing.assert_allclose(v.RWS, g["canopy0_RWS"], rtol=1e-9, atol=1e-11)
    assert np.array_equal(v.SoilMoistureStressDays, o["SoilMoistureStressDays"])
    assert v.WFilla.shape == (N,) and v.WFillb.shape == (N,)
    np.testing.assert_allclose(v.WFilla, o["WFilla"], rtol=1e-12)
    np.testing.assert_allclose(v.WFillb, o["WFillb"], rtol=1e-12)
    # without the options nothing of the kind is touched
    v2 = _model_var(N)
    for k in g.files:
        if k.startswith("static_"):
            setattr(v2, k[7:], g[k].copy())
        elif k.startswith("init_"):
            setattr(v2, k[5:], g[k].copy())
    v2.LeafDrainageK, v2.DtDay, v2.InvDtDay = v.LeafDrainageK, v.DtDay, v.InvDtDay
    v2.SoilMoistureStressDays = np.full((3, N), -1.0)
    for k in ("Rain", "EWRef", "ETRef", "ESRef"):
        setattr(v2, k, g["forc0_" + k])
    m2 = soilloop(v2)
    m2.initial()
    m2.dynamic_canopy()
    assert (v2.SoilMoistureStressDays == -1.0).all() and not hasattr(v2, "WFilla")


def test_soilloop_static_parameter_maps_are_uploaded_once_and_followed_when_they_change(amd):
    """the module classes keep the static [L,N] parameter maps on the device between calls (fingerprint check,
    BufferCache.put_static): a second call uploads none of them, a map that is recomputed is picked up"""
    from lisflood_amd import synthetic as syn
    from lisflood_amd import _lib
    from lisflood_amd.soilloop import soilloop
    g = golden("canopy_soil_step")
    N = g["init_W1a"].shape[1]

    def fresh():
        v = _model_var(N)
        for k in g.files:
            if k.startswith("static_"):
                setattr(v, k[7:], g[k].copy())
            elif k.startswith("init_"):
                setattr(v, k[5:], g[k].copy())
        v.LeafDrainageK, v.DtDay = float(g["LeafDrainageK"]), float(g["DtDay"])
        v.InvDtDay = 1 / v.DtDay
        v.AvWaterThreshold, v.CourantCrit, v.DrainedFraction = (float(g["AvWaterThreshold"]), float(g["CourantCrit"]),
                                                               float(g["DrainedFraction"]))
        for k in ("Rain", "EWRef", "ETRef", "ESRef"):
            setattr(v, k, g["forc0_" + k])
        m = soilloop(v)
        m.initial()
        return v, m
    v, m = fresh()
    uploads = []
    orig = _lib.DeviceArray.upload

    def counting(self, host):
        uploads.append(host.nbytes)
        return orig(self, host)
    _lib.DeviceArray.upload = counting
    try:
        m.dynamic_canopy(); m.dynamic_soil()
        first = sum(uploads)
        uploads.clear()
        m.dynamic_canopy(); m.dynamic_soil()
        second = sum(uploads)
    finally:
        _lib.DeviceArray.upload = orig
    assert second < 0.62 * first, (first, second)        # 40 of the ~75 staged arrays are parameter maps
    # a recomputed map is followed: KSat1a x 3 in place == a fresh module on the changed map
    v.KSat1a *= 3.0
    v3, m3 = fresh()
    m3.dynamic_canopy(); m3.dynamic_soil()
    m3.dynamic_canopy(); m3.dynamic_soil()
    v3.KSat1a *= 3.0
    m3._cache.static_uploads = False                      # the reference path: everything staged on every call
    m.dynamic_canopy(); m.dynamic_soil()
    m3.dynamic_canopy(); m3.dynamic_soil()
    for k in syn.SOIL_WRITTEN:
        assert np.array_equal(getattr(v, k), getattr(v3, k), equal_nan=True), k


def test_handles_created_after_a_fork():
    """SURVEY 8(b) threading row: the reference forks its Monte-Carlo / EnKF members (main.py:104-106); handles created
    in forked children (library loaded before the fork) and in the parent afterwards all work -- run in a fresh
    interpreter, this process has touched the device already"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "fork_worker.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "FORK_OK members=3" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_empty_inputs(amd):
    mask = np.zeros((3, 4), bool)
    kw = amd.kw.kinematicWave(np.zeros(0), mask, np.zeros(0), 0.6, 1000.0, 3600.0)
    Q = np.zeros(0)
    kw.kinematicWaveRouting(Q, np.zeros(0))
    assert kw.upstream_sum(np.zeros(0)).size == 0


def test_soil_pf_golden(amd):
    """soilloop.soil_pf (lf_soil_pf_device) against the pF values the reference's own dynamic_soil produced"""
    from lisflood_amd.soilloop import soilloop
    g = golden("soil_pf")
    N = g["W1a"].shape[1]
    v = _model_var(N)
    for k in g.files:
        if k not in ("pF0", "pF1", "pF2", "HeadMax"):
            setattr(v, k, g[k].copy())
    v.HeadMax = float(g["HeadMax"])
    m = soilloop(v, options={"simulatePF": True}); m.initial()
    m.soil_pf()
    for k in ("pF0", "pF1", "pF2"):
        np.testing.assert_allclose(getattr(v, k), g[k], rtol=1e-12, atol=1e-13, err_msg=k)
    assert (v.pF0 == 7.0).any() and (v.pF2 == -1.0).any()


@pytest.mark.parametrize("family", ["saddle", "shallow"])
def test_two_rank_rccl_halo_exchange(amd, family):
    """The multi-GPU transport itself: 2 processes, boundary discharge over RCCL Send/Recv (lf_dist_router_route) against
    the single-domain oracle.  With two visible devices, one GPU each over the real RCCL.  With one, RCCL refuses two ranks
    on the same device (test_real_rccl_gpu.py), so both ranks share it and the same Send/Recv calls go through the
    stand-in tests/fake_rccl (test_dist_multirank_gpu.py), which also checks that the two ranks issue them in matching
    order."""
    import subprocess
    import sys
    from lisflood_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if _lib.device_count() < 2:
        if os.path.join(root, "tests") not in sys.path:
            sys.path.insert(0, os.path.join(root, "tests"))
        import test_dist_multirank_gpu as M
        outs = M.run_ranks(M.fake_rccl_dir(), 2, "tests/dist_worker_rccl.py", {"LF_TEST_FAMILY": family})
        assert "DIST_RCCL_OK" in outs[0][0] and "ranks=2" in outs[0][0]
        return
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT="29561", TORCHELASTIC_RUN_ID="rccl%d" % os.getpid(), LF_TEST_FAMILY=family,
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "dist_worker_rccl.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, o[-2000:] + e[-2000:]
    assert "DIST_RCCL_OK" in outs[0][0]
