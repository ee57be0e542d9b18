"""Shared by tests/test_hotpath_members_gpu.py: the two element-wise ensemble stages (lf_pixel_aggregates_members_device,
lf_surface_step_members) run on member rows with padded strides and sentinels between the rows, beside the single calls on
each member's own copy."""
import ctypes as C

import numpy as np

from lisflood_amd import _lib
from lisflood_amd import pixel_aggregates as PA
from lisflood_amd import surface_routing as SR
from lisflood_amd.hotpath import OPTIONAL_MAPS, PA_READERS

SENTINEL = -777.25
PAD_V, PAD_N, PAD_F = 5, 3, 7        # elements between the members' [3,N] rows, [N] rows and forcing rows

PA_SHARED = ["SoilFraction", "SoilDepthTotal", "SMaxSealed", "DirectRunoffFraction", "WaterFraction", "LowerZoneK", "LZThreshold",
             "GwLossStep"]
PA_FORCING = ["Rain", "SnowMelt", "EWRef"]
PA_ROWS_V = [k for k in PA._V_IN if k not in PA_SHARED] + ["Theta"]
PA_ROWS_N = PA._STATE + PA._OUT
PA_OPTIONAL = [k for k in PA_ROWS_N + ["Theta"] if k in OPTIONAL_MAPS]
SR_SHARED = ["SoilFraction", "OFAlpha", "IsChannel"]
SR_ROWS_V = ["AvailableWaterForInfiltration", "Infiltration", "SurfaceRunSoil"]
SR_ROWS_N = [k for k in SR._N_IN if k != "IsChannel"] + SR._STATE + SR._OUT


def pixel_inputs(N, M, seed, forcing_per_member):
    """-> (shared name -> array, per member name -> array): random fields with the edges of the kernel in them -- pixels
    without any soil fraction (ThetaAll's 0 branch), LZ below its threshold, a loss that empties LZ, dry and wet forcing"""
    rng = np.random.default_rng(seed)
    frac = rng.dirichlet([3, 2, 1], N).T * rng.uniform(0.5, 1.0, N)
    frac[:, rng.random(N) < 0.05] = 0.0
    shared = dict(SoilFraction=frac, SoilDepthTotal=rng.uniform(300, 2000, (3, N)), SMaxSealed=rng.uniform(0.5, 1.5, N),
                  DirectRunoffFraction=rng.uniform(0, 0.15, N) * (rng.random(N) < 0.5),
                  WaterFraction=rng.uniform(0, 0.1, N) * (rng.random(N) < 0.3), LowerZoneK=rng.uniform(0.001, 0.05, N),
                  LZThreshold=rng.uniform(0, 60, N) * (rng.random(N) < 0.5), GwLossStep=rng.uniform(0, 3, N) * (rng.random(N) < 0.5))
    members = []
    for m in range(M):
        d = {k: rng.uniform(0, 10, (3, N)) * (rng.random((3, N)) < 0.8) for k in PA_ROWS_V if k != "Theta"}
        d["LZ"] = rng.uniform(0, 100, N)
        d["CumInterSealed"] = rng.uniform(0, 1.2, N)
        for k in PA._STATE[2:]:
            d[k] = rng.uniform(0, 5, N)
        members.append(d)
    forcing = []
    for m in range(M if forcing_per_member else 1):
        forcing.append(dict(Rain=rng.uniform(0, 20, N) * (rng.random(N) < 0.6), SnowMelt=rng.uniform(0, 2, N) * (rng.random(N) < 0.2),
                            EWRef=rng.uniform(0, 5, N)))
    for m in range(M):
        members[m].update(forcing[m if forcing_per_member else 0])
    return shared, members


def kept_of(report):
    """(outputs that exist, [3,N] inputs handed to the kernel) for report = None (all) or a set of optional maps"""
    if report is None:
        return set(PA_ROWS_N + ["Theta"]), set(PA._V_IN)
    keep = set(report) | ({"LZInflowCUM"} if "LZAvInflow" in report else set())
    outs = {k for k in PA_ROWS_N + ["Theta"] if k not in PA_OPTIONAL or k in keep}
    ins = {k for k in PA._V_IN if k not in PA_READERS or any(o in outs for o in PA_READERS[k])}
    return outs, ins


def rows_up(values, width, stride, device=0):
    """[M, width] host rows -> device vector of M rows `stride` apart, sentinels between them"""
    values = np.asarray(values, np.float64).reshape(len(values), width)
    host = np.full((values.shape[0], stride), SENTINEL)
    host[:, :width] = values
    return _lib.DeviceArray.from_host(host.reshape(-1), device)


def rows_down(d, M, width, stride):
    """-> ([M, width] rows, [M, stride - width] what lies between them)"""
    a = d.download().reshape(M, stride)
    return a[:, :width].copy(), a[:, width:].copy()


def run_pixel_single(shared, member, report, calls, N):
    """lf_pixel_aggregates_device on one member's own vectors, `calls` times -> per call name -> array"""
    outs, ins = kept_of(report)
    dev, a = {}, PA._PixelArgs()
    for k in PA._V_IN + PA._N_IN + PA_ROWS_N + ["Theta"]:
        if k in PA._V_IN and k not in ins or k in PA_ROWS_N + ["Theta"] and k not in outs:
            continue
        shape = (3, N) if k in PA._V_IN + ["Theta"] else (N,)
        host = shared[k] if k in shared else member.get(k, np.full(shape, SENTINEL))
        dev[k] = _lib.DeviceArray.from_host(np.ascontiguousarray(host, np.float64))
        setattr(a, k, dev[k].ptr.value)
    a.InvDtDay, a.N = 1.0, N
    got = []
    for s in range(calls):
        a.TimeSinceStart = float(s + 1)
        _lib.check(_lib.lib().lf_pixel_aggregates_device(0, C.byref(a)))
        got.append({k: dev[k].download() for k in outs})
    form = _lib.lib().lf_module_last_form(0, 0)
    for d in dev.values():
        d.free()
    return got, form


def run_pixel_members(shared, members, report, calls, N, forcing_per_member):
    """lf_pixel_aggregates_members_device on the member rows -> (per call name -> [M, ...] rows, gaps seen, form)"""
    M = len(members)
    outs, ins = kept_of(report)
    stride, pstride, fstride = 3 * N + PAD_V, N + PAD_N, N + PAD_F
    dev, a, layout = {}, PA._PixelArgs(), {}
    for k in PA._V_IN + PA._N_IN + PA_ROWS_N + ["Theta"]:
        if k in PA._V_IN and k not in ins or k in PA_ROWS_N + ["Theta"] and k not in outs:
            continue
        if k in shared:
            dev[k] = _lib.DeviceArray.from_host(np.ascontiguousarray(shared[k], np.float64))
        else:
            width, st = (3 * N, stride) if k in PA_ROWS_V else (N, fstride if k in PA_FORCING else pstride)
            rows = M if (k not in PA_FORCING or forcing_per_member) else 1
            dev[k] = rows_up([members[m].get(k, np.full(width, SENTINEL)) for m in range(rows)], width, st)
            layout[k] = (rows, width, st)
        setattr(a, k, dev[k].ptr.value)
    a.InvDtDay, a.N = 1.0, N
    got, gaps_ok = [], True
    for s in range(calls):
        a.TimeSinceStart = float(s + 1)
        _lib.check(_lib.lib().lf_pixel_aggregates_members_device(0, C.byref(a), M, stride, pstride, fstride if forcing_per_member else 0))
        out = {}
        for k, (rows, width, st) in layout.items():
            r, gap = rows_down(dev[k], rows, width, st)
            gaps_ok = gaps_ok and bool((gap == SENTINEL).all())
            if k in outs:
                out[k] = r.reshape((M, 3, N) if width == 3 * N else (M, N))
        got.append(out)
    form = _lib.lib().lf_module_last_form(0, 0)
    statics_ok = all(np.array_equal(dev[k].download().reshape(np.shape(shared[k])), shared[k]) for k in shared if k in dev)
    for d in dev.values():
        d.free()
    return got, gaps_ok and statics_ok, form


def surface_inputs(N, M, seed, values):
    """shared statics from the scenario's `values`, per member random runoff inputs and overland states"""
    rng = np.random.default_rng(seed)
    shared = dict(SoilFraction=np.asarray(values["SoilFraction"], np.float64), OFAlpha=np.asarray(values["OFAlpha"], np.float64),
                  IsChannel=np.ascontiguousarray(values["IsChannel"]).astype(np.uint8))
    members = []
    for m in range(M):
        d = dict(AvailableWaterForInfiltration=rng.uniform(0, 20, (3, N)), Infiltration=rng.uniform(0, 15, (3, N)),
                 DirectRunoff=rng.uniform(0, 4, N) * (rng.random(N) < 0.7), UZOutflowPixel=rng.uniform(0, 2, N),
                 LZOutflowToChannelPixel=rng.uniform(0, 1, N))
        for k in SR._STATE:
            d[k] = rng.uniform(0, 0.3, N) * (rng.random(N) < 0.9)
        members.append(d)
    return shared, members


def surface_scalars(a, sc, N):
    a.Beta, a.MMtoM3, a.M3toMM = sc["Beta"], sc["MMtoM3"], sc["M3toMM"]
    a.PixelLength, a.InvPixelLength = sc["PixelLength"], 1 / sc["PixelLength"]
    a.DtSec, a.InvDtSec, a.InvNoRoutSteps, a.N = sc["DtSec"], 1 / sc["DtSec"], 1 / sc["NoRoutSteps"], N


def run_surface_single(routers, shared, member, sc, calls, N):
    dev, a = {}, SR._SurfaceArgs()
    for k in SR_SHARED + SR_ROWS_V + SR_ROWS_N + ["scratch"]:
        shape = (3, N) if k in SR._V_IN + ["SurfaceRunSoil", "scratch"] else (N,)
        host = shared[k] if k in shared else member.get(k, np.full(shape, SENTINEL))
        dev[k] = _lib.DeviceArray.from_host(np.ascontiguousarray(host))
        setattr(a, k, dev[k].ptr.value)
    surface_scalars(a, sc, N)
    got = []
    for s in range(calls):
        _lib.check(_lib.lib().lf_surface_step_ordered(*[r._h for r in routers], C.byref(a)))
        got.append({k: dev[k].download() for k in SR_ROWS_V[2:] + SR._STATE + SR._OUT})
    form = _lib.lib().lf_module_last_form(0, 1)
    for d in dev.values():
        d.free()
    return got, form


def run_surface_members(routers, shared, members, sc, calls, N):
    M = len(members)
    stride, pstride = 3 * N + PAD_V, N + PAD_N
    dev, a, layout = {}, SR._SurfaceArgs(), {}
    for k in SR_SHARED + SR_ROWS_V + SR_ROWS_N:
        if k in shared:
            dev[k] = _lib.DeviceArray.from_host(np.ascontiguousarray(shared[k]))
        else:
            width, st = (3 * N, stride) if k in SR_ROWS_V else (N, pstride)
            dev[k] = rows_up([members[m].get(k, np.full(width, SENTINEL)) for m in range(M)], width, st)
            layout[k] = (width, st)
        setattr(a, k, dev[k].ptr.value)
    dev["scratch"] = _lib.DeviceArray.from_host(np.full(3 * M * pstride, SENTINEL))
    a.scratch = dev["scratch"].ptr.value
    surface_scalars(a, sc, N)
    got, gaps_ok = [], True
    for s in range(calls):
        _lib.check(_lib.lib().lf_surface_step_members(*[r._h for r in routers], C.byref(a), M, stride, pstride))
        out = {}
        for k, (width, st) in layout.items():
            r, gap = rows_down(dev[k], M, width, st)
            gaps_ok = gaps_ok and bool((gap == SENTINEL).all())
            if k in SR_ROWS_V[2:] + SR._STATE + SR._OUT:
                out[k] = r.reshape((M, 3, N) if width == 3 * N else (M, N))
        got.append(out)
    form = _lib.lib().lf_module_last_form(0, 1)
    if form == 2:                      # the [3][M][pstride] scratch rows: nothing written between them
        gaps_ok = gaps_ok and bool((dev["scratch"].download().reshape(3 * M, pstride)[:, N:] == SENTINEL).all())
    for d in dev.values():
        d.free()
    return got, gaps_ok, form
