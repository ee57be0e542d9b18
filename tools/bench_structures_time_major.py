"""A model step of channel routing WITH lakes, reservoirs, inflow hydrographs and transmission loss in the loop
(lf_routing_substeps_fused_structures, 24 split sub-steps) in its two forms, same process, the forms alternating: the skewed
wavefront (LF_FUSED_TIME_MAJOR=0) and the time-major form (=1; the switch is read per call).  Every repeat starts from the
same device state (restored by device-to-device copies), so the forms do the same arithmetic; several repeats each, so the
spread of one form is known.  Reports ms per model step and launches per form, and whether every device vector of the
step -- routing state, site vectors, dense in-loop vectors -- is bit-identical between the forms.

    python tools/bench_structures_time_major.py [--size 3000] [--repeats 5] [--calls 3] [--case shallow hotpath] [--json out.json]

  shallow  syn.make_ldd("shallow", size, size, 2) with the default structures_scenario (64 lakes + 192 reservoirs)
  hotpath  the channel network of syn.hotpath_scenario(size, size) with the same structures (compact domain)"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lisflood-code_amd"))
from lisflood_amd import _lib, synthetic as syn          # noqa: E402
from lisflood_amd import routing as R                     # noqa: E402
from lisflood_amd._lib import DeviceArray                 # noqa: E402

SWITCH = "LF_FUSED_TIME_MAJOR"
OPTIONS = dict(SplitRouting=True, InitLisflood=False, simulateLakes=True, simulateReservoirs=True, inflow=True, TransLoss=True)


def shallow_case(size, nsteps):
    H = W = size
    N = H * W
    codes = syn.make_ldd("shallow", H, W, 2).reshape(-1).astype(np.float64)
    p = syn.router_params(N)
    rng = np.random.default_rng(17)
    beta, dt = p["beta"], 3600.0
    alpha, length = p["alpha"], p["dx"]
    alpha2 = alpha * rng.uniform(1.2, 2.0, N)
    qlimit = 2.0 * p["Q0"] * rng.uniform(0.3, 1.2, N)
    v = types.SimpleNamespace(
        ChanLength=length, InvChanLength=1 / length, ChannelAlpha=alpha, InvChannelAlpha=1 / alpha, ChannelAlpha2=alpha2,
        InvChannelAlpha2=1 / alpha2, QLimit=qlimit, M3Limit=alpha * length * qlimit ** beta,
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
    d, cut = syn.structures_scenario(codes, (H, W), v.ChanQ, dt)
    for k, x in d.items():
        setattr(v, k, x)
    return v, cut, np.ones((H, W), bool), False


def hotpath_case(size, nsteps):
    H = W = size
    N = H * W
    values, sc, mask, _, ldd_kin = syn.hotpath_scenario(H, W, nsteps=nsteps, block=min(N, 1 << 18))
    st, cut = syn.structures_scenario(ldd_kin, (H, W), values["ChanQ"], sc["DtRouting"])
    v = types.SimpleNamespace(**{k: a for k, a in values.items() if k in R._STATIC + R._STATE})
    v.Beta, v.InvBeta, v.DtRouting, v.InvDtRouting = sc["Beta"], 1 / sc["Beta"], sc["DtRouting"], 1 / sc["DtRouting"]
    v.DtSec, v.NoRoutSteps, v.InvNoRoutSteps = sc["DtSec"], int(sc["NoRoutSteps"]), 1 / sc["NoRoutSteps"]
    v.ToChanM3RunoffDt = syn.lateral_inflow(N, 3) * values["ChanLength"] * sc["DtRouting"]
    for k, a in st.items():
        setattr(v, k, a)
    return v, cut, mask, True


def run_case(name, size, nsteps, repeats, calls):
    t_build = time.perf_counter()
    v, cut, mask, compact = (shallow_case if name == "shallow" else hotpath_case)(size, nsteps)
    m = R.routing(v, options=OPTIONS, engine_order=True, compact=compact)
    m.attach_router(cut, mask)
    m.attach_structures()
    m.begin_step()
    os.environ[SWITCH] = "0"
    m.dynamic_fused()                                   # leaves every argument block wired (and the site lists checked)
    L, r = _lib.lib(), m.river_router
    live = dict(m._dev)
    live.update(("structures." + k, a) for k, a in m._st["dev"].items())
    backup = {k: DeviceArray(a.shape, a.dtype, a.device).copy_from(a) for k, a in live.items()}
    level_start = r.graph.layout()[2]
    out = dict(case=name, size=size, nsteps=nsteps, cells=int(r.num_pixels), levels=int(r.graph.num_levels),
               widest_level=int(np.diff(level_start).max()), lakes=int(m._st["lakes"]), reservoirs=int(m._st["res"]),
               build_s=round(time.perf_counter() - t_build, 1), forms={})

    def restore():
        for k, a in live.items():
            a.copy_from(backup[k])

    def call():
        _lib.check(L.lf_routing_substeps_fused_structures(r._h, C.byref(m._args), C.byref(m._inloop), nsteps))

    results = {}
    for switch in ("0", "1"):                           # one call each from the same state: the bits
        os.environ[SWITCH] = switch
        restore()
        call()
        _lib.synchronize()
        results[switch] = {k: a.download() for k, a in live.items() if not k.startswith("scratch")}
        out["forms"][switch] = dict(form=r.last_fused_form(), launches=int(r.last_launches()["launches"]), ms=[])
    differing = [k for k in results["0"] if not np.array_equal(results["0"][k].view(np.uint8), results["1"][k].view(np.uint8))]
    out["bit_identical"], out["differing"] = not differing, differing
    out["time_major_applies"] = out["forms"]["1"]["form"] == "time-major"      # (no: chained sites or a shared cell)
    out["finite_chanq"] = float(np.isfinite(results["1"]["ChanQ"]).mean())
    del results
    for rep in range(repeats):                          # the forms alternating
        for switch in ("0", "1"):
            os.environ[SWITCH] = switch
            restore()
            _lib.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            _lib.synchronize()
            out["forms"][switch]["ms"].append(round((time.perf_counter() - t0) * 1e3 / calls, 3))
    for f in out["forms"].values():
        f["ms_per_model_step"] = float(np.median(f["ms"]))
        f["spread_ms"] = round(max(f["ms"]) - min(f["ms"]), 3)
    os.environ.pop(SWITCH, None)
    restore()
    call()
    out["default_form"] = r.last_fused_form()
    _lib.synchronize()
    for a in backup.values():
        a.free()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=3000)
    ap.add_argument("--nsteps", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--case", nargs="+", default=["shallow", "hotpath"], choices=["shallow", "hotpath"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    report = dict(tool="bench_structures_time_major", device=_lib.device_name(0), library=os.path.basename(_lib.library_path()),
                  cases=[])
    for name in a.case:
        res = run_case(name, a.size, a.nsteps, a.repeats, a.calls)
        report["cases"].append(res)
        s, t = res["forms"]["0"], res["forms"]["1"]
        print("%s %d^2 (%d cells, %d levels): %s %.2f ms (spread %.2f, %d launches) | %s %.2f ms (spread %.2f, %d launches) | "
              "bit-identical: %s" % (name, res["size"], res["cells"], res["levels"], s["form"], s["ms_per_model_step"],
                                     s["spread_ms"], s["launches"], t["form"], t["ms_per_model_step"], t["spread_ms"],
                                     t["launches"], res["bit_identical"]), flush=True)
    print(json.dumps(report), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
