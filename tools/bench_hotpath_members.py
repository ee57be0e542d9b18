"""One model step of an ensemble through the device-resident chain (hotpath.HotPathEnsemble) against the same members
stepped one after the other through a HotPathDevice, in one process:

    python tools/bench_hotpath_members.py [--cases 2000,etrs89,etrs89_structures] [--members 2,4,16] [--reps 5]
                                          [--out profiles/hotpath_members.json]

Inputs: synthetic.hotpath_scenario (a size x size raster, fields drawn for a block of 10^6 pixels and repeated; `etrs89` is
the LF_ETRS89-sized case of 39 x 73 = 2 847 pixels, `etrs89_structures` the same with synthetic.structures_scenario's lakes,
reservoirs, inflow and transmission loss in the channel loop) and synthetic.hotpath_forcing, member m forced by seed 10 m.

Legs, timed alternately with the device stopwatch around whole model steps (both objects with overlap_channel=False, so a
step is one stream from its first kernel to its last), after one untimed round of all legs; the median of `reps` repetitions:
    single_steps      M steps of ONE HotPathDevice, fed the members' forcing in turn -- the launches and bytes of M objects
                      of their own without their memory; the reference of every ratio
    ensemble          one HotPathEnsemble step, every stage in its member form
    land_fallback     the same with LF_LAND_MEMBERS=0      (the land surface member after member)
    pixel_fallback    ... LF_PIXEL_MEMBERS=0               (the per-pixel aggregates member after member)
    surface_fallback  ... LF_SURFACE_MEMBERS=0             (the overland step member after member)
    single_resident / ensemble_resident: the first two with step(None) -- the forcing the device already holds, so no host
                      work and no PCIe traffic: what the device does (through step(forcing) both objects permute and
                      upload the forcing on the host, the ensemble with blocking copies)
    time_major        ... LF_FUSED_TIME_MAJOR=1            (the channel loop as ONE member launch per level where the library's
                      own width rule would go member after member: what the step costs once every stage is in member form)
Per leg: ms per model step of the ensemble, the spread (max - min) of the repetitions, the ratio to single_steps, the forms
the stages took and the launches of the overland sweep and of the channel loop.
A whole step hides a stage of a few launches behind the channel loop's noise, so the per-stage A/B is timed on the stage
itself: `stages` holds, for the land surface, the per-pixel aggregates and the overland step, the stage's own call on the
ensemble's vectors in its member form and member after member, alternating, and `member_form_no_worse`: the member form does
not exceed the fallback by more than the larger of the two spreads -- what a default has to satisfy."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "lisflood-code_amd"))
from lisflood_amd import _lib  # noqa: E402
from lisflood_amd import synthetic as syn  # noqa: E402
from lisflood_amd.hotpath import HotPathDevice, HotPathEnsemble  # noqa: E402

SWITCH = dict(land_fallback=("LF_LAND_MEMBERS", "0"), pixel_fallback=("LF_PIXEL_MEMBERS", "0"),
              surface_fallback=("LF_SURFACE_MEMBERS", "0"), time_major=("LF_FUSED_TIME_MAJOR", "1"))
STAGE = dict(land="LF_LAND_MEMBERS", pixel_aggregates="LF_PIXEL_MEMBERS", overland="LF_SURFACE_MEMBERS")


def stage_calls(ens):
    """stage -> its own call on the ensemble's vectors (what HotPathEnsemble.step runs for it)"""
    L, M = _lib.lib(), ens.members
    return dict(
        land=lambda: ens.land.step(),
        pixel_aggregates=lambda: _lib.check(L.lf_pixel_aggregates_members_device(
            ens.device, C.byref(ens.pixel), M, ens.stride, ens.pstride, ens.land.forcing_member_stride())),
        overland=lambda: _lib.check(L.lf_surface_step_members(ens.r_direct._h, ens.r_other._h, ens.r_forest._h,
                                                               C.byref(ens.surface), M, ens.stride, ens.pstride)))


def stage_ab(ens, reps):
    out = {}
    for stage, call in stage_calls(ens).items():
        ms = dict(member_form=[], member_after_member=[])
        for rep in range(reps + 1):
            for form in ms:
                if form == "member_after_member":
                    os.environ[STAGE[stage]] = "0"
                try:
                    t = timed(call)
                finally:
                    os.environ.pop(STAGE[stage], None)
                if rep:
                    ms[form].append(t)
        row = {form: dict(ms=statistics.median(x), spread_ms=max(x) - min(x)) for form, x in ms.items()}
        a, b = row["member_form"], row["member_after_member"]
        row["ratio"] = a["ms"] / b["ms"]
        row["member_form_no_worse"] = bool(a["ms"] - b["ms"] <= max(a["spread_ms"], b["spread_ms"]))
        out[stage] = row
    return out


def scenario(case):
    H, W = (39, 73) if case.startswith("etrs89") else (int(case), int(case))
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W, family="deep", block=1_000_000)
    st = None
    if case.endswith("_structures"):
        st, ldd_kin = syn.structures_scenario(ldd_kin, (H, W), values["ChanQ"], sc["DtRouting"], n_lakes=3, n_res=5)
    return values, sc, mask, ldd_to_chan, ldd_kin, st


def timed(fn):
    _lib.timer_start(0)
    fn()
    return _lib.timer_stop(0)


def run_case(case, member_counts, reps):
    values, sc, mask, ldd_to_chan, ldd_kin, st = scenario(case)
    N = int(mask.sum())
    cp = lambda d: None if d is None else {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}
    hp = HotPathDevice(values, sc, mask, ldd_to_chan, ldd_kin, split=True, structures=cp(st), overlap_channel=False)
    out = []
    for M in member_counts:
        ens = HotPathEnsemble(values, sc, mask, ldd_to_chan, ldd_kin, M, split=True, structures=cp(st), overlap_channel=False)
        step = [0]

        def forcing():
            return [syn.hotpath_forcing(N, step[0] + 10 * m) for m in range(M)]

        def single():
            f = forcing()
            return timed(lambda: [hp.step(x) for x in f])

        def ensemble(switch=None):
            f = forcing()
            rows = {k: np.stack([x[k] for x in f]) for k in f[0]}
            if switch:
                os.environ[switch[0]] = switch[1]
            try:
                return timed(lambda: ens.step(rows))
            finally:
                if switch:
                    del os.environ[switch[0]]
        legs = [("single_steps", single), ("ensemble", ensemble)] + [(k, (lambda s=s: ensemble(s))) for k, s in SWITCH.items()]
        legs += [("single_resident", lambda: timed(lambda: [hp.step(None) for _ in range(M)])),
                 ("ensemble_resident", lambda: timed(lambda: ens.step(None)))]
        ms, info = {k: [] for k, _ in legs}, {}
        for rep in range(reps + 1):                       # the first round of all legs is the warm-up
            step[0] = rep
            for name, fn in legs:
                t = fn()
                if rep:
                    ms[name].append(t)
                if name.startswith("single"):
                    info[name] = dict(overland_launches=hp.r_direct.last_launches(), channel_launches=hp.river.last_launches(),
                                      channel_form=hp.river.last_fused_form())
                else:
                    info[name] = dict(forms=ens.last_forms(), overland_launches=ens.r_direct.last_launches(),
                                      channel_launches=ens.river.last_launches())
        row = dict(case=case, pixels=N, channel_pixels=int(ens.Nk), members=M)
        for name, _ in legs:
            row[name] = dict(ms_per_model_step=statistics.median(ms[name]), spread_ms=max(ms[name]) - min(ms[name]), **info[name])
        one = row["single_steps"]
        for name, _ in legs[1:]:
            row[name]["ratio_to_single"] = row[name]["ms_per_model_step"] / one["ms_per_model_step"]
        row["ensemble_resident"]["ratio_to_single_resident"] = \
            row["ensemble_resident"]["ms_per_model_step"] / row["single_resident"]["ms_per_model_step"]
        row["stages"] = stage_ab(ens, max(reps, 9))
        out.append(row)
        print("[hotpath_members] %s" % json.dumps(row), file=sys.stderr, flush=True)
        ens.free()
    hp.free()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="2000,etrs89,etrs89_structures")
    ap.add_argument("--members", default=None, help="default 2,4,16 (etrs89 cases: 16,64)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hotpath_members.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    counts = lambda case: [int(x) for x in a.members.split(",")] if a.members else ([16, 64] if case.startswith("etrs89") else [2, 4, 16])
    results = []
    for case in a.cases.split(","):
        results += run_case(case, counts(case), a.reps)
    env = {k: os.environ[k] for k in ("LF_FUSED_TIME_MAJOR", "LF_MEMBERS_MB", "LF_GENERAL_POW") if k in os.environ}
    doc = dict(device=_lib.device_name(0), reps=a.reps, env=env, results=results)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
