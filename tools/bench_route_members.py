"""An ensemble on one router against the same members routed one by one, in one process:

    python tools/bench_route_members.py [--cases shallow:10000,deep:5000,river:10000,etrs89] [--members 1,2,4,8]
                                        [--reps 7] [--steps 10] [--mb 1,2,4]

Per case and member count M the two forms are timed alternately (lf_timer_start / lf_timer_stop around `steps` steps,
after a warm-up of both) on device-resident vectors in engine order:
    single   M calls of lf_router_route_ordered per step -- the only way to route M members before the member call
    members  one lf_router_route_ordered_members call per step
and the median of `reps` repetitions is reported: ms per step, ms per member, the ratio members / single, and the
spread (max - min) of each form's repetitions.  --mb times the member form once per value of LF_MEMBERS_MB (members per
lane of the wide-level kernel) instead of the library's default.  The LF_ETRS89 case defaults to M = 1, 4, 16, 64 and
20 x the steps.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "lisflood-code_amd"))
import bench  # noqa: E402
from lisflood_amd import _lib  # noqa: E402
from lisflood_amd import synthetic as syn  # noqa: E402
from lisflood_amd.kinematic_wave_parallel import kinematicWave  # noqa: E402


def build(case):
    if case == "etrs89":
        g = np.load(os.path.join(ROOT, "tests", "golden", "route_etrs89.npz"))
        kw = kinematicWave(g["codes"], g["mask"], g["alpha"], float(g["beta"]), g["dx"], float(g["dt"]))
        return kw, g["Q0"], lambda m: g["q"][m % g["q"].shape[0]] * (1 + 0.1 * m)
    family, size = case.split(":")
    kw, p, _ = bench.build_case(family, int(size), int(size))
    return kw, p["Q0"], lambda m: syn.lateral_inflow(kw.num_pixels, m)


def resident_rows(kw, members, row):
    """[members, N] in engine order on the device, row m = row(m) (pixel order on the host), uploaded row by row"""
    N = kw.num_pixels
    out, tmp = _lib.DeviceArray((members, N)), _lib.DeviceArray(N)
    for m in range(members):
        tmp.upload(np.ascontiguousarray(row(m), dtype=np.float64))
        _lib.check(_lib.lib().lf_router_to_engine_order(kw._h, tmp.ptr, out.ptr.value + 8 * m * N))
    _lib.synchronize()
    tmp.free()
    return out


def run_case(case, member_counts, reps, steps, mbs):
    kw, Q0, lateral = build(case)
    N, h, L = kw.num_pixels, kw._h, _lib.lib()
    mmax = max(member_counts)
    Q = resident_rows(kw, mmax, lambda m: Q0 * (1 + 0.25 * m))
    q = resident_rows(kw, mmax, lateral)

    def single(M):
        for m in range(M):
            _lib.check(L.lf_router_route_ordered(h, Q.ptr.value + 8 * m * N, q.ptr.value + 8 * m * N, 0))

    def members(M):
        _lib.check(L.lf_router_route_ordered_members(h, Q.ptr, q.ptr, M, N, 0))

    def timed(form, M):
        _lib.timer_start()
        for _ in range(steps):
            form(M)
        return _lib.timer_stop() / steps

    def summary(ms, M):
        med = statistics.median(ms)
        return dict(ms_per_step=med, ms_per_member=med / M, spread_ms=max(ms) - min(ms))

    rows = []
    for M in member_counts:
        legs = [("single", single, None)] + [("members" + ("_mb%s" % mb if mb else ""), members, mb) for mb in mbs]
        ms = {name: [] for name, _, _ in legs}
        for rep in range(reps + 1):                       # the first round of both forms is the warm-up
            for name, form, mb in legs:
                if mb:
                    os.environ["LF_MEMBERS_MB"] = mb
                else:
                    os.environ.pop("LF_MEMBERS_MB", None)
                t = timed(form, M)
                if rep:
                    ms[name].append(t)
        os.environ.pop("LF_MEMBERS_MB", None)
        row = dict(case=case, cells=N, members=M, launches=kw.last_launches()["launches"])
        for name, _, _ in legs:
            row[name] = summary(ms[name], M)
            if name != "single":
                row[name]["ratio_to_single"] = row[name]["ms_per_step"] / row["single"]["ms_per_step"]
        rows.append(row)
        print("[members] %s" % json.dumps(row), file=sys.stderr, flush=True)
    Q.free(); q.free(); kw.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="shallow:10000,deep:5000,river:10000,etrs89")
    ap.add_argument("--members", default=None, help="default 1,2,4,8 (etrs89: 1,4,16,64)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--mb", default="", help="comma list of LF_MEMBERS_MB values to time instead of the default")
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("at least 7 repetitions")
    mbs = [x for x in a.mb.split(",") if x] or [None]
    out = []
    for case in a.cases.split(","):
        counts = [int(x) for x in a.members.split(",")] if a.members else ([1, 4, 16, 64] if case == "etrs89" else [1, 2, 4, 8])
        out += run_case(case, counts, a.reps, a.steps * (20 if case == "etrs89" else 1), mbs)
    print(json.dumps(dict(device=_lib.device_name(0), reps=a.reps, results=out)))


if __name__ == "__main__":
    main()
