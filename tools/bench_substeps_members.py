"""A model step of an ensemble on one router (24 split-routing sub-steps) against the same members run one by one, in one
process:

    python tools/bench_substeps_members.py [--cases shallow:3000,deep:2000,etrs89] [--members 1,2,4,16] [--reps 7]
                                           [--out profiles/substeps_members.json]

Per case and member count M the two forms are timed alternately (lf_timer_start / lf_timer_stop around one model step of all
members, after a warm-up of both) on device-resident vectors in engine order:
    single_calls   M calls of lf_routing_substeps_fused, one per member -- the only way before the member call, and
                   the reference of every ratio
    member_call    one lf_routing_substeps_fused_members call
and the median of `reps` repetitions is reported: ms per model step, the spread (max - min) of each form's repetitions, the
ratio members / single, the schedule the member call took (lf_router_last_fused_form), its launches and its slice size.
`within_spread_of_single`: the member call's median does not exceed the single calls' by more than the larger of the two
spreads -- what the library's default choice of the member form has to satisfy wherever it makes it
(`member_form_by_default`).  Where the library's rule does not choose the member kernel a third leg
times it under LF_FUSED_TIME_MAJOR=1 (`member_call_forced_time_major`), for the record.
The synthetic cases default to M = 1, 2, 4, 16, the LF_ETRS89 graph (tests/golden/graph_etrs89.npz) to M = 1, 4, 16, 64.
The environment decides the schedule as in any call (LF_FUSED_TIME_MAJOR, LF_FUSED_MEMBERS_SLICE); it is recorded.
Writes one JSON object to --out and prints it."""
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
from lisflood_amd.kinematic_wave_parallel import Graph, kinematicWave  # noqa: E402
from lisflood_amd.routing import _OUT, _STATE, _STATIC, SubstepVectors, substep_host_vectors  # noqa: E402

SEEDS = {"shallow": 1, "deep": 2}
NSTEPS = 24


def build(case):
    """-> (router with floodplains, model-step values in pixel order, dt)"""
    if case == "etrs89":
        g = np.load(os.path.join(ROOT, "tests", "golden", "graph_etrs89.npz"))
        graph = Graph(g["codes"], g["mask"])
    else:
        family, size = case.split(":")
        graph = Graph(ldd_raster=syn.make_ldd(family, int(size), int(size), SEEDS[family]))
    N = graph.num_pixels
    p = syn.router_params(N)
    vals, dt = syn.model_step_values(N, p)
    kw = kinematicWave(None, None, p["alpha"], p["beta"], p["dx"], dt, alpha_floodplains=vals["ChannelAlpha2"], graph=graph)
    return kw, p, vals, dt


def run_case(case, member_counts, reps):
    kw, p, vals, dt = build(case)
    N, L = kw.num_pixels, _lib.lib()
    perm = kw.graph.layout()[0].astype(np.int64)
    mmax = max(member_counts)
    sv = SubstepVectors(substep_host_vectors(vals, N, perm, _STATIC), N, p["beta"], 1.0 / dt, dt * NSTEPS, True, True,
                        lengths={k: mmax * N for k in _STATE + _OUT}, sideflow=np.zeros((mmax, N)))
    start = substep_host_vectors(vals, N, perm, _STATE)
    rows = np.empty((mmax, N))

    def reset():
        """every member back to its start: member m's discharge is the case's times 1 + 0.25 m (volumes to match)"""
        for k in _STATE:
            for m in range(mmax):
                f = 1 + 0.25 * m
                rows[m] = start[k] * (f if k == "ChanQKin" else f ** p["beta"] if k == "ChanM3Kin" else 1.0)
            sv.upload(k, rows.reshape(-1))
        for m in range(mmax):
            rows[m] = vals["SideflowChanM3"][perm] * (1 + 0.1 * m)
        sv.upload("SideflowChanM3", rows.reshape(-1))

    per_member = [sv.with_overrides(**dict({k: sv.dev[k].ptr.value + 8 * m * N for k in _STATE + _OUT},
                                           SideflowChanM3=sv.dev["SideflowChanM3"].ptr.value + 8 * m * N)) for m in range(mmax)]

    def single(M):
        for m in range(M):
            _lib.check(L.lf_routing_substeps_fused(kw._h, C.byref(per_member[m]), NSTEPS, 0))

    def members(M):
        kw.routing_substeps_members(sv.args, NSTEPS, M, N, 0, N)

    def timed(form, M):
        _lib.timer_start()
        form(M)
        return _lib.timer_stop()

    def members_forced(M):
        """the member kernel where the library's own rule does not choose it (informative: what a wider rule would buy)"""
        before = os.environ.get("LF_FUSED_TIME_MAJOR")
        os.environ["LF_FUSED_TIME_MAJOR"] = "1"
        try:
            members(M)
        finally:
            os.environ.pop("LF_FUSED_TIME_MAJOR")
            if before is not None:
                os.environ["LF_FUSED_TIME_MAJOR"] = before

    levels = kw.graph.num_levels
    out = []
    for M in member_counts:
        reset()
        legs = [("single_calls", single), ("member_call", members), ("member_call_forced_time_major", members_forced)]
        ms = {name: [] for name, _ in legs}
        info = {}
        for rep in range(reps + 1):                       # the first round of all forms is the warm-up
            for name, form in legs:
                t = timed(form, M)
                if rep:
                    ms[name].append(t)
                info[name] = dict(form=kw.last_fused_form(), launches=kw.last_launches()["launches"])
            if rep == 0 and info["member_call"]["form"] == "time-major":
                legs = legs[:2]                           # the library's own choice already
        row = dict(case=case, cells=N, levels=levels, members=M, member_form_by_default=info["member_call"]["form"] == "time-major" and M > 1)
        for name, _ in legs:
            row[name] = dict(ms_per_model_step=statistics.median(ms[name]), spread_ms=max(ms[name]) - min(ms[name]), **info[name])
            if name != "single_calls":
                row[name]["ratio_to_single"] = row[name]["ms_per_model_step"] / row["single_calls"]["ms_per_model_step"]
                # not slower than the single calls by more than the larger of the two spreads
                row[name]["within_spread_of_single"] = bool(row[name]["ms_per_model_step"] - row["single_calls"]["ms_per_model_step"]
                                                            <= max(row[name]["spread_ms"], row["single_calls"]["spread_ms"]))
                # members per slice, from the launches: flag passes + one launch per level and slice
                nslices = row[name]["launches"] // levels if row[name]["form"] == "time-major" else 0   # (at most 2 flag passes)
                row[name]["slice"] = -(-M // nslices) if nslices else None
        row["single_calls"]["launches"] *= M                    # (the statistics are those of the last of the M calls)
        out.append(row)
        print("[substeps_members] %s" % json.dumps(row), file=sys.stderr, flush=True)
    sv.free()
    kw.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="shallow:3000,deep:2000,etrs89")
    ap.add_argument("--members", default=None, help="default 1,2,4,16 (etrs89: 1,4,16,64)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "substeps_members.json"))
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("at least 7 repetitions")
    results = []
    for case in a.cases.split(","):
        counts = [int(x) for x in a.members.split(",")] if a.members else ([1, 4, 16, 64] if case == "etrs89" else [1, 2, 4, 16])
        results += run_case(case, counts, a.reps)
    env = {k: os.environ[k] for k in ("LF_FUSED_TIME_MAJOR", "LF_FUSED_MEMBERS_SLICE", "LF_FUSED_TIME_MAJOR_LEVELS") if k in os.environ}
    doc = dict(device=_lib.device_name(0), nsteps=NSTEPS, split=True, reps=a.reps, env=env, results=results)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
