"""A model step of an ensemble on one router WITH lakes, reservoirs, inflow hydrographs and transmission loss in the loop
(24 split-routing sub-steps) against the same members run one by one, in one process:

    python tools/bench_structures_members.py [--size 3000] [--case shallow hotpath] [--members 2,4,16] [--reps 7]
                                             [--out profiles/structures_members_3000.json]

  shallow  syn.make_ldd("shallow", size, size, 2) with the default structures_scenario (64 lakes + 192 reservoirs)
  hotpath  the channel network of syn.hotpath_scenario(size, size) with the same structures (compact domain)
(the cases of tools/bench_structures_time_major.py).  Per case and member count M the forms are timed alternately
(lf_timer_start / lf_timer_stop around one model step of all members, after a warm-up round of every form) on device-resident
member rows in engine order, every member starting from the module's state (restored by device-to-device copies before every
timed call, so all repeats do the same arithmetic) and reading one shared set of forcing rows:
    single_calls   M calls of lf_routing_substeps_fused_structures, one per member -- the only way before the member call,
                   and the reference of every ratio
    member_call    one lf_routing_substeps_fused_structures_members call
and the median of `reps` repetitions is reported: ms per model step, the spread (max - min) of each form's repetitions, the
ratio members / single, the schedule each took (lf_router_last_fused_form) and its launches.  `within_spread_of_single`: the
member call's median does not exceed the single calls' by more than the spread of the single calls -- what the library's
default choice of the member form has to satisfy wherever it makes it (`member_form_by_default`).
Where the library's rule does not choose the member form a third leg times it under LF_FUSED_TIME_MAJOR=1
(`member_call_forced_time_major`), for the record.  The environment decides the schedule as in any call
(LF_FUSED_TIME_MAJOR, LF_FUSED_MEMBERS_SLICE); it is recorded.  Writes one JSON object to --out and prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lisflood-code_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from lisflood_amd import _lib  # noqa: E402
from lisflood_amd import routing as R  # noqa: E402
from lisflood_amd._lib import DeviceArray  # noqa: E402
from bench_structures_time_major import OPTIONS, hotpath_case, shallow_case  # noqa: E402

NSTEPS = 24
SWITCH = "LF_FUSED_TIME_MAJOR"


def run_case(name, size, member_counts, reps):
    v, cut, mask, compact = (shallow_case if name == "shallow" else hotpath_case)(size, NSTEPS)
    m = R.routing(v, options=OPTIONS, engine_order=True, compact=compact)
    m.attach_router(cut, mask)
    m.attach_structures()
    m.begin_step()
    m.dynamic_fused()                                   # leaves every argument block wired (and the site lists checked)
    L, kw, st = _lib.lib(), m.river_router, m._st
    N, nl, nr, mmax = kw.num_pixels, int(st["lakes"]), int(st["res"]), max(member_counts)
    # name -> (the module's device vector, entries of a member row, the block that points at it)
    rows = {k: (m._dev[k], N, "args") for k in R._STATE + R._OUT}
    rows["SideflowChanM3"] = (m._dev["SideflowChanM3"], N, "inloop")
    rows.update({k: (st["dev"][k], N, "inloop") for k in R._INLOOP_DENSE[:-1] if k in st["dev"]})
    rows.update({k: (st["dev"][k], nl, "inloop") for k in R._LAKE_STATE})
    rows.update({k: (st["dev"][k], nr, "inloop") for k in R._RES_STATE})
    dev = {k: DeviceArray(mmax * n, src.dtype, m.device) for k, (src, n, _) in rows.items()}

    def restore(M):
        """every member back to the module's state"""
        for k, (src, n, _) in rows.items():
            for i in range(M):
                _lib.check(L.lf_memcpy_d2d(m.device, C.c_void_p(dev[k].ptr.value + 8 * i * n), src.ptr, 8 * n))

    def blocks(i):
        """the two argument blocks with every per-member pointer at member i's row; forcing rows shared"""
        a, b = R._SubstepArgs.from_buffer_copy(m._args), R._InloopArgs.from_buffer_copy(m._inloop)
        for k, (_, n, where) in rows.items():
            setattr(a if where == "args" else b, k, dev[k].ptr.value + 8 * i * n)
        a.SideflowChanM3, b.ChanQ = b.SideflowChanM3, a.ChanQ
        return a, b

    per_member = [blocks(i) for i in range(mmax)]

    def single(M):
        for a, b in per_member[:M]:
            _lib.check(L.lf_routing_substeps_fused_structures(kw._h, C.byref(a), C.byref(b), NSTEPS))

    def members(M):
        kw.routing_substeps_structures_members(per_member[0][0], per_member[0][1], NSTEPS, M, N, nl, nr, 0)

    def members_forced(M):
        """the member form where the library's own rule does not choose it (informative)"""
        before = os.environ.get(SWITCH)
        os.environ[SWITCH] = "1"
        try:
            members(M)
        finally:
            os.environ.pop(SWITCH)
            if before is not None:
                os.environ[SWITCH] = before

    def timed(form, M):
        restore(M)
        _lib.synchronize()
        _lib.timer_start()
        form(M)
        return _lib.timer_stop()

    levels = kw.graph.num_levels
    out = []
    for M in member_counts:
        legs = [("single_calls", single), ("member_call", members), ("member_call_forced_time_major", members_forced)]
        ms = {leg: [] for leg, _ in legs}
        info = {}
        for rep in range(reps + 1):                       # the first round of all forms is the warm-up
            for leg, form in legs:
                t = timed(form, M)
                if rep:
                    ms[leg].append(t)
                info[leg] = dict(form=kw.last_fused_form(), launches=int(kw.last_launches()["launches"]))
            if rep == 0 and info["member_call"]["form"] == "time-major":
                legs = legs[:2]                           # the library's own choice already
        row = dict(case=name, size=size, cells=int(N), levels=int(levels), lakes=nl, reservoirs=nr, members=M,
                   member_form_by_default=info["member_call"]["form"] == "time-major")
        for leg, _ in legs:
            row[leg] = dict(ms_per_model_step=statistics.median(ms[leg]), spread_ms=max(ms[leg]) - min(ms[leg]), **info[leg])
            if leg != "single_calls":
                single_ms = row["single_calls"]
                row[leg]["ratio_to_single"] = row[leg]["ms_per_model_step"] / single_ms["ms_per_model_step"]
                row[leg]["within_spread_of_single"] = bool(row[leg]["ms_per_model_step"] - single_ms["ms_per_model_step"]
                                                           <= single_ms["spread_ms"])
        row["single_calls"]["launches"] *= M                    # (the statistics are those of the last of the M calls)
        out.append(row)
        print("[structures_members] %s" % json.dumps(row), file=sys.stderr, flush=True)
    for d in dev.values():
        d.free()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=3000)
    ap.add_argument("--case", nargs="+", default=["shallow", "hotpath"], choices=["shallow", "hotpath"])
    ap.add_argument("--members", default="2,4,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structures_members_3000.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    results = []
    for name in a.case:
        results += run_case(name, a.size, [int(x) for x in a.members.split(",")], a.reps)
    env = {k: os.environ[k] for k in (SWITCH, "LF_FUSED_MEMBERS_SLICE", "LF_FUSED_TIME_MAJOR_LEVELS") if k in os.environ}
    doc = dict(tool="bench_structures_members", device=_lib.device_name(0), nsteps=NSTEPS, split=True, reps=a.reps, env=env,
               results=results)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
