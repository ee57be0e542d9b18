"""The land surface of an ensemble (canopy + ESMax + soil columns of every member) in one launch against the same members
run one by one, in one process:

    python tools/bench_land_members.py [--cases 2000,etrs89] [--members 2,4,16] [--reps 7] [--plain LIBRARY.so]
                                       [--out profiles/land_members_2000.json]
    python tools/bench_land_members.py --profile --cases 2000 --members 4 [--steps 3]      (under rocprofv3 --pmc ...)
    python tools/bench_land_members.py --digest DIR [DIR ...]                             (the counter files of such runs)

Inputs: synthetic.hotpath_scenario (a size x size raster, fields drawn for a block of 10^6 pixels and repeated; `etrs89` is
the LF_ETRS89-sized case of 39 x 73 = 2 847 pixels) and synthetic.hotpath_forcing; member m is forced by seed 10 m and starts
from a seeded perturbation of the scenario's state (UZ, DSLR, CumInterception, W2 scaled towards WRes2).  Before every timed
call the state vectors are put back from a device-side copy, so every call of every form does the same work.

Forms, timed alternately (lf_timer_start / lf_timer_stop around the calls of one model step of all members, after one
untimed round of all forms), the median of `reps` repetitions reported:
    single_calls       M calls of lf_land_columns_device, one per member -- the only way before the member call, and the
                       reference of every ratio
    member_call        one lf_land_columns_members_device call (units tile-major, dealt XCD-contiguously)
    member_call_plain  the same call of a second library built with -DLF_LAND_MEMBERS_XCD=0 (tools/build_variant.sh
                       land_plain "-DLF_LAND_MEMBERS_XCD=0" lf_soil): plain tile-major launch order.  Left out without --plain.
Per form: ms per model step of the ensemble, the spread (max - min) of its repetitions, the ratio to the single calls, and
`within_spread_of_single`: its median does not exceed the single calls' by more than the larger of the two spreads -- what a
default has to satisfy.  `xcd_beats_plain`: the XCD-contiguous order is faster than plain order by more than the larger of
their spreads.

--profile runs `steps` model steps of the single calls and of the member call, untimed, for a counter pass of its own
(rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum, and --pmc FETCH_SIZE in another run); --digest sums the counters of
k_soil_fused per form (the member form is the instantiation whose last template argument is true) and prints the L2 hit
rate TCC_HIT / (TCC_HIT + TCC_MISS).  Infinity Cache hits are counted in FETCH_SIZE and L2 hits are not, so the L2 hit rate
is the number that shows whether the members of a tile shared its statics."""
import argparse
import collections
import csv
import ctypes as C
import glob
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "lisflood-code_amd"))
from lisflood_amd import _lib  # noqa: E402
from lisflood_amd import soilloop as SL  # noqa: E402
from lisflood_amd import synthetic as syn  # noqa: E402
from lisflood_amd._lib import DeviceArray  # noqa: E402

STATE = "W1a W1b W1 W2 UZ DSLR CumInterception".split()        # what a step reads of the step before


def shape_of(case):
    return (39, 73) if case == "etrs89" else (int(case), int(case))


def second_library(path):
    """the same C ABI from another build, loaded beside the tree's own (its own stream and workspace on the device)"""
    L = C.CDLL(os.path.abspath(path))
    for sig, names in _lib._SIGNATURES.items():
        args, _, ret = sig.partition(">")
        for name in names.split():
            f = getattr(L, "lf_" + name)
            f.argtypes, f.restype = [_lib._KIND[k] for k in args], _lib._KIND[ret or "i"]
    return L


class Ensemble:
    """mmax members of one scenario on the device; every form runs the first M of them"""

    def __init__(self, case, mmax):
        H, W = shape_of(case)
        self.N = N = H * W
        values, sc, _mask, _to_chan, _kin = syn.hotpath_scenario(H, W, family="deep", block=1_000_000)
        d = dict(values, **sc)
        del values
        self.ens = ens = SL.LandSurfaceEnsemble(d, mmax)
        rng = np.random.default_rng(77)
        f = rng.uniform(0.5, 1.5, (mmax, 1, 1))
        ens.set("UZ", d["UZ"][None] * f)
        ens.set("DSLR", d["DSLR"][None] + rng.integers(0, 5, (mmax, 1, 1)))
        ens.set("CumInterception", d["CumInterception"][None] * f)
        ens.set("W2", d["WRes2"][None] + (d["W2"] - d["WRes2"])[None] * rng.uniform(0.6, 1.0, (mmax, 1, 1)))
        for k in syn.hotpath_forcing(8, 0):
            ens.set(k, np.stack([syn.hotpath_forcing(N, 10 * m)[k] for m in range(mmax)]))
        self.snap = {k: DeviceArray(ens.dev[k].shape, np.float64).copy_from(ens.dev[k]) for k in STATE}
        # member m's own argument blocks, for the single calls
        self.blocks = []
        for m in range(mmax):
            c, s = SL._CanopyArgs(), SL._SoilArgs()
            C.memmove(C.byref(c), C.byref(ens.canopy), C.sizeof(c))
            C.memmove(C.byref(s), C.byref(ens.soil), C.sizeof(s))
            for blk in (c, s):
                for name, _kind in blk._fields_:
                    if name in ens._member and getattr(blk, name):
                        setattr(blk, name, getattr(blk, name) + 8 * m * ens.stride)
                    elif name in ens._forcing and getattr(blk, name):
                        setattr(blk, name, getattr(blk, name) + (1 if name in SL._BOOL else 8) * m * ens.fstride)
            self.blocks.append((c, s, ens.dev["ESRef"].ptr.value + 8 * m * ens.fstride))
        self.derived = 1 if ens.derived else 0

    def restore(self):
        for k, a in self.snap.items():
            self.ens.dev[k].copy_from(a)
        _lib.synchronize()

    def single(self, L, M):
        for c, s, es in self.blocks[:M]:
            _lib.check(L.lf_land_columns_device(0, C.byref(c), C.byref(s), es, self.derived))

    def members(self, L, M):
        e = self.ens
        rc = L.lf_land_columns_members_device(0, C.byref(e.canopy), C.byref(e.soil), e.dev["ESRef"].ptr, self.derived, M,
                                              e.stride, e.fstride)
        if rc != 0:
            raise RuntimeError("lf_land_columns_members_device: %d %s" % (rc, L.lf_last_error()))

    def free(self):
        for a in self.snap.values():
            a.free()
        self.ens.free()


def timed(E, L, form, M):
    E.restore()
    if L.lf_timer_start(0) != 0:
        raise RuntimeError("lf_timer_start")
    form(L, M)
    ms = C.c_double(0.0)
    if L.lf_timer_stop(0, C.byref(ms)) != 0:
        raise RuntimeError("lf_timer_stop")
    return ms.value


def run_case(case, member_counts, reps, plain):
    E = Ensemble(case, max(member_counts))
    L = _lib.lib()
    legs = [("single_calls", L, E.single), ("member_call", L, E.members)]
    if plain is not None:
        legs.append(("member_call_plain", plain, E.members))
    out = []
    for M in member_counts:
        ms = {name: [] for name, _, _ in legs}
        form = {}
        for rep in range(reps + 1):                       # the first round of all forms is the warm-up
            for name, lib, fn in legs:
                t = timed(E, lib, fn, M)
                if rep:
                    ms[name].append(t)
                form[name] = lib.lf_soil_last_form(0)
        row = dict(case=case, pixels=E.N, columns_per_member=3 * E.N, members=M)
        for name, _, _ in legs:
            row[name] = dict(ms_per_model_step=statistics.median(ms[name]), spread_ms=max(ms[name]) - min(ms[name]),
                             form=form[name])
        one = row["single_calls"]
        for name, _, _ in legs[1:]:
            r = row[name]
            r["ratio_to_single"] = r["ms_per_model_step"] / one["ms_per_model_step"]
            r["within_spread_of_single"] = bool(r["ms_per_model_step"] - one["ms_per_model_step"]
                                                <= max(r["spread_ms"], one["spread_ms"]))
        if plain is not None:
            a, b = row["member_call"], row["member_call_plain"]
            row["xcd_beats_plain"] = bool(b["ms_per_model_step"] - a["ms_per_model_step"] > max(a["spread_ms"], b["spread_ms"]))
        out.append(row)
        print("[land_members] %s" % json.dumps(row), file=sys.stderr, flush=True)
    E.free()
    return out


def profile(case, M, steps):
    E = Ensemble(case, M)
    L = _lib.lib()
    for _ in range(steps):
        E.restore()
        E.single(L, M)
        _lib.synchronize()
        E.restore()
        E.members(L, M)
        _lib.synchronize()
    print("land members profile: case %s, %d members, %d steps of each form" % (case, M, steps), flush=True)
    E.free()


def digest(dirs):
    total = collections.defaultdict(lambda: collections.defaultdict(float))
    for d in dirs:
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                m = re.search(r"k_soil_fused<([^>]*)>", r["Kernel_Name"])
                if m:
                    form = "member_call" if m.group(1).replace(" ", "").split(",")[-1] in ("true", "1") and \
                        len(m.group(1).split(",")) == 4 else "single_calls"
                    total[form][r["Counter_Name"]] += float(r["Counter_Value"])
    out = {}
    for form, c in sorted(total.items()):
        row = dict(c)
        if c.get("TCC_HIT_sum", 0) + c.get("TCC_MISS_sum", 0) > 0:
            row["l2_hit_rate"] = c["TCC_HIT_sum"] / (c["TCC_HIT_sum"] + c["TCC_MISS_sum"])
        out[form] = row
    print(json.dumps(dict(kernel="k_soil_fused", counters=out), indent=1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="2000,etrs89")
    ap.add_argument("--members", default=None, help="default 2,4,16 (etrs89: 16,64)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--plain", default=None, help="a second build of the library, in plain launch order")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "land_members_2000.json"))
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--digest", nargs="+", default=None)
    a = ap.parse_args()
    if a.digest:
        digest(a.digest)
        return
    counts = lambda case: [int(x) for x in a.members.split(",")] if a.members else ([16, 64] if case == "etrs89" else [2, 4, 16])
    if a.profile:
        for case in a.cases.split(","):
            profile(case, max(counts(case)), a.steps)
        return
    if a.reps < 7:
        ap.error("at least 7 repetitions")
    plain = second_library(a.plain) if a.plain and os.path.exists(a.plain) else None
    results = []
    for case in a.cases.split(","):
        results += run_case(case, counts(case), a.reps, plain)
    env = {k: os.environ[k] for k in ("LF_LAND_MEMBERS", "LF_SOIL_TRIP_CAP", "LF_GENERAL_POW", "LF_SOIL_NO_DERIVED") if k in os.environ}
    doc = dict(device=_lib.device_name(0), reps=a.reps, env=env, plain_order_library=bool(plain), results=results)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
