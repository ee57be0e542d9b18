"""What new forcing costs an ensemble per model step: hotpath.HotPathEnsemble fed through its double-buffered upload
(prefetch / pinned_forcing, lf_upload_rows) against the same members stepped one after the other through a HotPathDevice and
its own prefetch, in one process:

    python tools/bench_members_upload.py [--cases 2000,etrs89] [--members 2,4,16] [--reps 5] [--steps 4]
                                         [--out profiles/members_upload.json]

Inputs: the scenario of tools/bench_hotpath_members.py (synthetic.hotpath_scenario; `etrs89` is the LF_ETRS89-sized case of
39 x 73 pixels) and synthetic.hotpath_forcing, member m forced by seed 10 m.  Both objects run as a user runs them, with
overlap_channel=True.

A leg is a window of `steps` model steps of the whole ensemble, timed with the host clock from a synchronised device to a
synchronised device; its figure is the window over `steps`.  The forcing of the window's first step is handed over before the
clock starts and every step hands over the forcing of the step after it, so a window holds `steps` uploads and `steps` steps
in the steady state of a run.  The page-locked sets are filled before the clock starts (two of them, handed over
alternately): filling them is the meteo reader's work and the same for every leg.  Legs, alternating, after one untimed round
of all of them; median and spread (max - min) of `reps` repetitions:
    single_prefetch          members x steps steps of ONE HotPathDevice through its prefetch + pinned_forcing + upload_wait,
                             float64 in pixel order (it permutes on the host); the reference of ratio_to_single_prefetch
    single_prefetch_ordered  the same with prefetch(ordered=True): a caller that compresses its rasters with the composed index
    ensemble_prefetch_f64    HotPathEnsemble.step on prefetched [members, N] float64 rows, upload_wait, prefetch of the next
    ensemble_prefetch_f32    the same from float32 rows (what the meteo files hold)
    ensemble_step_pageable   step(rows) from ordinary numpy arrays, float64, no prefetch
    ensemble_resident        step(None): the device's own work
    copy_only / copy_only_f32  the bytes of the two prefetch legs from page-locked memory with lf_upload_copy into vectors of
                             their own, no kernels: the floor the link sets on this box
Per row also: floor = max(copy_only, ensemble_resident) and exposed_over_floor = ensemble_prefetch / floor, and `reached`:
ensemble_prefetch / single_prefetch <= 1 + the larger relative spread of the two legs."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "lisflood-code_amd"))
from lisflood_amd import _lib  # noqa: E402
from lisflood_amd import synthetic as syn  # noqa: E402
from lisflood_amd.hotpath import FORCING, HotPathDevice, HotPathEnsemble  # noqa: E402


def scenario(case):
    H, W = (39, 73) if case.startswith("etrs89") else (int(case), int(case))
    return syn.hotpath_scenario(H, W, family="deep", block=1_000_000)


def window(prime, body, steps):
    """ms per step of `steps` calls of body(s), between two synchronised states of the device"""
    prime()
    _lib.synchronize(0)
    t0 = time.perf_counter()
    for s in range(steps):
        body(s)
    _lib.synchronize(0)
    return (time.perf_counter() - t0) * 1e3 / steps


def run_case(case, member_counts, reps, steps):
    values, sc, mask, ldd_to_chan, ldd_kin = scenario(case)
    N = int(mask.sum())
    L = _lib.lib()
    hp = HotPathDevice(values, sc, mask, ldd_to_chan, ldd_kin, split=True)
    one = [hp.pinned_forcing() for _ in range(2)]           # the single object's two sets: member 0's vectors
    one_ordered = [hp.pinned_forcing() for _ in range(2)]
    for s in range(2):
        for k, a in syn.hotpath_forcing(N, s).items():
            one[s][k][...] = a
            one_ordered[s][k][...] = a[hp.pixel_of_position]
    out = []
    for M in member_counts:
        ens = HotPathEnsemble(values, sc, mask, ldd_to_chan, ldd_kin, M, split=True)
        rows = []                                           # two steps' forcing, [M, N] float64 in ordinary memory
        for s in range(2):
            f = [syn.hotpath_forcing(N, s + 10 * m) for m in range(M)]
            rows.append({k: np.stack([x[k] for x in f]) for k in FORCING})
        pin = {}
        for name, dtype in (("f64", np.float64), ("f32", np.float32)):
            pin[name] = [ens.pinned_forcing(dtype) for _ in range(2)]
            for s in range(2):
                for k in FORCING:
                    pin[name][s][k][...] = rows[s][k]
        scratch = [_lib.DeviceArray(M * N, np.float64) for _ in FORCING]

        def single(sets, ordered):
            def body(t):
                hp.step(sets[t % 2], ordered=ordered)
                hp.upload_wait()
                hp.prefetch(sets[(t + 1) % 2], ordered=ordered)
            return lambda: window(lambda: hp.prefetch(sets[0], ordered=ordered), body, steps * M) * M

        def prefetched(sets):
            def body(s):
                ens.step(sets[s % 2])
                ens.upload_wait()
                ens.prefetch(sets[(s + 1) % 2])
            return lambda: window(lambda: ens.prefetch(sets[0]), body, steps)

        def copies(sets):
            def body(s):
                _lib.check(L.lf_upload_begin(0, s % 2))
                for d, k in zip(scratch, FORCING):
                    a = sets[s % 2][k]
                    _lib.check(L.lf_upload_copy(0, d.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes))
                _lib.check(L.lf_upload_end(0, s % 2))
            return lambda: window(lambda: None, body, steps)

        def resident():
            ens.step(rows[0])                               # (the rows of a step, not what a prefetch left pending)
            return window(lambda: None, lambda s: ens.step(None), steps)
        legs = [("single_prefetch", single(one, False)), ("single_prefetch_ordered", single(one_ordered, True)),
                ("ensemble_prefetch_f64", prefetched(pin["f64"])), ("ensemble_prefetch_f32", prefetched(pin["f32"])),
                ("ensemble_step_pageable", lambda: window(lambda: None, lambda s: ens.step(rows[s % 2]), steps)),
                ("ensemble_resident", resident), ("copy_only", copies(pin["f64"])), ("copy_only_f32", copies(pin["f32"]))]
        ms = {k: [] for k, _ in legs}
        for rep in range(reps + 1):                         # the first round of all legs is the warm-up
            for name, fn in legs:
                t = fn()
                if rep:
                    ms[name].append(t)
        row = dict(case=case, pixels=N, channel_pixels=int(ens.Nk), members=M, steps_per_window=steps,
                   forcing_bytes_per_step=dict(f64=5 * M * N * 8, f32=5 * M * N * 4), forms=ens.last_forms())
        for name, _ in legs:
            med = statistics.median(ms[name])
            row[name] = dict(ms_per_model_step=med, spread_ms=max(ms[name]) - min(ms[name]),
                             relative_spread=(max(ms[name]) - min(ms[name])) / med)
        ref = row["single_prefetch"]
        for name, _ in legs[1:]:
            row[name]["ratio_to_single_prefetch"] = row[name]["ms_per_model_step"] / ref["ms_per_model_step"]
        for kind, floor in (("f64", "copy_only"), ("f32", "copy_only_f32")):
            leg = row["ensemble_prefetch_" + kind]
            leg["floor_ms"] = max(row[floor]["ms_per_model_step"], row["ensemble_resident"]["ms_per_model_step"])
            leg["exposed_over_floor"] = leg["ms_per_model_step"] / leg["floor_ms"]
            leg["reached"] = bool(leg["ratio_to_single_prefetch"] <= 1 + max(leg["relative_spread"], ref["relative_spread"]))
        out.append(row)
        print("[members_upload] %s" % json.dumps(row), file=sys.stderr, flush=True)
        for d in scratch:
            d.free()
        ens.free()
    hp.free()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="2000,etrs89")
    ap.add_argument("--members", default=None, help="default 2,4,16 (etrs89: 16,64)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4, help="model steps per timed window")
    ap.add_argument("--before", default=None, help="JSON of tools/bench_hotpath_members.py run on the parent commit")
    ap.add_argument("--after", default=None, help="JSON of tools/bench_hotpath_members.py run on this commit, same box")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "members_upload.json"))
    a = ap.parse_args()
    if a.reps < 5 or a.steps < 2:
        ap.error("at least 5 repetitions of at least 2 steps")
    counts = lambda case: [int(x) for x in a.members.split(",")] if a.members else ([16, 64] if case.startswith("etrs89") else [2, 4, 16])
    results = []
    for case in a.cases.split(","):
        results += run_case(case, counts(case), a.reps, a.steps)
    doc = dict(device=_lib.device_name(0), reps=a.reps, steps_per_window=a.steps, results=results)
    for key, path in (("parent_commit", a.before), ("this_commit", a.after)):
        if path:                                            # the legs of bench_hotpath_members.py that (a) compares
            with open(path) as f:
                rows = json.load(f)["results"]
            doc["bench_hotpath_members_" + key] = [
                dict(case=r["case"], members=r["members"], **{leg: {k: r[leg][k] for k in ("ms_per_model_step", "spread_ms")}
                                                             for leg in ("single_steps", "ensemble", "single_resident",
                                                                         "ensemble_resident")}) for r in rows]
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
