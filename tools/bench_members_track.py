"""What products over the steps of a run cost per model step: every member's peak of ChanQAvg and the step it came with, the
sum, and for three threshold maps the first step above and the steps above -- folded on the device by the tracker
(HotPathEnsemble.track_begin: one lf_members_track_device per step) against download("sumDisDay") every step and the same
folds in numpy on the host (all there was before), in one process:

    python tools/bench_members_track.py [--size 2000] [--members 4,16,51] [--reps 5] [--steps 6]
                                        [--out profiles/members_track.json]

Inputs as tools/bench_report_rasters.py: synthetic.hotpath_scenario (size x size), report=REPORT, every member forced by its
own scaling of synthetic.hotpath_forcing out of page-locked float32 arrays, three model steps before anything is timed.
Three paths, alternating in one loop after one untimed round; each measurement is `steps` model steps, host clock from a
synchronised device to a synchronised device, divided by `steps`; median and spread (max - min) of `reps` repetitions:
    a  step() alone
    b  step() with the tracker on (nothing else: the accumulators stay on the device)
    c  step(), chan_q_avg() (download("sumDisDay") / NoRoutSteps) and the folds in numpy, in place
(b) and (c) give the same bits (checked once per member count over three steps).  Alone, device stopwatch
(lf_timer_start / lf_timer_stop) around 20 calls: the update kernel with every output, not a first update, and its bytes --
(32 + 8 T) per (member, element): the source row read, peak read, sum read and written, steps_above read and written per
threshold; peak, peak_step and first_above are stored only where they change -- per second against the measured copy ceiling
of the MI355X, 6.29 TB/s."""
import argparse
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
from lisflood_amd.hotpath import FORCING, HotPathEnsemble  # noqa: E402

REPORT = ("TaPixel", "ThetaAll", "LZAvInflow", "Theta1bPixel", "Sat1", "GwLossCUM")
COPY_CEILING = 6.29e12       # B/s, float4 copy
KERNEL_CALLS = 20
NAME = "ChanQAvg"
KEYS = ("peak", "peak_step", "sum", "first_above", "steps_above")


def log(text):
    print("[members_track] " + text, file=sys.stderr, flush=True)


def update_bytes(members, n, n_thresholds):
    """what a plain update with every output moves at most"""
    return (32 + 8 * n_thresholds) * members * n


class HostFold:
    """the tracker's accumulators on the host, [members, N] / [T, members, N], folded in place"""

    def __init__(self, thr):
        self.thr, self.steps, self.acc = thr, 0, None

    def update(self, x):
        step, thr = self.steps, self.thr
        with np.errstate(invalid="ignore"):
            if step == 0:
                above = [x > t for t in thr]
                self.acc = dict(peak=x.copy(), peak_step=np.zeros(x.shape, np.int32), sum=x.copy(),
                                first_above=np.stack([np.where(a, 0, -1).astype(np.int32) for a in above]),
                                steps_above=np.stack([a.astype(np.int32) for a in above]))
            else:
                acc = self.acc
                take = (x > acc["peak"]) | (np.isnan(x) & ~np.isnan(acc["peak"]))
                np.copyto(acc["peak"], x, where=take)
                acc["peak_step"][take] = step
                acc["sum"] += x
                for t in range(thr.shape[0]):
                    a = x > thr[t]
                    acc["first_above"][t][a & (acc["steps_above"][t] == 0)] = step
                    acc["steps_above"][t] += a
        self.steps += 1


def measure(paths, reps, steps):
    """paths: name -> fn(steps) that runs `steps` model steps"""
    ms = {k: [] for k in paths}
    for rep in range(reps + 1):                             # the first round of every path is the warm-up
        for name, fn in paths.items():
            _lib.synchronize(0)
            t0 = time.perf_counter()
            fn(steps)
            _lib.synchronize(0)
            t = (time.perf_counter() - t0) * 1e3 / steps
            log("round %d %s %.2f ms per step" % (rep, name, t))
            if rep:
                ms[name].append(t)
    return {name: dict(ms=statistics.median(v), spread_ms=max(v) - min(v)) for name, v in ms.items()}


def kernel_alone(ens):
    """ms per plain update of the tracker's accumulators with every output"""
    L = _lib.lib()
    t = ens._trackers[NAME]
    src, n, stride, divisor, _ = ens._source_rows(NAME)
    p = lambda k: t.dev[k].ptr
    call = lambda step: _lib.check(L.lf_members_track_device(0, src.ptr, ens.members, stride, n, divisor, step, 0, t.stride, p("peak"),
                                                             p("peak_step"), p("sum"), t.T, t.thr.ptr, n, p("first_above"),
                                                             p("steps_above")))
    _lib.check(L.lf_side_stream_join(0))
    call(t.steps)
    _lib.synchronize(0)
    _lib.timer_start(0)
    for k in range(KERNEL_CALLS):
        call(t.steps + 1 + k)
    ms = _lib.timer_stop(0) / KERNEL_CALLS
    moved = update_bytes(ens.members, n, t.T)
    return dict(update_ms=ms, update_bytes=moved, update_bytes_per_s=moved / (ms * 1e-3),
                update_fraction_of_copy_ceiling=moved / (ms * 1e-3) / COPY_CEILING)


def run(size, M, reps, steps):
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(size, size, family="deep", block=1_000_000)
    N = int(mask.sum())
    ens = HotPathEnsemble(values, sc, mask, ldd_to_chan, ldd_kin, M, split=True, report=REPORT)
    log("%d^2, %d members: built" % (size, M))
    scale = (1.0 + 0.02 * np.arange(M, dtype=np.float32))[:, None]
    forcing = ens.pinned_forcing(np.float32)
    for k, a in syn.hotpath_forcing(N, 0).items():
        if k in FORCING:
            forcing[k][:] = np.asarray(a, np.float32)[None] * scale
    for s in range(3):
        ens.step(forcing)
    x = ens.chan_q_avg()
    level = np.median(x[:, ens.ids], axis=0).mean()
    del x
    thr = np.stack([np.full(N, f * level) for f in (0.5, 1.0, 2.0)])
    row = dict(size=size, pixels=N, channel_pixels=int(ens.Nk), members=M, thresholds=int(thr.shape[0]), steps_per_measurement=steps)
    host = HostFold(thr)
    ens.track_begin(NAME, thresholds=thr)                   # (the accumulators are made once, outside every measurement)
    trackers = ens._trackers

    def tracking(on):
        """paths a and c run the ensemble as it is without a tracker: step() sees none"""
        ens._trackers = trackers if on else {}

    def a(steps):
        tracking(False)
        for _ in range(steps):
            ens.step(forcing)

    def b(steps):
        tracking(True)
        ens.track_reset(NAME)                               # a new horizon: the first update reads no accumulator
        for _ in range(steps):
            ens.step(forcing)

    def c(steps):
        tracking(False)
        host.steps = 0
        for _ in range(steps):
            ens.step(forcing)
            host.update(ens.chan_q_avg())
    row.update(measure(dict(a=a, b=b, c=c), reps, steps))
    row["tracker_ms"] = row["b"]["ms"] - row["a"]["ms"]
    row["host_folds_ms"] = row["c"]["ms"] - row["a"]["ms"]
    # the same three steps on both paths
    tracking(True)
    ens.track_reset(NAME)
    host.steps = 0
    for _ in range(3):
        ens.step(forcing)
        host.update(ens.chan_q_avg())
    same = True
    for k in KEYS:
        got, want = ens.download("%s.%s" % (NAME, k)), host.acc[k]
        if got.dtype == np.int32:                           # (the int32 rows are not tracked outside the channel domain)
            got, want = got[..., ens.ids], want[..., ens.ids]
        same &= got.dtype == want.dtype and bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
    row["same_bits"] = bool(same)
    row["alone"] = kernel_alone(ens)
    row["tracked_step_within_step_plus_kernel_and_spread"] = bool(
        row["b"]["ms"] <= row["a"]["ms"] + row["alone"]["update_ms"] + row["a"]["spread_ms"])
    ens.free()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--members", default="4,16,51")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "members_track.json"))
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("at least 3 repetitions")
    doc = dict(device=_lib.device_name(0), reps=a.reps, copy_ceiling_bytes_per_s=COPY_CEILING, ensemble=[])
    for M in (int(x) for x in a.members.split(",") if x):
        doc["ensemble"].append(run(a.size, M, a.reps, a.steps))
        log(json.dumps(doc["ensemble"][-1]))
        with open(a.out, "w") as f:                         # (after every member count: the rows measured so far)
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
