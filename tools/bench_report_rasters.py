"""What report maps cost per model step when they are written every step: the products of an ensemble (and the `dis` map of a
single run) as float32 [H, W] rasters, fetched synchronously and converted on the host (all there was before) against packed
on the device and downloaded beside the next step (summary_rasters() / rasters()), in one process:

    python tools/bench_report_rasters.py [--size 2000] [--members 4,16,51] [--reps 5] [--steps 6]
                                         [--out profiles/report_rasters.json] [--kernel-only]

Inputs as tools/bench_members_summary.py: synthetic.hotpath_scenario (size x size), report=REPORT, every member forced by its
own scaling of synthetic.hotpath_forcing out of page-locked float32 arrays, three model steps before anything is timed.  The
products, of ChanQAvg: mean, minimum, maximum, the members above three threshold maps and three order statistics -- nine maps.
Three paths, alternating in one loop after one untimed round; each measurement is `steps` model steps, host clock from a
synchronised device to a synchronised device with every map on the host, divided by `steps`; median and spread (max - min) of
`reps` repetitions:
    a  step() alone
    b  step(), summary(), then per map output.decompress and astype(float32) (int32 for the exceedance counts)
    c  step(), summary_rasters(); the handle is waited for after the FOLLOWING step() has been issued
(c) - (a) against (b) - (a) is what the maps cost a step.  (b) and (c) give the same bits (checked once per member count).
The same three paths for one HotPathDevice and its `dis` map: decompress(chan_q_avg()).astype(float32) against
rasters(["ChanQAvg"]).  Alone, device stopwatch around 20 calls: the pack kernel of the nine product maps, its bytes (index
table per source, source rows, rasters) per second against the measured copy ceiling of the MI355X, 6.29 TB/s; and the
download of the nine rasters from a synchronised device, bytes per second against the 63 GB/s of the PCIe Gen5 x16 link.
--kernel-only: only the pack kernel alone, at 4 members (for a second process with LF_PACK_CELLS=1: one cell per lane)."""
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
from lisflood_amd import _lib, output  # noqa: E402
from lisflood_amd import synthetic as syn  # noqa: E402
from lisflood_amd.hotpath import FORCING, HotPathDevice, HotPathEnsemble  # noqa: E402

REPORT = ("TaPixel", "ThetaAll", "LZAvInflow", "Theta1bPixel", "Sat1", "GwLossCUM")
COPY_CEILING = 6.29e12       # B/s, float4 copy
LINK = 63e9                  # B/s, PCIe Gen5 x16
KERNEL_CALLS = 20


def log(text):
    print("[report_rasters] " + text, file=sys.stderr, flush=True)


def host_rasters(maps, mask):
    """today's path behind summary(): per map decompress and the conversion the writer wants"""
    out = {}
    for k, a in maps.items():
        dt = np.int32 if k == "exceed" else np.float32
        out[k] = output.decompress(a, mask).astype(dt) if a.ndim == 1 else np.stack([output.decompress(r, mask).astype(dt) for r in a])
    return out


def measure(paths, reps, steps):
    """paths: name -> fn(steps) that runs `steps` model steps and leaves the device idle and every map on the host"""
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
    out = {}
    for name, v in ms.items():
        out[name] = dict(ms=statistics.median(v), spread_ms=max(v) - min(v))
    out["maps_sync_ms"] = out["b"]["ms"] - out["a"]["ms"]
    out["maps_async_ms"] = out["c"]["ms"] - out["a"]["ms"]
    out["largest_spread_ms"] = max(out[k]["spread_ms"] for k in "abc")
    out["async_below_sync_by_more_than_the_spread"] = bool(out["maps_sync_ms"] - out["maps_async_ms"] > out["largest_spread_ms"])
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def pack_alone(ens, thr, ranks):
    """ms per pack launch of the nine product maps, and per download of the nine rasters"""
    L = _lib.lib()
    q = ens._summary_request("ChanQAvg", True, True, True, thr, ranks)
    maps = ens._summary_maps(q)
    ens._summary_outside(q, maps)
    _lib.check(L.lf_side_stream_join(0))
    ens._summary_kernels(q, maps)
    cells, N = ens.land_mask.size, ens.N
    table = ens._raster_table("pixel")
    srcs = list(maps.values())
    rows = [d.shape[0] if len(d.shape) == 2 else 1 for d in srcs]
    size = [4 * r * cells for r in rows]
    stage, pin = ens._report_buffers(0, sum(size))
    n, at = len(srcs), np.concatenate([[0], np.cumsum(size)[:-1]])
    kinds = [ens._PACK_KIND[d.dtype] for d in srcs]
    call = lambda: _lib.check(L.lf_pack_rasters_device(
        0, n, (C.c_void_p * n)(*[d.ptr.value for d in srcs]), (C.c_void_p * n)(*[stage.ptr.value + int(o) for o in at]),
        (C.c_int32 * n)(*rows), (C.c_int64 * n)(*[N] * n), (C.c_int32 * n)(*kinds),
        (C.c_int32 * n)(*[1 if k == 0 else k for k in kinds]), (C.c_double * n)(*[1.0] * n), table.ptr, cells, output.FILL))
    call()
    _lib.synchronize(0)
    _lib.timer_start(0)
    for _ in range(KERNEL_CALLS):
        call()
    ms = _lib.timer_stop(0) / KERNEL_CALLS
    moved = sum(4 * cells + r * N * (8 if k == 0 else 4) + 4 * r * cells for r, k in zip(rows, kinds))
    copies = []
    for _ in range(6):
        _lib.synchronize(0)
        t0 = time.perf_counter()
        _lib.check(L.lf_download_begin(0, 0))
        _lib.check(L.lf_download_copy(0, pin.ptr, stage.ptr, sum(size)))
        _lib.check(L.lf_download_end(0, 0))
        _lib.check(L.lf_download_wait(0, 0))
        copies.append((time.perf_counter() - t0) * 1e3)
    copy_ms = statistics.median(copies[1:])
    return dict(cells_per_lane=1 if os.environ.get("LF_PACK_CELLS", "")[:1] == "1" else 4, maps=sum(rows), pack_ms=ms,
                pack_bytes=moved, pack_bytes_per_s=moved / (ms * 1e-3), pack_fraction_of_copy_ceiling=moved / (ms * 1e-3) / COPY_CEILING,
                download_bytes=sum(size), download_ms=copy_ms, download_bytes_per_s=sum(size) / (copy_ms * 1e-3),
                download_fraction_of_link=sum(size) / (copy_ms * 1e-3) / LINK)


def run_ensemble(size, M, reps, steps, kernel_only=False):
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
    ranks = tuple(int(round(q * (M - 1))) for q in (0.25, 0.5, 0.75))
    row = dict(size=size, pixels=N, channel_pixels=int(ens.Nk), members=M, ranks=list(ranks), steps_per_measurement=steps)
    if not kernel_only:
        kept = {}

        def a(steps):
            for _ in range(steps):
                ens.step(forcing)

        def b(steps):
            for _ in range(steps):
                ens.step(forcing)
                kept["b"] = host_rasters(ens.summary("ChanQAvg", thresholds=thr, ranks=ranks), mask)

        def c(steps):
            pending = None
            for _ in range(steps):
                ens.step(forcing)
                if pending is not None:
                    kept["c"] = pending.wait()
                pending = ens.summary_rasters("ChanQAvg", thresholds=thr, ranks=ranks)
            kept["c"] = pending.wait()
        row.update(measure(dict(a=a, b=b, c=c), reps, steps))
        # the same step's maps on both paths: no step in between
        ref = host_rasters(ens.summary("ChanQAvg", thresholds=thr, ranks=ranks), mask)
        got = ens.summary_rasters("ChanQAvg", thresholds=thr, ranks=ranks).wait()
        row["same_bits"] = sorted(ref) == sorted(got) and all(same(ref[k], got[k]) for k in ref)
    row["alone"] = pack_alone(ens, thr, ranks)
    ens.free()
    return row


def run_single(size, reps, steps):
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(size, size, family="deep", block=1_000_000)
    N = int(mask.sum())
    hp = HotPathDevice(values, sc, mask, ldd_to_chan, ldd_kin, split=True, report=REPORT)
    log("%d^2, single run: built" % size)
    forcing = hp.pinned_forcing(np.float32)
    for k, a in syn.hotpath_forcing(N, 0).items():
        if k in FORCING:
            forcing[k][:] = np.asarray(a, np.float32)
    for s in range(3):
        hp.step(forcing, ordered=True)
    kept = {}

    def a(steps):
        for _ in range(steps):
            hp.step(forcing, ordered=True)

    def b(steps):
        for _ in range(steps):
            hp.step(forcing, ordered=True)
            kept["b"] = output.decompress(hp.chan_q_avg(), mask).astype(np.float32)

    def c(steps):
        pending = None
        for _ in range(steps):
            hp.step(forcing, ordered=True)
            if pending is not None:
                kept["c"] = pending.wait()
            pending = hp.rasters(["ChanQAvg"])
        kept["c"] = pending.wait()
    row = dict(size=size, pixels=N, channel_pixels=int(hp.Nk), steps_per_measurement=steps)
    row.update(measure(dict(a=a, b=b, c=c), reps, steps))
    row["same_bits"] = same(output.decompress(hp.chan_q_avg(), mask).astype(np.float32), hp.rasters(["ChanQAvg"]).wait()["ChanQAvg"])
    hp.free()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--members", default="4,16,51")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_rasters.json"))
    ap.add_argument("--append", action="store_true", help="keep what --out already holds")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--no-single", action="store_true", help="leave the HotPathDevice part out")
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("at least 3 repetitions")
    doc = dict(device=_lib.device_name(0), reps=a.reps, copy_ceiling_bytes_per_s=COPY_CEILING, link_bytes_per_s=LINK,
               ensemble=[], single=[], pack_kernel_only=[])
    if a.append and os.path.exists(a.out):
        with open(a.out) as f:
            doc.update(json.load(f))

    def save():
        with open(a.out, "w") as f:                         # (after every part: the rows measured so far)
            json.dump(doc, f, indent=1)
            f.write("\n")
    if a.kernel_only:
        doc["pack_kernel_only"].append(run_ensemble(a.size, 4, a.reps, a.steps, kernel_only=True))
        save()
    else:
        for M in (int(x) for x in a.members.split(",") if x):
            doc["ensemble"].append(run_ensemble(a.size, M, a.reps, a.steps))
            log(json.dumps(doc["ensemble"][-1]))
            save()
        if not a.no_single:
            doc["single"].append(run_single(a.size, a.reps, a.steps))
            log(json.dumps(doc["single"][-1]))
            save()
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
