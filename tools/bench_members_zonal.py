"""What an areal product of an ensemble costs: hotpath.HotPathEnsemble.zonal(), which sums the member rows over zones on the
device, against download() plus np.bincount on the host (all there was before), in one process:

    python tools/bench_members_zonal.py [--size 2000] [--members 4,16,51] [--reps 5] [--out profiles/members_zonal.json]

Inputs: synthetic.hotpath_scenario (size x size, fields drawn for a block of 10^6 pixels and repeated), a subset of the optional
maps reported (report=REPORT, to keep 51 members at 2000^2 well inside one device's memory), every member forced by its own
scaling of synthetic.hotpath_forcing, three model steps before anything is timed.  The product: the zone means of
Theta1aPixel over three zone sets, each a label map -- one zone over the whole domain, 64 compact blocks (8 x 8), and
footprints of 5 x 5 pixels on a lattice 25 pixels apart (6 400 of them at 2000^2; the pixels between them are in no zone).
Two paths, alternating, after one untimed round; host clock from a synchronised device to the moment the [members, zones]
means are on the host; median and spread (max - min) of `reps` repetitions:
    host    download("Theta1aPixel") (every member's full vector over PCIe, permuted into pixel order with numpy), then
            np.bincount(labels, weights=row) per member, divided by the pixel counts
    device  zonal("Theta1aPixel", labels)
The two agree to rounding (another order of the additions; the largest relative difference is reported); the device path has
the bits of the plan's own host sums on the download (checked at the first member count).  For the first pass alone
(lf_members_zonal_device, device stopwatch around 20 calls): bytes read per second, members * 8 B per entry plus the 4 B index
once, against the measured copy ceiling of the MI355X, 6.29 TB/s -- with the default launch shape, with every wavefront
walking all members (LF_ZONAL_GRID=0) and with the members on the grid (LF_ZONAL_GRID=1)."""
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

REPORT = ("TaPixel", "ThetaAll", "LZAvInflow", "Theta1aPixel", "Sat1", "GwLossCUM")
COPY_CEILING = 6.29e12       # B/s, float4 copy
ROW = "Theta1aPixel"
KERNEL_CALLS = 20


def zone_sets(mask):
    size = mask.shape[0]
    rows, cols = np.nonzero(mask)
    block = -(-size // 8)
    foot = np.where((rows % 25 < 5) & (cols % 25 < 5), (rows // 25) * (-(-size // 25)) + cols // 25, -1)
    return {"whole": np.zeros(rows.size, np.int32), "blocks64": ((rows // block) * 8 + cols // block).astype(np.int32),
            "footprints": foot.astype(np.int32)}


def host_means(ens, labels):
    x = ens.download(ROW)
    inside = labels >= 0
    lab = labels[inside]
    Z = int(lab.max()) + 1
    count = np.bincount(lab, minlength=Z)
    with np.errstate(all="ignore"):
        return np.stack([np.bincount(lab, weights=x[m, inside], minlength=Z) for m in range(x.shape[0])]) / count


def timed(fn):
    _lib.synchronize(0)
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def first_pass_alone(ens, labels):
    """ms per call of pass 1 and of all passes, by launch shape, and the bytes pass 1 reads"""
    L = _lib.lib()
    src, _, stride, divisor, channel = ens._product_rows(ROW)
    t = ens._zonal_tables(labels, None, channel)
    plan, M = t.plan, ens.members

    def passes(count):
        rows, s, entries = src.ptr, stride, plan.entries
        for p in range(count):
            runs, out = plan.runs(p), t.partial[p % 2]
            _lib.check(L.lf_members_zonal_device(0, rows, M, s, divisor if p == 0 else 1.0, entries, t.index.ptr if p == 0 else None,
                                                 None, runs, t.run_start[p].ptr, out.ptr, runs))
            rows, s, entries = out.ptr, runs, runs

    def stopwatch(count):
        passes(count)
        _lib.synchronize(0)
        _lib.timer_start(0)
        for _ in range(KERNEL_CALLS):
            passes(count)
        return _lib.timer_stop(0) / KERNEL_CALLS
    _lib.check(L.lf_side_stream_join(0))
    read = M * plan.entries * 8 + plan.entries * 4
    out = dict(entries=plan.entries, runs=plan.runs(0), passes=plan.passes, bytes_read=read)
    for shape, env in (("default", None), ("walk_members", "0"), ("members_on_grid", "1")):
        os.environ.pop("LF_ZONAL_GRID", None)
        if env is not None:
            os.environ["LF_ZONAL_GRID"] = env
        ms = stopwatch(1)
        out[shape] = dict(first_pass_ms=ms, all_passes_ms=stopwatch(plan.passes), read_bytes_per_s=read / (ms * 1e-3),
                          fraction_of_copy_ceiling=read / (ms * 1e-3) / COPY_CEILING)
    os.environ.pop("LF_ZONAL_GRID", None)
    return out


def run(size, M, reps, check_bits):
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(size, size, family="deep", block=1_000_000)
    N = int(mask.sum())
    ens = HotPathEnsemble(values, sc, mask, ldd_to_chan, ldd_kin, M, split=True, report=REPORT)
    print("[members_zonal] %d^2, %d members: built" % (size, M), file=sys.stderr, flush=True)
    scale = (1.0 + 0.02 * np.arange(M, dtype=np.float32))[:, None]
    for s in range(3):
        ens.step({k: np.asarray(a, np.float32)[None] * scale for k, a in syn.hotpath_forcing(N, s).items() if k in FORCING})
    print("[members_zonal] %d^2, %d members: stepped" % (size, M), file=sys.stderr, flush=True)
    rows = []
    for kind, labels in zone_sets(mask).items():
        paths = (("host", lambda: host_means(ens, labels)), ("device", lambda: ens.zonal(ROW, labels)))
        ms, last = {k: [] for k, _ in paths}, {}
        for rep in range(reps + 1):                             # the first round of both paths is the warm-up (and the plan)
            for name, fn in paths:
                t, last[name] = timed(fn)
                print("[members_zonal] %s round %d %s %.1f ms" % (kind, rep, name, t), file=sys.stderr, flush=True)
                if rep:
                    ms[name].append(t)
        plan = ens.zonal_plan(labels, None, ROW)
        with np.errstate(all="ignore"):
            rel = float(np.nanmax(np.abs(last["device"] - last["host"]) / np.abs(last["host"])))
        row = dict(size=size, pixels=N, members=M, zones_kind=kind, zones=plan.zones, entries=plan.entries, passes=plan.passes,
                   largest_relative_difference_to_bincount=rel, host_bytes_over_pcie=M * ens.pstride * 8,
                   device_bytes_over_pcie=M * plan.zones * 8)
        if check_bits:
            x = ens.download(ROW)
            with np.errstate(all="ignore"):
                want = plan.sums(x[:, plan.pixels]) / plan.weight_sum
            row["same_bits_as_the_host_sums_of_the_plan"] = bool(np.array_equal(want.view(np.uint64), last["device"].view(np.uint64)))
            del x
        for name, _ in paths:
            med = statistics.median(ms[name])
            row[name] = dict(ms=med, spread_ms=max(ms[name]) - min(ms[name]), relative_spread=(max(ms[name]) - min(ms[name])) / med)
        row["device_over_host"] = row["device"]["ms"] / row["host"]["ms"]
        row["first_pass_alone"] = first_pass_alone(ens, labels)
        print("[members_zonal] %s" % json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    ens.free()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--members", default="4,16,51")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "members_zonal.json"))
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("at least 3 repetitions")
    doc = dict(device=_lib.device_name(0), reps=a.reps, copy_ceiling_bytes_per_s=COPY_CEILING, row=ROW, results=[])
    for i, M in enumerate(int(x) for x in a.members.split(",")):
        doc["results"] += run(a.size, M, a.reps, i == 0)
        with open(a.out, "w") as f:                         # (after every member count: the rows measured so far)
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
