"""What the products of an ensemble cost per model step: hotpath.HotPathEnsemble.summary() and sample(), which make them on
the device, against download() plus numpy on the host (all there was before), in one process:

    python tools/bench_members_summary.py [--size 2000] [--members 4,16,51] [--reps 5] [--out profiles/members_summary.json]
                                          [--append]

Inputs: synthetic.hotpath_scenario (size x size, fields drawn for a block of 10^6 pixels and repeated), a subset of the optional
maps reported (report=REPORT, to keep 51 members at 2000^2 well inside one device's memory), every member forced by its own
scaling of synthetic.hotpath_forcing, three model steps before anything is timed.  The products, of ChanQAvg: mean, minimum,
maximum, the members above three threshold maps, the order statistics at 0.25, 0.5 and 0.75 of members - 1 (rounded), and
every member at 64 gauges.  Two paths, alternating, after one untimed round; host clock from a synchronised device to the
moment the products are on the host; median and spread (max - min) of `reps` repetitions:
    host    chan_q_avg() (every member's full vector over PCIe, scattered to the land domain with numpy), then numpy: the sum
            and the folds member by member, np.sort(kind="stable") for the order statistics, fancy indexing for the gauges
    device  summary("ChanQAvg", thresholds=, ranks=) and sample("ChanQAvg", gauges)
Both give the same bits (checked once per member count).  For lf_members_summary_device alone (device stopwatch around 20 calls,
every output and three thresholds), on the channel rows (n = channel pixels) and on a land row (n = all pixels): bytes read
per second, members * 8 B per element, against the measured copy ceiling of the MI355X, 6.29 TB/s."""
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
LAND_ROW = "DirectRunoff"
KERNEL_CALLS = 20


def npmin(a, b):
    return np.where(a != a, a, np.where(b != b, b, np.where(b < a, b, a)))


def npmax(a, b):
    return np.where(a != a, a, np.where(b != b, b, np.where(b > a, b, a)))


def host_products(ens, thr, ranks, pix):
    x = ens.chan_q_avg()
    acc, lo, hi = x[0].copy(), x[0].copy(), x[0].copy()
    exceed = np.zeros(thr.shape, np.int32)
    for m in range(x.shape[0]):
        if m:
            acc = acc + x[m]
            lo, hi = npmin(lo, x[m]), npmax(hi, x[m])
        for t in range(thr.shape[0]):
            exceed[t] += x[m] > thr[t]
    order = np.sort(x, axis=0, kind="stable")[list(ranks)]
    return dict(mean=acc / np.float64(x.shape[0]), min=lo, max=hi, exceed=exceed, order=order), x[:, pix]


def device_products(ens, thr, ranks, pix):
    return ens.summary("ChanQAvg", thresholds=thr, ranks=ranks), ens.sample("ChanQAvg", pix)


def timed(fn):
    _lib.synchronize(0)
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def kernel_alone(ens, name, thr):
    """ms per lf_members_summary_device call with every output and the thresholds, and the bytes of the member rows it reads"""
    L = _lib.lib()
    src, n, stride, divisor, channel = ens._product_rows(name)
    d_thr, T, _ = ens._cached(ens._thresholds, thr, channel, ens._upload_thresholds)
    index = ens._row_index(channel)
    outs = [ens._product(k, ens.N) for k in ("mean", "min", "max")]
    exceed = ens._product("exceed", (T, ens.N), np.int32)
    call = lambda: _lib.check(L.lf_members_summary_device(0, src.ptr, ens.members, stride, n, divisor, index.ptr, ens.N, outs[0].ptr,
                                                          outs[1].ptr, outs[2].ptr, T, d_thr.ptr, n, exceed.ptr))
    _lib.check(L.lf_side_stream_join(0))
    call()
    _lib.synchronize(0)
    _lib.timer_start(0)
    for _ in range(KERNEL_CALLS):
        call()
    ms = _lib.timer_stop(0) / KERNEL_CALLS
    read = ens.members * n * 8
    return dict(row=name, elements=int(n), ms=ms, member_bytes_read=read, read_bytes_per_s=read / (ms * 1e-3),
                fraction_of_copy_ceiling=read / (ms * 1e-3) / COPY_CEILING)


def run(size, M, reps):
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(size, size, family="deep", block=1_000_000)
    N = int(mask.sum())
    ens = HotPathEnsemble(values, sc, mask, ldd_to_chan, ldd_kin, M, split=True, report=REPORT)
    print("[members_summary] %d^2, %d members: built" % (size, M), file=sys.stderr, flush=True)
    scale = (1.0 + 0.02 * np.arange(M, dtype=np.float32))[:, None]
    for s in range(3):
        ens.step({k: np.asarray(a, np.float32)[None] * scale for k, a in syn.hotpath_forcing(N, s).items() if k in FORCING})
    print("[members_summary] %d^2, %d members: stepped" % (size, M), file=sys.stderr, flush=True)
    x = ens.chan_q_avg()
    level = np.median(x[:, ens.ids], axis=0).mean()
    thr = np.stack([np.full(N, f * level) for f in (0.5, 1.0, 2.0)])
    ranks = tuple(int(round(q * (M - 1))) for q in (0.25, 0.5, 0.75))
    pix = np.random.default_rng(1).choice(ens.ids, 64, replace=False)
    del x
    paths = (("host", host_products), ("device", device_products))
    ms = {k: [] for k, _ in paths}
    last = {}
    for rep in range(reps + 1):                             # the first round of both paths is the warm-up
        for name, fn in paths:
            t, last[name] = timed(lambda: fn(ens, thr, ranks, pix))
            print("[members_summary] round %d %s %.1f ms" % (rep, name, t), file=sys.stderr, flush=True)
            if rep:
                ms[name].append(t)
    (maps_h, gauges_h), (maps_d, gauges_d) = last["host"], last["device"]
    equal = all(same(maps_h[k], maps_d[k]) for k in maps_h) and same(gauges_h, gauges_d)
    row = dict(size=size, pixels=N, channel_pixels=int(ens.Nk), members=M, ranks=list(ranks), gauges=int(pix.size),
               same_bits=equal, host_bytes_over_pcie=M * ens.kstride * 8,
               device_bytes_over_pcie=(3 + len(ranks)) * N * 8 + 3 * N * 4 + M * pix.size * 8)
    for name, _ in paths:
        med = statistics.median(ms[name])
        row[name] = dict(ms=med, spread_ms=max(ms[name]) - min(ms[name]), relative_spread=(max(ms[name]) - min(ms[name])) / med)
    row["device_over_host"] = row["device"]["ms"] / row["host"]["ms"]
    row["kernel_alone"] = [kernel_alone(ens, "ChanQAvg", thr), kernel_alone(ens, LAND_ROW, thr)]
    ens.free()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--members", default="4,16,51")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "members_summary.json"))
    ap.add_argument("--append", action="store_true", help="keep the rows --out already holds (another size, same box)")
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("at least 3 repetitions")
    doc = dict(device=_lib.device_name(0), reps=a.reps, copy_ceiling_bytes_per_s=COPY_CEILING, results=[])
    if a.append and os.path.exists(a.out):
        with open(a.out) as f:
            doc["results"] = json.load(f)["results"]
    for M in (int(x) for x in a.members.split(",")):
        doc["results"].append(run(a.size, M, a.reps))
        print("[members_summary] %s" % json.dumps(doc["results"][-1]), file=sys.stderr, flush=True)
        with open(a.out, "w") as f:                         # (after every member count: the rows measured so far)
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
