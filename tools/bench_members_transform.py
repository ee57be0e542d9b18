"""What the analysis step of an assimilation cycle costs: every member's state rewritten on the device
(HotPathEnsemble.transform with a taper and bounds, HotPathEnsemble.resample with half the members replaced) against the
host route there was before -- download(name), the same sums in numpy, set_member_state(name) -- in one process:

    python tools/bench_members_transform.py [--size 2000] [--members 4,16,51] [--reps 5] [--host-names LZ] [--host-full-members 4]
                                            [--out profiles/members_transform.json]

Inputs as tools/bench_members_track.py: synthetic.hotpath_scenario (size x size), report=REPORT, every member forced by its
own scaling of synthetic.hotpath_forcing, three model steps before anything is timed.  Three paths, alternating in one loop
after one untimed round, host clock from a synchronised device to a synchronised device, median and spread (max - min) of
`reps` repetitions:
    transform  ens.transform(W, taper=, bounds=) on every vector of analysis_names(): the full default state
    resample   ens.resample(parents) on the same vectors, every second member replaced by its neighbour
    host       download + numpy + set_member_state of the vectors of --host-names ONLY (one [N] row by default: the full
               state by that route is its bytes / the bytes of those vectors times as much, given as
               host_full_state_ms_scaled and marked as scaled, not measured -- at 51 members it would take minutes per
               repetition)
    host_full  the same route over EVERY vector of analysis_names(), with the bounds of the transform path: the comparison
               for the full state, measured -- up to --host-full-members members (4 by default; about 17 s a repetition)
The numpy sums are the restatement of tests/members_transform.py evaluated in column chunks that stay in cache: the same
bits (checked once per member count against the device), the fastest form of that arithmetic numpy has.
Alone, device stopwatch (lf_timer_start / lf_timer_stop) around 20 calls of lf_members_transform_device on the member rows
of one [N] vector: bytes moved (every row read and written once) per second against the measured copy ceiling the other
member kernels report against, 6.29 TB/s, and multiplies and adds (2 members^2 per element, never fused) per second
against the SPEC-SHEET fp64 vector rate -- 78.6 TFLOPS counted as fused multiply-adds, 39.3e12 unfused operations per
second; nobody has measured that rate here."""
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
COPY_CEILING = 6.29e12            # B/s, float4 copy (measured)
SPEC_FP64_UNFUSED = 39.3e12       # operations/s: the spec sheet's 78.6 TFLOPS are fused multiply-adds counted twice
KERNEL_CALLS = 20
CHUNK = 4096                      # columns per numpy chunk: [51, 4096] doubles are 1.6 MB


def log(text):
    print("[members_transform] " + text, file=sys.stderr, flush=True)


def host_transform(x, W, taper, lower, upper):
    """tests/members_transform.py: transform(), chunk by chunk over the columns; x [members, n] -> new array"""
    M, n = x.shape
    out = np.empty_like(x)
    cols = [np.ascontiguousarray(W[k][:, None]) for k in range(M)]
    with np.errstate(all="ignore"):
        for a in range(0, n, CHUNK):
            c = x[:, a:a + CHUNK]
            t = c[0][None, :] * cols[0]
            for k in range(1, M):
                t = t + c[k][None, :] * cols[k]
            v = c + taper[None, a:a + CHUNK] * (t - c)
            lo = lower if np.ndim(lower) == 0 else lower[None, a:a + CHUNK]
            hi = upper if np.ndim(upper) == 0 else upper[None, a:a + CHUNK]
            v = np.where((lo > v) | ((lo != lo) & (v == v)), lo, v)
            out[:, a:a + CHUNK] = np.where((hi < v) | ((hi != hi) & (v == v)), hi, v)
    return out


def measure(paths, reps):
    ms = {k: [] for k in paths}
    for rep in range(reps + 1):                             # the first round of every path is the warm-up
        for name, fn in paths.items():
            _lib.synchronize(0)
            t0 = time.perf_counter()
            fn()
            _lib.synchronize(0)
            t = (time.perf_counter() - t0) * 1e3
            log("round %d %s %.2f ms" % (rep, name, t))
            if rep:
                ms[name].append(t)
    return {name: dict(ms=statistics.median(v), spread_ms=max(v) - min(v)) for name, v in ms.items()}


def state_bytes(ens, names):
    return sum(8 * ens.members * n * 1 for name in names for _, n, _, _, _ in ens._analysis_rows(name))


def kernel_alone(ens, w, taper, name):
    """ms per lf_members_transform_device on the member rows of one [N] vector, plain and with taper and both bound rows"""
    L, M = _lib.lib(), ens.members
    (base, n, stride, order, _), = ens._analysis_rows(name)
    tp = ens._pixel_rows(taper, order).ptr
    out = {}
    for key, args in (("plain", (None, None, -np.inf, None, np.inf)), ("taper_and_bound_rows", (tp, tp, 0.0, tp, 0.0))):
        call = lambda: _lib.check(L.lf_members_transform_device(0, base, M, stride, n, w.ptr, *args))
        _lib.check(L.lf_side_stream_join(0))
        call()
        _lib.synchronize(0)
        _lib.timer_start(0)
        for _ in range(KERNEL_CALLS):
            call()
        out[key + "_ms"] = _lib.timer_stop(0) / KERNEL_CALLS
    ms, moved, ops = out["plain_ms"], 16 * M * n, 2 * M * M * n
    out.update(elements=n, bytes=moved, bytes_per_s=moved / (ms * 1e-3), fraction_of_copy_ceiling=moved / (ms * 1e-3) / COPY_CEILING,
               operations=ops, operations_per_s=ops / (ms * 1e-3),
               fraction_of_spec_sheet_fp64_unfused=ops / (ms * 1e-3) / SPEC_FP64_UNFUSED)
    return out


def run(size, M, reps, host_names, host_full):
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
    rng = np.random.default_rng(M)
    weights = 0.8 * np.eye(M) + 0.2 * rng.dirichlet(np.ones(M), M).T          # convex: the state stays physical
    taper = rng.uniform(0.0, 1.0, N)
    zeros = np.zeros(N)
    names = ens.analysis_names()
    bounds = {k: (0.0, None) for k in names}                                   # a scalar bound on every vector ...
    bounds.update({k: (zeros, None) for k in host_names})                      # ... and a row on the ones the host route takes
    parents = np.arange(M, dtype=np.int32)
    parents[1::2] = parents[0:M - 1:2]
    row = dict(size=size, pixels=N, channel_pixels=int(ens.Nk), members=M, vectors=len(names),
               row_sets=sum(len(ens._analysis_rows(k)) for k in names), state_bytes=state_bytes(ens, names),
               host_names=list(host_names), host_bytes=state_bytes(ens, host_names))

    def host():
        for k in host_names:
            ens.set_member_state(k, host_transform(ens.download(k), weights, taper, zeros, np.inf))

    def host_all():
        for k in names:
            x = ens.download(k)
            flat = x.reshape(M, -1)
            reps_of = flat.shape[1] // N
            lower = np.tile(zeros, reps_of) if k in host_names else 0.0
            ens.set_member_state(k, host_transform(flat, weights, np.tile(taper, reps_of), lower, np.inf).reshape(x.shape))

    # the same bits by both routes, once: the device on a copy of what the host route starts from
    k = host_names[0]
    start = ens.download(k)
    want = host_transform(start, weights, taper, zeros, np.inf)
    ens.transform(weights, names=[k], taper=taper, bounds={k: bounds[k]})
    got = ens.download(k)
    canon = lambda a: np.where(np.isnan(a), np.float64(np.nan), a).view(np.uint64)
    row["same_bits"] = bool(np.array_equal(canon(got), canon(want)))
    del start, want, got
    paths = dict(transform=lambda: ens.transform(weights, taper=taper, bounds=bounds), resample=lambda: ens.resample(parents),
                 host=host)
    if host_full:
        paths["host_full"] = host_all
    row.update(measure(paths, reps))
    row["host_full_state_ms_scaled"] = row["host"]["ms"] * row["state_bytes"] / row["host_bytes"]
    row["device_beats_host"] = bool(max(row["transform"]["ms"], row["resample"]["ms"]) < row["host"]["ms"])
    if host_full:
        row["device_beats_host_full"] = bool(max(row["transform"]["ms"], row["resample"]["ms"]) < row["host_full"]["ms"])
    w = ens._weights[1]
    row["alone"] = kernel_alone(ens, w, taper, host_names[0])
    ens.free()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--members", default="4,16,51")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-names", default="LZ")
    ap.add_argument("--host-full-members", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "members_transform.json"))
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("at least 3 repetitions")
    doc = dict(device=_lib.device_name(0), reps=a.reps, copy_ceiling_bytes_per_s=COPY_CEILING,
               spec_sheet_fp64_unfused_operations_per_s=SPEC_FP64_UNFUSED, ensemble=[])
    for M in (int(x) for x in a.members.split(",") if x):
        doc["ensemble"].append(run(a.size, M, a.reps, [k for k in a.host_names.split(",") if k], M <= a.host_full_members))
        log(json.dumps(doc["ensemble"][-1]))
        with open(a.out, "w") as f:                         # (after every member count: the rows measured so far)
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
