"""What spread in the forcing costs an ensemble per model step: hotpath.HotPathEnsemble with Rain and ETRef perturbed from
`rank` patterns on the device (forcing_perturbation + coefficients, lf_upload_perturb_rows: only [members, rank] tables cross
PCIe) against the same rows made on the host and sent over the link, in one process:

    python tools/bench_members_perturb.py [--size 2000] [--members 4,16,51] [--rank 8] [--reps 5] [--steps 4]
                                          [--out profiles/members_perturb.json]

Inputs: the scenario of tools/bench_members_upload.py (synthetic.hotpath_scenario, synthetic.hotpath_forcing),
assimilation.fourier_patterns and ar1_coefficients.  A leg is a window of `steps` prefetched model steps of the whole ensemble,
timed with the host clock from a synchronised device to a synchronised device (bench_members_upload.py's window: every step
hands over the forcing of the step after it); its figure is the window over `steps`.  Legs, alternating, after one untimed
round of all of them; median and spread (max - min) of `reps` repetitions:
    shared       (a) [N] float64 forcing and nothing else: the lower line, which cannot carry spread
    host_rows    (b) Rain and ETRef as [members, N] float64 rows, page-locked, made on the host by the restatement
                 (tests/members_perturb.py: perturb(), chunk by chunk) before the clock starts; `numpy_ms` is what making the
                 rows of ONE step costs the host, measured apart and not part of the leg
    device       (c) [N] forcing plus coefficients: the rows are written on the device behind the upload
Per row also the kernel alone on one row set (Rain of the set in use; zero coefficients, so the rows keep their values while
the arithmetic is the same) in both forms -- spread from member 0's row (base_dev = rows_dev) and in place -- as bytes per
second against the measured copy ceiling of the MI355X, 6.29 TB/s, with the bytes-per-element model 8 (rank + 1 + members)
and 8 (rank + 2 members); `device_over_shared_ms` = (c) - (a) beside `kernels_ms`, the two spreading kernels of a step, and
`explained`: (c) - (a) <= kernels_ms + the spread of (a)."""
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
from lisflood_amd import assimilation as AS  # noqa: E402
from lisflood_amd import synthetic as syn  # noqa: E402
from lisflood_amd.hotpath import FORCING, HotPathEnsemble  # noqa: E402

COPY_CEILING = 6.29e12            # B/s, float4 copy (measured)
KERNEL_CALLS = 20
CHUNK = 4096                      # columns per numpy chunk
PERTURBED = {"Rain": (True, 0.0, np.inf), "ETRef": (False, 0.0, np.inf)}      # name -> multiplicative, lower, upper


def log(text):
    print("[members_perturb] " + text, file=sys.stderr, flush=True)


def host_rows(f, c, P, multiplicative, lower, upper, out):
    """tests/members_perturb.py: perturb() with base = f [N], chunk by chunk over the columns, into out [members, N]"""
    cols = [np.ascontiguousarray(c[:, r][:, None]) for r in range(P.shape[0])]
    with np.errstate(all="ignore"):
        for a in range(0, f.size, CHUNK):
            p = P[:, a:a + CHUNK]
            s = cols[0] * p[0][None, :]
            for r in range(1, P.shape[0]):
                s = s + cols[r] * p[r][None, :]
            b = f[None, a:a + CHUNK]
            v = b * (1.0 + s) if multiplicative else b + s
            v = np.where((lower > v) | ((lower != lower) & (v == v)), lower, v)
            out[:, a:a + CHUNK] = np.where((upper < v) | ((upper != upper) & (v == v)), upper, v)


def window(prime, body, steps):
    prime()
    _lib.synchronize(0)
    t0 = time.perf_counter()
    for s in range(steps):
        body(s)
    _lib.synchronize(0)
    return (time.perf_counter() - t0) * 1e3 / steps


def kernel_alone(ens, rank, patterns_dev):
    """ms per lf_members_perturb_device on the member rows of Rain (the set in use), both forms"""
    L, M, N = _lib.lib(), ens.members, ens.N
    rows, zero = ens.force[ens._cur]["Rain"].ptr, np.zeros((M, rank))
    out = {}
    for key, base, per_element in (("from_member_0", rows, 8 * (rank + 1 + M)), ("in_place", None, 8 * (rank + 2 * M))):
        call = lambda: _lib.check(L.lf_members_perturb_device(0, rows, M, ens.pstride, N, base, rank, patterns_dev.ptr, N,
                                                              _lib.ptr(zero), 1, None, 0.0, None, np.inf))
        _lib.check(L.lf_side_stream_join(0))
        call()
        _lib.synchronize(0)
        _lib.timer_start(0)
        for _ in range(KERNEL_CALLS):
            call()
        ms = _lib.timer_stop(0) / KERNEL_CALLS
        moved = per_element * N
        out[key] = dict(ms=ms, bytes_per_element=per_element, bytes=moved, bytes_per_s=moved / (ms * 1e-3),
                        fraction_of_copy_ceiling=moved / (ms * 1e-3) / COPY_CEILING, operations=(2 * rank + 2) * M * N)
    return out


def run(size, M, rank, reps, steps):
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(size, size, family="deep", block=1_000_000)
    N = int(mask.sum())
    ens = HotPathEnsemble(values, sc, mask, ldd_to_chan, ldd_kin, M, split=True)
    log("%d^2, %d members: built" % (size, M))
    rng = np.random.default_rng(M)
    patterns = {k: AS.fourier_patterns(mask, rank, 40.0, rng) for k in PERTURBED}
    coeff = [{k: AS.ar1_coefficients(None, (M, rank), 0.3, rng) for k in PERTURBED} for _ in range(2)]
    shared = [ens.pinned_forcing(per_member=False) for _ in range(2)]
    for s in range(2):
        for k, a in syn.hotpath_forcing(N, s).items():
            shared[s][k][...] = a
    # (b): one page-locked set (two would be 2 x 2 x members x N x 8 bytes of page-locked memory), refilled never: the rows
    # of step 0, handed over every step behind upload_wait()
    rows = dict(shared[0])
    pinned = {k: _lib.PinnedArray((M, N), np.float64) for k in PERTURBED}
    numpy_ms = []
    for rep in range(3 if M <= 16 else 1):
        t0 = time.perf_counter()
        for k, (multiplicative, lower, upper) in PERTURBED.items():
            host_rows(shared[0][k], coeff[0][k], patterns[k], multiplicative, lower, upper, pinned[k].a)
        numpy_ms.append((time.perf_counter() - t0) * 1e3)
    rows.update({k: pinned[k].a for k in PERTURBED})
    log("host rows made: %s ms" % numpy_ms)

    def plain(sets):
        def body(s):
            ens.step(sets[s % len(sets)])
            ens.upload_wait()
            ens.prefetch(sets[(s + 1) % len(sets)])
        return lambda: window(lambda: ens.prefetch(sets[0]), body, steps)

    def device():
        def body(s):
            ens.step(shared[s % 2])
            ens.upload_wait()
            ens.prefetch(shared[(s + 1) % 2], coefficients=coeff[(s + 1) % 2])
        return window(lambda: ens.prefetch(shared[0], coefficients=coeff[0]), body, steps)

    def registered(on):
        for k, (multiplicative, lower, upper) in PERTURBED.items():
            ens.forcing_perturbation(k, patterns[k] if on else None, multiplicative, lower, upper)
    registered(True)
    # the same bits by both routes, once
    ens.step(shared[0], coefficients=coeff[0])
    got = {k: ens.download(k) for k in PERTURBED}
    canon = lambda a: np.where(np.isnan(a), np.float64(np.nan), a).view(np.uint64)
    same = all(np.array_equal(canon(got[k]), canon(pinned[k].a)) for k in PERTURBED)
    del got
    legs = [("shared", plain(shared)), ("host_rows", plain([rows])), ("device", device)]
    ms = {k: [] for k, _ in legs}
    for rep in range(reps + 1):                             # the first round of all legs is the warm-up
        for name, fn in legs:
            t = fn()
            log("round %d %s %.2f ms" % (rep, name, t))
            if rep:
                ms[name].append(t)
    row = dict(size=size, pixels=N, members=M, rank=rank, steps_per_window=steps, perturbed=list(PERTURBED), same_bits=bool(same),
               numpy_ms=dict(ms=statistics.median(numpy_ms), runs=len(numpy_ms)),
               link_bytes_per_step=dict(shared=5 * N * 8, host_rows=(3 + 2 * M) * N * 8, device=5 * N * 8 + 2 * M * rank * 8))
    for name, _ in legs:
        med = statistics.median(ms[name])
        row[name] = dict(ms_per_model_step=med, spread_ms=max(ms[name]) - min(ms[name]))
    ens.step(shared[0], coefficients=coeff[0])              # (member rows in the set in use)
    row["alone"] = kernel_alone(ens, rank, ens._perturbations["Rain"][0])
    row["kernels_ms"] = 2 * row["alone"]["from_member_0"]["ms"]
    row["device_over_shared_ms"] = row["device"]["ms_per_model_step"] - row["shared"]["ms_per_model_step"]
    row["explained"] = bool(row["device_over_shared_ms"] <= row["kernels_ms"] + row["shared"]["spread_ms"])
    row["device_over_host_rows"] = row["device"]["ms_per_model_step"] / row["host_rows"]["ms_per_model_step"]
    registered(False)
    for p in pinned.values():
        p.free()
    ens.free()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--members", default="4,16,51")
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4, help="model steps per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "members_perturb.json"))
    a = ap.parse_args()
    if a.reps < 5 or a.steps < 2:
        ap.error("at least 5 repetitions of at least 2 steps")
    doc = dict(device=_lib.device_name(0), reps=a.reps, steps_per_window=a.steps, copy_ceiling_bytes_per_s=COPY_CEILING, ensemble=[])
    for M in (int(x) for x in a.members.split(",") if x):
        doc["ensemble"].append(run(a.size, M, a.rank, a.reps, a.steps))
        log(json.dumps(doc["ensemble"][-1]))
        with open(a.out, "w") as f:                         # (after every member count: the rows measured so far)
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
