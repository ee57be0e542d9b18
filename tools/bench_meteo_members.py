"""What snow and frost on the device cost an ensemble per model step: hotpath.HotPathEnsemble(meteo=...), whose forcing is
precipitation and temperature and whose first launch is lf_snow_frost_members_device, against the same ensemble without
meteo= fed the Rain / SnowMelt rows a host would have to make per member and step, in one process:

    python tools/bench_meteo_members.py [--size 2000] [--members 4,16,51] [--rank 8] [--reps 5] [--steps 4]
                                        [--out profiles/meteo_members.json]

Inputs: synthetic.hotpath_scenario / hotpath_forcing as tools/bench_members_perturb.py takes them; snow statics, packs, frost
index, precipitation and temperature seeded here (uniform, as tests/snow_frost.py draws them, without its planted cases).  A
leg is a window of `steps` prefetched model steps, host clock from a synchronised device to a synchronised device, its figure
the window over `steps`; median and spread (max - min) of `reps` repetitions after one untimed round.  An ensemble of 51
members at 2000^2 fills most of the device, so the two objects live one after the other and the legs alternate within each:
    without meteo=   shared      [N] Rain / SnowMelt / E*Ref: the step as it was, which cannot carry snow
                     host_rows   (1) Rain and SnowMelt as [members, N] float64 rows, page-locked, made before the clock starts;
                                 `numpy_ms` is what the restatement of snow and frost costs the host for the members of ONE
                                 step (chunk by chunk, measured apart, not part of the leg)
    with meteo=      meteo       (2) [N] Precipitation / Tavg / E*Ref, the kernel in front of the land surface
                     perturbed   (3) the same with Tavg (additive) and Precipitation (multiplicative) perturbed at `rank`
(4) the kernel alone on the row set in use: ms per call over KERNEL_CALLS calls between device events, and its rate over
the bytes it has to move -- per member and pixel 48 B read and 57 B written (65 with Snow), per pixel and slice of 8 members
24 B of statics, and with one forcing row for all 16 B of meteo per pixel and slice instead of per member -- against the
measured copy ceiling of the MI355X, 6.29 TB/s.  `front_end_ms` = (2) - shared beside `kernel_ms`, and `explained`:
(2) - shared <= kernel_ms + the spread of (2)."""
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
from lisflood_amd import assimilation as AS  # noqa: E402
from lisflood_amd import synthetic as syn  # noqa: E402
from lisflood_amd.hotpath import HotPathEnsemble  # noqa: E402

COPY_CEILING = 6.29e12            # B/s, float4 copy (measured)
KERNEL_CALLS = 20
CHUNK = 4096                      # columns per numpy chunk
SCALARS = dict(TempSnow=1.0, TempMelt=0.0, IceMeltCoef=7.0, DtDay=1.0, Afrost=0.97, SnowWaterEquivalent=0.45,
               FrostIndexThreshold=56.0)
SEASON = (0.5, 0.25)


def log(text):
    print("[meteo_members] " + text, file=sys.stderr, flush=True)


def host_snow_frost(m, zones, frost, P, T, rain, melt, frozen):
    """snow.dynamic and frost.dynamic of every member in numpy, as tests/snow_frost.py restates them, chunk by chunk over the
    columns: zones [members, 3, N] and frost [members, N] advanced in place, Rain / SnowMelt / isFrozenSoil rows written"""
    with np.errstate(all="ignore"):
        for a in range(0, P.size, CHUNK):
            c = slice(a, a + CHUNK)
            p, t, delta, factor = P[None, c], T[None, c], m["DeltaTSnow"][None, c], m["SnowFactor"][None, c]
            seas = SEASON[0] + m["SnowMeltCoef"][None, c]
            rn = ml = cover = 0.0
            for i in range(3):
                ts = t + delta * float(i - 1)
                snow_s = np.where(ts < m["TempSnow"], factor * p, 0.0)
                rain_s = np.where(ts >= m["TempSnow"], p, 0.0)
                melt_s = np.maximum((ts - m["TempMelt"]) * seas * (1 + 0.01 * rain_s) * m["DtDay"], 0.0)
                ice_s = np.maximum((t if i < 2 else ts) * m["IceMeltCoef"] * m["DtDay"] * SEASON[1], 0.0)
                melt_s = np.maximum(np.minimum(melt_s + ice_s, zones[:, i, c]), 0.0)
                zones[:, i, c] = zones[:, i, c] + snow_s - melt_s
                rn, ml, cover = rn + rain_s, ml + melt_s, cover + zones[:, i, c]
            rain[:, c], melt[:, c], cover = rn / 3, ml / 3, cover / 3
            e = np.exp(-0.04 * np.where(t < 0, 0.08, 0.5) * cover / m["SnowWaterEquivalent"])
            frost[:, c] = np.maximum(frost[:, c] + (-(1 - m["Afrost"]) * frost[:, c] - t * e) * m["DtDay"], 0.0)
            frozen[:, c] = frost[:, c] > m["FrostIndexThreshold"]


def window(prime, body, steps):
    prime()
    _lib.synchronize(0)
    t0 = time.perf_counter()
    for s in range(steps):
        body(s)
    _lib.synchronize(0)
    return (time.perf_counter() - t0) * 1e3 / steps


def alternate(legs, reps):
    ms = {k: [] for k, _ in legs}
    for rep in range(reps + 1):                             # the first round of all legs is the warm-up
        for name, fn in legs:
            t = fn()
            log("round %d %s %.2f ms" % (rep, name, t))
            if rep:
                ms[name].append(t)
    return {k: dict(ms_per_model_step=statistics.median(v), spread_ms=max(v) - min(v)) for k, v in ms.items()}


def kernel_alone(ens):
    """ms per lf_snow_frost_members_device on the rows of the set in use, with the forcing stride of the last step"""
    L, M, N = _lib.lib(), ens.members, ens.N
    one = ens._shared[ens._cur]["Precipitation"] and ens._shared[ens._cur]["Tavg"]
    call = lambda: _lib.check(L.lf_snow_frost_members_device(0, C.byref(ens.snow_frost), M, ens.stride, ens.pstride,
                                                             0 if one else ens.pstride))
    _lib.check(L.lf_side_stream_join(0))
    call()
    _lib.synchronize(0)
    _lib.timer_start(0)
    for _ in range(KERNEL_CALLS):
        call()
    ms = _lib.timer_stop(0) / KERNEL_CALLS
    slices = -(-M // 8)
    moved = N * (M * (32 + 57 + (8 if ens.meteo["Snow"] else 0)) + slices * 24 + (slices if one else M) * 16)
    return dict(ms=ms, forcing_rows="one" if one else "per member", bytes=moved, bytes_per_s=moved / (ms * 1e-3),
                fraction_of_copy_ceiling=moved / (ms * 1e-3) / COPY_CEILING)


def run(size, M, rank, reps, steps):
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(size, size, family="deep", block=1_000_000)
    N = int(mask.sum())
    rng = np.random.default_rng(M)
    meteo = dict(SCALARS, DeltaTSnow=rng.uniform(0.0, 4.0, N), SnowMeltCoef=rng.uniform(2.0, 6.0, N),
                 SnowFactor=rng.uniform(0.8, 1.2, N), SnowCoverS=rng.uniform(0.0, 50.0, (3, N)) * (rng.random((3, N)) < 0.6),
                 FrostIndex=rng.uniform(0.0, 100.0, N))
    P = [rng.uniform(0.0, 20.0, N) * (rng.random(N) < 0.6) for _ in range(2)]
    T = [rng.uniform(-15.0, 15.0, N) for _ in range(2)]
    land = [syn.hotpath_forcing(N, s) for s in range(2)]
    row = dict(size=size, pixels=N, members=M, rank=rank, steps_per_window=steps)
    # ---- without meteo= ---------------------------------------------------------------------------------------------------
    ens = HotPathEnsemble(values, sc, mask, ldd_to_chan, ldd_kin, M, split=True)
    log("%d^2, %d members: built without meteo=" % (size, M))
    shared = [ens.pinned_forcing(per_member=False) for _ in range(2)]
    for s in range(2):
        for k in shared[s]:
            shared[s][k][...] = land[s][k]
    pinned = {k: _lib.PinnedArray((M, N), np.float64) for k in ("Rain", "SnowMelt")}
    zones, frost = np.broadcast_to(meteo["SnowCoverS"], (M, 3, N)).copy(), np.broadcast_to(meteo["FrostIndex"], (M, N)).copy()
    frozen, numpy_ms = np.empty((M, N), bool), []
    for rep in range(3 if M <= 16 else 1):
        t0 = time.perf_counter()
        host_snow_frost(meteo, zones, frost, P[0], T[0], pinned["Rain"].a, pinned["SnowMelt"].a, frozen)
        numpy_ms.append((time.perf_counter() - t0) * 1e3)
    del zones, frost, frozen
    log("host snow and frost: %s ms" % numpy_ms)
    rows = dict(shared[0], Rain=pinned["Rain"].a, SnowMelt=pinned["SnowMelt"].a)

    def plain(e, sets, **kw):
        def body(s):
            e.step(sets[s % len(sets)], **kw)
            e.upload_wait()
            e.prefetch(sets[(s + 1) % len(sets)])
        return lambda: window(lambda: e.prefetch(sets[0]), body, steps)
    row.update(alternate([("shared", plain(ens, shared)), ("host_rows", plain(ens, [rows]))], reps))
    row["numpy_ms"] = dict(ms=statistics.median(numpy_ms), runs=len(numpy_ms))
    for p in pinned.values():
        p.free()
    ens.free()
    # ---- with meteo= ------------------------------------------------------------------------------------------------------
    ens = HotPathEnsemble(values, sc, mask, ldd_to_chan, ldd_kin, M, split=True, meteo=meteo)
    log("built with meteo=")
    sets = [ens.pinned_forcing(per_member=False) for _ in range(2)]
    for s in range(2):
        for k in sets[s]:
            sets[s][k][...] = P[s] if k == "Precipitation" else T[s] if k == "Tavg" else land[s][k]
    patterns = {k: AS.fourier_patterns(mask, rank, 40.0, rng) for k in ("Tavg", "Precipitation")}
    coeff = [{k: AS.ar1_coefficients(None, (M, rank), 0.3, rng) for k in patterns} for _ in range(2)]
    ens.forcing_perturbation("Tavg", patterns["Tavg"] * 3.0, multiplicative=False, lower=-np.inf)
    ens.forcing_perturbation("Precipitation", patterns["Precipitation"])

    def perturbed():
        def body(s):
            ens.step(sets[s % 2], season=SEASON)
            ens.upload_wait()
            ens.prefetch(sets[(s + 1) % 2], coefficients=coeff[(s + 1) % 2])
        return window(lambda: ens.prefetch(sets[0], coefficients=coeff[0]), body, steps)
    row.update(alternate([("meteo", plain(ens, sets, season=SEASON)), ("perturbed", perturbed)], reps))
    ens.step(sets[0], season=SEASON)
    row["alone"] = kernel_alone(ens)
    ens.step(sets[0], coefficients=coeff[0], season=SEASON)
    row["alone_forcing_rows"] = kernel_alone(ens)
    frozen = ens.download("isFrozenSoil")
    row["members_differ_in_frozen_soil"] = bool((frozen[0] != frozen[-1]).any())
    row["kernel_ms"] = row["alone"]["ms"]
    row["front_end_ms"] = row["meteo"]["ms_per_model_step"] - row["shared"]["ms_per_model_step"]
    row["explained"] = bool(row["front_end_ms"] <= row["kernel_ms"] + row["meteo"]["spread_ms"])
    row["link_bytes_per_step"] = dict(shared=5 * N * 8, host_rows=(3 + 2 * M) * N * 8, meteo=5 * N * 8,
                                      perturbed=5 * N * 8 + 2 * M * rank * 8)
    ens.free()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--members", default="4,16,51")
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4, help="model steps per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meteo_members.json"))
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
