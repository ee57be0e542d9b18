"""What a localised serial analysis costs: HotPathEnsemble.regress() -- every gauge in ONE pass over the state -- against the
route there was before it, one transform(W_j, taper=rho_j) per gauge, in one process:

    python tools/bench_members_regress.py [--size 2000] [--members 4,16,51] [--gauges 8,64] [--halfwidths 20,100] [--reps 5]
                                          [--out profiles/members_regress.json]

Inputs as tools/bench_members_transform.py: synthetic.hotpath_scenario (size x size), report=REPORT, every member forced by
its own scaling of synthetic.hotpath_forcing, three model steps before anything is timed; the full default state
(analysis_names()) with a scalar lower bound of 0 on every vector.  The gauges lie on seeded land pixels, their increments
are assimilation.serial_increments() of seeded priors.  Two paths, alternating in one loop after one untimed round, host
clock from a synchronised device to a synchronised device, median and spread (max - min) of `reps` repetitions:
    regress    ens.regress(increments, bounds=)
    gauge_by_gauge   for every gauge j, ens.transform(I + s_j A_j D_j^T, taper=rho_j, bounds=): the same analysis up to the order
               of the sums, G passes; the [N] taper maps are resident before the clock starts -- what it takes to make them
               on the host (assimilation.localisation) and to lay them out and upload them is timed once, apart
Alone, device stopwatch (lf_timer_start / lf_timer_stop) around 20 calls of lf_members_regress_device on the member rows of
one [N] vector, without bounds: bytes moved at most ((16 members + 16) per element: a column no gauge touches is not
stored) per second against the measured copy ceiling the other member kernels report against, 6.29 TB/s, and fp64
operations (7 per element and gauge for the distance test, 4 members + 40 per element and gauge in range, counted from the
coordinates) per second against the SPEC-SHEET fp64 vector rate -- 78.6 TFLOPS counted as fused multiply-adds, 39.3e12
unfused operations per second; nobody has measured that rate here.  The share of (wavefront, gauge) pairs the kernel's
wave-wide vote skips is counted on the host from the land rows' order (and the channel rows').  The two timed paths carry
the same two fractions over the whole state: bytes -- regress() with bounds reads and stores every column once, the other
route once per gauge plus its taper row -- and operations, 2 members^2 + 3 members per element and pass for transform().
"variants" says which kernels ran; "variants_tried" holds the measurements of variants that were not kept."""
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

REPORT = ("TaPixel", "ThetaAll", "LZAvInflow", "Theta1bPixel", "Sat1", "GwLossCUM")
COPY_CEILING = 6.29e12            # B/s, float4 copy (measured)
SPEC_FP64_UNFUSED = 39.3e12       # operations/s: the spec sheet's 78.6 TFLOPS are fused multiply-adds counted twice
KERNEL_CALLS = 20
# what runs at this commit; a variant that was measured and not kept is in the output's "variants_tried", which a new run
# carries over from the file it replaces (the build that could run it is gone)
VARIANTS = "column in registers up to 16 members (k_members_regress_reg), in LDS beyond (k_members_regress)"


def log(text):
    print("[members_regress] " + text, file=sys.stderr, flush=True)


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


def reach_census(order, inc, rows, cols):
    """from the coordinates, in the order of a row set (`order`: the pixel of every position): (element, gauge) pairs in
    range, elements some gauge reaches, and of the (wavefront of 64 consecutive elements, gauge) pairs the share with no
    lane in range"""
    x, y = rows[order], cols[order]
    n = x.size
    waves = (n + 63) // 64
    pairs, skipped, reached = 0, 0, np.zeros(n, bool)
    for j in range(inc.gauges):
        inside = (x - inc.gx[j]) ** 2 + (y - inc.gy[j]) ** 2 < inc.cut2[j]
        pairs += int(inside.sum())
        reached |= inside
        padded = np.zeros(waves * 64, bool)
        padded[:n] = inside
        skipped += int((~padded.reshape(waves, 64).any(axis=1)).sum())
    return dict(pairs_in_range=pairs, elements_reached=int(reached.sum()), wave_gauge_pairs=waves * inc.gauges,
                wave_gauge_pairs_skipped=skipped, share_skipped=skipped / (waves * inc.gauges))


def whole_state(ens, inc, sets, census, out):
    """bytes and fp64 operations of the two timed paths over every row set (the few lake and reservoir rows count as moved
    but not as computed on) -> their rates as fractions of the copy ceiling and of the spec-sheet fp64 rate, in place"""
    M, G = ens.members, inc.gauges
    elements = sum(n for n, _ in sets)
    ops = {"regress": 0, "gauge_by_gauge": G * elements * (2 * M * M + 3 * M)}
    for n, order in sets:
        if order in census:
            ops["regress"] += 7 * n * G + (4 * M + 40) * census[order]["pairs_in_range"]
    moved = {"regress": 16 * M * elements + 16 * elements,           # bounded: every column is read and stored
             "gauge_by_gauge": G * (16 * M * elements + 8 * elements)}
    for name in [k for k in out if k.split("_")[0] == "regress" and isinstance(out[k], dict)] + ["gauge_by_gauge"]:
        key = "gauge_by_gauge" if name == "gauge_by_gauge" else "regress"
        sec = out[name]["ms"] * 1e-3
        out[name].update(bytes=moved[key], fraction_of_copy_ceiling=moved[key] / sec / COPY_CEILING, operations=ops[key],
                         fraction_of_spec_sheet_fp64_unfused=ops[key] / sec / SPEC_FP64_UNFUSED)


def kernel_alone(ens, inc, name, census):
    """ms per lf_members_regress_device on the member rows of one [N] vector, the table and coordinates regress() left"""
    L, M = _lib.lib(), ens.members
    (base, n, stride, order, _), = ens._analysis_rows(name)
    cx, cy = (ens._pixel_rows(a, order).ptr for a in ens._regress_coords)
    call = lambda: _lib.check(L.lf_members_regress_device(0, base, M, stride, n, inc.gauges, cx, cy, ens._regress_table.ptr,
                                                          None, -np.inf, None, np.inf))
    _lib.check(L.lf_side_stream_join(0))
    call()
    _lib.synchronize(0)
    _lib.timer_start(0)
    for _ in range(KERNEL_CALLS):
        call()
    ms = _lib.timer_stop(0) / KERNEL_CALLS
    moved = 8 * M * n + 16 * n + 8 * M * census["elements_reached"]
    ops = 7 * n * inc.gauges + (4 * M + 40) * census["pairs_in_range"]
    return dict(ms=ms, elements=n, bytes=moved, bytes_per_s=moved / (ms * 1e-3), fraction_of_copy_ceiling=moved / (ms * 1e-3) / COPY_CEILING,
                operations=ops, operations_per_s=ops / (ms * 1e-3), fraction_of_spec_sheet_fp64_unfused=ops / (ms * 1e-3) / SPEC_FP64_UNFUSED)


def point(ens, G, halfwidth, reps, rows, cols, bounds, sets):
    M, N = ens.members, ens.N
    rng = np.random.default_rng(1000 * G + int(halfwidth))
    at = np.sort(rng.choice(N, G, replace=False))
    xy = np.stack([rows[at], cols[at]], axis=1)
    hx = rng.standard_normal((M, G)) + 5.0
    inc = AS.serial_increments(hx, hx.mean(axis=0) + 0.05, np.full(G, 0.5), xy, float(halfwidth))
    assert inc.gauges == G
    out = dict(gauges=G, halfwidth=halfwidth, table_bytes=int(inc.table.nbytes))
    census = dict(land=reach_census(ens.pixel_of_position, inc, rows, cols), channel=reach_census(ens.gpix, inc, rows, cols))
    out.update(census["land"])
    out["channel_rows"] = census["channel"]
    # the route of one transform() per gauge: its matrices, and its taper maps made, laid out and uploaded
    t0 = time.perf_counter()
    tapers = [AS.localisation(rows - inc.gx[j], cols - inc.gy[j], inc.halfwidth[j], inc.cut2[j]) for j in range(G)]
    out["taper_maps_make_ms"] = (time.perf_counter() - t0) * 1e3
    weights = [np.eye(M) + inc.scale[j] * np.outer(inc.anomalies[j], inc.increments[j]) for j in range(G)]
    _lib.synchronize(0)
    t0 = time.perf_counter()
    for tp in tapers:
        for order in ("land", "channel"):
            ens._pixel_rows(tp, order)
    _lib.synchronize(0)
    out["taper_maps_upload_ms"] = (time.perf_counter() - t0) * 1e3
    out["taper_maps_bytes"] = int(8 * G * (N + ens.Nk))

    def gauge_by_gauge():
        for j in range(G):
            ens.transform(weights[j], taper=tapers[j], bounds=bounds)

    out.update(measure(dict(regress=lambda: ens.regress(inc, bounds=bounds), gauge_by_gauge=gauge_by_gauge), reps))
    whole_state(ens, inc, sets, census, out)
    r, g = out["regress"], out["gauge_by_gauge"]
    out["regress_over_gauge_by_gauge"] = r["ms"] / g["ms"]
    out["regress_faster_beyond_the_spread"] = bool(r["ms"] + r["spread_ms"] < g["ms"] - g["spread_ms"])
    out["alone"] = kernel_alone(ens, inc, "LZ", out)
    for key in list(ens._analysis_cache):                   # the taper maps of this point make room for the next one's
        if any(key[0] == id(tp) for tp in tapers):
            _lib.synchronize(0)
            ens._analysis_cache.pop(key)[1].free()
    return out


def run(size, M, gauges, halfwidths, reps):
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(size, size, family="deep", block=1_000_000)
    N = int(mask.sum())
    ens = HotPathEnsemble(values, sc, mask, ldd_to_chan, ldd_kin, M, split=True, report=REPORT)
    ens._ROWS_CACHED = 4 * max(gauges) + 64                 # every taper map of a point stays resident, in both row orders
    log("%d^2, %d members: built" % (size, M))
    scale = (1.0 + 0.02 * np.arange(M, dtype=np.float32))[:, None]
    forcing = ens.pinned_forcing(np.float32)
    for k, a in syn.hotpath_forcing(N, 0).items():
        if k in FORCING:
            forcing[k][:] = np.asarray(a, np.float32)[None] * scale
    for s in range(3):
        ens.step(forcing)
    names = ens.analysis_names()
    bounds = {k: (0.0, None) for k in names}
    r, c = np.nonzero(mask)
    rows, cols = r.astype(np.float64), c.astype(np.float64)
    sets = [(n, order) for k in names for _, n, _, order, _ in ens._analysis_rows(k) if n]
    row = dict(size=size, pixels=N, channel_pixels=int(ens.Nk), members=M, vectors=len(names),
               row_sets=sum(len(ens._analysis_rows(k)) for k in names),
               state_bytes=sum(8 * M * n for k in names for _, n, _, _, _ in ens._analysis_rows(k)), points=[])
    for G in gauges:
        for c in halfwidths:
            row["points"].append(point(ens, G, c, reps, rows, cols, bounds, sets))
            log(json.dumps(row["points"][-1]))
    ens.free()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--members", default="4,16,51")
    ap.add_argument("--gauges", default="8,64")
    ap.add_argument("--halfwidths", default="20,100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--append", action="store_true", help="keep the member counts already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "members_regress.json"))
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("at least 3 repetitions")
    ints = lambda text: [int(x) for x in text.split(",") if x]
    doc = dict(device=_lib.device_name(0), reps=a.reps, copy_ceiling_bytes_per_s=COPY_CEILING,
               spec_sheet_fp64_unfused_operations_per_s=SPEC_FP64_UNFUSED, variants=VARIANTS, variants_tried=[], ensemble=[])
    if os.path.exists(a.out):
        old = json.load(open(a.out))
        doc["variants_tried"] = old.get("variants_tried", [])   # (measured with builds this commit no longer has: carried over)
        if a.append:
            doc["ensemble"] = old["ensemble"]
    for M in ints(a.members):
        doc["ensemble"].append(run(a.size, M, ints(a.gauges), ints(a.halfwidths), a.reps))
        with open(a.out, "w") as f:                         # (after every member count: the rows measured so far)
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
