"""The zonal sums of member rows (lf_members_zonal_device, lisflood-code_amd/csrc/lf_members.hip; the order:
lisflood_amd/zonal.py) restated in numpy.  It takes nothing from the library but the plan arrays it is handed -- pixels, the
run table of every pass -- and builds every pass from the rule of the run sum:

    the run's values v[0 .. len) are padded to 256 with +0.0;
    lane l of 64:  s = 0.0;  s = s + v[l];  s = s + v[l + 64];  s = s + v[l + 128];  s = s + v[l + 192];
    for d = 32, 16, 8, 4, 2, 1:  s[l] = s[l] + s[l + d]  for l < d;   the run sum is s[0].

The pass-1 value of an entry is x / divisor (skipped at divisor == 1.0), times the weight if there are weights, each
rounded on its own; the values of a later pass are the run sums of the pass before, in run order.  run_sum() is the rule one
float at a time, pass_sums() the same for every run and member at once (test_members_zonal_cpu.py holds one to the other)."""
import numpy as np

RUN, LANES = 256, 64


def run_sum(v):
    """the rule on one run, one float at a time"""
    v = [float(x) for x in v]
    assert len(v) <= RUN
    v = v + [0.0] * (RUN - len(v))
    with np.errstate(all="ignore"):
        s = []
        for l in range(LANES):
            t = np.float64(0.0)
            for k in range(RUN // LANES):
                t = t + np.float64(v[l + LANES * k])
            s.append(t)
        d = LANES // 2
        while d >= 1:
            for l in range(d):
                s[l] = s[l] + s[l + d]
            d //= 2
    return float(s[0])


def pass_sums(values, run_start):
    """values [M, E], run_start [runs + 1] -> [M, runs]: every run padded into its own row of 256, then the rule on columns"""
    values = np.asarray(values, np.float64)
    start = np.asarray(run_start, np.int64)
    M, runs = values.shape[0], start.size - 1
    length = np.diff(start)
    assert start[0] == 0 and start[-1] == values.shape[1] and (length >= 0).all() and (length <= RUN).all()
    run_of = np.repeat(np.arange(runs), length)
    slot = run_of * RUN + (np.arange(values.shape[1]) - start[run_of])
    padded = np.zeros((M, runs * RUN))                    # +0.0 everywhere; the entries overwrite their slots
    padded[:, slot] = values
    padded = padded.reshape(M, runs, RUN)
    with np.errstate(all="ignore"):
        s = np.zeros((M, runs, LANES))
        for k in range(RUN // LANES):
            s = s + padded[:, :, LANES * k:LANES * (k + 1)]
        d = LANES // 2
        while d >= 1:
            s[:, :, :d] = s[:, :, :d] + s[:, :, d:2 * d]
            d //= 2
    return np.ascontiguousarray(s[:, :, 0])


def terms(values, pixels, weights=None, divisor=1.0):
    """the pass-1 values [M, entries]: values [M, N] in pixel order at plan.pixels, divided, weighted"""
    with np.errstate(all="ignore"):
        t = np.asarray(values, np.float64)[:, np.asarray(pixels, np.int64)]
        if divisor != 1.0:
            t = t / np.float64(divisor)
        if weights is not None:
            t = t * np.asarray(weights, np.float64)[np.asarray(pixels, np.int64)]
    return t


def zonal_sums(values, pixels, run_starts, weights=None, divisor=1.0, passes=None):
    """[M, Z] (or, with passes=p, the [M, runs_p] run sums after p passes): every pass from the run tables"""
    v = terms(values, pixels, weights, divisor)
    for start in run_starts[:passes]:
        v = pass_sums(v, start)
    return v


def weight_sums(pixels, run_starts, weights=None):
    """[Z]: the same rule on the weights, or on 1.0 per entry"""
    ones = np.ones((1, np.asarray(pixels).size))
    w = ones if weights is None else terms(np.asarray(weights, np.float64)[None], pixels)
    for start in run_starts:
        w = pass_sums(w, start)
    return w[0]


def zonal_means(values, pixels, run_starts, weights=None, divisor=1.0):
    with np.errstate(all="ignore"):
        return zonal_sums(values, pixels, run_starts, weights, divisor) / weight_sums(pixels, run_starts, weights)
