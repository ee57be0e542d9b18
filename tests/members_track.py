"""The streaming update of an ensemble's run-long accumulators (lf_members_track_device, lisflood-code_amd/csrc/lf_members.hip)
restated in plain numpy, word for word as include/lisflood_amd.h defines it, and the inputs the tests feed both with.

The value of (m, i) is v = rows[m * stride + i] / divisor.  An accumulator that is not asked for does not exist.
first:      peak = v, peak_step = step, sum = v, first_above[t] = step if v > thr[t] else -1, steps_above[t] = 1 if v > thr[t] else 0
otherwise:  take = v > peak or (v is a NaN and peak is none);  peak = v if take else peak;  peak_step = step if take else peak_step
            sum = sum + v
            a = v > thr[t] (false with a NaN on either side);  first_above[t] = step if a and steps_above[t] == 0 else first_above[t]
            (without steps_above: if a and first_above[t] < 0);  steps_above[t] += a"""
import numpy as np

import members_products as MP

F64_SENTINEL, I32_SENTINEL = -7.0, -7          # preset in every accumulator: what lies between the rows must still hold it
KEYS = ("peak", "peak_step", "sum", "first_above", "steps_above")
STEPS = (0, 3, 4, 9)                           # the step numbers of the four updates: the caller's, no counter
# column -> the case planted there along the time axis, in every member (census() names the ones that are there)
PLANTS = ("all_equal", "rise_to_a_tie", "minus_zero_first", "plus_zero_first", "plus_inf_middle", "minus_inf_last", "nan_first",
          "nan_middle", "nan_last", "nan_only", "at_threshold", "ulp_above", "ulp_below", "nan_threshold", "above_first_only",
          "above_last_only", "never_above")
THRESHOLD_PLANTS = PLANTS[10:]
COLUMN = {name: k for k, name in enumerate(PLANTS)}


def planted_in(n, n_thresholds):
    """the cases a series of n columns holds"""
    return {p for p in PLANTS if COLUMN[p] < n and (n_thresholds > 0 or p not in THRESHOLD_PLANTS)}


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def make_series(n, members, steps, seed, n_thresholds=0):
    """-> (raw [steps, members, n], thresholds [n_thresholds, n]): seeded values -- a third of the columns small integers, so
    that steps tie -- with the cases of PLANTS in columns 0 .. 16 along the time axis, for every member (as far as n
    reaches).  The threshold cases are completed by plant_thresholds(), on the values after the division."""
    assert steps >= 4
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((steps, members, n)) * 10.0
    ties = rng.random(n) < 1 / 3
    raw[:, :, ties] = rng.integers(-3, 4, (steps, members, int(ties.sum()))).astype(np.float64)
    mid, last = steps // 2, steps - 1

    def put(name, values):
        """values: one per step, or a scalar"""
        k = COLUMN[name]
        if k < n:
            raw[:, :, k] = np.broadcast_to(np.asarray(values, np.float64), (steps,))[:, None]

    series = lambda rest, **at: [at.get("s%d" % s, rest) for s in range(steps)]
    put("all_equal", 3.25)
    put("rise_to_a_tie", series(1.0, s0=5.0, **{"s%d" % last: 5.0}))
    put("minus_zero_first", series(0.0, s0=-0.0))
    put("plus_zero_first", series(-0.0, s0=0.0))
    for name, s, value in (("plus_inf_middle", mid, np.inf), ("minus_inf_last", last, -np.inf), ("nan_first", 0, np.nan),
                           ("nan_middle", mid, np.nan), ("nan_last", last, -np.nan)):
        k = COLUMN[name]
        if k < n:
            raw[s, :, k] = value
    put("nan_only", series(np.nan, s0=-np.nan))
    for name in ("at_threshold", "ulp_above", "ulp_below"):      # one value at every step: the threshold goes at / beside it
        put(name, 1.7 + COLUMN[name])
    put("above_first_only", series(-5.0, s0=5.0))                # (their threshold is 0.0)
    put("above_last_only", series(-5.0, **{"s%d" % last: 5.0}))
    put("never_above", -5.0)
    thresholds = rng.standard_normal((n_thresholds, n)) * 5.0
    return raw, thresholds


def plant_thresholds(x, thresholds):
    """the threshold cases on x = raw / divisor ([steps, members, n]), in place, in every threshold row"""
    n = x.shape[2]
    for name, value in (("at_threshold", lambda v: v), ("ulp_above", lambda v: np.nextafter(v, -np.inf)),
                        ("ulp_below", lambda v: np.nextafter(v, np.inf)), ("nan_threshold", lambda v: np.nan),
                        ("above_first_only", lambda v: 0.0), ("above_last_only", lambda v: 0.0), ("never_above", lambda v: 0.0)):
        k = COLUMN[name]
        if k < n:
            thresholds[:, k] = value(x[0, 0, k])
    return thresholds


def values_of(raw, divisor):
    """x[s, m, i] = raw[s, m, i] / divisor, an IEEE division (divisor 1: the element itself)"""
    return raw / np.float64(divisor)


def census(x, thresholds):
    """which of PLANTS the values (after the division, [steps, members, n]) and the thresholds ([T, n]) hold in their column"""
    S, _, n = x.shape
    mid, last = S // 2, S - 1
    col = lambda name: x[:, :, COLUMN[name]]
    nan, neg = np.isnan(x), np.signbit(x)
    ncol = lambda name: nan[:, :, COLUMN[name]]
    checks = {
        "all_equal": lambda c: (c == c[0]).all() and (c != 0).all(),
        "rise_to_a_tie": lambda c: (c[0] == c[last]).all() and (c[1:last] < c[0]).all(),
        "minus_zero_first": lambda c: (c == 0).all() and neg[0, :, 2].all() and not neg[1:, :, 2].any(),
        "plus_zero_first": lambda c: (c == 0).all() and not neg[0, :, 3].any() and neg[1:, :, 3].all(),
        "plus_inf_middle": lambda c: (c[mid] == np.inf).all() and np.isfinite(np.delete(c, mid, 0)).all(),
        "minus_inf_last": lambda c: (c[last] == -np.inf).all() and np.isfinite(c[:last]).all(),
        "nan_first": lambda c: ncol("nan_first")[0].all() and not ncol("nan_first")[1:].any(),
        "nan_middle": lambda c: ncol("nan_middle")[mid].all() and ncol("nan_middle").sum(0).max() == 1,
        "nan_last": lambda c: ncol("nan_last")[last].all() and not ncol("nan_last")[:last].any(),
        "nan_only": lambda c: ncol("nan_only").all(),
    }
    found = {name for name, check in checks.items() if COLUMN[name] < n and check(col(name))}
    if thresholds is not None and thresholds.shape[0]:
        with np.errstate(invalid="ignore"):
            for name, check in (("at_threshold", lambda c, t: (c == t).all()),
                                ("ulp_above", lambda c, t: (c == np.nextafter(t, np.inf)).all()),
                                ("ulp_below", lambda c, t: (c == np.nextafter(t, -np.inf)).all()),
                                ("nan_threshold", lambda c, t: np.isnan(t).all()),
                                ("above_first_only", lambda c, t: (c[0] > t).all() and not (c[1:] > t).any()),
                                ("above_last_only", lambda c, t: (c[last] > t).all() and not (c[:last] > t).any()),
                                ("never_above", lambda c, t: not (c > t).any())):
                k = COLUMN[name]
                if k < n and check(x[:, :, k], thresholds[:, None, None, k] if name != "nan_threshold" else thresholds[:, k]):
                    found.add(name)
    return found


# ---- the restatement --------------------------------------------------------------------------------------------------------
def fresh(members, n, n_thresholds, keys=KEYS, f64=F64_SENTINEL, i32=I32_SENTINEL):
    """the accumulators asked for, holding what a `first` update must not read"""
    shape = {"peak": (members, n), "sum": (members, n), "peak_step": (members, n),
             "first_above": (n_thresholds, members, n), "steps_above": (n_thresholds, members, n)}
    return {k: (np.full(shape[k], f64, np.float64) if k in ("peak", "sum") else np.full(shape[k], i32, np.int32))
            for k in keys if n_thresholds or k not in ("first_above", "steps_above")}


def update(acc, v, thresholds, step, first):
    """one call: v [members, n] folded into the accumulators of `acc` in place"""
    assert step >= 0
    T = thresholds.shape[0]
    with np.errstate(invalid="ignore"):
        if first:
            if "peak" in acc:
                acc["peak"][:] = v
            if "peak_step" in acc:
                acc["peak_step"][:] = step
            if "sum" in acc:
                acc["sum"][:] = v
            for t in range(T):
                if "first_above" in acc:
                    acc["first_above"][t] = np.where(v > thresholds[t], step, -1)
                if "steps_above" in acc:
                    acc["steps_above"][t] = np.where(v > thresholds[t], 1, 0)
            return acc
        if "peak" in acc:
            peak = acc["peak"]
            take = (v > peak) | ((v != v) & (peak == peak))
            acc["peak"] = np.where(take, v, peak)
            if "peak_step" in acc:
                acc["peak_step"] = np.where(take, np.int32(step), acc["peak_step"])
        if "sum" in acc:
            acc["sum"] = acc["sum"] + v
        for t in range(T):
            a = v > thresholds[t]
            if "first_above" in acc:
                before = acc["steps_above"][t] == 0 if "steps_above" in acc else acc["first_above"][t] < 0
                acc["first_above"][t] = np.where(a & before, np.int32(step), acc["first_above"][t])
            if "steps_above" in acc:
                acc["steps_above"][t] = acc["steps_above"][t] + a
    return acc


def fold(x, thresholds, steps=None, keys=KEYS):
    """every update of x [S, members, n] in turn -> the accumulators after the last one"""
    S, members, n = x.shape
    steps = range(S) if steps is None else steps
    acc = fresh(members, n, thresholds.shape[0], keys)
    for s in range(S):
        update(acc, x[s], thresholds, steps[s], s == 0)
    return acc


def layout(rows, stride, sentinel):
    """[..., n] -> flat [rows * stride] with the sentinel in every element between n and the stride"""
    flat = rows.reshape(-1, rows.shape[-1])
    out = np.full((flat.shape[0], stride), sentinel, rows.dtype)
    out[:, :flat.shape[1]] = flat
    return out.reshape(-1)


def same(a, b):
    """the same bits (int32), or the same bits with NaN equal to NaN (float64)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return bool(np.array_equal(a, b) if a.dtype == np.int32 else MP.same_bits_at(a, b).all())
