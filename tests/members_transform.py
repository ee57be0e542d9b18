"""The analysis step of an ensemble on its member rows (lf_members_transform_device, lf_members_resample_device,
lisflood-code_amd/csrc/lf_members.hip) restated in numpy, with the inputs and weight matrices the tests of both share.

The restatement is the header's lines: for output member m the sum over k in ascending order, one multiply and one add
each (numpy never fuses them), then the taper, then the two bounds.  The loop runs over k; its operands are whole rows,
x[k] against column-of-members W[k], so every (m, i) sees exactly the sequence of the header.

Comparisons are on the uint64 view.  What a NaN carries beside being one -- its sign and payload -- is not laid down by
IEEE 754 for the result of an operation (0 * inf is a NaN of either sign, a NaN operand comes back with one operand's payload
or the other's), and the host's vector units and the device differ there; canonical() maps every NaN to one pattern first.
The resample is a copy: its comparison is on the raw bits, payloads included."""
import numpy as np

SENTINEL = -777.25                     # between the rows; must keep its bits
NAN_PAYLOAD = np.array([0x7FF800000000BEEF], np.uint64).view(np.float64)[0]    # a NaN a copy must carry over as it is
# planted in column j (as far as n reaches) at member j % members
PLANTS = (-0.0, np.inf, -np.inf, np.nan, 5e-324, -2.5e-310, 1e300, -1e300, NAN_PAYLOAD)
MINUS_ZERO_KEPT = len(PLANTS)          # column: -0.0 in member 0, every other member negative -- the identity keeps the sign
ALL_ZERO = len(PLANTS) + 1             # column: +0.0 in every member
TAPER_PLANTS = (0.0, 1.0, 0.5, np.nan)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def canonical(a):
    """the uint64 view with every NaN as one pattern"""
    a = np.ascontiguousarray(a, np.float64)
    out = a.view(np.uint64).copy()
    out[np.isnan(a)] = 0x7FF8000000000000
    return out


def same(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(canonical(a), canonical(b))


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def bound_low(v, lo):
    lo = np.broadcast_to(np.float64(lo) if np.ndim(lo) == 0 else lo, v.shape)
    return np.where((lo > v) | ((lo != lo) & (v == v)), lo, v)


def bound_high(v, hi):
    hi = np.broadcast_to(np.float64(hi) if np.ndim(hi) == 0 else hi, v.shape)
    return np.where((hi < v) | ((hi != hi) & (v == v)), hi, v)


def transform(x, W, taper=None, lower=-np.inf, upper=np.inf):
    """x [members, n] as it was before the call, W [members, members], taper None or [n], lower / upper a scalar or [n]
    -> the rows after the call"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    M = x.shape[0]
    with np.errstate(all="ignore"):
        t = x[0][None, :] * W[0][:, None]                     # t[m, i] = x[0, i] * W[0][m]
        for k in range(1, M):
            t = t + x[k][None, :] * W[k][:, None]
        v = t if taper is None else x + np.asarray(taper, np.float64)[None, :] * (t - x)
        return bound_high(bound_low(v, lower), upper)


def resample(x, parents):
    return np.asarray(x)[np.asarray(parents)].copy()


def transform_by_element(x, W, taper=None, lower=-np.inf, upper=np.inf):
    """the same lines once more, one Python float at a time (what the restatement itself is held to)"""
    M, n = x.shape
    out = np.empty((M, n))
    at = lambda b, i: float(b) if np.ndim(b) == 0 else float(b[i])
    with np.errstate(all="ignore"):
        for i in range(n):
            col = [np.float64(x[k, i]) for k in range(M)]
            for m in range(M):
                t = col[0] * np.float64(W[0, m])
                for k in range(1, M):
                    t = t + col[k] * np.float64(W[k, m])
                v = t if taper is None else col[m] + np.float64(taper[i]) * (t - col[m])
                lo, hi = np.float64(at(lower, i)), np.float64(at(upper, i))
                v = lo if (lo > v or (lo != lo and v == v)) else v
                v = hi if (hi < v or (hi != hi and v == v)) else v
                out[m, i] = v
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def make_rows(n, members, seed):
    """[members, n]: seeded values with PLANTS in columns 0 .. (as far as n reaches), then the two zero columns"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((members, n)) * 10.0
    for j, value in enumerate(PLANTS):
        if j < n:
            x[j % members, j] = value
    if members > 1:                    # (the -0.0 of column 0 has a positive neighbour: the identity matrix loses its sign)
        x[1, 0] = np.abs(x[1, 0]) + 1.0
    if MINUS_ZERO_KEPT < n:
        x[:, MINUS_ZERO_KEPT] = -np.abs(x[:, MINUS_ZERO_KEPT]) - 1.0
        x[0, MINUS_ZERO_KEPT] = -0.0
    if ALL_ZERO < n:
        x[:, ALL_ZERO] = 0.0
    return x


def make_taper(n, seed):
    """[n] in [0, 1) with 0, 1, 0.5 and a NaN planted from the last element backwards"""
    t = np.random.default_rng(seed).uniform(0.0, 1.0, n)
    for j, value in reversed(list(enumerate(TAPER_PLANTS))):
        t[(n - 1 - j) % n] = value
    return t


def make_bound_row(n, seed, lower):
    """[n]: a bound that bites on about half of the elements, with a NaN, the bound's own infinity and a zero planted"""
    b = np.random.default_rng(seed).uniform(-8.0, 2.0, n) if lower else np.random.default_rng(seed).uniform(-2.0, 8.0, n)
    for j, value in enumerate((np.nan, -np.inf if lower else np.inf, -0.0 if lower else 0.0)):
        b[(3 * j + 2) % n] = value
    return b


def bound_of(kind, n, seed, lower):
    """kind "absent" / "scalar" / "row" -> (what the restatement takes, the row for the device or None, the scalar)"""
    if kind == "absent":
        inf = -np.inf if lower else np.inf
        return inf, None, inf
    if kind == "scalar":
        s = -1.5 if lower else 4.0
        return s, None, s
    row = make_bound_row(n, seed, lower)
    return row, row, 0.0


def identity(members):
    return np.eye(members)


def selection(members, parents):
    """W with x_new[m] = x[parents[m]] up to what 0 * x adds"""
    W = np.zeros((members, members))
    W[np.asarray(parents), np.arange(members)] = 1.0
    return W


def affine(members, seed):
    """random, every column summing to 1 (to rounding): an update that keeps a constant column constant"""
    W = np.random.default_rng(seed).standard_normal((members, members)) * 0.3
    return W + (1.0 - W.sum(axis=0)) / members


def with_nan(members, seed):
    W = affine(members, seed)
    W[members // 2, 0] = np.nan
    return W


def cycle(members):
    """[1, 2, ..., members - 1, 0]"""
    return ((np.arange(members) + 1) % members).astype(np.int32)


MATRICES = ("identity", "selection", "affine", "with_nan")


def matrix(kind, members, seed=0):
    return {"identity": lambda: identity(members), "selection": lambda: selection(members, cycle(members)),
            "affine": lambda: affine(members, seed), "with_nan": lambda: with_nan(members, seed)}[kind]()


def layout(rows, stride):
    """[R, n] -> flat [(R - 1) * stride + n ... R * stride] image with the sentinel between the rows"""
    out = np.full((rows.shape[0], stride), SENTINEL)
    out[:, :rows.shape[1]] = rows
    return out.reshape(-1)
