"""Member rows perturbed from low-rank patterns (lf_members_perturb_device, lf_upload_perturb_rows,
lisflood-code_amd/csrc/lf_members.hip) restated in numpy, with the inputs the tests of both share.

The restatement is the header's lines, one ufunc per operation (numpy never fuses a multiply and an add): the sum over r in
ascending order, the base, the mode, the two bounds.  The loop runs over r; its operands are whole [members, n] arrays,
column-of-members c[:, r] against row P[r], so every (m, i) sees exactly the sequence of the header.

Comparisons are on the uint64 view with every NaN as one pattern (members_transform.canonical): the sign and payload of a
NaN that an operation made are the device's own."""
import numpy as np

from members_transform import SENTINEL, bits, bound_high, bound_low, bound_of, canonical, layout, make_rows, same  # noqa: F401

BASE_FORMS = ("shared", "alias", "absent")   # base_dev: a row of its own, rows_dev itself (member 0's row), NULL (in place)
# planted in base, rows and patterns: both zeros, both infinities, a NaN, the smallest subnormal, a subnormal, huge values
PLANTS = (-0.0, 0.0, np.inf, -np.inf, np.nan, 5e-324, -2.5e-310, 1e300, -1e300)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def perturb(rows, coeff, patterns, base=None, multiplicative=False, lower=-np.inf, upper=np.inf):
    """rows [members, n] as they were before the call (not read where base is given: None will do), coeff [members, rank],
    patterns [rank, n], base None or [n], lower / upper a scalar or [n] -> the rows after the call"""
    c, P = np.asarray(coeff, np.float64), np.asarray(patterns, np.float64)
    with np.errstate(all="ignore"):
        s = np.multiply(c[:, 0][:, None], P[0][None, :])
        for r in range(1, P.shape[0]):
            s = np.add(s, np.multiply(c[:, r][:, None], P[r][None, :]))
        b = np.asarray(rows, np.float64) if base is None else np.broadcast_to(np.asarray(base, np.float64), s.shape)
        v = np.multiply(b, np.add(1.0, s)) if multiplicative else np.add(b, s)
        return bound_high(bound_low(v, lower), upper)


def perturb_by_element(rows, coeff, patterns, base=None, multiplicative=False, lower=-np.inf, upper=np.inf):
    """the same lines once more, one Python float at a time (what the restatement itself is held to)"""
    M, rank = np.shape(coeff)
    n = np.shape(patterns)[1]
    out = np.empty((M, n))
    at = lambda b, i: np.float64(b) if np.ndim(b) == 0 else np.float64(b[i])
    with np.errstate(all="ignore"):
        for i in range(n):
            for m in range(M):
                s = np.float64(coeff[m][0]) * np.float64(patterns[0][i])
                for r in range(1, rank):
                    s = s + np.float64(coeff[m][r]) * np.float64(patterns[r][i])
                b = np.float64(base[i]) if base is not None else np.float64(rows[m][i])
                v = b * (np.float64(1.0) + s) if multiplicative else b + s
                lo, hi = at(lower, i), at(upper, i)
                v = lo if (lo > v or (lo != lo and v == v)) else v
                v = hi if (hi < v or (hi != hi and v == v)) else v
                out[m, i] = v
    return out


def census(rows, coeff, patterns, base=None, multiplicative=False, lower=-np.inf, upper=np.inf):
    """how many (member, element) pairs take each side of each bound comparison, and the NaN-bound branch:
    {"total", "lower_takes" (lo > v), "lower_nan" (lo is a NaN and v is none), "lower_passes", and the same for upper}"""
    unbounded = perturb(rows, coeff, patterns, base, multiplicative)
    lo = np.broadcast_to(np.float64(lower) if np.ndim(lower) == 0 else lower, unbounded.shape)
    with np.errstate(all="ignore"):
        takes, nan = lo > unbounded, (lo != lo) & (unbounded == unbounded)
        out = {"total": unbounded.size, "lower_takes": int(takes.sum()), "lower_nan": int(nan.sum()),
               "lower_passes": int((~takes & ~nan).sum())}
        v = bound_low(unbounded, lower)
        hi = np.broadcast_to(np.float64(upper) if np.ndim(upper) == 0 else upper, v.shape)
        takes, nan = hi < v, (hi != hi) & (v == v)
        out.update(upper_takes=int(takes.sum()), upper_nan=int(nan.sum()), upper_passes=int((~takes & ~nan).sum()))
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def make_base(n, seed):
    """[n]: seeded values with PLANTS from the last element backwards (as far as n reaches)"""
    b = np.random.default_rng(seed).standard_normal(n) * 10.0
    for j, value in enumerate(PLANTS):
        if j < n:
            b[n - 1 - j] = value
    return b


def make_patterns(rank, n, seed):
    """[rank, n]: smooth-field sized values (|P| about 0.5) with PLANTS in the middle of the rows, in row j % rank"""
    P = np.random.default_rng(seed).standard_normal((rank, n)) * 0.5
    for j, value in enumerate(PLANTS):
        if j < n:
            P[j % rank, (n // 2 + j) % n] = value
    return P


def make_coefficients(members, rank, seed):
    """[members, rank]: values about 0.5 with a +0.0 and a -0.0 planted and, from three members on, member 2 all zero (what a
    zero coefficient does to an infinite pattern value, and to the sign of a zero)"""
    c = np.random.default_rng(seed).standard_normal((members, rank)) * 0.5
    c[0, 0] = 0.0
    c[members - 1, rank - 1] = -0.0
    if members >= 3:
        c[2] = 0.0
    return c


def base_of(form, x, n, seed):
    """base form -> (what the restatement takes as base, the row to upload or None)"""
    if form == "shared":
        b = make_base(n, seed)
        return b, b
    if form == "alias":
        return x[0].copy(), None
    return None, None
