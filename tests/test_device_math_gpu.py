"""-m gpu: the device math helpers (lf_math.h, their copies in lf_sweep.h / lf_fused.h, lf_soil_math.h) value by value.

The parity tests check whole module outputs on the values their inputs happen to hold; here every helper runs on its own
(tests/probes/lf_math_probe.hip, built with the product's CXXFLAGS) over a fixed set of edges -- the fast-range limits and
their neighbours, +-0, denormals, inf, NaN, negatives, results that overflow or underflow, roots next to the 1e-12 floor --
plus seeded log-uniform samples, against references computed in mpmath at 240 bits from the exact double inputs, against
the CPU oracle's own iteration, and against one another bit for bit where the code says "the same operations".

Not covered here: the copies of these formulas written inline in kernel bodies (the beta = 3/5 power and solve inside the
level loops of lf_sweep.h) cannot be called on their own; the bit-equality tests of the whole kernels cover them.
"""
import ctypes as C
import math
import os
import sys

import mpmath
import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "probes"))
import probe_build  # noqa: E402


pytestmark = pytest.mark.gpu

MP_PREC = 240
FAST_MIN, FAST_MAX = 1e-30, 1e30                  # LF_FAST_MIN / LF_FAST_MAX
NEWTON_TOL = 1e-12                                # LF_NEWTON_TOL
ROOT_FLOOR = float.fromhex("0x1.04e74cc73ee88p-8")  # LF_ROOT_FLOOR
DEN_MIN = 5e-324
DBL_MIN = 2.2250738585072014e-308
DEN_MAX = np.nextafter(DBL_MIN, 0.0)
DBL_MAX = np.finfo(np.float64).max
EPS = 2.0 ** -52
INF, NAN = math.inf, math.nan

# accuracy bounds asserted below and quoted in lf_math.h / DESIGN.md
POW_BETA_ULP = {0: 4.5, 1: 3.5}  # (measured 3.6 and 3.0) lf_pow_3_5 / lf_pow_5_3 in the fast range, against the exact x^(3/5) / x^(5/3)
SOLVE_ULP = 9.0           # (measured 7.5) lf_solve_3_5: Q against the exact root of r^5 + a r^3 = c, Q = r^5
POW_POS_REL = 7e-15       # lf_pow_pos, |y log2 x| <= 50 (measured 6.3e-15)
POW_POS_REL_WIDE = 1.3e-14  # lf_pow_pos, |y log2 x| > 50, normal results (measured 1.1e-14)


# ---- probe ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="session")
def probe(tmp_path_factory):
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    return probe_build.load(probe_build.build(str(tmp_path_factory.mktemp("lf_math_probe"))))


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def pow_beta(lib, fam, variant, x, slot=0):
    x = _f(x)
    out = np.empty_like(x)
    assert lib.probe_pow_beta(fam, variant, slot, x.size, _d(x), _d(out)) == 0
    return out


def solve(lib, variant, c, a, beta=0.6, slot=0):
    c, a = _f(c), _f(a)
    out = np.empty_like(c)
    assert lib.probe_solve(variant, slot, C.c_double(beta), c.size, _d(c), _d(a), _d(out)) == 0
    return out


def pow_pos(lib, variant, x, y, slot=0):
    x, y = _f(x), _f(y)
    out = np.empty_like(x)
    assert lib.probe_pow_pos(variant, slot, x.size, _d(x), _d(y), _d(out)) == 0
    return out


def unsat_k(lib, variant, s, slot=0):
    a = {k: _f(s[k]) for k in ("w", "wres", "ws", "ksat", "inv_m", "m")}
    pore = np.ascontiguousarray(s["pore"], dtype=np.uint8)
    out = np.empty_like(a["w"])
    assert lib.probe_unsat_k(variant, slot, out.size, _d(a["w"]), pore.ctypes.data_as(C.POINTER(C.c_ubyte)), _d(a["wres"]),
                             _d(a["ws"]), _d(a["ksat"]), _d(a["inv_m"]), _d(a["m"]), _d(out)) == 0
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_bits(got, want, what, inputs=()):
    bad = bits(got) != bits(want)
    if bad.any():
        i = np.flatnonzero(bad)[:5]
        ins = " ".join(f"{n}={np.asarray(v)[i].tolist()}" for n, v in inputs)
        raise AssertionError(f"{what}: {bad.sum()} of {bad.size} differ: got {got[i].tolist()} want {want[i].tolist()} {ins}")


def neighbours(v):
    return [np.nextafter(v, -INF), v, np.nextafter(v, INF)]


# ---- exact references -------------------------------------------------------------------------------------------------

def mp_split(v):
    """an mpf as hi + lo doubles (hi the nearest double; lo = 0 where hi overflows)"""
    h = float(v)
    return h, float(v - h) if math.isfinite(h) else 0.0


def mp_pow(x, y):
    """x^y for positive finite doubles, exact to MP_PREC bits, as (hi, lo)"""
    hi, lo = np.empty(len(x)), np.empty(len(x))
    with mpmath.workprec(MP_PREC):
        for i, (xv, yv) in enumerate(zip(x, y)):
            v = mpmath.power(mpmath.mpf(float(xv)), yv if isinstance(yv, mpmath.mpf) else mpmath.mpf(float(yv)))
            hi[i], lo[i] = mp_split(v)
    return hi, lo


def ulp_err(got, hi, lo):
    """|got - (hi + lo)| in units of the last place of hi (normal hi)"""
    return np.abs((got - hi) - lo) / np.spacing(np.abs(hi))


def rel_err(got, hi, lo):
    return np.abs((got - hi) - lo) / np.abs(hi)


def fast_range(x):
    return (x >= FAST_MIN) & (x <= FAST_MAX)


def assert_close_to_reference(got, want):
    """rtol 1e-9 / atol 1e-12, except at the reference's floor: its iteration clamps q to 1e-12 and reports a q that
    stays there as 0, so it reports 0 for roots up to 2e-12 (|closure error| <= 1e-12 at the clamp) and the
    same iteration with a last-place different pow can land on either side"""
    ok = np.abs(got - want) <= 1e-12 + 1e-9 * np.abs(want)
    ok |= ((got == 0) & (want <= 2e-12)) | ((want == 0) & (got <= 2e-12))
    assert ok.all(), (np.flatnonzero(~ok)[:5], got[~ok][:5], want[~ok][:5])


def log_uniform(rng, lo, hi, n):
    return 10.0 ** rng.uniform(math.log10(lo), math.log10(hi), n)


# ---- a. x^0.6 and x^(1/0.6) -------------------------------------------------------------------------------------------

def pow_beta_inputs():
    edges = [0.0, -0.0, DEN_MIN, DEN_MAX, DBL_MIN, 1e-300, *neighbours(FAST_MIN), *neighbours(FAST_MAX),
             *neighbours(1.0), 32.0, 243.0, 2.0 ** 50, 1e300, DBL_MAX, INF, -INF, NAN, -1.0, -1e-10, -32.0, -DEN_MIN, -INF]
    rng = np.random.default_rng(2026)
    x = np.concatenate([edges, log_uniform(rng, 1e-320, 1e308, 20000), log_uniform(rng, FAST_MIN, FAST_MAX, 10000)])
    return x


POW_BETA_COPIES = {
    0: [(0, 0)] + [(n, s) for n in (1, 2, 3, 4) for s in range(n)] + [(5, 0), (6, 0), (7, 0), (8, 0), (8, 1), (9, 0)],
    1: [(0, 0), (6, 0), (7, 0), (8, 0), (8, 1), (9, 0)],
}
POW_BETA_NAMES = {0: "lf_pow_3_5", 1: "lf_pow_5_3"}
VARIANT_NAMES = {1: "_n<1>", 2: "_n<2>", 3: "_n<3>", 4: "_n<4>", 5: "_hot", 6: "cone<true>", 7: "cone<false>",
                 8: "cone_two<true>", 9: "cone_two<false>"}


@pytest.mark.parametrize("fam", [0, 1])
def test_pow_beta_copies_agree_bit_for_bit(probe, fam):
    """Every copy of x^0.6 (lf_pow_3_5, _n<1..4> in every lane slot, _hot, cone_pow_3_5<true/false>,
    cone_pow_3_5_two<true/false> in both slots) and of x^(5/3) gives the bits of the first, NaN and the sign of zero
    included."""
    x = pow_beta_inputs()
    ref = pow_beta(probe, fam, 0, x)
    for v, s in POW_BETA_COPIES[fam][1:]:
        assert_same_bits(pow_beta(probe, fam, v, x, s), ref, f"{POW_BETA_NAMES[fam]}{VARIANT_NAMES[v]} slot {s}", [("x", x)])


@pytest.mark.parametrize("fam", [0, 1])
def test_pow_beta_accuracy_in_the_fast_range(probe, fam):
    """Inside [LF_FAST_MIN, LF_FAST_MAX]: within POW_BETA_ULP of the exact x^(3/5) (x^(5/3)).  Against numpy's x ** 0.6
    the exponent itself differs: 0.6 is 0.59999999999999997780 as a double (1 / 0.6 is 1.6666666666666667407), so numpy's
    value is off the exact x^(3/5) by |ln x| * 2.2e-17 relative (|ln x| * 7.4e-17 for 5/3) besides its own rounding
    (< 1 ulp); the test allows the bound + 1 ulp + |ln x| * 2.3e-17 (7.5e-17)."""
    x = pow_beta_inputs()
    x = x[(x >= FAST_MIN) & (x <= FAST_MAX)]
    got = pow_beta(probe, fam, 0, x)
    with mpmath.workprec(MP_PREC):
        e = mpmath.mpf(3) / 5 if fam == 0 else mpmath.mpf(5) / 3
        hi, lo = mp_pow(x, [e] * len(x))
    err = ulp_err(got, hi, lo)
    print(f"{POW_BETA_NAMES[fam]}: max {err.max():.3f} ulp over {x.size} values in the fast range")
    assert err.max() <= POW_BETA_ULP[fam], (err.max(), x[np.argmax(err)])
    npy = x ** (0.6 if fam == 0 else 1.0 / 0.6)
    slope = 2.3e-17 if fam == 0 else 7.5e-17
    rel = np.abs(got - npy) / npy
    allowed = (POW_BETA_ULP[fam] + 1.0) * EPS + np.abs(np.log(x)) * slope
    assert (rel <= allowed).all(), (x[rel > allowed][:5], rel[rel > allowed][:5])


@pytest.mark.parametrize("fam", [0, 1])
def test_pow_beta_outside_the_fast_range(probe, fam):
    """Beyond the fast range: OCML pow bit for bit (+-0 -> +0 without it), and numpy's special values: +-0, +-inf, NaN,
    negatives, overflow."""
    x = pow_beta_inputs()
    out = ~((x >= FAST_MIN) & (x <= FAST_MAX))
    x = x[out]
    got = pow_beta(probe, fam, 0, x)
    ocml = pow_beta(probe, fam, 10, x)
    nz = x != 0
    assert_same_bits(got[nz], ocml[nz], "OCML pow", [("x", x[nz])])
    assert_same_bits(got[~nz], np.zeros((~nz).sum()), "+-0 -> +0")
    with np.errstate(invalid="ignore", over="ignore"):
        npy = x ** (0.6 if fam == 0 else 1.0 / 0.6)
    special = (x == 0) | ~np.isfinite(x) | (x < 0) | np.isinf(npy)
    npy = npy[special]
    assert np.array_equal(np.isnan(got[special]), np.isnan(npy))
    ok = ~np.isnan(npy)
    assert_same_bits(got[special][ok], npy[ok], "numpy special values", [("x", x[special][ok])])


# ---- b. closure solve, beta = 3/5 -------------------------------------------------------------------------------------

def exact_roots(c, a):
    """root r of r^5 + a r^3 = c (c, a > 0) and Q = r^5 to MP_PREC bits: float64 Newton from the upper bound
    min(c^(1/5), (c/a)^(1/3)) (monotone), then Newton at MP_PREC bits until the step is below 2^-200 relative."""
    r = np.minimum(c ** 0.2, (c / a) ** (1.0 / 3.0))
    for _ in range(200):
        r2 = r * r
        r = r - (r2 * r2 * r + a * r2 * r - c) / (r2 * (5.0 * r2 + 3.0 * a))
    hi, lo = np.empty(c.size), np.empty(c.size)
    with mpmath.workprec(MP_PREC):
        tiny = mpmath.mpf(2) ** -200
        for i in range(c.size):
            cv, av, rv = mpmath.mpf(float(c[i])), mpmath.mpf(float(a[i])), mpmath.mpf(float(r[i]))
            for it in range(8):
                r2 = rv * rv
                step = (r2 * r2 * rv + av * r2 * rv - cv) / (r2 * (5 * r2 + 3 * av))
                rv -= step
                if abs(step) <= tiny * rv:
                    break
            else:
                raise AssertionError(f"no convergence at c={c[i]!r} a={a[i]!r}")
            hi[i], lo[i] = mp_split(rv ** 5)
    return hi, lo


def solve_inputs():
    lc, la = np.meshgrid(np.linspace(-12, 30, 211), np.linspace(-30, 30, 211), indexing="ij")
    c, a = [10.0 ** lc.ravel()], [10.0 ** la.ravel()]
    avals = np.array([1e-30, 1e-6, 0.1, 1.0, 3.7, 1e3, 1e12, 1e30])
    for cv in neighbours(NEWTON_TOL):                   # c = 1e-12 and its neighbours
        c.append(np.full(avals.size, cv))
        a.append(avals)
    # roots next to the floor: r = LF_ROOT_FLOOR +- a few ulp, c = r^5 + a r^3 rounded, so the exact Q = r^5 lies within a
    # few ulp of 1e-12 on either side
    with mpmath.workprec(MP_PREC):
        rs, as_ = [], []
        for k in range(-6, 7):
            r = ROOT_FLOOR + k * np.spacing(ROOT_FLOOR)
            for av in (1e-30, 1e-20, 1e-12, 1e-9, 1e-6):
                rs.append(float(mpmath.mpf(r) ** 5 + mpmath.mpf(av) * mpmath.mpf(r) ** 3))
                as_.append(av)
    c.append(np.array(rs))
    a.append(np.array(as_))
    return np.concatenate(c), np.concatenate(a)


def solve_out_of_range():
    bad = [0.0, -0.0, -1.0, 1e-31, 1e31, INF, -INF, NAN]
    good = [1e-6, 1.0, 1e3]
    c = [bv for bv in bad for _ in good] + [gv for _ in bad for gv in good]
    a = [gv for _ in bad for gv in good] + [bv for bv in bad for _ in good]
    return np.array(c), np.array(a)


def test_solve_3_5_copies_agree_bit_for_bit(probe):
    """lf_solve_3_5, lf_solve_3_5_pre (af, laf made on the device as the cone kernel makes them), solve_any(b35),
    cone_solve<true/false> and cone_solve_two<true/false> in both slots give the same bits; beyond the fast range (c or a
    0, negative, 1e-31, 1e31, inf, NaN) the forms that route give the bits of lf_solve_cell."""
    c, a = solve_inputs()
    ref = solve(probe, 2, c, a)
    inr = (c > NEWTON_TOL) & fast_range(c) & fast_range(a)    # where the callers call lf_solve_3_5 itself
    for v in (0, 1):
        assert_same_bits(solve(probe, v, c[inr], a[inr]), ref[inr], f"solve variant {v}", [("c", c[inr]), ("a", a[inr])])
    for v, s in ((3, 0), (4, 0), (5, 0), (5, 1), (6, 0)):
        assert_same_bits(solve(probe, v, c, a, slot=s), ref, f"solve variant {v} slot {s}", [("c", c), ("a", a)])
    co, ao = solve_out_of_range()
    cell = solve(probe, 7, co, ao)
    assert_same_bits(solve(probe, 8, co, ao), cell, "lf_solve_cell_cold")
    for v, s in ((2, 0), (3, 0), (4, 0), (5, 0), (5, 1), (6, 0)):
        assert_same_bits(solve(probe, v, co, ao, slot=s), cell, f"out of range, variant {v} slot {s}", [("c", co), ("a", ao)])


def test_solve_3_5_against_the_exact_root_and_the_floor(probe):
    """Q within SOLVE_ULP of the exact r^5 where Q is clear of the 1e-12 floor; Q == 0 exactly where c <= 1e-12 or the
    exact root's r^5 <= 1e-12 (within the bound of the floor, either 0 or a Q within the bound)."""
    c, a = solve_inputs()
    got = solve(probe, 2, c, a)
    assert (got[c <= NEWTON_TOL] == 0).all()
    m = (c > NEWTON_TOL) & fast_range(c) & fast_range(a)      # the quintic path (the rest: the reference's iteration)
    c, a, got = c[m], a[m], got[m]
    hi, lo = exact_roots(c, a)
    band = SOLVE_ULP * 2 * EPS * NEWTON_TOL
    below, above = hi + lo < NEWTON_TOL - band, hi + lo > NEWTON_TOL + band
    assert (got[below] == 0).all(), (c[below][got[below] != 0][:5], a[below][got[below] != 0][:5])
    err = ulp_err(got[above], hi[above], lo[above])
    print(f"lf_solve_3_5: max {err.max():.3f} ulp over {above.sum()} roots clear of the floor")
    assert err.max() <= SOLVE_ULP, (err.max(), c[above][np.argmax(err)], a[above][np.argmax(err)])
    near = ~below & ~above
    assert near.sum() >= 20, near.sum()     # the floor pairs of solve_inputs land here
    en = ulp_err(got[near], hi[near], lo[near])
    assert ((got[near] == 0) | (en <= SOLVE_ULP)).all()
    assert (got[near] > 0).any() and (got[near] == 0).any()


def test_solve_3_5_against_the_reference_iteration(probe, oracle):
    """The quintic solve against the reference's own Newton iteration (oracle, beta = 0.6, no upstream cells) at the
    suite's bars, rtol 1e-9 / atol 1e-12 (assert_close_to_reference: the reference's floor)."""
    c, a = solve_inputs()
    got = solve(probe, 2, c, a)
    want = np.zeros_like(c)
    oracle.sweep_positions(want, c, np.zeros(c.size + 1, np.int32), np.zeros(1, np.int32), a, 0.6 * a, 0.6, 0, c.size)
    assert_close_to_reference(got, want)


# ---- c. general solve -------------------------------------------------------------------------------------------------

def reference_stop(c, a, beta):
    """why solve1Pixel (kinematic_wave_parallel_tools.py:59-82) stops at (c, a): 'tol', 'prev' (q == previous) or 'maxit'"""
    ba, ib, bm1 = beta * a, 1 / beta, beta - 1
    t = ba * c ** bm1
    sec = c / (1 + t) if t <= 1 else c / (1 + t ** ib)
    q = (sec + ((c - sec) / a) ** ib) / 2
    err, prev, n = q + a * q ** beta - c, -1.0, 0
    while abs(err) > NEWTON_TOL and q != prev and n < 3000:
        prev = q
        q -= err / (1 + ba * q ** bm1)
        q = max(q, NEWTON_TOL)
        err = q + a * q ** beta - c
        n += 1
    return "tol" if abs(err) <= NEWTON_TOL else ("prev" if q == prev else "maxit")


# (beta, c, a) where the reference's loop ends on q == previous or on LF_MAX_ITERS (found with reference_stop)
GENERAL_STOPS = [(0.6, 1e-11, 0.01, "prev"), (0.6, 1e5, 1e4, "maxit"), (0.5, 1e-11, 1e-4, "prev"),
                 (0.5, 1e5, 1e8, "maxit"), (0.75, 1e-11, 0.01, "prev"), (0.75, 1e4, 1e10, "maxit"),
                 (0.9, 1e-10, 100.0, "prev"), (0.9, 1e5, 1e6, "maxit")]


@pytest.mark.parametrize("beta", [0.6, 0.5, 0.75, 0.9])
def test_general_solve_against_the_reference_iteration(probe, oracle, beta):
    """lf_solve_cell (and its out-of-line copy, bit for bit) against the oracle's iteration at rtol 1e-9 / atol 1e-12
    (assert_close_to_reference),
    including cases that stop on q == previous and on LF_MAX_ITERS."""
    lc, la = np.meshgrid(np.linspace(-12, 30, 43), np.linspace(-30, 30, 31), indexing="ij")
    stops = [(cv, av, why) for b, cv, av, why in GENERAL_STOPS if b == beta]
    for cv, av, why in stops:
        assert reference_stop(cv, av, beta) == why, (beta, cv, av, why)
    c = np.concatenate([10.0 ** lc.ravel(), [s[0] for s in stops], neighbours(NEWTON_TOL), [0.0, -1.0]])
    a = np.concatenate([10.0 ** la.ravel(), [s[1] for s in stops], [1.0, 1.0, 1.0], [1.0, 1.0]])
    got = solve(probe, 7, c, a, beta)
    assert_same_bits(solve(probe, 8, c, a, beta), got, "lf_solve_cell_cold")
    want = np.zeros_like(c)
    oracle.sweep_positions(want, c, np.zeros(c.size + 1, np.int32), np.zeros(1, np.int32), a, beta * a, beta, 0, c.size)
    assert_close_to_reference(got, want)


# ---- d. lf_pow_pos ----------------------------------------------------------------------------------------------------

def pow_pos_inputs():
    rng = np.random.default_rng(7)
    n = 6000
    xs = np.concatenate([log_uniform(rng, DEN_MIN, 1.0, n), rng.uniform(0.0, 1.0, n // 2), log_uniform(rng, 1.0, 1e300, n // 2)])
    kind = rng.integers(0, 3, xs.size)
    ys = np.where(kind == 0, rng.uniform(1.05, 50.0, xs.size),                  # GenuInvM
                  np.where(kind == 1, rng.uniform(0.02, 0.95, xs.size),         # GenuM
                           rng.choice([0.5, 1.5, 2.0, 3.7, 1e-6, 200.0], xs.size)))  # transmission, extremes
    xe = np.array([0.0, DEN_MIN, DEN_MAX, DBL_MIN, 1e-300, 0.5, *neighbours(1.0), 2.0, 1e300, DBL_MAX, INF, NAN, -0.0,
                   -1.0, -0.5])
    ye = np.array([1e-6, 0.02, 0.5, 1.05, 1.5, 2.0, 3.7, 50.0, 200.0, NAN])
    X, Y = np.meshgrid(xe, ye, indexing="ij")
    return np.concatenate([xs, X.ravel()]), np.concatenate([ys, Y.ravel()])


def test_pow_pos_lane_slots_agree_bit_for_bit(probe):
    """lf_pow_pos, lf_pow_pos_n<1, 2, 3> in every lane slot and powxy<true> give the same bits."""
    x, y = pow_pos_inputs()
    ref = pow_pos(probe, 0, x, y)
    for v, s in [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (4, 0)]:
        assert_same_bits(pow_pos(probe, v, x, y, s), ref, f"lf_pow_pos variant {v} slot {s}", [("x", x), ("y", y)])


def test_pow_pos_accuracy(probe):
    """Relative error <= POW_POS_REL where |y log2 x| <= 50, POW_POS_REL_WIDE beyond for normal results; results that
    overflow are inf; results that underflow are within one denormal ulp (2^-1074) of the exact value."""
    x, y = pow_pos_inputs()
    m = (x > 0) & np.isfinite(x) & ~np.isnan(y)
    x, y = x[m], y[m]
    got = pow_pos(probe, 0, x, y)
    with mpmath.workprec(MP_PREC):
        ex = [mpmath.power(mpmath.mpf(float(a)), mpmath.mpf(float(b))) for a, b in zip(x, y)]
        big = np.array([v > DBL_MAX for v in ex])
        small = np.array([v < DBL_MIN for v in ex])
        hi, lo = np.zeros(x.size), np.zeros(x.size)
        for i, v in enumerate(ex):
            if not big[i]:
                hi[i], lo[i] = mp_split(v)
        # underflow: |got - exact| in units of 2^-1074
        und = np.array([float(abs(mpmath.mpf(float(got[i])) - ex[i]) * mpmath.mpf(2) ** 1074) if small[i] else 0.0
                        for i in range(x.size)])
    normal = ~big & ~small & np.isfinite(hi)
    span = np.abs(y * np.log2(x))
    rel = rel_err(got[normal], hi[normal], lo[normal])
    narrow = span[normal] <= 50
    print(f"lf_pow_pos: max rel {rel[narrow].max():.3e} at |y log2 x| <= 50 ({narrow.sum()} values), "
          f"{rel[~narrow].max() if (~narrow).any() else 0:.3e} beyond ({(~narrow).sum()}), "
          f"{small.sum()} underflow (max {und.max():.2f} denormal ulp), {big.sum()} overflow")
    assert np.isposinf(got[big]).all(), (x[big][~np.isposinf(got[big])][:5], y[big][~np.isposinf(got[big])][:5])
    assert (und <= 1.0).all(), (und.max(), x[np.argmax(und)], y[np.argmax(und)])
    assert rel[narrow].max() <= POW_POS_REL, (rel[narrow].max(), x[normal][narrow][np.argmax(rel[narrow])],
                                              y[normal][narrow][np.argmax(rel[narrow])])
    assert rel[~narrow].max() <= POW_POS_REL_WIDE, (rel[~narrow].max(), x[normal][~narrow][np.argmax(rel[~narrow])],
                                                    y[normal][~narrow][np.argmax(rel[~narrow])])


def test_pow_pos_special_values(probe):
    """0 and NaN bases, a NaN exponent at x = 0: numpy's x ** y.  Negative bases give NaN, numpy's value for a finite base
    and a non-integer exponent.  Outside lf_pow_pos's domain (lf_math.h) and not compared with numpy: x = +inf and a NaN
    exponent at x = 1 (pow: +inf and 1, lf_pow_pos: NaN), -inf and negative bases with integer exponents.  No caller
    passes them: the soil bases are saturation degrees in [0, 1] with parameter exponents, and lf_pow_scalar_exponent sends
    +inf, NaN exponents and negative bases to OCML pow (test_pow_scalar_exponent)."""
    xe = [0.0, -0.0, 1.0, INF, NAN, -1.0, -0.5]
    ye = [1e-6, 0.02, 0.5, 1.05, 3.7, 50.0, 200.0, NAN]
    X, Y = np.meshgrid(xe, ye, indexing="ij")
    x, y = X.ravel(), Y.ravel()
    keep = ~((x < 0) & (np.floor(y) == y)) & ~(x == INF) & ~((x == 1.0) & np.isnan(y))
    x, y = x[keep], y[keep]
    got = pow_pos(probe, 0, x, y)
    with np.errstate(invalid="ignore"):
        want = np.float64(x) ** np.float64(y)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), list(zip(x[bad], y[bad], got[bad], want[bad]))
    z = want == 0
    assert (np.signbit(got[z]) == np.signbit(want[z])).all()


# ---- e. lf_pow_scalar_exponent ----------------------------------------------------------------------------------------

def test_pow_scalar_exponent(probe):
    """y = 2 is x * x and y = 0.5 the IEEE square root, bit for bit (numpy computes arr ** 2.0 and arr ** 0.5 as np.square
    and np.sqrt: asserted here too); negative bases keep pow's semantics (y = 2: x^2, y = 1.5: NaN); y = 0 and y >= 1e6
    take OCML pow, as does x = +inf; every other finite positive y gives the bits of lf_pow_pos."""
    rng = np.random.default_rng(3)
    x = np.concatenate([log_uniform(rng, 1e-300, 1e300, 4000), -log_uniform(rng, 1e-10, 1e3, 500),
                        [0.0, -0.0, 1.0, INF, NAN, -0.3, DEN_MIN, DBL_MAX]])
    assert_same_bits(x ** 2.0, np.square(x), "numpy x ** 2.0")
    assert_same_bits(x ** 0.5, np.sqrt(x), "numpy x ** 0.5")
    for yv in (2.0, 0.5, 1.5, 0.0, 1e6, 2e6, 3.7, 0.3, 1e-6, 200.0):
        y = np.full(x.size, yv)
        got = pow_pos(probe, 5, x, y)
        if yv == 2.0:
            assert_same_bits(got, x * x, "y = 2", [("x", x)])
        elif yv == 0.5:
            with np.errstate(invalid="ignore"):
                want = np.sqrt(x)
            assert np.array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            assert_same_bits(got[ok], want[ok], "y = 0.5", [("x", x[ok])])
        elif yv in (0.0, 1e6, 2e6):
            assert_same_bits(got, pow_pos(probe, 6, x, y), f"y = {yv}: OCML pow", [("x", x)])
        else:
            neg = (x < 0) | (x == INF)
            assert_same_bits(got[~neg], pow_pos(probe, 0, x[~neg], y[~neg]), f"y = {yv}: lf_pow_pos", [("x", x[~neg])])
            assert_same_bits(got[neg], pow_pos(probe, 6, x[neg], y[neg]), f"y = {yv}: negative or +inf x, OCML pow")
            assert (got[x == INF] == INF).all()
            if yv != math.floor(yv):
                assert np.isnan(got[neg & np.isfinite(x)]).all()
    xn = np.array([-0.3, -2.0, -1e-3])
    assert_same_bits(pow_pos(probe, 5, xn, np.full(3, 2.0)), xn * xn, "negative x, y = 2")


# ---- f. soil conductivity ---------------------------------------------------------------------------------------------

def soil_inputs():
    rng = np.random.default_rng(17)
    rows = []
    for den in 10.0 ** np.linspace(-3, 4, 15):
        for wres in (0.0, 0.7, 12.5, 333.0):
            ws = wres + den
            den_ = ws - wres
            w = np.concatenate([np.linspace(wres - den_, ws + den_, 13), neighbours(wres), neighbours(ws)])
            for wv in w:
                rows.append((wv, wres, ws))
    for wres in (0.0, 5.0, 47.3, 1e3):        # ws == wres: w above, at and below
        for wv in (wres + 1.0, np.nextafter(wres, INF), wres, np.nextafter(wres, -INF), wres - 1.0):
            rows.append((wv, wres, wres))
    w, wres, ws = np.array(rows).T
    n = w.size
    m = log_uniform(rng, 0.02, 0.95, n)
    s = dict(w=w, wres=wres, ws=ws, m=m, inv_m=1.0 / m, ksat=log_uniform(rng, 1.0, 1e3, n), pore=rng.random(n) < 0.9)
    s["ksat"][rng.random(n) < 0.05] = 0.0
    return s


def oracle_unsat_k(s):
    """numpy transcription of lf_oracle.c:384-396 (saturation_degree, unsat_k)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (s["w"] - s["wres"]) / (s["ws"] - s["wres"])
        mn = np.where(1.0 < q, 1.0, q)            # dmin(q, 1): (b < a) ? b : a
        sat = np.where(0.0 > mn, 0.0, mn)         # dmax(., 0)
        sat = np.where(s["pore"], sat, 0.0)
        t = 1.0 - (1.0 - sat ** s["inv_m"]) ** s["m"]
        return s["ksat"] * np.sqrt(sat) * (t * t)


@pytest.mark.parametrize("fast", [True, False])
def test_soil_conductivity_forms_agree_bit_for_bit(probe, fast):
    """The conductivity the sub-step loop computes after the first sub-step (unsat_k_r with soil_den_of, as layer_loop
    calls them) and the three-layer form unsat_k3 (every layer slot) give the bits of unsat_k, ws == wres included."""
    s = soil_inputs()
    ref = unsat_k(probe, 0 if fast else 1, s)
    inputs = [(k, s[k]) for k in ("w", "wres", "ws", "pore")]
    assert_same_bits(unsat_k(probe, 2 if fast else 3, s), ref, "sub-step loop (unsat_k_r)", inputs)
    for slot in range(3):
        assert_same_bits(unsat_k(probe, 4 if fast else 5, s, slot), ref, f"unsat_k3 layer {slot}", inputs)


def test_soil_conductivity_against_the_oracle(probe):
    """unsat_k<false> (OCML pow) and unsat_k<true> (lf_pow_pos) against a numpy transcription of the oracle within rtol
    1e-12, with the same NaN and zero pattern -- plus what a last-place difference of the inner powers (OCML against
    glibc: 2 ulp; lf_pow_pos: its POW_POS_REL) becomes through t = 1 - (1 - s^(1/m))^m: next to s = 1 (w one ulp below
    WS) 1 - s^(1/m) is a few ulp and its relative error is large, next to s = 0 t itself cancels."""
    s = soil_inputs()
    want = oracle_unsat_k(s)
    with np.errstate(all="ignore"):
        sat = np.where(s["pore"], np.clip((s["w"] - s["wres"]) / (s["ws"] - s["wres"]), 0.0, 1.0), 0.0)
        p1 = sat ** s["inv_m"]
        u = 1.0 - p1
        t = 1.0 - u ** s["m"]
    for v, d in ((1, 2 * EPS), (0, POW_POS_REL)):
        got = unsat_k(probe, v, s)
        assert np.array_equal(np.isnan(got), np.isnan(want)), v
        assert np.array_equal(got == 0, want == 0), (v, s["w"][(got == 0) != (want == 0)][:5])
        ok = ~np.isnan(want)
        with np.errstate(all="ignore"):
            du = d * p1 + EPS                                     # 1 - s^(1/m): the power's error and the rounding
            dum = np.where(u > 0, s["m"] * u ** (s["m"] - 1.0) * du, 0.0) + d * u ** s["m"]
            allowed = 1e-12 * np.abs(want) + s["ksat"] * np.sqrt(sat) * 2 * np.abs(t) * (dum + EPS) * 4
        dev = np.abs(got - want)
        bad = np.flatnonzero(ok & ~(dev <= allowed))[:5]
        print(f"unsat_k variant {v}: max |dk| / allowed {np.max(dev[ok] / np.where(allowed[ok] > 0, allowed[ok], 1)):.3f}")
        assert not bad.size, (v, {k: np.asarray(s[k])[bad].tolist() for k in ("w", "wres", "ws", "m")},
                              got[bad].tolist(), want[bad].tolist())
    assert np.isnan(want).any() and (want == 0).any()
