"""No GPU: the host side of the perturbation of member rows from low-rank patterns -- lf_members_perturb_device and
lf_upload_perturb_rows are in the header, the library and the ctypes table; every refusal comes back as LF_E_INVALID with the
argument named before a device is touched (there is none here); the restatement the GPU tests compare with
(members_perturb.py) is held to the header's lines evaluated one float at a time, its inputs take every branch of the bound
lines, the consequences the header states hold; and the host helpers fourier_patterns / ar1_coefficients of
lisflood_amd.assimilation."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import members_perturb as MP
from lisflood_amd import _lib
from lisflood_amd import assimilation as AS

HEADER = os.path.join(ROOT, "include", "lisflood_amd.h")
SIGNATURE = "ipiqqpipqpipdpd"
EXPORTS = ("lf_members_perturb_device", "lf_upload_perturb_rows")
N = 600
FAKE = C.c_void_p(64)              # a pointer that is never dereferenced: every call here ends before a device is touched


def last_error():
    return _lib.lib().lf_last_error()


@pytest.mark.parametrize("name", EXPORTS)
def test_the_export_is_in_the_header_the_library_and_the_table(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    table = {"lf_" + n: sig for sig, names in _lib._SIGNATURES.items() for n in names.split()}
    f = getattr(_lib.lib(), name)
    assert re.search(r"\bint\s+%s\s*\(" % name, text)
    assert re.search(r"\sT\s+%s$" % name, dynamic, flags=re.M)
    assert table[name] == SIGNATURE
    assert list(f.argtypes) == [_lib._KIND[k] for k in SIGNATURE] and f.restype is C.c_int


def test_the_header_holds_the_definition_and_its_consequences():
    text = " ".join(open(HEADER).read().replace("\n *", " ").split())
    for line in ("s = c[m][0] * P[0][i]; for r = 1 .. rank-1: s = s + c[m][r] * P[r][i]",
                 "b = base_dev ? base_dev[i] : rows_dev[m*stride + i]",
                 "v = multiplicative ? b * (1.0 + s) : b + s",
                 "lo = lower_dev ? lower_dev[i] : lower; v = (lo > v || (lo != lo && v == v)) ? lo : v",
                 "hi = upper_dev ? upper_dev[i] : upper; v = (hi < v || (hi != hi && v == v)) ? hi : v",
                 "rows_dev[m*stride + i] = v",
                 "has read b before its first store, so the in-place form is safe",
                 "leave every non-NaN bit of b, -0.0 included", "-0.0 + (+0.0) is +0.0", "0 * inf in a pattern gives NaN"):
        assert line in text, line
    transform = text[text.index("lf_members_transform_device: with x[k]"):]        # the bound lines are transform's own
    for line in ("lo = lower_dev ? lower_dev[i] : lower; v = (lo > v || (lo != lo && v == v)) ? lo : v",
                 "hi = upper_dev ? upper_dev[i] : upper; v = (hi < v || (hi != hi && v == v)) ? hi : v"):
        assert line in transform[:transform.index("lf_members_resample_device")]


def call(name, **kw):
    a = dict(rows=FAKE, members=3, stride=N + 5, n=N, base=None, rank=4, patterns=FAKE, pattern_stride=N + 3,
             coeff=np.zeros((3, 4)), multiplicative=0, lower_dev=None, lower=-np.inf, upper_dev=None, upper=np.inf)
    a.update(kw)
    return getattr(_lib.lib(), name)(0, a["rows"], a["members"], a["stride"], a["n"], a["base"], a["rank"], a["patterns"],
                                     a["pattern_stride"], _lib.ptr(a["coeff"]), a["multiplicative"], a["lower_dev"], a["lower"],
                                     a["upper_dev"], a["upper"])


REFUSED = {                        # arguments, the word of the message
    "rows_null": (dict(rows=None), b"rows_dev"),
    "patterns_null": (dict(patterns=None), b"patterns_dev"),
    "coeff_null": (dict(coeff=None), b"coeff_host"),
    "members_0": (dict(members=0), b"members"),
    "members_negative": (dict(members=-2), b"members"),
    "members_129": (dict(members=129), b"at most 128 members"),
    "rank_0": (dict(rank=0), b"rank"),
    "rank_17": (dict(rank=17), b"rank"),
    "n_negative": (dict(n=-1, stride=0, pattern_stride=0), b"n = -1"),
    "n_beyond_a_launch": (dict(n=2 ** 31, stride=2 ** 31, pattern_stride=2 ** 31), b"n = 2147483648"),
    "stride_short": (dict(stride=N - 1), b"stride"),
    "pattern_stride_short": (dict(pattern_stride=N - 1), b"pattern_stride"),
    "multiplicative_2": (dict(multiplicative=2), b"multiplicative"),
    "multiplicative_negative": (dict(multiplicative=-1), b"multiplicative"),
    "lower_above_upper": (dict(lower=2.0, upper=1.0), b"lower = 2 is greater than upper = 1"),
    "lower_above_upper_at_n_0": (dict(n=0, stride=0, lower=2.0, upper=1.0), b"lower"),
}


@pytest.mark.parametrize("name", EXPORTS)
@pytest.mark.parametrize("case", list(REFUSED))
def test_refused_before_a_device_is_touched(case, name):
    kw, word = REFUSED[case]
    assert call(name, **kw) == _lib.LF_E_INVALID, case
    assert word in last_error(), (case, last_error())
    if case == "stride_short":                                    # (not the message of pattern_stride)
        assert b"pattern_stride" not in last_error()


def test_what_needs_no_device_is_ok_without_one():
    """n == 0 is LF_OK and launches nothing; with it the limits themselves pass the checks -- 128 members, rank 16; bounds the
    wrong way round are refused only where both are scalars"""
    name = "lf_members_perturb_device"
    assert call(name, n=0, stride=0, pattern_stride=0) == _lib.LF_OK
    assert call(name, n=0, members=128, rank=16, coeff=np.zeros((128, 16)), multiplicative=1) == _lib.LF_OK
    assert call(name, n=0, lower=2.0, upper=1.0, lower_dev=FAKE) == _lib.LF_OK
    assert call(name, n=0, lower=2.0, upper=1.0, upper_dev=FAKE) == _lib.LF_OK
    assert call(name, n=0, lower=np.nan, upper=1.0) == _lib.LF_OK
    assert call(name, n=0, base=FAKE) == _lib.LF_OK


# ---- the restatement ---------------------------------------------------------------------------------------------------------
FAMILIES = list(itertools.product((False, True), MP.BASE_FORMS, ("scalar", "row"), ("scalar", "row")))


def family_inputs(family, members=5, rank=3, n=41):
    multiplicative, form, lower, upper = family
    x = MP.make_rows(n, members, 11)
    base, _ = MP.base_of(form, x, n, 13)
    lo, hi = MP.bound_of(lower, n, 7, True)[0], MP.bound_of(upper, n, 8, False)[0]
    if upper == "row":
        hi = np.roll(hi, 1)                                       # (its NaN beside the lower row's, not on it)
    return x, MP.make_coefficients(members, rank, 3), MP.make_patterns(rank, n, 5), base, multiplicative, lo, hi


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: "-".join(str(k) for k in f))
def test_the_restatement_is_the_header_one_float_at_a_time(family):
    args = family_inputs(family)
    got, want = MP.perturb(*args), MP.perturb_by_element(*args)
    assert MP.same(got, want), np.argwhere(MP.canonical(got) != MP.canonical(want))[:4]
    assert np.isnan(got).any() and np.isfinite(got).any()
    if args[3] is not None:                                       # with a base the rows themselves are not read
        assert MP.same(MP.perturb(None, *args[1:]), got)


@pytest.mark.parametrize("rank", [1, 2, 16])
def test_the_restatement_at_the_ranks_edges(rank):
    x, c, P = MP.make_rows(23, 4, 1), MP.make_coefficients(4, rank, 2), MP.make_patterns(rank, 23, 3)
    for multiplicative in (False, True):
        assert MP.same(MP.perturb(x, c, P, None, multiplicative), MP.perturb_by_element(x, c, P, None, multiplicative))


def test_the_planted_values_are_there():
    b, P, c = MP.make_base(37, 5), MP.make_patterns(3, 37, 5), MP.make_coefficients(5, 3, 5)
    for j, value in enumerate(MP.PLANTS):
        assert MP.bits(b[36 - j]) == MP.bits(np.float64(value)), j
        assert MP.bits(P[j % 3, 18 + j]) == MP.bits(np.float64(value)), j
    assert MP.bits(c[0, 0]) == MP.bits(np.float64(0.0)) and MP.bits(c[4, 2]) == MP.bits(np.float64(-0.0)) and not c[2].any()
    assert np.count_nonzero(c) == 15 - 5
    x = MP.make_rows(37, 5, 11)
    assert np.isnan(x).any() and np.isinf(x).any() and np.signbit(x[0, 0]) and x[0, 0] == 0


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: "-".join(str(k) for k in f))
def test_every_branch_of_the_bound_lines_is_taken_and_none_by_all(family):
    """per case family: lo > v true and false, hi < v true and false; with a bound row also the NaN-bound branch (a scalar
    bound is a number in these families: its NaN branch is empty by construction)"""
    count = MP.census(*family_inputs(family))
    total = count["total"]
    assert total == 5 * 41
    for side, kind in (("lower", family[2]), ("upper", family[3])):
        taken = [count[side + "_takes"], count[side + "_passes"]] + ([count[side + "_nan"]] if kind == "row" else [])
        assert all(0 < k < total for k in taken), (family, side, count)
        assert sum(taken) == total and (kind == "row" or count[side + "_nan"] == 0), (family, side, count)


def test_zero_coefficients_under_multiplicative_keep_every_non_nan_bit():
    x, b = MP.make_rows(41, 5, 11), MP.make_base(41, 13)
    P = np.random.default_rng(2).standard_normal((3, 41))                     # finite patterns: 0 * P is a zero
    zero = np.zeros((5, 3))
    zero[1], zero[3, 1] = -0.0, -0.0                                           # (zeros of either sign)
    for rows, base, before in ((x, None, x), (None, b, np.broadcast_to(b, x.shape))):
        got = MP.perturb(rows, zero, P, base, True)
        keep = ~np.isnan(before)
        assert np.array_equal(MP.bits(got)[keep], MP.bits(before)[keep]) and np.isnan(got[~keep]).all()
        assert (np.signbit(got) & (got == 0)).any() and np.isinf(got).any()    # -0.0 and the infinities among them
    # ... and an infinite pattern value is not switched off by a zero coefficient: 0 * inf is a NaN
    got = MP.perturb(x, zero, MP.make_patterns(3, 41, 5), None, True)
    planted = [(41 // 2 + j) % 41 for j, value in enumerate(MP.PLANTS) if np.isinf(value)]
    assert np.isnan(got[:, planted]).all() and len(planted) == 2


def test_additive_mode_loses_the_sign_of_a_zero():
    x = MP.make_rows(41, 5, 11)
    P = np.abs(np.random.default_rng(2).standard_normal((3, 41))) + 0.1      # (positive: every product is +0.0)
    got = MP.perturb(x, np.zeros((5, 3)), P, None, False)
    assert np.signbit(x[0, 0]) and x[0, 0] == 0 and got[0, 0] == 0 and not np.signbit(got[0, 0])    # -0.0 + (+0.0) = +0.0
    other = np.ones(x.shape, bool)
    other[0, 0] = other[0, 9] = False                              # (column 9: member 0's other -0.0 of make_rows)
    other &= ~np.isnan(x)
    assert np.array_equal(MP.bits(got)[other], MP.bits(x)[other])


# ---- the host helpers --------------------------------------------------------------------------------------------------------
MASK = np.random.default_rng(4).random((19, 23)) < 0.8


@pytest.mark.parametrize("rank", [1, 5, 16])
def test_fourier_patterns(rank):
    P = AS.fourier_patterns(MASK, rank, 6.0, np.random.default_rng(8))
    assert P.shape == (rank, int(MASK.sum())) and P.dtype == np.float64
    assert (np.abs(P) <= np.sqrt(2.0 / rank)).all() and np.abs(P).max() > 0.5 * np.sqrt(2.0 / rank)
    assert np.array_equal(P, AS.fourier_patterns(MASK, rank, 6.0, np.random.default_rng(8)))
    assert not np.array_equal(P, AS.fourier_patterns(MASK, rank, 6.0, np.random.default_rng(9)))
    # the definition, pixel by pixel, from the same draws in the same order
    rng = np.random.default_rng(8)
    w, phi = rng.standard_normal((rank, 2)) / 6.0, rng.uniform(0.0, 2.0 * np.pi, rank)
    rows, cols = np.nonzero(MASK)
    for r, i in ((0, 0), (rank - 1, 7), (rank // 2, len(rows) - 1)):
        want = np.sqrt(2.0 / rank) * np.cos(w[r, 0] * rows[i] + w[r, 1] * cols[i] + phi[r])
        assert abs(P[r, i] - want) < 1e-12


def test_fourier_patterns_make_a_smooth_field_of_about_unit_variance():
    """c @ P with iid N(0, 1) coefficients: variance 1 over members at every pixel (exactly 2 / rank sum cos^2 in
    expectation over c; over many patterns draws it averages 1), neighbours correlated, far pixels not"""
    mask = np.ones((40, 40), bool)
    rng = np.random.default_rng(0)
    P = AS.fourier_patterns(mask, 16, 5.0, rng)
    assert abs((P * P).sum(axis=0).mean() - 1.0) < 0.15            # E over phase of 2 cos^2 is 1; 16 features, 1600 pixels
    cov = P.T @ P                                                  # the field's covariance given the patterns
    near, far = cov[0, 1], cov[0, 39 * 40 + 39]
    assert near > 0.8 * cov[0, 0] and abs(far) < 0.5


def test_fourier_patterns_refuse_bad_arguments():
    rng = np.random.default_rng(1)
    for args, word in (((MASK.astype(np.uint8), 3, 5.0), "boolean"), ((MASK.ravel(), 3, 5.0), "boolean"),
                       ((MASK, 0, 5.0), "rank"), ((MASK, 17, 5.0), "rank"), ((MASK, 2.5, 5.0), "rank"),
                       ((MASK, 3, 0.0), "length_scale"), ((MASK, 3, -1.0), "length_scale"), ((MASK, 3, np.nan), "length_scale")):
        with pytest.raises(ValueError, match=word):
            AS.fourier_patterns(*args, rng)


def test_ar1_coefficients():
    first = AS.ar1_coefficients(None, (7, 4), 0.5, np.random.default_rng(3))
    assert first.shape == (7, 4) and first.dtype == np.float64
    assert np.array_equal(first, 0.5 * np.random.default_rng(3).standard_normal((7, 4)))
    nxt = AS.ar1_coefficients(first, 0.9, 0.5, np.random.default_rng(4))
    assert nxt.shape == (7, 4)
    assert np.array_equal(nxt, AS.ar1_coefficients(first, 0.9, 0.5, np.random.default_rng(4)))
    noise = np.random.default_rng(4).standard_normal((7, 4))
    assert np.allclose(nxt, 0.9 * first + np.sqrt(1 - 0.81) * 0.5 * noise, rtol=1e-14, atol=0)
    # rho = 1: previous bit for bit, the sign of a zero included; the generator moves on all the same
    previous = first.copy()
    previous[0, 0], previous[1, 1] = -0.0, 0.0
    rng = np.random.default_rng(5)
    kept = AS.ar1_coefficients(previous, 1.0, 0.5, rng)
    assert kept is not previous and np.array_equal(MP.bits(kept), MP.bits(previous))
    moved = np.random.default_rng(5)
    moved.standard_normal((7, 4))
    assert rng.standard_normal() == moved.standard_normal()
    # rho = 0: white noise of standard deviation sigma, per pattern where sigma is [rank]
    sigma = np.array([0.0, 1.0, 2.0, 3.0])
    white = AS.ar1_coefficients(first, 0.0, sigma, np.random.default_rng(6))
    assert np.array_equal(white, sigma * np.random.default_rng(6).standard_normal((7, 4))) and not white[:, 0].any()
    # the stationary spread is sigma
    c, rng = AS.ar1_coefficients(None, (2000, 2), 0.3, np.random.default_rng(7)), np.random.default_rng(8)
    for _ in range(20):
        c = AS.ar1_coefficients(c, 0.8, 0.3, rng)
    assert abs(c.std() - 0.3) < 0.02


def test_ar1_coefficients_refuse_bad_arguments():
    rng, previous = np.random.default_rng(1), np.zeros((3, 2))
    for args, word in (((None, 0.5, 1.0), "first draw"), ((None, (3, 0), 1.0), "first draw"), ((None, (3, 2, 1), 1.0), "first draw"),
                       ((np.zeros(3), 0.5, 1.0), "previous must be"), ((previous, 1.5, 1.0), "rho"), ((previous, -1.1, 1.0), "rho"),
                       ((previous, np.nan, 1.0), "rho"), ((previous, 0.5, -1.0), "sigma"), ((previous, 0.5, np.inf), "sigma"),
                       ((previous, 0.5, np.ones(3)), "broadcast"), ((None, (3, 2), np.ones(3)), "broadcast")):
        with pytest.raises(ValueError, match=word):
            AS.ar1_coefficients(*args, rng)
