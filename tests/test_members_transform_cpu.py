"""No GPU: the host side of the analysis step of an ensemble -- lf_members_transform_device and lf_members_resample_device
are in the header, the library and the ctypes table; every refusal comes back as LF_E_INVALID with the argument named before
a device is touched (there is none here); the restatement the GPU tests compare with (members_transform.py) is held to the
same lines evaluated one float at a time; the identity and a selection matrix change exactly what the header says they
may; and the host helpers of lisflood_amd.assimilation against hand-worked and textbook cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import members_transform as MX
from lisflood_amd import _lib
from lisflood_amd import assimilation as AS

HEADER = os.path.join(ROOT, "include", "lisflood_amd.h")
EXPORTS = {"lf_members_transform_device": "ipiqqpppdpd", "lf_members_resample_device": "ipiqqp"}
N = 600
FAKE = C.c_void_p(64)              # a pointer that is never dereferenced: every call here ends before a device is touched


def last_error():
    return _lib.lib().lf_last_error()


@pytest.mark.parametrize("name", list(EXPORTS))
def test_the_export_is_in_the_header_the_library_and_the_table(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    table = {"lf_" + n: sig for sig, names in _lib._SIGNATURES.items() for n in names.split()}
    f = getattr(_lib.lib(), name)
    assert re.search(r"\bint\s+%s\s*\(" % name, text)
    assert re.search(r"\sT\s+%s$" % name, dynamic, flags=re.M)
    assert table[name] == EXPORTS[name]
    assert list(f.argtypes) == [_lib._KIND[k] for k in EXPORTS[name]] and f.restype is C.c_int


def test_the_header_says_that_a_selection_matrix_is_no_resample():
    text = " ".join(open(HEADER).read().replace("\n *", " ").split())
    assert "The identity matrix is NOT a bit-exact no-op" in text
    assert "A selection matrix is therefore no substitute for lf_members_resample_device" in text


def transform(**kw):
    a = dict(rows=FAKE, members=3, stride=N + 5, n=N, weights=FAKE, taper=FAKE, lower_dev=None, lower=-np.inf, upper_dev=None,
             upper=np.inf)
    a.update(kw)
    return _lib.lib().lf_members_transform_device(0, a["rows"], a["members"], a["stride"], a["n"], a["weights"], a["taper"],
                                                  a["lower_dev"], a["lower"], a["upper_dev"], a["upper"])


def resample(**kw):
    a = dict(rows=FAKE, members=3, stride=N + 5, n=N, parents=(1, 2, 0))
    a.update(kw)
    parents = None if a["parents"] is None else np.asarray(a["parents"], np.int32)
    return _lib.lib().lf_members_resample_device(0, a["rows"], a["members"], a["stride"], a["n"], _lib.ptr(parents))


TRANSFORM_REFUSED = {              # arguments, the word of the message
    "rows_null": (dict(rows=None), b"rows_dev"),
    "weights_null": (dict(weights=None), b"weights_dev"),
    "members_0": (dict(members=0), b"members"),
    "members_negative": (dict(members=-2), b"members"),
    "members_65": (dict(members=65), b"at most 64 members"),
    "stride_short": (dict(stride=N - 1), b"stride"),
    "n_negative": (dict(n=-1, stride=0), b"n = -1"),
    "lower_above_upper": (dict(lower=2.0, upper=1.0), b"lower = 2 is greater than upper = 1"),
    "lower_above_upper_at_n_0": (dict(n=0, stride=0, lower=2.0, upper=1.0), b"lower"),
}
RESAMPLE_REFUSED = {
    "rows_null": (dict(rows=None), b"rows_dev"),
    "parents_null": (dict(parents=None), b"parents_host"),
    "members_0": (dict(members=0, parents=()), b"members"),
    "members_129": (dict(members=129, parents=tuple(range(129))), b"at most 128 members"),
    "stride_short": (dict(stride=N - 1), b"stride"),
    "n_negative": (dict(n=-1, stride=0), b"n = -1"),
    "parent_negative": (dict(parents=(0, -1, 2)), b"parents_host[1]"),
    "parent_is_members": (dict(parents=(0, 1, 3)), b"parents_host[2]"),
}


@pytest.mark.parametrize("case", list(TRANSFORM_REFUSED))
def test_transform_refuses_before_a_device_is_touched(case):
    kw, word = TRANSFORM_REFUSED[case]
    assert transform(**kw) == _lib.LF_E_INVALID, case
    assert word in last_error(), (case, last_error())


@pytest.mark.parametrize("case", list(RESAMPLE_REFUSED))
def test_resample_refuses_before_a_device_is_touched(case):
    kw, word = RESAMPLE_REFUSED[case]
    assert resample(**kw) == _lib.LF_E_INVALID, case
    assert word in last_error(), (case, last_error())


def test_what_needs_no_device_is_ok_without_one():
    """n == 0 is LF_OK; so is the identity, which launches nothing -- and with it the limits themselves pass the checks:
    128 members, one member with a stride below n; bounds the wrong way round are refused only where both are scalars"""
    assert transform(n=0, stride=0) == _lib.LF_OK
    assert transform(n=0, stride=0, members=64, taper=None, lower=0.0, upper=0.0) == _lib.LF_OK
    assert transform(n=0, stride=0, lower=2.0, upper=1.0, lower_dev=FAKE) == _lib.LF_OK
    assert transform(n=0, stride=0, lower=2.0, upper=1.0, upper_dev=FAKE) == _lib.LF_OK
    assert transform(n=0, stride=0, lower=np.nan, upper=1.0) == _lib.LF_OK
    assert resample(n=0, stride=0) == _lib.LF_OK
    assert resample(parents=(0, 1, 2)) == _lib.LF_OK
    assert resample(members=128, parents=tuple(range(128)), stride=N) == _lib.LF_OK
    assert resample(members=1, parents=(0,), stride=0) == _lib.LF_OK


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MX.MATRICES)
@pytest.mark.parametrize("taper,lower,upper", [(False, "absent", "absent"), (True, "scalar", "row"), (True, "row", "scalar"),
                                               (False, "row", "row"), (True, "absent", "absent")])
def test_the_restatement_is_the_header_one_float_at_a_time(kind, taper, lower, upper):
    M, n = 5, 37
    x, W = MX.make_rows(n, M, 11), MX.matrix(kind, M, 3)
    tp = MX.make_taper(n, 5) if taper else None
    lo, hi = MX.bound_of(lower, n, 7, True)[0], MX.bound_of(upper, n, 8, False)[0]
    got, want = MX.transform(x, W, tp, lo, hi), MX.transform_by_element(x, W, tp, lo, hi)
    assert MX.same(got, want), np.argwhere(MX.canonical(got) != MX.canonical(want))[:4]
    assert np.isnan(got).any() and np.isfinite(got).any()


def test_the_planted_values_are_there():
    x = MX.make_rows(37, 5, 11)
    for j, value in enumerate(MX.PLANTS):
        assert MX.bits(x[j % 5, j]) == MX.bits(np.float64(value)), j
    assert np.signbit(x[:, MX.MINUS_ZERO_KEPT]).all() and x[0, MX.MINUS_ZERO_KEPT] == 0
    assert not np.signbit(x[:, MX.ALL_ZERO]).any() and (x[:, MX.ALL_ZERO] == 0).all()
    tp = MX.make_taper(37, 5)
    assert [tp[36 - j] for j in range(3)] == [0.0, 1.0, 0.5] and np.isnan(tp[33]) and np.isnan(tp).sum() == 1
    assert MX.make_taper(1, 5)[0] == 0.0 and MX.make_taper(2, 5).tolist() == [1.0, 0.0]
    W = MX.affine(7, 3)
    assert np.abs(W.sum(axis=0) - 1.0).max() < 1e-15 and np.isnan(MX.with_nan(7, 3)).sum() == 1
    assert np.array_equal(MX.selection(4, MX.cycle(4)), np.roll(np.eye(4), 1, axis=0))


def may_differ(x, parents):
    """where x_new[m] = sum_k x[k] S[k][m] with S the selection matrix of `parents` differs from x[parents[m]], by the header:
    a -0.0 unless every OTHER member of its column has the sign bit set, and every element whose column holds an inf or a
    NaN in another member (it becomes a NaN; an element that was a NaN stays one)"""
    M, n = x.shape
    out = np.zeros((M, n), bool)
    for m in range(M):
        p = parents[m]
        others = np.delete(x, p, axis=0)
        poisoned = (~np.isfinite(others)).any(axis=0)
        minus_zero = (x[p] == 0) & np.signbit(x[p])
        out[m] = (poisoned & ~np.isnan(x[p])) | (~poisoned & minus_zero & ~np.signbit(others).all(axis=0))
    return out


@pytest.mark.parametrize("members,n", [(5, 37), (2, 12), (1, 20)])
def test_identity_and_selection_change_what_the_header_says_and_nothing_else(members, n):
    x = MX.make_rows(n, members, 21)
    for parents in (np.arange(members), MX.cycle(members)):
        got, copy = MX.transform(x, MX.selection(members, parents)), MX.resample(x, parents)
        differs = MX.canonical(got) != MX.canonical(copy)
        assert np.array_equal(differs, may_differ(x, parents)), (members, n, parents)
        if members == 1:
            assert not differs.any() and np.array_equal(MX.bits(got), MX.bits(x))      # one member: every bit stays
        else:
            assert differs.any() and not differs.all()
    if members == 5:                   # the column whose other members are all negative keeps its -0.0; the others lose it
        got = MX.transform(x, MX.identity(5))
        assert np.signbit(got[0, MX.MINUS_ZERO_KEPT]) and x[0, 0] == 0 and np.signbit(x[0, 0]) and not np.signbit(got[0, 0])


def test_resample_of_the_restatement_is_a_copy_of_the_bits():
    x = MX.make_rows(37, 5, 2)
    got = MX.resample(x, [2, 0, 3, 4, 4])
    assert np.array_equal(MX.bits(got), MX.bits(x[[2, 0, 3, 4, 4]])) and got.base is None
    assert (MX.bits(got) == MX.bits(MX.NAN_PAYLOAD)).any()


# ---- systematic resampling ---------------------------------------------------------------------------------------------------
def counts_of(parents):
    return np.bincount(parents, minlength=len(parents)).tolist()


def test_uniform_weights_give_the_identity():
    for M, u in ((5, 0.3), (5, 0.5), (51, 0.9), (4, 0.0), (8, 0.0), (1, 0.0), (128, 0.25)):
        p = AS.systematic_parents(np.full(M, 1.0 / M), u)
        assert p.dtype == np.int32 and np.array_equal(p, np.arange(M)), (M, u)
    assert np.array_equal(AS.systematic_parents(np.full(6, 7.0), 0.5), np.arange(6))        # (normalised inside)


def test_one_dominant_weight_gives_every_member_the_same_parent():
    for M, k in ((5, 3), (9, 0), (51, 50)):
        w = np.zeros(M)
        w[k] = 1.0
        for u in (0.0, 0.4, np.nextafter(1.0, 0.0)):
            assert np.array_equal(AS.systematic_parents(w, u), np.full(M, k)), (M, k, u)
        w[w == 0] = 1e-9               # (the others' intervals are shorter than the distance of a point to them)
        assert np.array_equal(AS.systematic_parents(w, 0.4), np.full(M, k)), (M, k)


def test_the_counts_are_the_textbook_counts_at_both_ends_of_u():
    """weights 1/2, 1/4, 1/8, 1/8: cumulated 0.5, 0.75, 0.875, 1 (exact).  u = 0: the points 0, 0.25, 0.5, 0.75 fall into
    [0, .5) twice, [.5, .75) and [.75, .875) once: counts 2 1 1 0.  u just below 1: the points just below 0.25, 0.5, 0.75 and
    1 fall into [0, .5) twice, [.5, .75) once and [.875, 1) once: counts 2 1 0 1.  A member that is drawn keeps its slot."""
    w = np.array([0.5, 0.25, 0.125, 0.125])
    p = AS.systematic_parents(w, 0.0)
    assert counts_of(p) == [2, 1, 1, 0] and p.tolist() == [0, 1, 2, 0]
    p = AS.systematic_parents(w, np.nextafter(1.0, 0.0))
    assert counts_of(p) == [2, 1, 0, 1] and p.tolist() == [0, 1, 0, 3]
    # u = 1/2: the points 1/8, 3/8, 5/8, 7/8 -> 2 1 0 1 (7/8 is the left end of the last interval)
    assert counts_of(AS.systematic_parents(w, 0.5)) == [2, 1, 0, 1]
    # three copies of one member and two of another: the spare copies fill the free slots in ascending order
    p = AS.systematic_parents(np.array([0.0, 0.6, 0.0, 0.0, 0.4]), 0.5)
    assert counts_of(p) == [0, 3, 0, 0, 2] and p.tolist() == [1, 1, 1, 4, 4]
    for bad in (dict(weights=[0.0, 0.0], u=0.5), dict(weights=[0.5, -0.1], u=0.5), dict(weights=[0.5, 0.5], u=1.0),
                dict(weights=[0.5, np.nan], u=0.5), dict(weights=[[0.5, 0.5]], u=0.5)):
        with pytest.raises(ValueError):
            AS.systematic_parents(**bad)


# ---- the stochastic EnKF as a transform ------------------------------------------------------------------------------------
def enkf_problem():
    """6 members, 3 gauges, 40 state elements; the gauges observe three of the elements; obs_var 1.5 x the ensemble variance"""
    rng = np.random.default_rng(2024)
    M, G, S = 6, 3, 40
    X = rng.standard_normal((M, S)) * 3.0 + rng.uniform(-5, 5, S)
    hx = X[:, [3, 17, 30]].copy()
    obs_var = 1.5 * hx.var(axis=0, ddof=1)
    obs = hx.mean(axis=0) + rng.standard_normal(G)
    Y = obs + np.sqrt(obs_var) * rng.standard_normal((M, G))
    return X, hx, obs, obs_var, Y


def test_enkf_weights_of_no_innovation_are_the_identity():
    X, hx, obs, obs_var, _ = enkf_problem()
    W = AS.enkf_weights(hx, obs, obs_var, hx)
    assert W.dtype == np.float64 and np.array_equal(W, np.eye(6))
    with pytest.raises(ValueError):
        AS.enkf_weights(hx, obs[:2], obs_var, hx)
    with pytest.raises(ValueError):
        AS.enkf_weights(hx, obs, obs_var, hx[:5])
    with pytest.raises(ValueError):
        AS.enkf_weights(hx[:1], obs, obs_var, hx[:1])


def test_enkf_weights_are_the_textbook_update():
    """X W against X + K (Y - HX), K = P_xy (P_yy + R)^-1 with the sample covariances, both in float64.  The two differ in
    association order only.  Measured on the CPU this was written on: the largest difference is 3.553e-15 absolute,
    3.040e-16 of the largest |X| (11.686); asserted at 16 x that, 4.864e-15 of the largest |X|."""
    X, hx, obs, obs_var, Y = enkf_problem()
    M = X.shape[0]
    W = AS.enkf_weights(hx, obs, obs_var, Y)
    got = MX.transform(X, W)                                          # X_a[m] = sum_k X[k] W[k][m], as the device sums it
    Xc, A = X - X.mean(axis=0), hx - hx.mean(axis=0)
    Pxy, Pyy = Xc.T @ A / (M - 1), A.T @ A / (M - 1)
    K = Pxy @ np.linalg.inv(Pyy + np.diag(obs_var))                   # [state, gauges]
    want = X + (Y - hx) @ K.T
    scale = np.abs(X).max()
    worst = np.abs(got - want).max() / scale
    print("enkf: largest difference %.3e absolute, %.3e of max |X| = %.3f" % (np.abs(got - want).max(), worst, scale))
    assert worst <= 16 * 3.040e-16
    assert np.abs(want - X).max() > 0.01 * scale                      # (the update moved the state: something to compare)
    assert np.abs(W.sum(axis=0) - 1.0).max() < 1e-14                  # columns sum to 1: a constant state row stays constant
