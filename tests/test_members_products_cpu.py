"""No GPU: the host side of the products over an ensemble's members -- lf_members_summary_device and
lf_members_order_statistics_device are in the header, the library and the ctypes table; every refusal comes back as
LF_E_INVALID with the argument named before a device is touched (there is none here); and the restatement the GPU tests
compare with (members_products.py) is itself held to np.sort(kind="stable"), to math.fsum and to the list of planted cases."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import members_products as MP
from lisflood_amd import _lib
from module_edges import first_difference, same_bits

HEADER = os.path.join(ROOT, "include", "lisflood_amd.h")
EXPORTS = {"lf_members_summary_device": "ipiqqdpqpppipqp", "lf_members_order_statistics_device": "ipiqqdpqipp"}
N = 600
FAKE = C.c_void_p(64)              # a pointer that is never dereferenced: every call here ends before a device is touched


def last_error():
    return _lib.lib().lf_last_error()


def test_the_exports_are_in_the_header_the_library_and_the_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    table = {"lf_" + name: sig for sig, names in _lib._SIGNATURES.items() for name in names.split()}
    L = _lib.lib()
    for name, sig in EXPORTS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert re.search(r"\sT\s+%s$" % name, dynamic, flags=re.M), name
        assert table[name] == sig, name
        assert list(getattr(L, name).argtypes) == [_lib._KIND[k] for k in sig] and getattr(L, name).restype is C.c_int


def summary(**kw):
    a = dict(rows=FAKE, members=3, stride=N + 5, n=N, divisor=1.0, index=FAKE, dst_n=N + 7, mean=FAKE, min=FAKE, max=FAKE,
             n_thresholds=2, thresholds=FAKE, threshold_stride=N, exceed=FAKE)
    a.update(kw)
    return _lib.lib().lf_members_summary_device(0, a["rows"], a["members"], a["stride"], a["n"], a["divisor"], a["index"], a["dst_n"],
                                                a["mean"], a["min"], a["max"], a["n_thresholds"], a["thresholds"],
                                                a["threshold_stride"], a["exceed"])


def order(**kw):
    a = dict(rows=FAKE, members=5, stride=N + 5, n=N, divisor=1.0, index=FAKE, dst_n=N + 7, ranks=(0, 2, 4), out=FAKE)
    a.update(kw)
    ranks = None if a["ranks"] is None else np.array(a["ranks"], np.int32)
    n_ranks = a.get("n_ranks", 0 if ranks is None else ranks.size)
    return _lib.lib().lf_members_order_statistics_device(0, a["rows"], a["members"], a["stride"], a["n"], a["divisor"], a["index"],
                                                         a["dst_n"], n_ranks, _lib.ptr(ranks), a["out"])


BOTH = {                           # refused by both entry points: arguments, the word of the message
    "members_0": (dict(members=0), b"members"),
    "members_negative": (dict(members=-3), b"members"),
    "n_negative": (dict(n=-1, stride=0, dst_n=0), b"n = -1"),
    "n_beyond_a_launch": (dict(n=2 ** 31, stride=2 ** 31, dst_n=2 ** 31, threshold_stride=2 ** 31), b"32-bit"),
    "stride_short": (dict(stride=N - 1), b"stride"),
    "no_index_and_another_length": (dict(index=None, dst_n=N + 1), b"dst_n"),
    "dst_n_short": (dict(dst_n=N - 1), b"dst_n"),
    "rows_null": (dict(rows=None), b"rows_dev"),
}
SUMMARY_ONLY = {
    "thresholds_negative": (dict(n_thresholds=-1), b"n_thresholds"),
    "thresholds_5": (dict(n_thresholds=5), b"n_thresholds"),
    "thresholds_null": (dict(thresholds=None), b"thresholds_dev"),
    "exceed_null": (dict(exceed=None), b"exceed_dev"),
    "threshold_stride_short": (dict(threshold_stride=N - 1), b"threshold_stride"),
    "no_output": (dict(mean=None, min=None, max=None, n_thresholds=0, thresholds=None, exceed=None), b"no output"),
}
ORDER_ONLY = {
    "ranks_0": (dict(ranks=(), n_ranks=0), b"n_ranks"),
    "ranks_9": (dict(ranks=(0,) * 9), b"n_ranks"),
    "ranks_null": (dict(ranks=None, n_ranks=2), b"ranks_host"),
    "rank_negative": (dict(ranks=(0, -1)), b"rank -1"),
    "rank_is_members": (dict(ranks=(4, 5)), b"rank 5"),
    "members_129": (dict(members=129, ranks=(0, 128)), b"at most 128 members"),
    "out_null": (dict(out=None), b"out_dev"),
}


@pytest.mark.parametrize("case", list(BOTH) + list(SUMMARY_ONLY))
def test_the_summary_call_refuses_before_a_device_is_touched(case):
    kw, word = (BOTH if case in BOTH else SUMMARY_ONLY)[case]
    assert summary(**kw) == _lib.LF_E_INVALID, case
    assert word in last_error(), (case, last_error())


@pytest.mark.parametrize("case", list(BOTH) + list(ORDER_ONLY))
def test_the_order_call_refuses_before_a_device_is_touched(case):
    kw, word = (BOTH if case in BOTH else ORDER_ONLY)[case]
    kw = {k: v for k, v in kw.items() if k != "threshold_stride"}
    assert order(**kw) == _lib.LF_E_INVALID, case
    assert word in last_error(), (case, last_error())


def test_an_empty_call_is_ok_and_launches_nothing():
    """n == 0: LF_OK with no device on the box, and with one nothing reads the fake pointers; the arguments are still checked"""
    assert summary(n=0, stride=0, dst_n=0, index=None, threshold_stride=0) == _lib.LF_OK
    assert summary(n=0, stride=0, dst_n=0, rows=None) == _lib.LF_OK
    assert order(n=0, stride=0, dst_n=0, index=None, rows=None, out=None) == _lib.LF_OK
    assert summary(n=0, stride=0, dst_n=0, n_thresholds=7) == _lib.LF_E_INVALID
    assert order(n=0, stride=0, dst_n=0, ranks=(5,)) == _lib.LF_E_INVALID


@pytest.mark.skipif(_lib.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_a_valid_call_needs_a_device():
    """the limits themselves pass the checks: 4 thresholds, 8 ranks, 128 members, no index with dst_n == n"""
    assert summary(n_thresholds=4) == _lib.LF_E_NO_DEVICE
    assert summary(mean=None, min=None, max=None, n_thresholds=1) == _lib.LF_E_NO_DEVICE
    assert summary(n_thresholds=0, thresholds=None, exceed=None, min=None, index=None, dst_n=N) == _lib.LF_E_NO_DEVICE
    assert order(members=128, ranks=(0, 1, 2, 3, 64, 126, 127, 127)) == _lib.LF_E_NO_DEVICE
    assert order(members=1, ranks=(0,), index=None, dst_n=N, stride=N) == _lib.LF_E_NO_DEVICE


# ---- the restatement ---------------------------------------------------------------------------------------------------------
CASES = [(300, 2), (300, 5), (300, 9), (40, 51), (64, 128)]       # n, members


def planted(n, members, divisor, n_thresholds=2):
    raw, thr = MP.make_values(n, members, 7 * n + members, n_thresholds)
    stride = n + 37
    x = MP.values_of(MP.layout(raw, stride), members, stride, n, divisor)
    return x, MP.plant_thresholds(x, thr)


@pytest.mark.parametrize("divisor", [1.0, 24.0])
@pytest.mark.parametrize("n,members", CASES)
def test_every_planted_case_is_there(n, members, divisor):
    x, thr = planted(n, members, divisor)
    assert MP.census(x, thr) == set(MP.PLANTS)
    assert not np.isnan(x[:, 13:]).any() and x.shape == (members, n)          # the pads were not read
    # ... and the threshold cases count what their names say
    e = MP.exceed_of(x, thr)
    assert (e[:, 9] == 0).all() and (e[:, 10] == members).all() and (e[:, 11] == 0).all() and (e[:, 12] == 0).all()
    assert 0 < e[:, 13:].max() <= members and e.min() == 0


@pytest.mark.parametrize("divisor", [1.0, 24.0])
@pytest.mark.parametrize("n,members", CASES)
def test_the_order_statistics_are_the_stable_sort(n, members, divisor):
    x, _ = planted(n, members, divisor)
    want = np.sort(x, axis=0, kind="stable")
    got = MP.order_table(x)
    assert same_bits(got, want), first_difference(got, want)
    assert (np.signbit(got[:, 1]) == np.signbit(want[:, 1])).all() and np.signbit(got[0, 1]) and not np.signbit(got[0, 2])


@pytest.mark.parametrize("n,members", CASES)
def test_the_mean_is_within_the_bound_of_a_sequential_sum(n, members):
    """M - 1 additions and one division, each rounded once: |mean - exact| <= M u sum|x| / M to first order in u = 2^-53
    (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2, plus one rounding for the division); asserted
    with gamma_M = M u / (1 - M u) in place of (M - 1) u, which also covers the higher-order terms"""
    x, _ = planted(n, members, 24.0)
    got = MP.mean_of(x)
    u = 2.0 ** -53
    gamma = members * u / (1 - members * u)
    finite = np.isfinite(x).all(axis=0)
    assert finite.sum() >= n - 9
    for i in np.flatnonzero(finite):
        exact = math.fsum(x[:, i]) / members
        bound = gamma * math.fsum(np.abs(x[:, i])) / members + abs(exact) * u
        assert abs(got[i] - exact) <= bound, (i, got[i], exact, bound)
    assert np.isnan(got[~finite][2:]).all() and got[3] == np.inf and got[4] == -np.inf


def test_the_folds_keep_the_earlier_member_and_the_nan():
    x, _ = planted(300, 5, 1.0)
    lo, hi = MP.min_of(x), MP.max_of(x)
    assert np.signbit(lo[1]) and np.signbit(hi[1]) and not np.signbit(lo[2]) and not np.signbit(hi[2])    # -0.0 / +0.0 came first
    assert np.isnan(lo[5:9]).all() and np.isnan(hi[5:9]).all()
    assert lo[3] < np.inf and hi[3] == np.inf and lo[4] == -np.inf
    ok = ~np.isnan(x).any(axis=0)
    assert np.array_equal(lo[ok], x[:, ok].min(axis=0)) and np.array_equal(hi[ok], x[:, ok].max(axis=0))


def test_scatter_leaves_the_sentinel():
    index = MP.make_index(20, 31, 3)
    assert np.unique(index).size == 20 and not np.array_equal(index, np.sort(index))
    out = MP.scatter(np.arange(20.0), index, 31)
    assert (out == MP.OUT_SENTINEL).sum() == 11 and np.array_equal(out[index], np.arange(20.0))
    assert np.array_equal(MP.scatter(np.arange(5, dtype=np.int32), None, 5), np.arange(5))
