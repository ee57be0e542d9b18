"""No GPU: the host side of the run-long accumulators of an ensemble -- lf_members_track_device is in the header, the library
and the ctypes table; every refusal comes back as LF_E_INVALID with the argument named before a device is touched (there is
none here); and the restatement the GPU tests compare with (members_track.py) is itself held to numpy where numpy says the
same thing (max / argmax / argmax of the comparison / its sum), to math.fsum and to the list of planted cases."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import members_track as MT
from lisflood_amd import _lib

HEADER = os.path.join(ROOT, "include", "lisflood_amd.h")
NAME, SIGNATURE = "lf_members_track_device", "ipiqqdiiqpppipqpp"
N = 600
FAKE = C.c_void_p(64)              # a pointer that is never dereferenced: every call here ends before a device is touched
# the shapes of tests/test_members_track_gpu.py
MEMBERS, SIZES, THRESHOLDS, DIVISORS = (1, 2, 8, 9, 17, 51), (1, 255, 256, 257, 1000), (0, 1, 4), (1.0, 24.0)


def last_error():
    return _lib.lib().lf_last_error()


def test_the_export_is_in_the_header_the_library_and_the_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    table = {"lf_" + name: sig for sig, names in _lib._SIGNATURES.items() for name in names.split()}
    f = getattr(_lib.lib(), NAME)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, text)
    assert re.search(r"\sT\s+%s$" % NAME, dynamic, flags=re.M)
    assert table[NAME] == SIGNATURE
    assert list(f.argtypes) == [_lib._KIND[k] for k in SIGNATURE] and f.restype is C.c_int
    assert SIGNATURE.count("p") == 7 and SIGNATURE.count("q") == 4 and SIGNATURE.count("d") == 1


def track(**kw):
    a = dict(rows=FAKE, members=3, stride=N + 5, n=N, divisor=1.0, step=0, first=1, track_stride=N + 3, peak=FAKE, peak_step=FAKE,
             sum=FAKE, n_thresholds=2, thresholds=FAKE, threshold_stride=N, first_above=FAKE, steps_above=FAKE)
    a.update(kw)
    return _lib.lib().lf_members_track_device(0, a["rows"], a["members"], a["stride"], a["n"], a["divisor"], a["step"], a["first"],
                                              a["track_stride"], a["peak"], a["peak_step"], a["sum"], a["n_thresholds"],
                                              a["thresholds"], a["threshold_stride"], a["first_above"], a["steps_above"])


NOTHING = dict(peak=None, peak_step=None, sum=None, n_thresholds=0, thresholds=None, first_above=None, steps_above=None)
REFUSED = {                        # arguments, the word of the message
    "members_0": (dict(members=0), b"members"),
    "members_negative": (dict(members=-3), b"members"),
    "n_negative": (dict(n=-1, stride=0, track_stride=0), b"n = -1"),
    "n_beyond_a_launch": (dict(n=2 ** 31, stride=2 ** 31, track_stride=2 ** 31, threshold_stride=2 ** 31), b"32-bit"),
    "stride_short": (dict(stride=N - 1), b"stride"),
    "rows_null": (dict(rows=None), b"rows_dev"),
    "track_stride_short": (dict(track_stride=N - 1), b"track_stride"),
    "step_negative": (dict(step=-1), b"step"),
    "thresholds_negative": (dict(n_thresholds=-1), b"n_thresholds"),
    "thresholds_5": (dict(n_thresholds=5), b"n_thresholds"),
    "thresholds_null": (dict(thresholds=None), b"thresholds_dev"),
    "threshold_stride_short": (dict(threshold_stride=N - 1), b"threshold_stride"),
    "both_threshold_outputs_null": (dict(first_above=None, steps_above=None), b"first_above_dev and steps_above_dev"),
    "peak_step_without_peak": (dict(peak=None), b"peak_step_dev without peak_dev"),
    "no_output": (NOTHING, b"no output"),
    "no_output_with_unused_threshold_rows": (dict(NOTHING, first_above=FAKE, steps_above=FAKE), b"no output"),
}


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("case", list(REFUSED))
def test_the_call_refuses_before_a_device_is_touched(case, first):
    kw, word = REFUSED[case]
    assert track(first=first, **kw) == _lib.LF_E_INVALID, case
    assert word in last_error(), (case, last_error())


def test_an_empty_call_is_ok_and_launches_nothing():
    """n == 0: LF_OK with no device on the box, and with one nothing reads the fake pointers; the arguments are still checked"""
    assert track(n=0, stride=0, track_stride=0, threshold_stride=0) == _lib.LF_OK
    assert track(n=0, stride=0, track_stride=0, rows=None, first=0, step=7) == _lib.LF_OK
    assert track(n=0, stride=0, track_stride=0, n_thresholds=7) == _lib.LF_E_INVALID
    assert track(n=0, stride=0, track_stride=0, step=-2) == _lib.LF_E_INVALID


@pytest.mark.skipif(_lib.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_a_valid_call_needs_a_device():
    """the limits themselves pass the checks: 4 thresholds, strides equal to n, one member, each output alone"""
    assert track(n_thresholds=4) == _lib.LF_E_NO_DEVICE
    assert track(members=1, stride=N, track_stride=N, threshold_stride=N, step=2 ** 31 - 1, first=0) == _lib.LF_E_NO_DEVICE
    assert track(**dict(NOTHING, peak=FAKE)) == _lib.LF_E_NO_DEVICE
    assert track(**dict(NOTHING, sum=FAKE)) == _lib.LF_E_NO_DEVICE
    assert track(peak=None, peak_step=None, sum=None, steps_above=None) == _lib.LF_E_NO_DEVICE
    assert track(peak=None, peak_step=None, sum=None, first_above=None, n_thresholds=1) == _lib.LF_E_NO_DEVICE


# ---- the restatement ---------------------------------------------------------------------------------------------------------
CASES = [(300, 2, 4), (300, 5, 7), (40, 9, 12), (64, 3, 25)]       # n, members, steps


def planted(n, members, steps, divisor, n_thresholds=2):
    raw, thr = MT.make_series(n, members, steps, 7 * n + members, n_thresholds)
    x = MT.values_of(raw, divisor)
    return x, MT.plant_thresholds(x, thr)


@pytest.mark.parametrize("members", MEMBERS)
def test_every_planted_case_is_there_in_every_shape_of_the_gpu_test(members):
    """the census equals the list of the cases planted in the columns a shape has"""
    for n, T, divisor in itertools.product(SIZES, THRESHOLDS, DIVISORS):
        raw, thr = MT.make_series(n, members, len(MT.STEPS), 1000 * members + n, 4)
        x = MT.values_of(raw, divisor)
        thr = MT.plant_thresholds(x, thr)[:T]
        assert MT.census(x, thr) == MT.planted_in(n, T), (n, T, divisor)
    assert MT.planted_in(255, 1) == set(MT.PLANTS) and MT.planted_in(1, 4) == {"all_equal"}
    assert MT.planted_in(1000, 0) == set(MT.PLANTS) - set(MT.THRESHOLD_PLANTS)


@pytest.mark.parametrize("divisor", DIVISORS)
@pytest.mark.parametrize("n,members,steps", CASES)
def test_the_restatement_is_numpy_where_numpy_says_the_same(n, members, steps, divisor):
    x, thr = planted(n, members, steps, divisor)
    assert MT.census(x, thr) == set(MT.PLANTS)
    numbers = np.arange(steps) * 3 + 1                                  # the caller's step numbers: ascending, not 0 .. S - 1
    acc = MT.fold(x, thr, numbers)
    ok = ~np.isnan(x).any(axis=0)                                       # [members, n]: the NaN-free columns
    assert ok.sum() >= members * (n - 4)
    assert np.array_equal(acc["peak"][ok], x.max(axis=0)[ok])
    assert np.array_equal(acc["peak_step"][ok], numbers[np.argmax(x, axis=0)][ok])         # (argmax: the first occurrence)
    with np.errstate(invalid="ignore"):
        for t in range(thr.shape[0]):
            above = x > thr[t]                                          # every column: a NaN on either side is never above
            want = np.where(above.any(axis=0), numbers[np.argmax(above, axis=0)], -1)
            assert np.array_equal(acc["first_above"][t], want)
            assert np.array_equal(acc["steps_above"][t], above.sum(axis=0))
    assert acc["peak_step"].dtype == acc["first_above"].dtype == acc["steps_above"].dtype == np.int32
    # first_above without steps_above says the same
    alone = MT.fold(x, thr, numbers, keys=("first_above",))
    assert sorted(alone) == ["first_above"] and np.array_equal(alone["first_above"], acc["first_above"])


@pytest.mark.parametrize("n,members,steps", CASES)
def test_the_sum_is_within_the_bound_of_a_sequential_sum(n, members, steps):
    """S - 1 additions, each rounded once: |sum - exact| <= (S - 1) u sum|x| to first order in u = 2^-53 (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2); asserted with gamma_S = S u / (1 - S u), which also covers the
    higher-order terms"""
    x, thr = planted(n, members, steps, 24.0)
    got = MT.fold(x, thr)["sum"]
    u = 2.0 ** -53
    gamma = steps * u / (1 - steps * u)
    finite = np.isfinite(x).all(axis=0)
    assert finite.sum() >= members * (n - 6)
    for m, i in np.argwhere(finite):
        exact = math.fsum(x[:, m, i])
        assert abs(got[m, i] - exact) <= gamma * math.fsum(np.abs(x[:, m, i])), (m, i, got[m, i], exact)
    c = MT.COLUMN
    assert np.isnan(got[:, [c["nan_first"], c["nan_middle"], c["nan_last"], c["nan_only"]]]).all()
    assert (got[:, c["plus_inf_middle"]] == np.inf).all() and (got[:, c["minus_inf_last"]] == -np.inf).all()


def test_the_peak_keeps_the_earlier_step_and_the_nan():
    x, thr = planted(300, 5, 7, 1.0)
    numbers = (0, 2, 3, 5, 8, 9, 11)
    acc = MT.fold(x, thr, numbers)
    c, last, mid = MT.COLUMN, numbers[-1], numbers[7 // 2]
    peak, at = acc["peak"], acc["peak_step"]
    assert (at[:, c["all_equal"]] == 0).all() and (at[:, c["rise_to_a_tie"]] == 0).all() and (peak[:, c["rise_to_a_tie"]] == 5).all()
    assert np.signbit(peak[:, c["minus_zero_first"]]).all() and (at[:, c["minus_zero_first"]] == 0).all()
    assert not np.signbit(peak[:, c["plus_zero_first"]]).any() and (at[:, c["plus_zero_first"]] == 0).all()
    assert (peak[:, c["plus_inf_middle"]] == np.inf).all() and (at[:, c["plus_inf_middle"]] == mid).all()
    assert np.isfinite(peak[:, c["minus_inf_last"]]).all() and (at[:, c["minus_inf_last"]] != last).all()
    for name, when in (("nan_first", 0), ("nan_middle", mid), ("nan_last", last), ("nan_only", 0)):   # a NaN sticks from its step
        assert np.isnan(peak[:, c[name]]).all() and (at[:, c[name]] == when).all(), name
    for name, first, count in (("at_threshold", -1, 0), ("ulp_above", 0, 7), ("ulp_below", -1, 0), ("nan_threshold", -1, 0),
                               ("above_first_only", 0, 1), ("above_last_only", last, 1), ("never_above", -1, 0)):
        assert (acc["first_above"][:, :, c[name]] == first).all() and (acc["steps_above"][:, :, c[name]] == count).all(), name


def test_layout_puts_the_sentinel_between_the_rows():
    rows = np.arange(12, dtype=np.int32).reshape(2, 2, 3)
    flat = MT.layout(rows, 5, MT.I32_SENTINEL).reshape(4, 5)
    assert np.array_equal(flat[:, :3].reshape(2, 2, 3), rows) and (flat[:, 3:] == MT.I32_SENTINEL).all() and flat.dtype == np.int32
    assert MT.same(np.array([np.nan, -0.0]), np.array([-np.nan, -0.0])) and not MT.same(np.array([0.0]), np.array([-0.0]))
