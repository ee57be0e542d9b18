"""lf_members_track_device on the device against its restatement (members_track.py), bit for bit with NaN equal to NaN, after
every one of four updates: member counts on both sides of the rows in flight, every size around a workgroup, plain and padded
strides of the source and of the accumulators independently (what lies between the rows keeps its sentinel, the source rows
and their NaN pads stay as they were), 0 / 1 / 4 thresholds, divisor 1 and 24, every subset of the outputs left out once."""
import itertools

import numpy as np
import pytest

import members_products as MP
import members_track as MT
from module_edges import same_bits

pytestmark = pytest.mark.gpu

F64, I32 = ("peak", "sum"), ("peak_step", "first_above", "steps_above")
# the outputs a call may leave out: peak_step needs peak, thresholds need first_above or steps_above
PLAIN = [s for s in itertools.product((False, True), repeat=3) if s[0] or not s[1]]               # peak, peak_step, sum
THRESHOLDED = [(True, True), (True, False), (False, True)]                                         # first_above, steps_above
SUBSETS = [(p, (False, False)) for p in PLAIN if any(p)] + [(p, t) for p in PLAIN for t in THRESHOLDED]


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


_values = {}


def case(n, members, divisor, n_thresholds=4):
    """(raw [4, members, n], x = raw / divisor, thresholds with their cases planted on x): made once per shape"""
    key = (n, members, divisor)
    if key not in _values:
        raw, thr = MT.make_series(n, members, len(MT.STEPS), 1000 * members + n, n_thresholds)
        x = MT.values_of(raw, divisor)
        _values[key] = (raw, x, MT.plant_thresholds(x, thr))
    return _values[key]


def keys_of(subset, T):
    (peak, peak_step, total), (first_above, steps_above) = subset
    on = dict(peak=peak, peak_step=peak_step, sum=total, first_above=T > 0 and first_above, steps_above=T > 0 and steps_above)
    return tuple(k for k in MT.KEYS if on[k])


class Device:
    """the accumulators `keys` of one tracker on the device, preset with a sentinel everywhere, and its thresholds"""

    def __init__(self, amd, members, n, track_stride, thresholds, tstride, keys, f64=MT.F64_SENTINEL, i32=MT.I32_SENTINEL):
        self.amd, self.members, self.n, self.track_stride, self.tstride = amd, members, n, track_stride, tstride
        self.T = thresholds.shape[0]
        self.preset = MT.fresh(members, n, self.T, keys, f64, i32)
        self.acc = {k: amd.DeviceArray.from_host(np.full(a.size // n * track_stride, a.reshape(-1)[0], a.dtype))
                    for k, a in self.preset.items()}
        self.thr = amd.DeviceArray.from_host(MP.layout(thresholds, tstride)) if self.T else None

    def update(self, raw, stride, divisor, step, first):
        """one call with raw [members, n]; the source rows and their NaN pads must be as they were afterwards"""
        amd, p = self.amd, lambda d: None if d is None else d.ptr
        image = MP.layout(raw, stride)
        d_rows = amd.DeviceArray.from_host(image)
        amd.check(amd.lib().lf_members_track_device(0, d_rows.ptr, self.members, stride, self.n, divisor, step, int(first),
                                                    self.track_stride, p(self.acc.get("peak")), p(self.acc.get("peak_step")),
                                                    p(self.acc.get("sum")), self.T, p(self.thr), self.tstride,
                                                    p(self.acc.get("first_above")), p(self.acc.get("steps_above"))))
        assert same_bits(d_rows.download(), image)
        d_rows.free()

    def read(self):
        """key -> (rows as the restatement shapes them, the elements between the rows)"""
        out = {}
        for k, d in self.acc.items():
            rows = d.download().reshape(-1, self.track_stride)
            out[k] = rows[:, :self.n].reshape(self.preset[k].shape), rows[:, self.n:]
        return out

    def free(self):
        for d in list(self.acc.values()) + [self.thr]:
            if d is not None:
                d.free()


def check(dev, ref, what, f64=MT.F64_SENTINEL, i32=MT.I32_SENTINEL):
    got = dev.read()
    assert sorted(got) == sorted(ref), what
    for k, (rows, gaps) in got.items():
        assert MT.same(rows, ref[k]), (what, k, np.argwhere(~(MP.same_bits_at(rows, ref[k]) if k in F64 else rows == ref[k]))[:3])
        assert MT.same(gaps, np.full(gaps.shape, f64 if k in F64 else i32, gaps.dtype)), (what, k, "written between the rows")


@pytest.mark.parametrize("members", [1, 2, 8, 9, 17, 51])
def test_four_updates_against_the_restatement(amd, members):
    seen, count = set(), {False: 0, True: 0}
    for n, pad, tpad, T, divisor in itertools.product((1, 255, 256, 257, 1000), (0, 37), (0, 5), (0, 1, 4), (1.0, 24.0)):
        raw, x, thr = case(n, members, divisor)
        choices = [s for s in SUBSETS if (s[1] != (False, False)) == (T > 0)]       # 5 without thresholds, 18 with
        subset = choices[count[T > 0] % len(choices)]
        count[T > 0] += 1
        seen.add(subset)
        keys = keys_of(subset, T)
        dev = Device(amd, members, n, n + tpad, thr[:T], n + (5 if pad else 0), keys)
        ref = MT.fresh(members, n, T, keys)
        for s, step in enumerate(MT.STEPS):
            dev.update(raw[s], n + pad, divisor, step, s == 0)
            MT.update(ref, x[s], thr[:T], step, s == 0)
            check(dev, ref, (n, pad, tpad, T, divisor, keys, step))
        dev.free()
    assert seen == set(SUBSETS) and len(SUBSETS) == 23              # every subset of the outputs was left out once


@pytest.mark.parametrize("members,n,T", [(1, 257, 4), (9, 1000, 1), (17, 255, 0), (51, 256, 4)])
def test_a_first_update_reads_no_accumulator(amd, members, n, T):
    """on accumulators full of garbage -- NaN and -7 in the rows and between them -- a first update leaves the bits it leaves
    on fresh ones, and the garbage between the rows"""
    raw, x, thr = case(n, members, 24.0)
    keys = keys_of(((True, True, True), (True, True)), T)
    dev = Device(amd, members, n, n + 5, thr[:T], n, keys, f64=np.nan, i32=-7)
    ref = MT.fresh(members, n, T, keys)
    for s, step in enumerate(MT.STEPS[:2]):
        dev.update(raw[s], n + 37, 24.0, step, True)                # (twice: a first update after others starts over, too)
        MT.update(ref, x[s], thr[:T], step, True)
        check(dev, ref, (members, n, T, step), f64=np.nan, i32=-7)
    dev.update(raw[2], n + 37, 24.0, 4, False)
    MT.update(ref, x[2], thr[:T], 4, False)
    check(dev, ref, (members, n, T, "then a plain one"), f64=np.nan, i32=-7)
    dev.free()


@pytest.mark.parametrize("members,n,T", [(2, 257, 1), (9, 1000, 4), (51, 255, 2)])
def test_first_above_alone_is_first_above_with_steps_above(amd, members, n, T):
    raw, x, thr = case(n, members, 1.0)
    both = Device(amd, members, n, n + 5, thr[:T], n + 5, ("first_above", "steps_above"))
    alone = Device(amd, members, n, n, thr[:T], n, ("first_above",))
    for s, step in enumerate(MT.STEPS):
        for dev in (both, alone):
            dev.update(raw[s], n, 1.0, step, s == 0)
        a, b = both.read()["first_above"][0], alone.read()["first_above"][0]
        assert np.array_equal(a, b), (members, n, T, step)
    want = MT.fold(x, thr[:T], MT.STEPS, keys=("first_above", "steps_above"))["first_above"]
    assert np.array_equal(a, want) and (a == -1).any() and (a == 9).any() and (a == 0).any()
    both.free(); alone.free()


@pytest.mark.parametrize("members", [1, 9, 51])
def test_the_sum_runs_in_step_order(amd, members):
    """Two steps' inputs swapped: the sum keeps its bits exactly where the restatement's does.  Steps 0 and 1 meet in the first
    addition, which commutes, so nothing may change; steps 1 and 2, or 0 and 3, change the rounding in places."""
    n = 1000
    raw, x, thr = case(n, members, 24.0)

    def run(order):
        dev = Device(amd, members, n, n + 5, thr[:0], n, ("sum",))
        for s, step in enumerate(MT.STEPS):
            dev.update(raw[order[s]], n + 37, 24.0, step, s == 0)
        got = dev.read()["sum"][0]
        dev.free()
        return got

    base, ref_base = run((0, 1, 2, 3)), MT.fold(x, thr[:0], keys=("sum",))["sum"]
    assert MT.same(base, ref_base)
    differs = False
    for order in ((1, 0, 2, 3), (0, 2, 1, 3), (3, 1, 2, 0)):
        got, ref = run(order), MT.fold(x[list(order)], thr[:0], keys=("sum",))["sum"]
        assert MT.same(got, ref), order
        assert np.array_equal(MP.same_bits_at(got, base), MP.same_bits_at(ref, ref_base)), order
        if order == (1, 0, 2, 3):
            assert MP.same_bits_at(got, base).all()
        differs |= not MP.same_bits_at(ref, ref_base).all()
    assert differs                                                  # (the check had something to see)
