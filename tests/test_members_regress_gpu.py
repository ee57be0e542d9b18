"""lf_members_regress_device on the device against its restatement (members_regress.py) on the uint64 view, with no
tolerance: every NaN as one pattern where a gauge touched the element, the raw bits elsewhere.  Every size around a
wavefront and a workgroup, member counts on both sides of the rows staged at once and of the two workgroup widths, gauge
counts from one to the limit of a call, plain and padded strides with a sentinel between the rows that must keep its
bits, each bound absent, a scalar and a row.  The inputs plant both sides and the ties of every comparison of the kernel
(test_members_regress_cpu.py holds the census)."""
import itertools

import numpy as np
import pytest

import members_regress as MR

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
MEMBERS = (2, 3, 7, 8, 9, 16, 17, 51, 64)
GAUGES = (1, 2, 7, 64, 256)
BOUNDS = ("absent", "scalar", "row")
OPTIONS = list(itertools.product(BOUNDS, BOUNDS, (0, 5)))            # lower, upper, pad: 18


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def up(amd, a):
    return None if a is None else amd.DeviceArray.from_host(np.ascontiguousarray(a, np.float64))


def run(amd, x, stride, cx, cy, table, gauges, lower=("absent", None, -np.inf), upper=("absent", None, np.inf), times=1):
    """the call on x [members, n] laid out with `stride` -> (rows after it, what lies between them)"""
    members, n = x.shape
    d_rows, d_cx, d_cy, d_t = up(amd, MR.layout(x, stride)), up(amd, cx), up(amd, cy), up(amd, table)
    d_lo, d_hi = up(amd, lower[1]), up(amd, upper[1])
    p = lambda d: None if d is None else d.ptr
    for _ in range(times):
        amd.check(amd.lib().lf_members_regress_device(0, d_rows.ptr, members, stride, n, gauges, d_cx.ptr, d_cy.ptr, d_t.ptr,
                                                      p(d_lo), lower[2], p(d_hi), upper[2]))
    image = d_rows.download().reshape(members, stride)
    for d in (d_rows, d_cx, d_cy, d_t, d_lo, d_hi):
        if d is not None:
            d.free()
    return image[:, :n], image[:, n:]


def untouched(gaps):
    return np.array_equal(MR.bits(gaps), MR.bits(np.full(gaps.shape, MR.SENTINEL)))


@pytest.mark.parametrize("members", MEMBERS)
def test_regress_against_the_restatement(amd, members):
    seen, count = set(), MEMBERS.index(members)
    for n, gauges in itertools.product(SIZES, GAUGES):
        option = OPTIONS[count % len(OPTIONS)]
        count += 1
        seen.add(option)
        lower, upper, pad = option
        x, cx, cy, table = MR.make_case(n, members, gauges, 100 * members + n + gauges)
        lo, hi = MR.bound_of(lower, n, n + 2, True), MR.bound_of(upper, n, n + 3, False)
        got, gaps = run(amd, x, n + pad, cx, cy, table, gauges, (lower,) + lo[1:], (upper,) + hi[1:])
        want, touched = MR.regress(x, cx, cy, table, gauges, lo[0], hi[0])
        bad = np.argwhere(MR.agree(got, want, touched))
        assert bad.size == 0, (members, n, gauges, option, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
        assert untouched(gaps), (members, n, gauges, option)
        assert touched.any() and (n < 10 or not touched.all())
        if lower == upper == "absent":                   # no bounds: what no gauge touched keeps every bit it had
            assert np.array_equal(MR.bits(got[:, ~touched]), MR.bits(x[:, ~touched])), (members, n, gauges)
    assert seen == set(OPTIONS)                          # every combination of bounds and padding came up for this member count


@pytest.mark.parametrize("members,n,gauges", [(2, 65, 1), (7, 257, 7), (17, 64, 64), (51, 1000, 256), (64, 255, 2)])
def test_a_call_with_every_gauge_out_of_range_leaves_the_raw_bits(amd, members, n, gauges):
    """the gauges moved far from every element: no column is stored, -0.0, the NaN payload and the sentinel between the rows
    stay; with a NaN for every coordinate as well"""
    x, cx, cy, table = MR.make_case(n, members, gauges, 9)
    A, D, s, gx, gy, c, cut2 = MR.sections(table, members, gauges)
    away = np.concatenate([A.ravel(), D.ravel(), s, gx - 5000.0, gy + 7000.0, c, cut2])
    _, touched = MR.regress(x, cx, cy, away, gauges)
    assert not touched.any()
    got, gaps = run(amd, x, n + 5, cx, cy, away, gauges)
    assert np.array_equal(MR.bits(got), MR.bits(x)) and untouched(gaps)
    assert (MR.bits(got) == MR.bits(MR.NAN_PAYLOAD)).any() and (np.signbit(got) & (got == 0)).any()
    got, gaps = run(amd, x, n, np.full(n, np.nan), np.full(n, np.nan), table, gauges)
    assert np.array_equal(MR.bits(got), MR.bits(x))
    # infinite scalar bounds are no bounds; a finite one is applied to the elements no gauge touched too
    lo = MR.bound_of("scalar", n, 1, True)
    got, gaps = run(amd, x, n + 5, cx, cy, away, gauges, ("scalar",) + lo[1:])
    want, _ = MR.regress(x, cx, cy, away, gauges, lo[0])
    assert np.array_equal(MR.bits(got), MR.bits(want)) and untouched(gaps) and not np.array_equal(MR.bits(got), MR.bits(x))


@pytest.mark.parametrize("members,n,gauges", [(3, 63, 2), (9, 256, 7), (51, 257, 64)])
def test_twice_is_the_restatement_twice(amd, members, n, gauges):
    """two calls are one call with the gauges listed twice: the filter is serial (how regress() splits more than 256)"""
    x, cx, cy, table = MR.make_case(n, members, gauges, 8)
    got, gaps = run(amd, x, n + 5, cx, cy, table, gauges, times=2)
    once, t1 = MR.regress(x, cx, cy, table, gauges)
    want, t2 = MR.regress(once, cx, cy, table, gauges)
    assert not MR.agree(got, want, t1 | t2).any() and untouched(gaps) and MR.agree(once, want, t1).any()
    if 2 * gauges <= 256:
        A, D, s, gx, gy, c, cut2 = (np.concatenate([a, a]) for a in MR.sections(table, members, gauges))
        both = np.concatenate([A.ravel(), D.ravel(), s, gx, gy, c, cut2])
        single, _ = run(amd, x, n, cx, cy, both, 2 * gauges)
        assert not MR.agree(single, want, t1 | t2).any()
