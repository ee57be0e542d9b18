"""lf_members_transform_device and lf_members_resample_device on the device against their restatement
(members_transform.py), on the uint64 view (every NaN as one pattern for the transform, the raw bits for the resample):
every size around a wavefront and a workgroup, member counts on both sides of a register block, of the rows staged at
once and of the two workgroup widths, plain and padded strides with a sentinel between the rows that must keep its bits,
with and without a taper, each bound absent, a scalar and a row, four weight matrices."""
import itertools

import numpy as np
import pytest

import members_transform as MX

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
MEMBERS = (1, 2, 7, 8, 9, 16, 17, 51, 64)
BOUNDS = ("absent", "scalar", "row")
OPTIONS = list(itertools.product((False, True), BOUNDS, BOUNDS))          # taper, lower, upper: 18


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def up(amd, a):
    return None if a is None else amd.DeviceArray.from_host(np.ascontiguousarray(a, np.float64))


def run_transform(amd, x, stride, W, taper=None, lower=("absent", None, -np.inf), upper=("absent", None, np.inf), times=1):
    """the call on x [members, n] laid out with `stride` -> (rows after it, what lies between them)"""
    members, n = x.shape
    d_rows, d_w, d_t = up(amd, MX.layout(x, stride)), up(amd, W), up(amd, taper)
    d_lo, d_hi = up(amd, lower[1]), up(amd, upper[1])
    p = lambda d: None if d is None else d.ptr
    for _ in range(times):
        amd.check(amd.lib().lf_members_transform_device(0, d_rows.ptr, members, stride, n, d_w.ptr, p(d_t), p(d_lo), lower[2],
                                                        p(d_hi), upper[2]))
    image = d_rows.download().reshape(members, stride)
    for d in (d_rows, d_w, d_t, d_lo, d_hi):
        if d is not None:
            d.free()
    return image[:, :n], image[:, n:]


def run_resample(amd, x, stride, parents):
    members, n = x.shape
    d_rows = up(amd, MX.layout(x, stride))
    rc = amd.lib().lf_members_resample_device(0, d_rows.ptr, members, stride, n, amd.ptr(np.asarray(parents, np.int32)))
    image = d_rows.download().reshape(members, stride)
    d_rows.free()
    return rc, image[:, :n], image[:, n:]


def untouched(gaps):
    return np.array_equal(MX.bits(gaps), MX.bits(np.full(gaps.shape, MX.SENTINEL)))


@pytest.mark.parametrize("members", MEMBERS)
def test_transform_against_the_restatement(amd, members):
    seen, count = set(), MEMBERS.index(members)
    for n, kind, pad in itertools.product(SIZES, MX.MATRICES, (0, 5)):
        option = OPTIONS[count % len(OPTIONS)]
        count += 1
        seen.add(option)
        with_taper, lower, upper = option
        x, W = MX.make_rows(n, members, 100 * members + n), MX.matrix(kind, members, members + n)
        taper = MX.make_taper(n, n + 1) if with_taper else None
        lo, hi = MX.bound_of(lower, n, n + 2, True), MX.bound_of(upper, n, n + 3, False)
        got, gaps = run_transform(amd, x, n + pad, W, taper, (lower,) + lo[1:], (upper,) + hi[1:])
        want = MX.transform(x, W, taper, lo[0], hi[0])
        bad = np.argwhere(MX.canonical(got) != MX.canonical(want))
        assert bad.size == 0, (members, n, kind, pad, option, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
        assert untouched(gaps), (members, n, kind, pad, option)
    assert seen == set(OPTIONS)                      # every combination of taper and bounds came up for this member count


@pytest.mark.parametrize("members,n", [(1, 65), (7, 257), (17, 64), (51, 1000), (64, 255)])
def test_infinite_scalar_bounds_and_no_taper_leave_every_bit_of_the_sum(amd, members, n):
    """the call without taper and bounds is the call with them absent: -inf / +inf take nothing, -0.0 and NaN included; and
    a taper of exactly 0 keeps the member's own value where t is finite"""
    x, W = MX.make_rows(n, members, 5), MX.affine(members, 9)
    got, gaps = run_transform(amd, x, n + 5, W)
    want = MX.transform(x, W)
    assert MX.same(got, want) and untouched(gaps)
    assert np.isnan(got).any() or n < 4
    zero = np.zeros(n)
    kept, _ = run_transform(amd, x, n, W, zero)
    finite = np.isfinite(want)
    assert MX.same(kept, MX.transform(x, W, zero)) and np.array_equal(kept[finite], x[finite])


@pytest.mark.parametrize("n", [65, 257])
def test_one_member_under_the_identity_keeps_every_raw_bit(amd, n):
    """Where the arithmetic cannot touch a NaN -- one member, W = [[1]], t = x * 1 -- the raw bits are held, the payload of
    the planted NaN included: with no bounds (-inf / +inf leave every bit of v), with finite scalar bounds and bound rows
    (a NaN v passes either: no comparison with it is true) wherever the bound itself takes nothing, and under a taper of 1
    on the finite elements.  (With more members the NaN is the result of an operation, and its sign and payload are the
    device's own: those comparisons count every NaN as one pattern.)"""
    x = MX.make_rows(n, 1, 17)
    x[0, 20] = MX.NAN_PAYLOAD
    one = np.ones((1, 1))
    got, gaps = run_transform(amd, x, n + 5, one)
    assert np.array_equal(MX.bits(got), MX.bits(x)) and untouched(gaps)
    assert (MX.bits(got) == MX.bits(MX.NAN_PAYLOAD)).sum() == 2 and np.signbit(got[0, 0]) and got[0, 0] == 0
    lo, hi = MX.bound_of("scalar", n, 1, True), MX.bound_of("row", n, 2, False)
    got, _ = run_transform(amd, x, n, one, None, ("scalar",) + lo[1:], ("row",) + hi[1:])
    want = MX.transform(x, one, None, lo[0], hi[0])
    assert np.array_equal(MX.bits(got), MX.bits(want))               # raw bits: the restatement's NaNs are copies here too
    nan = np.isnan(x)
    assert np.array_equal(MX.bits(got[nan & ~np.isnan(hi[0])[None, :]]), MX.bits(x[nan & ~np.isnan(hi[0])[None, :]]))


@pytest.mark.parametrize("members,n", [(2, 63), (9, 256), (51, 257)])
def test_twice_is_the_restatement_twice(amd, members, n):
    x, W, taper = MX.make_rows(n, members, 8), MX.affine(members, 4), MX.make_taper(n, 6)
    lo, hi = MX.bound_of("row", n, 1, True), MX.bound_of("scalar", n, 2, False)
    got, gaps = run_transform(amd, x, n + 5, W, taper, ("row",) + lo[1:], ("scalar",) + hi[1:], times=2)
    once = MX.transform(x, W, taper, lo[0], hi[0])
    want = MX.transform(once, W, taper, lo[0], hi[0])
    assert MX.same(got, want) and untouched(gaps) and not MX.same(once, want)


def parents_of(kind, members):
    if kind == "identity":
        return np.arange(members, dtype=np.int32)
    if kind == "cycle":
        return MX.cycle(members)
    if kind == "one_parent":
        return np.full(members, members // 2, np.int32)
    return np.random.default_rng(members).integers(0, members, members).astype(np.int32)       # "drawn"


@pytest.mark.parametrize("kind", ["identity", "cycle", "one_parent", "drawn"])
def test_resample_copies_the_bits(amd, kind):
    for members, n, pad in [(m, n, pad) for m in (1, 2, 7, 9, 33, 51, 65) for n in SIZES for pad in (0, 5)] + [(128, 65, 0), (128, 65, 5)]:
        x = MX.make_rows(n, members, 3 * members + n)
        parents = parents_of(kind, members)
        rc, got, gaps = run_resample(amd, x, n + pad, parents)
        assert rc == amd.LF_OK, (kind, members, n, pad)
        assert np.array_equal(MX.bits(got), MX.bits(MX.resample(x, parents))), (kind, members, n, pad)
        assert untouched(gaps), (kind, members, n, pad)
        if kind == "identity":                       # the rows keep their bits and the call reports success
            assert np.array_equal(MX.bits(got), MX.bits(x))
        elif n > len(MX.PLANTS) and members > 1:     # (a NaN's payload was among the bits that moved)
            assert (MX.bits(x) == MX.bits(MX.NAN_PAYLOAD)).any()
