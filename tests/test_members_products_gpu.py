"""lf_members_summary_device and lf_members_order_statistics_device on the device against their restatement
(members_products.py), bit for bit with NaN equal to NaN: every size around a workgroup, every tile width of the order kernel
and both sides of each switch, plain and padded strides, with and without a permuting destination index into longer outputs
(what nothing maps to keeps its sentinel), 0 / 1 / 4 thresholds, every subset of the outputs left out, divisor 1 and 24."""
import itertools

import numpy as np
import pytest

import members_products as MP
from module_edges import first_difference, same_bits

pytestmark = pytest.mark.gpu

SUBSETS = list(itertools.product((False, True), repeat=3))          # mean, min, max asked for


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


_values = {}


def case(n, members, divisor, n_thresholds=4):
    """(raw, x = raw / divisor, thresholds with their cases planted on x, order table of x): made once per shape"""
    key = (n, members, divisor)
    if key not in _values:
        raw, thr = MP.make_values(n, members, 1000 * members + n, n_thresholds)
        x = MP.values_of(MP.layout(raw, n), members, n, n, divisor)
        _values[key] = (raw, x, MP.plant_thresholds(x, thr), {})
    return _values[key]


def run_summary(amd, raw, stride, divisor, index, dst_n, want, thresholds, tstride):
    """the device call -> {"mean" / "min" / "max": [dst_n], "exceed": [T, dst_n]} of the outputs asked for"""
    L = amd.lib()
    members, n = raw.shape
    T = thresholds.shape[0]
    d_rows = amd.DeviceArray.from_host(MP.layout(raw, stride))
    d_index = None if index is None else amd.DeviceArray.from_host(index)
    d_thr = amd.DeviceArray.from_host(MP.layout(thresholds, tstride)) if T else None
    outs = {k: amd.DeviceArray.from_host(np.full(dst_n, MP.OUT_SENTINEL)) for k, on in zip(("mean", "min", "max"), want) if on}
    if T:
        outs["exceed"] = amd.DeviceArray.from_host(np.full((T, dst_n), int(MP.OUT_SENTINEL), np.int32))
    p = lambda d: None if d is None else d.ptr
    amd.check(L.lf_members_summary_device(0, d_rows.ptr, members, stride, n, divisor, p(d_index), dst_n, p(outs.get("mean")),
                                          p(outs.get("min")), p(outs.get("max")), T, p(d_thr), tstride, p(outs.get("exceed"))))
    got = {k: d.download() for k, d in outs.items()}
    assert same_bits(d_rows.download(), MP.layout(raw, stride))               # the rows and their pads are as they were
    for d in [d_rows, d_index, d_thr] + list(outs.values()):
        if d is not None:
            d.free()
    return got


def summary_reference(x, index, dst_n, want, thresholds):
    ref = {k: MP.scatter(f(x), index, dst_n) for (k, f), on in zip((("mean", MP.mean_of), ("min", MP.min_of), ("max", MP.max_of)), want)
           if on}
    if thresholds.shape[0]:
        ref["exceed"] = MP.scatter(MP.exceed_of(x, thresholds), index, dst_n, int(MP.OUT_SENTINEL))
    return ref


@pytest.mark.parametrize("members", [1, 2, 5, 9, 51])
def test_summary_against_the_restatement(amd, members):
    seen, count = set(), 0
    for n, pad, indexed, T, divisor in itertools.product((1, 255, 256, 257, 1000), (0, 37), (False, True), (0, 1, 4), (1.0, 24.0)):
        raw, x, thr, _ = case(n, members, divisor)
        want = SUBSETS[count % 8]
        if T == 0 and not any(want):                # (nothing asked for at all is refused: test_members_products_cpu.py)
            want = SUBSETS[(count + 3) % 8]
        count += 1
        seen.add((want, T > 0))
        dst_n = n + 11 if indexed else n
        index = MP.make_index(n, dst_n, n + members) if indexed else None
        got = run_summary(amd, raw, n + pad, divisor, index, dst_n, want, thr[:T], n + (5 if pad else 0))
        ref = summary_reference(x, index, dst_n, want, thr[:T])
        what = (n, pad, indexed, T, divisor, want)
        assert sorted(got) == sorted(ref), what
        for k in ref:
            if k == "exceed":
                assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (what, k)
            else:
                assert same_bits(got[k], ref[k]), (what, k, first_difference(got[k], ref[k]))
            if indexed:
                assert (np.delete(got[k], index, axis=-1) == MP.OUT_SENTINEL).all(), (what, k)
    assert {w for w, _ in seen} == set(SUBSETS) and ((False, False, False), True) in seen      # every subset was left out once


@pytest.mark.parametrize("members", [2, 5, 9, 51])
def test_the_sum_runs_in_member_order(amd, members):
    """Two members swapped: the mean keeps its bits exactly where the restatement's does.  Members 0 and 1 meet in the first
    addition, which commutes, so nothing may change; members 1 and 2 (last two of more) change the rounding in places.  A sum
    in another order -- pairs, a tree, from the last member down -- changes elsewhere."""
    n, stride = 1000, 1037
    raw, x, thr, _ = case(n, members, 24.0)
    base = run_summary(amd, raw, stride, 24.0, None, n, (True, False, False), thr[:0], n)["mean"]
    assert same_bits(base, MP.mean_of(x))
    differs = False
    for a, b in ((0, 1), (1, 2), (0, members - 1)):
        if b >= members or a == b:
            continue
        swapped = raw.copy()
        swapped[[a, b]] = raw[[b, a]]
        got = run_summary(amd, swapped, stride, 24.0, None, n, (True, False, False), thr[:0], n)["mean"]
        ref = MP.mean_of(MP.values_of(MP.layout(swapped, stride), members, stride, n, 24.0))
        assert same_bits(got, ref), ((a, b), first_difference(got, ref))
        assert np.array_equal(MP.same_bits_at(got, base), MP.same_bits_at(ref, MP.mean_of(x))), (a, b)
        if (a, b) == (0, 1):
            assert MP.same_bits_at(got, base).all()
        differs |= not MP.same_bits_at(ref, MP.mean_of(x)).all()
    assert differs == (members > 2)                # (the check had something to see)


def run_order(amd, raw, stride, divisor, index, dst_n, ranks):
    L = amd.lib()
    members, n = raw.shape
    ranks = np.array(ranks, np.int32)
    d_rows = amd.DeviceArray.from_host(MP.layout(raw, stride))
    d_index = None if index is None else amd.DeviceArray.from_host(index)
    d_out = amd.DeviceArray.from_host(np.full((ranks.size, dst_n), MP.OUT_SENTINEL))
    rc = L.lf_members_order_statistics_device(0, d_rows.ptr, members, stride, n, divisor, None if index is None else d_index.ptr,
                                              dst_n, ranks.size, amd.ptr(ranks), d_out.ptr)
    got = d_out.download()
    assert same_bits(d_rows.download(), MP.layout(raw, stride))
    for d in (d_rows, d_index, d_out):
        if d is not None:
            d.free()
    return rc, got


@pytest.mark.parametrize("members", [1, 2, 32, 33, 64, 65, 128])
def test_order_statistics_against_the_restatement(amd, members):
    count = 0
    for n, pad, indexed in itertools.product((1, 63, 64, 65, 300), (0, 37), (False, True)):
        for ranks in ((0,), (members - 1,), (0, members // 2, members - 1)):
            divisor = (1.0, 24.0)[count % 2]
            count += 1
            raw, x, _, tables = case(n, members, divisor)
            if "order" not in tables:
                tables["order"] = MP.order_table(x)
            dst_n = n + 11 if indexed else n
            index = MP.make_index(n, dst_n, n + members) if indexed else None
            rc, got = run_order(amd, raw, n + pad, divisor, index, dst_n, ranks)
            amd.check(rc)
            ref = MP.scatter(tables["order"][list(ranks)], index, dst_n)
            what = (n, pad, indexed, ranks, divisor)
            assert same_bits(got, ref), (what, first_difference(got, ref))
            for c in (1, 2):                       # the zeros kept their signs
                if c < n and not indexed:
                    assert np.array_equal(np.signbit(got[:, c]), np.signbit(ref[:, c])), what


def test_129_members_are_refused(amd):
    raw = np.zeros((129, 5))
    rc, got = run_order(amd, raw, 5, 1.0, None, 5, (0, 128))
    assert rc == amd.LF_E_INVALID and b"at most 128 members" in amd.lib().lf_last_error()
    assert (got == MP.OUT_SENTINEL).all()
