"""No GPU: the host side of the zonal sums -- the invariants of zonal.ZonePlan (every pair once, positions ascending within
a zone, runs of 0 .. 256 entries inside one zone, the last pass one run per zone, the pass counts of a census of zone
sizes), the two forms of zones, a channel row's plan on a channel domain from synthetic; the restatement the GPU tests
compare with (members_zonal.py) one float at a time, on planted values whose bits tell the order, on -0.0, NaN, inf and
padding, and against math.fsum within the bound of its additions; the plan's own host sums against the restatement;
assimilation.zone_geometry against hand-computed centroids; lf_members_zonal_device in the header, the library and the
ctypes table, and what it refuses device-free."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import members_zonal as MZ
from lisflood_amd import _lib
from lisflood_amd import assimilation as AS
from lisflood_amd import zonal as ZN

HEADER = os.path.join(ROOT, "include", "lisflood_amd.h")
NAME, SIGNATURE = "lf_members_zonal_device", "ipiqdqppqppq"
FAKE = C.c_void_p(64)              # a pointer that is never dereferenced: every call here ends before a device is touched
U = 2.0 ** -53                     # the unit roundoff of a double
CENSUS = [0, 1, 63, 64, 65, 255, 256, 257, 512, 513, 65536, 65537]
PASSES = [1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3]
ROW = 70000
BIG = 2.0 ** 53


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def census_pairs(seed=0):
    """zones of the census sizes on a row of 70 000 positions, each zone's positions distinct, the pairs shuffled"""
    rng = np.random.default_rng(seed)
    zone = np.repeat(np.arange(len(CENSUS)), CENSUS)
    pos = np.concatenate([rng.choice(ROW, size, replace=False) for size in CENSUS])
    order = rng.permutation(zone.size)
    return zone[order], pos[order]


@pytest.fixture(scope="module")
def census():
    zone, pos = census_pairs()
    return zone, pos, ZN.ZonePlan(zone, pos, len(CENSUS))


def check_plan(plan, zone, pos):
    Z = plan.zones
    assert plan.entries == zone.size and plan.passes == len(plan.run_start) == len(plan.zone_of_run)
    got = np.stack([plan.zone_of_entry.astype(np.int64), plan.positions.astype(np.int64)])
    want = np.stack([zone, pos])
    assert np.array_equal(got[:, np.lexsort(got[::-1])], want[:, np.lexsort(want[::-1])])       # every pair exactly once
    same = np.diff(plan.zone_of_entry) == 0
    assert (np.diff(plan.zone_of_entry) >= 0).all() and (np.diff(plan.positions.astype(np.int64))[same] >= 0).all()
    values_zone = plan.zone_of_entry
    for p in range(plan.passes):
        start, zr = plan.run_start[p].astype(np.int64), plan.zone_of_run[p]
        assert start.dtype == np.int64 and plan.run_start[p].dtype == np.int32 and zr.dtype == np.int32
        assert start.size == zr.size + 1 == plan.runs(p) + 1 and start[0] == 0 and start[-1] == values_zone.size
        length = np.diff(start)
        assert (length >= 0).all() and (length <= 256).all()
        assert np.array_equal(np.repeat(zr, length), values_zone)                                # no run crosses a zone
        assert (np.diff(zr) >= 0).all() and np.array_equal(np.unique(zr), np.arange(Z))           # every zone has a run
        per_zone = np.bincount(values_zone, minlength=Z)
        assert np.array_equal(np.bincount(zr, minlength=Z), np.maximum(1, -(-per_zone // 256)))   # no run more than needed
        full = np.ones(zr.size, bool)
        full[np.concatenate([np.flatnonzero(np.diff(zr)), [zr.size - 1]])] = False                # all but a zone's last run
        assert (length[full] == 256).all()
        values_zone = zr
    assert np.array_equal(plan.zone_of_run[-1], np.arange(Z))
    assert all(plan.runs(p) > Z for p in range(plan.passes - 1))                                  # no pass after the last


def test_plan_invariants_on_the_census(census):
    zone, pos, plan = census
    check_plan(plan, zone, pos)
    assert np.array_equal(plan.pixels, plan.positions)
    assert np.array_equal(plan.weight_sum, np.asarray(CENSUS, np.float64)) and plan.weights is None


def test_pass_counts_of_the_census(census):
    """a zone's passes: 1 + the passes in which it still has more than one run"""
    _, _, plan = census
    many = [np.bincount(zr, minlength=plan.zones) > 1 for zr in plan.zone_of_run]
    assert (1 + np.sum(many, axis=0)).tolist() == PASSES and plan.passes == 3
    assert ZN.ZonePlan(np.zeros(65536, int), np.arange(65536), 1).passes == 2
    assert ZN.ZonePlan(np.zeros(65537, int), np.arange(65537), 1).passes == 3
    one = ZN.ZonePlan(np.zeros(0, int), np.zeros(0, int), 3)
    assert one.passes == 1 and one.run_start[0].tolist() == [0, 0, 0, 0] and one.weight_sum.tolist() == [0.0, 0.0, 0.0]
    none = ZN.ZonePlan(np.zeros(0, int), np.zeros(0, int), 0)
    assert none.passes == 1 and none.runs(0) == 0 and none.run_start[0].tolist() == [0]


def test_plan_refuses_what_it_cannot_place():
    for zone, pos, Z, word in [([0, 1], [0], 2, "one length"), ([0, 2], [0, 1], 2, "0 .. zones - 1"), ([-1], [0], 1, "0 .. zones - 1"),
                               ([0], [-1], 1, "negative"), ([0], [2 ** 31], 1, "32-bit")]:
        with pytest.raises(ValueError, match=word):
            ZN.ZonePlan(zone, pos, Z)
    with pytest.raises(ValueError, match="weight_of_entry"):
        ZN.ZonePlan([0, 0], [1, 2], 1, None, [1.0])


def test_negative_labels_are_dropped_and_overlapping_lists_kept():
    labels = np.array([2, -1, 0, 0, -7, 2, 1, 0], np.int32)
    zone, pix, Z = ZN.zone_pairs(labels, 8)
    assert Z == 3 and pix.tolist() == [0, 2, 3, 5, 6, 7] and zone.tolist() == [2, 0, 0, 2, 1, 0]
    plan = ZN.row_plan(labels, None, 8, np.arange(8)[::-1])                 # position p holds pixel 7 - p
    assert plan.zone_of_entry.tolist() == [0, 0, 0, 1, 2, 2] and plan.positions.tolist() == [0, 4, 5, 1, 2, 7]
    assert plan.pixels.tolist() == [7, 3, 2, 6, 5, 0] and plan.weight_sum.tolist() == [3.0, 1.0, 2.0]
    lists = [np.arange(8), np.array([2, 3, 4]), np.array([3]), np.zeros(0, int)]
    zone, pix, Z = ZN.zone_pairs(lists, 8)
    assert Z == 4 and zone.tolist() == [0] * 8 + [1] * 3 + [2] and pix.tolist() == list(range(8)) + [2, 3, 4, 3]
    plan = ZN.row_plan(lists, np.arange(8.0), 8, np.arange(8))
    check_plan(plan, zone, pix)
    assert plan.weight_sum.tolist() == [28.0, 9.0, 3.0, 0.0] and plan.weights.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 2, 3, 4, 3]
    for bad, word in [(np.zeros(7, int), "label map"), (np.zeros(8), "label map"), ([np.array([8])], "compressed land indices"),
                      ([np.array([-1])], "compressed land indices")]:
        with pytest.raises(ValueError, match=word):
            ZN.zone_pairs(bad, 8)
    with pytest.raises(ValueError, match="weights must be"):
        ZN.row_plan(labels, np.zeros(7), 8, np.arange(8))


def test_a_channel_row_drops_the_pixels_outside_its_domain():
    """on the channel domain of synthetic.hotpath_scenario, in an engine order of its own: a zone holds its pixels inside
    the domain, each at the position that holds it, and the weight sum is over those alone"""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.channel_domain import channel_domain
    H, W = 30, 40
    values, _, mask, _, kin = syn.hotpath_scenario(H, W)
    N = H * W
    ids, _ = channel_domain(values, kin, mask, True)
    assert 0 < ids.size < N
    rng = np.random.default_rng(5)
    gpix = ids[rng.permutation(ids.size)]
    rows, cols = np.nonzero(mask)
    labels = (2 * (rows >= H // 2) + (cols >= W // 2)).astype(np.int64)
    labels[rng.choice(N, 50, replace=False)] = -1
    weights = rng.uniform(0.5, 2.0, N)
    lists = [np.arange(N), np.flatnonzero(rows < 10), np.flatnonzero((rows < 10) & (cols < 7)), np.setdiff1d(np.arange(N), ids)]
    for zones in (labels, lists):
        zone, pix, Z = ZN.zone_pairs(zones, N)
        plan = ZN.row_plan(zones, weights, N, gpix)
        keep = np.isin(pix, ids)
        assert 0 < keep.sum() < pix.size
        assert np.array_equal(gpix[plan.positions], plan.pixels)
        for z in range(Z):
            assert np.array_equal(np.sort(plan.pixels[plan.zone_of_entry == z]), np.sort(pix[keep & (zone == z)])), z
        assert np.array_equal(plan.weights, weights[plan.pixels])
        assert np.array_equal(bits(plan.weight_sum), bits(MZ.weight_sums(plan.pixels, plan.run_start, weights)))
        land = ZN.row_plan(zones, None, N, rng.permutation(N))
        assert land.entries == pix.size and np.array_equal(land.weight_sum, np.bincount(zone, minlength=Z))
    assert plan.weight_sum[3] == 0.0 and not (plan.zone_of_entry == 3).any()      # the zone outside the domain: one empty run


# ---- the restatement itself --------------------------------------------------------------------------------------------
PLANTED = {                      # entry -> value in one zone laid on positions 0 .. len - 1, and the sum its order gives
    "lane_small_first": (256, {0: 1.0, 64: BIG, 128: -BIG}, 0.0),        # ((0 + 1) + 2^53) - 2^53: the 1 is rounded away
    "lane_small_last": (256, {0: BIG, 64: -BIG, 128: 1.0}, 1.0),
    "lane_fourth": (256, {0: BIG, 64: 1.0, 128: 1.0, 192: -BIG}, 0.0),    # each 1 rounded away on its own
    "fold_32_before_16": (64, {0: 1.0, 32: BIG, 16: -BIG}, 0.0),          # d = 32 makes 1 + 2^53, d = 16 takes it away
    "fold_16_after_32": (64, {0: BIG, 32: -BIG, 16: 1.0}, 1.0),
    "fold_1_last": (64, {0: BIG, 2: -BIG, 1: 1.0}, 1.0),                  # d = 2: 2^53 - 2^53; d = 1: 0 + 1
    "fold_2_before_1": (64, {0: 1.0, 2: BIG, 1: -BIG}, 0.0),              # d = 2: 1 + 2^53 -> 2^53; d = 1: 2^53 - 2^53
    "run_boundary_lost": (257, {0: BIG, 1: 1.0, 256: -BIG}, 0.0),         # run 0 = 2^53 + 1 -> 2^53, run 1 = -2^53
    "run_boundary_kept": (257, {0: BIG, 1: -BIG, 256: 1.0}, 1.0),
    "second_run_lane": (512, {256: 1.0, 320: BIG, 384: -BIG, 0: 1.0}, 1.0),
    "third_pass": (65537, {0: BIG, 65535: 1.0, 65536: -BIG}, 0.0),        # pass 2: run 0 = 2^53 (+ 1 lost), run 1 = -2^53
    "third_pass_kept": (65537, {0: BIG, 255: -BIG, 65536: 1.0}, 1.0),
}


@pytest.mark.parametrize("case", list(PLANTED))
def test_planted_values_tell_the_order(case):
    n, planted, want = PLANTED[case]
    v = np.zeros((1, n))
    for e, x in planted.items():
        v[0, e] = x
    plan = ZN.ZonePlan(np.zeros(n, int), np.arange(n), 1)
    got = MZ.zonal_sums(v, plan.pixels, plan.run_start)
    assert got.shape == (1, 1) and got[0, 0] == want and not np.signbit(got[0, 0])
    assert np.array_equal(bits(plan.sums(v)), bits(got))
    if n <= 256:
        assert MZ.run_sum(v[0]) == want


def test_the_vector_form_is_the_rule_one_float_at_a_time():
    rng = np.random.default_rng(11)
    for length in (0, 1, 63, 64, 65, 128, 200, 255, 256):
        v = rng.standard_normal(length) * 10.0 ** rng.integers(-8, 9, length)
        got = MZ.pass_sums(v[None], [0, length])
        assert np.array_equal(bits(got), bits([[MZ.run_sum(v)]])), length
    v = rng.standard_normal(700)
    start = [0, 256, 300, 300, 556, 700]
    want = [MZ.run_sum(v[a:b]) for a, b in zip(start[:-1], start[1:])]
    assert np.array_equal(bits(MZ.pass_sums(np.stack([v, -v]), start)), bits([want, [-x if x else 0.0 for x in want]]))


def test_zeros_nan_inf_and_padding():
    one = lambda v, w=None, divisor=1.0: MZ.zonal_sums(np.asarray([v], np.float64), np.arange(len(v)), [np.array([0, len(v)])],
                                                       w, divisor)[0, 0]
    assert bits(one([-0.0])) == bits(0.0)                                   # 0.0 + -0.0
    assert bits(one([-0.0] * 256)) == bits(0.0)
    assert bits(one([])) == bits(0.0)                                       # an empty run: every lane the padding
    assert np.isnan(one([1.0, np.nan, 2.0])) and np.isnan(one([np.inf, 1.0, np.nan]))
    assert one([1.0, np.inf]) == np.inf and one([-np.inf] + [1.0] * 200) == -np.inf
    assert np.isnan(one([np.inf, -np.inf]))
    # padding never multiplies: a run of one entry with an infinite weight or value stays what the entry makes it -- a
    # padding lane times the weight would be 0 * inf, a NaN
    assert one([3.0], np.array([np.inf])) == np.inf and one([np.inf], np.array([2.0])) == np.inf
    assert one([3.0], np.array([2.0]), 24.0) == (3.0 / 24.0) * 2.0
    x, w, d = 0.1, 3.0, 7.0
    assert one([x], np.array([w]), d) == (x / d) * w and (x / d) * w != (x * w) / d      # two roundings, in this order
    assert bits(one([5e-324], None, 2.0)) == bits(0.0)                      # the division is IEEE: ties to even, to zero
    # the run sum of the library's own host sums does the same
    plan = ZN.ZonePlan([0, 0, 1, 3], [0, 1, 2, 3], 4)
    got = plan.sums(np.array([[-0.0, -0.0, np.nan, np.inf]]))
    assert np.array_equal(bits(got[0, [0, 2, 3]]), bits([0.0, 0.0, np.inf])) and np.isnan(got[0, 1])


def test_against_fsum_within_the_bound_of_the_additions():
    """|sum - fsum(t)| <= gamma_k sum |t| + half an ulp of the result, k = 10 passes (three inexact lane additions and six
    folds per pass, rounded up), gamma_k = k u / (1 - k u); t: the rounded terms"""
    zone, pos = census_pairs(3)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, ROW)) * 10.0 ** rng.integers(-6, 7, (2, ROW))
    w = rng.uniform(0.0, 3.0, ROW)
    plan = ZN.ZonePlan(zone, pos, len(CENSUS), None, w[pos])
    for weights, divisor in ((None, 1.0), (w, 24.0)):
        t = MZ.terms(x, plan.pixels, weights, divisor)
        got = MZ.zonal_sums(x, plan.pixels, plan.run_start, weights, divisor)
        many = [np.bincount(zr, minlength=plan.zones) > 1 for zr in plan.zone_of_run]
        passes = 1 + np.sum(many, axis=0)
        for m in range(2):
            for z in range(plan.zones):
                tz = t[m, plan.zone_of_entry == z]
                exact = math.fsum(tz)
                k = 10 * int(passes[z])
                bound = k * U / (1 - k * U) * math.fsum(np.abs(tz)) + 0.5 * np.spacing(abs(got[m, z]))
                assert abs(got[m, z] - exact) <= bound, (m, z, got[m, z], exact, bound)
    wsum = MZ.weight_sums(plan.pixels, plan.run_start, w)
    assert np.array_equal(bits(plan.weight_sum), bits(wsum))
    assert np.allclose(wsum, np.bincount(zone, w[pos], minlength=plan.zones), rtol=1e-12)


def test_the_plans_host_sums_are_the_restatement(census):
    zone, pos, _ = census
    rng = np.random.default_rng(9)
    x = rng.standard_normal((3, ROW))
    x[0, pos[:5]] = [-0.0, np.inf, np.nan, 1e300, -1e300]
    w = rng.uniform(0.5, 2.0, ROW)
    plan = ZN.ZonePlan(zone, pos, len(CENSUS), None, w[pos])
    want = MZ.zonal_sums(x, plan.pixels, plan.run_start, w, 24.0)
    assert np.array_equal(bits(plan.sums(MZ.terms(x, plan.pixels, w, 24.0))), bits(want))
    means = MZ.zonal_means(x, plan.pixels, plan.run_start, w, 24.0)
    assert np.isnan(means[:, 0]).all() and (want[:, 0] == 0.0).all()        # the empty zone: sum 0.0, mean NaN


def test_zone_geometry_against_hand_computed_centroids():
    mask = np.ones((4, 5), bool)
    mask[0, 0] = mask[3, 4] = False                     # pixel p of 18: the land cells in row-major order
    rows, cols = np.nonzero(mask)
    labels = np.full(18, -1)
    labels[[0, 1, 4, 5]] = 0                            # cells (0,1) (0,2) (1,0) (1,1)
    labels[17] = 2                                      # cell (3,3); zone 1 stays empty
    assert [(int(rows[p]), int(cols[p])) for p in (0, 1, 4, 5, 17)] == [(0, 1), (0, 2), (1, 0), (1, 1), (3, 3)]
    xy, radius = AS.zone_geometry(labels, mask)
    assert xy[0].tolist() == [0.5, 1.0] and np.isnan(xy[1]).all() and xy[2].tolist() == [3.0, 3.0]
    assert np.array_equal(radius, np.sqrt(np.array([4, 0, 1]) / np.pi))
    w = np.ones(18)
    w[[0, 1, 4, 5]] = [1.0, 3.0, 0.0, 4.0]              # rows: (0 + 0 + 0 + 4) / 8, columns: (1 + 6 + 0 + 4) / 8
    xy, radius = AS.zone_geometry([np.array([0, 1, 4, 5]), np.array([5, 17])], mask, w)
    assert xy.tolist() == [[0.5, 1.375], [(4.0 + 3.0) / 5.0, (4.0 + 3.0) / 5.0]]
    assert np.array_equal(radius, np.sqrt(np.array([4, 2]) / np.pi))
    hx = np.array([[1.0, 2.0], [2.0, 1.5], [4.0, 0.5]])
    inc = AS.serial_increments(hx, np.array([2.0, 1.0]), np.ones(2), xy, np.maximum(2.0, radius))     # takes them as gauges
    assert inc.gauges == 2 and np.array_equal(inc.gx, xy[:, 0])
    for bad, word in [((labels, np.ones((4, 5))), "boolean"), ((labels, mask, np.ones(17)), "weights must be")]:
        with pytest.raises(ValueError, match=word):
            AS.zone_geometry(*bad)


# ---- the C entry point ------------------------------------------------------------------------------------------------
def last_error():
    return _lib.lib().lf_last_error()


def test_the_export_is_in_the_header_the_library_and_the_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    table = {"lf_" + n: sig for sig, names in _lib._SIGNATURES.items() for n in names.split()}
    f = getattr(_lib.lib(), NAME)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, text)
    assert re.search(r"\sT\s+%s$" % NAME, dynamic, flags=re.M)
    assert table[NAME] == SIGNATURE
    assert list(f.argtypes) == [_lib._KIND[k] for k in SIGNATURE] and f.restype is C.c_int


def test_the_header_states_the_arithmetic():
    text = " ".join(open(HEADER).read().replace("\n *", " ").split())
    for line in ("x = rows_dev[m * stride + (index_dev ? index_dev[e] : e)]", "t = divisor == 1.0 ? x : x / divisor",
                 "t = weights_dev ? t * weights_dev[e] : t", "padded to 256 with +0.0", "never a product",
                 "s = 0.0; s = s + v[l]; s = s + v[l + 64]; s = s + v[l + 128]; s = s + v[l + 192]",
                 "for d = 32, 16, 8, 4, 2, 1: s[l] = s[l] + s[l + d] for l < d", "out_dev[m * out_stride + r] = s[0]",
                 "no atomics"):
        assert line in text, line


def zonal(**kw):
    a = dict(rows=FAKE, members=3, stride=1005, divisor=1.0, entries=1000, index=FAKE, weights=FAKE, runs=8, run_start=FAKE,
             out=FAKE, out_stride=8)
    a.update(kw)
    return _lib.lib().lf_members_zonal_device(0, a["rows"], a["members"], a["stride"], a["divisor"], a["entries"], a["index"],
                                              a["weights"], a["runs"], a["run_start"], a["out"], a["out_stride"])


REFUSED = {                        # arguments, the word of the message
    "members_0": (dict(members=0), b"members must be at least 1"),
    "members_negative": (dict(members=-2), b"members must be at least 1"),
    "entries_negative": (dict(entries=-1), b"entries = -1"),
    "entries_beyond_32_bits": (dict(entries=2 ** 31), b"entries = 2147483648 outside the 32-bit range"),
    "runs_negative": (dict(runs=-1), b"runs = -1"),
    "runs_beyond_32_bits": (dict(runs=2 ** 31, out_stride=2 ** 31), b"runs = 2147483648 outside the 32-bit range"),
    "run_start_null": (dict(run_start=None), b"run_start_dev"),
    "out_null": (dict(out=None), b"out_dev"),
    "out_stride_short": (dict(out_stride=7), b"out_stride 7 is less than runs = 8"),
    "rows_null": (dict(rows=None), b"rows_dev"),
    "divisor_0": (dict(divisor=0.0), b"divisor"),
    "divisor_minus_0": (dict(divisor=-0.0), b"divisor"),
    "divisor_nan": (dict(divisor=np.nan), b"divisor"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_the_call_refuses_before_a_device_is_touched(case):
    kw, word = REFUSED[case]
    assert zonal(**kw) == _lib.LF_E_INVALID, case
    assert word in last_error(), (case, last_error())


def test_what_needs_no_device_is_ok_without_one():
    """runs == 0 launches nothing, whatever the other pointers; rows_dev may be NULL where there is no entry to read"""
    assert zonal(runs=0, out_stride=0) == _lib.LF_OK
    assert zonal(runs=0, out_stride=0, run_start=None, out=None, index=None, weights=None) == _lib.LF_OK
    assert zonal(runs=0, out_stride=0, entries=0, rows=None) == _lib.LF_OK
    assert zonal(runs=0, out_stride=0, divisor=24.0, members=1) == _lib.LF_OK
