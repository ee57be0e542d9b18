"""lf_members_zonal_device on the device against its restatement (members_zonal.py) on the uint64 view, with no tolerance:
1, 3 and 5 members on rows of 70 000 elements with a padded stride and NaN sentinels between the rows (a finite result
proves they are not read), zones of the census sizes 0 .. 65 537 in one plan (three passes, an empty zone), with and
without weights, divisor 1.0 and 24.0, the rows in a permuted order and an index that does not ascend, rows holding -0.0,
inf and a NaN, every pass's output in rows with a sentinel behind the runs that must survive; and the same bits whether the
members go on the grid or not."""
import numpy as np
import pytest

import members_zonal as MZ
from test_members_zonal_cpu import CENSUS, ROW, bits, census_pairs

pytestmark = pytest.mark.gpu

PAD, OUT_PAD = 37, 3
SENTINEL = np.float64(np.nan)
MEMBERS = 5


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


@pytest.fixture(scope="module")
def case():
    """values [5, 70 000] in pixel order, the order of the row (position -> pixel), weights, and the plan of the census zones
    on that row; -0.0 is the single entry of zone 1, an inf lies in zone 2, a NaN in zone 4, one more of each and a -0.0
    in the zone of 65 537"""
    from lisflood_amd import zonal as ZN
    rng = np.random.default_rng(17)
    x = rng.standard_normal((MEMBERS, ROW)) * 10.0 ** rng.integers(-3, 4, (MEMBERS, ROW))
    w = rng.uniform(0.5, 2.0, ROW)
    pixel_of_position = rng.permutation(ROW)
    zone, pix = census_pairs(1)
    lists = [pix[zone == z] for z in range(len(CENSUS))]
    plan = ZN.row_plan(lists, w, ROW, pixel_of_position)
    assert plan.passes == 3 and plan.entries == sum(CENSUS) and not np.array_equal(plan.pixels, plan.positions)
    big = lists[-1]
    x[:, lists[1][0]] = -0.0
    x[0, lists[2][5]] = np.inf
    x[1, lists[4][60]] = np.nan
    x[2, big[[100, 40000, 65000]]] = [np.inf, -0.0, np.inf]
    x[3, big[300]] = np.nan
    return x, w, pixel_of_position, plan


def run_passes(amd, x, order, plan, index, weights, divisor, members):
    """every pass on the device -> the list of [members, runs_p] outputs; rows and outputs are padded and hold sentinels"""
    from lisflood_amd._lib import DeviceArray
    L = amd.lib()
    stride = ROW + PAD
    host = np.full((members, stride), SENTINEL)
    host[:, :ROW] = x[:members][:, order]
    keep = [DeviceArray.from_host(host.reshape(-1)), DeviceArray.from_host(np.ascontiguousarray(index, np.int32))]
    d_w = None
    if weights is not None:
        d_w = DeviceArray.from_host(np.ascontiguousarray(weights, np.float64))
        keep.append(d_w)
    rows, entries, outs = keep[0], plan.entries, []
    for p in range(plan.passes):
        runs, first = plan.runs(p), p == 0
        out_stride = runs + OUT_PAD
        d_start = DeviceArray.from_host(plan.run_start[p])
        d_out = DeviceArray.from_host(np.full(members * out_stride, SENTINEL))
        keep += [d_start, d_out]
        amd.check(L.lf_members_zonal_device(0, rows.ptr, members, stride, divisor if first else 1.0, entries,
                                            keep[1].ptr if first else None, d_w.ptr if first and d_w else None, runs,
                                            d_start.ptr, d_out.ptr, out_stride))
        got = d_out.download().reshape(members, out_stride)
        assert np.isnan(got[:, runs:]).all() and np.array_equal(bits(got[:, runs:]), bits(np.full((members, OUT_PAD), SENTINEL)))
        outs.append(got[:, :runs].copy())
        rows, stride, entries = d_out, out_stride, runs
    amd.synchronize(0)
    for d in keep:
        d.free()
    return outs


_WANT = {}


def want_passes(case, weighted, divisor):
    x, w, _, plan = case
    key = (weighted, divisor)
    if key not in _WANT:
        _WANT[key] = [MZ.zonal_sums(x, plan.pixels, plan.run_start, w if weighted else None, divisor, passes=p + 1)
                      for p in range(plan.passes)]
    return _WANT[key]


@pytest.mark.parametrize("divisor", [1.0, 24.0])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("members", [1, 3, 5])
def test_every_pass_is_the_restatement(amd, case, members, weighted, divisor):
    x, w, order, plan = case
    got = run_passes(amd, x, order, plan, plan.positions, plan.weights if weighted else None, divisor, members)
    want = want_passes(case, weighted, divisor)
    for p in range(plan.passes):
        assert got[p].shape == (members, plan.runs(p))
        assert np.array_equal(bits(got[p]), bits(want[p][:members])), (p, np.flatnonzero(bits(got[p]) != bits(want[p][:members]))[:8])
    sums = got[-1]
    assert sums.shape == (members, len(CENSUS))
    assert np.array_equal(bits(sums[:, :2]), bits(np.zeros((members, 2))))           # the empty zone and the lone -0.0: +0.0
    finite = np.isfinite(want[-1][:members])                     # (the zones overlap: a planted inf or NaN may lie in several)
    assert finite.sum() >= finite.size - 3 * len(CENSUS) // 2 and finite[4:].all()
    assert np.isfinite(sums[finite]).all()                                            # no sentinel between the rows was read
    if members == 5:
        assert sums[0, 2] == np.inf and np.isnan(sums[1, 4]) and sums[2, -1] == np.inf and np.isnan(sums[3, -1])


def test_an_index_that_does_not_ascend(amd, case):
    """the kernel takes the entries in the order of the index, whatever it is: each zone's entries shuffled"""
    x, w, order, plan = case
    rng = np.random.default_rng(3)
    shuffle = np.argsort(plan.zone_of_entry + rng.uniform(0.0, 0.9, plan.entries), kind="stable")
    assert np.array_equal(plan.zone_of_entry[shuffle], plan.zone_of_entry) and (np.diff(plan.positions[shuffle].astype(np.int64)) < 0).any()
    got = run_passes(amd, x, order, plan, plan.positions[shuffle], plan.weights[shuffle], 24.0, 3)[-1]
    want = MZ.zonal_sums(x[:3], plan.pixels[shuffle], plan.run_start, w, 24.0)
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(want), bits(want_passes(case, True, 24.0)[-1][:3]))          # (another order, other bits)


@pytest.mark.parametrize("grid", ["0", "1"])
def test_the_bits_do_not_depend_on_the_members_on_the_grid(amd, case, grid, monkeypatch):
    """5 members are more than a wavefront walks at a time: once every wavefront walks them all, once they go on the grid's
    second dimension in groups, the last group short"""
    x, w, order, plan = case
    monkeypatch.setenv("LF_ZONAL_GRID", grid)
    got = run_passes(amd, x, order, plan, plan.positions, plan.weights, 24.0, 5)
    for p, want in enumerate(want_passes(case, True, 24.0)):
        assert np.array_equal(bits(got[p]), bits(want)), p


def test_without_an_index_entry_e_reads_element_e(amd, case):
    """pass 1 with index_dev NULL on rows that are already in summation order"""
    from lisflood_amd import zonal as ZN
    x = case[0]
    plan = ZN.ZonePlan(np.repeat([0, 2], [300, 77]), np.arange(377), 3)
    assert np.array_equal(plan.positions, np.arange(377))
    from lisflood_amd._lib import DeviceArray
    host = np.full((2, 400), SENTINEL)
    host[:, :377] = x[:2, :377]
    d_rows, d_start = DeviceArray.from_host(host.reshape(-1)), DeviceArray.from_host(plan.run_start[0])
    d_out = DeviceArray.from_host(np.full(2 * 4, SENTINEL))
    amd.check(amd.lib().lf_members_zonal_device(0, d_rows.ptr, 2, 400, 1.0, 377, None, None, 4, d_start.ptr, d_out.ptr, 4))
    got = d_out.download().reshape(2, 4)
    want = MZ.zonal_sums(x[:2], np.arange(377), plan.run_start, passes=1)
    assert plan.runs(0) == 4 and np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got[:, 2]), bits(np.zeros(2)))
    for d in (d_rows, d_start, d_out):
        d.free()
