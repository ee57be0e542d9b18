"""HotPathEnsemble.zonal(): sums and means of member rows over zones against the restatement (members_zonal.py) on
download(name) with the plan zonal_plan() hands out, bit for bit.  Two identical ensembles of three members
(synthetic.hotpath_scenario(48, 60) with lakes, reservoirs and inflow in the loop, padded member rows with a sentinel
between them, a compact channel domain) run two steps with LZ tracked; A calls zonal() on LZ, Theta1aPixel, ChanQAvg, ChanQ
and LZ.peak over a label map (four quadrants with holes, an empty zone, a single-pixel zone) and over index lists (the
whole domain and two nested sub-areas), sums and means, with and without weights.  A channel row's zones hold their pixels
inside the channel domain; the single-pixel zone is sample() there; the same arrays reuse the device tables; the gaps and
steps_done stay; after the next step A has the bits of B, which never called zonal()."""
import numpy as np
import pytest

import members_zonal as MZ
from test_hotpath_transform_gpu import amd, assert_same, gaps_of, make, state_of, step  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPE = (48, 60)
NAMES = ["LZ", "Theta1aPixel", "ChanQAvg", "ChanQ", "LZ.peak"]
CHANNEL = {"ChanQAvg", "ChanQ"}
EMPTY, SINGLE = 4, 5


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def pair(amd):
    (A, st), (B, _) = (make(True, 3, SHAPE) for _ in range(2))
    for ens in (A, B):
        ens.track_begin("LZ")
        for s in (0, 1):
            step(ens, st, s)
    yield A, B, st
    A.free()
    B.free()


@pytest.fixture(scope="module")
def zones(pair):
    """(label map, index lists, weights, the pixel of the single-pixel zone)"""
    A = pair[0]
    H, W = SHAPE
    N = A.N
    rows, cols = np.nonzero(A.land_mask)
    rng = np.random.default_rng(8)
    labels = (2 * (rows >= H // 2) + (cols >= W // 2)).astype(np.int32)
    labels[rng.choice(N, N // 9, replace=False)] = -1
    labels[rng.choice(N, 5, replace=False)] = -3
    single = int(A.ids[A.ids.size // 2])                               # a pixel inside the channel domain
    labels[single] = SINGLE
    lists = [np.arange(N), np.flatnonzero(rows < 30), np.flatnonzero((rows < 30) & (cols < 17))]
    return labels, lists, rng.uniform(0.5, 2.0, N), single


def source(A, name):
    """([members, N] in pixel order, divisor): what zonal(name) sums, from download()"""
    if name == "ChanQAvg":
        return A.download("sumDisDay"), float(A.sc["NoRoutSteps"])
    return A.download(name), 1.0


def test_zonal_is_the_restatement_on_the_download(pair, zones):
    A = pair[0]
    labels, lists, w, single = zones
    N = A.N
    assert A.Nk < N and A.kstride > A.Nk and A.pstride > N
    gaps, done = gaps_of(A), A.steps_done
    inside = np.zeros(N, bool)
    inside[A.ids] = True
    for name in NAMES:
        x, divisor = source(A, name)
        assert x.shape == (3, N) and np.isfinite(x).all()
        for form, zs in (("labels", labels), ("lists", lists)):
            members_of = [np.flatnonzero(labels == z) for z in range(SINGLE + 1)] if form == "labels" else lists
            for weights in (None, w):
                plan = A.zonal_plan(zs, weights, name)
                assert plan.zones == len(members_of)
                for z, pix in enumerate(members_of):                     # the zone's pixels, each once, in the plan's own order
                    pix = pix[inside[pix]] if name in CHANNEL else pix
                    assert np.array_equal(np.sort(plan.pixels[plan.zone_of_entry == z]), np.sort(pix)), (name, form, z)
                want = MZ.zonal_sums(x, plan.pixels, plan.run_start, weights, divisor)
                wsum = MZ.weight_sums(plan.pixels, plan.run_start, weights)
                assert np.array_equal(bits(plan.weight_sum), bits(wsum))
                got = A.zonal(name, zs, weights, mean=False)
                assert got.shape == (3, plan.zones) and np.array_equal(bits(got), bits(want)), (name, form, weights is not None)
                mean = A.zonal(name, zs, weights)
                with np.errstate(all="ignore"):
                    assert np.array_equal(bits(mean), bits(want / wsum)), (name, form)
                assert np.allclose(got, (MZ.terms(x, np.arange(N), weights, divisor)[:, None, :] *
                                         np.array([np.isin(np.arange(N), p) for p in members_of])[None]).sum(axis=2), rtol=1e-12)
                if form == "labels":
                    assert np.array_equal(bits(got[:, EMPTY]), bits(np.zeros(3))) and np.isnan(mean[:, EMPTY]).all()
                    assert (got[:, :EMPTY] != 0.0).all() and np.isfinite(mean[:, [0, 1, 2, 3, SINGLE]]).all()
    assert_same(gaps_of(A), gaps, "gaps after zonal")
    assert A.steps_done == done


def test_the_single_pixel_zone_is_sample_there(pair, zones):
    A = pair[0]
    labels, _, w, single = zones
    at = np.array([single])
    for name in NAMES:
        got = A.zonal(name, labels, mean=False)[:, SINGLE]
        assert np.array_equal(got, A.sample(name, at)[:, 0]) and (name == "LZ.peak" or (got != 0.0).any()), name
        assert np.array_equal(A.zonal(name, labels)[:, SINGLE], got)                       # the mean over one pixel
    outside = np.setdiff1d(np.arange(A.N), A.ids)[:1]
    assert np.array_equal(bits(A.zonal("ChanQ", [outside], mean=False)), bits(np.zeros((3, 1))))       # as sample() gives 0.0


def test_the_same_arrays_reuse_the_device_tables(pair, zones):
    A = pair[0]
    labels, w = zones[0].copy(), zones[2].copy()                         # arrays of this test's own: the newest entries
    first = A.zonal("LZ", labels, w)
    key = (id(labels), id(w), False)
    t, keys = A._zonal[key], list(A._zonal)
    pointers = [d.ptr.value for d in t.arrays]
    assert t.plan.passes == 2 and len(t.partial) == 2 and t.index.shape == (t.plan.entries,) and all(pointers)
    A.zonal("Theta1aPixel", labels, w)
    A.zonal("LZ.peak", labels, w, mean=False)
    assert np.array_equal(bits(A.zonal("LZ", labels, w)), bits(first))
    assert list(A._zonal) == keys and A._zonal[key] is t and [d.ptr.value for d in t.arrays] == pointers
    A.zonal("ChanQ", labels, w)                                          # the other row kind: tables of its own
    other = A._zonal[(id(labels), id(w), True)]
    assert other is not t and other.plan.entries < t.plan.entries and A._zonal[key] is t
    copy = labels.copy()
    assert A.zonal_plan(copy, w, "LZ") is not t.plan and A._zonal[key] is t
    for _ in range(2 * A._CACHED):                                       # no more than _CACHED entries are kept
        A.zonal("LZ", labels.copy())
    assert len(A._zonal) == A._CACHED and key not in A._zonal
    with pytest.raises(ValueError, match="integer rows"):
        A.zonal("LZ.peak_step", labels)
    with pytest.raises(ValueError, match="weights must be"):
        A.zonal("LZ", labels, w[:-1])
    with pytest.raises(ValueError, match="label map"):
        A.zonal("LZ", labels[:-1])


def test_the_next_step_does_not_see_the_calls(pair):
    A, B, st = pair
    assert A._zonal and not B._zonal
    for ens in (A, B):
        step(ens, st, 2)
    assert_same(state_of(A, True), state_of(B, True), "the step after zonal()")
    assert_same(gaps_of(A), gaps_of(B), "gaps after the step")
    assert np.array_equal(bits(A.download("LZ.peak")), bits(B.download("LZ.peak")))
