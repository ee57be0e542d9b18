"""HotPathEnsemble.regress(): the localised serial analysis on the device against the host route.  Two identical ensembles
(synthetic.hotpath_scenario(48, 60) with lakes, reservoirs and inflow in the loop, padded member rows with a sentinel
between them, 3 and 5 members) run two steps; A calls regress() with the increments of 5 gauges of half-widths 4 to 12
pixels, B brings every vector of analysis_names() to the host, applies the restatement (members_regress.py) with the
pixel's row and column as coordinates and uploads it again; both step once more.  Every state vector, every site row and
ChanQAvg have the same bits after the call and after the step behind it; pixels beyond every gauge's reach keep theirs;
coords= given explicitly is the default; an ensemble that never calls regress(), stepped beside one that does, has the
bits of one that ran the same steps alone."""
import numpy as np
import pytest

import members_regress as MR
from test_hotpath_transform_gpu import amd, assert_same, fetch, gaps_of, is_site, make, put, site_pixels, state_of, step  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPE = (48, 60)
GAUGE_RC = np.array([[10.0, 12.0], [30.0, 40.0], [24.0, 25.0], [40.0, 8.0], [8.0, 50.0]])     # (row, column) of the 5 gauges
HALFWIDTH = np.array([4.0, 12.0, 6.5, 8.0, 5.0])


def increments_of(ens):
    """serial_increments() from the members' lower-zone storage at the gauges, as a cycle makes them: a gentle analysis
    (observations 2 % above the ensemble mean, error variance twice the spread), so that the state stays physical"""
    from lisflood_amd import assimilation as AS
    q = ens.download("LZ")                                                # [members, N] in pixel order
    rows, cols = np.nonzero(ens.land_mask)
    pix = [int(np.flatnonzero((rows == r) & (cols == c))[0]) for r, c in GAUGE_RC]
    hx = q[:, pix] + np.random.default_rng(4).standard_normal((ens.members, 5)) * 0.05 * (1.0 + np.abs(q[:, pix]))
    assert np.isfinite(hx).all()
    obs = hx.mean(axis=0) * 1.02 + 0.01
    return AS.serial_increments(hx, obs, 2.0 * hx.var(axis=0, ddof=1) + 1e-6, GAUGE_RC, HALFWIDTH)


def host_regress(ens, inc, bounds, st, names=None, coords=None):
    """the route regress() replaces: download, the restatement, upload -- once per vector"""
    rows, cols = np.nonzero(ens.land_mask)
    cx, cy = coords or (rows.astype(np.float64), cols.astype(np.float64))
    touched_by_name = {}
    for name in names or ens.analysis_names():
        x = fetch(ens, name)
        pick = (lambda b: np.asarray(b)[..., site_pixels(st, name)]) if is_site(name) else (lambda b: np.asarray(b))
        spread = lambda b, inf: inf if b is None else b if np.ndim(b) == 0 else np.broadcast_to(pick(b), x.shape[1:]).reshape(-1)
        lower, upper = bounds.get(name, (None, None))
        flat = x.reshape(x.shape[0], -1)
        ex, ey = (np.broadcast_to(pick(a), x.shape[1:]).reshape(-1) for a in (cx, cy))
        new, touched = MR.regress(flat, ex, ey, inc.table, inc.gauges, spread(lower, -np.inf), spread(upper, np.inf))
        touched_by_name[name] = touched.reshape(x.shape[1:])
        put(ens, name, new.reshape(x.shape))
    return touched_by_name


@pytest.mark.parametrize("members", [3, 5])
def test_the_device_route_is_the_host_route(amd, members):
    (A, st), (B, _), (C, _) = (make(True, members, SHAPE) for _ in range(3))
    N = A.N
    assert A.Nk < N and A.kstride > A.Nk and A.pstride > N and A.land_mask.shape == SHAPE
    names = A.analysis_names()
    assert {"W1a", "UZ", "LZ", "ChanQ", "LakeStorageM3CC", "ReservoirStorageM3CC", "TransCum"} <= set(names)
    for s in (0, 1):
        for ens in (A, B, C):
            step(ens, st, s)
    assert_same(state_of(A), state_of(B), "before")
    inc = increments_of(A)
    assert inc.gauges == 5 and inc.members == members
    bounds = {k: (0.0, None) for k in names}                               # no storage or flow goes below zero ...
    bounds.update({"LZ": (A.download("LZ").mean(axis=0), None), "ReservoirFillCC": (0.0, np.full(N, 0.5)),        # ... and rows
                   "ChanQ": (0.0, float(np.median(A.download("ChanQ").max(axis=0)[A.ids])))})
    gaps, done, before = gaps_of(A), A.steps_done, state_of(A)
    A.regress(inc, bounds=bounds)
    touched = host_regress(B, inc, bounds, st)
    after = state_of(A)
    assert_same(after, state_of(B), "after regress")
    assert_same(gaps_of(A), gaps, "gaps after regress")
    assert A.steps_done == done
    moved = [k for k in names if not np.array_equal(MR.bits(before[k]), MR.bits(after[k]))]
    assert {"W1a", "LZ", "ChanQ", "UZ"} <= set(moved), moved
    rows, cols = np.nonzero(A.land_mask)
    d2 = (rows[None, :] - GAUGE_RC[:, :1]) ** 2 + (cols[None, :] - GAUGE_RC[:, 1:]) ** 2          # (integers: exact)
    beyond = (d2 >= (2.0 * HALFWIDTH[:, None]) ** 2).all(axis=0)
    assert N // 10 < beyond.sum() < N - N // 10 and np.array_equal(~beyond, touched["UZ"][0])
    assert (MR.bits(after["W1a"][..., ~beyond]) != MR.bits(before["W1a"][..., ~beyond])).any()
    assert (after["LZ"] >= bounds["LZ"][0]).all() and (after["ChanQ"] <= bounds["ChanQ"][1]).all()
    assert (after["ReservoirFillCC"] <= 0.5).all() and any(is_site(k) for k in moved)
    # the table is resident and sized for a whole call; the coordinates went up once per row order
    table = A._regress_table.ptr.value
    assert A._regress_table.nbytes == 256 * (2 * members + 5) * 8
    held = set(A._analysis_cache)
    step(A, st, 2)
    step(B, st, 2)
    assert_same(state_of(A, True), state_of(B, True), "the step after regress")
    for k in ("W1a", "UZ", "LZ", "ChanQ", "ChanM3Kin"):                   # (a gentle analysis: the state it left is a state)
        assert np.isfinite(fetch(A, k)).all(), k
    assert_same(gaps_of(A), gaps, "gaps after the step")
    # coords= given explicitly, a subset of the names, no bounds: the default's bits; the other vectors keep theirs
    inc = increments_of(A)
    before = state_of(A)
    A.regress(inc, names=["LZ", "ChanQ", "LakeStorageM3CC"])
    assert A._regress_table.ptr.value == table and set(A._analysis_cache) == held      # nothing new on the device
    host_regress(B, inc, {}, st, names=["LZ", "ChanQ", "LakeStorageM3CC"])
    after = state_of(A)
    assert_same(after, state_of(B), "after a second regress")
    for k in names:
        assert k in ("LZ", "ChanQ", "LakeStorageM3CC") or np.array_equal(MR.bits(after[k]), MR.bits(before[k])), k
    for k in ("LZ", "ChanQ"):                                             # no bounds: beyond every gauge's reach nothing is stored
        assert np.array_equal(MR.bits(after[k][..., beyond]), MR.bits(before[k][..., beyond])), k
    assert (MR.bits(after["LZ"][..., ~beyond]) != MR.bits(before["LZ"][..., ~beyond])).any()
    A.regress(inc, names=["UZ"], coords=(rows.astype(np.float64), cols.astype(np.float64)))
    host_regress(B, inc, {}, st, names=["UZ"])
    assert_same(state_of(A), state_of(B), "with the coordinates given")
    # other coordinates are other distances: every pixel at the first gauge's place is reached whatever its own place
    here = (np.full(N, GAUGE_RC[0, 0]), np.full(N, GAUGE_RC[0, 1]))
    A.regress(inc, names=["UZ", "ReservoirFillCC"], coords=here)
    reached = host_regress(B, inc, {}, st, names=["UZ", "ReservoirFillCC"], coords=here)
    assert reached["UZ"].all() and reached["ReservoirFillCC"].all()
    assert_same(state_of(A), state_of(B), "with every pixel at the first gauge")
    A.free(); B.free()
    # an ensemble that never calls regress() is not touched by one that does: C, which stepped beside A and steps on after
    # A's calls, against a fourth that runs the same steps alone
    step(C, st, 2)
    D, _ = make(True, members, SHAPE)
    for s in (0, 1, 2):
        step(D, st, s)
    assert_same(state_of(C, True), state_of(D, True), "no regress")
    assert C._regress_table is None and C._regress_coords is None
    C.free(); D.free()


def test_the_refusals_and_more_gauges_than_a_call_takes(amd):
    from lisflood_amd import assimilation as AS
    (A, st), (B, _) = make(False, 3, (24, 30)), make(False, 3, (24, 30))
    n = A.N
    step(A, None, 0)
    step(B, None, 0)
    inc = increments_of_many(A, 5)
    refused = [
        (lambda: A.regress(inc, names=["NoSuchVector"]), "no state vector"),
        (lambda: A.regress(inc, names=["Rain"]), "no state vector"),
        (lambda: A.regress(inc, names=["LZ", "LZ"]), "twice"),
        (lambda: A.regress(inc, names=["LZ"], bounds={"UZ": (0.0, None)}), "not among the names"),
        (lambda: A.regress(inc, bounds={"UZ": (2.0, 1.0)}), "greater than upper"),
        (lambda: A.regress(inc, coords=(np.zeros(n), np.zeros(n - 1))), "coords must be"),
        (lambda: A.regress(inc.table), "serial_increments"),
        (lambda: A.regress(AS.serial_increments(np.eye(4)[:, :2], np.zeros(2), np.ones(2), np.zeros((2, 2)), 1.0)), "of 4 members"),
    ]
    before = state_of(A)
    for call, word in refused:
        with pytest.raises(ValueError, match=word):
            call()
    assert A._regress_table is None and A._analysis_cache == {}           # refused before anything went to the device
    nothing = AS.serial_increments(np.full((3, 2), 2.0), np.zeros(2), np.ones(2), np.zeros((2, 2)), 4.0)
    A.regress(nothing)                                                    # no gauge kept: nothing is launched
    assert_same(state_of(A), before, "no gauge kept")
    # 300 gauges: two calls per row set, in order -- the restatement with all 300 at once
    many = increments_of_many(A, 300)
    assert many.gauges == 300
    A.regress(many, names=["LZ", "UZ", "ChanQ"])
    host_regress(B, many, {}, None, names=["LZ", "UZ", "ChanQ"])
    assert_same(state_of(A), state_of(B), "300 gauges")
    assert A._regress_table.nbytes == 256 * (2 * 3 + 5) * 8
    A.free(); B.free()


def increments_of_many(ens, gauges):
    """gauges on a lattice over the raster with half-widths of 2 to 4.5 pixels, increments from seeded priors"""
    from lisflood_amd import assimilation as AS
    rng = np.random.default_rng(gauges)
    H, W = ens.land_mask.shape
    k = np.arange(gauges)
    xy = np.stack([(k * 7) % H, (k * 11) % W], axis=1).astype(np.float64)
    hx = rng.standard_normal((ens.members, gauges)) + 3.0
    return AS.serial_increments(hx, np.full(gauges, 3.0), np.full(gauges, 0.5), xy, 2.0 + (k % 6) * 0.5)
