"""HotPathEnsemble.transform() and resample(): the analysis step on the device against the host route it replaces.  Two
identical ensembles of three members (the scenario of test_hotpath_products_gpu.py: padded member rows with a sentinel
planted between them, a compact channel domain, once with lakes, reservoirs and inflow in the loop) run two steps; A calls
transform(), B brings every vector of analysis_names() to the host, applies the restatement (members_transform.py) and
uploads it again; both step once more.  Every state vector, every site row and ChanQAvg have the same bits after the call
and after the step behind it, the elements between the rows keep theirs, a tracker begun before the call holds the same
accumulators.  Then the same with resample([2, 0, 0]), after which, under shared forcing, members 1 and 2 stay identical."""
import numpy as np
import pytest

import hotpath_members as HM
import members_transform as MX

pytestmark = pytest.mark.gpu

H, W, M, PAD = 70, 90, 3, 5
N = H * W
SEED = 23                  # of structures_scenario(n_lakes=3, n_res=5), as tests/test_hotpath_products_gpu.py draws it
OUTPUTS = ["DirectRunoff", "ToChanM3RunoffDt", "FlowVelocity"]


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def cp(d):
    return {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}


def make(with_structures, members=M, shape=(H, W)):
    from lisflood_amd import synthetic as syn
    from lisflood_amd.hotpath import HotPathEnsemble
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(*shape)
    st = None
    if with_structures:
        st, ldd_kin = syn.structures_scenario(ldd_kin, shape, values["ChanQ"], sc["DtRouting"], n_lakes=3, n_res=5, seed=SEED)
    ens = HotPathEnsemble(cp(values), sc, mask, ldd_to_chan, ldd_kin, members=members, structures=cp(st) if st else None, pad=PAD)
    ens.set_gaps(HM.SENTINEL)
    return ens, st


def step(ens, st, s, shared=False):
    """a step with every member's own forcing (or one for all); the inflow hydrograph is the same for all members"""
    from lisflood_amd import synthetic as syn
    n = ens.N
    f = [syn.hotpath_forcing(n, s + 10 * m) for m in range(ens.members)]
    forcing = f[0] if shared else {k: np.stack([x[k] for x in f]) for k in f[0]}
    ens.step(forcing, time_since_start=s + 1, QInM3=st["QInM3Old"] * (1.0 + 0.1 * s) if st else None)


def is_site(name):
    from lisflood_amd import routing as RT
    return name in RT._LAKE_STATE + RT._RES_STATE


def fetch(ens, name):
    return ens.download_site(name) if is_site(name) or name == "TransCum" else ens.download(name)


def put(ens, name, rows):
    if is_site(name):
        ens._set_channel_rows(name, rows)
    elif name == "TransCum":
        ens._set_channel_rows(name, rows[:, ens.gpix])
    else:
        ens.set_member_state(name, rows)


def site_pixels(st, name):
    """the land pixel of every lake or reservoir from the scenario itself: its raster is all land, so the site lists of
    synthetic.structures_scenario ARE land pixels, in the order of the site rows (not from the object under test, which
    renumbers them into its channel domain)"""
    from lisflood_amd import routing as RT
    return np.asarray(st["LakeIndex" if name in RT._LAKE_STATE else "ReservoirIndex"], np.int64)


def host_transform(ens, weights, taper, bounds, st=None, names=None):
    """the route transform() replaces: download, the restatement, upload -- once per vector"""
    for name in names or ens.analysis_names():
        x = fetch(ens, name)
        pick = (lambda b: np.asarray(b)[..., site_pixels(st, name)]) if is_site(name) else (lambda b: np.asarray(b))
        spread = lambda b, inf: inf if b is None else b if np.ndim(b) == 0 else np.broadcast_to(pick(b), x.shape[1:]).reshape(-1)
        lower, upper = bounds.get(name, (None, None))
        flat = x.reshape(x.shape[0], -1)
        new = MX.transform(flat, weights, np.broadcast_to(pick(taper), x.shape[1:]).reshape(-1), spread(lower, -np.inf),
                           spread(upper, np.inf))
        put(ens, name, new.reshape(x.shape))


def host_resample(ens, parents):
    for name in ens.analysis_names():
        put(ens, name, MX.resample(fetch(ens, name), parents))


def state_of(ens, outputs=False):
    out = {k: fetch(ens, k) for k in ens.analysis_names() + (OUTPUTS if outputs else [])}
    out["ChanQAvg"] = ens.chan_q_avg()
    return out


def gaps_of(ens):
    return {k: ens.gaps(k) for k in ens.gap_names()}


def assert_same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert a[k].shape == b[k].shape, (what, k)
        bad = np.argwhere(MX.bits(a[k]) != MX.bits(b[k]))                # the raw bits, those of a NaN included
        assert bad.size == 0, (what, k, len(bad), bad[:3], a[k][tuple(bad[0])], b[k][tuple(bad[0])])


def analysis_inputs(ens):
    """a convex update (weights not negative, columns summing to 1: every member stays inside the members' range, the state
    stays physical), a taper with 0 and 1 planted, and bounds of every kind, some of which bite"""
    rng = np.random.default_rng(77)
    weights = 0.7 * np.eye(M) + 0.3 * rng.dirichlet(np.ones(M), M).T
    taper = rng.uniform(0.0, 1.0, N)
    taper[::7], taper[3::11] = 0.0, 1.0
    uz = ens.download("UZ")
    bounds = {"W1a": (0.0, None), "ChanM3Kin": (0.0, None), "CumInterception": (0.0, 1e9),
              "UZ": (None, 0.9 * uz.min(axis=0) + 1e-3), "LZ": (ens.download("LZ").mean(axis=0), None),
              "ChanQ": (None, float(np.median(ens.download("ChanQ").max(axis=0)[ens.ids])))}
    if "LakeStorageM3CC" in ens.analysis_names():
        bounds["LakeStorageM3CC"] = (np.zeros(N), None)
        bounds["ReservoirFillCC"] = (None, np.full(N, 0.5))
    return weights, taper, bounds


@pytest.mark.parametrize("with_structures", [False, True], ids=["plain", "structures"])
def test_the_device_route_is_the_host_route(amd, with_structures):
    (A, st), (B, _) = make(with_structures), make(with_structures)
    assert A.Nk < A.N and A.kstride > A.Nk and A.pstride > A.N and A._outside.size
    names = A.analysis_names()
    assert set(A.state_names()) <= set(names) and {"W1a", "UZ", "LZ", "ChanQ", "ChanM3Kin", "sumDisDay"} <= set(names)
    assert ("LakeStorageM3CC" in names and "ReservoirStorageM3CC" in names and "TransCum" in names) == with_structures
    assert not set(names) & {"Rain", "QInM3Old", "QDelta", "DirectRunoff", "ToChanM3RunoffDt"}
    step(A, st, 0)
    step(B, st, 0)
    thr = np.median(A.chan_q_avg(), axis=0)
    for ens in (A, B):                                                # a tracker begun before the call
        ens.track_begin("ChanQAvg", thresholds=thr)
    step(A, st, 1)
    step(B, st, 1)
    assert_same(state_of(A), state_of(B), "before")
    weights, taper, bounds = analysis_inputs(A)
    gaps, done = gaps_of(A), A.steps_done
    before = state_of(A)
    # ---- transform -----------------------------------------------------------------------------------------------------------
    A.transform(weights, taper=taper, bounds=bounds)
    host_transform(B, weights, taper, bounds, st)
    after = state_of(A)
    assert_same(after, state_of(B), "after transform")
    assert_same(gaps_of(A), gaps, "gaps after transform")
    assert A.steps_done == done
    if with_structures:                                              # (the scenario's site lists are what the object was given)
        assert np.array_equal(A.ids[np.asarray(A.rmod.var.LakeIndex)], site_pixels(st, "LakeStorageM3CC"))
    moved = [k for k in names if not MX.same(before[k], after[k])]
    assert {"W1a", "LZ", "ChanQ"} <= set(moved), moved
    assert (after["UZ"] <= bounds["UZ"][1]).all() and (after["LZ"] >= bounds["LZ"][0]).all()
    assert (after["ChanQ"] <= bounds["ChanQ"][1]).all() and not (before["ChanQ"] <= bounds["ChanQ"][1]).all()
    assert (taper == 0).sum() > N // 10 and (taper == 1).sum() > N // 20
    assert np.array_equal(after["W1a"][..., taper == 0], before["W1a"][..., taper == 0])      # taper 0: the member's own value
    if with_structures:
        assert any(is_site(k) for k in moved) and (after["ReservoirFillCC"] <= 0.5).all()
    step(A, st, 2)
    step(B, st, 2)
    assert_same(state_of(A, True), state_of(B, True), "the step after transform")
    assert_same(gaps_of(A), gaps, "gaps after the step")
    for key in ("peak", "peak_step", "sum", "first_above", "steps_above"):
        a, b = A.download("ChanQAvg." + key), B.download("ChanQAvg." + key)
        assert a.dtype == b.dtype and np.array_equal(a, b) and A.track_steps("ChanQAvg") == 2, key
    # the same call again on the same arrays: nothing goes to the device twice
    on_device = lambda: [(key, hit[1].ptr.value) for key, hit in A._analysis_cache.items()] + [A._weights[1].ptr.value]
    held = on_device()
    assert A._weights[0] is weights
    A.transform(weights, taper=taper, bounds=bounds)
    host_transform(B, weights, taper, bounds, st)
    assert on_device() == held and A._weights[0] is weights
    assert_same(state_of(A), state_of(B), "after a second transform")
    # ---- resample ------------------------------------------------------------------------------------------------------------
    parents = [2, 0, 0]
    before = state_of(A)
    A.resample(parents)
    host_resample(B, parents)
    after = state_of(A)
    assert_same(after, state_of(B), "after resample")
    for k in names:
        assert np.array_equal(MX.bits(after[k]), MX.bits(before[k][parents])), k
    assert_same(gaps_of(A), gaps, "gaps after resample")
    step(A, st, 3, shared=True)
    step(B, st, 3, shared=True)
    final = state_of(A, True)
    assert_same(final, state_of(B, True), "the step after resample")
    for k, a in final.items():                                       # shared forcing: members 1 and 2 are one particle twice
        assert np.array_equal(MX.bits(a[1]), MX.bits(a[2])), k
    assert not np.array_equal(final["W1a"][0], final["W1a"][1]) and not np.array_equal(final["ChanQ"][0], final["ChanQ"][1])
    # a subset of the names: the others keep their bits
    before = state_of(A)
    A.resample(np.array([1, 1, 0]), names=["LZ", "ChanQ"])
    after = state_of(A)
    for k in names:
        want = before[k][[1, 1, 0]] if k in ("LZ", "ChanQ") else before[k]
        assert np.array_equal(MX.bits(after[k]), MX.bits(want)), k
    A.free(); B.free()


def test_the_refusals(amd):
    ens, _ = make(False, shape=(24, 30))
    n = ens.N
    good = np.eye(M)
    refused = [
        (lambda: ens.transform(np.eye(M + 1)), "weights must be"),
        (lambda: ens.transform(np.eye(M, dtype=np.float32)), "weights must be"),
        (lambda: ens.transform(good.tolist()), "weights must be"),
        (lambda: ens.transform(good, names=["NoSuchVector"]), "no state vector"),
        (lambda: ens.transform(good, names=["DirectRunoff"]), "no state vector"),
        (lambda: ens.transform(good, names=["Rain"]), "no state vector"),
        (lambda: ens.transform(good, names=["LZ", "LZ"]), "twice"),
        (lambda: ens.transform(good, taper=np.ones(n - 1)), "taper must be"),
        (lambda: ens.transform(good, taper=np.ones((M, n))), "taper must be"),
        (lambda: ens.transform(good, names=["LZ"], bounds={"UZ": (0.0, None)}), "not among the names"),
        (lambda: ens.transform(good, bounds={"NoSuchVector": (0.0, None)}), "not among the names"),
        (lambda: ens.transform(good, bounds={"LZ": (np.zeros((3, n)), None)}), "a bound of LZ"),
        (lambda: ens.transform(good, bounds={"UZ": (None, np.zeros(n + 1))}), "a bound of UZ"),
        (lambda: ens.transform(good, bounds={"UZ": 0.0}), "must be \\(lower, upper\\)"),
        (lambda: ens.transform(good, bounds={"UZ": (2.0, 1.0)}), "greater than upper"),
        (lambda: ens.resample([0, 1]), "parents must be"),
        (lambda: ens.resample([0, 1, 3]), "parents must be"),
        (lambda: ens.resample([0, -1, 2]), "parents must be"),
        (lambda: ens.resample([0.0, 1.0, 2.0]), "parents must be"),
        (lambda: ens.resample([0, 1, 2], names=["ChanQAvg"]), "no state vector"),
    ]
    before = {k: ens.download(k) for k in ens.analysis_names()}
    for call, word in refused:
        with pytest.raises(ValueError, match=word):
            call()
    assert ens._weights is None and ens._analysis_cache == {}          # refused before anything went to the device
    ens.transform(good, names=["UZ"], bounds={"UZ": (np.zeros((3, n)), None)})      # (a [3, N] bound of a [3, N] vector is fine)
    after = {k: ens.download(k) for k in ens.analysis_names()}
    for k in before:
        assert MX.same(before[k], after[k]), k
    ens.free()
    many, _ = make(False, members=65, shape=(24, 30))
    with pytest.raises(ValueError, match="at most 64 members"):
        many.transform(np.eye(65))
    many.resample(np.roll(np.arange(65), 1), names=["LZ"])           # (resample takes up to 128)
    many.free()


def test_rows_of_the_call_in_hand_outlive_the_cache_limit(amd):
    """A fixed taper and bound arrays made anew every cycle, as an assimilation driver does: the row cache fills, rows of
    earlier cycles make room, and the taper row -- the oldest entry of all, used by every call -- must never be the one that
    goes while a call holds its address.  Then one call that needs more rows than the cache keeps.  Every call against
    the host route on a twin, on the raw bits."""
    (A, _), (B, _) = make(False, shape=(24, 30)), make(False, shape=(24, 30))
    n, limit = A.N, A._ROWS_CACHED
    rng = np.random.default_rng(5)
    weights = 0.7 * np.eye(M) + 0.3 * rng.dirichlet(np.ones(M), M).T
    taper = rng.uniform(0.0, 1.0, n)
    wide = [k for k in A.analysis_names() if k in A.land._member]
    assert len(wide) * 6 + 2 > limit
    step(A, None, 0)
    step(B, None, 0)
    seen, cycle = set(), 0
    while len(seen) <= 2 * limit:                                     # rows enough to fill the cache twice over
        bounds = {"LZ": (rng.uniform(0.0, 5.0, n), None), "ChanQ": (None, rng.uniform(50.0, 500.0, n))}
        for k in wide[cycle % 3:cycle % 3 + 2]:
            bounds[k] = (np.zeros((3, n)), rng.uniform(1e3, 1e4, (3, n)))
        A.transform(weights, taper=taper, bounds=bounds)
        host_transform(B, weights, taper, bounds)
        seen |= set(A._analysis_cache)
        assert len(A._analysis_cache) <= limit and A._analysis_pinned == set()
        assert any(key[0] == id(taper) for key in A._analysis_cache), cycle          # (used by every call: never the oldest)
        assert_same(state_of(A), state_of(B), ("cycle", cycle))
        cycle += 1
    assert cycle > 3
    bounds = {k: (np.full((3, n), -1e30), np.full((3, n), 1e30)) for k in wide}       # 6 rows per vector: more than the limit
    bounds[wide[0]] = (np.zeros((3, n)), np.full((3, n), 1e30))
    A.transform(weights, taper=taper, bounds=bounds)
    host_transform(B, weights, taper, bounds)
    assert len(A._analysis_cache) == len(wide) * 6 + 2 > limit        # nothing the call used was let go
    assert_same(state_of(A), state_of(B), "one call beyond the limit")
    A.transform(weights, names=["LZ"], taper=taper, bounds={"LZ": (np.zeros(n), None)})     # the next call brings it back down
    host_transform(B, weights, taper, {"LZ": (np.zeros(n), None)}, names=["LZ"])
    assert len(A._analysis_cache) <= limit
    step(A, None, 1)
    step(B, None, 1)
    assert_same(state_of(A, True), state_of(B, True), "the step behind it")
    A.free(); B.free()
