"""-m gpu: the soil columns and the land surface of an ensemble in ONE launch (lf_soil_columns_members_device,
lf_land_columns_members_device; csrc/lf_soil.hip: k_soil_fused<.., MEMBERS>, k_soil_stragglers<.., MEMBERS>) against the
single calls on each member alone.  Everything is compared bit for bit, NaN equal to NaN (module_edges.same_bits); there is
no tolerance anywhere in this file.

  soil form   the inputs of tests/soil_edges.py as member 0, members 1 and 2 a seeded perturbation of its state and forcing
              that keeps every water content inside [WRes, WS]: the pow-free family (N = 300: two tiles per row, the second
              ragged, paddy rows included) and the planted sub-step counts (63 tiles per member, so with 3 members a straggler
              group of 16 tiles spans a member boundary), under LF_SOIL_NO_DERIVED / LF_SOIL_TRIP_CAP / LF_GENERAL_POW
  land form   synthetic.hotpath_scenario(70, 90), 3 members forced by hotpath_forcing(N, s + 10 m), four model steps
  strides, NULL diagnostics, isolation of the members, members = 1, LF_LAND_MEMBERS=0

The preconditions on the members' own single calls (some column goes to the straggler kernel, some multi-sub-step column
stays in its tile) are asserted on the sub-step family, whose counts are planted: the pow-free family takes one sub-step per
column by construction (that is what makes it pow-free), so its member 0 has no such column under any setting."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import module_edges as E
import soil_edges as S

pytestmark = pytest.mark.gpu

M = 3
ENV = ("LF_SOIL_NO_DERIVED", "LF_SOIL_TRIP_CAP", "LF_GENERAL_POW", "LF_LAND_MEMBERS")
SETTINGS = {
    "default": {},
    "streamed": {"LF_SOIL_NO_DERIVED": "1"},
    "trip_cap_0": {"LF_SOIL_TRIP_CAP": "0"},
    "trip_cap_1": {"LF_SOIL_TRIP_CAP": "1"},
    "streamed_trip_cap_1": {"LF_SOIL_NO_DERIVED": "1", "LF_SOIL_TRIP_CAP": "1"},
    "general_pow": {"LF_GENERAL_POW": "1"},
}
DEFAULT_TRIP_CAP = 6               # kSoilTripCap


@contextlib.contextmanager
def environment(setting):
    """the switches of ENV as `setting` says, everything else of them unset; restored afterwards"""
    before = {k: os.environ.get(k) for k in ENV}
    for k in ENV:
        os.environ.pop(k, None)
    os.environ.update(setting)
    try:
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def same(got, want, what):
    assert E.same_bits(got, want), "%s: %s" % (what, E.first_difference(got, want))


# ======================================================================================================================
# soil form
# ======================================================================================================================
def _perturbed(d, m, family, active):
    """member m >= 1 of the soil families: a seeded perturbation of member 0's state and forcing.  Every water content ends
    inside [WRes, WS] of its layer; columns the reference skips (active False) keep what member 0 has there."""
    rng = np.random.default_rng(1000 + m)
    lu = d["index_landuse_all"]
    V, N = d["W1a"].shape
    p = S.clone(d)
    if family == "substeps":
        # layers 1a / 1b a little above WRes (their conductivity stays ~1e-3 of layer 2's, which stays saturated: the planted
        # sub-step counts are those of member 0), other frozen pixels, rain, evaporation and interception
        for l in ("1a", "1b"):
            p["W" + l] = d["WRes" + l][lu] + 8.0 * rng.random((V, N))
        p["isFrozenSoil"] = np.roll(d["isFrozenSoil"], m)
        p["Rain"] = rng.uniform(0, 4, N) * (rng.random(N) < 0.5)
    else:
        for l in S.LAYERS:
            wres, ws = d["WRes" + l][lu], d["WS" + l][lu]
            p["W" + l] = wres + (ws - wres) * rng.random((V, N))
        p["isFrozenSoil"] = rng.random(N) < 0.15
        p["Rain"] = d["Rain"] * rng.choice([0.0, 0.5, 1.0, 1.5], N) + rng.uniform(0, 1, N) * (rng.random(N) < 0.3)
    p["W1"] = p["W1a"] + p["W1b"]
    p["SnowMelt"] = rng.uniform(0, 1, N) * (rng.random(N) < 0.3)
    p["UZ"] = d["UZ"] * rng.uniform(0.5, 1.5, (V, N))
    p["DSLR"] = d["DSLR"] + rng.integers(0, 4, (V, N))
    p["LeafDrainage"] = rng.uniform(0, 0.5, (V, N))
    p["Interception"] = rng.uniform(0, 0.25, (V, N))
    p["ESMax"] = rng.uniform(0, 2, (V, N)) * (rng.random((V, N)) < 0.7)
    for k in S.STATE:
        p[k] = np.where(active, p[k], d[k])
    for l in S.LAYERS:                                   # the precondition of the perturbation itself
        w, wres, ws = p["W" + l], d["WRes" + l][lu], d["WS" + l][lu]
        assert ((w >= wres) & (w <= ws))[active].all(), l
    return p


def _soil_family(name):
    if name == "substeps":
        d, counts, frozen = S.substep_inputs()
        active = np.ones(d["W1a"].shape, bool)
    else:
        d = S.powfree_case(**S.POWFREE_SETS[name]["kw"])[0]
        d.pop("powfree_drawn", None)
        counts, active = None, S.powfree_active(d)
    members = [d] + [_perturbed(d, m, name, active) for m in range(1, M)]
    for a in range(M):
        for b in range(a + 1, M):                        # no two members are equal
            for k in S.STATE + S.V_IN + ["Rain", "SnowMelt", "isFrozenSoil"]:
                if name == "substeps" and k == "W2":     # (stays saturated there: it plants the counts)
                    continue
                assert not np.array_equal(members[a][k], members[b][k]), (name, a, b, k)
    return dict(name=name, members=members, counts=counts, active=active)


@pytest.fixture(scope="module")
def soil_families():
    return {name: _soil_family(name) for name in list(S.POWFREE_SETS) + ["substeps"]}


def _stack(members, k):
    return np.stack([np.asarray(m[k]) for m in members])


def _single_soil(amd, d):
    """the member's own single call -> (the 22 written arrays, histogram, deferred count)"""
    from lisflood_amd import soilloop
    dev = soilloop.SoilColumnsDevice(d)
    assert dev.derived
    dev.step()
    out = {k: dev.get(k) for k in S.WRITTEN}
    hist = dev.substep_histogram()
    nd = C.c_int64(0)
    amd.check(amd.lib().lf_soil_last_deferred(0, C.byref(nd)))
    assert amd.lib().lf_soil_last_form(0) == 1
    for a in dev.dev.values():
        a.free()
    return out, hist, nd.value


def _ensemble_soil(members, pad=0):
    from lisflood_amd import soilloop
    d = dict(members[0])
    for k in soilloop._V_IN + soilloop._V_IO + soilloop._SOIL_FORCING:
        d[k] = _stack(members, k)
    ens = soilloop.SoilColumnsEnsemble(d, M, pad=pad)
    assert ens.derived and ens.forcing_member_stride() == ens.fstride
    return ens


def _substep_preconditions(family, setting, hists):
    """each member's own single call sends a column to the straggler kernel and keeps a multi-sub-step column in its tile,
    from its histogram and LF_SOIL_TRIP_CAP"""
    cap = int(SETTINGS[setting].get("LF_SOIL_TRIP_CAP", DEFAULT_TRIP_CAP))
    counts = family["counts"]
    for m, hist in enumerate(hists):
        live = ~np.asarray(family["members"][m]["isFrozenSoil"], bool)
        want = S.trip_histogram(counts[:, live])         # (the engine lists no frozen column and no one-sub-step column)
        want[:2] = 0
        assert np.array_equal(hist, want), (m, np.nonzero(hist != want)[0])    # the perturbation kept the planted counts
        if cap > 0:
            assert hist[cap + 1:].sum() > 0, (m, "no straggler")
        if cap != 1:
            assert hist[2:(cap + 1 if cap else None)].sum() > 0, (m, "nothing stays in the tile")
        else:
            # cap 1: every multi-sub-step column is a straggler while its tile has records left (48); tile 4 of row 0 holds
            # 256 such columns (soil_edges.substep_layout, no frozen pixel there), so 208 of them stay in the tile
            t4 = counts[0, 4 * S.TILE:5 * S.TILE][live[4 * S.TILE:5 * S.TILE]]
            assert (t4 > 1).sum() > 48, m


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", list(S.POWFREE_SETS) + ["substeps"])
def test_soil_members_equal_their_single_calls(amd, soil_families, name, setting):
    family = soil_families[name]
    members, active = family["members"], family["active"]
    with environment(SETTINGS[setting]):
        singles = [_single_soil(amd, S.clone(d)) for d in members]
        if name == "substeps":
            _substep_preconditions(family, setting, [h for _, h, _ in singles])
        ens = _ensemble_soil(members)
        ens.step()
        assert ens.last_form() == 2
        hist, deferred = ens.substep_histogram(), ens.last_deferred()
        for k in S.WRITTEN:
            got = ens.get(k)
            assert got.shape == (M,) + active.shape
            for m in range(M):
                same(got[m], singles[m][0][k], "%s %s member %d %s" % (name, setting, m, k))
                if name.startswith("paddy"):
                    assert (got[m][~active] == S.SENTINEL).all(), (name, setting, m, k)
        ens.free()
    assert np.array_equal(hist, sum(h for _, h, _ in singles)), (name, setting)
    assert deferred == sum(n for _, _, n in singles) and deferred == hist.sum(), (name, setting)
    if name.startswith("paddy"):
        assert (~active).any()


# ======================================================================================================================
# land form
# ======================================================================================================================
H, W = 70, 90                      # 6 300 pixels: 25 tiles per row, the last ragged
STEPS = 4


@pytest.fixture(scope="module")
def land():
    from lisflood_amd import soilloop as SL
    from lisflood_amd import synthetic as syn
    values, sc, _mask, _to_chan, _kin = syn.hotpath_scenario(H, W)
    d = dict(values, **sc)
    N = H * W
    forcing = [[syn.hotpath_forcing(N, s + 10 * m) for m in range(M)] for s in range(STEPS)]
    for a in range(M):
        for b in range(a + 1, M):
            assert not any(np.array_equal(forcing[0][a][k], forcing[0][b][k]) for k in ("Rain", "EWRef", "ETRef", "ESRef"))
    return dict(d=d, N=N, forcing=forcing, names=list(dict.fromkeys(SL._CANOPY_IO + SL._V_IO)))


def _member_forcing(forcing_of_step):
    return {k: np.stack([f[k] for f in forcing_of_step]) for k in forcing_of_step[0]}


def _single_land_step(amd, one, forcing):
    """lf_land_columns_device itself on the blocks of a one-member object"""
    for k, x in forcing.items():
        one.set(k, x)
    amd.check(amd.lib().lf_land_columns_device(0, C.byref(one.canopy), C.byref(one.soil), one.dev["ESRef"].ptr,
                                               1 if one.derived else 0))


def _land_single_runs(amd, land, start=None, forcing=None, steps=STEPS):
    """every member alone through lf_land_columns_device -> out[step][name] = [M,V,N], and the histogram / deferred sums of
    the last step"""
    from lisflood_amd import soilloop as SL
    out = [{k: [None] * M for k in land["names"]} for _ in range(steps)]
    hist, deferred = 0, 0
    for m in range(M):
        d = dict(land["d"])
        for k, x in (start or {}).items():
            d[k] = x[m]
        one = SL.LandSurfaceEnsemble(d, 1)
        for s in range(steps):
            _single_land_step(amd, one, forcing[s] if forcing else land["forcing"][s][m])
            assert one.last_form() == 1
            for k in land["names"]:
                out[s][k][m] = one.get(k)[0]
        hist, deferred = hist + one.substep_histogram(), deferred + one.last_deferred()
        one.free()
    return [{k: np.stack(v) for k, v in step.items()} for step in out], hist, deferred


def _land_ensemble_run(land, steps=STEPS, pad=0, start=None, forcing=None, before_step=None):
    from lisflood_amd import soilloop as SL
    d = dict(land["d"], **(start or {}))
    ens = SL.LandSurfaceEnsemble(d, M, pad=pad)
    if before_step:
        before_step(ens)
    out = []
    for s in range(steps):
        ens.step(forcing[s] if forcing else _member_forcing(land["forcing"][s]))
        out.append({k: ens.get(k) for k in land["names"] if k in ens.dev})
    return ens, out


@pytest.fixture(scope="module")
def land_default(amd, land):
    """the single calls and the member call under the default settings, shared by the tests below"""
    with environment({}):
        singles, hist, deferred = _land_single_runs(amd, land)
        ens, out = _land_ensemble_run(land)
        form, ehist, edeferred = ens.last_form(), ens.substep_histogram(), ens.last_deferred()
        ens.free()
    return dict(singles=singles, hist=hist, deferred=deferred, out=out, form=form, ehist=ehist, edeferred=edeferred)


LAND_SETTINGS = {"fast_pow": {}, "general_pow": {"LF_GENERAL_POW": "1"}, "fast_pow_trip_cap_1": {"LF_SOIL_TRIP_CAP": "1"},
                 "general_pow_trip_cap_1": {"LF_GENERAL_POW": "1", "LF_SOIL_TRIP_CAP": "1"}}


@pytest.mark.parametrize("setting", list(LAND_SETTINGS))
def test_land_members_equal_their_single_calls_step_by_step(amd, land, land_default, setting):
    if setting == "fast_pow":
        singles, hist, deferred = (land_default[k] for k in ("singles", "hist", "deferred"))
        out, form, ehist, edeferred = (land_default[k] for k in ("out", "form", "ehist", "edeferred"))
    else:
        with environment(LAND_SETTINGS[setting]):
            singles, hist, deferred = _land_single_runs(amd, land)
            ens, out = _land_ensemble_run(land)
            form, ehist, edeferred = ens.last_form(), ens.substep_histogram(), ens.last_deferred()
            ens.free()
    assert form == 2
    for s in range(STEPS):
        for k in land["names"]:
            for m in range(M):
                same(out[s][k][m], singles[s][k][m], "%s step %d member %d %s" % (setting, s, m, k))
    assert deferred > 0 and np.array_equal(ehist, hist) and edeferred == deferred
    assert not np.array_equal(out[-1]["W1a"][0], out[-1]["W1a"][1])       # the members did go different ways


def _different_starts(land):
    """[M,V,N] starts that differ between the members (for runs in which the forcing does not)"""
    d = land["d"]
    f = (1 + 0.1 * np.arange(M))[:, None, None]
    return dict(UZ=d["UZ"][None] * f, CumInterception=d["CumInterception"][None] + 0.1 * (f - 1), DSLR=d["DSLR"][None] + (f - 1) * 10)


@pytest.mark.parametrize("forcing_kind", ["per_member", "shared"])
def test_strides_with_sentinels_in_the_gaps(amd, land, forcing_kind):
    steps, pad = 2, 5
    start = _different_starts(land)
    shared = [land["forcing"][s][0] for s in range(steps)] if forcing_kind == "shared" else None
    planted = []

    def plant(ens):
        ens.set_gaps(S.SENTINEL)
        planted.append(ens)
    with environment({}):
        singles, _, _ = _land_single_runs(amd, land, start=start, forcing=shared, steps=steps)
        ens, out = _land_ensemble_run(land, steps=steps, pad=pad, start=start, forcing=shared, before_step=plant)
        assert ens.last_form() == 2 and ens.stride == 3 * land["N"] + pad and ens.fstride == land["N"] + pad
        assert ens.forcing_member_stride() == (0 if shared else ens.fstride)
        from lisflood_amd import soilloop as SL
        for k in ens._member + ens._forcing:
            gap = ens.gaps(k)
            assert gap.shape == (M, pad)
            assert (gap == (SL.GAP_BYTE if gap.dtype == np.uint8 else S.SENTINEL)).all(), k
        ens.free()
    for s in range(steps):
        for k in land["names"]:
            for m in range(M):
                same(out[s][k][m], singles[s][k][m], "%s step %d member %d %s" % (forcing_kind, s, m, k))
    assert not np.array_equal(out[-1]["UZ"][0], out[-1]["UZ"][1])


DIAGNOSTICS = "Theta1a Theta1b Theta2 Sat1a Sat1b Sat1 Sat2".split()


def test_null_diagnostics_change_nothing_else(amd, land, land_default):
    def drop(ens):
        for k in DIAGNOSTICS:
            setattr(ens.soil, k, None)
            ens.set(k, np.full((3, land["N"]), S.SENTINEL))
    with environment({}):
        ens, out = _land_ensemble_run(land, before_step=drop)
        assert ens.last_form() == 2
        ens.free()
    for s in range(STEPS):
        for k in land["names"]:
            if k in DIAGNOSTICS:
                assert (out[s][k] == S.SENTINEL).all(), (s, k)        # not reported: not written, for any member
            else:
                same(out[s][k], land_default["out"][s][k], "step %d %s" % (s, k))


def test_a_member_does_not_reach_its_neighbours(amd, land, land_default):
    w2 = np.repeat(land["d"]["W2"][None], M, axis=0)
    lu_ws2, lu_wres2 = land["d"]["WS2"], land["d"]["WRes2"]
    w2[1] = lu_wres2 + 0.5 * (w2[1] - lu_wres2)                            # member 1 starts drier in layer 2
    assert not np.array_equal(w2[1], w2[0]) and (w2[1] <= lu_ws2).all()
    with environment({}):
        ens, out = _land_ensemble_run(land, steps=2, start=dict(W2=w2))
        ens.free()
    for s in range(2):
        for k in land["names"]:
            for m in (0, 2):
                same(out[s][k][m], land_default["out"][s][k][m], "step %d member %d %s" % (s, m, k))
    assert not np.array_equal(out[1]["W2"][1], land_default["out"][1]["W2"][1])


def test_one_member_is_the_single_call_and_the_fallback_gives_the_same_bits(amd, land, land_default):
    from lisflood_amd import soilloop as SL
    with environment({}):
        one = SL.LandSurfaceEnsemble(land["d"], 1)
        one.step(land["forcing"][0][0])
        assert one.last_form() == 1
        for k in land["names"]:
            same(one.get(k)[0], land_default["singles"][0][k][0], "members = 1, %s" % k)
        one.free()
    with environment({"LF_LAND_MEMBERS": "0"}):
        ens, out = _land_ensemble_run(land)
        assert ens.last_form() == 3
        hist, deferred = ens.substep_histogram(), ens.last_deferred()
        ens.free()
    for s in range(STEPS):
        for k in land["names"]:
            same(out[s][k], land_default["out"][s][k], "member after member, step %d %s" % (s, k))
    assert np.array_equal(hist, land_default["ehist"]) and deferred == land_default["edeferred"]
