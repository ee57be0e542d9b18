"""HotPathDevice(meteo=...) and HotPathEnsemble(meteo=...): the snow and frost kernel as the first launch of the resident
model step, precipitation and temperature as forcing.

  * every member of the ensemble is, bit for bit, a HotPathDevice(meteo=...) of its own over four steps -- both run the
    device's exp, so no tolerance anywhere -- on [N] meteo, [members, N] meteo and perturbed Tavg / Precipitation, once with
    structures=;
  * a HotPathDevice(meteo=...) against a plain HotPathDevice fed the Rain / SnowMelt / isFrozenSoil the numpy restatement
    makes on the host from the exact family (no snow cover: the frost line is exact), bit for bit: the wiring;
  * resample / transform / trackers / state files see SnowCoverS and FrostIndex;
  * without meteo= an object has the names it had before."""
import numpy as np
import pytest

import members_perturb as MP
import snow_frost as S
from module_edges import first_difference, same_bits

pytestmark = pytest.mark.gpu

H, W, M, STEPS, PAD, RANK = 48, 60, 3, 4, 5, 3
N = H * W
LAND = ("EWRef", "ETRef", "ESRef")


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def cp(d):
    return {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}


@pytest.fixture(scope="module")
def scenario():
    from lisflood_amd import synthetic as syn
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    assert int(np.asarray(mask).sum()) == N
    st, cut = syn.structures_scenario(ldd_kin, (H, W), values["ChanQ"], sc["DtRouting"], n_lakes=3, n_res=5, seed=24)
    return values, sc, mask, ldd_to_chan, ldd_kin, st, cut


@pytest.fixture(scope="module")
def family():
    return S.inputs(N, M, nan=False)


def meteo_of(x, member=None, **kw):
    m = dict({k: x[k] for k in S.STATICS}, **S.SCALARS, **kw)
    m["SnowCoverS"] = x["SnowCoverS"] if member is None else x["SnowCoverS"][member]
    m["FrostIndex"] = x["FrostIndex"] if member is None else x["FrostIndex"][member]
    return m


def build(scenario, cls, structures=False, **kw):
    values, sc, mask, ldd_to_chan, ldd_kin, st, cut = scenario
    return cls(cp(values), sc, mask, ldd_to_chan, cut if structures else ldd_kin, structures=cp(st) if structures else None, **kw)


def land_forcing(s):
    from lisflood_amd import synthetic as syn
    f = syn.hotpath_forcing(N, s)
    return {k: f[k] for k in LAND}


def inflow(scenario, m, s):
    return scenario[5]["QInM3Old"] * (1.0 + 0.1 * s + 0.05 * m)


def patterns():
    rng = np.random.default_rng(77)
    return rng.standard_normal((RANK, N)) * 0.5


def coefficients(s):
    return np.random.default_rng(900 + s).standard_normal((M, RANK)) * 0.5


def member_meteo(x, mode, m, s):
    """Precipitation and Tavg of member m at step s as the ensemble of `mode` sees them"""
    if mode == "one_row":
        return x["Precipitation"][s][0], x["Tavg"][s][0]
    if mode == "rows":
        return x["Precipitation"][s][m], x["Tavg"][s][m]
    # "perturbed": member 0's rows, Tavg + sum and Precipitation * (1 + sum) bounded below by 0, in the kernel's arithmetic
    P, c = patterns(), coefficients(s)
    prec = MP.perturb(None, c, P, x["Precipitation"][s][0], True, 0.0, np.inf)[m]
    tavg = MP.perturb(None, c, P, x["Tavg"][s][0], False, -np.inf, np.inf)[m]
    return prec, tavg


def snapshot(hp):
    out = {k: hp.download(k) for k in hp.state_names() + ["isFrozenSoil", "SnowCover", "Rain", "SnowMelt"]}
    out["chan_q_avg"] = hp.chan_q_avg()
    return out


_singles = {}


def singles(scenario, x, mode, structures):
    """per step, per member: snapshot of that member's own HotPathDevice(meteo=...)"""
    from lisflood_amd.hotpath import HotPathDevice
    key = (mode, structures)
    if key not in _singles:
        out = [[None] * M for _ in range(STEPS)]
        for m in range(M):
            hp = build(scenario, HotPathDevice, structures, meteo=meteo_of(x, m))
            for s in range(STEPS):
                prec, tavg = member_meteo(x, mode, m, s)
                hp.step(dict(land_forcing(s), Precipitation=prec, Tavg=tavg), time_since_start=s + 1, season=x["seasons"][s],
                        QInM3=inflow(scenario, m, s) if structures else None)
                out[s][m] = snapshot(hp)
            hp.free()
        _singles[key] = out
    return _singles[key]


def assert_members(ens, want, s):
    for k in want[0]:
        got = ens.chan_q_avg() if k == "chan_q_avg" else ens.download(k)
        for m in range(M):
            ok = np.array_equal(got[m], want[m][k]) if got.dtype == np.uint8 else same_bits(got[m], want[m][k])
            assert ok, (s, k, m, first_difference(got[m].astype(np.float64), want[m][k].astype(np.float64)))


def run_ensemble(scenario, x, mode, structures, check):
    from lisflood_amd.hotpath import HotPathEnsemble
    ens = build(scenario, HotPathEnsemble, structures, members=M, pad=PAD, meteo=meteo_of(x))
    ens.set_gaps(S.SENTINEL)
    if mode == "perturbed":
        ens.forcing_perturbation("Tavg", patterns(), multiplicative=False, lower=-np.inf)
        ens.forcing_perturbation("Precipitation", patterns())
    for s in range(STEPS):
        if mode == "rows":
            f = dict(land_forcing(s), Precipitation=x["Precipitation"][s], Tavg=x["Tavg"][s])
        else:
            f = dict(land_forcing(s), Precipitation=x["Precipitation"][s][0], Tavg=x["Tavg"][s][0])
        c = {"Tavg": coefficients(s), "Precipitation": coefficients(s)} if mode == "perturbed" else None
        q = np.stack([inflow(scenario, m, s) for m in range(M)]) if structures else None
        ens.step(f, time_since_start=s + 1, coefficients=c, QInM3=q, season=x["seasons"][s])
        check(ens, s)
    return ens


def assert_gaps(ens):
    from lisflood_amd.soilloop import GAP_BYTE
    for k in ens.gap_names():
        g = ens.gaps(k)
        assert g.shape == (ens.members, PAD), (k, g.shape)
        if g.dtype == np.uint8:
            assert (g == GAP_BYTE).all(), k
        else:
            ok = (g == S.SENTINEL) | np.isnan(g)
            assert ok.all() and not np.isnan(g[:-1]).any(), (k, g)


@pytest.mark.parametrize("mode,structures", [("one_row", False), ("rows", False), ("perturbed", False), ("rows", True)])
def test_every_member_is_its_own_hot_path_with_meteo(amd, scenario, family, mode, structures):
    want = singles(scenario, family, mode, structures)

    def check(ens, s):
        assert_members(ens, want[s], s)
        assert_gaps(ens)
        assert ens.land.forcing_member_stride() == ens.pstride      # Rain, SnowMelt and isFrozenSoil are member rows
    ens = run_ensemble(scenario, family, mode, structures, check)
    assert {"SnowCoverS", "FrostIndex"} <= set(ens.state_names()) and {"SnowCoverS", "FrostIndex"} <= set(ens.analysis_names())
    ens.free()


def test_perturbed_temperature_makes_the_members_differ(amd, scenario, family):
    """The members start from ONE state and get ONE row of meteo: only the perturbation of Tavg on the device tells them
    apart -- in frozen soil and snow pack, which no forcing perturbation could reach before, and from there in discharge,
    each member as its own single run says."""
    from lisflood_amd.hotpath import HotPathEnsemble
    x = dict(family, SnowCoverS=family["SnowCoverS"][0], FrostIndex=family["FrostIndex"][0])
    ens = build(scenario, HotPathEnsemble, False, members=M, pad=PAD, meteo=meteo_of(x))
    ens.forcing_perturbation("Tavg", patterns() * 8.0, multiplicative=False, lower=-np.inf)
    x3 = dict(family, SnowCoverS=np.stack([x["SnowCoverS"]] * M), FrostIndex=np.stack([x["FrostIndex"]] * M))
    from lisflood_amd.hotpath import HotPathDevice
    alone = [build(scenario, HotPathDevice, False, meteo=meteo_of(x3, m)) for m in range(M)]
    for s in range(STEPS):
        f = dict(land_forcing(s), Precipitation=family["Precipitation"][s][0], Tavg=family["Tavg"][s][0])
        c = coefficients(s)
        ens.step(f, time_since_start=s + 1, coefficients={"Tavg": c}, season=family["seasons"][s])
        rows = MP.perturb(None, c, patterns() * 8.0, family["Tavg"][s][0], False, -np.inf, np.inf)
        for m in range(M):
            alone[m].step(dict(f, Tavg=rows[m]), time_since_start=s + 1, season=family["seasons"][s])
    frozen, packs, dis = ens.download("isFrozenSoil"), ens.download("SnowCoverS"), ens.chan_q_avg()
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(frozen[a], frozen[b]) and not same_bits(packs[a], packs[b]) and not same_bits(dis[a], dis[b])
    for m in range(M):
        assert np.array_equal(frozen[m], alone[m].download("isFrozenSoil"))
        assert same_bits(packs[m], alone[m].download("SnowCoverS")) and same_bits(dis[m], alone[m].chan_q_avg()), m
        alone[m].free()
    ens.free()


def test_meteo_on_the_device_is_the_restatement_on_the_host(amd, scenario):
    """the exact family: HotPathDevice(meteo=...) against a plain HotPathDevice whose Rain, SnowMelt and isFrozenSoil the numpy
    restatement makes, every state vector and dis bit for bit after each of four steps; step(None) repeats the meteo"""
    from lisflood_amd.hotpath import HotPathDevice
    from lisflood_amd._lib import u8
    x = S.exact_inputs(N, 1)
    ref = S.run(x)
    hp = build(scenario, HotPathDevice, False, meteo=meteo_of(x, 0, Snow=True))
    plain = build(scenario, HotPathDevice, False)
    assert "SnowCoverS" not in plain.state_names() and hp.state_names() == plain.state_names() + ["SnowCoverS", "FrostIndex"]
    for s in range(STEPS):
        land = land_forcing(s)
        hp.step(dict(land, Precipitation=x["Precipitation"][s][0], Tavg=x["Tavg"][s][0]), time_since_start=s + 1,
                season=x["seasons"][s])
        amd.synchronize(0)
        plain.d["isFrozenSoil"].upload(u8(plain._ordered(ref[s]["isFrozenSoil"][0])))
        plain.step(dict(land, Rain=ref[s]["Rain"][0], SnowMelt=ref[s]["SnowMelt"][0]), time_since_start=s + 1)
        for k in ("Rain", "SnowMelt", "Snow", "SnowCover", "SnowCoverS", "FrostIndex"):
            assert same_bits(hp.download(k), ref[s][k][0]), (s, k)
        assert np.array_equal(hp.download("isFrozenSoil"), ref[s]["isFrozenSoil"][0].astype(np.uint8)), s
        for k in plain.state_names():
            assert same_bits(hp.download(k), plain.download(k)), (s, k, first_difference(hp.download(k), plain.download(k)))
        assert same_bits(hp.chan_q_avg(), plain.chan_q_avg()), s
    assert ref[-1]["isFrozenSoil"].any() and not ref[-1]["isFrozenSoil"].all() and (ref[-1]["Rain"] > 0).any()
    # step(None): the meteo its buffer set holds (the step before the last) once more, the frost index advances all the same
    again = S.step(x, ref[-1]["SnowCoverS"], ref[-1]["FrostIndex"], x["Precipitation"][STEPS - 2], x["Tavg"][STEPS - 2], (0.1, 0.2))
    hp.step(None, time_since_start=STEPS + 1, season=(0.1, 0.2))
    assert same_bits(hp.download("FrostIndex"), again["FrostIndex"][0]) and same_bits(hp.download("Rain"), again["Rain"][0])
    with pytest.raises(ValueError, match="season="):
        hp.step(None)
    with pytest.raises(ValueError, match="Rain in the forcing"):
        hp.step(dict(land_forcing(0), Precipitation=np.zeros(N), Tavg=np.zeros(N), Rain=np.zeros(N)), season=(0.0, 0.0))
    with pytest.raises(ValueError, match="season= without meteo="):
        plain.step(None, season=(0.0, 0.0))
    r = hp.rasters(["SnowCover", "Snow"]).wait()
    assert r["SnowCover"].shape == (H, W)
    hp.free(); plain.free()


def test_analysis_trackers_and_state_files_see_the_snow(amd, scenario, family, tmp_path):
    from lisflood_amd.hotpath import HotPathDevice, HotPathEnsemble
    x = family
    ens = build(scenario, HotPathEnsemble, False, members=M, pad=PAD, meteo=meteo_of(x))
    ens.set_gaps(S.SENTINEL)
    ens.track_begin("SnowCover")
    covers = []
    for s in range(2):
        ens.step(dict(land_forcing(s), Precipitation=x["Precipitation"][s], Tavg=x["Tavg"][s]), time_since_start=s + 1,
                 season=x["seasons"][s])
        covers.append(ens.download("SnowCover"))
    peak, step_of = covers[0].copy(), np.zeros(covers[0].shape, np.int32)
    later = covers[1] > peak
    peak[later], step_of[later] = covers[1][later], 1
    assert same_bits(ens.download("SnowCover.peak"), peak) and np.array_equal(ens.download("SnowCover.peak_step"), step_of)
    got = ens.summary("SnowCover", minimum=False, maximum=False)["mean"]
    assert same_bits(got, ((covers[1][0] + covers[1][1]) + covers[1][2]) / 3.0)
    ens.track_end("SnowCover")
    names = ("SnowCoverS", "FrostIndex")
    before = {k: ens.download(k) for k in names}
    assert not same_bits(before["SnowCoverS"][0], before["SnowCoverS"][1])             # snow differs between the members
    ens.transform(np.eye(M))
    for k in names:
        assert same_bits(ens.download(k), before[k]), k
    perm = np.array([2, 0, 1])
    weights = np.zeros((M, M))
    weights[perm, np.arange(M)] = 1.0
    ens.transform(weights)
    for k in names:
        assert same_bits(ens.download(k), before[k][perm]), k
    now = {k: ens.download(k) for k in names}
    ens.resample(np.array([1, 1, 0]))
    for k in names:
        assert same_bits(ens.download(k), now[k][[1, 1, 0]]), k
    assert same_bits(ens.download("LZ")[0], ens.download("LZ")[1])                   # (the particle: every state vector)
    # state files: the two vectors round-trip; a file written without meteo= is refused by an object with it, and loads
    # into an object without it as before
    path = str(tmp_path / "state.npz")
    ens.save_state(path)
    saved = {k: ens.download(k) for k in names}
    ens.set_member_state("FrostIndex", np.zeros((M, N)))
    ens.set_member_state("SnowCoverS", np.ones((M, 3, N)))
    ens.load_state(path)
    for k in names:
        assert same_bits(ens.download(k), saved[k]), k
    for k in ens.gap_names():
        g = ens.gaps(k)
        assert ((g == S.SENTINEL) | np.isnan(g)).all() if g.dtype != np.uint8 else True, k
    plain = build(scenario, HotPathEnsemble, False, members=M)
    old = str(tmp_path / "old.npz")
    plain.save_state(old)
    assert "SnowCoverS" not in np.load(old).files
    plain.load_state(old)
    with pytest.raises(ValueError, match="without SnowCoverS and FrostIndex"):
        ens.load_state(old)
    plain.free(); ens.free()
    one = build(scenario, HotPathDevice, False, meteo=meteo_of(x, 0))
    one.step(dict(land_forcing(0), Precipitation=x["Precipitation"][0][0], Tavg=x["Tavg"][0][0]), season=x["seasons"][0])
    one.save_state(path)
    kept = {k: one.download(k) for k in names}
    one.step(dict(land_forcing(1), Precipitation=x["Precipitation"][1][0], Tavg=x["Tavg"][1][0]), season=x["seasons"][1])
    assert not same_bits(one.download("FrostIndex"), kept["FrostIndex"])
    one.load_state(path)
    for k in names:
        assert same_bits(one.download(k), kept[k]), k
    one.free()


def test_without_meteo_nothing_has_a_new_name(amd, scenario):
    """state_names() and the device vectors of objects without meteo=, against lists written down from the commit before the
    feature"""
    from lisflood_amd.hotpath import FORCING, HotPathDevice, HotPathEnsemble
    from parent_names import DEVICE_VECTORS, ENSEMBLE_LAND_VECTORS, STATE_NAMES
    hp = build(scenario, HotPathDevice, False)
    assert hp.state_names() == STATE_NAMES and sorted(hp.d) == DEVICE_VECTORS
    assert hp.forcing_names == FORCING and hp.meteo is None and not hasattr(hp, "snow_frost")
    assert "snow_frost" not in hp.stage_bytes()
    hp.free()
    ens = build(scenario, HotPathEnsemble, False, members=2)
    assert ens.state_names() == STATE_NAMES and ens.analysis_names() == STATE_NAMES
    assert sorted(ens.land.dev) == ENSEMBLE_LAND_VECTORS and sorted(ens.force[1]) == sorted(FORCING)
    assert ens.land.forcing_member_stride() == 0 and not hasattr(ens, "snow_frost")
    ens.free()
