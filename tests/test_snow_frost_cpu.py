"""Snow and frost without a device: the input families take every branch (census), the numpy restatement of
tests/snow_frost.py is the stated arithmetic -- against a per-element Python loop and against mpmath at 240 bits rounded after
every operation --, no FrostIndex of the families lies within its error bound of the threshold, season_terms, the C ABI's
exports and refusals, and the argument checks of meteo=."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import snow_frost as S
from conftest import ROOT

from lisflood_amd import _lib
from lisflood_amd import snow_frost as SF

N = 257
FAMILIES = {"general": lambda: S.inputs(N, 2), "exact": lambda: S.exact_inputs(N, 2)}


@pytest.fixture(scope="module")
def family():
    made = {}

    def get(name):
        if name not in made:
            x, traces = FAMILIES[name](), []
            made[name] = (x, S.run(x, traces=traces), traces)
        return made[name]
    return get


def test_census_every_branch_and_tie_is_taken(family):
    x, _, traces = family("general")
    c = S.census(x, traces)
    print(S.counts_table("general family, N = %d, 2 members, 4 steps" % N, c))
    empty = [k for k, v in c.items() if v == 0]
    assert not empty, empty
    x, _, traces = family("exact")
    c = S.census(x, traces)
    print(S.counts_table("exact family", c))
    total = 4 * 2 * N
    assert c["without snow cover"] == total and c["empty zone"] == 3 * total
    for k in ("FrostIndex == threshold, no cover (not frozen)", "FrostIndex one ulp above threshold, no cover (frozen)",
              "FrostIndex clamped at 0", "frozen", "not frozen", "Tavg < 0", "Tavg > 0", "zero precipitation"):
        assert c[k] > 0, k


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_restatement_is_the_per_element_loop(family, name):
    """every value bit for bit, FrostIndex too: both sides take exp from mpmath, correctly rounded"""
    x = FAMILIES[name]()
    ref = S.run(x, exp=S.exp_rounded, steps=2)
    zones, frost = x["SnowCoverS"], x["FrostIndex"]
    for s in range(2):
        for m in (0, 1):
            got = S.elements_step(S.FloatOps, x, zones, frost, s, m)
            for k, a in got.items():
                want = ref[s][k][m]
                assert (np.array_equal(a, want) if a.dtype == bool else S.same_bits(a, want)), \
                    (name, s, m, k, S.first_difference(a, want))
        zones, frost = ref[s]["SnowCoverS"], ref[s]["FrostIndex"]


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_restatement_against_mpmath_operation_by_operation(family, name):
    """Every operation of the restatement is the correctly rounded one: mpmath at 240 bits, rounded to a double after each.
    Every value but FrostIndex bit for bit; FrostIndex (numpy's own exp, taken as within 0.5 ulp) within the bound."""
    x, ref, _ = family(name)
    zones, frost = x["SnowCoverS"], x["FrostIndex"]
    worst = 0.0
    for s in range(len(ref)):
        trace = {}
        exact = S.step(x, zones, frost, x["Precipitation"][s], x["Tavg"][s], x["seasons"][s], S.exp_rounded, trace)
        bound = S.frost_bound(x, frost, trace, 0.5)
        got = S.elements_step(S.MpOps, x, zones, frost, s, 0)
        for k in ("SnowCoverS",) + S.OUTPUTS:
            assert S.same_bits(got[k], ref[s][k][0]), (name, s, k, S.first_difference(got[k], ref[s][k][0]))
        assert S.same_bits(got["FrostIndex"], exact["FrostIndex"][0]), (name, s)
        with np.errstate(invalid="ignore"):
            diff = np.abs(ref[s]["FrostIndex"] - exact["FrostIndex"])
        assert np.array_equal(np.isnan(diff), np.isnan(exact["FrostIndex"]))
        ok = np.isnan(diff) | (diff <= bound)
        worst = max(worst, float(np.nanmax(diff)))
        assert ok.all(), (name, s, float(np.nanmax(diff - bound)))
        zones, frost = ref[s]["SnowCoverS"], ref[s]["FrostIndex"]
    print("largest |FrostIndex(np.exp) - FrostIndex(exp correctly rounded)|: %.3g" % worst)


GPU_FAMILIES = ([(S.inputs, n, m) for n in (1, 63, 64, 65, 257, 1031) for m in (1, 2, 3, 8, 9, 17)] +
                [(S.exact_inputs, 257, 3), (S.exact_inputs, 1031, 9), (S.exact_inputs, 2880, 1),
                 (lambda n, m: S.inputs(n, m, nan=False), 2880, 3), (lambda n, m: S.inputs(n, m, seed=3), 1000, 1)])


@pytest.mark.parametrize("make", [lambda f=f, n=n, m=m: f(n, m) for f, n, m in GPU_FAMILIES],
                         ids=["%s-%d-%d" % (getattr(f, "__name__", "inputs"), n, m) for f, n, m in GPU_FAMILIES])
def test_no_frost_index_within_its_bound_of_the_threshold(make):
    """the condition of the isFrozenSoil comparison on the device: E = 1 ulp of exp, every family the GPU tests use"""
    x = make()
    per_step = S.inside_threshold(x, E=1.0)
    bounds = [float(np.nanmax(b)) for _, b, _ in per_step]
    print("largest bound per step:", bounds)
    assert [int(i.sum()) for _, _, i in per_step] == [0] * len(per_step)
    assert max(bounds) < 1e-12


def test_season_terms():
    import mpmath
    with mpmath.workprec(240):
        for day in (1, 81, 165, 166, 259, 260, 366):
            term = float(mpmath.sin(mpmath.pi * (day - 81) * 360 / mpmath.mpf("365.25") / 180))
            assert abs(SF.season_terms(day, 1.0)[0] - term) < 4e-16, day
    assert SF.season_terms(81, 3.7)[0] == 0.0
    for day in (1, 81, 165, 166, 259, 260, 366):
        term, summer = SF.season_terms(day, 2.5)
        assert term == 2.5 * math.sin(math.radians((day - 81) * 360 / 365.25))
        want = math.sin(math.radians((day - 165) * 180 / (259 - 165))) if 165 < day < 260 else 0.0
        assert summer == want
    assert SF.season_terms(165, 1.0)[1] == 0.0 and SF.season_terms(260, 1.0)[1] == 0.0
    assert 0.0 < SF.season_terms(166, 1.0)[1] < 0.04 and abs(SF.season_terms(166, 1.0)[1] - math.sin(math.pi / 94)) < 1e-15
    assert 0.0 < SF.season_terms(259, 1.0)[1] < 1e-15           # sin of the double next to pi
    assert SF.season_terms(212, 1.0)[1] == 1.0                  # the middle of the ice season


def test_abi_exports_and_struct_mirror():
    L = _lib.lib()
    f = L.lf_snow_frost_members_device
    assert list(f.argtypes) == [_lib._KIND[k] for k in "ipiqqq"] and f.restype is C.c_int
    text = open(os.path.join(ROOT, "include", "lisflood_amd.h")).read()
    body = re.search(r"typedef struct lf_snow_frost_args \{(.*?)\} lf_snow_frost_args;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *\n") for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?(double|uint8_t|int64_t)", "", decl.strip()).split(",")]
    assert names == [k for k, _ in SF._SnowFrostArgs._fields_]
    assert C.sizeof(SF._SnowFrostArgs) == 8 * len(names) == 176


# ---- refusals: nothing here touches a device ---------------------------------------------------------------------------
def block(n=8, snow=True, frost=True, snow_row=True):
    """an argument block of distinct fake addresses, 1 MiB apart (they are compared, never read)"""
    a = SF._SnowFrostArgs()
    base = 1 << 30
    for i, k in enumerate(SF._POINTERS):
        setattr(a, k, base + (i << 20))
    for k in S.SCALARS:
        setattr(a, k, S.SCALARS[k])
    a.N = n
    if not snow:
        for k in ("SnowCoverS", "Precipitation", "Rain", "SnowMelt", "Snow"):
            setattr(a, k, None)
    if not frost:
        a.FrostIndex = a.isFrozenSoil = None
    if not snow_row:
        a.Snow = None
    return a


def call(a, members=2, zone_stride=None, row_stride=None, forcing_stride=0):
    n = a.N
    return _lib.lib().lf_snow_frost_members_device(0, C.byref(a), members, 3 * n if zone_stride is None else zone_stride,
                                                   n if row_stride is None else row_stride, forcing_stride)


def refused(rc, word):
    assert rc == _lib.LF_E_INVALID, rc
    msg = _lib.lib().lf_last_error().decode()
    assert word in msg, msg


def test_refusals_before_any_device_is_touched():
    L = _lib.lib()
    assert L.lf_snow_frost_members_device(0, None, 1, 0, 0, 0) == _lib.LF_E_INVALID
    a = block()
    a.N = -1
    refused(call(a, zone_stride=24, row_stride=8), "N = -1")
    refused(call(block(), members=0), "members")
    refused(call(block(), zone_stride=23), "zone_stride")
    refused(call(block(), row_stride=7), "row_stride")
    refused(call(block(), forcing_stride=7), "forcing_stride")
    refused(call(block(), forcing_stride=-8), "forcing_stride")
    # NULL combinations: everything but the two halves and the optional Snow row
    a = block()
    a.Tavg = None
    refused(call(a), "Tavg")
    for k in ("Precipitation", "Rain", "SnowMelt", "DeltaTSnow", "SnowMeltCoef", "SnowFactor"):
        a = block()
        setattr(a, k, None)
        refused(call(a), "snow half")
    a = block()
    a.SnowCover = None
    refused(call(a), "SnowCover")
    a = block()
    a.isFrozenSoil = None
    refused(call(a), "isFrozenSoil")
    a = block()
    a.FrostIndex = None                       # snow only, but isFrozenSoil given
    refused(call(a), "isFrozenSoil")
    a = block(snow=False, frost=False)
    refused(call(a), "both NULL")
    for k in ("Precipitation", "Rain", "SnowMelt", "Snow"):      # frost only, with something of the snow half
        a = block(snow=False)
        setattr(a, k, 1 << 29)
        refused(call(a), "frost only")
    # aliases: an output on an input or on another output, also through the members' rows
    a = block()
    a.Rain = a.SnowMelt
    refused(call(a), "overlap")
    a = block()
    a.SnowCover = a.Tavg
    refused(call(a), "overlap")
    a = block()
    a.FrostIndex = a.SnowCoverS + 8 * 8       # inside zone 1 of member 0
    refused(call(a), "overlap")
    a = block()
    a.SnowMelt = a.Rain + 8 * 8               # member 1's Rain row is member 0's SnowMelt row
    refused(call(a, row_stride=8), "overlap")
    a = block()
    a.isFrozenSoil = a.Rain + 8 * 8 + 7       # the last byte of member 1's Rain row
    refused(call(a, row_stride=8), "overlap")
    a = block(snow=False)
    a.SnowCover = a.FrostIndex                # frost only: SnowCover is an input, FrostIndex is written
    refused(call(a), "overlap")


def test_empty_domain_succeeds_and_the_halves_are_accepted_without_a_launch():
    for kw in (dict(), dict(frost=False), dict(snow=False), dict(snow_row=False)):
        a = block(n=0, **kw)
        assert call(a, members=3) == _lib.LF_OK, (kw, _lib.lib().lf_last_error())


# ---- meteo= ----------------------------------------------------------------------------------------------------------------
def good_meteo(n, members=None):
    x = S.inputs(n, members or 1)
    m = {k: x[k] for k in S.STATICS}
    m.update(S.SCALARS)
    m["SnowCoverS"], m["FrostIndex"] = (x["SnowCoverS"], x["FrostIndex"]) if members else (x["SnowCoverS"][0], x["FrostIndex"][0])
    return m


def test_check_meteo():
    n = 12
    m = SF.check_meteo(good_meteo(n), n)
    assert m["Snow"] is False and m["SnowCoverS"].shape == (3, n) and isinstance(m["DtDay"], float)
    assert SF.check_meteo(dict(good_meteo(n), Snow=True), n)["Snow"] is True
    assert SF.check_meteo(good_meteo(n, 4), n, 4)["SnowCoverS"].shape == (4, 3, n)
    with pytest.raises(ValueError, match="must be a dict"):
        SF.check_meteo([1, 2], n)
    for k in SF.STATICS + SF.SCALARS + SF.STATE:
        bad = good_meteo(n)
        del bad[k]
        with pytest.raises(ValueError, match="lacks %s" % k):
            SF.check_meteo(bad, n)
    with pytest.raises(ValueError, match="unknown entries: Rain"):
        SF.check_meteo(dict(good_meteo(n), Rain=np.zeros(n)), n)
    with pytest.raises(ValueError, match=r"DeltaTSnow\] must be \[12\]"):
        SF.check_meteo(dict(good_meteo(n), DeltaTSnow=np.zeros(n + 1)), n)
    with pytest.raises(ValueError, match="must be a scalar"):
        SF.check_meteo(dict(good_meteo(n), TempSnow=np.zeros(n)), n)
    with pytest.raises(ValueError, match="SnowCoverS"):
        SF.check_meteo(good_meteo(n, 4), n)                      # member rows for a single run
    with pytest.raises(ValueError, match="SnowCoverS"):
        SF.check_meteo(good_meteo(n, 4), n, 5)
    with pytest.raises(ValueError, match="FrostIndex"):
        SF.check_meteo(dict(good_meteo(n), FrostIndex=np.zeros((3, n))), n)


@pytest.mark.parametrize("ensemble", [False, True])
def test_hotpath_refuses_a_bad_meteo_before_it_builds_anything(ensemble):
    from lisflood_amd import hotpath
    mask = np.ones((3, 4), bool)
    bad = good_meteo(12)
    del bad["Afrost"]
    args = ({}, {}, mask, None, None) + ((3,) if ensemble else ())
    with pytest.raises(ValueError, match="lacks Afrost"):
        (hotpath.HotPathEnsemble if ensemble else hotpath.HotPathDevice)(*args, meteo=bad)
    with pytest.raises(ValueError, match="DeltaTSnow"):
        (hotpath.HotPathEnsemble if ensemble else hotpath.HotPathDevice)(*args, meteo=good_meteo(11))


def test_forcing_names_and_state_with_and_without_meteo():
    from lisflood_amd import hotpath
    assert hotpath.FORCING == ("Rain", "SnowMelt", "EWRef", "ETRef", "ESRef")
    assert hotpath.METEO_FORCING == ("Precipitation", "Tavg", "EWRef", "ETRef", "ESRef")
    assert hotpath._HotPath.STATE[-2:] == ("SnowCoverS", "FrostIndex")
    h = hotpath._HotPath()
    h._begin({}, np.ones((2, 3), bool), True, 0, True, None)
    assert h.meteo is None and h.forcing_names == hotpath.FORCING
    h._check_forcing({})                                          # (not this object's business without meteo=)
    with pytest.raises(ValueError, match="season= without meteo="):
        h._season((0.0, 0.0))
    h._begin({}, np.ones((2, 3), bool), True, 0, True, None, good_meteo(6))
    h.snow_frost = SF._SnowFrostArgs()
    assert h.forcing_names == hotpath.METEO_FORCING
    with pytest.raises(ValueError, match="season="):
        h._season(None)
    h._season((0.25, 0.5))
    assert (h.snow_frost.SnowSeasonTerm, h.snow_frost.SummerSeason) == (0.25, 0.5)
    ok = {k: np.zeros(6) for k in hotpath.METEO_FORCING}
    h._check_forcing(ok)
    with pytest.raises(ValueError, match="Rain and SnowMelt in the forcing"):
        h._check_forcing(dict(ok, Rain=np.zeros(6), SnowMelt=np.zeros(6)))
    with pytest.raises(ValueError, match="forcing lacks Tavg"):
        h._check_forcing({k: v for k, v in ok.items() if k != "Tavg"})
    with pytest.raises(ValueError, match="without SnowCoverS and FrostIndex"):
        h._check_state_file(["ChanQ", "LZ"])
    h._check_state_file(["ChanQ", "SnowCoverS", "FrostIndex"])


@pytest.mark.parametrize("halves", S.HALVES)
def test_the_device_harness_accepts_the_restatement_and_sees_a_wrong_value(halves):
    """tests/test_snow_frost_gpu.py's comparison (snow_frost.check_steps over a Layout with sentinels), rehearsed without a
    device: the restatement with numpy's exp in the kernel's place passes, a value off by one ulp or a touched gap does not"""
    x = S.inputs(65, 3)
    lay = S.Layout(65, 3, 5, True, True, halves)
    S.check_steps(x, lay, lambda par, season: lay.fake(par, season))

    def off_by_an_ulp(par, season):
        lay.fake(par, season)
        lay.h["SnowMelt"][1, 7] = np.nextafter(lay.h["SnowMelt"][1, 7], np.inf)
    lay = S.Layout(65, 3, 5, True, True, halves)
    if halves != "frost":                  # (a frost index one ulp off is inside its bound: that is what the bound is for)
        with pytest.raises(AssertionError, match="SnowMelt"):
            S.check_steps(x, lay, off_by_an_ulp)

    def touches_a_gap(par, season):
        lay.fake(par, season)
        lay.h["SnowCover"][0, 65 + 2] = 0.0
    lay = S.Layout(65, 3, 5, True, True, halves)
    with pytest.raises(AssertionError, match="SnowCover"):
        S.check_steps(x, lay, touches_a_gap)
