"""lf_snow_frost_members_device on the device against the numpy restatement of tests/snow_frost.py: every pixel count around a
wavefront and a workgroup, member counts on both sides of the slice of 8, padded strides with sentinels in every gap, one
forcing row for all and rows per member, the Snow row present and NULL, both halves and either one, four consecutive updates.
Everything but FrostIndex and isFrozenSoil bit for bit; FrostIndex bit for bit where there is no snow cover (exp is exactly
1) and within the bound derived in snow_frost.frost_bound from 1 ulp of exp elsewhere (OCML's documented accuracy of the fp64
exp, not anything measured here); isFrozenSoil wherever the reference is further than the bound from the threshold, and the
inputs are such that no element is nearer (tests/test_snow_frost_cpu.py asserts it).  Then the module classes and the resident
classes of lisflood_amd.snow_frost."""
import types

import numpy as np
import pytest

import snow_frost as S

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 1031)
MEMBERS = (1, 2, 3, 8, 9, 17)           # 9 and 17: a full slice of 8 and one member more; 3: a partial slice
CASES = [(n, m) for n in SIZES for m in MEMBERS]


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def variant(case, h):
    """(pad, forcing rows per member, Snow row) of half h of case number `case`: 3 * case + h runs through all eight
    combinations for every half as the cases go by"""
    combo = (3 * case + h) % 8
    return 5 * (combo & 1), bool(combo & 2), bool(combo & 4)


def test_the_variants_cover_every_combination():
    for h in range(3):
        assert {variant(c, h) for c in range(len(CASES))} == {(p, f, s) for p in (0, 5) for f in (False, True) for s in (False, True)}


@pytest.mark.parametrize("N,members", CASES)
def test_kernel_against_the_restatement(amd, N, members):
    from lisflood_amd import snow_frost as SF
    x = S.inputs(N, members)
    case = CASES.index((N, members))
    for h, halves in enumerate(S.HALVES):
        pad, per_member, snow_row = variant(case, h)
        lay = S.Layout(N, members, pad, per_member, snow_row, halves)
        worst = S.check_steps(x, lay, lambda par, season: lay.device(par, season, amd, SF))
        print("N = %d, %d members, %s, pad %d, forcing rows %s, Snow %s: largest |FrostIndex - reference| %.3g"
              % (N, members, halves, pad, per_member, snow_row, worst))


@pytest.mark.parametrize("N,members", [(257, 3), (1031, 9)])
def test_exact_family_bit_for_bit(amd, N, members):
    """all packs empty and no snow: exp is exactly 1, FrostIndex and isFrozenSoil bit for bit too, the planted threshold
    ties among them (FrostIndex == threshold: not frozen; one ulp above: frozen)"""
    from lisflood_amd import snow_frost as SF
    x = S.exact_inputs(N, members)
    for halves in ("both", "frost"):
        lay = S.Layout(N, members, 5, True, True, halves)
        assert S.check_steps(x, lay, lambda par, season: lay.device(par, season, amd, SF)) == 0.0
    lay = S.Layout(N, members, 0, True, False, "both")
    lay.put("SnowCoverS", x["SnowCoverS"]); lay.put("FrostIndex", x["FrostIndex"])
    lay.put("Precipitation", x["Precipitation"][0]); lay.put("Tavg", x["Tavg"][0])
    lay.device(x, x["seasons"][0], amd, SF)
    at, above = S.spots(0, N), S.spots(1, N)
    assert (lay.get("FrostIndex")[:, at] == 56.0).all() and not lay.h["isFrozenSoil"][:, at].any()
    assert (lay.get("FrostIndex")[:, above] == np.nextafter(56.0, np.inf)).all() and lay.h["isFrozenSoil"][:, above].all()


def test_module_classes_on_a_var_namespace(amd):
    """snow.dynamic() then frost.dynamic(), four steps on `var`: the restatement's values (FrostIndex within the bound)"""
    from lisflood_amd import snow_frost as SF
    N = 257
    x = S.inputs(N, 1)
    v = types.SimpleNamespace(**{k: x[k] for k in S.STATICS}, **S.SCALARS)
    v.SnowCoverS, v.FrostIndex = x["SnowCoverS"][0].copy(), x["FrostIndex"][0].copy()
    v.Tavg = x["Tavg"][0][0]
    snow, frost = SF.snow(v), SF.frost(v)
    snow.initial(); frost.initial()
    for s in range(4):
        v.Precipitation, v.Tavg = x["Precipitation"][s][0], x["Tavg"][s][0]
        v.SnowSeasonTerm, v.SummerSeason = x["seasons"][s]
        zones, fi = v.SnowCoverS.copy(), v.FrostIndex.copy()
        snow.dynamic()
        want = S.snow_step(x, zones, v.Precipitation, v.Tavg, x["seasons"][s])
        for k in ("SnowCoverS",) + S.OUTPUTS:
            assert S.same_bits(getattr(v, k), want[k]), (s, k, S.first_difference(getattr(v, k), want[k]))
        frost.dynamic()
        trace = {}
        ref = S.frost_step(x, fi, want["SnowCover"], v.Tavg, S.exp_rounded, trace)
        bound = S.frost_bound(x, fi, trace, 1.0)
        with np.errstate(invalid="ignore"):
            ok = np.isnan(ref["FrostIndex"]) | (np.abs(v.FrostIndex - ref["FrostIndex"]) <= bound)
        assert ok.all() and np.array_equal(np.isnan(v.FrostIndex), np.isnan(ref["FrostIndex"])), s
        assert v.isFrozenSoil.dtype == bool and np.array_equal(v.isFrozenSoil, ref["isFrozenSoil"]), s


@pytest.mark.parametrize("members,pad,per_member", [(1, 0, True), (3, 5, False), (9, 5, True)])
def test_resident_classes(amd, members, pad, per_member):
    """SnowFrostEnsemble (members = 1: SnowFrostDevice): rows laid out by soilloop._EnsembleVectors' code, nothing written
    between them, the same values as the bare call"""
    from lisflood_amd import snow_frost as SF
    from lisflood_amd.soilloop import GAP_BYTE
    N = 65
    x = S.inputs(N, members)
    meteo = dict({k: x[k] for k in S.STATICS}, **S.SCALARS, SnowCoverS=x["SnowCoverS"], FrostIndex=x["FrostIndex"], Snow=True)
    if members == 1:
        meteo["SnowCoverS"], meteo["FrostIndex"] = x["SnowCoverS"][0], x["FrostIndex"][0]
        e = SF.SnowFrostDevice(meteo)
    else:
        e = SF.SnowFrostEnsemble(meteo, members, pad=pad)
    e.set_gaps(S.SENTINEL)
    lay = S.Layout(N, members, pad, per_member, True, "both")
    lay.put("SnowCoverS", x["SnowCoverS"]); lay.put("FrostIndex", x["FrostIndex"])
    for s in range(4):
        P, T = lay.forcing(x, s)
        lay.put("Precipitation", P); lay.put("Tavg", T)
        lay.device(x, x["seasons"][s], amd, SF)
        one = members == 1 or not per_member
        e.step(dict(Precipitation=P[0] if one else P, Tavg=T[0] if one else T), x["seasons"][s])
        assert e.forcing_member_stride() == (0 if one else N + pad)
        for k in ("SnowCoverS", "FrostIndex", "isFrozenSoil", "SnowCover", "Snow", "Rain", "SnowMelt"):
            got, want = e.get(k), lay.get(k) if k != "isFrozenSoil" else lay.h[k][:, :N]
            got = got[None] if members == 1 else got
            assert (np.array_equal(got, want) if got.dtype == np.uint8 else S.same_bits(got, want)), (s, k)
        if members > 1:
            for k in e._member + e._forcing + e._pixel:
                g = e.gaps(k)
                assert g.shape == (members, pad) and (g == (GAP_BYTE if g.dtype == np.uint8 else S.SENTINEL)).all(), (s, k)
    with pytest.raises(ValueError, match="no forcing of this call"):
        e.step(dict(Rain=np.zeros(N)))
    e.free()
